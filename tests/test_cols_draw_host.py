"""CPU tests of section 2f of include/qwen3_hip.h (q3_batch_step_cols_draw / q3_generate_many_sampled): the two names are declared,
listed and exported, and the requests the GPU test runs can tell right from wrong -- on the C oracle with oracle.Sampler, the row of
every sampled request under the chat rule differs from the row with the other seed, from the row drawn without the prompt's
discarded coins and from the greedy row.  A condition on the inputs, not a measurement of the product."""
import os
import re
import subprocess

import pytest

from cols_draw_cases import CKPT_SEED, N_NEW, PROMPT_LEN, SAMPLERS, SEEDS, prompts, sampler_id
from conftest import ROOT

NEW = {"q3_batch_step_cols_draw", "q3_generate_many_sampled"}
NAME = "tiny-g64"


def test_header_symbol_list_and_binary_agree_on_the_new_names(q3):
    hdr = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    declared = set(re.findall(r"\b(q3_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(q3.EXPORTED_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", q3.lib_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert NEW <= exported
    lib = q3.load_library()
    assert len(lib.q3_batch_step_cols_draw.argtypes) == len(lib.q3_batch_step_cols.argtypes) + 1          # keep
    assert len(lib.q3_generate_many_sampled.argtypes) == len(lib.q3_generate_many_greedy.argtypes) + 3    # temperature, top-p, seeds


@pytest.fixture(scope="module")
def rows(q3, oracle, tmp_ckpt_dir):
    """row(r, T, p, seed, discard): request r on the C oracle.  discard = True is the chat rule: a sample drawn (and dropped) at
    every prompt position, the last one kept; False draws at the prompt's last position only.  T = 0 is the argmax."""
    shape = q3.checkpoint.SHAPES[NAME]
    path = os.path.join(tmp_ckpt_dir, f"colsdraw-{NAME}-{CKPT_SEED}.bin")
    q3.checkpoint.ensure_synthetic_checkpoint(path, shape, seed=CKPT_SEED)
    m = oracle.OracleModel(path, 0)
    P = prompts(shape.vocab_size)
    made = {}

    def row(r, T, p, seed, discard=True):
        key = (r, T, p, seed, discard)
        if key not in made:
            s = oracle.Sampler(shape.vocab_size, T, p, seed)
            pick = (lambda lg: s.sample(lg)) if T > 0 else oracle.sample_argmax
            tok, out = None, []
            for pos, t in enumerate(P[r]):                   # a column reads rows 0 .. pos only: no reset between requests
                lg = m.forward(t, pos)
                if discard or pos == len(P[r]) - 1:
                    tok = pick(lg)
            out.append(tok)
            for k in range(N_NEW[r] - 1):
                tok = pick(m.forward(tok, len(P[r]) + k))
                out.append(tok)
            made[key] = out
        return made[key]
    yield row
    m.close()


@pytest.mark.parametrize("r", range(len(PROMPT_LEN)), ids=lambda r: f"len{PROMPT_LEN[r]}")
@pytest.mark.parametrize("which", [0, 1], ids=lambda w: f"s{SEEDS[w] & 0xffff}")
@pytest.mark.parametrize("sampler", SAMPLERS, ids=sampler_id)
def test_cases_tell_right_from_wrong(rows, sampler, which, r):
    T, p = sampler
    right = rows(r, T, p, SEEDS[which])
    assert len(right) == N_NEW[r]
    assert right != rows(r, T, p, SEEDS[1 - which]), "the two seeds swapped give the same row"
    if PROMPT_LEN[r] > 1:                                     # a prompt of one token has no discarded coin
        assert right != rows(r, T, p, SEEDS[which], discard=False), "the row does not depend on the prompt's discarded coins"
    assert right != rows(r, 0.0, p, 0), "the sampled row is the greedy row"
