"""CPU tests of section 2d of include/qwen3_hip.h (q3_verify_draw / q3_generate_lookup_draw): the two names are declared, listed and
exported, and the cases the GPU lookup test runs are not vacuous -- on the C oracle's own sampled output each of them accepts at
least one draft and rejects at least one."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from spec_draw_cases import N_REF, ORACLE_MODELS, case_id, g7, lookup_cases
from spec_sim import simulate

NEW = {"q3_verify_draw", "q3_generate_lookup_draw"}


def test_header_symbol_list_and_binary_agree_on_the_new_names(q3):
    hdr = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    declared = set(re.findall(r"\b(q3_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(q3.EXPORTED_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", q3.lib_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert NEW <= exported
    lib = q3.load_library()
    assert lib.q3_verify_draw.argtypes == lib.q3_verify.argtypes
    assert lib.q3_generate_lookup_draw.argtypes == lib.q3_generate_lookup.argtypes
    # the product still does not link the oracle
    assert "oracle" not in subprocess.check_output(["ldd", q3.lib_path()], text=True)
    assert not [l for l in out.splitlines() if "q3o_" in l]


_oracle_runs = {}


def oracle_sampled(q3, oracle, tmp_ckpt_dir, name, T, p, seed, p0):
    """G = the sampled loop of generation.rs:153-162 on the C oracle: forward, Sampler::sample, N_REF tokens from position p0"""
    key = (name, T, p, seed, p0)
    if key not in _oracle_runs:
        ck_seed, tok0, ctx = ORACLE_MODELS[name]
        path = os.path.join(tmp_ckpt_dir, f"draw-{name}-{ck_seed}.bin")
        q3.checkpoint.ensure_synthetic_checkpoint(path, q3.checkpoint.SHAPES[name], seed=ck_seed)
        m = oracle.OracleModel(path, ctx)
        s = oracle.Sampler(q3.checkpoint.SHAPES[name].vocab_size, T, p, seed)
        G, tok = [], tok0
        for k in range(N_REF):
            tok = s.sample(m.forward(tok, p0 + k))
            G.append(tok)
        m.close()
        _oracle_runs[key] = G
    return _oracle_runs[key]


@pytest.mark.parametrize("case", lookup_cases(), ids=case_id)
def test_gpu_lookup_cases_accept_and_reject(q3, oracle, tmp_ckpt_dir, case):
    name, T, p, seed, ngram, draft_len, p0 = case
    G = oracle_sampled(q3, oracle, tmp_ckpt_dir, name, T, p, seed, p0)
    sim = simulate(G, g7(G, q3.checkpoint.SHAPES[name].vocab_size), ORACLE_MODELS[name][1], ngram, draft_len)
    assert sim["accepted"] > 0, sim
    assert sim["drafted"] > sim["accepted"] and any(a < d for d, a in sim["passes"]), sim
