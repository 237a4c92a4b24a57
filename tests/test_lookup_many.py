"""Prompt-lookup drafts inside generate_many (include/qwen3_hip.h section 2u; csrc/q3_lookup_dev.h).  Nothing here has a tolerance:
the device drafter equals the host definition q3_lookup_draft, and q3_generate_many_lookup equals q3_generate_many_stop token for
token, whatever ngram, draft_len and fill_width are.

The loop runs on the synthetic tiny-g64 checkpoint (seed 2468, the one test_cols_stop.py uses), not on tests/golden/tiny.bin: tiny.bin
has group_size 16, which q3_batch_init refuses, so no batched loop can run on it.  The requests and cases are the ones asked for."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C = 4096                                 # Q3_LOOKUP_CHUNK: candidate starts the search stages in LDS at a time
Z = [0] * (C + 97)                       # with (1, 2, 1) behind it: C + 100 tokens whose suffix occurs nowhere else; the cases add one match

DRAFT_CASES = {
    # name: (sequence, ngram, draft_len)
    "n_below_ngram": ([0, 1], 3, 4),
    "n_equals_ngram": ([0, 1], 2, 4),
    "no_match": ([0] * 9 + [1], 1, 4),
    "only_match_at_0": ([1, 2] + [0] * 20 + [1], 1, 4),
    "latest_match_overlaps_suffix": ([0] * 10, 3, 5),                       # i = n - g - 1: a draft of one token
    "cut_by_draft_len": ([0, 1, 2] * 10, 2, 2),
    "cut_by_end_of_s": ([0, 1, 2] * 10, 2, 31),                             # i = n - g - 3: three tokens are left
    "ngram_longer_than_lds_window": ([0, 1, 2, 2, 1] * 20, 40, 31),
    # the only match at i = 0 with n - ngram = C - 2 .. C + 1 candidate starts: one chunk, exactly one, one start into a second
    "n_chunk_minus_1": ([1, 2] + [0] * (C - 4) + [1], 1, 3),
    "n_chunk": ([1, 2] + [0] * (C - 3) + [1], 1, 3),
    "n_chunk_plus_1": ([1, 2] + [0] * (C - 2) + [1], 1, 3),
    "n_chunk_plus_2": ([1, 2] + [0] * (C - 1) + [1], 1, 3),
    # n = C + 100, ngram 3: the chunk nearest the end holds starts 97 .. C + 96
    "window_straddles_two_chunks": (Z[:96] + [1, 2, 1] + Z[99:] + [1, 2, 1], 3, 4),     # starts at 96, ends at 98
    "first_start_of_last_chunk": (Z[:97] + [1, 2, 1] + Z[100:] + [1, 2, 1], 3, 4),
    "match_in_second_chunk_only": (Z[:10] + [1, 2, 1, 2] + Z[14:] + [1, 2, 1], 3, 4),
}


@pytest.mark.parametrize("name", list(DRAFT_CASES))
def test_device_drafter_equals_the_definition(q3, name):
    seq, ngram, draft_len = DRAFT_CASES[name]
    want = q3.lookup_draft(seq, ngram, draft_len)
    assert q3.op_lookup_draft(seq, ngram, draft_len) == want
    if name not in ("n_below_ngram", "n_equals_ngram", "no_match"):
        assert want, "the case is meant to have a draft"


# One request set for every loop test: ragged prompts (one of a single token), more requests than slots, n_new of 1 and 2, request 4
# runs to the last position of the context (17 + 80 - 1 = 96 = seq_len of tiny-g64).  STOP = 347 is in the plain loop's rows: request 5
# produces 376 sixteen times and then 347, its 17th token -- under ngram 1 and fill_width >= 8 an accepted draft that ends the request.
SLOTS = 4
PROMPT_LEN = [5, 1, 9, 3, 17, 2, 4]
N_NEW = [12, 20, 1, 2, 80, 40, 16]
STOP = [347]


@pytest.fixture(scope="module")
def loop(q3, tmp_path_factory):
    """the engine, the prompts and what the plain stop loop makes of them, with and without the stop token: computed once"""
    rng = np.random.default_rng(7)
    prompts = [[int(v) for v in rng.integers(0, 512, k)] for k in PROMPT_LEN]
    path = str(tmp_path_factory.mktemp("lookup") / "tiny-g64.bin")
    q3.checkpoint.write_synthetic_checkpoint(path, q3.checkpoint.SHAPES["tiny-g64"], seed=2468)
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(SLOTS)
        plain = {stop: t.generate_many_stop(prompts, N_NEW, list(stop), raw=True) for stop in ((), tuple(STOP))}
        yield t, prompts, plain


@pytest.mark.parametrize("draft_len", [1, 7])
@pytest.mark.parametrize("ngram", [1, 3])
@pytest.mark.parametrize("fill_width", [0, 8, 32])
def test_lookup_loop_equals_the_plain_loop(loop, fill_width, ngram, draft_len):
    t, prompts, plain = loop
    want_out, want_n, want_stats = plain[tuple(STOP)]
    assert want_n == [12, 20, 1, 2, 80, 17, 16]              # the set is what the comment above says
    out, n_out, stats, ls = t.generate_many_lookup(prompts, N_NEW, STOP, ngram=ngram, draft_len=draft_len, fill_width=fill_width, raw=True)
    assert n_out == want_n
    assert out == want_out                                   # the -1 behind every request's last token included
    assert ls.accepted <= ls.drafted
    assert stats.passes <= want_stats.passes
    assert stats.live_columns == stats.prompt_columns + stats.decode_columns + ls.drafted


def test_accepted_drafts_save_passes(loop):
    """The same requests without a stop token, ngram 1, draft_len 7, fill_width 8.  Found on the CPU: the greedy rows of the checkpoint
    came from the C oracle (forward + sample_argmax per token), and a host restatement of the loop -- q3_lookup_draft over prompt +
    row so far, rule 6 and the accept walk -- counted 81 passes for the plain loop and 54 passes, 93 drafted, 55 accepted here:
    requests 4 and 5 settle into long repeats (246 ..., 285 ..., 376 ..., 347 ...) that a one-token match continues."""
    t, prompts, plain = loop
    want_out, want_n, want_stats = plain[()]
    out, n_out, stats, ls = t.generate_many_lookup(prompts, N_NEW, [], ngram=1, draft_len=7, fill_width=8, raw=True)
    assert (out, n_out) == (want_out, want_n)
    assert ls.accepted >= 1
    assert stats.passes < want_stats.passes


@pytest.mark.parametrize("setting", ["sampling_batch", "penalties"])
def test_refusals_leave_the_engine_usable(q3, loop, setting):
    t, prompts, plain = loop
    if setting == "sampling_batch":
        t.set_batch_sampler(0.8, 0.9, list(range(SLOTS)))
    else:
        t.set_penalties(0.5, 0.0)
    try:
        with pytest.raises(q3.Q3Error) as err:
            t.generate_many_lookup(prompts, N_NEW, STOP)
        assert err.value.code == -5 and ("sampler" if setting == "sampling_batch" else "q3_sampler_penalties") in err.value.msg
    finally:
        t.set_batch_sampler(0.0, 0.9, list(range(SLOTS)))
        t.set_penalties(0.0, 0.0)
    assert t.generate_many_stop(prompts, N_NEW, STOP, raw=True) == plain[tuple(STOP)]
