"""Scores (include/qwen3_hip.h section 2l): what can be checked without a GPU -- the entry point's first refusal and its place in
the ABI, the record restated in numpy (tests/score_ref.py) against the C oracle's softmax and argmax, the log-probability's error
bound, the host-only schedule count, and generation.score / loglikelihood / perplexity and the command line over a stub."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import score_ref
from conftest import ROOT, assert_biteq, golden_path

f32 = np.float32


def test_a_null_engine_is_refused_before_anything_touches_the_gpu(q3):
    lib = q3.load_library()
    lens = (C.c_size_t * 1)(3)
    toks = (C.c_int32 * 3)(1, 2, 3)
    out = (C.c_float * 8)()
    assert lib.q3_score_many(None, toks, lens, 1, None, 0, out, None) == -3
    assert b"null engine" in lib.q3_last_error()


def test_the_symbols_are_exported_declared_and_listed(q3):
    header = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    for sym in ("q3_score_many", "q3_score_pack"):
        assert sym in q3.EXPORTED_SYMBOLS and hasattr(q3.load_library(), sym)
    assert "int q3_score_many(q3_engine* e," in header and "int q3_score_pack(const size_t* prompt_len," in header
    assert "#define Q3_SCORE_PREFIX " in header
    assert int(header.split("#define Q3_SCORE_PREFIX ")[1].split()[0].rstrip("u")) == q3.SCORE_PREFIX == q3.EMBED_PREFIX
    assert "typedef struct q3_score_rec { float target; float max; float sum; int32_t argmax; } q3_score_rec;" in header
    assert q3.SCORE_DTYPE == score_ref.DTYPE and q3.SCORE_DTYPE.itemsize == 16
    assert header.index("2l. (behind 2k") > header.index("int q3_choice_many(")


@pytest.mark.parametrize("name", ["tiny.bin", "tiny-untied.bin"])
def test_the_record_is_the_oracles_softmax_and_argmax(oracle, q3, name):
    """at every position of three prompts: expf(target - max) * (1.0f / sum) of the record is q3o_softmax(logits)[target] bit for
    bit, the record's argmax is q3o_sample_argmax, and logprobs_of is within the bound of a float64 log-softmax"""
    path = golden_path(name)
    om = oracle.OracleModel(path)
    V = om.get_config().vocab_size
    for prompt in ([5, 9], [1, 2, 3, 4, V - 1, 0], [200, 17, 17, 3, 90, 41, 8, 17]):
        om.reset()
        for pos in range(len(prompt) - 1):
            l = np.array(om.forward(prompt[pos], pos), copy=True)
            t = prompt[pos + 1]
            rec = score_ref.record(l, t)
            assert_biteq(np.array([score_ref.prob(l, t)]), oracle.softmax(l)[t:t + 1], f"{name}: position {pos} of {prompt}")
            assert int(rec["argmax"]) == oracle.sample_argmax(l)
            assert rec["max"] == l.max() and rec["target"] == l[t]
            d = abs(float(q3.logprobs_of(rec.reshape(1))[0]) - score_ref.log_softmax64(l, t))
            assert d <= 2 * V * 2.0 ** -24, (name, pos, d)


def test_logprobs_of_on_a_full_size_gaussian_row(q3):
    """151,936 Gaussian logits: |logprobs_of - float64 log-softmax| <= 2 V 2^-24, twice the first-order bound of a sequential f32
    sum of V non-negative terms"""
    V = 151936
    l = (np.random.default_rng(5).standard_normal(V) * 3.0).astype(f32)
    for t in (0, V - 1, int(np.argmax(l)), int(np.argmin(l))):
        rec = score_ref.record(l, t).reshape(1)
        got = q3.logprobs_of(rec)
        assert got.dtype == np.float64 and np.array_equal(got, score_ref.logprobs_of(rec))
        assert abs(float(got[0]) - score_ref.log_softmax64(l, t)) <= 2 * V * 2.0 ** -24
    assert int(rec["argmax"][0]) == int(np.argmax(l))


def test_score_ref_on_hand_made_rows():
    # ties: the last index wins; -0.0 sorts below +0.0; the sum starts from -0.0 and walks in index order
    l = np.array([1.0, 3.0, -2.0, 3.0, 0.5], dtype=f32)
    r = score_ref.record(l, 2)
    assert (float(r["target"]), float(r["max"]), int(r["argmax"])) == (-2.0, 3.0, 3)
    e = score_ref.expf((l - f32(3.0)).astype(f32))
    assert r["sum"] == f32(f32(f32(f32(e[0] + e[1]) + e[2]) + e[3]) + e[4])
    assert score_ref.argmax_last(np.array([0.0, -0.0, 0.0, -0.0], dtype=f32)) == 2
    assert score_ref.argmax_last(np.array([-0.0, -0.0], dtype=f32)) == 1
    big = np.array([2.0 ** -24] * 4 + [1.0], dtype=f32)          # order matters: the small terms first survive, behind the 1.0 they would not
    assert score_ref.seq_sum(big) == f32(1.0) + f32(2.0 ** -22) and score_ref.seq_sum(big[::-1]) == f32(1.0)


def test_logprobs_of_on_hand_made_records(q3):
    V = 151936
    recs = np.zeros(4, dtype=q3.SCORE_DTYPE)
    recs["sum"] = [V, 0.0, np.nan, np.inf]
    recs["argmax"] = V - 1
    lp = q3.logprobs_of(recs)
    assert lp.dtype == np.float64 and lp[0] == -math.log(V)                      # a flat row: exactly -log(V)
    with np.errstate(divide="ignore"):
        assert lp[1] == 0.0 - np.log(np.float64(0.0)) and np.isinf(lp[1])        # sum == 0: what numpy's log gives
    assert np.isnan(lp[2]) and lp[3] == -np.inf
    nan_t = np.zeros(1, dtype=q3.SCORE_DTYPE)
    nan_t["target"], nan_t["sum"] = np.nan, 1.0
    assert np.isnan(q3.logprobs_of(nan_t)[0])
    one = np.zeros(1, dtype=q3.SCORE_DTYPE)
    one["target"], one["max"], one["sum"] = -np.inf, 0.0, 2.0
    assert q3.logprobs_of(one)[0] == -np.inf
    assert q3.perplexity([np.array([-1.0, -2.0]), np.array([]), np.array([-3.0])]) == math.exp(2.0) and math.isnan(q3.perplexity([]))


def stats_tuple(st):
    return (st.waves, st.blocks, st.live_columns, st.pad_columns, st.chunks, st.scored)


@pytest.mark.parametrize("scored", [31, 32, 33, 64, 65])
def test_the_schedule_count_at_chunk_edges(q3, scored):
    """one request of scored + 1 tokens is one block with `scored` scored columns"""
    st = q3.score_pack([scored + 1], None, 4, 2048)
    assert stats_tuple(st) == (1, 1, scored + 1, (-(scored + 1)) % 8, (scored + 31) // 32, scored)
    assert stats_tuple(st) == score_ref.schedule([scored + 1], None, 4, 2048)
    # ... and split over three requests of one block
    lens = [10, scored - 20, 13]
    st = q3.score_pack(lens, None, 4, 2048)
    assert st.blocks == 1 and st.chunks == (scored + 31) // 32 and st.scored == scored
    assert stats_tuple(st) == score_ref.schedule(lens, None, 4, 2048)


def test_the_schedule_count_on_hand_made_requests(q3):
    # score_from empties the first block of a request split over two: its 8 scored columns, inputs 39 .. 46, all lie in the second
    st = q3.score_pack([48], [40], 2, 32)
    assert stats_tuple(st) == (1, 2, 48, 0, 1, 8) == score_ref.schedule([48], [40], 2, 32)
    st = q3.score_pack([48], [8], 2, 32)                  # inputs 7 .. 46: 25 in the first block, 15 in the second, a chunk each
    assert (st.chunks, st.scored) == (2, 40)
    # score_from == n and one-token requests give no record; a block with none has no chunk
    st = q3.score_pack([1, 9, 1], [1, 9, 1], 8, 2048)
    assert stats_tuple(st) == (1, 1, 11, 21, 0, 0)            # columns 0, 8 .. 16 and 24 of a 32-column block
    st = q3.score_pack([5, 1, 7], None, 2, 2048)          # two waves: {5, 1} and {7}
    assert stats_tuple(st) == (2, 2, 13, 11, 2, 10) == score_ref.schedule([5, 1, 7], None, 2, 2048)
    rng = np.random.default_rng(11)
    for _ in range(60):
        n = int(rng.integers(1, 12))
        lens = [int(v) for v in rng.integers(1, 150, n)]
        sf = None if rng.random() < 0.3 else [int(rng.integers(1, v + 1)) for v in lens]
        streams, cap = int(rng.integers(1, 9)), int(rng.choice([32, 64, 128, 2048]))
        assert stats_tuple(q3.score_pack(lens, sf, streams, cap)) == score_ref.schedule(lens, sf, streams, cap), (lens, sf, streams, cap)
    for lens, sf, streams, cap in (([], None, 2, 32), ([3, 0], None, 2, 32), ([3], [0], 2, 32), ([3], [4], 2, 32), ([3], None, 0, 32),
                                   ([3], None, 33, 32), ([3], None, 2, 24)):
        with pytest.raises(IndexError):
            q3.score_pack(lens, sf, streams, cap)
    with pytest.raises(IndexError):
        q3.score_pack([3, 4], [1], 2, 32)


class _Stub:
    """a transformer whose score_many answers from a table of hand-made records per (token, next token) and records its calls"""

    def __init__(self):
        self.calls, self.prefix = [], []

    def batch_prefix_get(self):
        return self.prefix

    def batch_prefix_set(self, p):
        self.prefix = list(p)

    @staticmethod
    def rec(a, b):
        """behind token a with target b: two candidates carry all the mass; the greedy next token is a + 1"""
        r = np.zeros((), dtype=score_ref.DTYPE)
        r["target"], r["max"], r["sum"], r["argmax"] = (0.0 if b == a + 1 else -1.0 - (b % 3)), 0.0, 2.0, a + 1
        return r

    def score_many(self, prompts, score_from=None, use_prefix=False):
        self.calls.append(([list(p) for p in prompts], None if score_from is None else list(score_from), use_prefix))
        sf = [1] * len(prompts) if score_from is None else score_from
        out = []
        for p, f in zip(prompts, sf):
            out.append(np.array([self.rec(p[i], p[i + 1]) for i in range(f - 1, len(p) - 1)], dtype=score_ref.DTYPE).reshape(max(0, len(p) - f)))
        return out, None


def test_score_loglikelihood_and_perplexity_on_a_stub(q3):
    t = _Stub()
    prompts = [[1, 2, 3, 9], [7], [4, 5]]
    lps = q3.score(t, prompts)
    assert [a.size for a in lps] == [3, 0, 1] and all(a.dtype == np.float64 for a in lps)
    ln2 = math.log(2.0)
    assert np.array_equal(lps[0], np.array([-ln2, -ln2, -1.0 - ln2])) and lps[2][0] == -ln2
    assert t.calls[-1] == (prompts, None, False)
    assert q3.perplexity(lps) == math.exp(-np.concatenate(lps).mean())
    part = q3.score(t, prompts, [3, 1, 2])
    assert np.array_equal(part[0], lps[0][2:]) and part[1].size == 0 and part[2].size == 0
    assert t.calls[-1][1] == [3, 1, 2]
    with pytest.raises(ValueError):
        q3.score(t, [[1], []])
    # a token list as the prefix: prompts and score_from are the suffixes'
    q3.score(t, [[2, 3], [2, 9]], [1, 2], shared_prefix=[1])
    assert t.prefix == [1] and t.calls[-1] == ([[2, 3], [2, 9]], [1, 2], True)
    # True: the common prefix, cut so that the earliest scored position's input stays in the suffix
    t2 = _Stub()
    full = [[1, 2, 3, 4, 5], [1, 2, 3, 4, 9, 9]]
    got = q3.score(t2, full, [4, 4], shared_prefix=True)
    assert t2.prefix == [1, 2, 3] and t2.calls[-1] == ([[4, 5], [4, 9, 9]], [1, 1], True)
    assert [a.tolist() for a in got] == [a.tolist() for a in q3.score(_Stub(), full, [4, 4])]
    t3 = _Stub()
    q3.score(t3, full, None, shared_prefix=True)                  # every position is scored: nothing can be resident
    assert t3.prefix == [] and t3.calls[-1] == (full, None, False)
    # loglikelihood: one call, score_from = len(context); greedy means argmax == target at every continuation position
    t4 = _Stub()
    ll = q3.loglikelihood(t4, [[1, 2], [1, 2], [5]], [[3, 4], [3, 9], [6]])
    assert len(t4.calls) == 1 and t4.calls[0] == ([[1, 2, 3, 4], [1, 2, 3, 9], [5, 6]], [2, 2, 1], False)
    assert ll[0] == (-2 * ln2, True) and ll[2] == (-ln2, True)
    assert ll[1][1] is False and ll[1][0] == (-ln2) + (-1.0 - ln2)
    with pytest.raises(ValueError):
        q3.loglikelihood(t4, [[]], [[1]])
    with pytest.raises(ValueError):
        q3.loglikelihood(t4, [[1]], [[1], [2]])


def test_the_command_line_knows_the_score_verb(q3):
    from qwen3_rs_amd import cli
    a = cli.build_parser().parse_args(["score", "model.bin", "-i", "one", "-i", "two", "--context", "Given", "--streams", "4", "-o", "out.npy"])
    assert (a.cmd, a.checkpoint, a.input, a.context, a.streams, a.output, a.ctx) == ("score", "model.bin", ["one", "two"], "Given", 4, "out.npy", None)
    b = cli.build_parser().parse_args(["score", "model.bin", "-i", "one"])
    assert (b.context, b.output, b.streams) == (None, None, 8)
    # what the verb asks generation.score for
    assert cli.score_requests([], [[1, 2], [3]]) == ([[1, 2], [3]], None, None)
    assert cli.score_requests([7, 8, 9], [[1, 2]]) == ([[7, 8, 9, 1, 2]], [3], None)
    assert cli.score_requests([7, 8, 9], [[1, 2], [3]]) == ([[9, 1, 2], [9, 3]], [1, 1], [7, 8])
    assert cli.score_requests([7], [[1, 2], [3]]) == ([[7, 1, 2], [7, 3]], [1, 1], None)
