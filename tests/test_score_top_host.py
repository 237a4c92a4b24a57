"""Top-k log-probabilities (include/qwen3_hip.h section 2m): what can be checked without a GPU -- the entry point's first refusals
and its place in the ABI, the order restated in numpy (tests/score_top_ref.py) on hand-made rows and against the C oracle's argmax,
the error bound of the alternatives' log-probabilities, and generation.top_logprobs and the command line over a stub."""
import ctypes as C
import os

import numpy as np
import pytest

import score_ref
import score_top_ref as tr
from conftest import ROOT, golden_path
from test_score_host import _Stub

f32 = np.float32


def test_the_symbol_is_exported_declared_and_listed(q3):
    header = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    assert "q3_score_top_many" in q3.EXPORTED_SYMBOLS and hasattr(q3.load_library(), "q3_score_top_many")
    assert "int q3_score_top_many(q3_engine* e," in header
    assert header.index("2m. (behind 2l") > header.index("int q3_score_pack(")
    assert "typedef struct q3_score_top { float logit; int32_t index; } q3_score_top;" in header
    assert int(header.split("#define Q3_SCORE_TOP_MAX ")[1].split()[0]) == q3.SCORE_TOP_MAX == tr.TOP_MAX == 64
    assert int(header.split("#define Q3_ABI_VERSION ")[1].split()[0]) == 1 and q3.load_library().q3_abi_version() == 1
    assert q3.TOP_DTYPE == tr.DTYPE and q3.TOP_DTYPE.itemsize == 8
    # everything in front of the new section is what it was: the section stands behind the last declaration of 2l
    assert header.index("int q3_score_top_many(") > header.index("#define Q3_SCORE_TOP_MAX") > header.index("2m. (behind 2l")


@pytest.mark.parametrize("k", [5, 0, -1, 65])
def test_a_null_engine_and_a_k_out_of_range_are_refused_before_anything_touches_the_gpu(q3, k):
    lib = q3.load_library()
    lens = (C.c_size_t * 1)(3)
    toks = (C.c_int32 * 3)(1, 2, 3)
    out, top, rank = (C.c_float * 8)(), (C.c_float * 2 * 2 * 64)(), (C.c_int32 * 2)()
    assert lib.q3_score_top_many(None, toks, lens, 1, None, 0, k, out, top, rank, None) == -3
    assert (b"null engine" if k == 5 else b"out of range (1..64)") in lib.q3_last_error()


def test_the_reference_on_hand_made_rows():
    # ties in the logit go to the higher index
    l = np.array([1.0, 3.0, -2.0, 3.0, 0.5, 1.0], dtype=f32)
    t = tr.top(l, 4)
    assert t["index"].tolist() == [3, 1, 5, 0] and t["logit"].tolist() == [3.0, 3.0, 1.0, 1.0]
    assert int(tr.top(l, 1)["index"][0]) == score_ref.argmax_last(l)
    # -0.0 sorts below +0.0
    z = np.array([0.0, -0.0, 0.0, -0.0], dtype=f32)
    tz = tr.top(z, 4)
    assert tz["index"].tolist() == [2, 0, 3, 1] and np.signbit(tz["logit"]).tolist() == [False, False, True, True]
    # k == V: the whole row, sorted; the keys strictly descending
    full = tr.top(l, l.size)
    assert full["index"].tolist() == [3, 1, 5, 0, 4, 2] and (tr.keys_of(full)[1:] < tr.keys_of(full)[:-1]).all()
    assert np.array_equal(tr.keys_of(full), tr.top_keys(l, l.size))
    # the rank of tied targets: the higher index stands in front
    assert [tr.rank(l, i) for i in range(l.size)] == [3, 1, 5, 0, 4, 2]
    assert [tr.rank(z, i) for i in range(4)] == [1, 3, 0, 2]
    for i in range(l.size):
        assert int(full["index"][tr.rank(l, i)]) == i
    # -inf and +inf are ordinary entries
    e = np.array([-np.inf, 2.0, np.inf, -np.inf], dtype=f32)
    assert tr.top(e, 4)["index"].tolist() == [2, 1, 3, 0]
    with pytest.raises(AssertionError):
        tr.assert_tops(tr.top(l, 2), tr.top(l, 3)[1:], "shifted")
    with pytest.raises(AssertionError):
        tr.assert_tops(tr.top(z, 4), tr.top(z, 4)[[0, 1, 3, 2]], "a swapped tie")
    tr.assert_tops(tr.top(l, 3), full[:3], "a prefix")


@pytest.mark.parametrize("name", ["tiny.bin", "tiny-untied.bin"])
def test_the_first_is_the_oracles_argmax_and_the_logprobs_are_in_bound(oracle, q3, name):
    """at every position of three prompts, on the C oracle's logits: top(l, 1) is q3o_sample_argmax; top_logprobs_of over the
    reference's record and top 64 is within 2 V 2^-24 of a float64 log-softmax at every alternative (the bound of logprobs_of: the
    same expression with another logit in the place of the target's)"""
    om = oracle.OracleModel(golden_path(name))
    V = om.get_config().vocab_size
    k = min(64, V)
    for prompt in ([5, 9], [1, 2, 3, 4, V - 1, 0], [200, 17, 17, 3, 90, 41, 8, 17]):
        om.reset()
        for pos in range(len(prompt) - 1):
            l = np.array(om.forward(prompt[pos], pos), copy=True)
            t = tr.top(l, k)
            assert int(tr.top(l, 1)["index"][0]) == int(t["index"][0]) == oracle.sample_argmax(l)
            rec = score_ref.record(l, prompt[pos + 1]).reshape(1)
            lp = q3.top_logprobs_of(rec, t.reshape(1, k))
            assert lp.dtype == np.float64 and lp.shape == (1, k) and (np.diff(lp[0]) <= 0).all()
            for j in range(k):
                assert abs(lp[0, j] - score_ref.log_softmax64(l, int(t["index"][j]))) <= 2 * V * 2.0 ** -24, (name, pos, j)
            r = tr.rank(l, prompt[pos + 1])
            if r < k:
                assert lp[0, r] == q3.logprobs_of(rec)[0]


class _TopStub(_Stub):
    """test_score_host's stub with score_top_many: behind token a the alternatives are a + 1 (logit 0.0), then a + 2, a + 3, ...
    (logits -1.0, -2.0, ...); the rank of target b is b - a - 1 where that is not negative, 99 otherwise"""

    def score_top_many(self, prompts, k, score_from=None, use_prefix=False):
        recs, _ = self.score_many(prompts, score_from, use_prefix)
        self.calls[-1] = self.calls[-1] + (k,)
        sf = [1] * len(prompts) if score_from is None else score_from
        tops, ranks = [], []
        for p, f in zip(prompts, sf):
            ins = p[f - 1:len(p) - 1] if f >= 1 else []
            t = np.zeros((len(ins), k), dtype=tr.DTYPE)
            for i, a in enumerate(ins):
                t["index"][i] = a + 1 + np.arange(k)
                t["logit"][i] = -np.arange(k, dtype=f32)
            tops.append(t)
            ranks.append(np.array([b - a - 1 if b > a else 99 for a, b in zip(ins, p[f:])], dtype=np.int32))
        return recs, tops, ranks, None


def test_top_logprobs_on_a_stub(q3):
    t = _TopStub()
    prompts = [[1, 2, 3, 9], [7], [4, 5]]
    res = q3.top_logprobs(t, prompts, 3)
    assert t.calls[-1] == (prompts, None, False, 3)
    assert [len(x) for x in res] == [4, 4, 4] and [x[0].size for x in res] == [3, 0, 1]
    lps = q3.score(_Stub(), prompts)
    ln2 = np.log(2.0)
    for (lp, ids, tlp, rank), want in zip(res, lps):
        assert np.array_equal(lp, want) and lp.dtype == np.float64 and tlp.dtype == np.float64
        assert ids.dtype == np.int32 and rank.dtype == np.int32 and ids.shape == tlp.shape == (lp.size, 3) and rank.shape == lp.shape
        assert np.array_equal(tlp, np.tile(np.array([0.0, -1.0, -2.0]) - ln2, (lp.size, 1)))
    assert res[0][1].tolist() == [[2, 3, 4], [3, 4, 5], [4, 5, 6]] and res[0][3].tolist() == [0, 0, 5] and res[1][1].shape == (0, 3)
    # score_from
    part = q3.top_logprobs(t, prompts, 2, [3, 1, 2])
    assert t.calls[-1] == (prompts, [3, 1, 2], False, 2)
    assert np.array_equal(part[0][0], lps[0][2:]) and part[0][1].tolist() == [[4, 5]] and part[2][0].size == 0
    # a token list as the prefix, and True: the handling of score()
    q3.top_logprobs(t, [[2, 3], [2, 9]], 4, [1, 2], shared_prefix=[1])
    assert t.prefix == [1] and t.calls[-1] == ([[2, 3], [2, 9]], [1, 2], True, 4)
    t2 = _TopStub()
    full = [[1, 2, 3, 4, 5], [1, 2, 3, 4, 9, 9]]
    got = q3.top_logprobs(t2, full, 2, [4, 4], shared_prefix=True)
    assert t2.prefix == [1, 2, 3] and t2.calls[-1] == ([[4, 5], [4, 9, 9]], [1, 1], True, 2)
    plain = q3.top_logprobs(_TopStub(), full, 2, [4, 4])
    for a, b in zip(got, plain):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        q3.top_logprobs(t, [[1], []], 2)


def test_top_logprobs_of_on_hand_made_records(q3):
    recs = np.zeros(2, dtype=q3.SCORE_DTYPE)
    recs["max"], recs["sum"] = [1.0, 0.0], [4.0, 151936.0]
    tops = np.zeros((2, 3), dtype=q3.TOP_DTYPE)
    tops["logit"] = [[1.0, 0.5, -np.inf], [0.0, 0.0, 0.0]]
    lp = q3.top_logprobs_of(recs, tops)
    assert lp.dtype == np.float64 and lp.shape == (2, 3)
    assert lp[0].tolist() == [-np.log(4.0), -0.5 - np.log(4.0), -np.inf] and (lp[1] == -np.log(151936.0)).all()
    # the same expression as logprobs_of
    recs["target"] = tops["logit"][:, 1]
    assert np.array_equal(lp[:, 1], q3.logprobs_of(recs))
    assert q3.top_logprobs_of(recs[:0], tops[:0]).shape == (0, 3)


def test_score_over_the_existing_stub_still_works(q3):
    """score, loglikelihood and perplexity pass score_many exactly (prompts, score_from, use_prefix)"""
    t = _Stub()
    lps = q3.score(t, [[1, 2, 3], [4, 5]], [2, 1], shared_prefix=None)
    assert t.calls[-1] == ([[1, 2, 3], [4, 5]], [2, 1], False) and [a.size for a in lps] == [1, 1]
    assert q3.loglikelihood(t, [[1]], [[2, 3]])[0] == (2 * -np.log(2.0), True)
    assert not hasattr(t, "score_top_many")


def test_the_command_line_knows_top(q3):
    from qwen3_rs_amd import cli
    a = cli.build_parser().parse_args(["score", "model.bin", "-i", "one", "--top", "5", "-o", "out.npz"])
    assert (a.cmd, a.top, a.output, a.input) == ("score", 5, "out.npz", ["one"])
    b = cli.build_parser().parse_args(["score", "model.bin", "-i", "one", "-i", "two", "--context", "Given", "--streams", "4", "-o", "out.npy"])
    assert (b.cmd, b.checkpoint, b.input, b.context, b.streams, b.output, b.ctx, b.top) == ("score", "model.bin", ["one", "two"], "Given", 4, "out.npy", None, None)
    for bad in ("0", "65"):
        assert cli.run_score(cli.build_parser().parse_args(["score", "model.bin", "-i", "one", "--top", bad])) == 1
