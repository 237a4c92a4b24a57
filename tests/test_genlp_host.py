"""Log-probabilities of generated tokens (include/qwen3_hip.h section 2o): what can be checked without a GPU -- the three entry
points' place in the ABI and their first refusals, the Python wrappers' checks in front of the library, and the cutting of rows and
tuples to n_out over a stub library and a stub engine."""
import ctypes as C
import os

import numpy as np
import pytest

import genlp_ref
import score_ref
import score_top_ref as tr
from conftest import ROOT

f32 = np.float32
SYMBOLS = ("q3_gen_logprobs", "q3_gen_logprobs_get", "q3_gen_logprobs_read")


def test_the_symbols_are_exported_declared_and_listed(q3):
    header = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    lib = q3.load_library()
    for sym in SYMBOLS:
        assert sym in q3.EXPORTED_SYMBOLS and hasattr(lib, sym) and f"int {sym}(" in header
    # the section stands behind the last declaration of 2n; the ABI version stays
    assert header.index("int q3_gen_logprobs(") > header.index("2o. (behind 2n") > header.index("int q3_op_sample_top_k(")
    assert int(header.split("#define Q3_ABI_VERSION ")[1].split()[0]) == 1 and lib.q3_abi_version() == 1
    # it says what it leaves alone
    section = header[header.index("2o. (behind 2n"):]
    for name in ("q3_batch_step_cols[_draw]", "section 2b", "verify paths", "single-stream decode"):
        assert name in section, name


@pytest.mark.parametrize("top_n", [5, -2, 65])
def test_a_null_engine_and_a_top_n_out_of_range_are_refused_before_anything_touches_the_gpu(q3, top_n):
    lib = q3.load_library()
    assert lib.q3_gen_logprobs(None, top_n) == -3
    assert (b"null engine" if top_n == 5 else b"out of range (-1..64)") in lib.q3_last_error()


def test_get_and_read_refuse_a_null_engine(q3):
    lib = q3.load_library()
    out = C.c_int(7)
    assert lib.q3_gen_logprobs_get(None, C.byref(out)) == -3 and out.value == 7
    recs = np.zeros(2, dtype=q3.SCORE_DTYPE)
    assert lib.q3_gen_logprobs_read(None, 0, 2, recs.ctypes.data_as(C.c_void_p), None, None) == -3
    assert b"null engine" in lib.q3_last_error()


class _Lib:
    """A library object that answers the three calls of section 2o as the engine of one finished q3_generate_many_* call would:
    `cap` records per request, of which the first `got` are filled -- record i of the call holds target i, max i + 0.5, sum 2 and
    argmax i, its tops are {-j, 100 i + j}, its rank i % 3 -- and zero bytes behind them"""

    def __init__(self, cap, got, top_n):
        self.cap, self.got, self.top_n, self.setting, self.calls = cap, got, top_n, -1, []
        total = sum(cap)
        self.recs = np.zeros(total, dtype=score_ref.DTYPE)
        self.top = np.zeros((total, max(top_n, 0)), dtype=tr.DTYPE)
        self.rank = np.zeros(total, dtype=np.int32)
        at = 0
        for c, g in zip(cap, got):
            for i in range(at, at + g):
                self.recs[i] = (i, i + 0.5, 2.0, i)
                self.top["logit"][i], self.top["index"][i] = -np.arange(max(top_n, 0), dtype=f32), 100 * i + np.arange(max(top_n, 0))
                self.rank[i] = i % 3
            at += c

    def q3_gen_logprobs(self, h, top_n):
        self.calls.append(("set", top_n))
        self.setting = top_n
        return 0

    def q3_gen_logprobs_get(self, h, out):
        out._obj.value = self.setting
        return 0

    def q3_gen_logprobs_read(self, h, first, count, recs, top, rank):
        self.calls.append(("read", first, count))
        if first + count > self.recs.size or (self.top_n > 0 and not top):
            return -3
        C.memmove(recs, self.recs[first:].ctypes.data, 16 * count)
        if self.top_n > 0:
            C.memmove(top, self.top[first:].ctypes.data, 8 * self.top_n * count)
            if rank:
                C.memmove(rank, self.rank[first:].ctypes.data, 4 * count)
        return 0

    def q3_last_error(self):
        return b"stub"


def _engine(q3, lib, vocab=4096):
    class NoEngine(q3.Transformer):                    # the wrappers' own work, over the stub library
        def __init__(self):
            self._config = type("C", (), {"vocab_size": vocab})()
            self._h = None
            self._lib = lib

        def __del__(self):
            pass
    return NoEngine()


@pytest.mark.parametrize("top_n", [0, 3])
def test_read_gen_logprobs_cuts_to_n_out(q3, top_n):
    cap, got = [3, 1, 4, 2], [2, 1, 0, 2]
    lib = _Lib(cap, got, top_n)
    t = _engine(q3, lib)
    t.set_gen_logprobs(top_n)
    assert lib.calls == [("set", top_n)] and t.get_gen_logprobs() == top_n
    t._gen_last = (cap, got, top_n)                    # what _generate_many leaves behind a call
    res = t.read_gen_logprobs()
    assert lib.calls[-1] == ("read", 0, sum(cap)) and len(res) == 4
    starts = [0, 3, 4, 8]
    for (recs, tops, ranks), s, g in zip(res, starts, got):
        assert recs.dtype == q3.SCORE_DTYPE and tops.dtype == q3.TOP_DTYPE and ranks.dtype == np.int32
        assert recs.shape == (g,) and tops.shape == (g, top_n) and ranks.shape == ((g,) if top_n else (0,))
        assert recs["argmax"].tolist() == list(range(s, s + g)) and recs["target"].tolist() == [float(i) for i in range(s, s + g)]
        if top_n:
            assert tops["index"].tolist() == [[100 * i + j for j in range(top_n)] for i in range(s, s + g)]
            assert ranks.tolist() == [i % 3 for i in range(s, s + g)]
    # the whole stretch of every request: zero bytes behind what it got
    full = t.read_gen_logprobs(cap)
    assert [x[0].size for x in full] == cap
    genlp_ref.assert_zero_behind(full, got, "stub")
    with pytest.raises(AssertionError):
        genlp_ref.assert_zero_behind(full, [1, 1, 0, 2], "stub")
    for bad in ([4, 1, 4, 2], [1, 1, 1], [-1, 0, 0, 0]):
        with pytest.raises(IndexError):
            t.read_gen_logprobs(bad)


def test_the_wrappers_refuse_before_they_call(q3):
    lib = _Lib([1], [1], 0)
    t = _engine(q3, lib, vocab=32)
    for top_n in (-2, 65, 33):
        with pytest.raises(ValueError):
            t.set_gen_logprobs(top_n)
    for top_n in (True, 2.0):
        with pytest.raises(TypeError):
            t.set_gen_logprobs(top_n)
    assert lib.calls == []
    # a read behind a call that ran without the setting: the library's refusal comes through
    t._gen_last = ([1], [1], -1)
    lib.top_n, lib.recs = 0, lib.recs[:0]
    with pytest.raises(IndexError):
        t.read_gen_logprobs()


class _Stub:
    """An engine for generation.generate_many: request r produces prompt[-1] + 1, + 2, ... (the stop loop ends a request at its
    stop token); read_gen_logprobs hands out, per token x, a record with target -1, max 0, sum 2 and argmax x, tops x + j with
    logits -j, rank x % 3.  It records every call it gets"""

    def __init__(self, ctx=64, fail=False):
        self.ctx, self.fail, self.setting, self.calls, self.prefix, self.rows, self.k_at_call = ctx, fail, -1, [], [], None, None

    def get_config(self):
        return type("C", (), {"seq_len": self.ctx, "vocab_size": 4096})()

    def get_gen_logprobs(self):
        return self.setting

    def set_gen_logprobs(self, k):
        self.calls.append(("set", k))
        self.setting = k

    def _run(self, name, prompts, n_new, stop=()):
        self.calls.append((name, self.setting))
        if self.fail:
            raise RuntimeError("the call failed")
        rows = []
        for p, n in zip(prompts, n_new):
            row = []
            for i in range(n):
                row.append(p[-1] + 1 + i)
                if row[-1] in stop:
                    break
            rows.append(row)
        self.rows, self.k_at_call = rows, self.setting
        return rows, "stats"

    def generate_many_greedy(self, prompts, n_new):
        return self._run("greedy", prompts, n_new)

    def generate_many_sampled(self, prompts, n_new, temperature, topp, seeds):
        return self._run("sampled", prompts, n_new)

    def generate_many_dense(self, prompts, n_new, sampler=None, dense_min=64):
        return self._run("dense", prompts, n_new) + ("dense stats",)

    def generate_many_stop(self, prompts, n_new, stop_tokens, sampler=None, raw=False):
        return self._run("stop", prompts, n_new, stop_tokens)

    def generate_many_prefix(self, suffixes, n_new, stop_tokens=(), sampler=None, raw=False):
        return self._run("prefix", suffixes, n_new, stop_tokens)

    def batch_prefix_get(self):
        return self.prefix

    def batch_prefix_set(self, tokens):
        self.prefix = list(tokens)

    def read_gen_logprobs(self, n_per_row=None):
        self.calls.append(("read", self.setting))
        k, out = self.k_at_call, []
        for row in self.rows:
            recs = np.zeros(len(row), dtype=score_ref.DTYPE)
            recs["target"], recs["sum"], recs["argmax"] = -1.0, 2.0, row
            tops = np.zeros((len(row), k), dtype=tr.DTYPE)
            for i, x in enumerate(row):
                tops["index"][i], tops["logit"][i] = x + np.arange(k), -np.arange(k, dtype=f32)
            out.append((recs, tops, np.array([x % 3 for x in row], dtype=np.int32) if k else np.zeros(0, dtype=np.int32)))
        return out


PROMPTS = [[1, 2, 10], [20], [5, 30]]


def test_generate_many_refuses_logprobs_out_of_range_before_any_library_call(q3):
    t = _Stub()
    for bad in (65, -1, True, 2.5):
        with pytest.raises(ValueError):
            q3.generate_many(t, PROMPTS, 4, logprobs=bad)
    assert t.calls == []


@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("kw,loop", [({}, "greedy"), (dict(sampler=(0.8, 0.9, 7)), "sampled"), (dict(dense_min=2), "dense"),
                                     (dict(stop_tokens=[12, 21], stop_on_device=True), "stop"), (dict(shared_prefix=[9, 9]), "prefix"),
                                     (dict(stop_tokens=[12, 21]), "greedy")])
def test_generate_many_with_logprobs_on_a_stub(q3, k, kw, loop):
    t = _Stub()
    t.setting = 7                                      # whatever the engine was set to is put back
    plain = q3.generate_many(_Stub(), PROMPTS, 4, **kw)
    assert len(plain) == 2
    rows, stats, lps = q3.generate_many(t, PROMPTS, 4, logprobs=k, **kw)
    assert (rows, stats) == plain
    assert t.calls == [("set", k), (loop, k), ("read", k), ("set", 7)] and t.setting == 7
    ln2 = np.log(2.0)
    assert len(lps) == len(rows)
    for row, (lp, ids, tlp, rank) in zip(rows, lps):
        n = len(row)                                   # cut to the row: at its stop token, whoever cut it
        assert [x.dtype for x in (lp, ids, tlp, rank)] == [np.float64, np.int32, np.float64, np.int32]
        assert lp.shape == (n,) and ids.shape == tlp.shape == (n, k) and rank.shape == ((n,) if k else (0,))
        assert np.array_equal(lp, np.full(n, -1.0 - ln2))
        if k:
            assert ids.tolist() == [[x + j for j in range(k)] for x in row] and rank.tolist() == [x % 3 for x in row]
            assert np.array_equal(tlp, np.tile(-np.arange(k) - ln2, (n, 1)))
    if "stop_tokens" in kw:
        assert rows == [[11, 12], [21], [31, 32, 33, 34]]


def test_generate_many_puts_the_setting_back_on_an_exception(q3):
    t = _Stub(fail=True)
    with pytest.raises(RuntimeError):
        q3.generate_many(t, PROMPTS, 4, logprobs=5)
    assert t.calls == [("set", 5), ("greedy", 5), ("set", -1)] and t.setting == -1


def test_a_request_the_context_leaves_no_room_for_gets_empty_arrays(q3):
    t = _Stub(ctx=3)                                   # the first prompt fills the context but for one token; none is left out
    rows, _, lps = q3.generate_many(t, [[1, 2, 3, 4], [7]], 2, logprobs=2)
    assert rows == [[], [8, 9]]
    assert lps[0][0].shape == (0,) and lps[0][1].shape == (0, 2) and lps[0][2].shape == (0, 2) and lps[0][3].shape == (0,)
    assert lps[1][1].tolist() == [[8, 9], [9, 10]]


def test_the_reference_helper_on_hand_made_rows():
    seqs, sf = genlp_ref.score_call([[1, 2], [7]], [[3, 4, 5], []])
    assert seqs == [[1, 2, 3, 4, 5], [7]] and sf == [2, 1]
    l = np.array([[1.0, 3.0, -2.0, 3.0], [0.5, 0.25, 0.0, -1.0]], dtype=f32)
    recs, tops, ranks = genlp_ref.from_logits(l, [3, 1], 2)
    assert recs["argmax"].tolist() == [3, 0] and ranks.tolist() == [0, 1] and tops["index"].tolist() == [[3, 1], [0, 1]]
    genlp_ref.assert_same([(recs, tops, ranks)], [(recs, tops, ranks)], [[3, 1]], 2, "itself")
    genlp_ref.assert_greedy_identities(recs[:1], ranks[:1], [3], "the argmax")
    with pytest.raises(AssertionError):
        genlp_ref.assert_greedy_identities(recs, ranks, [3, 1], "a token that is not the argmax")
    other = recs.copy()
    other["sum"][1] = np.nextafter(other["sum"][1], f32(9))
    with pytest.raises(AssertionError):
        genlp_ref.assert_same([(other, tops, ranks)], [(recs, tops, ranks)], [[3, 1]], 2, "one ulp in the sum")
