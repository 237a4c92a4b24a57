"""Presence and frequency penalties (include/qwen3_hip.h section 2p): what can be checked without a GPU -- the three entry points'
place in the ABI and their refusals in front of any GPU use, the Python wrappers' checks, the host statement of the rule
(tests/pen_ref.py) on hand-made vectors, a (frequency, c, presence) triple that tells the rule from its fused form, and
generate_many's handling of the setting over a stub engine."""
import ctypes as C
import os

import numpy as np
import pytest

import pen_ref as pr
from conftest import ROOT

f32 = np.float32
SYMBOLS = ("q3_sampler_penalties", "q3_sampler_get_penalties", "q3_op_penalize")
BAD = [float("nan"), float("inf"), float("-inf"), 2.0001, -2.0001]


def test_the_symbols_are_exported_declared_and_listed(q3):
    header = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    lib = q3.load_library()
    for sym in SYMBOLS:
        assert sym in q3.EXPORTED_SYMBOLS and hasattr(lib, sym) and f"int {sym}(" in header
    # the section stands behind the last declaration of 2o; the ABI version stays
    assert header.index("int q3_sampler_penalties(") > header.index("2p. (behind 2o") > header.index("int q3_gen_logprobs_read(")
    assert int(header.split("#define Q3_ABI_VERSION ")[1].split()[0]) == 1 and lib.q3_abi_version() == 1
    section = header[header.index("2p. (behind 2o"):]
    # it says what it leaves alone, and that the records' greedy identities no longer hold
    for name in ("q3_batch_step_cols[_draw]", "section 2b", "verify paths", "single-stream decode", "NO LONGER HOLD", "RAW ROW"):
        assert name in section, name


@pytest.mark.parametrize("bad", BAD)
def test_values_out_of_range_are_refused_before_the_engine_is_looked_at(q3, bad):
    lib = q3.load_library()
    for p, f in ((bad, 0.0), (0.0, bad), (bad, bad)):
        assert lib.q3_sampler_penalties(None, p, f) == -3 and b"out of range" in lib.q3_last_error(), (p, f)
        l, c, out, idx = np.zeros(4, dtype=f32), np.zeros(4, dtype=np.uint32), np.full(4, 7, dtype=f32), C.c_int32(-5)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        assert lib.q3_op_penalize(fp(l), c.ctypes.data_as(C.POINTER(C.c_uint32)), 4, p, f, fp(out), C.byref(idx), 0) == -3
        assert b"out of range" in lib.q3_last_error() and idx.value == -5 and (out == 7).all()


def test_null_arguments_are_refused_before_anything_touches_the_gpu(q3):
    lib = q3.load_library()
    assert lib.q3_sampler_penalties(None, 1.5, 0.5) == -3 and b"null engine" in lib.q3_last_error()
    assert lib.q3_sampler_penalties(None, 2.0, -2.0) == -3 and b"null engine" in lib.q3_last_error()       # the ends of the range pass the first check
    p, f = C.c_float(9.0), C.c_float(9.0)
    assert lib.q3_sampler_get_penalties(None, C.byref(p), C.byref(f)) == -3 and (p.value, f.value) == (9.0, 9.0)
    l, c, out, idx = np.zeros(4, dtype=f32), np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=f32), C.c_int32(-5)
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    up = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))
    for ll, cc, oo, ii, n in ((None, c, out, idx, 4), (l, None, out, idx, 4), (l, c, None, idx, 4), (l, c, out, None, 4), (l, c, out, idx, 0)):
        rc = lib.q3_op_penalize(fp(ll), up(cc), n, 1.0, 0.5, fp(oo), None if ii is None else C.byref(ii), 0)
        assert rc == -3 and b"null argument" in lib.q3_last_error(), (ll is None, cc is None, oo is None, ii is None, n)


def test_the_python_wrappers_check_before_the_library(q3):
    calls = []

    class Lib:
        def q3_sampler_penalties(self, h, p, f):
            calls.append((p, f))
            return 0

    class NoEngine(q3.Transformer):
        def __init__(self):
            self._h, self._lib = None, Lib()

        def __del__(self):
            pass
    t = NoEngine()
    for bad in BAD + [1e39]:
        with pytest.raises(ValueError):
            t.set_penalties(bad, 0.0)
        with pytest.raises(ValueError):
            t.set_penalties(0.0, bad)
        with pytest.raises(ValueError):
            q3.ops.penalize(np.zeros(4, dtype=f32), np.zeros(4, dtype=np.uint32), bad, 0.0)
    for bad in ("1", None, True, [1.0]):
        with pytest.raises(TypeError):
            t.set_penalties(bad, 0.0)
        with pytest.raises(TypeError):
            t.set_penalties(0.0, bad)
    assert calls == []
    t.set_penalties(2, -2.0)
    t.set_penalties(np.float32(1.5), 0)
    assert calls == [(2.0, -2.0), (1.5, 0.0)]
    with pytest.raises(ValueError):
        q3.ops.penalize(np.zeros(4, dtype=f32), np.zeros(3, dtype=np.uint32), 1.0, 0.0)
    with pytest.raises(ValueError):
        q3.ops.penalize(np.zeros(0, dtype=f32), np.zeros(0, dtype=np.uint32), 1.0, 0.0)


def test_the_rule_on_hand_made_vectors():
    tiny = np.finfo(f32).tiny
    l = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, tiny / 4, -tiny / 4, np.finfo(f32).max, 3.5, np.nan], dtype=f32)
    l[-1:].view(np.uint32)[0] = 0x7fc12345                               # a NaN with a payload
    none = np.zeros(l.size, dtype=np.uint32)
    # c == 0: the same bits whatever the values, -0.0 and the payload included
    assert pr.penalize(l, none, 1.5, 0.5).tobytes() == l.tobytes()
    assert pr.penalize(l, none, -2.0, 2.0).view(np.uint32)[1] == 0x80000000
    # c > 0
    c = np.array([1, 1, 2, 65536, 1, 1, 1, 1, 1, 0, 1], dtype=np.uint32)
    got = pr.penalize(l, c, 1.5, 0.5)
    assert got[0] == f32(-2.0) and got[1] == f32(-2.0) and got[2] == f32(1.0 - 2.5) and got[3] == f32(-1.0) - f32(1.5 + 32768.0)
    assert got[4] == np.inf and got[5] == -np.inf and got[6] == f32(-2.0) and got[8] == np.finfo(f32).max
    assert got.view(np.uint32)[9] == l.view(np.uint32)[9] and np.isnan(got[10])
    # both values zero and c > 0: l - 0.0, which keeps every value (and -0.0: -0.0 - 0.0 = -0.0)
    assert pr.penalize(l[:10], c[:10], 0.0, 0.0).tobytes() == l[:10].tobytes()
    # a negative setting raises what was produced
    assert pr.penalize(np.array([1.0, 1.0], dtype=f32), [0, 3], -1.0, -0.25)[1] == f32(2.75)


def test_the_largest_key_argmax():
    assert pr.argmax_key(np.array([1.0, 3.0, 3.0, 2.0], dtype=f32)) == 2        # equal values: the higher index
    assert pr.argmax_key(np.array([-0.0, 0.0, -0.0], dtype=f32)) == 1           # +0.0 above -0.0 in the total order
    assert pr.argmax_key(np.full(7, -np.inf, dtype=f32)) == 6
    # a penalty that produces an exact tie between a penalised lower index and an unpenalised higher one: the higher wins
    l = np.array([5.0, 0.0, 3.75, 0.0], dtype=f32)
    d = f32(l[0] - l[2])
    row = pr.penalize(l, [1, 0, 0, 0], d, 0.0)
    assert row[0] == row[2] and pr.argmax_key(row) == 2 and pr.argmax_key(l) == 0


def test_a_fused_multiply_add_is_told_apart():
    fr, c, p = pr.fma_triple()
    one = np.zeros(1, dtype=f32)
    a, b = pr.penalize(one, [c], p, fr), pr.penalize_fma(one, [c], p, fr)
    assert a.tobytes() != b.tobytes(), (fr, c, p)
    assert 0.0 < fr <= 2.0 and 0.0 < p <= 2.0 and 0 < c < 2 ** 24
    # the rule's three roundings, step by step in Python floats rounded to float32
    m = f32(np.float64(f32(fr)) * np.float64(c))
    s = f32(np.float64(f32(p)) + np.float64(m))
    assert a[0] == f32(0.0) - s


def test_the_reference_loop_counts_only_what_the_request_produced():
    """logits that depend on the last token alone: token t is followed by t + 1 (mod 4) unless penalised away"""
    V = 6

    def row_of(seq):
        l = np.zeros(V, dtype=f32)
        l[(seq[-1] + 1) % 4] = 2.0
        l[5] = 1.0
        return l
    nodraw = lambda *a: pytest.fail("a greedy request draws nothing")
    free = pr.request(row_of, nodraw, [0, 1, 2], 6, 0.0, 0.0)
    assert free == ([3, 0, 1, 2, 3, 0], 0, 2, False)
    # the prompt's 0, 1, 2 do not count: 3, 0, 1, 2 pass unpenalised, then 3 (count 1) stands at 2 - 1.5 = 0.5 below token 5
    pen = pr.request(row_of, nodraw, [0, 1, 2], 6, 1.5, 0.0)
    assert pen[0] == [3, 0, 1, 2, 5, 2] and pen[3] and pen[2] == 2
    assert pr.request(row_of, nodraw, [0, 1, 2], 6, 1.5, 0.0, stop=(1,))[0] == [3, 0, 1]


class _Engine:
    """generate_many over a stub engine: the calls it makes about the setting"""

    def __init__(self, fail=False):
        self.pen, self.log, self.fail = (0.25, 0.0), [], fail

    def get_penalties(self):
        return self.pen

    def set_penalties(self, p, f):
        self.log.append(("set", p, f))
        self.pen = (p, f)

    def get_config(self):
        return type("C", (), {"seq_len": 64})()

    def batch_context(self):
        return 64

    def generate_many_greedy(self, prompts, n_new):
        self.log.append(("run", self.pen))
        if self.fail:
            raise RuntimeError("the call failed")
        return [[1] * n for n in n_new], None


def test_generate_many_sets_the_penalties_for_the_call_and_puts_them_back(q3):
    t = _Engine()
    try:
        rows, _ = q3.generate_many(t, [[3, 4]], 2, presence_penalty=1.5, frequency_penalty=0.5)
    except AttributeError as e:                                          # the stub lacks something generate_many asks its engine
        pytest.fail(f"the stub engine is incomplete: {e}")
    assert rows == [[1, 1]]
    assert t.log == [("set", 1.5, 0.5), ("run", (1.5, 0.5)), ("set", 0.25, 0.0)] and t.pen == (0.25, 0.0)
    t = _Engine(fail=True)
    with pytest.raises(RuntimeError):
        q3.generate_many(t, [[3, 4]], 2, presence_penalty=1.0)
    assert t.log == [("set", 1.0, 0.0), ("run", (1.0, 0.0)), ("set", 0.25, 0.0)] and t.pen == (0.25, 0.0)
    # without the arguments the call runs at (0, 0): the setting of the call, not the engine's
    t = _Engine()
    q3.generate_many(t, [[3, 4]], 2)
    assert t.log == [("set", 0.0, 0.0), ("run", (0.0, 0.0)), ("set", 0.25, 0.0)]
