"""Logit bias, banned and allowed tokens, min_tokens (include/qwen3_hip.h section 2q): what can be checked without a GPU -- the three
entry points' place in the ABI and their refusals in front of any GPU use, the Python wrappers' checks, the host statement of the
rule (tests/bias_ref.py) on hand-made vectors, a triple that tells bias-then-penalty from penalty-then-bias, generate_many's merge of
its four arguments into lists, and its handling of the engine's table over a stub engine."""
import ctypes as C
import os

import numpy as np
import pytest

import bias_ref as br
import pen_ref as pr
from conftest import ROOT

f32 = np.float32
INF = float("inf")
SYMBOLS = ("q3_logit_bias_set", "q3_logit_bias_get", "q3_op_logit_bias")


def test_the_symbols_are_exported_declared_and_listed(q3):
    header = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    lib = q3.load_library()
    for sym in SYMBOLS:
        assert sym in q3.EXPORTED_SYMBOLS and hasattr(lib, sym) and f"int {sym}(" in header
    # the section stands behind the last declaration of 2p; the ABI version stays
    assert header.index("int q3_logit_bias_set(") > header.index("2q. (behind 2p") > header.index("int q3_op_penalize(")
    assert int(header.split("#define Q3_ABI_VERSION ")[1].split()[0]) == 1 and lib.q3_abi_version() == 1
    section = header[header.index("2q. (behind 2p"):]
    for name in ("typedef struct q3_bias_entry { int32_t token; float bias; uint32_t until; } q3_bias_entry;", "#define Q3_BIAS_MAX   4096",
                 "#define Q3_BIAS_ADD   0", "#define Q3_BIAS_ALLOW 1"):
        assert name in section, name
    # it says what it leaves alone, that the records stay on the raw row, what a banned token's probability is and what a NaN does
    for name in ("q3_batch_step_cols[_draw]", "section 2b", "verify paths", "single-stream decode", "q3_embed_many", "q3_choice_many", "q3_score_many",
                 "q3_score_top_many", "RAW ROW", "y_0 TOO", "probability exactly 0", "fall-through", "NaN"):
        assert name in section, name
    assert q3.BIAS_MAX == 4096 and (q3.BIAS_ADD, q3.BIAS_ALLOW) == (0, 1) and q3.BIAS_DTYPE.itemsize == 12


def table_args(q3, lists, modes=None):
    flat = np.zeros(sum(len(l) for l in lists), dtype=q3.BIAS_DTYPE)
    for i, e in enumerate(x for l in lists for x in l):
        flat[i] = e
    n = (C.c_size_t * max(len(lists), 1))(*[len(l) for l in lists])
    m = None if modes is None else (C.c_uint8 * len(modes))(*modes)
    return flat, flat.ctypes.data_as(C.c_void_p), n, m, len(lists)


REFUSED = {
    "nan": ([[(3, float("nan"), 0)]], None, b"bias"),
    "+inf": ([[(3, INF, 0)]], None, b"bias"),
    "100.0001": ([[(3, 100.0001, 0)]], None, b"bias"),
    "-100.0001": ([[(1, 0.0, 0)], [(3, -100.0001, 0)]], None, b"bias"),
    "a token twice": ([[(3, 1.0, 0), (5, 1.0, 0), (3, 2.0, 4)]], None, b"twice"),
    "a negative token": ([[(-1, 1.0, 0)]], None, b"negative"),
    "4097 entries": ([[(t, 0.5, 0) for t in range(4097)]], None, b"at most 4096"),
    "ALLOW of -inf only": ([[(3, -INF, 0), (4, -INF, 2)]], [1], b"ALLOW"),
    "an empty ALLOW list": ([[(3, 1.0, 0)], []], [0, 1], b"ALLOW"),
    "mode 2": ([[(3, 1.0, 0)]], [2], b"mode"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_bad_tables_are_refused_before_the_engine_is_looked_at(q3, case):
    lib = q3.load_library()
    lists, modes, word = REFUSED[case]
    flat, ent, n, m, k = table_args(q3, lists, modes)
    before = flat.tobytes()
    assert lib.q3_logit_bias_set(None, ent, n, m, k) == -3 and word in lib.q3_last_error() and b"null engine" not in lib.q3_last_error()
    assert flat.tobytes() == before
    if k == 1:
        # the operator entry refuses the same list, nothing written
        l, out, idx = np.zeros(8192, dtype=f32), np.full(8192, 7, dtype=f32), C.c_int32(-5)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        mode = 0 if modes is None else modes[0]
        assert lib.q3_op_logit_bias(fp(l), l.size, ent, len(lists[0]), mode, 0, None, 0.0, 0.0, fp(out), C.byref(idx), 0) == -3
        assert word in lib.q3_last_error() and idx.value == -5 and (out == 7).all()


def test_null_arguments_are_refused_before_anything_touches_the_gpu(q3):
    lib = q3.load_library()
    # a table that passes every check: the null engine is what is left to refuse; the ends of the range and -inf pass
    flat, ent, n, m, k = table_args(q3, [[(3, 100.0, 0), (9, -100.0, 0), (1, -INF, 7), (2, -0.0, 0)], [(5, 0.0, 0), (0, -INF, 0)]], [0, 1])
    assert lib.q3_logit_bias_set(None, ent, n, m, k) == -3 and b"null engine" in lib.q3_last_error()
    assert lib.q3_logit_bias_set(None, ent, n, None, k) == -3 and b"null engine" in lib.q3_last_error()
    assert lib.q3_logit_bias_set(None, None, None, None, 0) == -3 and b"null engine" in lib.q3_last_error()
    # a null array with a non-zero count
    assert lib.q3_logit_bias_set(None, None, n, m, k) == -3 and b"null entries" in lib.q3_last_error()
    assert lib.q3_logit_bias_set(None, ent, None, m, k) == -3 and b"null n_entries" in lib.q3_last_error()
    a, b = C.c_size_t(9), C.c_size_t(9)
    assert lib.q3_logit_bias_get(None, C.byref(a), C.byref(b)) == -3 and (a.value, b.value) == (9, 9)
    l, out, idx = np.zeros(4, dtype=f32), np.zeros(4, dtype=f32), C.c_int32(-5)
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    one, e1, _, _, _ = table_args(q3, [[(3, 1.0, 0)]])
    for ll, oo, ii, nn in ((None, out, idx, 4), (l, None, idx, 4), (l, out, None, 4), (l, out, idx, 0)):
        rc = lib.q3_op_logit_bias(fp(ll), nn, e1, 1, 0, 0, None, 0.0, 0.0, fp(oo), None if ii is None else C.byref(ii), 0)
        assert rc == -3 and b"null argument" in lib.q3_last_error(), (ll is None, oo is None, ii is None, nn)
    # what needs the vocabulary: a token >= n, an ADD list that bans every token; a penalty out of range; a null list with a count
    assert lib.q3_op_logit_bias(fp(l), 3, e1, 1, 0, 0, None, 0.0, 0.0, fp(out), C.byref(idx), 0) == -3 and b"index out of range" in lib.q3_last_error()
    ban, eb, _, _, _ = table_args(q3, [[(t, -INF, 0) for t in range(4)]])
    assert lib.q3_op_logit_bias(fp(l), 4, eb, 4, 0, 0, None, 0.0, 0.0, fp(out), C.byref(idx), 0) == -3 and b"bans every token" in lib.q3_last_error()
    assert lib.q3_op_logit_bias(fp(l), 4, e1, 1, 0, 0, None, 2.5, 0.0, fp(out), C.byref(idx), 0) == -3 and b"out of range" in lib.q3_last_error()
    assert lib.q3_op_logit_bias(fp(l), 4, None, 1, 0, 0, None, 0.0, 0.0, fp(out), C.byref(idx), 0) == -3 and b"null entries" in lib.q3_last_error()
    assert idx.value == -5


class _Lib:
    def __init__(self):
        self.calls = []

    def q3_logit_bias_set(self, h, entries, n, modes, n_lists):
        self.calls.append((n_lists, [n[i] for i in range(n_lists)], [modes[i] for i in range(n_lists)]))
        self.size = (n_lists, sum(n[i] for i in range(n_lists)))
        return 0

    def q3_logit_bias_get(self, h, n_lists, n_total):
        n_lists._obj.value, n_total._obj.value = self.size
        return 0


def _no_engine(q3):
    class NoEngine(q3.Transformer):
        def __init__(self):
            self._h, self._lib = None, _Lib()

        def __del__(self):
            pass
    return NoEngine()


def test_the_python_wrappers_check_before_the_library(q3):
    t = _no_engine(q3)
    l4 = np.zeros(4, dtype=f32)
    for lists, modes, _ in REFUSED.values():
        with pytest.raises(ValueError):
            t.set_logit_bias(lists, modes)
        if len(lists) == 1:
            with pytest.raises(ValueError):
                q3.ops.logit_bias(np.zeros(8192, dtype=f32), lists[0], 0 if modes is None else modes[0])
    for lists, modes in (([[(3, 1e39, 0)]], None), ([[(3, 1.0, -1)]], None), ([[(3, 1.0, 2 ** 32)]], None), ([[(2 ** 31, 1.0, 0)]], None),
                         ([[(3, 1.0, 0)]], [0, 1]), ([{3: 1.0}, {4: 1.0}], [0])):
        with pytest.raises(ValueError):
            t.set_logit_bias(lists, modes)
    for lists, modes in (({3: 1.0}, None), ("abc", None), (5, None), ([[("3", 1.0, 0)]], None), ([[(3, "1", 0)]], None), ([[(3, None)]], None),
                         ([[(3, True)]], None), ([[(True, 1.0)]], None), ([[(3, 1.0, 0.5)]], None), ([[(3,)]], None), ([[3]], None), ([[(3, 1.0)]], 1),
                         ([[(3, 1.0)]], ["0"]), ([[(3, 1.0)]], [True])):
        with pytest.raises(TypeError):
            t.set_logit_bias(lists, modes)
    assert t._lib.calls == []
    # a token outside the row, vectors of two lengths, an empty row, g out of range: the operator's own
    for kw in (dict(logits=l4, entries=[(4, 1.0)]), dict(logits=l4, entries=[(3, 1.0)], counts=np.zeros(3, dtype=np.uint32)),
               dict(logits=np.zeros(0, dtype=f32), entries=[]), dict(logits=l4, entries=[(3, 1.0)], g=-1),
               dict(logits=l4, entries=[(3, 1.0)], counts=np.zeros(4, dtype=np.uint32), presence=3.0)):
        with pytest.raises(ValueError):
            q3.ops.logit_bias(**kw)
    with pytest.raises(TypeError):
        q3.ops.logit_bias(l4, [(3, 1.0)], g=1.5)
    # what passes: dicts and tuples, any order, the table read back sorted; [] turns it off
    t.set_logit_bias([{7: 1, 3: -INF}, [(9, np.float32(0.5), 4), (2, 0.0)]], [0, 1])
    assert t._lib.calls == [(2, [2, 2], [0, 1])]
    assert t.get_logit_bias() == ([[(3, -INF, 0), (7, 1.0, 0)], [(2, 0.0, 0), (9, 0.5, 4)]], [0, 1])
    t.set_logit_bias([[]])
    assert t.get_logit_bias() == ([[]], [0])
    t.set_logit_bias([])
    assert t.get_logit_bias() == ([], []) and t._lib.calls[-1] == (0, [], [])


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def test_the_rule_on_hand_made_vectors():
    tiny = np.finfo(f32).tiny
    l = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, tiny / 4, -tiny / 4, np.finfo(f32).max, 3.5, np.nan, -0.0], dtype=f32)
    l[10:11].view(np.uint32)[0] = 0x7fc12345                             # a NaN with a payload
    # no entries under ADD: the same bits; under ALLOW every entry is -inf
    assert br.adjust(l, [], br.ADD, 0).tobytes() == l.tobytes()
    assert (bits(br.adjust(l, [], br.ALLOW, 0)) == 0xFF800000).all()
    # -0.0 with a bias of +-0 keeps its bits (-0.0 + 0.0 would be +0.0); with 1.0 it gives 1.0
    for z in (0.0, -0.0):
        for mode in (br.ADD, br.ALLOW):
            a = br.adjust(l, [(1, z, 0), (10, z, 0)], mode, 3)
            assert bits(a)[1] == 0x80000000 and bits(a)[10] == 0x7fc12345, (z, mode)
    assert bits(br.adjust(l, [(1, 1.0, 0)], br.ADD, 0))[1] == bits([1.0])[0]
    # a -inf bias gives -inf whatever stood there (but +inf, whose sum is a NaN: outside the standard)
    a = br.adjust(l, [(v, -INF, 0) for v in (0, 1, 2, 3, 6, 8, 9)], br.ADD, 0)
    assert (bits(a)[[0, 1, 2, 3, 6, 8, 9]] == 0xFF800000).all() and bits(a)[4] == bits(l)[4] and bits(a)[10] == bits(l)[10]
    assert np.isnan(br.adjust(l, [(4, -INF, 0)], br.ADD, 0)[4])
    # one rounding: max + 100 stays max, a subnormal plus 1 is 1
    a = br.adjust(l, [(8, 100.0, 0), (6, 1.0, 0), (2, -100.0, 0)], br.ADD, 0)
    assert a[8] == np.finfo(f32).max and a[6] == f32(1.0) and a[2] == f32(-99.0)
    # an unlisted entry under ALLOW becomes 0xFF800000, a listed one keeps its bits or takes its bias
    a = br.adjust(l, [(1, 0.0, 0), (9, 2.0, 0), (11, -0.0, 0)], br.ALLOW, 0)
    assert bits(a)[1] == 0x80000000 and a[9] == f32(5.5) and bits(a)[11] == 0x80000000
    assert (bits(a)[[0, 2, 3, 4, 5, 6, 7, 8, 10]] == 0xFF800000).all()
    # until: active below it, and an expired entry gives the same bits under both modes -- a listed token stays allowed
    for g, active in ((0, True), (2, True), (3, False), (4, False), (2 ** 31, False)):
        add, allow = br.adjust(l, [(9, -INF, 3), (2, 0.0, 0)], br.ADD, g), br.adjust(l, [(9, -INF, 3), (2, 0.0, 0)], br.ALLOW, g)
        assert bits(add)[9] == bits(allow)[9] == (0xFF800000 if active else bits(l)[9]), g
        assert bits(add)[2] == bits(allow)[2] == bits(l)[2] and bits(allow)[0] == 0xFF800000 and bits(add)[0] == bits(l)[0]
    # until == 0: always
    assert br.adjust(l, [(9, 1.0, 0)], br.ADD, 2 ** 32 - 1)[9] == f32(4.5)
    # the penalties on top: c > 0 takes presence + frequency * c off the ADJUSTED value, c == 0 keeps its bits
    c = np.zeros(l.size, dtype=np.uint32)
    c[[2, 9, 1]] = (1, 2, 0)
    got = br.rule(l, [(2, 3.0, 0), (1, 0.0, 0)], br.ALLOW, 0, c, 1.5, 0.5)
    assert got[2] == f32(4.0) - f32(2.0) and bits(got)[9] == 0xFF800000 and bits(got)[1] == 0x80000000
    # the argmax of designed rows: the last three of an all-equal row banned; a tie made by a bias goes to the higher index
    flat = np.full(9, 2.5, dtype=f32)
    assert pr.argmax_key(br.adjust(flat, [(8, -INF, 0), (7, -INF, 0), (6, -INF, 0)], br.ADD, 0)) == 5
    t = np.array([5.0, 0.0, 3.75, 0.0], dtype=f32)
    assert pr.argmax_key(br.adjust(t, [(0, -1.25, 0)], br.ADD, 0)) == 2 and pr.argmax_key(br.adjust(t, [(2, 1.25, 0)], br.ADD, 0)) == 2
    # a bias of 0 on the row's only -0.0 among +0.0s keeps the order: the last +0.0 wins, not the -0.0 behind it
    z = np.array([0.0, 0.0, 0.0, -0.0], dtype=f32)
    assert pr.argmax_key(br.adjust(z, [(3, 0.0, 0)], br.ADD, 0)) == 2 and pr.argmax_key(z) == 2


def test_bias_then_penalty_is_told_apart_from_penalty_then_bias():
    l, b, p = br.order_triple()
    one = np.array([l], dtype=f32)
    first = br.rule(one, [(0, b, 0)], br.ADD, 0, [1], p, 0.0)
    other = br.adjust(pr.penalize(one, [1], p, 0.0), [(0, b, 0)], br.ADD, 0)
    assert first.tobytes() != other.tobytes(), (l, b, p)
    assert 0.0 < b <= 100.0 and 0.0 < p <= 2.0
    # the rule's roundings, step by step: the sum, then the penalty off it
    assert first[0] == f32(f32(np.float64(f32(l)) + np.float64(f32(b))) - f32(p))


def test_the_reference_loop_applies_the_list_from_the_first_output_on():
    """logits that depend on the last token alone: token t is followed by t + 1 (mod 4)"""
    V = 6

    def row_of(seq):
        l = np.zeros(V, dtype=f32)
        l[(seq[-1] + 1) % 4] = 2.0
        l[5] = 1.0
        return l
    nodraw = lambda *a: pytest.fail("a greedy request draws nothing")
    assert br.request(row_of, nodraw, [0, 1, 2], 6, [], br.ADD)[0] == [3, 0, 1, 2, 3, 0]
    # y_0 is under the rule too: 3 banned, 5 (1.0) is the best left; behind 5 comes (5 + 1) % 4 = 2
    assert br.request(row_of, nodraw, [0, 1, 2], 6, [(3, -INF, 0)], br.ADD)[0] == [5, 2, 5, 2, 5, 2]
    # until counts the request's outputs, not its prompt: 3 banned for g < 2
    assert br.request(row_of, nodraw, [0, 1, 2], 6, [(3, -INF, 2)], br.ADD)[0] == [5, 2, 3, 0, 1, 2]
    # ALLOW {0, 5}: every token is one of them
    assert br.request(row_of, nodraw, [0, 1, 2], 5, [(0, 0.0, 0), (5, 0.0, 0)], br.ALLOW)[0] == [5, 5, 5, 5, 5]
    # min_tokens as an entry: stop token 0 cannot come before three tokens; free-running it ends the row at its second token
    assert br.request(row_of, nodraw, [0, 1, 2], 6, [], br.ADD, stop=(0,))[0] == [3, 0]
    assert br.request(row_of, nodraw, [0, 1, 2], 6, [(0, -INF, 3)], br.ADD, stop=(0,))[0] == [3, 5, 2, 3, 0]
    # bias first, penalties on top: 3 at 2 + 0.5, produced once -> 2.5 - 1.5 = 1.0, which ties with token 5 and loses to the higher index
    assert br.request(row_of, nodraw, [2], 3, [(3, 0.5, 0)], br.ADD, presence=1.5)[0] == [3, 0, 1]
    assert br.request(row_of, nodraw, [2, 3, 0, 1, 2], 2, [(3, 0.5, 0)], br.ADD, presence=1.5)[0] == [3, 0]


# ---- generate_many's four arguments
def test_the_merge_of_the_four_arguments(q3):
    m = q3.merge_logit_bias
    # single values: one list
    assert m(3) == ([[]], [0])
    assert m(3, {7: 1.5, 2: -3}) == ([[(2, -3, 0), (7, 1.5, 0)]], [0])
    assert m(3, None, [9, 4]) == ([[(4, -INF, 0), (9, -INF, 0)]], [0])
    assert m(3, {4: 2.0}, [4]) == ([[(4, -INF, 0)]], [0])                               # a ban wins over a bias
    assert m(3, {7: 1.5}, None, [7, 8]) == ([[(7, 1.5, 0), (8, 0.0, 0)]], [1])          # allowed: bias 0 unless logit_bias names it
    assert m(3, None, [8], [7, 8]) == ([[(7, 0.0, 0), (8, -INF, 0)]], [1])
    # min_tokens with stop tokens: (-inf, until min_tokens) per stop token
    assert m(3, None, None, None, 4, [11, 12]) == ([[(11, -INF, 4), (12, -INF, 4)]], [0])
    assert m(3, None, None, None, 4) == ([[]], [0]) and m(3, None, None, None, 0, [11]) == ([[]], [0])
    # ... skipped where the token is banned already, or unlisted under ALLOW; an allowed stop token opens at min_tokens
    assert m(3, None, [11], None, 4, [11, 12]) == ([[(11, -INF, 0), (12, -INF, 4)]], [0])
    assert m(3, None, None, [5, 12], 4, [11, 12]) == ([[(5, 0.0, 0), (12, -INF, 4)]], [1])
    # ... and a ValueError where the token also carries a finite bias
    with pytest.raises(ValueError):
        m(3, {11: 1.0}, None, None, 4, [11])
    with pytest.raises(ValueError):
        m(3, {11: 0.0}, None, [11, 5], 2, [11])
    assert m(3, {11: 1.0}, None, None, 0, [11]) == ([[(11, 1.0, 0)]], [0])
    # one value per request in any argument: one list per request
    assert m(2, [{1: 1.0}, None]) == ([[(1, 1.0, 0)], []], [0, 0])
    assert m(2, {1: 1.0}, [[3], []]) == ([[(1, 1.0, 0), (3, -INF, 0)], [(1, 1.0, 0)]], [0, 0])
    assert m(2, None, None, [[3, 4], [5]]) == ([[(3, 0.0, 0), (4, 0.0, 0)], [(5, 0.0, 0)]], [1, 1])
    assert m(2, None, None, None, [0, 3], [9]) == ([[], [(9, -INF, 3)]], [0, 0])
    for bad in (dict(logit_bias=[{1: 1.0}]), dict(banned_tokens=[[1], [2], [3]]), dict(allowed_tokens=[[1]]), dict(min_tokens=[1])):
        with pytest.raises(ValueError):
            m(2, **bad)
    with pytest.raises(ValueError):
        m(2, min_tokens=-1)
    for bad in (dict(logit_bias=[(1, 1.0), (2, 1.0)]), dict(min_tokens=1.5), dict(min_tokens=True)):
        with pytest.raises(TypeError):
            m(2, **bad)


class _Engine:
    """generate_many over a stub engine: the calls it makes about the table"""

    def __init__(self, fail=False, with_bias=True):
        self.pen, self.bias, self.log, self.fail = (0.0, 0.0), ([[(1, 0.5, 0)]], [0]), [], fail
        if with_bias:
            self.get_logit_bias = lambda: self.bias
            self.set_logit_bias = self._set_bias

    def _set_bias(self, lists, modes=None):
        self.log.append(("bias", lists, modes))
        self.bias = (lists, modes)

    def get_penalties(self):
        return self.pen

    def set_penalties(self, p, f):
        self.pen = (p, f)

    def get_config(self):
        return type("C", (), {"seq_len": 8})()

    def generate_many_greedy(self, prompts, n_new):
        self.log.append(("run", len(prompts), self.bias if hasattr(self, "set_logit_bias") else None))
        if self.fail:
            raise RuntimeError("the call failed")
        return [[1] * n for n in n_new], None

    def generate_many_stop(self, prompts, n_new, stop, sampler):
        self.log.append(("stop", len(prompts), self.bias))
        return [[1] * n for n in n_new], None


def test_generate_many_sets_the_table_for_the_call_and_puts_it_back(q3):
    kept = ([[(1, 0.5, 0)]], [0])
    t = _Engine()
    rows, _ = q3.generate_many(t, [[3, 4]], 2, banned_tokens=[7])
    table = ([[(7, -INF, 0)]], [0])
    assert rows == [[1, 1]] and t.log == [("bias",) + table, ("run", 1, table), ("bias",) + kept] and t.bias == kept
    t = _Engine(fail=True)
    with pytest.raises(RuntimeError):
        q3.generate_many(t, [[3, 4]], 2, logit_bias={5: 2.0})
    table = ([[(5, 2.0, 0)]], [0])
    assert t.log == [("bias",) + table, ("run", 1, table), ("bias",) + kept] and t.bias == kept
    # min_tokens through the stop loop
    t = _Engine()
    q3.generate_many(t, [[3, 4]], 4, stop_tokens=[6], stop_on_device=True, min_tokens=2)
    table = ([[(6, -INF, 2)]], [0])
    assert t.log == [("bias",) + table, ("stop", 1, table), ("bias",) + kept]
    # per-request lists follow the requests the context leaves room for: a prompt of 9 tokens in a context of 8 gets no row and no list
    t = _Engine()
    rows, _ = q3.generate_many(t, [[3], [4] * 9, [5]], 2, allowed_tokens=[[1], [2], [3]])
    table = ([[(1, 0.0, 0)], [(3, 0.0, 0)]], [1, 1])
    assert rows == [[1, 1], [], [1, 1]] and t.log == [("bias",) + table, ("run", 2, table), ("bias",) + kept]
    # a bad argument raises before anything is set
    t = _Engine()
    with pytest.raises(ValueError):
        q3.generate_many(t, [[3, 4]], 2, stop_tokens=[6], logit_bias={6: 1.0}, min_tokens=2)
    assert t.log == []


def test_without_the_arguments_no_table_call_is_made(q3):
    """the table of set_logit_bias simply holds; an engine stand-in that lacks the two methods serves the call as it did"""
    t = _Engine()
    q3.generate_many(t, [[3, 4]], 2)
    q3.generate_many(t, [[3, 4]], 2, presence_penalty=1.0, min_tokens=0)
    assert t.log == [("run", 1, t.bias), ("run", 1, t.bias)]
    t = _Engine(with_bias=False)
    assert q3.generate_many(t, [[3, 4]], 2)[0] == [[1, 1]] and t.log == [("run", 1, None)]
