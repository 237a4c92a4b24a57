"""Guided decoding (include/qwen3_hip.h section 2r): what can be checked without a GPU -- the three entry points' place in the ABI
and their refusals in front of any GPU use, the host statement of the rule (tests/guide_ref.py) on hand-made vectors, the two
builders of guide.Automaton, and generate_many's handling of the engine's guide over a stub engine."""
import ctypes as C
import os

import numpy as np
import pytest

import bias_ref as br
import guide_ref as gr
import pen_ref as pr
from conftest import ROOT

f32 = np.float32
INF = float("inf")
SYMBOLS = ("q3_guide_set", "q3_guide_get", "q3_op_guide")


def test_the_symbols_are_exported_declared_and_listed(q3):
    header = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    lib = q3.load_library()
    for sym in SYMBOLS:
        assert sym in q3.EXPORTED_SYMBOLS and hasattr(lib, sym) and f"int {sym}(" in header
    # the section stands behind the last declaration of 2q; the ABI version stays
    assert header.index("int q3_guide_set(") > header.index("2r. (behind 2q") > header.index("int q3_op_logit_bias(")
    assert int(header.split("#define Q3_ABI_VERSION ")[1].split()[0]) == 1 and lib.q3_abi_version() == 1
    section = header[header.index("2r. (behind 2q"):]
    assert "#define Q3_GUIDE_MAX_STATES 4096" in section and q3.GUIDE_MAX_STATES == 4096 == q3.guide.GUIDE_MAX_STATES
    # it says what it leaves alone (2q's list), that the records stay on the raw row, that y_0 is under the rule, and defines the else branch
    for name in ("q3_batch_step_cols[_draw]", "section 2b", "verify paths", "single-stream decode", "q3_embed_many", "q3_choice_many", "q3_score_many",
                 "q3_score_top_many", "RAW ROW", "y_0 TOO", "fall-through", "else s_g", "0xFF800000", "ELSE BRANCH"):
        assert name in section, name


def guide_args(next, start, dtype=np.int16):
    nx = np.ascontiguousarray(next, dtype=dtype)
    st = np.ascontiguousarray(start, dtype=np.int32)
    return nx, st, nx.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.POINTER(C.c_int32))


GOOD = [[1, -1, 0], [-1, 1, 1]]          # two states over three tokens
REFUSED = {
    "4097 states": (np.zeros((4097, 2)), [0], b"at most 4096"),
    "no start state": (GOOD, [], b"no start"),
    "start == n_states": (GOOD, [0, 2], b"start[1]"),
    "start == -2": (GOOD, [-2], b"start[0]"),
    "an entry == n_states": ([[1, -1, 2], [-1, 1, 1]], [0], b"next[0][2]"),
    "an entry == -2": ([[1, -1, 0], [-2, 1, 1]], [0], b"next[1][0]"),
    "a state that allows no token": ([[1, -1, 0], [-1, -1, -1]], [0], b"state 1 allows no token"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_bad_guides_are_refused_before_the_engine_is_looked_at(q3, case):
    lib = q3.load_library()
    next, start, word = REFUSED[case]
    nx, st, pn, ps = guide_args(next, start)
    before = (nx.tobytes(), st.tobytes())
    assert lib.q3_guide_set(None, pn, nx.shape[0], nx.shape[1], ps, st.size) == -3
    assert word in lib.q3_last_error() and b"null engine" not in lib.q3_last_error(), lib.q3_last_error()
    assert (nx.tobytes(), st.tobytes()) == before


def test_null_arrays_and_the_vocabulary_are_refused_before_the_engine_is_looked_at(q3):
    lib = q3.load_library()
    nx, st, pn, ps = guide_args(GOOD, [1, -1, 0])
    # a guide that passes every check: the null engine is what is left to refuse; and turning it off on no engine
    assert lib.q3_guide_set(None, pn, 2, 3, ps, 3) == -3 and b"null engine" in lib.q3_last_error()
    assert lib.q3_guide_set(None, None, 0, 0, None, 0) == -3 and b"null engine" in lib.q3_last_error()
    # a null array with a non-zero count
    assert lib.q3_guide_set(None, None, 2, 3, ps, 3) == -3 and b"null next" in lib.q3_last_error()
    assert lib.q3_guide_set(None, pn, 2, 3, None, 3) == -3 and b"null start" in lib.q3_last_error()
    assert lib.q3_guide_set(None, None, 0, 0, None, 2) == -3 and b"null start" in lib.q3_last_error()
    # vocab == 0 and vocab >= 2^31 (nothing of the table is read)
    for vocab in (0, 2 ** 31, 2 ** 40):
        assert lib.q3_guide_set(None, pn, 2, vocab, ps, 3) == -3 and b"tokens" in lib.q3_last_error() and b"null engine" not in lib.q3_last_error()
    a, b = C.c_size_t(9), C.c_size_t(9)
    assert lib.q3_guide_get(None, C.byref(a), C.byref(b)) == -3 and (a.value, b.value) == (9, 9)
    assert nx.tolist() == GOOD and st.tolist() == [1, -1, 0]


def test_the_operator_refuses_what_q3_op_logit_bias_refuses_and_writes_nothing(q3):
    from test_bias_host import REFUSED as LISTS, table_args
    lib = q3.load_library()
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    row = np.zeros(8192, dtype=np.int16)
    pr_ = row.ctypes.data_as(C.c_void_p)
    for lists, modes, word in LISTS.values():
        if len(lists) != 1:
            continue
        flat, ent, n, m, k = table_args(q3, lists, modes)
        l, out, idx = np.zeros(8192, dtype=f32), np.full(8192, 7, dtype=f32), C.c_int32(-5)
        mode = 0 if modes is None else modes[0]
        assert lib.q3_op_guide(fp(l), l.size, pr_, ent, len(lists[0]), mode, 0, None, 0.0, 0.0, fp(out), C.byref(idx), 0) == -3
        assert word in lib.q3_last_error() and idx.value == -5 and (out == 7).all()
    l, out, idx = np.zeros(4, dtype=f32), np.full(4, 7, dtype=f32), C.c_int32(-5)
    one, e1, _, _, _ = table_args(q3, [[(3, 1.0, 0)]])
    for ll, rr, oo, ii, nn in ((None, pr_, out, idx, 4), (l, None, out, idx, 4), (l, pr_, None, idx, 4), (l, pr_, out, None, 4), (l, pr_, out, idx, 0)):
        rc = lib.q3_op_guide(fp(ll), nn, rr, e1, 1, 0, 0, None, 0.0, 0.0, fp(oo), None if ii is None else C.byref(ii), 0)
        assert rc == -3 and b"null argument" in lib.q3_last_error(), (ll is None, rr is None, oo is None, ii is None, nn)
    assert lib.q3_op_guide(fp(l), 3, pr_, e1, 1, 0, 0, None, 0.0, 0.0, fp(out), C.byref(idx), 0) == -3 and b"index out of range" in lib.q3_last_error()
    ban, eb, _, _, _ = table_args(q3, [[(t, -INF, 0) for t in range(4)]])
    assert lib.q3_op_guide(fp(l), 4, pr_, eb, 4, 0, 0, None, 0.0, 0.0, fp(out), C.byref(idx), 0) == -3 and b"bans every token" in lib.q3_last_error()
    assert lib.q3_op_guide(fp(l), 4, pr_, e1, 1, 0, 0, None, 2.5, 0.0, fp(out), C.byref(idx), 0) == -3 and b"out of range" in lib.q3_last_error()
    assert lib.q3_op_guide(fp(l), 4, pr_, None, 1, 0, 0, None, 0.0, 0.0, fp(out), C.byref(idx), 0) == -3 and b"null entries" in lib.q3_last_error()
    assert lib.q3_op_guide(fp(l), 4, pr_, e1, 1, 2, 0, None, 0.0, 0.0, fp(out), C.byref(idx), 0) == -3 and b"mode" in lib.q3_last_error()
    assert idx.value == -5 and (out == 7).all()
    # the Python wrapper checks before the library
    for kw in (dict(logits=l, next_row=[0, 0, 0]), dict(logits=l, next_row=[0, 0, 0, 2 ** 15]), dict(logits=l, next_row=[0.0] * 4),
               dict(logits=l, next_row=[0] * 4, entries=[(4, 1.0)]), dict(logits=l, next_row=[0] * 4, g=-1)):
        with pytest.raises(ValueError):
            q3.ops.guide(**kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def test_the_rule_on_hand_made_vectors():
    l = np.array([0.0, -0.0, 1.0, np.nan, np.inf, -np.inf, 3.5, -0.0], dtype=f32)
    l[3:4].view(np.uint32)[0] = 0x7fc12345                               # a NaN with a payload
    row = np.array([0, 5, -1, -1, 2, -1, 7, -1], dtype=np.int16)
    m = gr.mask(l, row)
    # a forbidden NaN becomes -inf; an allowed -0.0 keeps its bits; allowed entries keep theirs whatever the state number
    assert bits(m)[3] == 0xFF800000 and bits(m)[1] == 0x80000000
    assert (bits(m)[[0, 1, 4, 6]] == bits(l)[[0, 1, 4, 6]]).all() and (bits(m)[[2, 3, 5, 7]] == 0xFF800000).all()
    # an allowed NaN keeps its payload; an all-allowed row is the input
    assert bits(gr.mask(l, np.zeros(8, dtype=np.int16)))[3] == 0x7fc12345 and gr.mask(l, np.zeros(8)).tobytes() == l.tobytes()
    assert gr.rule(l, np.zeros(8)).tobytes() == l.tobytes()
    # mask, then bias, then penalty on one entry: 3.5 allowed, + 0.5, produced twice under (1.5, 0.5): 4.0 - 2.5
    c = np.zeros(8, dtype=np.uint32)
    c[6] = 2
    got = gr.rule(l, row, [(6, 0.5, 0), (2, 4.0, 0)], br.ADD, 0, c, 1.5, 0.5)
    assert got[6] == f32(f32(4.0) - f32(2.5)) and bits(got)[2] == 0xFF800000          # -inf + 4 is -inf: a forbidden token stays forbidden
    # the mask comes first: under ALLOW a token must be allowed by both
    got = gr.rule(l, row, [(6, 0.0, 0), (2, 0.0, 0)], br.ALLOW, 0)
    assert bits(got)[6] == bits(l)[6] and (bits(got)[[0, 1, 2, 3, 4, 5, 7]] == 0xFF800000).all()
    # a row with no finite entry: the largest key is V - 1
    assert pr.argmax_key(gr.rule(l, row, [(0, -INF, 0), (1, -INF, 0), (4, -INF, 0), (6, -INF, 0)], br.ADD, 0)) == 7


def test_the_state_step():
    next = np.array([[1, -1, 0], [-1, 1, 1]], dtype=np.int16)
    assert gr.step(next, 0, 0) == 1 and gr.step(next, 0, 2) == 0 and gr.step(next, 1, 1) == 1
    # a forbidden token: the state stays
    assert gr.step(next, 0, 1) == 0 and gr.step(next, 1, 0) == 1
    # an unguided request stays unguided
    assert gr.step(next, -1, 0) == -1
    assert gr.state_of(next, 0, [2, 1, 0, 0, 2]) == 1 and gr.state_of(next, -1, [0, 1]) == -1


def test_the_reference_loop_masks_from_the_first_output_on():
    """logits that depend on the last token alone: token t is followed by t + 1 (mod 4), token 5 is second best"""
    V = 6

    def row_of(seq):
        l = np.zeros(V, dtype=f32)
        l[(seq[-1] + 1) % 4] = 2.0
        l[5] = 1.0
        return l
    nodraw = lambda *a: pytest.fail("a greedy request draws nothing")
    free = [3, 0, 1, 2, 3, 0]
    assert gr.request(row_of, nodraw, [0, 1, 2], 6, None, -1)[0] == free
    # state 0 forbids 3 (y_0 is under the rule) and goes to 1 over 5; state 1 allows everything and stays
    next = np.array([[0, 0, 0, -1, 0, 1], [1] * 6], dtype=np.int16)
    assert gr.request(row_of, nodraw, [0, 1, 2], 6, next, 0)[0] == [5, 2, 3, 0, 1, 2]
    assert gr.request(row_of, nodraw, [0, 1, 2], 6, next, 1)[0] == free
    # a bias that bans state 0's only way out: nothing finite is left, V - 1 comes and the state stays
    only = np.array([[-1, -1, -1, -1, 1, -1], [1] * 6], dtype=np.int16)
    assert gr.request(row_of, nodraw, [0, 1, 2], 4, only, 0)[0] == [4, 1, 2, 3]
    assert gr.request(row_of, nodraw, [0, 1, 2], 4, only, 0, [(4, -INF, 2)], br.ADD)[0] == [5, 5, 4, 1]


# ---- the builders
def test_from_sequences(q3):
    A = q3.guide.Automaton
    seqs, V, eos = [[1, 2, 3], [1, 2, 4], [1, 5], [6]], 10, 9
    a = A.from_sequences(seqs, V, eos)
    # a shared prefix is shared: root, 1, 1 2, 1 2 3, 1 2 4, 1 5, 6, and the end state
    assert a.n_states == 8 and a.vocab_size == V and a.start == 0
    assert (a.next >= 0).any(axis=1).all()
    # walk accepts exactly the given sequences followed by eos (and eos again)
    import itertools
    accepted = set()
    for n in range(1, 4):
        for s in itertools.product([v for v in range(V) if v != eos], repeat=n):
            state, bad = a.walk(list(s) + [eos])
            if bad is None:
                accepted.add(s)
                assert a.walk(list(s) + [eos, eos, eos]) == (a.n_states - 1, None)
    assert accepted == {tuple(s) for s in seqs}
    assert a.walk([1, 2]) == (a.walk([1, 2])[0], None) and a.walk([1, 2, eos])[1] == 2 and a.walk([1, 3])[1] == 1 and a.walk([eos])[1] == 0
    assert a.walk([1, 2, 3, eos, 1])[1] == 4
    # the stay-put step of the rule
    assert a.step(0, 7) == 0 and a.step(0, 1) == int(a.next[0, 1])
    # a sequence that is a prefix of another: eos or the continuation
    b = A.from_sequences([[1], [1, 2]], V, eos)
    assert b.walk([1, eos])[1] is None and b.walk([1, 2, eos])[1] is None and b.walk([1, 2, 2])[1] == 2
    for bad in ([], [[]], [[1, V]], [[eos]]):
        with pytest.raises(ValueError):
            A.from_sequences(bad, V, eos)
    with pytest.raises(ValueError):
        A.from_sequences([[v] * 3 for v in range(2000)], 5000, 4999)              # 1 + 6000 + 1 states
    # what the constructor refuses
    for next, start in (([[-1, -1]], 0), ([[1, 0]], 0), ([[0, -2]], 0), ([[0, 0]], 1), ([[0, 0]], -1), (np.zeros((4097, 1), dtype=int), 0), ([0, 0], 0)):
        with pytest.raises(ValueError):
            A(next, start)
    with pytest.raises(TypeError):
        A([[0.0, 0.0]], 0)


def yes_no_dfa():
    """(yes|no) over bytes: 0 start, 1 y, 2 ye, 3 n, 4 accepting, 5 a dead state (no way on) behind 'x'"""
    trans = np.full((6, 256), -1, dtype=np.int32)
    trans[0, ord("y")], trans[1, ord("e")], trans[2, ord("s")] = 1, 2, 4
    trans[0, ord("n")], trans[3, ord("o")] = 3, 4
    trans[0, ord("x")] = 5
    return trans, 0, [4]


def test_from_byte_dfa(q3):
    A = q3.guide.Automaton
    trans, start, accepting = yes_no_dfa()
    vocab = [b"y", b"e", b"s", b"n", b"o", b"x", b"ye", b"es", b"no", b"yes!", b"", b"<eos>"]
    Y, E, S, N, O, X, YE, ES, NO, YESX, SPECIAL, EOS = range(12)
    a = A.from_byte_dfa(trans, start, accepting, vocab, EOS)
    allowed = lambda s: set(np.flatnonzero(a.next[s] >= 0).tolist())
    at = lambda toks: a.walk(toks)[0]
    assert a.start == 0 and allowed(0) == {Y, N, YE, NO}                     # x leads to a dead byte state; yes!, the special and eos are out
    # a token may cross several byte transitions
    assert a.walk([YE, S, EOS])[1] is None and a.walk([Y, ES, EOS])[1] is None and a.walk([NO, EOS])[1] is None and a.walk([Y, E, S, EOS, EOS])[1] is None
    assert at([YE]) == at([Y, E]) and at([YE, S]) == at([Y, ES]) == at([NO]) == at([N, O])
    assert allowed(at([Y])) == {E, ES} and allowed(at([YE])) == {S} and allowed(at([N])) == {O}
    # eos only behind yes / no, and it leads to a looping end state
    for s in range(a.n_states):
        assert (a.next[s, EOS] >= 0) == (s in (at([NO]), a.n_states - 1)), s
    assert allowed(at([NO])) == {EOS} and allowed(a.n_states - 1) == {EOS} and a.next[a.n_states - 1, EOS] == a.n_states - 1
    # yes! and the special are forbidden everywhere; a dead byte state never becomes a token state: start, y, ye, n, accepting, end
    assert (a.next[:, [YESX, SPECIAL, X]] < 0).all() and a.n_states == 6
    assert (a.next >= 0).any(axis=1).all()
    # a dead start state; too many states
    with pytest.raises(ValueError, match="dead"):
        A.from_byte_dfa(trans, 5, accepting, vocab, EOS)
    with pytest.raises(ValueError, match="dead"):
        A.from_byte_dfa(trans, 0, [], vocab, EOS)
    n = 5000                                                                 # a chain of 5000 byte states under one byte
    chain = np.full((n, 256), -1, dtype=np.int32)
    chain[np.arange(n - 1), ord("a")] = np.arange(1, n)
    with pytest.raises(ValueError, match="4096"):
        A.from_byte_dfa(chain, 0, [n - 1], [b"a", b"<eos>"], 1)
    chain[3999, ord("a")] = -1
    assert A.from_byte_dfa(chain[:4000], 0, [3999], [b"a", b"<eos>"], 1).n_states == 4001


# ---- generate_many(guide=...)
def test_the_merge_shifts_states_and_none_becomes_minus_one(q3):
    A, merge = q3.guide.Automaton, q3.guide.merge_guides
    a = A([[1, -1, 0], [-1, 1, 1]], 1)
    b = A([[0, 2, -1], [1, 1, 1], [-1, -1, 0]], 2)
    next, start = merge(a, 4)
    assert next.tolist() == a.next.tolist() and start == [1] and next.dtype == np.int16
    next, start = merge([b, None, a, b, None, a], 6)
    # distinct automata one behind the other in the order met, each once; -1 stays -1
    assert next.tolist() == [[0, 2, -1], [1, 1, 1], [-1, -1, 0], [4, -1, 3], [-1, 4, 4]] and next.dtype == np.int16
    assert start == [2, -1, 4, 2, -1, 4]
    with pytest.raises(ValueError):
        merge([a, b], 3)
    with pytest.raises(ValueError):
        merge([None, None], 2)
    with pytest.raises(ValueError):
        merge([a, A([[0, 0]], 0)], 2)                                         # another vocabulary
    with pytest.raises(TypeError):
        merge([a, [[0]]], 2)
    big = A(np.zeros((3000, 3), dtype=np.int16), 0)
    with pytest.raises(ValueError, match="4096"):
        merge([big, A(np.zeros((3000, 3), dtype=np.int16), 0)], 2)


class _Engine:
    """generate_many over a stub engine: the calls it makes about the guide"""

    def __init__(self, fail=False, with_guide=True):
        self.kept = (np.array([[0, 0]], dtype=np.int16), [0])
        self.guide, self.log, self.fail = self.kept, [], fail
        if with_guide:
            self.get_guide = lambda: self.guide
            self.set_guide = self._set_guide

    def _set_guide(self, next, start):
        self.log.append(("guide", None if next is None else np.asarray(next).tolist(), list(start)))
        self.guide = (next, start)

    def get_config(self):
        return type("C", (), {"seq_len": 8})()

    def generate_many_greedy(self, prompts, n_new):
        self.log.append(("run", len(prompts), list(self.guide[1])))
        if self.fail:
            raise RuntimeError("the call failed")
        return [[1] * n for n in n_new], None


def test_generate_many_sets_the_guide_for_the_call_and_puts_it_back(q3):
    A = q3.guide.Automaton
    a, b = A([[1, -1], [-1, 1]], 1), A([[0, 0]], 0)
    kept = ("guide", [[0, 0]], [0])
    t = _Engine()
    rows, _ = q3.generate_many(t, [[3, 4], [5]], 2, guide=a)
    assert rows == [[1, 1], [1, 1]] and t.log == [("guide", a.next.tolist(), [1]), ("run", 2, [1]), kept] and t.guide[0] is t.kept[0]
    # also when the call raises
    t = _Engine(fail=True)
    with pytest.raises(RuntimeError):
        q3.generate_many(t, [[3, 4]], 2, guide=[b])
    assert t.log == [("guide", [[0, 0]], [0]), ("run", 1, [0]), kept] and t.guide[0] is t.kept[0]
    # one per request, cut to the requests the context leaves room for: a prompt of 9 tokens in a context of 8 gets no row and no start state
    t = _Engine()
    rows, _ = q3.generate_many(t, [[3], [4] * 9, [5], [6]], 2, guide=[a, b, None, b])
    merged = [[1, -1], [-1, 1], [2, 2]]
    assert rows == [[1, 1], [], [1, 1], [1, 1]] and t.log == [("guide", merged, [1, -1, 2]), ("run", 3, [1, -1, 2]), kept]
    # a bad argument raises before anything is set
    t = _Engine()
    with pytest.raises(ValueError):
        q3.generate_many(t, [[3, 4]], 2, guide=[a, b])
    assert t.log == []


def test_without_the_argument_no_guide_call_is_made(q3):
    """the guide of set_guide simply holds; an engine stand-in that lacks the two methods serves the call as it did"""
    t = _Engine()
    q3.generate_many(t, [[3, 4]], 2)
    q3.generate_many(t, [[3, 4]], 2, guide=None)
    assert t.log == [("run", 1, [0]), ("run", 1, [0])]
    t = _Engine(with_guide=False)
    t.guide = (None, [])
    assert q3.generate_many(t, [[3, 4]], 2)[0] == [[1, 1]] and t.log == [("run", 1, [])]
