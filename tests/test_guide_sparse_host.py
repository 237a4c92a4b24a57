"""Sparse guides (include/qwen3_hip.h section 2s): what can be checked without a GPU -- the three entry points' place in the ABI,
the refusals of guide_sparse_check in front of the engine, guide.SparseAutomaton against its dense twin, merge_guides over both
forms, the regular-expression compiler against re.fullmatch on every string of a small alphabet, and the lift of a byte DFA to
tokens at the edge of a UTF-8 code point.  There is no tolerance: tables are compared as integers."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("q3_guide_set_sparse", "q3_guide_get_sparse", "q3_op_guide_sparse")


def test_the_symbols_are_exported_declared_and_placed_behind_2r(q3):
    header = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    lib = q3.load_library()
    for sym in SYMBOLS:
        assert sym in q3.EXPORTED_SYMBOLS and hasattr(lib, sym) and f"int {sym}(" in header
    assert header.index("int q3_guide_set_sparse(") > header.index("2s. (behind 2r") > header.index("int q3_op_guide(")
    assert int(header.split("#define Q3_ABI_VERSION ")[1].split()[0]) == 1 and lib.q3_abi_version() == 1
    section = header[header.index("2s. (behind 2r"):]
    assert "#define Q3_GUIDE_SPARSE_MAX_STATES 1048576" in section and q3.GUIDE_SPARSE_MAX_STATES == 1048576 == q3.guide.GUIDE_SPARSE_MAX_STATES
    assert "#define Q3_GUIDE_SPARSE_MAX_EDGES 134217728" in section and q3.GUIDE_SPARSE_MAX_EDGES == 134217728 == q3.guide.GUIDE_SPARSE_MAX_EDGES
    assert "typedef struct q3_guide_edge { int32_t token; int32_t next; } q3_guide_edge;" in section and q3.EDGE_DTYPE.itemsize == 8
    for name in ("UNCHANGED", "0xFF800000", "RAW ROW", "ONE GUIDE HOLDS AT A TIME", "clears both", "dflt[s]", "strictly", "q3_score_top_many"):
        assert name in section, name


def sparse_args(q3, dflt, off, edges, start):
    d = np.ascontiguousarray(dflt, dtype=np.int32)
    o = np.ascontiguousarray(off, dtype=np.uint32)
    e = np.array([tuple(x) for x in edges], dtype=q3.EDGE_DTYPE)
    s = np.ascontiguousarray(start, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return (d, o, e, s), (p(d), p(o), p(e), d.size, e.size), (s.ctypes.data_as(C.POINTER(C.c_int32)), s.size)


# two states over three tokens: state 0 allows token 0 (to 1) and token 2 (stays); state 1 allows everything but token 0
GOOD = ([-1, 1], [0, 2, 3], [(0, 1), (2, 0), (0, -1)], [0])
REFUSED = {
    "row_off[0] != 0": (([-1, 1], [1, 2, 3], GOOD[2], [0]), 3, b"row_off[0]"),
    "offsets that decrease": (([-1, 1], [0, 3, 2], GOOD[2], [0]), 3, b"below row_off"),
    "offsets that do not end at n_edges": (([-1, 1], [0, 2, 2], GOOD[2], [0]), 3, b"does not end"),
    "a token == vocab": (([-1, 1], [0, 2, 3], [(0, 1), (3, 0), (0, -1)], [0]), 3, b"edges[1].token"),
    "a token == -1": (([-1, 1], [0, 2, 3], [(-1, 1), (2, 0), (0, -1)], [0]), 3, b"edges[0].token"),
    "tokens that repeat": (([-1, 1], [0, 2, 3], [(2, 1), (2, 0), (0, -1)], [0]), 3, b"ascend strictly"),
    "tokens that descend": (([-1, 1], [0, 2, 3], [(2, 1), (0, 0), (0, -1)], [0]), 3, b"ascend strictly"),
    "a next == n_states": (([-1, 1], [0, 2, 3], [(0, 2), (2, 0), (0, -1)], [0]), 3, b"edges[0].next"),
    "a next == -2": (([-1, 1], [0, 2, 3], [(0, 1), (2, 0), (0, -2)], [0]), 3, b"edges[2].next"),
    "a dflt == n_states": (([-1, 2], GOOD[1], GOOD[2], [0]), 3, b"dflt[1]"),
    "a dflt == -2": (([-2, 1], GOOD[1], GOOD[2], [0]), 3, b"dflt[0]"),
    "start == n_states": ((GOOD[0], GOOD[1], GOOD[2], [0, 2]), 3, b"start[1]"),
    "start == -2": ((GOOD[0], GOOD[1], GOOD[2], [-2]), 3, b"start[0]"),
    "no start state": ((GOOD[0], GOOD[1], GOOD[2], []), 3, b"no start"),
    "a state of -1 with edges that all forbid": (([-1, 1], [0, 2, 3], [(0, -1), (2, -1), (0, -1)], [0]), 3, b"state 0 allows no token"),
    "a state of -1 without edges": (([1, -1], [0, 3, 3], [(0, 1), (1, 0), (2, -1)], [0]), 3, b"state 1 allows no token"),
    "a state whose every token is listed as forbidden": (([1, 1], [0, 3, 3], [(0, -1), (1, -1), (2, -1)], [0]), 3, b"state 0 allows no token"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_bad_guides_are_refused_before_the_engine_is_looked_at(q3, case):
    lib = q3.load_library()
    guide, vocab, word = REFUSED[case]
    kept, (pd, po, pe, ns, ne), (ps, nst) = sparse_args(q3, *guide)
    before = [a.tobytes() for a in kept]
    assert lib.q3_guide_set_sparse(None, pd, po, pe, ns, ne, vocab, ps, nst) == -3
    assert word in lib.q3_last_error() and b"null engine" not in lib.q3_last_error(), lib.q3_last_error()
    assert [a.tobytes() for a in kept] == before


def test_null_arrays_the_caps_and_the_vocabulary_are_refused_before_the_engine_is_looked_at(q3):
    lib = q3.load_library()
    kept, (pd, po, pe, ns, ne), (ps, nst) = sparse_args(q3, *GOOD)
    # a guide that passes every check: the null engine is what is left to refuse; and turning it off on no engine
    assert lib.q3_guide_set_sparse(None, pd, po, pe, ns, ne, 3, ps, nst) == -3 and b"null engine" in lib.q3_last_error()
    assert lib.q3_guide_set_sparse(None, None, None, None, 0, 0, 0, None, 0) == -3 and b"null engine" in lib.q3_last_error()
    for args, word in (((None, po, pe, ns, ne, 3, ps, nst), b"null dflt"), ((pd, None, pe, ns, ne, 3, ps, nst), b"null row_off"),
                       ((pd, po, None, ns, ne, 3, ps, nst), b"null edges"), ((pd, po, pe, ns, ne, 3, None, nst), b"null start"),
                       ((None, None, None, 0, 0, 0, None, 2), b"null start"), ((None, None, pe, 0, 3, 3, None, 0), b"no state")):
        assert lib.q3_guide_set_sparse(None, *args) == -3 and word in lib.q3_last_error(), word
        assert b"null engine" not in lib.q3_last_error()
    # the caps, refused on the counts alone: nothing of the arrays is read
    assert lib.q3_guide_set_sparse(None, pd, po, pe, 2 ** 20 + 1, ne, 3, ps, nst) == -3 and b"at most 1048576" in lib.q3_last_error()
    assert lib.q3_guide_set_sparse(None, pd, po, pe, ns, 2 ** 27 + 1, 3, ps, nst) == -3 and b"at most 134217728" in lib.q3_last_error()
    for vocab in (0, 2 ** 31, 2 ** 40):
        assert lib.q3_guide_set_sparse(None, pd, po, pe, ns, ne, vocab, ps, nst) == -3 and b"tokens" in lib.q3_last_error()
        assert b"null engine" not in lib.q3_last_error()
    a, b, c = C.c_size_t(9), C.c_size_t(9), C.c_size_t(9)
    assert lib.q3_guide_get_sparse(None, C.byref(a), C.byref(b), C.byref(c)) == -3 and (a.value, b.value, c.value) == (9, 9, 9)


def test_the_operator_refuses_bad_edges_and_writes_nothing(q3):
    lib = q3.load_library()
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    l, out, idx = np.zeros(4, dtype=np.float32), np.full(4, 7, dtype=np.float32), C.c_int32(-5)
    edges = lambda *e: np.array(list(e), dtype=q3.EDGE_DTYPE)
    call = lambda dflt, e, n=None, lp=l: lib.q3_op_guide_sparse(fp(lp), 4, dflt, None if e is None else e.ctypes.data_as(C.c_void_p),
                                                                 (0 if e is None else e.size) if n is None else n, None, 0, 0, 0, None, 0.0, 0.0,
                                                                 fp(out), C.byref(idx), 0)
    for dflt, e, n, word in ((0, None, 2, b"null edges"), (0, edges((4, 0)), None, b"edges[0].token"), (0, edges((-1, 0)), None, b"edges[0].token"),
                             (0, edges((1, 0), (1, 0)), None, b"ascend strictly"), (0, edges((1, -2)), None, b"edges[0].next"),
                             (0, edges((1, 2 ** 20)), None, b"edges[0].next"), (-2, None, None, b"dflt"), (2 ** 20, None, None, b"dflt"),
                             (0, edges((0, 0), (1, 0), (2, 0), (3, 0), (3, 0)), None, b"5 edges over 4 logits")):
        assert call(dflt, e, n) == -3 and word in lib.q3_last_error(), (word, lib.q3_last_error())
    assert call(0, None, lp=None) == -3 and b"null argument" in lib.q3_last_error()
    assert lib.q3_op_guide_sparse(fp(l), 4, 0, None, 0, None, 0, 2, 0, None, 0.0, 0.0, fp(out), C.byref(idx), 0) == -3 and b"mode" in lib.q3_last_error()
    assert lib.q3_op_guide_sparse(fp(l), 4, 0, None, 0, None, 1, 0, 0, None, 0.0, 0.0, fp(out), C.byref(idx), 0) == -3 and b"null entries" in lib.q3_last_error()
    assert lib.q3_op_guide_sparse(fp(l), 4, 0, None, 0, None, 0, 0, 0, None, 2.5, 0.0, fp(out), C.byref(idx), 0) == -3 and b"out of range" in lib.q3_last_error()
    assert idx.value == -5 and (out == 7).all()
    for kw in (dict(default=0, tokens=[1, 1], targets=[0, 0]), dict(default=0, tokens=[4], targets=[0]), dict(default=0, tokens=[1], targets=[0, 1]),
               dict(default=-2), dict(default=0, tokens=[1], targets=[2 ** 20]), dict(default=0, g=-1)):
        with pytest.raises(ValueError):
            q3.ops.guide_sparse(l, **kw)


# ---- SparseAutomaton against its dense twin
def random_automaton(q3, rng, S, V):
    next = rng.integers(-1, S, (S, V)).astype(np.int16)
    next[np.arange(S), rng.integers(0, V, S)] = rng.integers(0, S, S)         # no dead state
    return q3.Automaton(next, int(rng.integers(0, S)))


@pytest.mark.parametrize("V", [1, 3, 2000])
def test_from_dense_gives_every_row_back(q3, V):
    rng = np.random.default_rng(50 + V)
    SA = q3.SparseAutomaton
    for S in (1, 2, 7, 40):
        a = random_automaton(q3, rng, S, V)
        if S >= 2:
            a.next[0] = 1                                                    # a row with all entries equal
            a.next[1] = -1                                                   # a row of all -1 but one
            a.next[1, V - 1] = 0
        s = SA.from_dense(a)
        assert (s.n_states, s.vocab_size, s.start) == (a.n_states, V, a.start)
        for st in range(S):
            row = s.row(st)
            assert row.dtype == np.int32 and np.array_equal(row, a.next[st]), (S, st)
            # the default is the row's most frequent value: no more edges than entries that differ from it
            assert int(s.offsets[st + 1] - s.offsets[st]) == V - np.bincount(a.next[st].astype(np.int64) + 1).max()
        if S >= 2:
            assert s.default[0] == 1 and s.offsets[1] == 0 and s.default[1] == (-1 if V > 2 else s.default[1])
        assert np.array_equal(s.to_dense().next, a.next) and s.to_dense().start == a.start
        for _ in range(50):
            st, tok = int(rng.integers(0, S)), int(rng.integers(0, V))
            assert s.step(st, tok) == a.step(st, tok)
        toks = rng.integers(0, V, 12).tolist()
        assert s.walk(toks) == a.walk(toks)


def test_the_constructor_refuses_what_the_library_refuses(q3):
    SA = q3.SparseAutomaton
    ok = SA([-1, 1], [0, 2, 3], [0, 2, 0], [1, 0, -1], 0, 3)
    assert ok.n_states == 2 and ok.n_edges == 3 and ok.row(0).tolist() == [1, -1, 0] and ok.row(1).tolist() == [-1, 1, 1]
    for guide, vocab, _ in REFUSED.values():
        dflt, off, edges, start = guide
        if len(start) != 1 or not 0 <= start[0] < 2:
            continue
        with pytest.raises(ValueError):
            SA(dflt, off, [t for t, _ in edges], [n for _, n in edges], start[0], vocab)
    for args in (([0], [0, 0], [], [], 1, 3), ([0], [0, 0], [], [], -1, 3), ([0], [0, 0], [], [], 0, None), ([0], [0, 0], [], [], 0, 0), ([], [0], [], [], 0, 3)):
        with pytest.raises(ValueError):
            SA(*args)
    with pytest.raises(TypeError):
        SA([0.5], [0, 0], [], [], 0, 3)
    # above 4,096 states there is no dense twin
    big = SA(np.zeros(5000, dtype=np.int32), np.zeros(5001, dtype=np.int64), [], [], 0, 3)
    assert big.n_states == 5000 and big.row(4999).tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="4096"):
        big.to_dense()


def test_from_sequences_equals_its_dense_twin(q3):
    A, SA = q3.Automaton, q3.SparseAutomaton
    for seqs, V, eos in (([[1, 2, 3], [1, 2, 4], [1, 5], [6]], 10, 9), ([[1], [1, 2]], 10, 9), ([[0]], 2, 1), ([[3, 3, 3], [3, 3]], 5, 0)):
        s, a = SA.from_sequences(seqs, V, eos), A.from_sequences(seqs, V, eos)
        assert np.array_equal(s.to_dense().next, a.next) and s.start == a.start == 0
        assert (s.default == -1).all()
    for bad in ([], [[]], [[1, 10]], [[9]]):
        with pytest.raises(ValueError):
            SA.from_sequences(bad, 10, 9)
    # a trie the dense form refuses: 6,002 states, and no dense row on the way (V = 2^30 would not fit one)
    s = SA.from_sequences([[v] * 3 for v in range(2000)], 2 ** 30, 2 ** 30 - 1)
    assert s.n_states == 6002 and s.n_edges == 6000 + 2000 + 1 and s.walk([7, 7, 7, 2 ** 30 - 1]) == (6001, None) and s.walk([7, 8])[1] == 1


VOCAB = [bytes([b]) for b in range(256)] + [b"ye", b"es", b"no", b"yes!", b"", b"12", b"a1", b"\xc3", b"\xa9x", "é".encode(), "日本".encode(),
                                             "日".encode()[:2], b"x\xe6", b"<eos>"]
EOS = len(VOCAB) - 1


@pytest.mark.parametrize("pattern", [r"yes|no", r"[a-c]+\d{1,3}", r".*", r"(12|a1)*x", r"[^a]+", r"é\d?", r"\w+( \w+)*"])
def test_from_byte_dfa_equals_its_dense_twin(q3, pattern):
    A, SA = q3.Automaton, q3.SparseAutomaton
    dfa = q3.regex_dfa(pattern)
    s, a = SA.from_byte_dfa(*dfa, VOCAB, EOS), A.from_byte_dfa(*dfa, VOCAB, EOS)
    assert np.array_equal(s.to_dense().next, a.next) and s.start == a.start == 0
    f = SA.from_regex(pattern, VOCAB, EOS)
    assert all(np.array_equal(getattr(f, k), getattr(s, k)) for k in ("default", "offsets", "tokens", "targets"))


def test_from_byte_dfa_is_not_bound_by_the_dense_cap(q3):
    n = 5000
    chain = np.full((n, 256), -1, dtype=np.int32)
    chain[np.arange(n - 1), ord("a")] = np.arange(1, n)
    s = q3.SparseAutomaton.from_byte_dfa(chain, 0, [n - 1], [b"a", b"<eos>", b"aaa"], 1)
    assert s.n_states == n + 1 and s.walk([0] * (n - 1) + [1])[1] is None and s.walk([2] * 1666 + [0, 1])[1] is None and s.walk([0, 1])[1] == 1
    with pytest.raises(ValueError, match="dead"):
        q3.SparseAutomaton.from_byte_dfa(chain, 0, [], [b"a", b"<eos>"], 1)


def test_the_merge_takes_sparse_mixed_and_none(q3):
    A, SA, merge = q3.Automaton, q3.SparseAutomaton, q3.guide.merge_guides
    a = A([[1, -1, 0], [-1, 1, 1]], 1)
    b = SA.from_dense(A([[0, 2, -1], [1, 1, 1], [-1, -1, 0]], 2))
    # one sparse automaton for all
    m, start = merge(b, 4)
    assert m is b and start == [2]
    # sparse alone, with None
    m, start = merge([b, None, b], 3)
    assert isinstance(m, SA) and start == [2, -1, 2] and [m.row(s).tolist() for s in range(3)] == [[0, 2, -1], [1, 1, 1], [-1, -1, 0]]
    # mixed: the dense one enters through from_dense; distinct automata one behind the other in the order met, each once
    m, start = merge([b, None, a, b, None, a], 6)
    assert isinstance(m, SA) and m.n_states == 5 and start == [2, -1, 4, 2, -1, 4]
    assert [m.row(s).tolist() for s in range(5)] == [[0, 2, -1], [1, 1, 1], [-1, -1, 0], [4, -1, 3], [-1, 4, 4]]
    assert m.n_edges == b.n_edges + SA.from_dense(a).n_edges
    # dense alone: as ever
    next, start = merge([a, None], 2)
    assert isinstance(next, np.ndarray) and next.dtype == np.int16 and start == [1, -1]
    # sparse automata are not bound by the dense cap
    big = SA(np.zeros(3000, dtype=np.int32), np.zeros(3001, dtype=np.int64), [], [], 0, 3)
    m, start = merge([big, SA(np.zeros(3000, dtype=np.int32), np.zeros(3001, dtype=np.int64), [], [], 5, 3)], 2)
    assert m.n_states == 6000 and start == [0, 3005] and m.default[3000] == 3000
    with pytest.raises(ValueError):
        merge([b, SA([0], [0, 0], [], [], 0, 2)], 2)                           # another vocabulary
    with pytest.raises(ValueError):
        merge([b, a], 3)
    with pytest.raises(TypeError):
        merge([b, [[0]]], 2)


class _Engine:
    """generate_many over a stub engine: the calls it makes about the guide of either form"""

    def __init__(self, sparse_kept=None):
        self.dense, self.sparse, self.log = (None, []), sparse_kept or (None, None, None, None, []), []
        if sparse_kept is None:
            self.dense = (np.array([[0, 0]], dtype=np.int16), [0])

    def get_guide(self):
        return self.dense

    def get_guide_sparse(self):
        return self.sparse

    def set_guide(self, next, start):
        self.log.append(("dense", None if next is None else np.asarray(next).tolist(), list(start)))
        self.dense, self.sparse = (next, start), (None, None, None, None, [])

    def set_guide_sparse(self, default, offsets, tokens, targets, start):
        self.log.append(("sparse", np.asarray(default).tolist(), list(start)))
        self.dense, self.sparse = (None, []), (default, offsets, tokens, targets, start)

    def get_config(self):
        return type("C", (), {"seq_len": 8})()

    def generate_many_greedy(self, prompts, n_new):
        self.log.append(("run", len(prompts)))
        return [[1] * n for n in n_new], None


def test_generate_many_sets_either_form_and_puts_the_previous_one_back(q3):
    A, SA = q3.Automaton, q3.SparseAutomaton
    a = A([[1, -1], [-1, 1]], 1)
    b = SA.from_dense(A([[0, 0]], 0))
    # a dense guide held: a sparse call sets the sparse form, and the dense one comes back
    t = _Engine()
    q3.generate_many(t, [[3, 4], [5]], 2, guide=b)
    assert t.log == [("sparse", [0], [0]), ("run", 2), ("dense", [[0, 0]], [0])]
    # a sparse guide held: a dense call, a sparse call and a mixed call all put the sparse one back
    kept = ([0, 0], [0, 0, 0], [], [], [1])
    for guide, first in ((a, ("dense", a.next.tolist(), [1])), (b, ("sparse", [0], [0])), ([a, b], ("sparse", [-1, -1, 2], [1, 2]))):
        t = _Engine(kept)
        q3.generate_many(t, [[3, 4], [5]], 2, guide=guide)
        assert t.log == [first, ("run", 2), ("sparse", [0, 0], [1])], t.log
    # one per request, cut to the requests the context leaves room for
    t = _Engine()
    rows, _ = q3.generate_many(t, [[3], [4] * 9, [5], [6]], 2, guide=[b, b, None, a])
    assert rows == [[1, 1], [], [1, 1], [1, 1]] and t.log[0] == ("sparse", [0, -1, -1], [0, -1, 2])
    # regex= is refused together with guide=, without a tokenizer, and without exactly one stop token
    t = _Engine()
    tok = type("T", (), {"vocab": VOCAB})()
    for kw in (dict(guide=a, tokenizer=tok, stop_tokens=[EOS]), dict(stop_tokens=[EOS]), dict(tokenizer=tok), dict(tokenizer=tok, stop_tokens=[EOS, 3])):
        with pytest.raises(ValueError):
            q3.generate_many(t, [[3]], 2, regex="a+", **kw)
    with pytest.raises(ValueError, match="position 0"):
        q3.generate_many(t, [[3]], 2, regex="^a", tokenizer=tok, stop_tokens=[EOS])
    assert t.log == []
    # the shorthand compiles once per (pattern, tokenizer, eos)
    import qwen3_rs_amd.generation as gen
    q3.generate_many(t, [[3]], 2, regex="a+b", tokenizer=tok, stop_tokens=[EOS])
    first = gen._REGEX_GUIDES[("a+b", id(tok), EOS)][0]
    q3.generate_many(t, [[3]], 2, regex="a+b", tokenizer=tok, stop_tokens=[EOS])
    assert gen._REGEX_GUIDES[("a+b", id(tok), EOS)][0] is first and isinstance(first, SA)
    assert [e[0] for e in t.log] == ["sparse", "run", "dense"] * 2


# ---- the regular-expression compiler
def accepts(dfa, data: bytes) -> bool:
    trans, s, accepting = dfa
    for b in data:
        s = int(trans[s, b])
        if s < 0:
            return False
    return s in accepting


# (pattern, a 4-symbol alphabet, matching strings, non-matching strings)
PATTERNS = [
    (r"(ab|cd)+", "abcd", ["ab", "cd", "abcd", "cdab", "ababab"], ["", "a", "abc", "ac", "abé", "é"]),
    (r"a(b|c)*d", "abcd", ["ad", "abd", "acbd", "abbbcd", "accd"], ["", "a", "d", "abdd", "aed", "aéd"]),
    (r"(?:ab|a)+b?", "abc.", ["a", "ab", "aab", "abb", "abab"], ["", "b", "abbb", "ac", "aé", "é"]),
    (r"\d{2,3}[a-c]?", "12ad", ["12", "123", "12a", "999c", "00b"], ["1", "1234", "12d", "12ab", "١٢", "12é"]),
    (r"a{2}b{1,}c{,2}", "abcd", ["aab", "aabb", "aabc", "aabcc", "aabbbcc"], ["ab", "aa", "aaab", "aabccc", "aabd", "aabé"]),
    (r"[^a]b.", "ab\né", ["bbb", "\nba", "ébé", "bbé", "éb日"], ["abb", "bb\n", "bb", "bbbb", "éb", "b"]),
    (r"\w+\s\W", "a _é", ["a é", "a_  ", "_ é", "aa\té", "Z9 !"], ["a", "a a", " é", "é é", "a é ", "aé"]),
    (r"\D\S*", "1 aé", ["a", "é", " a", "aé1", "éé"], ["", "1", "1a", "a ", "aé a", "1é"]),
    (r"é+x|", "éxa\n", ["", "éx", "ééx", "éééx", "ééééx"], ["é", "x", "éxx", "ex", "\n", "éxé"]),
    (r"\x41\.[\]x-]\n?", "A.]\n", ["A.]", "A.x", "A.-", "A.]\n", "A.-\n"], ["A", "Ab]", "A.a", "A.]]", "a.]", "A.é"]),
    (r"[a-c\d_]*\t?\r?", "a1_\t", ["", "abc", "a1_", "c9\t", "\t\r", "\r"], ["d", "a\t\t", "\r\t", "é", "aé", "a d"]),
    (r"(a|b)(c|)\??\{x}\\", "ac?\\", ["a{x}\\", "ac{x}\\", "b?{x}\\", "bc?{x}\\", "b{x}\\"], ["a", "a{x}", "acc{x}\\", "a??{x}\\", "é{x}\\", "ax\\"]),
    (r"日本?語*", "日本語a", ["日", "日本", "日語語", "日本語", "日語"], ["", "本", "日本本", "日a", "語", "日本語a"]),
    (r"[\W\d]+|x{0}y", "a1é ", ["1", "é", " 1é", "y", "é é"], ["", "a", "1a", "xy", "yy", "aé"]),
]


@pytest.mark.parametrize("case", PATTERNS, ids=[p[0] for p in PATTERNS])
def test_regex_dfa_agrees_with_re_fullmatch(q3, case):
    pattern, alphabet, yes, no = case
    assert len(set(alphabet)) == 4
    dfa = q3.regex_dfa(pattern)
    trans, start, accepting = dfa
    assert trans.shape[1] == 256 and trans.dtype == np.int32 and start == 0 and trans.min() >= -1 and trans.max() < trans.shape[0]
    # the hand-written lists are right by re itself, then the DFA agrees with them
    assert len(yes) >= 5 and len(no) >= 5
    assert any(ord(c) > 127 for s in yes + no for c in s)
    for s in yes:
        assert re.fullmatch(pattern, s, re.ASCII), s
        assert accepts(dfa, s.encode()), s
    for s in no:
        assert not re.fullmatch(pattern, s, re.ASCII), s
        assert not accepts(dfa, s.encode()), s
    # every string over the alphabet up to length 6: 5,461 of them
    rx, count, wrong = re.compile(pattern, re.ASCII), 0, []
    for n in range(7):
        for tup in itertools.product(alphabet, repeat=n):
            s = "".join(tup)
            count += 1
            if bool(rx.fullmatch(s)) != accepts(dfa, s.encode()):
                wrong.append(s)
    assert count == 5461 and not wrong, wrong[:5]


def test_the_dfa_is_minimal(q3):
    # (a|b)*abb: the four states of the textbook; two spellings of one language give one table
    assert q3.regex_dfa(r"(a|b)*abb")[0].shape[0] == 4
    x, y = q3.regex_dfa(r"(?:ab|a)+"), q3.regex_dfa(r"a(b?a)*b?")
    assert np.array_equal(x[0], y[0]) and x[1:] == y[1:]
    # no state is dead: from every state an accepting one is reachable, so -1 is the only way to fail
    trans, start, accepting = q3.regex_dfa(r"ab(c|d)e")
    assert trans.shape[0] == 5 and accepting == [4]
    # nothing matches (a digit that is no digit): the start state alone, not accepting, and the lift calls it dead
    trans, start, accepting = q3.regex_dfa(r"a[^\x00-\x7f\D][^\d\D]")
    assert trans.shape[0] == 1 and (trans == -1).all() and accepting == []
    with pytest.raises(ValueError, match="dead"):
        q3.SparseAutomaton.from_regex(r"a[^\d\D]", VOCAB, EOS)


@pytest.mark.parametrize("pattern, at", [("^a", 0), ("a$", 1), (r"a\b", 1), (r"\Aa", 0), (r"(a)\1", 3), ("(?=a)a", 0), ("(?!a)b", 0), ("(?<=a)b", 0),
                                         ("(?P<n>a)", 0), ("(?i)a", 0), ("a*?", 2), ("a+?", 2), ("a??", 2), ("a{1,2}?", 6), ("a*+", 2), ("a++", 2),
                                         ("[é]", 1), ("[a-é]", 3), (r"[\xe9]", 1), ("a**", 2), ("*a", 0), ("a|*", 2), ("(a", 0), ("a)", 1), ("[a", 0),
                                         ("[b-a]", 3), (r"\q", 0), (r"\x4", 0), ("a{3,2}", 1), ("a\\", 2), ("(a{1000}){1000}", 15)])
def test_refused_constructs_raise_with_the_position(q3, pattern, at):
    with pytest.raises(ValueError, match=f"position {at} of"):
        q3.regex_dfa(pattern)


def test_a_pattern_above_the_state_limit_is_refused(q3):
    with pytest.raises(ValueError, match="limit of"):
        q3.regex_dfa("(a|b)*a" + "(a|b)" * 16)                                    # 2^17 DFA states
    with pytest.raises(ValueError, match="limit of"):
        q3.regex_dfa("a{300000}")
    with pytest.raises(TypeError):
        q3.regex_dfa(b"a")


# ---- UTF-8 and the token lift
def walk(dfa, data: bytes):
    trans, s, accepting = dfa
    for b in data:
        s = int(trans[s, b])
        if s < 0:
            return None
    return s


@pytest.mark.parametrize("pattern", [".", "[^a]", r"\D", r"\W", r"\S"])
def test_a_truncated_code_point_is_not_accepted(q3, pattern):
    dfa = q3.regex_dfa(pattern)
    for ch in ("é", "日", "😀", "߿", "ࠀ", "￿", "\U00010000", "\U0010ffff"):
        full = ch.encode()
        assert accepts(dfa, full), ch
        for cut in range(1, len(full)):
            s = walk(dfa, full[:cut])
            assert s is not None and s not in dfa[2], (ch, cut)             # on the way, and not accepting
    # ill-formed sequences lead nowhere: a lone continuation byte, overlong forms, a surrogate, above U+10FFFF, 0xff
    for bad in (b"\x80", b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf0\x80\x80\x80", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xff"):
        assert walk(dfa, bad) is None, bad
    assert not accepts(dfa, "éé".encode()) and accepts(q3.regex_dfa(pattern + "+"), "é日😀".encode())


def test_the_token_lift_at_the_edge_of_a_code_point(q3):
    SA = q3.SparseAutomaton
    tok = {bytes(b): i for i, b in enumerate(VOCAB)}
    dfa = q3.regex_dfa(r"[^a]\d")
    g = SA.from_byte_dfa(*dfa, VOCAB, EOS)
    allowed = lambda s: set(np.flatnonzero(g.row(s) >= 0).tolist())
    # a token whose bytes end inside a code point is allowed: the next token can complete it
    half, rest, whole = tok[b"\xc3"], tok[b"\xa9"], tok["é".encode()]
    assert half in allowed(0) and whole in allowed(0) and tok["日".encode()[:2]] in allowed(0)
    mid = g.step(0, half)
    assert mid != 0 and allowed(mid) == set(range(0x80, 0xc0)) and g.step(mid, rest) == g.step(0, whole)
    # a token that starts with the rest of one code point and goes on
    dfa2 = q3.regex_dfa(r"[^a]x\d")
    g2 = SA.from_byte_dfa(*dfa2, VOCAB, EOS)
    assert g2.step(g2.step(0, half), tok[b"\xa9x"]) == g2.step(g2.step(0, whole), tok[b"x"])
    # a token that ends inside an ill-formed sequence is forbidden, and so are eos outside accepting states and the empty token
    assert tok[b"\x80"] not in allowed(0) and tok[b"\xa9x"] not in allowed(0) and tok[b""] not in allowed(0) and EOS not in allowed(0)
    assert tok[b"x\xe6"] not in allowed(0) and tok[b"x\xe6"] in set(np.flatnonzero(SA.from_regex(r"x.", VOCAB, EOS).row(0) >= 0).tolist())
    # eos is allowed exactly where the byte state accepts: walk the token states beside the byte states
    seen, todo = {0: dfa[1]}, [0]
    while todo:
        s = todo.pop()
        for v in allowed(s) - {EOS}:
            to, b = g.step(s, v), walk((dfa[0], seen[s], dfa[2]), VOCAB[v])
            assert b is not None
            if to not in seen:
                seen[to] = b
                todo.append(to)
            assert seen[to] == b
    assert len(seen) == g.n_states - 1
    for s, b in seen.items():
        assert (EOS in allowed(s)) == (b in dfa[2]), s
    end = g.n_states - 1
    assert allowed(end) == {EOS} and g.step(end, EOS) == end
    # a whole string through tokens of several bytes, then eos; eos too early is refused
    assert g.walk([whole, tok[b"1"], EOS])[1] is None and g.walk([half, rest, tok[b"7"], EOS, EOS])[1] is None
    assert g.walk([whole, EOS])[1] == 1 and g.walk([tok[b"a"]])[1] == 0 and g.walk([whole, tok[b"12"]])[1] == 1
