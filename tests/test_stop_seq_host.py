"""Stop sequences on the host (include/qwen3_hip.h section 2t): the two compilers of qwen3_rs_amd/stops.py against a brute-force
reference, q3_op_stop_seq -- the __host__ __device__ step the kernel calls -- on compiled and on hand-made tables,
q3_cols_schedule_stop_seq against the simulation of the five rules for (prompt_len, n_emit), and every refusal.  Host only: no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cols_sim
import stop_seq_ref as ref
from cols_stop_cases import CAP, PROMPT_LEN, SLOTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"q3_stop_seq_set", "q3_stop_seq_get", "q3_cols_schedule_stop_seq", "q3_op_stop_seq"}
N = len(PROMPT_LEN)
V = len(ref.VOCAB)


def test_names_declared_listed_exported(q3):
    hdr = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    declared = set(re.findall(r"\b(q3_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(q3.EXPORTED_SYMBOLS)
    lib = q3.load_library()
    for s in NEW:
        assert hasattr(lib, s)
    assert "#define Q3_STOP_SEQ_MAX_STATES 65536" in hdr and q3.STOP_SEQ_MAX_STATES == 65536
    assert "#define Q3_STOP_SEQ_MAX_EDGES 16777216" in hdr and q3.STOP_SEQ_MAX_EDGES == 1 << 24
    assert "#define Q3_ABI_VERSION 1" in hdr and lib.q3_abi_version() == 1


def walk_emit(a, stream):
    state, at = a.walk(stream)
    return (len(stream), state) if at is None else (at + 1, -1)


def check_stream(q3, a, stream, want):
    """walk, q3_op_stop_seq and the reference agree on n_emit; walk and q3_op_stop_seq on the end state"""
    w = walk_emit(a, stream)
    op = q3.ops.stop_seq(a.default, a.offsets, a.tokens, a.targets, a.vocab_size, a.start, stream)
    assert w[0] == want and op[0] == want, (stream, w, op, want)
    # (a match on the last token and no match both give len(stream): the end state tells them apart)
    assert op == w, (stream, w, op)


# ---- the compiler of strings, over the designed vocabulary

STRING_LISTS = [
    ["ab", "b"],                    # one a suffix of another
    ["aab"],                        # self-overlap: "aaab"
    ["\n\n"],
    ["a\nb"],                       # ends mid-token in "a\nba", spans tokens in "a", "\n", "b"
    ["ba\nab\na"],                  # seven bytes: three tokens at the least
    ["ab", "ba", "\n\n", "aab"],
    ["abab", "bab", "b\n"],
    ["a", "bbb\n"],
]


def random_stream(rng, n=64, plant=None):
    """n random tokens; plant: one of these strings is spelled into the stream in a random tokenisation, tokens of no bytes between,
    in every second stream -- so that long strings occur too"""
    stream = [int(t) for t in rng.integers(0, V, n)]
    if plant and rng.integers(0, 2):
        text, pieces = plant[int(rng.integers(0, len(plant)))].encode(), []
        while text:
            k = int(rng.integers(1, 4))
            pieces.append(ref.tok(text[:k]))
            text = text[k:]
            if rng.integers(0, 3) == 0:
                pieces.append(ref.EMPTY[int(rng.integers(0, 2))])
        at = int(rng.integers(0, n - len(pieces)))
        stream[at:at + len(pieces)] = pieces
    return stream


@pytest.mark.parametrize("strings", STRING_LISTS, ids=[repr(s) for s in STRING_LISTS])
def test_strings_against_brute_force(q3, strings):
    a = q3.stop_automaton_from_strings(strings, ref.VOCAB)
    rng = np.random.default_rng(600 + STRING_LISTS.index(strings))
    hit = 0
    for _ in range(60):
        stream = random_stream(rng, plant=strings)
        want = ref.n_emit_strings(stream, ref.VOCAB, strings)
        check_stream(q3, a, stream, want)
        hit += want < len(stream)
        # behind the match the stream goes on: cut in front of the completing token nothing matches
        check_stream(q3, a, stream[:want - 1], want - 1)
    assert hit >= 10


def test_random_string_lists(q3):
    rng = np.random.default_rng(99)
    early = late = 0
    for _ in range(40):
        k = int(rng.integers(1, 5))
        strings = sorted({"".join(rng.choice(["a", "b", "\n"], int(rng.integers(2, 7)))) for _ in range(k)})
        a = q3.stop_automaton_from_strings(strings, ref.VOCAB)
        for _ in range(6):
            stream = random_stream(rng)
            want = ref.n_emit_strings(stream, ref.VOCAB, strings)
            check_stream(q3, a, stream, want)
            early += want <= 8
            late += want > 8
    assert early >= 20 and late >= 20


def test_strings_designed_streams(q3):
    t = ref.tok
    e0, e1 = ref.EMPTY
    cases = [
        (["aab"], [t(b"a"), t(b"aa"), t(b"b")], 3),                        # "aaab": the self-overlap
        (["aab"], [t(b"aa"), e0, t(b"ab"), t(b"a")], 3),                   # a token of no bytes leaves the state
        (["ab", "b"], [t(b"a"), t(b"a\n"), t(b"\nb")], 3),                 # the suffix "b" alone
        (["a\nb"], [t(b"b"), t(b"a\nb")], 2),                              # whole inside one token
        (["a\nb"], [t(b"ba"), t(b"\nba")], 2),                             # ends mid-token
        (["a\nb"], [t(b"a"), e1, t(b"\n"), e0, t(b"b"), t(b"a")], 5),      # spans three tokens, empty ones between
        (["ba\nab\na"], [t(b"bba"), t(b"\nab"), t(b"\nab")], 3),           # seven bytes over three tokens, ends mid-token
        (["\n\n"], [t(b"a\n"), t(b"a\n"), t(b"\na")], 3),
        (["\n\n"], [e0, e1, e0], 3),                                       # nothing but empty tokens: no match
        (["ab"], [t(b"a")], 1),                                            # mid-match at the end: no match
    ]
    for strings, stream, want in cases:
        assert ref.n_emit_strings(stream, ref.VOCAB, strings) == want
        check_stream(q3, q3.stop_automaton_from_strings(strings, ref.VOCAB), stream, want)
    # a state mid-match is not the root: the end state of "a" under ["ab"] differs from that of "b"
    a = q3.stop_automaton_from_strings(["ab"], ref.VOCAB)
    assert a.walk([t(b"a")])[0] != a.walk([t(b"b")])[0] == a.start


def test_strings_take_bytes_and_str(q3):
    a = q3.stop_automaton_from_strings([b"ab", "\n\n"], ref.VOCAB)
    b = q3.stop_automaton_from_strings(["ab", b"\n\n"], ref.VOCAB)
    for x, y in ((a.default, b.default), (a.offsets, b.offsets), (a.tokens, b.tokens), (a.targets, b.targets)):
        assert np.array_equal(x, y)


# ---- the compiler of token sequences

def test_token_sequences_against_brute_force(q3):
    rng = np.random.default_rng(7)
    hit = 0
    for case in range(60):
        vocab = int(rng.integers(2, 7))
        seqs = sorted({tuple(int(t) for t in rng.integers(0, vocab, int(rng.integers(1, 5)))) for _ in range(int(rng.integers(1, 5)))})
        a = q3.stop_automaton(seqs, vocab)
        for _ in range(8):
            stream = [int(t) for t in rng.integers(0, vocab, 64)]
            want = ref.n_emit_seqs(stream, seqs)
            check_stream(q3, a, stream, want)
            check_stream(q3, a, stream[:want - 1], want - 1)
            hit += want < 64
    assert hit >= 100


def test_token_sequences_designed(q3):
    cases = [
        ([[1, 2], [2]], [1, 1, 2], 3),                  # one a suffix of another: "2" completes first
        ([[1, 1, 2]], [1, 1, 1, 2, 0], 4),              # self-overlap
        ([[1, 2, 3], [2, 4]], [1, 2, 4, 3], 3),         # the failure link from "1 2" to "2"
        ([[1, 2, 3], [2]], [0, 1, 2, 3], 3),            # an output link: "1 2" holds the complete "2"
        ([[5]], [5], 1),
        ([[1, 2]], [1, 0, 2, 1], 4),                    # no match, mid-match at the end
    ]
    for seqs, stream, want in cases:
        assert ref.n_emit_seqs(stream, seqs) == want
        check_stream(q3, q3.stop_automaton(seqs, 6), stream, want)
    a = q3.stop_automaton([[1, 2, 3]], 151936)
    assert a.vocab_size == 151936 and a.n_states == 3 and list(a.default) == [0, 0, 0]
    # a vocabulary of one token whose only sequence is that token: the one state ends every request at y_0
    one = q3.stop_automaton([[0]], 1)
    assert one.n_states == 1 and one.next_of(0, 0) == -1
    check_stream(q3, one, [0, 0], 1)


def test_compilers_refuse(q3):
    for bad in ([], [[]], [[1], [1]], [[1, 2], [3], [1, 2]], [[6]], [[-1]]):
        with pytest.raises(ValueError):
            q3.stop_automaton(bad, 6)
    with pytest.raises(ValueError):
        q3.stop_automaton([[1]], 0)
    for bad in ([], [""], ["ab", "ab"], ["ab", b"ab"]):
        with pytest.raises(ValueError):
            q3.stop_automaton_from_strings(bad, ref.VOCAB)


def test_cut_at_stop(q3):
    assert q3.cut_at_stop("one\n\ntwo</a>", ["</a>", "\n\n"]) == "one"
    assert q3.cut_at_stop("one two", ["\n\n"]) == "one two"
    assert q3.cut_at_stop(b"xab", [b"b", b"ab"]) == b"x"
    assert q3.cut_at_stop("abc", []) == "abc"


def test_compile_stop_per_request(q3):
    from qwen3_rs_amd.stops import compile_stop, first_match

    class Tok:
        vocab = ref.VOCAB
    tk = Tok()
    assert compile_stop(None, 3, V) is None and compile_stop([None, None], 2, V) is None
    a, start = compile_stop(["ab"], 3, V, tk)
    assert start == [a.start] and a is compile_stop(["ab"], 3, V, tk)[0]              # compiled once
    b, start = compile_stop([[1, 2], [3]], 3, V)
    assert start == [0] and b.n_states == 2
    m, start = compile_stop([["ab"], None, [[1, 2]], ["ab"]], 4, V, tk)
    assert start[1] == -1 and start[0] == start[3] == 0 and start[2] == a.n_states and m.n_states == a.n_states + 2
    stream = [ref.tok(b"a"), 1, 2, ref.tok(b"b")]
    assert first_match(m, start[0], stream) == first_match(a, 0, stream) == ref.n_emit_strings(stream, ref.VOCAB, ["ab"]) - 1
    assert first_match(m, start[2], stream) == 2 and first_match(m, -1, stream) is None
    with pytest.raises(ValueError):
        compile_stop([["ab"], None], 3, V, tk)                                        # two values for three requests
    with pytest.raises(ValueError):
        compile_stop(["ab"], 3, V)                                                    # strings without a tokenizer
    with pytest.raises(TypeError):
        compile_stop("ab", 3, V, tk)


# ---- q3_op_stop_seq on hand-made tables

# state 0: dflt 0, edges 3 -> 1, 5 -> -1, 8 -> 2;  state 1: dflt -1, edge 4 -> 0;  state 2 (the last): dflt 2, no edges
HAND = dict(default=[0, -1, 2], offsets=[0, 3, 4, 4], tokens=[3, 5, 8, 4], targets=[1, -1, 2, 0], vocab_size=10)


def hand(q3, start, stream):
    return q3.ops.stop_seq(HAND["default"], HAND["offsets"], HAND["tokens"], HAND["targets"], HAND["vocab_size"], start, stream)


def test_op_on_hand_made_tables(q3):
    assert hand(q3, 0, [0, 5, 1]) == (2, -1)                    # a match through an edge
    assert hand(q3, 0, [3, 7]) == (2, -1)                       # a match through dflt == -1
    assert hand(q3, 0, [3, 4, 3, 4]) == (4, 0)                  # the edge of state 1 leads back
    assert hand(q3, 0, [2]) == (1, 0)                           # a token below the first edge: dflt
    assert hand(q3, 0, [4]) == (1, 0) and hand(q3, 0, [6, 7]) == (2, 0)      # between two edges
    assert hand(q3, 0, [9]) == (1, 0)                           # above the last edge
    assert hand(q3, 0, [3]) == (1, 1) and hand(q3, 0, [8]) == (1, 2)         # the first and the last edge themselves
    assert hand(q3, 2, [0, 3, 5, 8, 9]) == (5, 2)               # the last state: no edges, never leaves
    assert hand(q3, 0, [8, 5, 5]) == (3, 2)
    assert hand(q3, 1, [4, 5]) == (2, -1)
    assert hand(q3, -1, [5, 5, 5]) == (3, -1)                   # start -1: no stop sequences, nothing is stepped
    assert hand(q3, 0, []) == (0, 0)
    # a token outside the vocabulary is clamped into it, never an address: 12 acts as 9, -4 as 0
    assert hand(q3, 0, [12, -4]) == (2, 0) and hand(q3, 1, [-4]) == (1, -1)


def raw_tables(q3, default, offsets, tokens, targets):
    dflt = np.array(default, dtype=np.int32)
    off = np.array(offsets, dtype=np.uint32)
    edges = np.empty(len(tokens), dtype=q3.EDGE_DTYPE)
    edges["token"], edges["next"] = tokens, targets
    return dflt, off, edges


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_refusals_in_order(q3):
    """what q3_stop_seq_set refuses, in guide_sparse_check's order and before the engine is looked at (the engine is null
    throughout, and only a table with nothing to refuse gets as far as saying so); q3_op_stop_seq and the schedule twin refuse
    the same through the same code"""
    L = q3.load_library()
    i32, sz = C.c_int32, C.c_size_t
    dflt, off, edges = raw_tables(q3, HAND["default"], HAND["offsets"], HAND["tokens"], HAND["targets"])
    start = (i32 * 2)(0, -1)

    def err():
        return L.q3_last_error().decode()

    def set_(d=dflt, o=off, e=edges, ns=3, ne=4, vocab=10, st=start, nst=2):
        return L.q3_stop_seq_set(None, ptr(d) if d is not None else None, ptr(o) if o is not None else None, ptr(e) if e is not None else None, ns, ne,
                                 vocab, st, nst)

    def tab(**kw):
        t = dict(HAND)
        t.update(kw)
        return raw_tables(q3, t["default"], t["offsets"], t["tokens"], t["targets"])

    assert set_() == -3 and "null engine" in err()                      # nothing to refuse about the table
    assert set_(d=None) == -3 and "null dflt" in err()
    assert set_(o=None) == -3 and "null row_off" in err()
    assert set_(e=None) == -3 and "null edges" in err()
    assert set_(st=None) == -3 and "null start" in err()
    assert set_(ns=0) == -3 and "edges and no state" in err()
    assert set_(ns=65537) == -3 and "states, at most 65536" in err()
    assert set_(ne=(1 << 24) + 1) == -3 and "edges, at most 16777216" in err()
    assert set_(vocab=0) == -3 and "stop automaton over 0 tokens" in err()
    assert set_(vocab=1 << 31) == -3 and "tokens" in err()
    assert set_(nst=0) == -3 and "no start state" in err()
    assert set_(st=(i32 * 2)(0, 3)) == -3 and "start[1] = 3" in err()
    assert set_(st=(i32 * 2)(-2, 0)) == -3 and "start[0] = -2" in err()
    d, o, e = tab(offsets=[1, 3, 4, 4])
    assert set_(d, o, e) == -3 and "row_off[0]" in err()
    d, o, e = tab(offsets=[0, 3, 2, 4])
    assert set_(d, o, e) == -3 and "row_off[2] = 2 below" in err()
    d, o, e = tab(offsets=[0, 3, 3, 3])
    assert set_(d, o, e) == -3 and "does not end at the 4 edges" in err()
    d, o, e = tab(default=[0, -1, 3])
    assert set_(d, o, e) == -3 and "dflt[2] = 3" in err()
    d, o, e = tab(tokens=[3, 5, 10, 4])
    assert set_(d, o, e) == -3 and "edges[2].token = 10" in err()
    d, o, e = tab(tokens=[3, 3, 8, 4])
    assert set_(d, o, e) == -3 and "ascend strictly" in err()
    d, o, e = tab(targets=[1, -2, 2, 0])
    assert set_(d, o, e) == -3 and "edges[1].next = -2" in err()
    # the order: an earlier refusal wins over a later one
    d, o, e = tab(offsets=[1, 3, 4, 4], targets=[1, -2, 2, 0])
    assert set_(d, o, e, st=(i32 * 2)(0, 3)) == -3 and "start[1] = 3" in err()
    assert set_(d, o, e) == -3 and "row_off[0]" in err()
    # NOT refused: a state that allows no token (q3_guide_set_sparse refuses it) -- dflt -1 and no edges, or every edge -1
    d, o, e = raw_tables(q3, [-1, 0], [0, 0, 1], [2], [-1])
    one = (i32 * 1)(0)
    assert L.q3_stop_seq_set(None, ptr(d), ptr(o), ptr(e), 2, 1, 10, one, 1) == -3 and "null engine" in err()
    assert L.q3_guide_set_sparse(None, ptr(d), ptr(o), ptr(e), 2, 1, 10, one, 1) == -3 and "allows no token" in err()
    n_emit, end = sz(0), i32(0)
    assert L.q3_op_stop_seq(ptr(d), ptr(o), ptr(e), 2, 1, 10, 0, (i32 * 2)(4, 4), 2, C.byref(n_emit), C.byref(end)) == 0
    assert (n_emit.value, end.value) == (1, -1)
    # clearing needs no arrays; it gets as far as the engine
    assert L.q3_stop_seq_set(None, None, None, None, 0, 0, 0, None, 0) == -3 and "null engine" in err()
    n = sz(0)
    assert L.q3_stop_seq_get(None, C.byref(n), C.byref(n), C.byref(n)) == -3

    # q3_op_stop_seq: the table's refusals with start_state as the one start, then its own
    toks = (i32 * 2)(3, 4)

    def op(d=dflt, o=off, e=edges, ns=3, ne=4, vocab=10, st=0, tk=toks, nt=2, out=C.byref(n_emit), endp=C.byref(end)):
        return L.q3_op_stop_seq(ptr(d) if d is not None else None, ptr(o), ptr(e), ns, ne, vocab, st, tk, nt, out, endp)

    assert op() == 0 and (n_emit.value, end.value) == (2, 0)
    assert op(d=None) == -3 and "null dflt" in err()
    assert op(st=3) == -3 and "start[0] = 3" in err()
    assert op(st=-2) == -3
    d2, o2, e2 = tab(tokens=[3, 3, 8, 4])
    assert op(d2, o2, e2, tk=None) == -3 and "ascend strictly" in err()         # the table first
    assert op(ns=0, ne=0) == -3 and "no states" in err()
    assert op(tk=None) == -3 and "null tokens" in err()
    assert op(tk=None, nt=0) == 0 and (n_emit.value, end.value) == (0, 0)
    assert op(out=None) == -3 and op(endp=None) == -3

    # the schedule twin: q3_cols_schedule_stop's refusals, then the table's, then the lengths', then the start count
    plen, nnew, rows, stop = (sz * 2)(4, 2), (sz * 2)(3, 3), (i32 * 6)(1, 2, 3, 4, 5, 6), (i32 * 9)(*range(10, 19))

    def sched(pl=plen, nn=nnew, nr=2, ms=1, rw=rows, stp=stop, nstop=1, d=dflt, o=off, e=edges, ns=3, ne=4, vocab=10, st=start, nst=2):
        return L.q3_cols_schedule_stop_seq(pl, nn, nr, ms, rw, stp, nstop, ptr(d), ptr(o), ptr(e), ns, ne, vocab, st, nst, None, 0, C.byref(n), None, None)

    assert sched() == 0
    assert sched(rw=None) == -3 and "null rows" in err()
    assert sched(nstop=9) == -3 and "stop tokens" in err()
    assert sched(stp=None) == -3
    assert sched(d=d2, o=o2, e=e2, nr=0) == -3 and "ascend strictly" in err()    # the table in front of the request list
    assert sched(nr=0) == -3 and "request list" in err()
    assert sched(ms=0) == -3 and sched(ms=33) == -3
    assert sched(nst=1) == 0
    assert sched(nr=1) == -3 and "2 start states" in err()                       # neither one start nor one per request
    assert sched(nr=1, ms=0) == -3 and "max_streams" in err()                    # the lengths in front of the start count


# ---- the schedule twin against the simulation

def tup(stats):
    return (stats.passes, stats.live_columns, stats.prompt_columns, stats.decode_columns)


def check_schedule(q3, rows, seqs, stop_tokens, slots, starts=None, vocab=16, plen=PROMPT_LEN):
    a = q3.stop_automaton(seqs, vocab)
    tables = (a.default, a.offsets, a.tokens, a.targets)
    emit = ref.n_emit_rows(rows, seqs, stop_tokens, starts)
    want, wstats = cols_sim.schedule(plen, emit, slots)
    start = a.start if starts is None else starts
    got, n_out, stats = q3.cols_schedule_stop_seq(plen, [len(r) for r in rows], slots, rows, stop_tokens, tables, vocab, start)
    assert n_out == emit
    assert got == want and tup(stats) == tuple(wstats)
    return emit


def designed_rows():
    """rows of 1s with a reset case in them under the sequences [[7, 8], [9]]: request a never ends and its last token at the cap is 7,
    so its slot is left mid-match; the request b that takes the slot next begins with 8 and must not end there.  Request c ends
    inside its row on 7 8 with the two tokens in different passes, request d at y_0 on 9."""
    seqs = [[7, 8], [9]]
    for a in range(N):
        for b in range(N):
            for c in range(N):
                for d in range(N):
                    if len({a, b, c, d}) < 4:
                        continue
                    rows = [[1] * CAP for _ in range(N)]
                    rows[a][-1] = 7
                    rows[b][0] = 8
                    rows[c][3:5] = [7, 8]
                    rows[d][0] = 9
                    emit = ref.n_emit_rows(rows, seqs)
                    if any(x == a and y == b for _, x, y in ref.slot_successions(PROMPT_LEN, emit, SLOTS)):
                        assert emit[a] == CAP and emit[b] == CAP and emit[c] == 5 and emit[d] == 1
                        return rows, seqs, (a, b, c, d)
    raise AssertionError("no reset case among the requests")


def test_schedule_equals_simulation_on_designed_rows(q3):
    rows, seqs, (a, b, c, d) = designed_rows()
    emit = check_schedule(q3, rows, seqs, [], SLOTS)
    assert emit[b] == CAP and emit[c] == 5 and emit[d] == 1
    assert cols_sim.schedule(PROMPT_LEN, emit, SLOTS)[1].passes < cols_sim.schedule(PROMPT_LEN, [CAP] * N, SLOTS)[1].passes
    # sequences and stop tokens together: the earlier of the two ends the request
    rows[c][2] = 5                                          # a stop token in front of the sequence
    rows[b][6] = 5
    both = check_schedule(q3, rows, seqs, [5], SLOTS)
    assert both[c] == 3 and both[b] == 7 and both[d] == 1
    rows[c][2] = 1
    rows[c][6] = 5                                          # ... and behind it
    assert check_schedule(q3, rows, seqs, [5], SLOTS)[c] == 5
    for slots in (1, 2, 7, 32):
        check_schedule(q3, rows, seqs, [5], slots)


def test_schedule_per_request_starts(q3):
    rows, seqs, (a, b, c, d) = designed_rows()
    starts = [0] * N
    starts[c] = starts[d] = -1                              # no stop sequences for these two: they run to the cap
    emit = check_schedule(q3, rows, seqs, [], SLOTS, starts)
    assert emit == [CAP] * N
    starts[d] = 0
    emit = check_schedule(q3, rows, seqs, [], SLOTS, starts)
    assert emit[d] == 1 and emit[c] == CAP
    # a start state that is not the root: request c starts behind a 7, so an 8 at y_0 ends it
    auto = q3.stop_automaton(seqs, 16)
    mid = auto.next_of(0, 7)
    assert mid > 0
    rows2 = [list(r) for r in rows]
    rows2[c][0] = 8
    tables = (auto.default, auto.offsets, auto.tokens, auto.targets)
    st = [0] * N
    st[c] = mid
    _, n_out, _ = q3.cols_schedule_stop_seq(PROMPT_LEN, [CAP] * N, SLOTS, rows2, [], tables, 16, st)
    assert n_out[c] == 1 and n_out[b] == CAP


def test_schedule_random_cases(q3):
    rng = np.random.default_rng(31)
    ended = 0
    for _ in range(120):
        ms = int(rng.integers(1, 33))
        nr = int(rng.integers(1, 30))
        plen = [int(v) for v in rng.integers(1, 71, nr)]
        nnew = [int(v) for v in rng.integers(1, 13, nr)]
        rows = [[int(t) for t in rng.integers(0, 4, k)] for k in nnew]
        seqs = sorted({tuple(int(t) for t in rng.integers(0, 4, int(rng.integers(1, 4)))) for _ in range(int(rng.integers(1, 4)))})
        stop = [int(t) + 4 for t in rng.choice(2, int(rng.integers(0, 2)), replace=False)]
        starts = None if rng.integers(0, 2) else [int(s) for s in rng.choice([0, -1], nr)]
        emit = check_schedule(q3, rows, [list(q) for q in seqs], stop, ms, starts, vocab=8, plen=plen)
        ended += emit != nnew
    assert ended >= 60


def test_no_automaton_equals_cols_schedule_stop(q3):
    rng = np.random.default_rng(78)
    rows = [[int(t) for t in rng.integers(0, 6, CAP)] for _ in range(N)]
    for stop in ([], [0], [1, 5]):
        for ms in (1, 3, 32):
            assert q3.cols_schedule_stop_seq(PROMPT_LEN, [CAP] * N, ms, rows, stop, None, 0, 0) == q3.cols_schedule_stop(PROMPT_LEN, [CAP] * N, ms, rows, stop)
    # ... and so does an automaton that never matches, and one every request opts out of
    a = q3.stop_automaton([[7, 7]], 8)
    tables = (a.default, a.offsets, a.tokens, a.targets)
    want = q3.cols_schedule_stop(PROMPT_LEN, [CAP] * N, 3, rows, [0])
    assert q3.cols_schedule_stop_seq(PROMPT_LEN, [CAP] * N, 3, rows, [0], tables, 8, 0) == want
    b = q3.stop_automaton([[1]], 8)
    assert q3.cols_schedule_stop_seq(PROMPT_LEN, [CAP] * N, 3, rows, [0], (b.default, b.offsets, b.tokens, b.targets), 8, [-1] * N) == want


# ---- generate_many over an engine stand-in: the host-cut path and the engine path agree on what they ask of the engine

class StandIn:
    """answers generate_many_greedy with fixed rows and generate_many_stop with those rows cut by the automaton it was given"""

    def __init__(self, q3, rows, vocab):
        self.q3, self.rows, self.vocab, self.seq, self.calls = q3, rows, vocab, (None, []), []

    def get_config(self):
        class Cfg:
            vocab_size, seq_len = self.vocab, 4096
        return Cfg()

    def get_stop_sequences(self):
        return self.seq

    def set_stop_sequences(self, automaton, start=None):
        self.seq = (None, []) if automaton is None else (automaton, list(start))
        self.calls.append(("set", None if automaton is None else list(start)))

    def generate_many_greedy(self, prompts, n_new):
        return [r[:k] for r, k in zip(self.rows, n_new)], "stats"

    def generate_many_stop(self, prompts, n_new, stop_tokens, sampler=None, raw=False):
        from qwen3_rs_amd.stops import first_match
        a, start = self.seq
        out = []
        for i, (r, k) in enumerate(zip(self.rows, n_new)):
            cut = [j for j, t in enumerate(r[:k]) if t in set(stop_tokens)][:1]
            m = None if a is None else first_match(a, start[0 if len(start) == 1 else i], r[:k])
            cut += [] if m is None else [m]
            out.append(r[:min(cut) + 1] if cut else r[:k])
        self.calls.append(("stop", list(stop_tokens)))
        return out, "stats"


def test_generate_many_front_end_over_a_stand_in(q3):
    class Tok:
        vocab = ref.VOCAB
    t = ref.tok
    rows = [[t(b"a"), t(b"b"), t(b"a"), t(b"a")], [t(b"b\n"), t(b"\na"), t(b"a"), t(b"a")], [t(b"a"), t(b"a"), t(b"a"), t(b"a")]]
    prompts = [[1], [2], [3]]
    for stop, want in ((["ab", "\n\n"], [2, 2, 4]), ([[t(b"a"), t(b"a")]], [4, 4, 2]), ([["ab"], None, [[t(b"a")]]], [2, 4, 1])):
        eng = StandIn(q3, rows, V)
        host, _ = q3.generate_many(eng, prompts, 4, stop=stop, tokenizer=Tok())
        assert [len(r) for r in host] == want and eng.calls == []
        dev, _ = q3.generate_many(eng, prompts, 4, stop=stop, tokenizer=Tok(), stop_on_device=True)
        assert dev == host
        assert [c[0] for c in eng.calls] == ["set", "stop", "set"] and eng.calls[-1] == ("set", None) and eng.seq == (None, [])
    # with stop tokens too: the earlier of the two
    eng = StandIn(q3, rows, V)
    both, _ = q3.generate_many(eng, prompts, 4, stop_tokens=[t(b"a")], stop=[[t(b"b")]], stop_on_device=True)
    assert both == q3.generate_many(eng, prompts, 4, stop_tokens=[t(b"a")], stop=[[t(b"b")]])[0] == [rows[0][:1], rows[1][:3], rows[2][:1]]
    with pytest.raises(ValueError):
        q3.generate_many(eng, prompts, 4, stop=[[1]], stop_on_device=True, dense_min=8)
    with pytest.raises(ValueError):
        q3.generate_many(eng, prompts, 4, stop=["ab"])                           # strings without a tokenizer
