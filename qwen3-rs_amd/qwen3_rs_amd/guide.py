"""Guided decoding on the host side (include/qwen3_hip.h section 2r): token automata as Transformer.set_guide and
generate_many(guide=...) take them, and two ways to build one -- a trie over token sequences, and the lift of a byte-level DFA to
the tokens of a vocabulary.  Section 2s adds the sparse form of the same rule, SparseAutomaton (a default per state and a sorted
edge list, up to 2^20 states, for Transformer.set_guide_sparse), with the same builders vectorised over the vocabulary, and regex_dfa,
which compiles a regular expression into the byte DFA the lift takes."""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

GUIDE_MAX_STATES = 4096   # Q3_GUIDE_MAX_STATES
GUIDE_SPARSE_MAX_STATES = 1 << 20   # Q3_GUIDE_SPARSE_MAX_STATES (section 2s)
GUIDE_SPARSE_MAX_EDGES = 1 << 27    # Q3_GUIDE_SPARSE_MAX_EDGES


class Automaton:
    """next[n_states][V] of int16: next[s][v] >= 0, in state s token v may come and leads to that state; -1, it may not.  start: the
    state a request begins in."""

    def __init__(self, next, start: int = 0):
        next = np.ascontiguousarray(next)
        if next.ndim != 2 or next.shape[0] == 0 or next.shape[1] == 0:
            raise ValueError("next must be a table [n_states][vocab_size]")
        if not np.issubdtype(next.dtype, np.integer):
            raise TypeError(f"next must hold integers, got {next.dtype}")
        if next.shape[0] > GUIDE_MAX_STATES:
            raise ValueError(f"{next.shape[0]} states, at most {GUIDE_MAX_STATES}")
        if next.min() < -1 or next.max() >= next.shape[0]:
            raise ValueError(f"an entry of next lies outside -1 .. {next.shape[0] - 1}")
        dead = np.flatnonzero(~(next >= 0).any(axis=1))
        if dead.size:
            raise ValueError(f"state {int(dead[0])} allows no token")
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)):
            raise TypeError(f"start must be an integer, got {start!r}")
        if not 0 <= start < next.shape[0]:
            raise ValueError(f"start {start} is not a state (0 .. {next.shape[0] - 1})")
        self.next = next.astype(np.int16)
        self.start = int(start)

    @property
    def n_states(self) -> int:
        return self.next.shape[0]

    @property
    def vocab_size(self) -> int:
        return self.next.shape[1]

    def step(self, state: int, token: int) -> int:
        """the state step of the rule: next[state][token] where that is >= 0, else the state stays"""
        to = int(self.next[state, token])
        return to if to >= 0 else state

    def walk(self, tokens: Iterable[int]) -> Tuple[int, Optional[int]]:
        """Follows the rule from the start state.  Returns (the state behind the last token, None) where every token was allowed,
        else (the state in which the first forbidden token came, its index)."""
        s = self.start
        for i, t in enumerate(tokens):
            if not 0 <= t < self.vocab_size or self.next[s, t] < 0:
                return s, i
            s = int(self.next[s, t])
        return s, None

    @classmethod
    def from_sequences(cls, seqs: Sequence[Sequence[int]], vocab_size: int, eos: int) -> "Automaton":
        """One of several token sequences ("answer with one of these labels"): a trie over them, state 0 its root; behind a complete
        sequence only eos may come, and it loops."""
        seqs = [[int(t) for t in s] for s in seqs]
        if not seqs or any(len(s) == 0 for s in seqs):
            raise ValueError("from_sequences needs at least one sequence, none of them empty")
        if not 0 <= eos < vocab_size or any(not 0 <= t < vocab_size for s in seqs for t in s):
            raise ValueError(f"a token lies outside the vocabulary of {vocab_size}")
        if any(eos in s for s in seqs):
            raise ValueError(f"eos {eos} inside a sequence")
        children: List[dict] = [{}]
        complete = [False]
        for s in seqs:
            at = 0
            for t in s:
                if t not in children[at]:
                    children.append({})
                    complete.append(False)
                    children[at][t] = len(children) - 1
                at = children[at][t]
            complete[at] = True
        n = len(children) + 1                   # and the end state behind eos
        if n > GUIDE_MAX_STATES:
            raise ValueError(f"the trie has {n} states, at most {GUIDE_MAX_STATES}")
        nxt = np.full((n, vocab_size), -1, dtype=np.int16)
        for s, ch in enumerate(children):
            for t, to in ch.items():
                nxt[s, t] = to
            if complete[s]:
                nxt[s, eos] = n - 1
        nxt[n - 1, eos] = n - 1
        return cls(nxt, 0)

    @classmethod
    def from_byte_dfa(cls, trans, start: int, accepting: Iterable[int], token_bytes: Sequence[bytes], eos: int) -> "Automaton":
        """The lift of a byte-level DFA to tokens.  trans[S][256]: the byte state behind a byte, -1 where there is none.  A token is
        allowed in a state when walking its bytes ends in a state from which an accepting state is reachable; eos is allowed exactly
        in accepting states and leads to an end state in which it loops; a token with no bytes is forbidden.  Token states are the
        byte states reachable from `start` over allowed tokens, numbered in the order found (start is 0), the end state last.
        ValueError where the start state is dead or the result exceeds GUIDE_MAX_STATES states."""
        trans = np.asarray(trans)
        if trans.ndim != 2 or trans.shape[1] != 256 or trans.shape[0] == 0:
            raise ValueError("trans must be a table [S][256]")
        S, V = trans.shape[0], len(token_bytes)
        accepting = sorted(set(int(a) for a in accepting))
        if not 0 <= start < S or any(not 0 <= a < S for a in accepting) or not 0 <= eos < V:
            raise ValueError("start, accepting or eos out of range")
        if trans.min() < -1 or trans.max() >= S:
            raise ValueError(f"an entry of trans lies outside -1 .. {S - 1}")
        # live: an accepting state is reachable (backwards over the transitions from the accepting ones)
        before: List[list] = [[] for _ in range(S)]
        for s, c in zip(*np.nonzero(trans >= 0)):
            before[int(trans[s, c])].append(int(s))
        live = np.zeros(S, dtype=bool)
        live[accepting] = True
        todo = list(accepting)
        while todo:
            for s in before[todo.pop()]:
                if not live[s]:
                    live[s] = True
                    todo.append(s)
        if not live[start]:
            raise ValueError("the start state is dead: no accepting state is reachable from it")
        acc = set(accepting)

        def over(s, bs):
            for c in bs:
                s = int(trans[s, c])
                if s < 0:
                    return -1
            return s
        number, order, rows = {start: 0}, [start], []
        at = 0
        while at < len(order):
            s = order[at]
            at += 1
            row = {}
            for v, bs in enumerate(token_bytes):
                if v == eos or len(bs) == 0:
                    continue
                to = over(s, bs)
                if to < 0 or not live[to]:
                    continue
                if to not in number:
                    number[to] = len(order)
                    order.append(to)
                    if len(order) + 1 > GUIDE_MAX_STATES:
                        raise ValueError(f"more than {GUIDE_MAX_STATES} states")
                row[v] = number[to]
            rows.append(row)
        n = len(order) + 1
        nxt = np.full((n, V), -1, dtype=np.int16)
        for i, row in enumerate(rows):
            for v, to in row.items():
                nxt[i, v] = to
            if order[i] in acc:
                nxt[i, eos] = n - 1
        nxt[n - 1, eos] = n - 1
        return cls(nxt, 0)


# ---------------------------------------------------------------------------------------------------------------------
# the sparse form (include/qwen3_hip.h section 2s)
# ---------------------------------------------------------------------------------------------------------------------
def _live_states(trans: np.ndarray, accepting: Sequence[int]) -> np.ndarray:
    """the byte states from which an accepting state is reachable: backwards over the transitions from the accepting ones"""
    S = trans.shape[0]
    src, _ = np.nonzero(trans >= 0)
    dst = trans[trans >= 0]
    order = np.argsort(dst, kind="stable")
    src, dst = src[order], dst[order]
    first = np.searchsorted(dst, np.arange(S + 1))
    live = np.zeros(S, dtype=bool)
    live[list(accepting)] = True
    todo = list(accepting)
    while todo:
        s = todo.pop()
        before = np.unique(src[first[s]:first[s + 1]])
        new = before[~live[before]]
        live[new] = True
        todo.extend(int(x) for x in new)
    return live


def _compress(row: np.ndarray) -> Tuple[int, np.ndarray, np.ndarray]:
    """one dense row as (default, tokens, targets): the default is the row's most frequent value, the edges are the rest"""
    default = int(np.bincount(row + 1).argmax()) - 1
    tokens = np.flatnonzero(row != default).astype(np.int32)
    return default, tokens, row[tokens].astype(np.int32)


class SparseAutomaton:
    """The rule of Automaton on a compressed table: default[s] is what every unlisted token does in state s (-1: forbidden, else the
    state behind it); state s lists tokens[offsets[s] .. offsets[s + 1]), strictly ascending, with targets beside them (-1 or a
    state).  next[s][v] is the target where v is listed in s, else default[s].  Up to GUIDE_SPARSE_MAX_STATES states."""

    def __init__(self, default, offsets, tokens, targets, start: int = 0, vocab_size: Optional[int] = None, dead_ok: bool = False):
        """dead_ok: a state that allows no token is legal -- the stop automata of stops.py, where -1 reads "the sequence is complete"
        and a state may say so of every token"""
        for name, a in (("default", default), ("offsets", offsets), ("tokens", tokens), ("targets", targets)):
            a = np.asarray(a)
            if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
                raise TypeError(f"{name} must be a vector of integers")
        if vocab_size is None or isinstance(vocab_size, bool) or not isinstance(vocab_size, (int, np.integer)) or not 0 < vocab_size < 2 ** 31:
            raise ValueError(f"vocab_size must be an integer in 1 .. 2^31 - 1, got {vocab_size!r}")
        default = np.asarray(default, dtype=np.int64)
        offsets = np.asarray(offsets, dtype=np.int64)
        tokens = np.asarray(tokens, dtype=np.int64)
        targets = np.asarray(targets, dtype=np.int64)
        S, E, V = default.size, tokens.size, int(vocab_size)
        if S == 0 or S > GUIDE_SPARSE_MAX_STATES:
            raise ValueError(f"{S} states: 1 .. {GUIDE_SPARSE_MAX_STATES}")
        if E > GUIDE_SPARSE_MAX_EDGES:
            raise ValueError(f"{E} edges, at most {GUIDE_SPARSE_MAX_EDGES}")
        if offsets.size != S + 1 or targets.size != E:
            raise ValueError(f"offsets must hold {S + 1} entries and targets {E}")
        if offsets[0] != 0 or offsets[-1] != E or (np.diff(offsets) < 0).any():
            raise ValueError("offsets must start at 0, never decrease and end at the number of edges")
        if default.min() < -1 or default.max() >= S or (E and (targets.min() < -1 or targets.max() >= S)):
            raise ValueError(f"a default or a target lies outside -1 .. {S - 1}")
        if E and (tokens.min() < 0 or tokens.max() >= V):
            raise ValueError(f"a token lies outside the vocabulary of {V}")
        owner = np.repeat(np.arange(S), np.diff(offsets))
        if E > 1 and ((np.diff(tokens) <= 0) & (owner[1:] == owner[:-1])).any():
            raise ValueError("the tokens of a state must ascend strictly")
        listed = np.diff(offsets)
        allowed = np.bincount(owner[targets >= 0], minlength=S) if E else np.zeros(S, dtype=np.int64)
        dead = np.flatnonzero((allowed == 0) & ((default < 0) | (listed == V)))
        if dead.size and not dead_ok:
            raise ValueError(f"state {int(dead[0])} allows no token")
        self.dead_ok = bool(dead_ok)
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)):
            raise TypeError(f"start must be an integer, got {start!r}")
        if not 0 <= start < S:
            raise ValueError(f"start {start} is not a state (0 .. {S - 1})")
        self.default = default.astype(np.int32)
        self.offsets = offsets
        self.tokens = tokens.astype(np.int32)
        self.targets = targets.astype(np.int32)
        self.start = int(start)
        self._vocab = V

    @property
    def n_states(self) -> int:
        return self.default.size

    @property
    def n_edges(self) -> int:
        return self.tokens.size

    @property
    def vocab_size(self) -> int:
        return self._vocab

    def next_of(self, state: int, token: int) -> int:
        """next[state][token]"""
        a, b = int(self.offsets[state]), int(self.offsets[state + 1])
        k = a + int(np.searchsorted(self.tokens[a:b], token))
        return int(self.targets[k]) if k < b and self.tokens[k] == token else int(self.default[state])

    def step(self, state: int, token: int) -> int:
        """the state step of the rule: next[state][token] where that is >= 0, else the state stays"""
        to = self.next_of(state, token)
        return to if to >= 0 else state

    def walk(self, tokens: Iterable[int]) -> Tuple[int, Optional[int]]:
        """Automaton.walk: (the state behind the last token, None), or (the state in which the first forbidden token came, its index)"""
        s = self.start
        for i, t in enumerate(tokens):
            to = self.next_of(s, t) if 0 <= t < self._vocab else -1
            if to < 0:
                return s, i
            s = to
        return s, None

    def row(self, state: int) -> np.ndarray:
        """the dense int32 row of one state, made on demand"""
        if not 0 <= state < self.n_states:
            raise IndexError(f"state {state} of {self.n_states}")
        a, b = int(self.offsets[state]), int(self.offsets[state + 1])
        row = np.full(self._vocab, self.default[state], dtype=np.int32)
        row[self.tokens[a:b]] = self.targets[a:b]
        return row

    def to_dense(self) -> Automaton:
        if self.n_states > GUIDE_MAX_STATES:
            raise ValueError(f"{self.n_states} states, a dense table holds at most {GUIDE_MAX_STATES}")
        return Automaton(np.stack([self.row(s) for s in range(self.n_states)]), self.start)

    @classmethod
    def _of_rows(cls, rows, start: int, vocab_size: int) -> "SparseAutomaton":
        """from (default, tokens, targets) per state"""
        offsets = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum([r[1].size for r in rows], out=offsets[1:])
        cat = lambda k: np.concatenate([r[k] for r in rows]) if rows else np.zeros(0, dtype=np.int32)
        return cls(np.array([r[0] for r in rows], dtype=np.int32), offsets, cat(1), cat(2), start, vocab_size)

    @classmethod
    def from_dense(cls, a: Automaton) -> "SparseAutomaton":
        """per state the default is the most frequent value of the row, the edges are the rest"""
        return cls._of_rows([_compress(a.next[s].astype(np.int32)) for s in range(a.n_states)], a.start, a.vocab_size)

    @classmethod
    def from_sequences(cls, seqs: Sequence[Sequence[int]], vocab_size: int, eos: int) -> "SparseAutomaton":
        """Automaton.from_sequences with its state numbers; the default is -1 everywhere and no dense row is made"""
        seqs = [[int(t) for t in s] for s in seqs]
        if not seqs or any(len(s) == 0 for s in seqs):
            raise ValueError("from_sequences needs at least one sequence, none of them empty")
        if not 0 <= eos < vocab_size or any(not 0 <= t < vocab_size for s in seqs for t in s):
            raise ValueError(f"a token lies outside the vocabulary of {vocab_size}")
        if any(eos in s for s in seqs):
            raise ValueError(f"eos {eos} inside a sequence")
        children: List[dict] = [{}]
        complete = [False]
        for s in seqs:
            at = 0
            for t in s:
                if t not in children[at]:
                    children.append({})
                    complete.append(False)
                    children[at][t] = len(children) - 1
                at = children[at][t]
            complete[at] = True
        n = len(children) + 1                   # and the end state behind eos
        if n > GUIDE_SPARSE_MAX_STATES:
            raise ValueError(f"the trie has {n} states, at most {GUIDE_SPARSE_MAX_STATES}")
        rows = []
        for ch, done in zip(children + [{}], complete + [True]):
            edges = sorted(list(ch.items()) + ([(eos, n - 1)] if done else []))
            rows.append((-1, np.array([t for t, _ in edges], dtype=np.int32), np.array([to for _, to in edges], dtype=np.int32)))
        return cls._of_rows(rows, 0, vocab_size)

    @classmethod
    def from_byte_dfa(cls, trans, start: int, accepting: Iterable[int], token_bytes: Sequence[bytes], eos: int) -> "SparseAutomaton":
        """Automaton.from_byte_dfa -- the same semantics and the same state numbers -- vectorised over the vocabulary: one padded
        byte matrix [V][Lmax], and per token state Lmax gathers through trans over the tokens still on their way.  Not bound by
        GUIDE_MAX_STATES."""
        trans = np.asarray(trans)
        if trans.ndim != 2 or trans.shape[1] != 256 or trans.shape[0] == 0:
            raise ValueError("trans must be a table [S][256]")
        S, V = trans.shape[0], len(token_bytes)
        accepting = sorted(set(int(a) for a in accepting))
        if not 0 <= start < S or any(not 0 <= a < S for a in accepting) or not 0 <= eos < V:
            raise ValueError("start, accepting or eos out of range")
        if trans.min() < -1 or trans.max() >= S:
            raise ValueError(f"an entry of trans lies outside -1 .. {S - 1}")
        live = _live_states(trans, accepting)
        if not live[start]:
            raise ValueError("the start state is dead: no accepting state is reachable from it")
        # state S: the sink behind a missing transition or a dead state
        T = np.concatenate([np.where((trans >= 0) & np.append(live, False)[trans], trans, S), np.full((1, 256), S)]).astype(np.int32)
        lens = np.fromiter((len(b) for b in token_bytes), dtype=np.int64, count=V)
        lens[eos] = 0                                                   # eos and tokens without bytes take no part in the lift
        by_len = np.argsort(-lens, kind="stable")                       # tokens of at least i + 1 bytes: by_len[:n_at[i]]
        Lmax = int(lens.max()) if V else 0
        n_at = [int(np.count_nonzero(lens > i)) for i in range(Lmax)]
        B = np.zeros((V, max(Lmax, 1)), dtype=np.uint8)
        flat = np.frombuffer(b"".join(bytes(token_bytes[v]) for v in range(V) if lens[v]), dtype=np.uint8)
        has = np.flatnonzero(lens)
        B[np.repeat(has, lens[has]), np.arange(flat.size) - np.repeat(np.cumsum(lens[has]) - lens[has], lens[has])] = flat
        cols = [np.ascontiguousarray(B[by_len[:n_at[i]], i]) for i in range(Lmax)]          # in the order of by_len
        acc = set(accepting)
        number, order, rows = {start: 0}, [start], []
        at = 0
        while at < len(order):
            s = order[at]
            at += 1
            cur = np.full(V, s, dtype=np.int32)                        # in the order of by_len: the tokens on their way are in front
            for i in range(Lmax):
                cur[:n_at[i]] = T[cur[:n_at[i]], cols[i]]
            to = np.full(V, S, dtype=np.int32)
            to[by_len[:n_at[0]] if Lmax else by_len[:0]] = cur[:n_at[0] if Lmax else 0]
            ok = np.flatnonzero(to != S)
            # new byte states in the order of the first token that reaches them
            found, where = np.unique(to[ok], return_index=True)
            for b in found[np.argsort(where, kind="stable")]:
                if int(b) not in number:
                    number[int(b)] = len(order)
                    order.append(int(b))
                    if len(order) + 1 > GUIDE_SPARSE_MAX_STATES:
                        raise ValueError(f"more than {GUIDE_SPARSE_MAX_STATES} states")
            row = np.full(V, -1, dtype=np.int32)
            if ok.size:
                names = np.full(S, -1, dtype=np.int32)
                names[found] = [number[int(b)] for b in found]
                row[ok] = names[to[ok]]
            default, tokens, targets = _compress(row)
            if s in acc:                        # eos leads to the end state, numbered at the end: -2 until then
                k = int(np.searchsorted(tokens, eos))
                if k < tokens.size and tokens[k] == eos:
                    targets[k] = -2
                else:
                    tokens, targets = np.insert(tokens, k, eos), np.insert(targets, k, -2)
            rows.append((default, tokens, targets))
        n = len(order) + 1
        for r in rows:
            r[2][r[2] == -2] = n - 1
        rows.append((-1, np.array([eos], dtype=np.int32), np.array([n - 1], dtype=np.int32)))
        return cls._of_rows(rows, 0, V)

    @classmethod
    def from_regex(cls, pattern: str, token_bytes: Sequence[bytes], eos: int) -> "SparseAutomaton":
        """the tokens whose bytes, one behind the other, fully match `pattern` (regex_dfa), then eos"""
        return cls.from_byte_dfa(*regex_dfa(pattern), token_bytes, eos)


# ---------------------------------------------------------------------------------------------------------------------
# regular expressions
# ---------------------------------------------------------------------------------------------------------------------
REGEX_MAX_NFA_STATES = 200_000      # a counted repetition expands into copies: the limit on what a pattern may expand to
REGEX_MAX_DFA_STATES = 20_000

_DIGIT = frozenset(range(0x30, 0x3a))
_WORD = _DIGIT | frozenset(range(0x41, 0x5b)) | frozenset(range(0x61, 0x7b)) | {0x5f}
_SPACE = frozenset(b" \t\n\r\f\v")
_ASCII = frozenset(range(128))
_CLASSES = {"d": _DIGIT, "w": _WORD, "s": _SPACE}
_SIMPLE = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "a": 7, "0": 0}
_TAIL = frozenset(range(0x80, 0xc0))
# one well-formed UTF-8 code point above U+007F, byte by byte (no overlong forms, no surrogates, nothing above U+10FFFF)
_NON_ASCII = [
    [range(0xc2, 0xe0), _TAIL],
    [[0xe0], range(0xa0, 0xc0), _TAIL], [list(range(0xe1, 0xed)) + [0xee, 0xef], _TAIL, _TAIL], [[0xed], range(0x80, 0xa0), _TAIL],
    [[0xf0], range(0x90, 0xc0), _TAIL, _TAIL], [range(0xf1, 0xf4), _TAIL, _TAIL, _TAIL], [[0xf4], range(0x80, 0x90), _TAIL, _TAIL],
]


class _Regex:
    """A recursive-descent parser into a tree of ("set", bytes) | ("cat", [..]) | ("alt", [..]) | ("rep", node, m, n or None)."""

    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise TypeError("the pattern must be a str")
        self.p, self.i = pattern, 0

    def fail(self, what: str, at: Optional[int] = None):
        raise ValueError(f"{what} at position {self.i if at is None else at} of {self.p!r}")

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced parenthesis")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.i < len(self.p) and self.p[self.i] == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.p[self.i] not in "|)":
            at = self.i
            atom = self.atom()
            items.append(self.quantified(atom, at))
        return ("cat", items)

    @staticmethod
    def code_point(cls_ascii, non_ascii: bool):
        """one code point: an ASCII byte of the set, or (non_ascii) any well-formed sequence of a code point above U+007F"""
        branches = [("set", frozenset(cls_ascii))] if cls_ascii else []
        if non_ascii:
            branches += [("cat", [("set", frozenset(b)) for b in seq]) for seq in _NON_ASCII]
        return branches[0] if len(branches) == 1 else ("alt", branches)      # (no branch: a class such as [^\d\D] matches nothing)

    def escape(self):
        """behind a backslash: (ascii set, non_ascii) of a class escape, or the code point of a literal"""
        if self.i >= len(self.p):
            self.fail("a backslash at the end")
        c = self.p[self.i]
        self.i += 1
        if c in "dws":
            return _CLASSES[c], False
        if c in "DWS":
            return _ASCII - _CLASSES[c.lower()], True
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(x not in "0123456789abcdefABCDEF" for x in h):
                self.fail("\\x needs two hexadecimal digits", self.i - 2)
            self.i += 2
            return int(h, 16)
        if c in _SIMPLE and not (c == "0" and self.p[self.i:self.i + 1].isdigit()):
            return _SIMPLE[c]
        if c in "123456789":
            self.fail("backreferences are not supported", self.i - 2)
        if c in "bBAZ":
            self.fail("anchors are not supported", self.i - 2)
        if c.isascii() and c.isalnum():
            self.fail(f"unknown escape \\{c}", self.i - 2)
        return ord(c)

    def literal(self, cp: int):
        return ("cat", [("set", frozenset([b])) for b in chr(cp).encode("utf-8")])

    def atom(self):
        c = self.p[self.i]
        at = self.i
        if c == "(":
            self.i += 1
            if self.p[self.i:self.i + 1] == "?":
                if self.p[self.i:self.i + 2] != "?:":
                    self.fail("lookaround, named groups and inline flags are not supported; only (?:...)", at)
                self.i += 2
            node = self.alt()
            if self.i >= len(self.p) or self.p[self.i] != ")":
                self.fail("missing )", at)
            self.i += 1
            return node
        if c in "*+?":
            self.fail("nothing to repeat")
        if c in "^$":
            self.fail("anchors are not supported: the match is a full match")
        self.i += 1
        if c == ".":
            return self.code_point(_ASCII - {10}, True)
        if c == "[":
            return self.char_class(at)
        if c == "\\":
            e = self.escape()
            return self.code_point(*e) if isinstance(e, tuple) else self.literal(e)
        return self.literal(ord(c))

    def char_class(self, at: int):
        negate = self.p[self.i:self.i + 1] == "^"
        self.i += negate
        members, non_ascii, first = set(), False, True
        while True:
            if self.i >= len(self.p):
                self.fail("missing ]", at)
            c = self.p[self.i]
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            lo = self.class_item()
            if isinstance(lo, tuple):
                members |= lo[0]
                non_ascii |= lo[1]
                continue
            if self.p[self.i:self.i + 1] == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                here = self.i
                hi = self.class_item()
                if isinstance(hi, tuple) or hi < lo:
                    self.fail("bad character range", here)
                members |= set(range(lo, hi + 1))
            else:
                members.add(lo)
        if negate:
            members, non_ascii = _ASCII - members, not non_ascii
        return self.code_point(members, non_ascii)

    def class_item(self):
        c = self.p[self.i]
        here = self.i
        self.i += 1
        v = self.escape() if c == "\\" else ord(c)
        if not isinstance(v, tuple) and v > 127:
            self.fail("a non-ASCII character inside a class is not supported", here)
        return v

    def brace(self, i: int):
        """a counted quantifier at position i, or None"""
        import re
        q = re.match(r"\{(\d*)(,?)(\d*)\}", self.p[i:])
        return q if q and (q.group(1) or q.group(3)) else None

    def quantified(self, atom, at: int):
        if self.i >= len(self.p):
            return atom
        c = self.p[self.i]
        here = self.i
        if c == "*":
            m, n = 0, None
        elif c == "+":
            m, n = 1, None
        elif c == "?":
            m, n = 0, 1
        elif c == "{":
            q = self.brace(self.i)
            if not q:
                return atom                                     # a literal brace, as in Python
            m = int(q.group(1) or 0)
            n = (int(q.group(3)) if q.group(3) else None) if q.group(2) else m
            if n is not None and n < m:
                self.fail("min repeat greater than max repeat")
            self.i += q.end() - 1
        else:
            return atom
        self.i += 1
        if self.p[self.i:self.i + 1] in ("?", "+"):
            self.fail("lazy and possessive quantifiers are not supported")
        if self.p[self.i:self.i + 1] == "*" or self.brace(self.i):
            self.fail("multiple repeat")
        if max(m, n or 0) > REGEX_MAX_NFA_STATES:
            self.fail(f"a repetition above the limit of {REGEX_MAX_NFA_STATES} states", here)
        return ("rep", atom, m, n)


class _Nfa:
    """Thompson's construction: a state has epsilon moves and at most one move over a set of bytes"""

    def __init__(self, parser: _Regex):
        self.eps: List[list] = []
        self.on: List[Optional[frozenset]] = []
        self.to: List[int] = []
        self.parser = parser

    def state(self) -> int:
        if len(self.eps) >= REGEX_MAX_NFA_STATES:
            self.parser.fail(f"the pattern expands above the limit of {REGEX_MAX_NFA_STATES} states", len(self.parser.p))
        self.eps.append([])
        self.on.append(None)
        self.to.append(-1)
        return len(self.eps) - 1

    def build(self, node, a: int) -> int:
        """the fragment of `node` from state a; returns its end state"""
        kind = node[0]
        if kind == "set":
            b = self.state()
            self.on[a], self.to[a] = node[1], b
            return b
        if kind == "cat":
            for item in node[1]:
                mid = self.state()
                self.eps[a].append(mid)
                a = self.build(item, mid)
            return a
        if kind == "alt":
            end = self.state()
            for br in node[1]:
                s = self.state()
                self.eps[a].append(s)
                self.eps[self.build(br, s)].append(end)
            return end
        _, sub, m, n = node
        for _ in range(m):
            s = self.state()
            self.eps[a].append(s)
            a = self.build(sub, s)
        if n is None:
            s, end = self.state(), self.state()
            self.eps[a] += [s, end]
            e = self.build(sub, s)
            self.eps[e] += [s, end]
            return end
        end = self.state()
        for _ in range(n - m):
            self.eps[a].append(end)
            s = self.state()
            self.eps[a].append(s)
            a = self.build(sub, s)
        self.eps[a].append(end)
        return end


def regex_dfa(pattern: str):
    """A minimised byte DFA (trans[S][256] of int32 with -1 for no transition, start, accepting) that accepts exactly the UTF-8
    encodings of the strings `pattern` fully matches, for Automaton.from_byte_dfa / SparseAutomaton.from_byte_dfa.  Syntax: literals
    and backslash-escaped metacharacters, \\d \\w \\s \\D \\W \\S \\n \\t \\r \\f \\v \\xHH, ., [...] and [^...] with ranges, (...) and (?:...),
    |, * + ? {m} {m,} {m,n}.  The meaning is that of Python's re under re.ASCII: \\d \\w \\s are ASCII classes.  A non-ASCII literal
    enters as its UTF-8 bytes; ., a negated class and \\D \\W \\S match ONE WHOLE WELL-FORMED UTF-8 CODE POINT outside the excluded
    set (. excludes \\n alone), so no accepted string ends inside a code point.  ValueError, with the position: a non-ASCII character
    inside a class, anchors, backreferences, lookaround, lazy or possessive quantifiers, and a pattern that expands above
    REGEX_MAX_NFA_STATES NFA states or REGEX_MAX_DFA_STATES DFA states."""
    parser = _Regex(pattern)
    tree = parser.parse()
    nfa = _Nfa(parser)
    import sys
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 20_000))
    try:
        first = nfa.state()
        last = nfa.build(tree, first)
    finally:
        sys.setrecursionlimit(limit)
    # bytes that no set tells apart behave alike: one representative each
    sets = sorted({s for s in nfa.on if s is not None}, key=sorted)
    sig = np.zeros(256, dtype=object)
    for k, st in enumerate(sets):
        for b in st:
            sig[b] += 1 << k
    reps, cls_of = {}, np.zeros(256, dtype=np.int64)
    for b in range(256):
        cls_of[b] = reps.setdefault(sig[b], len(reps))
    rep_of = {}
    for b in range(256):
        rep_of.setdefault(int(cls_of[b]), b)
    C = len(reps)

    def closure(states):
        seen, todo = set(states), list(states)
        while todo:
            for t in nfa.eps[todo.pop()]:
                if t not in seen:
                    seen.add(t)
                    todo.append(t)
        return frozenset(seen)
    start_set = closure([first])
    ids, order, rows = {start_set: 0}, [start_set], []
    at = 0
    while at < len(order):
        cur = order[at]
        at += 1
        row = [-1] * C
        movers = [s for s in cur if nfa.on[s] is not None]
        for c in range(C):
            if sig[rep_of[c]] == 0:
                continue
            b = rep_of[c]
            moved = [nfa.to[s] for s in movers if b in nfa.on[s]]
            if not moved:
                continue
            nxt = closure(moved)
            if nxt not in ids:
                if len(order) >= REGEX_MAX_DFA_STATES:
                    parser.fail(f"the pattern expands above the limit of {REGEX_MAX_DFA_STATES} DFA states", len(pattern))
                ids[nxt] = len(order)
                order.append(nxt)
            row[c] = ids[nxt]
        rows.append(row)
    S = len(order)
    T = np.array(rows, dtype=np.int64).reshape(S, C)
    accept = np.array([last in st for st in order], dtype=bool)
    # states that reach no accepting state lead nowhere
    live = _live_states(T, np.flatnonzero(accept).tolist()) if C else accept.copy()
    T = np.where((T >= 0) & np.append(live, False)[T], T, S)                  # state S: the sink
    T = np.concatenate([T, np.full((1, C), S, dtype=np.int64)])
    # Moore's refinement: split blocks by where every byte class leads until nothing splits
    label = np.append(accept.astype(np.int64), 2)
    while True:
        keys = np.concatenate([label[:, None], label[T]], axis=1)
        _, new = np.unique(keys, axis=0, return_inverse=True)
        new = new.reshape(-1)
        split = int(new.max()) + 1 > len(np.unique(label))
        label = new
        if not split:
            break
    # number the blocks from the start state in breadth-first order; the sink's block gets no number
    sink = int(label[S])
    member = {}
    for s in range(S + 1):
        member.setdefault(int(label[s]), s)
    names, todo = {int(label[0]): 0}, [int(label[0])]
    out = []
    k = 0
    while k < len(todo):
        blk = todo[k]
        k += 1
        row = np.full(C, -1, dtype=np.int32)
        for c in range(C):
            to = int(label[T[member[blk], c]])
            if to == sink:
                continue
            if to not in names:
                names[to] = len(todo)
                todo.append(to)
            row[c] = names[to]
        out.append(row)
    small = np.array(out, dtype=np.int32).reshape(len(todo), C)
    trans = small[:, cls_of] if C else np.full((len(todo), 256), -1, dtype=np.int32)
    accepting = [names[b] for b in todo if member[b] < S and accept[member[b]]]
    return np.ascontiguousarray(trans, dtype=np.int32), 0, sorted(accepting)


def merge_guides(guide, n_requests: int):
    """generate_many's `guide` as the (next, start) of Transformer.set_guide: one Automaton for all requests gives its table and one
    start state; a sequence with one entry per request (None: unguided, start -1) gives the tables of the distinct automata one
    behind the other, the state numbers of each shifted by the states in front of it, and one start state per request.  With a
    SparseAutomaton among them the result is (a SparseAutomaton of all states, start) for Transformer.set_guide_sparse: the dense
    ones enter through SparseAutomaton.from_dense, the edges are concatenated."""
    if isinstance(guide, Automaton):
        return guide.next, [guide.start]
    if isinstance(guide, SparseAutomaton):
        return guide, [guide.start]
    guides = list(guide)
    if len(guides) != n_requests:
        raise ValueError(f"guide: {len(guides)} values for {n_requests} requests")
    if any(g is not None and not isinstance(g, (Automaton, SparseAutomaton)) for g in guides):
        raise TypeError("guide: an Automaton or a SparseAutomaton, or a sequence of them or None")
    sparse = any(isinstance(g, SparseAutomaton) for g in guides)
    distinct, tables, at = {}, [], 0
    for g in guides:
        if g is None or id(g) in distinct:
            continue
        if tables and g.vocab_size != tables[0].vocab_size:
            raise ValueError("guide: automata over different vocabularies")
        distinct[id(g)] = at
        tables.append(SparseAutomaton.from_dense(g) if sparse and isinstance(g, Automaton) else g)
        at += g.n_states
    if not tables:
        raise ValueError("guide: every request is unguided; pass guide=None")
    start = [-1 if g is None else distinct[id(g)] + g.start for g in guides]
    if sparse:
        if at > GUIDE_SPARSE_MAX_STATES:
            raise ValueError(f"guide: {at} states in all, at most {GUIDE_SPARSE_MAX_STATES}")
        shift = lambda a, by: np.where(a >= 0, a.astype(np.int64) + by, -1)
        bases = np.cumsum([0] + [t.n_states for t in tables[:-1]])
        edges = np.cumsum([0] + [t.n_edges for t in tables])
        return SparseAutomaton(np.concatenate([shift(t.default, b) for t, b in zip(tables, bases)]),
                               np.concatenate([t.offsets[:-1] + e for t, e in zip(tables, edges)] + [edges[-1:]]),
                               np.concatenate([t.tokens for t in tables]), np.concatenate([shift(t.targets, b) for t, b in zip(tables, bases)]),
                               0, tables[0].vocab_size, dead_ok=any(t.dead_ok for t in tables)), start
    if at > GUIDE_MAX_STATES:
        raise ValueError(f"guide: {at} states in all, at most {GUIDE_MAX_STATES}")
    bases = np.cumsum([0] + [t.n_states for t in tables[:-1]])
    return np.concatenate([np.where(t.next >= 0, t.next.astype(np.int32) + b, -1) for t, b in zip(tables, bases)]).astype(np.int16), start
