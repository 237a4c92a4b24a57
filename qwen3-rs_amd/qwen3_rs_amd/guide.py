"""Guided decoding on the host side (include/qwen3_hip.h section 2r): token automata as Transformer.set_guide and
generate_many(guide=...) take them, and two ways to build one -- a trie over token sequences, and the lift of a byte-level DFA to
the tokens of a vocabulary, the seam for a regular-expression or JSON-schema compiler."""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

GUIDE_MAX_STATES = 4096   # Q3_GUIDE_MAX_STATES


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


def merge_guides(guide, n_requests: int):
    """generate_many's `guide` as the (next, start) of Transformer.set_guide: one Automaton for all requests gives its table and one
    start state; a sequence with one entry per request (None: unguided, start -1) gives the tables of the distinct automata one
    behind the other, the state numbers of each shifted by the states in front of it, and one start state per request."""
    if isinstance(guide, Automaton):
        return guide.next, [guide.start]
    guides = list(guide)
    if len(guides) != n_requests:
        raise ValueError(f"guide: {len(guides)} values for {n_requests} requests")
    if any(g is not None and not isinstance(g, Automaton) for g in guides):
        raise TypeError("guide: an Automaton, or a sequence of Automaton or None")
    distinct, tables, at = {}, [], 0
    for g in guides:
        if g is None or id(g) in distinct:
            continue
        if tables and g.vocab_size != tables[0].shape[1]:
            raise ValueError("guide: automata over different vocabularies")
        distinct[id(g)] = at
        tables.append(np.where(g.next >= 0, g.next.astype(np.int32) + at, -1))
        at += g.n_states
    if not tables:
        raise ValueError("guide: every request is unguided; pass guide=None")
    if at > GUIDE_MAX_STATES:
        raise ValueError(f"guide: {at} states in all, at most {GUIDE_MAX_STATES}")
    start = [-1 if g is None else distinct[id(g)] + g.start for g in guides]
    return np.concatenate(tables).astype(np.int16), start
