"""Stop sequences (include/qwen3_hip.h section 2t): the host compilers of the stop automaton Transformer.set_stop_sequences takes.

A stop automaton is a guide.SparseAutomaton read differently: next[s][v] == -1 says "token v completes a sequence in state s, the
request ends with it", and every other target is the state behind the token.  SparseAutomaton.walk returns the index of the first
token whose target is -1, which is the reference reading of the rule: a row ends with that token.
stop_automaton compiles token sequences (Aho-Corasick over tokens), stop_automaton_from_strings compiles strings over the bytes
of a vocabulary, so that a stop string may end inside a token or span several tokens under any tokenisation.
"""
from collections import deque
from typing import Iterable, List, Optional, Sequence

import numpy as np

from .guide import SparseAutomaton, _compress, merge_guides

STOP_SEQ_MAX_STATES = 1 << 16       # Q3_STOP_SEQ_MAX_STATES
STOP_SEQ_MAX_EDGES = 1 << 24        # Q3_STOP_SEQ_MAX_EDGES


def _checked(a: SparseAutomaton) -> SparseAutomaton:
    if a.n_states > STOP_SEQ_MAX_STATES:
        raise ValueError(f"{a.n_states} states, a stop automaton holds at most {STOP_SEQ_MAX_STATES}")
    if a.n_edges > STOP_SEQ_MAX_EDGES:
        raise ValueError(f"{a.n_edges} edges, a stop automaton holds at most {STOP_SEQ_MAX_EDGES}")
    return a


def _aho_corasick(seqs: Sequence[Sequence[int]]):
    """The trie of seqs with failure links resolved into a DFA: (trans, done).  trans[s] maps every symbol on s's failure chain to
    its target (every other symbol leads to the root, state 0); done[s]: a sequence ends in s or in a state on its failure chain
    (the output links)."""
    children: List[dict] = [{}]
    done = [False]
    for q in seqs:
        at = 0
        for t in q:
            if t not in children[at]:
                children.append({})
                done.append(False)
                children[at][t] = len(children) - 1
            at = children[at][t]
        done[at] = True
    fail = [0] * len(children)
    trans: List[Optional[dict]] = [None] * len(children)
    trans[0] = dict(children[0])
    todo = deque(children[0].values())
    while todo:                                     # breadth first: a state's failure target is shallower and resolved before it
        s = todo.popleft()
        trans[s] = dict(trans[fail[s]])
        for t, c in children[s].items():
            fail[c] = trans[fail[s]].get(t, 0)
            done[c] = done[c] or done[fail[c]]
            todo.append(c)
        trans[s].update(children[s])
    return trans, done


def stop_automaton(token_seqs: Iterable[Sequence[int]], vocab_size: int) -> SparseAutomaton:
    """The stop automaton of token sequences: a row ends with the first token that completes any of them (plain sub-list search, every
    overlap included: Aho-Corasick as a full DFA).  Per state the default is the most frequent target -- the root unless the
    vocabulary is tiny -- and the edges are the tokens along the failure chain with resolved targets, -1 where the token completes a
    sequence, output links included.  ValueError: no sequence, an empty one, one given twice, a token outside the vocabulary."""
    seqs = [tuple(int(t) for t in q) for q in token_seqs]
    if isinstance(vocab_size, bool) or not isinstance(vocab_size, (int, np.integer)) or not 0 < vocab_size < 2 ** 31:
        raise ValueError(f"vocab_size must be an integer in 1 .. 2^31 - 1, got {vocab_size!r}")
    V = int(vocab_size)
    if not seqs or any(len(q) == 0 for q in seqs):
        raise ValueError("stop sequences: at least one, none of them empty")
    if len(set(seqs)) != len(seqs):
        raise ValueError("stop sequences: a sequence is given twice")
    if any(not 0 <= t < V for q in seqs for t in q):
        raise ValueError(f"a token lies outside the vocabulary of {V}")
    trans, done = _aho_corasick(seqs)
    # the states a row can be in: reached from the root without completing a sequence, numbered in the order they are found
    number, order = {0: 0}, [0]
    for s in order:
        for t in sorted(trans[s]):
            to = trans[s][t]
            if not done[to] and to not in number:
                number[to] = len(order)
                order.append(to)
    if len(order) > STOP_SEQ_MAX_STATES:
        raise ValueError(f"{len(order)} states, a stop automaton holds at most {STOP_SEQ_MAX_STATES}")
    rows = []
    for s in order:
        items = sorted(trans[s].items())
        toks = np.array([t for t, _ in items], dtype=np.int32)
        tgts = np.array([-1 if done[to] else number[to] for _, to in items], dtype=np.int32)
        counts = np.bincount(tgts + 1, minlength=2)
        counts[1] += V - toks.size                  # the unlisted tokens lead to the root
        default = int(counts.argmax()) - 1
        if default == 0:
            keep = tgts != 0
            rows.append((0, toks[keep], tgts[keep]))
        else:                                       # a tiny vocabulary: the root is not the most frequent target
            row = np.zeros(V, dtype=np.int32)
            row[toks] = tgts
            rows.append(_compress(row))
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([r[1].size for r in rows], out=offsets[1:])
    cat = lambda k: np.concatenate([r[k] for r in rows])
    return _checked(SparseAutomaton(np.array([r[0] for r in rows], dtype=np.int32), offsets, cat(1), cat(2), 0, V, dead_ok=True))


def stop_automaton_from_strings(strings: Iterable, token_bytes: Sequence[bytes]) -> SparseAutomaton:
    """The stop automaton of strings over a vocabulary whose token v spells token_bytes[v]: a row ends with the first token inside or
    at the end of which the row's bytes contain one of the strings -- a stop string may end inside a token, or span several tokens
    under any tokenisation.  A byte-level Aho-Corasick DFA over the UTF-8 bytes of the strings (bytes are taken as they are) is
    lifted to the tokens: from state s token t runs its bytes, the target is -1 if any byte position on the way reaches an accepting
    state, else the state behind the last byte; a token of zero bytes leaves the state where it is.  Vectorised over the tokens per
    byte position, as SparseAutomaton.from_byte_dfa is.  ValueError: no string, an empty one, one given twice."""
    pats = [bytes(p) if isinstance(p, (bytes, bytearray)) else str(p).encode("utf-8") for p in strings]
    if not pats or any(len(p) == 0 for p in pats):
        raise ValueError("stop strings: at least one, none of them empty")
    if len(set(pats)) != len(pats):
        raise ValueError("stop strings: a string is given twice")
    V = len(token_bytes)
    if not 0 < V < 2 ** 31:
        raise ValueError(f"a vocabulary of {V} tokens: 1 .. 2^31 - 1")
    trans, done = _aho_corasick([tuple(p) for p in pats])
    S = len(trans)
    T = np.zeros((S, 256), dtype=np.int32)          # the full byte DFA: an unlisted byte leads to the root
    for s, row in enumerate(trans):
        for b, to in row.items():
            T[s, b] = to
    acc = np.array(done, dtype=bool)
    lens = np.fromiter((len(b) for b in token_bytes), dtype=np.int64, count=V)
    by_len = np.argsort(-lens, kind="stable")       # tokens of at least i + 1 bytes: by_len[:n_at[i]]
    Lmax = int(lens.max())
    n_at = [int(np.count_nonzero(lens > i)) for i in range(Lmax)]
    B = np.zeros((V, max(Lmax, 1)), dtype=np.uint8)
    flat = np.frombuffer(b"".join(bytes(token_bytes[v]) for v in range(V) if lens[v]), dtype=np.uint8)
    has = np.flatnonzero(lens)
    B[np.repeat(has, lens[has]), np.arange(flat.size) - np.repeat(np.cumsum(lens[has]) - lens[has], lens[has])] = flat
    cols = [np.ascontiguousarray(B[by_len[:n_at[i]], i]) for i in range(Lmax)]      # in the order of by_len
    number, order, rows = {0: 0}, [0], []
    names = np.full(S, -1, dtype=np.int32)
    names[0] = 0
    at = 0
    while at < len(order):
        s = order[at]
        at += 1
        cur = np.full(V, s, dtype=np.int32)         # in the order of by_len: the tokens on their way are in front
        hit = np.zeros(V, dtype=bool)
        for i in range(Lmax):
            n = n_at[i]
            cur[:n] = T[cur[:n], cols[i]]
            hit[:n] |= acc[cur[:n]]
        to = np.empty(V, dtype=np.int32)
        to[by_len] = np.where(hit, -1, cur)
        ok = np.flatnonzero(to >= 0)
        # new byte states in the order of the first token that reaches them
        found, where = np.unique(to[ok], return_index=True)
        for b in found[np.argsort(where, kind="stable")]:
            if int(b) not in number:
                number[int(b)] = names[b] = len(order)
                order.append(int(b))
                if len(order) > STOP_SEQ_MAX_STATES:
                    raise ValueError(f"more than {STOP_SEQ_MAX_STATES} states")
        row = np.full(V, -1, dtype=np.int32)
        row[ok] = names[to[ok]]
        rows.append(_compress(row))
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([r[1].size for r in rows], out=offsets[1:])
    cat = lambda k: np.concatenate([r[k] for r in rows])
    return _checked(SparseAutomaton(np.array([r[0] for r in rows], dtype=np.int32), offsets, cat(1), cat(2), 0, V, dead_ok=True))


def first_match(automaton: SparseAutomaton, start: int, tokens: Iterable[int]) -> Optional[int]:
    """SparseAutomaton.walk from a start state of the caller's: the index of the first token whose target is -1, None where there is
    none.  start -1: no stop sequences, None."""
    s = int(start)
    if s < 0:
        return None
    for i, t in enumerate(tokens):
        s = automaton.next_of(s, int(t))
        if s < 0:
            return i
    return None


def cut_at_stop(text, strings: Iterable):
    """`text` in front of the earliest occurrence of any of `strings` (str with str, bytes with bytes): the convention of serving APIs,
    which exclude the stop string from what they return.  No occurrence: the text as it is."""
    hits = [text.find(s) for s in strings]
    hits = [h for h in hits if h >= 0]
    return text[:min(hits)] if hits else text


_COMPILED: dict = {}


def _is_tokens(v) -> bool:
    return not isinstance(v, (str, bytes, bytearray)) and hasattr(v, "__iter__") and all(
        isinstance(t, (int, np.integer)) and not isinstance(t, bool) for t in v)


def _compile_one(spec, vocab_size: int, tokenizer):
    """one stop list -- a SparseAutomaton, strings, or token lists -- as a SparseAutomaton, compiled once per list and vocabulary"""
    if isinstance(spec, SparseAutomaton):
        return spec
    items = list(spec)
    if not items:
        raise ValueError("stop: an empty list; pass None for no stop sequences")
    if all(isinstance(x, (str, bytes, bytearray)) for x in items):
        if tokenizer is None:
            raise ValueError("stop strings need tokenizer=: a Tokenizer or anything with a list `vocab` of the tokens' bytes")
        key = ("s", tuple(items), id(tokenizer))
        if key not in _COMPILED:
            _COMPILED[key] = (stop_automaton_from_strings(items, tokenizer.vocab), tokenizer)
        return _COMPILED[key][0]
    if all(_is_tokens(x) for x in items):
        key = ("t", tuple(tuple(int(t) for t in x) for x in items), int(vocab_size))
        if key not in _COMPILED:
            _COMPILED[key] = (stop_automaton(items, vocab_size), None)
        return _COMPILED[key][0]
    raise TypeError("stop: a list of strings, a list of token lists, or a SparseAutomaton")


def compile_stop(stop, n_requests: int, vocab_size: int, tokenizer=None):
    """generate_many's `stop` as (SparseAutomaton, start) for Transformer.set_stop_sequences, or None where nothing is asked for: a
    list of strings (needs the tokenizer), a list of token lists or a SparseAutomaton holds for all requests and gives one start
    state; a sequence of one such value per request (None: no stop sequences for that request, start -1) gives the automata of the
    distinct values one behind the other (guide.merge_guides) and one start state per request."""
    if stop is None:
        return None
    if isinstance(stop, (str, bytes, bytearray)):
        raise TypeError("stop: a list of strings, not one string")
    if isinstance(stop, SparseAutomaton):
        return stop, [stop.start]
    items = list(stop)
    per_request = any(x is None or isinstance(x, SparseAutomaton) or (not isinstance(x, (str, bytes, bytearray)) and not _is_tokens(x)) for x in items)
    if not per_request:
        a = _compile_one(items, vocab_size, tokenizer)
        return a, [a.start]
    if len(items) != n_requests:
        raise ValueError(f"stop: {len(items)} values for {n_requests} requests")
    if all(x is None for x in items):
        return None
    table, start = merge_guides([None if x is None else _compile_one(x, vocab_size, tokenizer) for x in items], n_requests)
    return _checked(table), start
