"""Guided decoding (include/qwen3_hip.h section 2r) restated on the host.  Helper module of tests/test_guide_host.py (CPU) and
tests/test_guide.py (GPU); not a conftest.

The rule: a guide is a table next[n_states][V] (>= 0: allowed, the state behind the token; -1: forbidden) and a list of start
states.  Request r in state s takes its output y_g from the MASKED row m of its classifier row l: the bits of l[v] where
next[s][v] >= 0, the bits of -inf (0xFF800000) elsewhere.  Section 2q's list (bias_ref.rule) then applies to m in place of l, section
2p's penalties on top.  After the commit the state is next[s][y_g] where that is >= 0, else it stays.  A start state of -1 leaves
the request unguided.

  mask        the mask on the bits;
  rule        mask, then bias_ref.rule;
  step        the state step, with its stay-put branch;
  state_of    the state behind a request's tokens so far;
  request     one request's tokens: pen_ref.request over rows masked in the state its tokens so far lead to, then adjusted;
  rows        what a generate_many_* call gives for these requests under a guide (next, start) and a table, over a pen_ref.Engine."""
from __future__ import annotations

import hashlib

import numpy as np

import bias_ref as br
import pen_ref as pr

NEG_INF_BITS = 0xFF800000


def mask(logits, next_row):
    l = np.ascontiguousarray(logits, dtype=np.float32)
    nx = np.asarray(next_row)
    assert nx.shape == l.shape
    return np.where(nx >= 0, l.view(np.uint32), np.uint32(NEG_INF_BITS)).astype(np.uint32).view(np.float32)


def rule(logits, next_row, entries=(), mode=br.ADD, g=0, counts=None, presence=0.0, frequency=0.0):
    return br.rule(mask(logits, next_row), entries, mode, g, counts, presence, frequency)


def step(next, s, token):
    """s_{g+1}: next[s][token] where that is >= 0, else s; an unguided request (-1) stays unguided"""
    if s < 0:
        return s
    to = int(next[s][token])
    return to if to >= 0 else s


def state_of(next, start, tokens):
    s = start
    for t in tokens:
        s = step(next, s, t)
    return s


def start_of(guide, r):
    """the start state of request r under a guide (next, start); None: unguided"""
    if guide is None:
        return -1
    start = guide[1]
    return int(start[0] if len(start) == 1 else start[r])


def request(row_of, draw, prompt, n_new, next, start, entries=(), mode=br.ADD, presence=0.0, frequency=0.0, temperature=0.0, topp=1.0, seed=0,
            burn=0, stop=()):
    """pen_ref.request over masked and adjusted rows: the mask of the state the tokens so far lead to, the bias, the penalties on
    top.  The state is walked on the host from `start` over the request's own outputs."""
    n_prompt = len(prompt)

    def row(seq):
        raw, produced = row_of(seq), seq[n_prompt:]
        s = state_of(next, start, produced)
        return br.adjust(raw if s < 0 else mask(raw, next[s]), entries, mode, len(produced))
    return pr.request(row, draw, prompt, n_new, presence, frequency, temperature, topp, seed, burn, stop)


def digest(guide):
    if guide is None:
        return None
    return hashlib.blake2b(np.ascontiguousarray(guide[0], dtype=np.int16).tobytes(), digest_size=16).digest()


def rows(ref, prompts, n_new, guide=None, table=None, presence=0.0, frequency=0.0, sampler=None, prefix=(), stop=()):
    """The rows of a generate_many_* call under `guide` (next, start) and `table` (lists, modes), request by request over the
    single-stream engine ref (pen_ref.Engine); a request ends with its first stop token.  Computed once per request and setting."""
    out, d = [], digest(guide)
    for r, (p, n) in enumerate(zip(prompts, n_new)):
        at = lambda v: v[r] if np.ndim(v) else v
        T, tp, seed = (0.0, 1.0, 0) if sampler is None else (at(sampler[0]), at(sampler[1]), sampler[2][r])
        entries, mode = br.list_of(table, r)
        s0 = start_of(guide, r)
        key = ("guide", d if s0 >= 0 else None, s0, tuple(prefix), tuple(p), n, tuple(tuple(e) for e in entries), mode, float(presence), float(frequency),
               float(T), float(tp), int(seed), ref.top_k, tuple(sorted(stop)))
        if key not in ref.memo:
            ref.memo[key] = request(lambda seq: ref.row_of(list(prefix) + seq), ref.draw, p, n, None if guide is None else guide[0], s0, entries, mode,
                                    presence, frequency, float(T), float(tp), int(seed), burn=len(prefix), stop=tuple(stop))[0]
        out.append(list(ref.memo[key]))
    return out
