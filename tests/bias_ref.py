"""Logit bias, banned and allowed tokens (include/qwen3_hip.h section 2q) restated on the host.  Helper module of
tests/test_bias_host.py (CPU) and tests/test_bias.py (GPU); not a conftest.

The rule: request r takes its output y_g from the ADJUSTED row a of its classifier row l.  An entry (token, bias, until) of its list
is active when until == 0 or g < until; a listed, active token with a bias other than +-0 gets l[v] + bias, rounded to float32 once;
every other listed token and, under ADD, every unlisted one keeps its bits; under ALLOW an unlisted token becomes -inf.  Section
2p's penalties (pen_ref.penalize) then apply to a in place of l.

  adjust      the rule on a vector;
  rule        adjust, then the penalties where counts are given;
  request     one request's tokens: pen_ref.request over rows adjusted with g = len(tokens so far) - len(prompt);
  rows        what a generate_many_* call gives for these requests under a table (lists, modes), over a pen_ref.Engine."""
from __future__ import annotations

import numpy as np

import pen_ref as pr

f32 = np.float32
ADD, ALLOW = 0, 1
NEG_INF_BITS = 0xFF800000


def adjust(logits, entries, mode, g):
    l = np.ascontiguousarray(logits, dtype=np.float32)
    out = l.view(np.uint32).copy()
    entries = list(entries)
    tokens = np.array([e[0] for e in entries], dtype=np.int64)
    bias = np.array([e[1] for e in entries], dtype=np.float32)
    until = np.array([e[2] if len(e) > 2 else 0 for e in entries], dtype=np.int64)
    assert len(set(tokens.tolist())) == len(entries), "a token twice in one list"
    if len(entries):
        act = ((until == 0) | (g < until)) & (bias != 0)                        # +-0: the bits stay
        with np.errstate(all="ignore"):
            summed = (l[tokens[act]] + bias[act]).astype(np.float32)           # one rounding
        out[tokens[act]] = summed.view(np.uint32)
    if mode == ALLOW:
        unlisted = np.ones(l.size, dtype=bool)
        unlisted[tokens] = False
        out[unlisted] = NEG_INF_BITS
    return out.view(np.float32)


def rule(logits, entries, mode, g, counts=None, presence=0.0, frequency=0.0):
    a = adjust(logits, entries, mode, g)
    return a if counts is None else pr.penalize(a, counts, presence, frequency)


def order_triple(limit=1 << 14):
    """(l, bias, presence) for which bias-then-penalty rounds to another float32 than penalty-then-bias: searched, not listed"""
    rng = np.random.Generator(np.random.PCG64(2025))
    for _ in range(limit):
        l, b, p = f32(rng.uniform(-8, 8)), f32(rng.uniform(0.1, 100.0)), f32(rng.uniform(0.1, 2.0))
        one = np.array([l], dtype=np.float32)
        first = rule(one, [(0, b, 0)], ADD, 0, [1], p, 0.0)
        other = adjust(pr.penalize(one, [1], p, 0.0), [(0, b, 0)], ADD, 0)
        if first.tobytes() != other.tobytes():
            return float(l), float(b), float(p)
    raise AssertionError("no triple found")


def list_of(table, r):
    """(entries, mode) of request r under a table (lists, modes); None or no list: the empty ADD list"""
    if not table or not table[0]:
        return [], ADD
    lists, modes = table
    i = 0 if len(lists) == 1 else r
    return lists[i], (modes[i] if modes is not None else ADD)


def request(row_of, draw, prompt, n_new, entries, mode, presence=0.0, frequency=0.0, temperature=0.0, topp=1.0, seed=0, burn=0, stop=()):
    """pen_ref.request over adjusted rows: bias first, penalties on top.  row_of sees whatever stands in front of the prompt itself
    (a shared prefix is the caller's closure), so the output index is len(seq) - len(prompt)."""
    n_prompt = len(prompt)
    return pr.request(lambda seq: adjust(row_of(seq), entries, mode, len(seq) - n_prompt), draw, prompt, n_new, presence, frequency, temperature,
                      topp, seed, burn, stop)


def rows(ref, prompts, n_new, table=None, presence=0.0, frequency=0.0, sampler=None, prefix=(), stop=()):
    """The rows of a generate_many_* call under `table`, request by request over the single-stream engine ref (pen_ref.Engine); a
    request ends with its first stop token.  Computed once per request and setting."""
    out = []
    for r, (p, n) in enumerate(zip(prompts, n_new)):
        at = lambda v: v[r] if np.ndim(v) else v
        T, tp, seed = (0.0, 1.0, 0) if sampler is None else (at(sampler[0]), at(sampler[1]), sampler[2][r])
        entries, mode = list_of(table, r)
        key = ("bias", tuple(prefix), tuple(p), n, tuple(tuple(e) for e in entries), mode, float(presence), float(frequency), float(T), float(tp),
               int(seed), ref.top_k, tuple(sorted(stop)))
        if key not in ref.memo:
            ref.memo[key] = request(lambda seq: ref.row_of(list(prefix) + seq), ref.draw, p, n, entries, mode, presence, frequency, float(T), float(tp),
                                    int(seed), burn=len(prefix), stop=tuple(stop))[0]
        out.append(list(ref.memo[key]))
    return out
