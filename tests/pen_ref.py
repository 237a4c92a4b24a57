"""Presence and frequency penalties (include/qwen3_hip.h section 2p) restated on the host.  Helper module of
tests/test_penalty_host.py (CPU) and tests/test_penalty.py (GPU); not a conftest.

The rule: a request that has produced token v c[v] > 0 times takes its next token from
    l'[v] = l[v] - (presence + frequency * (float)c[v])
with the multiply, the add and the subtract each rounded to float32 (numpy rounds every float32 operation on its own and fuses
nothing); an entry with c[v] == 0 keeps its bits.  The token is the index of the largest key (total_order_key(l'[v]) << 32) | v, or
the sampler's draw over l'.

  penalize       the rule on a vector;
  penalize_fma   the same with the multiply and the add fused (one rounding): what a kernel built with contraction would compute;
  argmax_key     the largest-key argmax;
  request        one request's tokens, given a function from the tokens so far to the classifier row and a function that draws;
  Engine         those two functions over a single-stream engine: forward() rows copied, ops.sample / ops.sample_top_k for the draws,
                 under the coin rules of section 2f (one discarded coin per prompt position but the last, one coin per draw, none at
                 temperature 0)."""
from __future__ import annotations

import numpy as np

from logit_ckpt import first_coin, total_order_key

f32 = np.float32


def keys_of(logits):
    l = np.ascontiguousarray(logits, dtype=np.float32)
    return (total_order_key(l).astype(np.uint64) << np.uint64(32)) | np.arange(l.size, dtype=np.uint64)


def argmax_key(logits) -> int:
    return int(np.argmax(keys_of(logits)))


def penalize(logits, counts, presence, frequency):
    l = np.ascontiguousarray(logits, dtype=np.float32)
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    with np.errstate(all="ignore"):
        m = (f32(frequency) * c.astype(np.float32)).astype(np.float32)          # rounded
        p = (f32(presence) + m).astype(np.float32)                              # rounded
        out = (l - p).astype(np.float32)                                        # rounded
    return np.where(c > 0, out.view(np.uint32), l.view(np.uint32)).view(np.float32)


def penalize_fma(logits, counts, presence, frequency):
    """presence + frequency * c with ONE rounding (exact in float64: 24 x 24 bits of product plus a 24-bit addend within 2^29 of
    it), then the subtraction"""
    l = np.ascontiguousarray(logits, dtype=np.float32)
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    p = (np.float64(f32(presence)) + np.float64(f32(frequency)) * c.astype(np.float32).astype(np.float64)).astype(np.float32)
    with np.errstate(all="ignore"):
        out = (l - p).astype(np.float32)
    return np.where(c > 0, out.view(np.uint32), l.view(np.uint32)).view(np.float32)


def fma_triple(limit=1 << 12):
    """(frequency, c, presence) for which the fused form rounds to another float32 than the rule: searched, not listed"""
    rng = np.random.Generator(np.random.PCG64(2024))
    for _ in range(limit):
        fr = f32(rng.uniform(0.1, 2.0))
        pr = f32(rng.uniform(0.1, 2.0))
        c = int(rng.integers(3, 1 << 20))
        one = np.zeros(1, dtype=np.float32)
        a = penalize(one, [c], pr, fr)
        b = penalize_fma(one, [c], pr, fr)
        if a.tobytes() != b.tobytes():
            return float(fr), c, float(pr)
    raise AssertionError("no triple found")


def request(row_of, draw, prompt, n_new, presence, frequency, temperature=0.0, topp=1.0, seed=0, burn=0, stop=()):
    """The tokens of one request.  row_of(tokens so far) -> the classifier row behind them; draw(row, temperature, topp, rng) ->
    (token, rng).  burn: coins discarded in front of the prompt (a shared prefix).  Returns (tokens, rng behind them, the largest
    count reached, did a penalised row differ from its raw row)."""
    seq = list(prompt)
    rng = seed
    if temperature > 0.0:
        for _ in range(burn + len(prompt) - 1):
            rng = first_coin(rng)[1]
    counts = None
    out, differs = [], False
    for _ in range(n_new):
        raw = np.array(row_of(seq), dtype=np.float32, copy=True)
        if counts is None:
            counts = np.zeros(raw.size, dtype=np.uint32)
        row = penalize(raw, counts, presence, frequency)
        differs = differs or row.tobytes() != raw.tobytes()
        if temperature > 0.0:
            tok, rng = draw(row, temperature, topp, rng)
        else:
            tok = argmax_key(row)
        counts[tok] += 1
        out.append(int(tok))
        seq.append(int(tok))
        if tok in stop:
            break
    return out, rng, int(counts.max()), differs


class Engine:
    """row_of and draw over a single-stream engine of the package (GPU)"""

    def __init__(self, q3, path, ctx=None, top_k=0):
        b = q3.TransformerBuilder(path)
        self.t = (b.with_ctx_length(ctx) if ctx else b).build()
        self.ops, self.top_k = q3.ops, top_k
        self.fed = []                   # the tokens whose cache rows the engine holds
        self.memo = {}

    def close(self):
        self.t.close()

    def row_of(self, seq):
        """forward() of the tokens whose cache rows the engine does not hold yet; the row behind the last one"""
        same = 0
        while same < min(len(self.fed), len(seq) - 1) and self.fed[same] == seq[same]:
            same += 1
        row = None
        for pos in range(same, len(seq)):
            row = self.t.forward(seq[pos], pos)
        self.fed = list(seq)
        return np.array(row, dtype=np.float32, copy=True)

    def draw(self, row, temperature, topp, rng):
        if self.top_k:
            return self.ops.sample_top_k(row, temperature, topp, self.top_k, rng)
        return self.ops.sample(row, temperature, topp, rng)

    def rows(self, prompts, n_new, presence, frequency, sampler=None, prefix=(), stop=()):
        """what a generate_many_* call gives for these requests: (rows, the largest count, did any penalised row differ)"""
        out, top, differs = [], 0, False
        for r, (p, n) in enumerate(zip(prompts, n_new)):
            at = lambda v: v[r] if np.ndim(v) else v
            T, tp, seed = (0.0, 1.0, 0) if sampler is None else (at(sampler[0]), at(sampler[1]), sampler[2][r])
            # computed once per request and setting, shared among the loops; a stop token cuts the free-running row
            key = (tuple(prefix), tuple(p), n, float(presence), float(frequency), float(T), float(tp), int(seed), self.top_k)
            if key not in self.memo:
                self.memo[key] = request(lambda seq: self.row_of(list(prefix) + seq), self.draw, p, n, presence, frequency, float(T), float(tp),
                                         int(seed), burn=len(prefix))
            toks, _, c, d = self.memo[key]
            cut = next((i for i, tok in enumerate(toks) if tok in stop), None)
            if cut is not None:
                toks = toks[:cut + 1]
                c = int(np.bincount(toks).max())
            out.append(list(toks))
            top = max(top, c)
            differs = differs or d
        return out, top, differs
