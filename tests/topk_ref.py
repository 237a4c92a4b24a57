"""Top-k sampling (include/qwen3_hip.h section 2n) restated twice on the CPU.  Helper module of tests/test_topk_host.py (CPU) and
tests/test_topk.py (GPU); not a conftest.

The rule: a draw with top_k = k is the reference's Sampler::sample on the logits with every entry outside the survivor set replaced
by -inf; the survivors are the k largest entries under the key (total_order_key(logit) << 32) | index, so ties go to the higher
index.  One deviation: a multinomial walk that falls through returns the highest-index survivor, not the (masked) index V - 1.

  sample_top_k     the C oracle's Sampler.sample on the masked copy, plus the fall-through rule;
  sample_top_k_np  an independent restatement on the COMPACTED survivors: sequential float32 sums in numpy, libm's expf.
Both take and return the xorshift64* state as an int: (token, state behind the draw)."""
from __future__ import annotations

import numpy as np

from logit_ckpt import first_coin, total_order_key

f32 = np.float32
TOP_K_MAX = 64


def keys_of(logits):
    l = np.ascontiguousarray(logits, dtype=np.float32)
    return (total_order_key(l).astype(np.uint64) << np.uint64(32)) | np.arange(l.size, dtype=np.uint64)


def survivors(logits, k: int):
    """the indices of the k largest keys, ascending"""
    keys = keys_of(logits)
    top = np.argsort(keys, kind="stable")[keys.size - k:]
    return np.sort(top).astype(np.int64)


def masked(logits, k: int):
    l = np.ascontiguousarray(logits, dtype=np.float32)
    m = np.full(l.size, -np.inf, dtype=np.float32)
    s = survivors(l, k)
    m[s] = l[s]
    return m, s


def sample_top_k(oracle, logits, temperature: float, topp: float, k: int, rng: int):
    """the oracle's draw on the masked copy.  The fall-through of the multinomial walk shows as the oracle returning V - 1 while
    V - 1 is not a survivor"""
    l = np.ascontiguousarray(logits, dtype=np.float32)
    if temperature == 0.0:
        return oracle.sample_argmax(l), rng
    m, s = masked(l, k)
    smp = oracle.Sampler(l.size, temperature, topp, rng)
    tok = smp.sample(m)
    if tok == l.size - 1 and (l.size - 1) not in s:
        tok = int(s[-1])
    return int(tok), int(smp.rng_state.value)


def sample_top_k_np(npo, logits, temperature: float, topp: float, k: int, rng: int):
    """npo: oracle.np_oracle (its expf is libm's, the reference's).  Works on the survivors alone, in ascending index order"""
    l = np.ascontiguousarray(logits, dtype=np.float32)
    if temperature == 0.0:
        return int(np.argmax(keys_of(l))), rng
    V = l.size
    s = survivors(l, k)
    coin, state = first_coin(rng)
    T, topp = f32(temperature), f32(topp)
    x = (l[s] / T).astype(np.float32)
    mx = f32(l[int(np.argmax(keys_of(l)))] / T)
    with np.errstate(invalid="ignore"):
        e = npo.expf((x - mx).astype(np.float32))
    total = f32(-0.0)
    for v in e:
        total = f32(total + v)
    inv = f32(f32(1.0) / total)
    p = (e * inv).astype(np.float32)
    if not (f32(0.0) < topp < f32(1.0)):
        cdf = f32(0.0)
        for i, v in enumerate(p):
            cdf = f32(cdf + v)
            if coin < cdf:
                return int(s[i]), state
        return int(s[-1]), state
    cutoff = f32(f32(f32(1.0) - topp) / f32(max(V - 1, 1)))
    cand = np.nonzero(p >= cutoff)[0]
    if cand.size == 0:
        return 0, state
    order = cand[np.lexsort((cand, -p[cand].astype(np.float64)))]
    cumulative, last = f32(0.0), order.size - 1
    for i, c in enumerate(order):
        cumulative = f32(cumulative + p[c])
        if cumulative > topp:
            last = i
            break
    r = f32(coin * cumulative)
    cdf = f32(0.0)
    for i in range(last + 1):
        cdf = f32(cdf + p[order[i]])
        if r < cdf:
            return int(s[order[i]]), state
    return int(s[order[last]]), state


def loop(oracle, logits_of, tok0: int, temperature: float, topp: float, k: int, seed: int, n: int, burn: int = 0):
    """the sampled loop under top-k from tok0: `burn` discarded coins (prompt positions), then n draws, each the next input;
    logits_of(token) gives the logits behind a token.  k = 0: the plain sampler.  Returns (tokens, rng state behind them)"""
    rng = seed
    for _ in range(burn):
        rng = first_coin(rng)[1]
    tok, out = tok0, []
    for _ in range(n):
        if k:
            tok, rng = sample_top_k(oracle, logits_of(tok), temperature, topp, k, rng)
        else:
            smp = oracle.Sampler(1, temperature, topp, rng)
            tok = smp.sample(logits_of(tok))
            rng = int(smp.rng_state.value)
        out.append(tok)
    return out, rng


# A fall-through of the multinomial walk: 37 equal survivors have p = fl(1 / 37) each and a sequential float32 cdf that ends at
# 0.99999982 = 1 - 3 / 2^24, and the first coin of this xorshift64* state is 1 - 1 / 2^24 (found by a search over states
# 1 .. 10^7: COIN_HIGH_SEEDS of logit_ckpt.py lists the states whose first coin is that high).  tests/test_topk_host.py checks
# that it is one.
FALL_THROUGH_SEED = 1574392
FALL_THROUGH_K = 37
FALL_THROUGH_V = 2000


def fall_through_logits():
    """37 equal logits at scattered indices, the last of them not V - 1; everything else far below"""
    l = np.full(FALL_THROUGH_V, -30.0, dtype=np.float32)
    l[(np.arange(FALL_THROUGH_K) * 53 + 11) % (FALL_THROUGH_V - 1)] = 2.0
    return l
