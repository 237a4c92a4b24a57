"""ref64.py -- plain float64, order-free restatement of the operations tolerance mode (Q3_FLAG_FAST) reorders, with the
quantity each order-independent error budget is stated in.  TEST INFRASTRUCTURE ONLY (numpy; no device, no oracle import).

Written from the reference's semantics like oracle/np_oracle.py (citations into reinterpretcat/qwen3-rs: tensor.rs, layers.rs),
but where the oracles reproduce ONE summation order in float32, this file computes the real-number value of every sum in
float64 and returns, next to it, the sum of absolute values of its terms.

The acceptance rule (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2): with u = 2^-24 an f32 sum of m
terms evaluated in ANY order (any binary tree, the chain included) satisfies
        |fl(sum) - S| <= gamma(m - 1) * A,    gamma(k) = k u / (1 - k u),   S = sum t_i,   A = sum |t_i|.
Nothing here is measured on a device.  For m <= 16,384 f32 terms the float64 sum itself is off by at most m * 2^-53 * A,
i.e. below 2^-15 u A: far under one unit of any budget.
"""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32
U = 2.0 ** -24                  # unit roundoff of float32 (round to nearest)
TINY = 2.0 ** -126              # smallest normal f32: absolute slack wherever a result may be subnormal
EPS = float(f32(1e-6))          # layers.rs:6
SECOND_ORDER = 1.0 + 2.0 ** -8  # every first-order budget below is < 2^-9 relative, so the O(u^2) cross terms are < 2^-8 of it


def gamma(k: int) -> float:
    k = max(int(k), 0)
    return k * U / (1.0 - k * U)


def sum64(terms, axis=-1):
    """(S, A) = (sum t_i, sum |t_i|) in float64 along axis; terms are f32 values."""
    t = np.asarray(terms, dtype=np.float64)
    return t.sum(axis=axis), np.abs(t).sum(axis=axis)


def sum_budget(m: int, A):
    """|fl(sum of m f32 terms, any order) - S| <= gamma(m-1) A   (an f32 addition never underflows inexactly)"""
    return gamma(m - 1) * np.asarray(A, dtype=np.float64)


# ---------------------------------------------------------------- tensor.rs
def quantize_quotients(x, group_size: int):
    """tensor.rs:91-119 up to (not including) the rounding: the f32 quotients x / scale, and the scales.  Used to screen
    first-layer rows: an element whose quotient is farther than delta from every half-integer rounds to the same int8 for every
    x' within a relative delta / 127 of x."""
    g = np.asarray(x, dtype=f32).reshape(-1, group_size)
    wmax = np.max(np.abs(g), axis=1).astype(f32)
    scale = (wmax / f32(127.0)).astype(f32)
    safe = np.where(scale != 0, scale, f32(1.0)).astype(f32)
    return (g / safe[:, None]).astype(f32).reshape(-1), scale


def group_terms(xq, xs, wq, ws, n: int, d: int, group_size: int) -> np.ndarray:
    """The f32 group terms of every row, [d][n/G]: t_g = fl32(fl32((f32)dot_g * ws_g) * xs_g) with dot_g the exact integer
    dot of the group (tensor.rs:53-60).  Tolerance mode does NOT reorder these roundings, only the sum of the terms."""
    ng = n // group_size
    w = np.asarray(wq, dtype=np.int8).reshape(d, ng, group_size).astype(np.int64)
    x = np.asarray(xq, dtype=np.int8).reshape(1, ng, group_size).astype(np.int64)
    dot = (w * x).sum(axis=2)                                   # exact: |dot| <= 1024 * 128 * 128 = 2^24
    t = (dot.astype(f32) * np.asarray(ws, dtype=f32).reshape(d, ng)).astype(f32)
    return (t * np.asarray(xs, dtype=f32).reshape(1, ng)).astype(f32)


def gemv_rows(xq, xs, wq, ws, n: int, d: int, group_size: int):
    """(S, A) per output row of the W8A8 matmul (tensor.rs:23-62)."""
    return sum64(group_terms(xq, xs, wq, ws, n, d, group_size), axis=1)


def gemv_budget(n: int, group_size: int, A):
    """any-order fold of the n/G group terms (the -0.0 the fold starts from and the kernel's -0.0 padding terms add nothing)"""
    return sum_budget(n // group_size, A)


# ---------------------------------------------------------------- layers.rs
def rmsnorm64(x, w):
    """RMSNorm::forward, layers.rs:109-119: w * (x / sqrt(mean(x^2) + eps)), float64."""
    x = np.asarray(x, dtype=np.float64)
    ss = float((x * x).sum())
    f = 1.0 / math.sqrt(ss / x.size + EPS)
    return np.asarray(w, dtype=np.float64) * (f * x)


def rmsnorm_rel_budget(n: int) -> float:
    """Relative error bound of one RMSNorm output element, any summation order.  In units of u, first order:
         sum of squares: each square one rounding (u), the any-order sum of n positive terms gamma(n-1): together <= n u on ss;
         ss / n: 1;  + eps: 1 (eps > 0, both terms positive: the relative error does not grow);   sqrt halves what is under
         it: (n + 2) / 2;   sqrt: 1;   1 / .: 1;   f * x: 1;   w * .: 1          =>   (n / 2 + 5) u,
       times SECOND_ORDER.  Vectors whose squares underflow are outside the bound (the tests do not use one)."""
    return (n / 2.0 + 5.0) * U * SECOND_ORDER


def rmsnorm_tree_rel_budget(n: int) -> float:
    """The same chain when the sum is known to be a balanced binary TREE (every term passes through ceil(log2 n) additions):
    squares + tree = (1 + ceil(log2 n)) u on ss, then as above: ((ceil(log2 n) + 3) / 2 + 4) u <= (ceil(log2 n) + 6) u.  Used
    only to SCREEN inputs on the CPU (which tokens keep their int8 operand under every tree), never to accept a device result."""
    return (math.ceil(math.log2(max(n, 2))) + 6.0) * U


def softmax64(a):
    """layers.rs:495-506 in float64: exp(a - max) / sum."""
    a = np.asarray(a, dtype=np.float64)
    e = np.exp(a - a.max())
    return e / e.sum()


def softmax_rel_budget(n: int, score_err: float = 0.0) -> float:
    """Relative budget of one f32 softmax output over n scores, any summation order; score_err = absolute error bound already
    carried by every score (0 for q3_op_softmax, whose input is exact).
         a_i - max: one rounding, u |a_i - max| <= 104 u wherever e_i is not yet 0 (exp(-104) < 2^-149); with score_err on a_i and
              on the max the exponent is off by d <= 2 score_err + 104 u, a relative error d on e_i;
         expf: <= 1 ulp = 2 u;   denominator: the same per-term errors plus the any-order sum gamma(n-1);
         1 / sum: 1;   e_i * inv: 1.
       => 2 (2 score_err + 106 u) + (n + 1) u.  Subnormal e_i get TINY absolute on top (softmax_budget)."""
    return (2.0 * (2.0 * score_err + 106.0 * U) + (n + 1.0) * U) * SECOND_ORDER


def softmax_budget(a, score_err: float = 0.0):
    p = softmax64(a)
    return p * softmax_rel_budget(p.size, score_err) + TINY


def sigmoid64(g):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(g, dtype=np.float64)))


def swiglu64(g, u):
    """layers.rs:472-475: g * sigmoid(g) * u"""
    g = np.asarray(g, dtype=np.float64)
    return g * sigmoid64(g) * np.asarray(u, dtype=np.float64)


def swiglu_budget(g, u, Eg, Eu):
    """hb = silu(g) * u with g, u carrying absolute errors Eg, Eu:  |u| * max|silu'| * Eg + |silu(g)| * Eu, max |silu'| < 1.1
    (silu' = s + g s (1 - s), maximum 1.0998 at g = 2.4), plus the epilogue's own roundings: expf 2 u and 1 + e 1 u on the
    denominator, reciprocal 1, g * . 1, * u 1 = 6 u relative on the result."""
    g = np.asarray(g, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    silu = g * sigmoid64(g)
    return (np.abs(u) * 1.1 * Eg + np.abs(silu) * Eu + 6.0 * U * np.abs(silu * u)) * SECOND_ORDER + TINY


def rope64(v, cs):
    """layers.rs:173-185 (rotate-half pairing); cs: the f32 [half][2] table of cos / sin the engine builds (layers.rs:161-171),
    taken as given so that the table is not part of the error."""
    v = np.asarray(v, dtype=np.float64)
    half = v.size // 2
    x, y = v[:half], v[half:]
    c, s = np.asarray(cs, dtype=np.float64)[:, 0], np.asarray(cs, dtype=np.float64)[:, 1]
    return np.concatenate([x * c - y * s, x * s + y * c])


def _norm_rope(v, w, cs, hd):
    """one head -> (value, absolute budget): the RMSNorm relative budget on both inputs of the rotation, then two products and
    one add / sub: 3 u, all on |x c| + |y s|."""
    y = rmsnorm64(v, w)
    half = hd // 2
    c, s = np.abs(np.asarray(cs, dtype=np.float64)[:, 0]), np.abs(np.asarray(cs, dtype=np.float64)[:, 1])
    ax, ay = np.abs(y[:half]), np.abs(y[half:])
    mag = np.concatenate([ax * c + ay * s, ax * s + ay * c])
    return rope64(y, cs), mag * (rmsnorm_rel_budget(hd) + 3.0 * U) * SECOND_ORDER + TINY


def attention64(q, key_layer, value_layer, q_norm_w, k_norm_w, pos, n_heads, n_kv_heads, head_dim, cs):
    """MultiHeadAttention of one layer, layers.rs:346-419, in float64, with per-element absolute budgets.
    Returns dict(xb, xb_budget, q, q_budget, krow, krow_budget).
    xb[i] budget = A_i * (rel_p + (m + 1) u), m = pos + 1, A_i = sum_t |p_t v_ti|: every product p_t * v one rounding, the sum of
    m terms onto 0.0 in any order gamma(m), and rel_p = softmax_rel_budget(m, score_err) with
    score_err = max_t [ scale * (sum_i Eq_i |k_i| + |q_i| Ek_i + gamma(hd) sum_i |q_i k_i|) + u |score_t| ]   (products and the
    any-order dot; the multiplication by scale; scale = fl32(1 / fl32(sqrt(hd))) is the f32 value the reference uses)."""
    hd = head_dim
    kvd = n_kv_heads * hd
    kv_mul = n_heads // n_kv_heads
    m = pos + 1
    q = np.asarray(q, dtype=np.float64).reshape(n_heads, hd)
    K = np.array(np.asarray(key_layer, dtype=np.float64).reshape(-1, kvd)[:m], copy=True)
    V = np.asarray(value_layer, dtype=np.float64).reshape(-1, kvd)[:m]
    qn, qe = np.zeros_like(q), np.zeros_like(q)
    for h in range(n_heads):
        qn[h], qe[h] = _norm_rope(q[h], q_norm_w, cs, hd)
    kn, ke = np.zeros(kvd), np.zeros(kvd)
    for h in range(n_kv_heads):
        kn[h * hd:(h + 1) * hd], ke[h * hd:(h + 1) * hd] = _norm_rope(K[pos, h * hd:(h + 1) * hd], k_norm_w, cs, hd)
    K[pos] = kn
    Ke = np.zeros_like(K)
    Ke[pos] = ke
    scale = float(f32(1.0) / np.sqrt(f32(hd), dtype=f32))
    xb, xbe = np.zeros((n_heads, hd)), np.zeros((n_heads, hd))
    for h in range(n_heads):
        kv = h // kv_mul
        Kh, Vh, Keh = K[:, kv * hd:(kv + 1) * hd], V[:, kv * hd:(kv + 1) * hd], Ke[:, kv * hd:(kv + 1) * hd]
        sc = (Kh @ qn[h]) * scale
        sc_err = scale * (np.abs(Kh) @ qe[h] + Keh @ np.abs(qn[h]) + gamma(hd) * (np.abs(Kh) @ np.abs(qn[h]))) + U * np.abs(sc)
        p = softmax64(sc)
        rel_p = softmax_rel_budget(m, float(sc_err.max()))
        A = (p[:, None] * np.abs(Vh)).sum(axis=0)
        xb[h] = p @ Vh
        xbe[h] = A * (rel_p + (m + 1.0) * U) * SECOND_ORDER + (m + 1) * TINY * (1.0 + float(np.abs(Vh).max()))
    return {"xb": xb.reshape(-1), "xb_budget": xbe.reshape(-1), "q": qn.reshape(-1), "q_budget": qe.reshape(-1),
            "krow": kn, "krow_budget": ke}


# ---------------------------------------------------------------- input families
def exact_int8_case(rng, n: int, d: int, group_size: int, amp: int = 3):
    """Exact-arithmetic W8A8 inputs: int8 values in [-amp, amp], scales 1 or 2 (weights) and 1/2 or 1 (activation).  Every group
    term is an integer multiple of 1/2 and a row's sum of |terms| stays below 2^23 (asserted), so every partial sum of every
    summation order is exactly representable: all orders return the same bits."""
    ng = n // group_size
    wq = rng.integers(-amp, amp + 1, (d, n)).astype(np.int8)
    xq = rng.integers(-amp, amp + 1, n).astype(np.int8)
    ws = (2.0 ** rng.integers(0, 2, (d, ng))).astype(f32)
    xs = (2.0 ** rng.integers(-1, 1, ng)).astype(f32)
    assert n * amp * amp * 2 < 2 ** 23, "exact-arithmetic family: row too long for this amplitude"
    return xq, xs, wq, ws


def bad_scale_terms(rng, m: int):
    """m f32 terms spanning 2^-20 .. 2^20 with mixed signs whose sum cancels to rounding size: A / |S| >= 1e3 (asserted)."""
    t = ((2.0 ** rng.uniform(-20, 20, m)) * rng.choice([-1.0, 1.0], m)).astype(f32)
    t[m // 2] = f32(0.0)
    t[m // 2] = f32(-np.asarray(t, dtype=np.float64).sum())       # one term cancels the rest up to its own rounding
    S, A = sum64(t)
    assert A >= 1e3 * abs(S), (A, S)
    return t
