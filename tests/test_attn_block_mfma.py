"""k_attn_pf_mfma (q3_op_attention_block, the dense-prefill attention of Q3_FLAG_FAST engines) against float64 attention.

The budget, derived and not fitted.  u = 2^-24 (ref64.U), ub = 2^-8 (bf16, 8-bit significand).
  Split: a = hi + lo + r, hi = bf16(a), lo = bf16(a - hi), |r| <= ub^2 |a| = 2^-16 |a| (inputs stay away from bf16 underflow).
  A product a b goes to the matrix cores as hi*hi + hi*lo + lo*hi, each exact in f32; dropped are lo*lo and the two r terms,
  together at most 3 * 2^-16 * (1 + 2^-7) |a||b|.
  Dot product of length n: 3n products added in f32 in the hardware's order, one rounding u per added product: gamma(3n) of the
  sum of magnitudes.  So |dot - exact| <= eps(n) sum_d |a_d||b_d|, eps(n) = 1.01 (3 * 2^-16 + gamma(3n)).
  Scores: E_s = max_t scale * eps(hd) * sum_d |q_d||k_td|.
  Output: |xb_d - ref_d| <= (2 E_s + eps(np) + (np + 64) u) * sum_t p_t |v_td| * SECOND_ORDER + TINY, p the float64 softmax over the
  column's np keys; (np + 64) u covers expf, the running sum, the per-chunk rescales and the final division.
"""
import os

import numpy as np
import pytest

import ref64

pytestmark = pytest.mark.gpu
HD = 128
SHAPES = [(4, 2, 33, 0), (8, 2, 70, 0), (10, 2, 65, 0), (16, 2, 64, 0), (8, 2, 45, 70), (4, 2, 100, 200)]   # n_heads, n_kv, n_pos, first_pos


def eps(n):
    return 1.01 * (3 * 2.0 ** -16 + ref64.gamma(3 * n))


def attention64(q, K, V, n_heads, n_kv, first_pos):
    """(xb, budget), [n_pos][n_heads * HD] each, in float64"""
    q, K, V = (np.asarray(x, dtype=np.float64) for x in (q, K, V))
    scale = float(np.float32(1.0) / np.sqrt(np.float32(HD)))
    n_pos = q.shape[0]
    xb, bud = np.zeros((n_pos, n_heads * HD)), np.zeros((n_pos, n_heads * HD))
    for i in range(n_pos):
        m = first_pos + i + 1
        for h in range(n_heads):
            kv = slice((h // (n_heads // n_kv)) * HD, (h // (n_heads // n_kv) + 1) * HD)
            qh = q[i, h * HD:(h + 1) * HD]
            p = ref64.softmax64(scale * (K[:m, kv] @ qh))
            e_s = float((scale * eps(HD) * (np.abs(K[:m, kv]) @ np.abs(qh))).max())
            xb[i, h * HD:(h + 1) * HD] = p @ V[:m, kv]
            bud[i, h * HD:(h + 1) * HD] = (2 * e_s + eps(m) + (m + 64) * ref64.U) * (p @ np.abs(V[:m, kv])) * ref64.SECOND_ORDER + ref64.TINY
    return xb, bud


@pytest.mark.parametrize("n_heads,n_kv,n_pos,first_pos", SHAPES)
def test_block_attention_fp64(q3, n_heads, n_kv, n_pos, first_pos):
    """KVM 2, 4, 5 and 8; a partial and an exact tile; key-chunk edges at 64 and 128; continuation blocks whose first chunks are
    unmasked.  N(0,1) data, and value rows scaled by 2^uniform(-20, 20) per timestep with keys times 4."""
    rng = np.random.default_rng(n_heads * 1000 + n_pos)
    rows = first_pos + n_pos
    q = rng.standard_normal((n_pos, n_heads * HD)).astype(np.float32)
    K = rng.standard_normal((rows, n_kv * HD)).astype(np.float32)
    V = rng.standard_normal((rows, n_kv * HD)).astype(np.float32)
    for what, k, v in (("normal", K, V), ("scaled", (4 * K).astype(np.float32), (V * 2.0 ** rng.uniform(-20, 20, (rows, 1))).astype(np.float32))):
        got = q3.ops.attention_block(q, k, v, first_pos, n_heads, n_kv, HD)
        ref, bud = attention64(q, k, v, n_heads, n_kv, first_pos)
        ratio = np.abs(got - ref) / bud
        print(f"TOLBUDGET|attention_block|{n_heads}/{n_kv} heads {n_pos}+{first_pos}|{what}|{ratio.max():.4f}")
        assert np.all(np.isfinite(got)) and ratio.max() <= 1.0, (what, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))


@pytest.mark.parametrize("n_heads,n_kv,n_pos,first_pos", [SHAPES[0], SHAPES[4], SHAPES[5]])
def test_block_attention_mask_is_exact(q3, n_heads, n_kv, n_pos, first_pos):
    """Every query is a sign vector s, every key -60 s except key t* = +60 s; value rows are an integer vector a except V[t*] = b
    (integers within +-999: exact in hi + lo).  Columns at t* and later return b bit for bit -- every other exponential underflows to
    0 and 1 * b is exact through the split and the accumulate; earlier columns return a, not b.  t* sweeps 0, the block's first
    position and the one before, and every multiple of 32 +- 1: a mask off by one, a dropped or doubled chunk or a mis-indexed
    head fails."""
    rng = np.random.default_rng(n_pos)
    rows, last = first_pos + n_pos, first_pos + n_pos - 1
    s = rng.choice([-1.0, 1.0], HD).astype(np.float32)
    a, b = ((rng.integers(1, 1000, n_kv * HD) * rng.choice([-1, 1], n_kv * HD)).astype(np.float32) for _ in range(2))
    q = np.tile(s, (n_pos, n_heads))
    sweep = {0, max(first_pos - 1, 0), first_pos} | {t + d for t in range(32, last + 2, 32) for d in (-1, 1) if t + d <= last}
    for t_star in sorted(sweep):
        K = np.tile(-60 * s, (rows, n_kv))
        K[t_star] = np.tile(60 * s, n_kv)
        V = np.tile(a, (rows, 1))
        V[t_star] = b
        got = q3.ops.attention_block(q, K, V, first_pos, n_heads, n_kv, HD)
        ref, bud = attention64(q, K, V, n_heads, n_kv, first_pos)
        want_b = np.tile(b.reshape(n_kv, 1, HD), (1, n_heads // n_kv, 1)).reshape(-1)
        for i in range(n_pos):
            if first_pos + i >= t_star:
                assert np.array_equal(got[i].view(np.uint32), want_b.view(np.uint32)), (t_star, i)
            else:
                assert np.all(np.abs(got[i] - ref[i]) <= bud[i]) and not np.array_equal(got[i], want_b), (t_star, i)


def test_refusals(q3):
    """flags = 0 (the reference-order block kernel is not an operator) and head_dim 64: Q3_ERR_UNSUPPORTED before any launch --
    the output the wrapper zeroed comes back untouched because the call raises before it returns anything."""
    z = np.zeros((4, 4 * HD), dtype=np.float32)
    for kw in (dict(head_dim=HD, strict=True), dict(head_dim=64)):
        with pytest.raises(q3.Q3Error) as e:
            q3.ops.attention_block(z, z[:, :2 * HD], z[:, :2 * HD], 0, 4 * HD // kw["head_dim"], 2 * HD // kw["head_dim"], **kw)
        assert e.value.code == -5, (kw, e.value)


def test_fast_prefill_two_blocks_within_the_stated_bound(q3, oracle):
    """A FAST engine whose prompt arrives as two dense blocks, 70 positions and then 45 from position 70 (the continuation block
    runs k_attn_pf_mfma with unmasked first chunks), then three forwards: the project's stated 0.15 sigma against the strict
    oracle (SIGMA_BOUND, tests/test_tolerance_mode.py)."""
    name, ctx = "qwen3-4b-dims-l2", 512
    path = os.path.join(os.environ.get("Q3_CKPT_DIR", "/tmp"), f"q3_{name}.bin")
    q3.checkpoint.ensure_synthetic_checkpoint(path, q3.checkpoint.SHAPES[name], seed=1235)
    prompt = q3.checkpoint.iter_prompt_tokens(q3.checkpoint.SHAPES[name], 5, 115)
    om = oracle.OracleModel(path, ctx)
    for pos, tok in enumerate(prompt):
        om.forward(tok, pos)
    with q3.TransformerBuilder(path).with_ctx_length(ctx).with_strict(False).build() as t:
        t.prefill(prompt[:70], 0, batched=True)
        t.prefill(prompt[70:], 70, batched=True)
        tok = 7
        for pos in range(115, 118):
            got, want = np.array(t.forward(tok, pos), copy=True), om.forward(tok, pos)
            d, sd = float(np.max(np.abs(got - want))), float(np.std(want))
            print(f"TOLBUDGET|engine_logits|{name}:two-blocks:pos{pos}|stated-0.15-sigma|fast|{d / (0.15 * sd):.4f}")
            assert np.all(np.isfinite(got)) and d <= 0.15 * sd, (pos, d, sd)
            tok = oracle.sample_argmax(want)
