"""CPU tests of tests/ref64.py, the float64 reference of the tolerance-mode GPU tests (tests/test_tolerance_mode.py).

The reference and its budgets are pinned on this side without a GPU: the strict C oracle is ONE particular summation order and
a balanced f32 tree (numpy, below) is another, so both must meet every budget on all input families, and must agree bit for bit
on the exact-arithmetic and one-hot families.  The checks are the GPU module's own check functions, run over `OracleOps`: the
oracles behind the interface of `qwen3_rs_amd.ops`.  np_oracle (the second, independent restatement) is held to the same
budgets on small shapes."""
import numpy as np
import pytest

import ref64
import test_tolerance_mode as T
from conftest import assert_biteq

f32 = np.float32


def tree_sum32(t, axis=-1):
    """balanced binary tree in float32 (halves added pairwise, zero padded to a power of two): a legitimate reordering"""
    t = np.moveaxis(np.asarray(t, dtype=f32), axis, -1)
    m = 1 << max(int(t.shape[-1]) - 1, 0).bit_length()
    t = np.concatenate([t, np.zeros(t.shape[:-1] + (m - t.shape[-1],), f32)], axis=-1)
    while t.shape[-1] > 1:
        h = t.shape[-1] // 2
        t = (t[..., :h] + t[..., h:]).astype(f32)
    return t[..., 0]


class OracleOps:
    """strict=True: the C oracle (reference order).  strict=False: the same elementwise operations with every reordered sum
    (RMSNorm sum of squares, group fold, softmax denominator, attention sums) as a balanced f32 tree."""

    def __init__(self, oracle):
        self.o = oracle

    def rmsnorm(self, x, w, strict=True):
        x, w = np.asarray(x, f32), np.asarray(w, f32)
        if strict:
            return self.o.rmsnorm(x, w)
        ss = tree_sum32((x * x).astype(f32))
        f = f32(1.0) / np.sqrt((ss / f32(x.size)).astype(f32) + f32(1e-6), dtype=f32)
        return (w * (f * x).astype(f32)).astype(f32)

    def softmax(self, a, strict=True):
        a = np.asarray(a, f32)
        if strict:
            return self.o.softmax(a)
        from oracle import np_oracle
        e = np_oracle.expf((a - a.max()).astype(f32))
        return (e * (f32(1.0) / tree_sum32(e))).astype(f32)

    def gemv_role(self, role, wq, ws, n, rows, group_size, x=None, norm_w=None, pre_q=None, pre_s=None, out=None, rows_kv=0,
                  head_dim=0, strict=True):
        G = group_size
        dw = T.weight_rows(role, rows, rows_kv)
        tap = self.rmsnorm(x, norm_w, strict) if role in T.NORM_ROLES else None
        if role in T.NORM_ROLES:
            xq, xs = self.o.quantize(tap, G)
        elif role == T.QUANT:
            xq, xs = self.o.quantize(x, G)
        else:
            xq, xs = pre_q, pre_s
        if strict:
            r = self.o.matmul(xq, xs, wq, ws, n, dw, G)
        else:
            r = tree_sum32(ref64.group_terms(xq, xs, wq, ws, n, dw, G), axis=1)
        if role in (T.QUANT, T.PREQR):
            r = (np.asarray(out, f32) + r).astype(f32)
        elif role == T.SWIGLU:
            r = self.o.swiglu(r[:rows], r[rows:])
        return {"out": r, "tap": tap, "argmax": self.o.sample_argmax(r) if role == T.LOGITS else -1,
                "info": [1 if (G == 64 and (role, n) in T.TABLE) else 0, 0, 0, 0]}

    def attention(self, q, K, V, qw, kw, pos, nh, nkv, hd, strict=True):
        if strict:
            return self.o.attention(q, K, V, qw, kw, pos, nh, nkv, hd)
        from oracle import np_oracle
        _, q2, k2 = self.o.attention(q, K, V, qw, kw, pos, nh, nkv, hd)      # (QK-norm + RoPE: elementwise after a 16..128-term sum)
        kvd = nkv * hd
        Kc, Vc = k2.reshape(-1, kvd)[:pos + 1], np.asarray(V, f32).reshape(-1, kvd)[:pos + 1]
        scale = f32(1.0) / np.sqrt(f32(hd), dtype=f32)
        xb = np.zeros((nh, hd), f32)
        for h in range(nh):
            kv = h // (nh // nkv)
            sc = (tree_sum32((Kc[:, kv * hd:(kv + 1) * hd] * q2[h * hd:(h + 1) * hd][None, :]).astype(f32), axis=1) * scale).astype(f32)
            e = np_oracle.expf((sc - sc.max()).astype(f32))
            p = (e * (f32(1.0) / tree_sum32(e))).astype(f32)
            xb[h] = tree_sum32((p[:, None] * Vc[:, kv * hd:(kv + 1) * hd]).astype(f32), axis=0)
        return xb.reshape(-1), q2, k2


@pytest.fixture(scope="module")
def cpu_ops(oracle):
    return OracleOps(oracle)


@pytest.mark.parametrize("strict", [True, False], ids=["oracle-order", "tree-order"])
@pytest.mark.parametrize("role,n,G", [(T.QKV, 1024, 64), (T.QKV, 2560, 64), (T.SWIGLU, 1024, 64), (T.LOGITS, 1024, 64),
                                      (T.PREQR, 2048, 64), (T.QUANT, 3072, 64), (T.QUANT, 9728, 64), (T.QUANT, 1024, 32),
                                      (T.SWIGLU, 1024, 128)])
def test_gemv_families_meet_the_budgets_in_two_orders(cpu_ops, oracle, role, n, G, strict):
    """The three input families of the GPU GEMV-role tests through the oracle's order and through a tree: budgets hold, and the
    exact-arithmetic / one-hot rows are bit-equal in both (asserted inside check_role)."""
    T.run_families(cpu_ops, oracle, role, n, G, strict, want_table=(G == 64 and (role, n) in T.TABLE))


@pytest.mark.parametrize("strict", [True, False], ids=["oracle-order", "tree-order"])
@pytest.mark.parametrize("role,n", [(T.QKV, 2560), (T.SWIGLU, 1024), (T.QUANT, 2048), (T.PREQR, 4096)])
def test_special_values_in_two_orders(cpu_ops, oracle, role, n, strict):
    """saturated dots, zero groups, the zero vector, rows of -0.0 terms: what the GPU test asks is consistent with the oracle"""
    T.test_gemv_role_special_values(cpu_ops, oracle, role, n, strict)


@pytest.mark.parametrize("role,n", [(T.QKV, 1024), (T.SWIGLU, 2560), (T.LOGITS, 768)])
def test_norm_prologue_one_hot_sweep_is_exact_in_a_tree(cpu_ops, oracle, role, n):
    T.test_norm_prologue_tree_counts_every_term_once(cpu_ops, oracle, role, n)


@pytest.mark.parametrize("name", T.SCREEN_SHAPES)
def test_screening_yield(q3, name):
    """Condition of the screened first-layer-row GPU tests, checked without a GPU: of the fixed pool of 64 candidate tokens of each
    shape at least 16 keep every quantization quotient farther than delta from a half-integer (float64 only; delta as derived in
    screen_tokens, never shrunk -- a shape that yields fewer needs a wider pool)."""
    ck = q3.checkpoint
    shape = ck.SHAPES[name]
    pool = T.candidate_pool(shape)
    assert len(set(pool)) == T.POOL_SIZE
    t0 = T.layer0_tensors(ck, shape, T.SCREEN_SEED.get(name, 1235))
    ok = T.screen_tokens(shape, t0, pool)
    print(f"screening yield {name}: {len(ok)} of {len(pool)}")
    assert len(ok) >= T.MIN_YIELD, (name, len(ok))
    # the C oracle's order (a legitimate one) produces the screened int8 operand and meets the row budget
    from oracle import q3_oracle as o
    g = shape.group_size
    for tok in list(ok)[:4]:
        x = (t0["eq"][tok].astype(f32).reshape(-1, g) * t0["es"][tok][:, None]).astype(f32).reshape(-1)
        xq, xs = o.quantize(o.rmsnorm(x, t0["w"]), g)
        row = o.matmul(xq, xs, t0["vq"], t0["vs"], shape.dim, shape.kv_dim, g)
        assert np.all(np.abs(row - ok[tok][0]) <= ok[tok][1])


def test_one_hot_generators_visit_every_index():
    rng = np.random.default_rng(0)
    for role, n in T.TABLE:
        rows, rkv = T.role_rows(role, partial=True)
        d = T.weight_rows(role, rows, rkv)
        wq, _ = T.one_hot_weights(rng, d, n, 64)
        live = np.abs(wq.reshape(d, n // 64, 64).astype(np.int32)).sum(axis=2) > 0
        assert np.all(live.sum(axis=1) <= 1), "at most one non-zero group per row"
        assert np.all(live.any(axis=0)), f"{T.ROLE_NAMES[role]} n={n}: a fold index without a one-hot row"
    xq, xs = T.exact_activation(rng, 12288, 64)
    assert np.all(np.abs(xq.reshape(-1, 64)).max(axis=1) == 127) and set(np.log2(xs).tolist()) <= {-1.0, 0.0}
    t = ref64.bad_scale_terms(rng, 4096)
    S, A = ref64.sum64(t)
    assert A >= 1e3 * abs(S)
    for order in (np.cumsum(t, dtype=f32)[-1], tree_sum32(t), np.cumsum(t[::-1], dtype=f32)[-1]):
        assert abs(float(order) - S) <= ref64.sum_budget(t.size, A)


@pytest.mark.parametrize("n", [64, 128, 1000, 2560])
def test_rmsnorm_reference_in_two_orders(cpu_ops, oracle, n):
    T.test_rmsnorm_fp64(cpu_ops, oracle, n)


@pytest.mark.parametrize("n", [1, 7, 64, 65, 777])
def test_softmax_reference_in_two_orders(cpu_ops, oracle, n):
    T.test_softmax_fp64(cpu_ops, oracle, n)


@pytest.mark.parametrize("shape", [(4, 2, 16, 64, 9), (8, 8, 64, 32, 0), (4, 1, 32, 100, 70), (4, 2, 128, 80, 64)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_attention_reference_in_two_orders(cpu_ops, oracle, shape):
    T.test_attention_fp64(cpu_ops, oracle, shape)


def test_np_oracle_meets_the_same_budgets(oracle, np_oracle):
    """The independent numpy restatement against ref64 on every operation (tiny shapes: it is slow)."""
    rng = np.random.default_rng(4)
    n, d, G = 256, 24, 32
    x = (rng.standard_normal(n) * 2.0 ** rng.uniform(-8, 8, n)).astype(f32)
    w = (1 + 0.1 * rng.standard_normal(n)).astype(f32)
    y = np_oracle.rmsnorm(x, w)
    y64 = ref64.rmsnorm64(x, w)
    assert np.all(np.abs(y - y64) <= np.abs(y64) * ref64.rmsnorm_rel_budget(n) + ref64.TINY)
    assert_biteq(y, oracle.rmsnorm(x, w))
    xq, xs = np_oracle.quantize(y, G)
    quot, sc = ref64.quantize_quotients(y, G)
    assert np.array_equal(sc, xs) and np.all(np.abs(quot - xq) <= 0.5)
    wq, ws = T.cancelling_weights(rng, d, n, G)
    S, A = ref64.gemv_rows(xq, xs, wq, ws, n, d, G)
    out = np_oracle.matmul(xq, xs, wq.reshape(-1), ws.reshape(-1), n, d, G)
    assert np.all(np.abs(out - S) <= ref64.gemv_budget(n, G, A))
    assert_biteq(out, oracle.matmul(xq, xs, wq, ws, n, d, G))
    a = rng.uniform(-80, 80, 300).astype(f32)
    p = np_oracle.softmax(a)
    assert np.all(np.abs(p - ref64.softmax64(a)) <= ref64.softmax_budget(a))
    g, u = rng.standard_normal(64).astype(f32) * 4, rng.standard_normal(64).astype(f32)
    assert np.all(np.abs(np_oracle.swiglu(g, u) - ref64.swiglu64(g, u)) <= ref64.swiglu_budget(g, u, 0.0, 0.0))
    cs = np_oracle.rope_freqs(32, 17)
    v = rng.standard_normal(32).astype(f32)
    r64 = ref64.rope64(v, cs)
    assert np.all(np.abs(np_oracle.rope_apply(v, cs) - r64) <= 3 * ref64.U * (np.abs(r64) + np.abs(v).max()))
