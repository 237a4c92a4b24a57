"""k_attn_pf_mfma (q3_op_attention_block) bit for bit: two properties of the kernel's structure that need no tolerance, the float64
budget at the magnitudes the hi / lo split has to survive, and the kernel inside engines at 2, 5 and 8 query heads per kv head.
DESIGN.md 4.24; measured ratios, times and the mutations these tests were run against: profiles/attn_block_exact.md.

Split invariance.  The output row of position p is a function of q_p, K[0..p] and V[0..p] alone: chunks start at key 0 and step by
64 whatever the block is, a chunk a wave skips and a chunk it processes with every key masked leave the column's state the same
(cmax = -inf, alpha = expf(0) = 1, csum = 0, o += V * 0), clamped duplicate rows are always masked, MFMA output columns do not mix,
and q3_expf_main and q3_expf_t agree wherever both apply.  So the block [a, a + n) returns the bits the block [0, N) returned for
those rows, wherever it lands relative to tiles, column blocks, waves and lanes.

Two-level softmax.  Every query a sign vector s, K[t] = 0 for t in a set T and -60 s otherwise: scores are exactly 0 or one common
value near -679, expf returns exactly 1 or 0.  With integer V within +-999 (exact in hi + lo, every partial sum an integer below
2^24) the output is f32(f32(sum of V[t] over the top-level keys t <= p) * (f32(1) / f32(count))), the top level being T once a key
of T is visible and every key before."""
import numpy as np
import pytest

from test_attn_block_mfma import HD, attention64

pytestmark = pytest.mark.gpu

# n_heads, n_kv, N, first_pos of the whole call:
#   KVM 2, three tiles of 128 columns, one kv head | KVM 4, four tiles of 64, an odd kv-head count | KVM 5, four tiles of 32, three
#   staging-only waves, an odd column count (the paired last head) | KVM 8, four tiles of 32 | KVM 2 over 34 chunks, row offsets past 2,048
LAUNCH = [(2, 1, 330, 0), (12, 3, 200, 0), (10, 2, 101, 0), (16, 2, 100, 0), (4, 2, 70, 2100)]
IDS = [f"{h}-{k}-{n}+{f}" for h, k, n, f in LAUNCH]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tile_cols(n_heads, n_kv):
    return 32 * (8 // (n_heads // n_kv))                 # attn_pf_mfma_cols


def pieces(n_heads, n_kv, N, base):
    """(first, n) relative to the whole call's first column"""
    if base:
        return [(a, N - a) for a in (1, 31, 37)] + [(a, 1) for a in (1, 31, 37)]
    c = tile_cols(n_heads, n_kv)
    ps = [(0, 1)] + [(a, 1) for a in (1, 31, 32, 63, 64, 65, N - 1)]
    ps += [(31, 33), (33, 31), (63, 2), (64, 32), (1, N - 1), (N - 33, 33)]
    ps += [(c - 1, min(N - (c - 1), c + 2)), (c + 1, min(N - (c + 1), c + 2))]      # one column before and after a tile edge
    assert all(0 <= a and n >= 1 and a + n <= N for a, n in ps)
    return ps


def ulps(a, b):
    """distance in units of the last place between two finite f32 arrays"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("n_heads,n_kv,N,base", LAUNCH, ids=IDS)
def test_split_invariance_bitwise(q3, n_heads, n_kv, N, base):
    """N(0,1) data.  The whole call is held to float64 within the budget (the anchor), returns the same bits twice, and every piece
    of it computed alone returns the whole call's bits for its rows."""
    rng = np.random.default_rng(7000 + n_heads * 100 + N)
    rows = base + N
    q = rng.standard_normal((N, n_heads * HD)).astype(np.float32)
    K = rng.standard_normal((rows, n_kv * HD)).astype(np.float32)
    V = rng.standard_normal((rows, n_kv * HD)).astype(np.float32)
    whole = q3.ops.attention_block(q, K, V, base, n_heads, n_kv, HD)
    ref, bud = attention64(q, K, V, n_heads, n_kv, base)
    ratio = np.abs(whole - ref) / bud
    print(f"TOLBUDGET|attention_block|{n_heads}/{n_kv} heads {N}+{base}|split-anchor|{ratio.max():.4f}")
    assert np.all(np.isfinite(whole)) and ratio.max() <= 1.0, (float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    again = q3.ops.attention_block(q, K, V, base, n_heads, n_kv, HD)
    assert np.array_equal(u32(again), u32(whole)), "two runs of one launch differ"
    bad = []
    for a, n in pieces(n_heads, n_kv, N, base):
        got = q3.ops.attention_block(q[a:a + n], K[:base + a + n], V[:base + a + n], base + a, n_heads, n_kv, HD)
        ne = u32(got) != u32(whole[a:a + n])
        if ne.any():
            r, c = np.nonzero(ne)
            bad.append(f"piece ({a}, {n}): {int(ne.sum())} elements differ, at most {int(ulps(got, whole[a:a + n]).max())} ulp; "
                       f"positions {sorted(set((base + a + r).tolist()))[:12]}, heads {sorted(set((c // HD).tolist()))}")
    assert not bad, "\n".join(bad)


def level_sets(rng, rows):
    """the sets T of top-level keys, as boolean vectors over the rows"""
    t = np.arange(rows)
    half = rng.random(rows) < 0.5
    late = (rng.random(rows) < 0.5) & (t >= 70)
    late[min(rows - 1, 75)] = True
    return {"every key": np.ones(rows, bool), "0 and a random half": half | (t == 0), "a random half past 69": late,
            "keys 5 mod 16": t % 16 == 5, "keys 10 mod 16": t % 16 == 10, "last of each chunk": t % 64 == 63,
            "first of each chunk": t % 64 == 0}


def two_level_expected(V, T, first_pos, n_pos, n_heads, n_kv):
    """[n_pos][n_heads * HD] f32 by the formula of the module docstring; V integer-valued [rows][n_kv * HD], T boolean [rows]"""
    Vi = V.astype(np.int64)
    sum_top, cnt_top = np.cumsum(Vi * T[:, None], axis=0), np.cumsum(T)
    sum_all, cnt_all = np.cumsum(Vi, axis=0), np.arange(1, V.shape[0] + 1)
    p = first_pos + np.arange(n_pos)
    top = cnt_top[p] > 0
    s = np.where(top[:, None], sum_top[p], sum_all[p])
    cnt = np.where(top, cnt_top[p], cnt_all[p])
    assert np.abs(s).max() < 2 ** 24
    want = (s.astype(np.float32) * (np.float32(1.0) / cnt.astype(np.float32))[:, None]).astype(np.float32)    # per kv head
    kvm = n_heads // n_kv
    return np.repeat(want.reshape(n_pos, n_kv, HD), kvm, axis=1).reshape(n_pos, n_heads * HD)            # head h: kv head h // KVM


@pytest.mark.parametrize("n_heads,n_kv,N,base", LAUNCH, ids=IDS)
def test_two_level_softmax_bitwise(q3, n_heads, n_kv, N, base):
    """Every key counted exactly once, at every position and alignment, each probability paired with its own value row (single
    slots of the 16-key groups: the V^T slot permutation), late sets through the alpha = 0 rescale; a different integer V per kv
    head.  The block of the launch table, and the continuation blocks (70, 45) and (200, 100) of tests/test_attn_block_mfma.py."""
    rng = np.random.default_rng(9000 + n_heads * 100 + N)
    s = rng.choice([-1.0, 1.0], HD).astype(np.float32)
    for first_pos, n_pos in ((base, N), (70, 45), (200, 100)):
        rows = first_pos + n_pos
        V = (rng.integers(1, 1000, (rows, n_kv * HD)) * rng.choice([-1, 1], (rows, n_kv * HD))).astype(np.float32)
        assert np.abs(V).astype(np.int64).sum(axis=0).max() < 2 ** 24          # every partial sum of every order is an exact integer
        q = np.tile(s, (n_pos, n_heads))
        for what, T in level_sets(rng, rows).items():
            K = np.where(T[:, None], np.float32(0.0), np.tile(-60 * s, (rows, n_kv))).astype(np.float32)
            got = q3.ops.attention_block(q, K, V, first_pos, n_heads, n_kv, HD)
            want = two_level_expected(V, T, first_pos, n_pos, n_heads, n_kv)
            ne = u32(got) != u32(want)
            if ne.any():
                r, c = np.nonzero(ne)
                raise AssertionError(f"{what}, block ({first_pos}, {n_pos}): {int(ne.sum())} elements differ; positions "
                                     f"{sorted(set((first_pos + r).tolist()))[:16]}, heads {sorted(set((c // HD).tolist()))}; first "
                                     f"{got[r[0], c[0]]!r} for {want[r[0], c[0]]!r}")


def magnitude_families(q, K, V):
    """name -> (q, K, V).  Powers of two scale hi, lo and the split remainder alike, so the budget moves with the data."""
    f = np.float32
    zq, zv = q.copy(), V.copy()
    zq[[0, 33, q.shape[0] - 1]] = 0.0
    zv[[0, 31, 64, V.shape[0] - 1]] = 0.0
    return {"V x 2^60": (q, K, V * f(2.0 ** 60)), "V x 2^-60": (q, K, V * f(2.0 ** -60)),
            "q x 2^30, K x 2^-30": (q * f(2.0 ** 30), K * f(2.0 ** -30), V), "q x 2^-30, K x 2^30": (q * f(2.0 ** -30), K * f(2.0 ** 30), V),
            "K x 16": (q, K * f(16.0), V), "zero query rows": (zq, K, V), "zero value rows": (q, K, zv)}


@pytest.mark.parametrize("n_heads,n_kv", [x[:2] for x in LAUNCH[:4]], ids=[f"{h}-{k}" for h, k, _, _ in LAUNCH[:4]])
def test_budget_at_split_magnitudes(q3, n_heads, n_kv):
    """The float64 budget of tests/test_attn_block_mfma.py, unchanged, on 70 positions per KVM: value rows times 2^+-60, queries and
    keys scaled against each other by 2^+-30 (the scores unchanged, the hi / lo exponents far from 1), keys times 16 (peaked
    softmax: score differences past 88 among unmasked keys, checked here, run the q3_expf_special path), zero query rows (a uniform
    mean) and zero value rows.
    Outside the budget's stated domain, and not tested: subnormal inputs and inputs whose lo part or products are subnormal (the
    split's 2^-16 remainder bound assumes no bf16 underflow), and magnitudes at which bf16(a) rounds to infinity (|a| >= 2^128 -
    2^119)."""
    rng = np.random.default_rng(5000 + n_heads)
    n_pos = 70
    q = rng.standard_normal((n_pos, n_heads * HD)).astype(np.float32)
    K = rng.standard_normal((n_pos, n_kv * HD)).astype(np.float32)
    V = rng.standard_normal((n_pos, n_kv * HD)).astype(np.float32)
    for what, (qf, kf, vf) in magnitude_families(q, K, V).items():
        if what == "K x 16":
            sc = np.einsum("phd,thd->pht", qf.astype(np.float64).reshape(n_pos, n_kv, -1, HD)[:, :, 0], kf.astype(np.float64).reshape(n_pos, n_kv, HD)) / np.sqrt(HD)
            spread = max(float(np.ptp(sc[p, :, :p + 1], axis=-1).max()) for p in range(n_pos))
            assert spread > 88.0, spread
        got = q3.ops.attention_block(qf, kf, vf, 0, n_heads, n_kv, HD)
        ref, bud = attention64(qf, kf, vf, n_heads, n_kv, 0)
        ratio = np.abs(got - ref) / bud
        print(f"TOLBUDGET|attention_block|{n_heads}/{n_kv} heads {n_pos}+0|{what}|{ratio.max():.4f}")
        assert np.all(np.isfinite(got)) and ratio.max() <= 1.0, (what, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))


ENGINES = ["small-hd128", "small-kvm5", "small-kvm8"]          # 8 / 4, 10 / 2 and 16 / 2 heads: k_attn_pf_mfma<2>, <5>, <8>
CTX, N_PROMPT = 512, 115


@pytest.fixture(scope="module")
def ckpt(q3, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = str(tmp_path_factory.mktemp("attn_exact") / f"{name}.bin")
            q3.checkpoint.write_synthetic_checkpoint(made[name], q3.checkpoint.SHAPES[name], seed=1235)
        return made[name], q3.checkpoint.iter_prompt_tokens(q3.checkpoint.SHAPES[name], 5, N_PROMPT)
    return get


def fast_engine(q3, path):
    return q3.TransformerBuilder(path).with_ctx_length(CTX).with_strict(False).build()


@pytest.mark.parametrize("name", ENGINES)
def test_fast_prefill_two_blocks_kvm_2_5_8(q3, oracle, ckpt, name):
    """test_fast_prefill_two_blocks_within_the_stated_bound (tests/test_attn_block_mfma.py) at 2, 5 and 8 query heads per kv head:
    115 tokens as dense blocks of 70 and 45 on a FAST engine, then three forwards within the project's stated 0.15 sigma of the
    strict oracle (SIGMA_BOUND, tests/test_tolerance_mode.py)."""
    path, prompt = ckpt(name)
    om = oracle.OracleModel(path, CTX)
    for pos, tok in enumerate(prompt):
        om.forward(tok, pos)
    with fast_engine(q3, path) as t:
        t.prefill(prompt[:70], 0, batched=True)
        t.prefill(prompt[70:], 70, batched=True)
        tok = 7
        for pos in range(N_PROMPT, N_PROMPT + 3):
            got, want = np.array(t.forward(tok, pos), copy=True), om.forward(tok, pos)
            d, sd = float(np.max(np.abs(got - want))), float(np.std(want))
            print(f"TOLBUDGET|engine_logits|{name}:two-blocks:pos{pos}|stated-0.15-sigma|fast|{d / (0.15 * sd):.4f}")
            assert np.all(np.isfinite(got)) and d <= 0.15 * sd, (pos, d, sd)
            tok = oracle.sample_argmax(want)


@pytest.mark.parametrize("name", ENGINES)
def test_fast_prefill_split_70_45_against_40_75(q3, ckpt, name):
    """Two FAST engines prefill the same 115 tokens, one as 70 + 45 and one as 40 + 75 (every block dense: more than 32 positions);
    the next forward's logits read every cache row either split wrote.  Held to the stated 0.15 sigma of each other; whether they
    are bit-equal is printed, not asserted: the block GEMMs around the attention are not argued order-invariant."""
    path, prompt = ckpt(name)
    logits = []
    for cut in (70, 40):
        with fast_engine(q3, path) as t:
            t.prefill(prompt[:cut], 0, batched=True)
            t.prefill(prompt[cut:], cut, batched=True)
            logits.append(np.array(t.forward(7, N_PROMPT), copy=True))
    a, b = logits
    d, sd = float(np.max(np.abs(a - b))), float(np.std(a))
    print(f"TOLBUDGET|engine_logits|{name}:70+45-vs-40+75|stated-0.15-sigma|fast|{d / (0.15 * sd):.4f}")
    print(f"BITEQUAL|engine_logits|{name}:70+45-vs-40+75|{bool(np.array_equal(u32(a), u32(b)))}")
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and d <= 0.15 * sd, (d, sd)
