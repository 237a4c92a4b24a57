"""Tolerance mode (Q3_FLAG_FAST) against a float64 reference, per kernel role and per path (run with -m gpu on an MI355X).

Every check compares the device with tests/ref64.py -- the real-number value of the operation in float64 -- under the
classical any-order summation bound (ref64's module docstring), never with another f32 rounding and never with a constant
fitted to device output.  What makes the checks sharp is the input, three families per operation:
  * exact arithmetic / one-hot: every partial sum of every order is exactly representable, so tolerance mode must return
    the SAME BITS as the strict C oracle; a dropped, doubled or mis-scaled term fails;
  * badly scaled, cancelling terms (A / |S| >= 1e3) and N(0,1) data against the per-element budget in units of u * A.
In reference order (flags = 0) every result must additionally be bit-equal to the C oracle, which gives the 16
shape-specialised k_gemv instantiations their first adversarial inputs.

Each budgeted check prints `TOLBUDGET|operation|shape|family|mode|observed/budget`; profiles/tolerance_mode_budget.md is
filled from those lines (a record, not a threshold).
"""
import os

import numpy as np
import pytest

import ref64
from conftest import assert_biteq

pytestmark = pytest.mark.gpu
f32 = np.float32
U = ref64.U


@pytest.fixture(scope="module")
def ops(q3):
    return q3.ops


def ratio(op, shape, family, strict, got, want64, budget):
    """max over elements of |got - want| / budget (0 / 0 = 0: where the budget is zero the result must be exact); printed."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want64, dtype=np.float64))
    budget = np.broadcast_to(np.asarray(budget, dtype=np.float64), err.shape)
    assert np.all(np.isfinite(np.asarray(got, dtype=np.float64))), (op, shape, family, "non-finite result")
    r = np.where(budget > 0, err / np.where(budget > 0, budget, 1.0), np.where(err == 0, 0.0, np.inf))
    worst = float(r.max()) if r.size else 0.0
    print(f"TOLBUDGET|{op}|{shape}|{family}|{'strict' if strict else 'fast'}|{worst:.4f}")
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# 1. The fused GEMV roles, alone (q3_op_gemv_role): every entry of both configuration tables + the generic path
# ----------------------------------------------------------------------------------------------------------------------
QKV, SWIGLU, QUANT, PREQR, LOGITS = range(5)
ROLE_NAMES = ["norm_qkv", "norm_swiglu", "quant_resid", "preqr_resid", "norm_logits"]
NORM_ROLES = (QKV, SWIGLU, LOGITS)
# (role, n) of every table entry (csrc/q3_gemv_inst.hip, Q3_CFG_LIST; PRO_EMBED_NORM shares the PRO_NORM forms)
TABLE = ([(r, n) for r in (QKV, SWIGLU, LOGITS) for n in (1024, 2560, 4096)] + [(PREQR, 2048), (PREQR, 4096)] +
         [(QUANT, n) for n in (3072, 9728, 12288, 2048, 4096)])
# generic path: an unlisted n at group 64, and group sizes 32 / 128 (find_cfg returns nothing for G != 64)
GENERIC = [(r, 1536, 64) for r in (QKV, SWIGLU, QUANT, LOGITS)] + [(r, 1024, G) for r in (QKV, SWIGLU, QUANT, LOGITS) for G in (32, 128)]
# group sizes of 4 and more 64-byte steps: a quantization group is a whole wave of float4 slots (256), two waves (512), the whole
# 256-thread workgroup (1024): the prologue's group maximum crosses waves from 512 on
GENERIC += [(r, n, G) for n, G in ((1024, 256), (2048, 512), (2048, 1024)) for r in (QKV, SWIGLU, QUANT, LOGITS)]
HD = 64                        # head_dim of the QKV launches: q rows 256, k / v rows 128 (segments must be whole heads)


def role_rows(role, partial):
    """(rows, rows_kv): a whole number of row tiles for every tile height (multiples of 64), or not (odd counts: the last
    wave batch of the last workgroup is partial).  QKV segments are whole heads by construction: no partial form exists."""
    if role == QKV:
        return 256, 128
    if role == LOGITS:
        return (1031 if partial else 1024), 0
    return (203 if partial else 256), 0


def weight_rows(role, rows, rows_kv):
    return rows + 2 * rows_kv if role == QKV else (2 * rows if role == SWIGLU else rows)


def one_hot_weights(rng, d, n, G):
    """row i: int8 weights in group i % (n/G) only, zero elsewhere -> a row's fold has ONE non-zero term, at fold index i % ng.
    With d >= ng rows every fold index 0..ng-1 carries the term in some row (asserted), in one launch."""
    ng = n // G
    assert d >= ng
    wq = np.zeros((d, ng, G), np.int8)
    g = np.arange(d) % ng
    wq[np.arange(d), g] = rng.integers(-127, 128, (d, G)).astype(np.int8)
    assert set(g.tolist()) == set(range(ng))
    ws = (0.5 + rng.random((d, ng))).astype(f32)
    return wq.reshape(d, n), ws


def exact_weights(rng, d, n, G):
    """first ng rows one-hot, the rest dense small integers with power-of-two scales (ref64.exact_int8_case's bound)"""
    ng = n // G
    wq, ws = one_hot_weights(rng, d, n, G)
    ws = (2.0 ** rng.integers(0, 2, (d, ng))).astype(f32)
    wq[ng:] = rng.integers(-3, 4, (d - ng, n)).astype(np.int8)
    wq[:ng] = np.clip(wq[:ng], -3, 3)
    return wq, ws


def exact_activation(rng, n, G):
    """x = xq * xs with |xq| <= 3 except one +-127 per group and xs a power of two: quantize() returns exactly (xq, xs)"""
    ng = n // G
    xq = rng.integers(-3, 4, (ng, G)).astype(np.int8)
    xq[np.arange(ng), rng.integers(0, G, ng)] = rng.choice([-127, 127], ng)
    xs = (2.0 ** rng.integers(-1, 1, ng)).astype(f32)
    # sum over a row of |terms| + |resid|, in units of 1/2 (|w| <= 3, scales <= 2 and <= 1): every partial sum exact
    assert ng * 3 * (3 * (G - 1) + 127) * 2 * 2 + 4000 < 2 ** 24
    return xq.reshape(-1), xs


def cancelling_weights(rng, d, n, G):
    """group scales over 2^-20 .. 2^20; the second half of the groups repeats the first with the weights negated and the scale
    times (1 + 2^-10): with an activation whose two halves are equal the terms cancel pairwise to 2^-10 of themselves."""
    ng = n // G
    h = ng // 2
    assert ng % 2 == 0
    wq = rng.integers(-127, 128, (d, ng, G)).astype(np.int8)
    wq[:, h:] = -wq[:, :h]
    ws = (2.0 ** rng.uniform(-20, 20, (d, ng))).astype(f32)
    ws[:, h:] = (ws[:, :h] * f32(1 + 2.0 ** -10)).astype(f32)
    return wq.reshape(d, n), ws


def normal_weights(rng, oracle, d, n, G):
    w = (rng.standard_normal(d * n) / np.sqrt(n)).astype(f32)
    wq, ws = oracle.quantize(w, G)
    return wq.reshape(d, n), ws.reshape(d, n // G)


def check_role(ops, oracle, role, n, G, rows, rows_kv, family, strict, wq, ws, x=None, norm_w=None, pre=None, resid=None,
               exact=False, check_tap=True, want_table=None, tap_exact=False):
    """One launch of one role against (a) float64 with the derived budgets, (b) the strict C oracle bit for bit when the mode
    is strict or the inputs are exact.  Budgets:
       normalised vector (NORM roles, the kernel's tap): |y64| * ref64.rmsnorm_rel_budget(n)  [(n/2 + 5) u];
       the int8 operand is then quantize(tap) on the host (elementwise IEEE, order-free), so no int8 flip can leak into (c);
       row sums: gamma(n/G - 1) * A per row (ref64.gemv_budget);
       x += epilogue: one more rounding of the result, u (|resid + S| + E);   SwiGLU epilogue: ref64.swiglu_budget."""
    shape = f"{ROLE_NAMES[role]}:n{n}:g{G}:rows{rows}"
    dw = weight_rows(role, rows, rows_kv)
    r = ops.gemv_role(role, wq, ws, n, rows, G, x=x, norm_w=norm_w, pre_q=None if pre is None else pre[0],
                      pre_s=None if pre is None else pre[1], out=resid, rows_kv=rows_kv, head_dim=HD if role == QKV else 0,
                      strict=strict)
    if want_table is not None:
        assert r["info"][0] == (1 if want_table else 0), (shape, r["info"])
    worst = 0.0
    if role in NORM_ROLES:
        tap = r["tap"]
        if check_tap:
            y64 = ref64.rmsnorm64(x, norm_w)
            worst = max(worst, ratio("rmsnorm_tap", shape, family, strict, tap, y64, np.abs(y64) * ref64.rmsnorm_rel_budget(n) + ref64.TINY))
        if strict or tap_exact:
            assert_biteq(tap, oracle.rmsnorm(x, norm_w), f"{shape} {family} {'strict' if strict else 'fast'}: normalised vector")
        xq, xs = oracle.quantize(tap, G)
    elif role == QUANT:
        xq, xs = oracle.quantize(x, G)
    else:
        xq, xs = pre
    S, A = ref64.gemv_rows(xq, xs, wq, ws, n, dw, G)
    E = ref64.gemv_budget(n, G, A)
    rows32 = oracle.matmul(xq, xs, wq, ws, n, dw, G)
    if role in (QUANT, PREQR):
        want64 = np.asarray(resid, np.float64) + S
        budget = E + U * (np.abs(want64) + E)
        want32 = (np.asarray(resid, f32) + rows32).astype(f32)
    elif role == SWIGLU:
        want64 = ref64.swiglu64(S[:rows], S[rows:])
        budget = ref64.swiglu_budget(S[:rows], S[rows:], E[:rows], E[rows:])
        want32 = oracle.swiglu(rows32[:rows], rows32[rows:])
    else:
        want64, budget, want32 = S, E, rows32
    worst = max(worst, ratio("gemv_" + ROLE_NAMES[role], shape, family, strict, r["out"], want64, budget))
    assert worst <= 1.0, (shape, family, "strict" if strict else "fast", worst)
    if strict or exact:
        assert_biteq(r["out"], want32, f"{shape} {family} {'strict' if strict else 'fast'}: bit equality with the C oracle")
    if role == LOGITS:
        # Sampler::sample_argmax (sampler.rs:57-59) of the logits THE DEVICE returned: last maximum under total_cmp
        assert r["argmax"] == oracle.sample_argmax(r["out"]), (shape, family, r["argmax"])
    return r


def role_inputs(rng, role, n, G, periodic=False, scale_spread=0):
    """N(0,1) activation (optionally with per-group scales over 2^-spread .. 2^spread and two equal halves) and norm weight"""
    ng = n // G
    x = rng.standard_normal(n)
    if scale_spread:
        x = (x.reshape(ng, G) * 2.0 ** rng.uniform(-scale_spread, scale_spread, (ng, 1))).reshape(-1)
    w = 1 + 0.1 * rng.standard_normal(n)
    if periodic:
        x[n // 2:] = x[:n // 2]
        w[n // 2:] = w[:n // 2]
    return x.astype(f32), (w.astype(f32) if role in NORM_ROLES else None)


def run_families(ops, oracle, role, n, G, strict, want_table):
    seed = 1000 * n + 10 * role + G
    rng = np.random.default_rng(seed)
    rows, rows_kv = role_rows(role, partial=True)
    dw = weight_rows(role, rows, rows_kv)
    ng = n // G
    kw = dict(want_table=want_table)
    resid = lambda exact=False: ((rng.integers(-2000, 2001, rows) * 0.5) if exact else rng.standard_normal(rows)).astype(f32) \
        if role in (QUANT, PREQR) else None
    # --- exact arithmetic + one-hot: bit equality in both modes
    if role in NORM_ROLES:
        # the operand is quantize(RMSNorm(x)): its scales are not powers of two, so only one-hot rows are exact here
        # (one non-zero term per row: adding the other rows' +0.0 terms is exact in every order).  x itself is from the exact
        # family of the RMSNorm sum: multiples of 1/2 up to 1, so the sum of squares (multiples of 1/4 below 2^14) is exact in
        # every order and the normalised vector must carry the strict oracle's bits in tolerance mode too
        x, nw = role_inputs(rng, role, n, G)
        x = (rng.integers(-2, 3, n) * 0.5).astype(f32)
        wq, ws = one_hot_weights(rng, dw, n, G)
        if role == SWIGLU:          # W3's one-hot group differs from W1's in the same hidden unit
            wq[rows:] = np.roll(wq[rows:].reshape(rows, ng, G), 7, axis=1).reshape(rows, n)
        check_role(ops, oracle, role, n, G, rows, rows_kv, "one-hot", strict, wq, ws, x=x, norm_w=nw, exact=True, tap_exact=True, **kw)
    else:
        xq, xs = exact_activation(rng, n, G)
        wq, ws = exact_weights(rng, dw, n, G)
        x = (xq.astype(f32).reshape(ng, G) * xs[:, None]).reshape(-1)
        if role == QUANT:
            q2, s2 = oracle.quantize(x, G)
            assert np.array_equal(q2, xq) and np.array_equal(s2, xs)
        check_role(ops, oracle, role, n, G, rows, rows_kv, "exact+one-hot", strict, wq, ws, x=x if role == QUANT else None,
                   pre=(xq, xs) if role == PREQR else None, resid=resid(True), exact=True, **kw)
    # --- badly scaled, cancelling
    x, nw = role_inputs(rng, role, n, G, periodic=True, scale_spread=6)
    wq, ws = cancelling_weights(rng, dw, n, G)
    pre = oracle.quantize(x, G) if role == PREQR else None
    xq_, xs_ = oracle.quantize(oracle.rmsnorm(x, nw) if role in NORM_ROLES else x, G)
    S, A = ref64.gemv_rows(xq_, xs_, wq, ws, n, dw, G)
    assert np.median(A / np.maximum(np.abs(S), 1e-300)) >= 1e3, "the generator must produce heavy cancellation"
    check_role(ops, oracle, role, n, G, rows, rows_kv, "cancelling", strict, wq, ws, x=None if role == PREQR else x, norm_w=nw,
               pre=pre, resid=resid(), **kw)
    # --- N(0,1), once with whole row tiles
    for partial in (True, False):
        if role == QKV and not partial:
            continue
        rws, rkv = role_rows(role, partial)
        d2 = weight_rows(role, rws, rkv)
        x, nw = role_inputs(rng, role, n, G)
        wq, ws = normal_weights(rng, oracle, d2, n, G)
        rs = rng.standard_normal(rws).astype(f32) if role in (QUANT, PREQR) else None
        check_role(ops, oracle, role, n, G, rws, rkv, "normal" if partial else "normal-whole-tiles", strict, wq, ws,
                   x=None if role == PREQR else x, norm_w=nw, pre=oracle.quantize(x, G) if role == PREQR else None, resid=rs, **kw)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("role,n", TABLE, ids=[f"{ROLE_NAMES[r]}-{n}" for r, n in TABLE])
def test_gemv_role_table_entries(ops, oracle, role, n, strict):
    """Every entry of kGemvCfgs (strict) and kGemvCfgsFast (tolerance mode, FIN = 2 tree fold), launched as the planner launches
    it, on the three input families.  One-hot coverage of the group fold: row i carries its only non-zero term at fold index
    i % (n/64) and there are more rows than fold indices, so every index of the tree is exercised in one launch."""
    run_families(ops, oracle, role, n, 64, strict, want_table=True)


NORM_TABLE = [(r, n) for r, n in TABLE if r in NORM_ROLES] + [(QKV, 1536), (LOGITS, 768)]


@pytest.mark.parametrize("role,n", NORM_TABLE, ids=[f"{ROLE_NAMES[r]}-{n}" for r, n in NORM_TABLE])
def test_norm_prologue_tree_counts_every_term_once(ops, oracle, role, n):
    """One-hot coverage of the RMSNorm tree inside the fused NORM prologues (tolerance mode): x = 3 at index i, zero elsewhere;
    the sum of squares is exactly 9 whatever the order, so the tapped normalised vector must equal the strict oracle's bit for
    bit.  i runs over EVERY index 0..n-1, for every NORM instantiation of the table (QKV, SwiGLU and classifier forms are
    separately compiled kernels with their own workgroup width and elements per thread) and for the generic prologue at the
    unlisted 1536 / 768: one launch per index, so every (lane, wave, slot) position of each tree carries the term once."""
    G = 64
    rng = np.random.default_rng(n + role)
    rows, rows_kv = (64, 64) if role == QKV else (8, 0)
    dw = weight_rows(role, rows, rows_kv)
    wq, ws = np.zeros((dw, n), np.int8), np.ones((dw, n // G), f32)
    nw = (1 + 0.1 * rng.standard_normal(n)).astype(f32)
    for i in range(n):
        x = np.zeros(n, f32)
        x[i] = 3.0
        r = ops.gemv_role(role, wq, ws, n, rows, G, x=x, norm_w=nw, rows_kv=rows_kv, head_dim=HD if role == QKV else 0, strict=False)
        assert_biteq(r["tap"], oracle.rmsnorm(x, nw), f"{ROLE_NAMES[role]} n={n}: one-hot at {i}")
        assert not np.any(r["out"] != 0)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("role,n,G", GENERIC, ids=[f"{ROLE_NAMES[r]}-{n}-g{G}" for r, n, G in GENERIC])
def test_gemv_role_generic_path(ops, oracle, role, n, G, strict):
    """Shapes without a table entry (an unlisted n; group sizes 32, 128, 256, 512 and 1024) take the run-time-n kernels."""
    run_families(ops, oracle, role, n, G, strict, want_table=False)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("role,n", [(QKV, 2560), (SWIGLU, 1024), (LOGITS, 4096), (QUANT, 9728), (QUANT, 2048), (PREQR, 4096)],
                         ids=lambda v: str(v))
def test_gemv_role_special_values(ops, oracle, role, n, strict):
    """Saturated dots (+-127 everywhere), an all-zero activation group, an all-zero vector (the reference's 0/0 quantize:
    scale 0, q 0) and rows whose every term underflows to -0.0 (the fold starts from -0.0, tensor.rs:53-60: in reference order
    the sign of a zero result must match the oracle; in tolerance mode it must be a zero -- the budget is 0 there)."""
    G = 64
    rng = np.random.default_rng(77 + n + role)
    rows, rows_kv = role_rows(role, partial=True)
    dw = weight_rows(role, rows, rows_kv)
    ng = n // G
    nw = np.ones(n, f32) if role in NORM_ROLES else None
    resid = (lambda: rng.standard_normal(rows).astype(f32)) if role in (QUANT, PREQR) else (lambda: None)

    def go(family, x, wq, ws, rs=None, **kw):
        pre = oracle.quantize(x, G) if role == PREQR else None
        return check_role(ops, oracle, role, n, G, rows, rows_kv, family, strict, wq, ws, x=None if role == PREQR else x,
                          norm_w=nw, pre=pre, resid=resid() if rs is None else rs, want_table=True, **kw)
    sat_w = rng.choice(np.array([-127, 127], np.int8), (dw, n))
    go("saturated", (0.75 * rng.choice([-1.0, 1.0], n)).astype(f32), sat_w, np.ones((dw, ng), f32))
    x = rng.standard_normal(n).astype(f32)
    x[G:2 * G] = 0.0
    x[-G:] = 0.0
    wq, ws = normal_weights(rng, oracle, dw, n, G)
    go("zero-groups", x, wq, ws)
    r = go("zero-vector", np.zeros(n, f32), wq, ws, rs=np.zeros(rows, f32) if role in (QUANT, PREQR) else None)
    assert not np.any(r["out"] != 0)
    if role != PREQR:            # (an attention epilogue never hands PREQR a zero scale next to non-zero int8 values)
        neg = np.full((dw, n), -1, np.int8)
        tiny_x = np.full(n, 2.0 ** -100, f32)
        r = go("all-terms-minus-zero", tiny_x, neg, np.full((dw, ng), 2.0 ** -70, f32),
               rs=np.full(rows, -0.0, f32) if role in (QUANT, PREQR) else None, check_tap=False)
        assert not np.any(r["out"] != 0)


def test_gemv_role_rejects_what_the_planner_cannot_launch(ops, q3):
    """Unsupported combinations return Q3_ERR_UNSUPPORTED (-5) before any launch; a bad role is Q3_ERR_ARG (-3)."""
    z = lambda *s: np.zeros(s, np.int8)
    o = lambda *s: np.ones(s, f32)
    bad = [dict(role=PREQR, n=1536, G=64, pre_q=z(1536), pre_s=o(24)),            # PREQR exists for the listed n only
           dict(role=PREQR, n=2048, G=128, pre_q=z(2048), pre_s=o(16)),
           dict(role=QUANT, n=1000, G=64, x=o(1000)),                              # n not a multiple of the group
           dict(role=QUANT, n=96, G=48, x=o(96)),                                  # group not a power of two
           dict(role=LOGITS, n=32768, G=64, x=o(32768), norm_w=o(32768))]          # beyond the LDS-staged activation
    for b in bad:
        n, G = b["n"], b["G"]
        with pytest.raises(q3.Q3Error) as e:
            ops.gemv_role(b["role"], z(4 * n), o(4 * (n // G)), n, 4, G, x=b.get("x"), norm_w=b.get("norm_w"), pre_q=b.get("pre_q"),
                          pre_s=b.get("pre_s"), out=o(4))
        assert e.value.code == -5, (b["role"], n, G, e.value)
    with pytest.raises(q3.Q3Error) as e:
        ops.gemv_role(9, z(4 * 64), o(4), 64, 4, 64, x=o(64), out=o(4))
    assert e.value.code == -3
    with pytest.raises(q3.Q3Error) as e:           # q / k / v segments must be whole heads
        ops.gemv_role(QKV, z(48 * 1024), o(48 * 16), 1024, 16, 64, x=o(1024), norm_w=o(1024), rows_kv=16, head_dim=64)
    assert e.value.code == -5


def test_logits_role_argmax_ties_and_signed_zero(ops, oracle):
    """LOGITS role: the argmax the launch computes is the LAST maximum under total_cmp of the logits it returned, with rows built
    to tie exactly (duplicated weight rows, spread over different workgroups) and with a -0.0 / +0.0 pair as the maximum."""
    n, G, rows = 1024, 64, 1031
    rng = np.random.default_rng(5)
    x = rng.standard_normal(n).astype(f32)
    nw = np.ones(n, f32)
    wq, ws = normal_weights(rng, oracle, rows, n, G)
    for strict in (True, False):
        base = ops.gemv_role(LOGITS, wq, ws, n, rows, G, x=x, norm_w=nw, strict=strict)
        top = int(np.argmax(base["out"]))
        w2, s2 = wq.copy(), ws.copy()
        for dup in (3, 517, 1030):                       # the winning row, three more times: exact ties, the last index wins
            w2[dup], s2[dup] = wq[top], ws[top]
        r = ops.gemv_role(LOGITS, w2, s2, n, rows, G, x=x, norm_w=nw, strict=strict)
        assert r["out"][3] == r["out"][517] == r["out"][1030] == r["out"].max()
        assert r["argmax"] == max(1030, top) == oracle.sample_argmax(r["out"])
        # every logit negative except two zeros of either sign: +0.0 > -0.0 under total_cmp whatever their indices
        xq, xs = oracle.quantize(base["tap"], G)         # the operand this mode's launch quantizes
        w3 = np.where(xq[None, :].astype(np.int32) * wq > 0, -wq, wq).astype(np.int8)   # every product <= 0: every logit <= 0
        w3[w3 == -128] = -127
        w3[700] = 0
        w3[200] = 0
        s3 = ws.copy()
        s3[200] = -s3[200]                               # 0 * negative scale = -0.0 in every term: logit -0.0 (fold from -0.0)
        r = ops.gemv_role(LOGITS, w3, s3, n, rows, G, x=x, norm_w=nw, strict=strict)
        assert np.all(r["out"] <= 0) and r["out"][700] == 0 and r["out"][200] == 0
        assert r["argmax"] == oracle.sample_argmax(r["out"])
        if strict:
            assert np.signbit(r["out"][200]) and not np.signbit(r["out"][700]) and r["argmax"] == 700


# ----------------------------------------------------------------------------------------------------------------------
# 2. q3_op_rmsnorm / q3_op_softmax / q3_op_attention
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 128, 1024, 2560, 4096, 8192, 1000])
def test_rmsnorm_fp64(ops, oracle, n):
    """Budget: ref64.rmsnorm_rel_budget, (n/2 + 5) u relative per element.  Exact family: entries in {+-1, +-2, 0} times one power of
    two -- the sum of squares is an integer below 2^24 in every order, so both modes must return the strict oracle's bits.
    One-hot: a single non-zero entry at index i, for EVERY i in 0..n-1 (n launches for n <= 1024; for larger n the stride-61 walk
    plus both ends: 61 is coprime to 64 and 256, so the walk visits every lane, every wave and every per-thread slot of the
    256-thread strided loop; the exhaustive sweep of a large n runs through the fused prologue in test_gemv_role_*)."""
    rng = np.random.default_rng(n)
    w = (1 + 0.1 * rng.standard_normal(n)).astype(f32)
    for k in (0, -7, 9):
        x = (rng.integers(-2, 3, n) * 2.0 ** k).astype(f32)
        ref = oracle.rmsnorm(x, w)
        for strict in (True, False):
            assert_biteq(ops.rmsnorm(x, w, strict=strict), ref, f"exact family 2^{k} strict={strict}")
    idx = list(range(n)) if n <= 1024 else sorted(set(range(0, n, 61)) | {n - 1, n - 2, n - 64, n - 256})
    for i in idx:
        x = np.zeros(n, f32)
        x[i] = 3.0
        assert_biteq(ops.rmsnorm(x, w, strict=False), oracle.rmsnorm(x, w), f"one-hot {i}")
    fams = {"normal": rng.standard_normal(n), "bad-scale": rng.standard_normal(n) * 2.0 ** rng.uniform(-20, 20, n)}
    for fam, x in fams.items():
        x = x.astype(f32)
        y64 = ref64.rmsnorm64(x, w)
        for strict in (True, False):
            got = ops.rmsnorm(x, w, strict=strict)
            assert ratio("rmsnorm", f"n{n}", fam, strict, got, y64, np.abs(y64) * ref64.rmsnorm_rel_budget(n) + ref64.TINY) <= 1.0
            if strict:
                assert_biteq(got, oracle.rmsnorm(x, w))


@pytest.mark.parametrize("n", [1, 7, 64, 65, 777, 5000, 40960])
def test_softmax_fp64(ops, oracle, n):
    """Budget: ref64.softmax_budget, (n + 213) u relative per element + 2^-126; the outputs must also sum to 1 within the sum of
    the per-element budgets.  Exact family: one dominant score (every other exponential underflows to 0: weights exactly one-hot)
    with the dominant index swept -- every index for n <= 777, else stride 61 (coprime to the 256-thread stride) plus both ends;
    all-equal scores with n a power of two are exact too (1/n).  Badly scaled: scores spread over +-80."""
    rng = np.random.default_rng(n)
    idx = list(range(n)) if n <= 777 else sorted(set(range(0, n, 61 if n < 10000 else 509)) | {0, n - 1, n - 2})
    for i in idx:
        a = np.full(n, -150.0, f32)
        a[i] = 11.0
        want = np.zeros(n, f32)
        want[i] = 1.0
        assert_biteq(ops.softmax(a, strict=False), want, f"dominant score at {i}")
    fams = {"all-equal": np.full(n, 3.25), "spread-80": rng.uniform(-80, 80, n), "normal": rng.standard_normal(n)}
    for fam, a in fams.items():
        a = a.astype(f32)
        p64, bud = ref64.softmax64(a), ref64.softmax_budget(a)
        for strict in (True, False):
            got = ops.softmax(a, strict=strict)
            assert ratio("softmax", f"n{n}", fam, strict, got, p64, bud) <= 1.0
            assert abs(float(got.astype(np.float64).sum()) - 1.0) <= float(bud.sum())
            if strict or fam == "all-equal":             # n equal exponentials sum to n exactly in every order (n < 2^24)
                assert_biteq(got, oracle.softmax(a), f"{fam} strict={strict}")


ATT_SHAPES = [(4, 2, 16, 64, 9), (16, 8, 128, 256, 200), (8, 8, 64, 32, 0), (4, 1, 32, 700, 650), (16, 8, 128, 160, 127),
              (16, 8, 128, 160, 128), (32, 8, 128, 300, 299),                                   # test_attention
              (16, 8, 128, 256, 7), (16, 8, 128, 256, 63), (16, 8, 128, 256, 64), (16, 8, 128, 256, 65), (16, 8, 128, 256, 255),
              (32, 8, 128, 136, 100), (16, 8, 128, 100, 99),                                    # ..._short_contexts_head_dim_128
              (16, 8, 128, 512, 256), (16, 8, 128, 512, 257), (4, 2, 64, 512, 255), (4, 2, 64, 512, 256),   # the plan boundary
              (4, 2, 64, 1100, 1023), (4, 2, 64, 1100, 1024), (4, 2, 64, 1100, 1025)]           # a chunk edge of the split path
ATT_LONG = [(4, 2, 64, 4600, 4500), (8, 2, 128, 4600, 4500), (4, 2, 128, 8500, 8400), (8, 2, 128, 4096, 4095)]


def _att_inputs(rng, nh, nkv, hd, S, kscale=1.0):
    kvd = nkv * hd
    q = rng.standard_normal(nh * hd).astype(f32)
    K = (kscale * rng.standard_normal((S, kvd))).astype(f32)
    V = rng.standard_normal((S, kvd)).astype(f32)
    qw = (1 + 0.1 * rng.standard_normal(hd)).astype(f32)
    kw = (1 + 0.1 * rng.standard_normal(hd)).astype(f32)
    return q, K, V, qw, kw


def _att_check(ops, oracle, shape, fam, q, K, V, qw, kw, strict):
    nh, nkv, hd, S, pos = shape
    ref = ref64.attention64(q, K, V, qw, kw, pos, nh, nkv, hd, oracle.rope_freqs(hd, pos))
    xb, q2, k2 = ops.attention(q, K, V, qw, kw, pos, nh, nkv, hd, strict=strict)
    name = "x".join(str(v) for v in shape)
    w = max(ratio("attention_q", name, fam, strict, q2, ref["q"], ref["q_budget"]),
            ratio("attention_krow", name, fam, strict, k2.reshape(S, -1)[pos], ref["krow"], ref["krow_budget"]),
            ratio("attention_xb", name, fam, strict, xb, ref["xb"], ref["xb_budget"]))
    assert w <= 1.0, (shape, fam, strict, w)
    return xb


def _att_dominant_sweep(ops, oracle, shape, rng):
    nh, nkv, hd, S, pos = shape
    # dominant score: all query heads share one raw vector, key rows are -60 sign(q_hat) except row t* (+60 sign(q_hat)); the row
    # of the current position is the negated raw query (k_hat = -q_hat with equal norm weights).  Scores: +60 s / -60 s / -|q_hat|^2
    # / sqrt(hd) with s = sum |q_hat| / sqrt(hd) >= 0.5 sqrt(hd): the gap to the dominant score exceeds 104 for hd >= 16.
    ones = np.ones(hd, f32)
    q1 = np.tile(rng.standard_normal(hd).astype(f32), nh)
    qhat = oracle.attention(q1, np.zeros((S, nkv * hd), f32), np.zeros((S, nkv * hd), f32), ones, ones, pos, nh, nkv, hd)[1][:hd]
    assert 60 * np.abs(qhat).sum() / np.sqrt(hd) > 104
    sgn = np.tile(np.where(qhat >= 0, 1.0, -1.0).astype(f32), nkv)
    Vi = rng.integers(-999, 1000, (S, nkv * hd)).astype(f32)
    if pos < 300:
        ts = list(range(pos))
    else:
        ts = sorted(t for t in set(range(0, pos, 61)) | {0, pos - 1} | {m + d for m in range(256, pos, 256) for d in (-1, 0, 1)} if t < pos)
    for t in ts:
        Kd = np.tile(-60 * sgn, (S, 1)).astype(f32)
        Kd[t] = 60 * sgn
        Kd[pos] = -q1[:nkv * hd]
        want = np.tile(Vi[t].reshape(nkv, 1, hd), (1, nh // nkv, 1)).reshape(-1)
        for strict in ((True, False) if t in (ts[0], ts[-1]) else (False,)):
            xb, _, _ = ops.attention(q1, Kd, Vi, ones, ones, pos, nh, nkv, hd, strict=strict)
            assert_biteq(xb, want, f"dominant score at t={t} strict={strict}")


@pytest.mark.parametrize("shape", ATT_SHAPES + ATT_LONG, ids=lambda s: "x".join(str(v) for v in s))
def test_attention_fp64(ops, oracle, shape):
    """QK-norm + RoPE + GQA attention of one layer against ref64.attention64 (budget derivation in its docstring), in both modes,
    on the shapes of test_attention / ..._short_contexts_head_dim_128 / ..._long_context and either side of the plan boundaries
    (63/64/65, 255/256/257, a chunk edge of the split path).  Families: N(0,1); badly scaled value rows (2^-20 .. 2^20 per
    timestep, mixed signs: heavy cancellation in sum att * V) with scores spread wide (keys x 4).
    Exact family, swept as the one-hot coverage of both attention sums: one DOMINANT score at timestep t* -- every other
    exponential underflows to exactly 0, the softmax row is exactly one-hot and xb must equal the value row t* bit for bit, in
    both modes.  t* runs over every timestep for pos < 300 (every term index of both sums: all lanes, waves and chunk slots of
    the single-kernel and short-context forms and of the first split chunks); longer contexts walk with stride 61 -- coprime to
    64 with at least 64 samples, so every lane of a wave carries the term; the wave / chunk slots beyond are sampled, not
    exhausted -- plus both ends and the neighbours of every multiple of 256."""
    nh, nkv, hd, S, pos = shape
    rng = np.random.default_rng(sum(shape))
    if pos > 0:
        _att_dominant_sweep(ops, oracle, shape, rng)
    q, K, V, qw, kw = _att_inputs(rng, nh, nkv, hd, S, 0.5 if pos > 1000 else 1.0)
    for strict in (True, False):
        xb = _att_check(ops, oracle, shape, "normal", q, K, V, qw, kw, strict)
        if strict:
            assert_biteq(xb, oracle.attention(q, K, V, qw, kw, pos, nh, nkv, hd)[0])
    V2 = (V * 2.0 ** rng.uniform(-20, 20, (S, 1))).astype(f32)
    for strict in (True, False):
        _att_check(ops, oracle, shape, "bad-scale", q, (4 * K).astype(f32), V2, qw, kw, strict)


# ----------------------------------------------------------------------------------------------------------------------
# 3. Engine level: paths with no operator entry
# ----------------------------------------------------------------------------------------------------------------------
L2 = ["qwen3-0.6b-dims-l2", "qwen3-4b-dims-l2", "qwen3-8b-dims-l2"]
SIGMA_BOUND = 0.15       # the project's stated tolerance (test_tolerance_mode_on_the_listed_layer_dims): x std of the strict logits


def _ckpt(q3, name, seed=1235):
    ck = q3.checkpoint
    path = os.path.join(os.environ.get("Q3_CKPT_DIR", "/tmp"), f"q3_{name}{'' if seed == 1235 else '_s%d' % seed}.bin")
    ck.ensure_synthetic_checkpoint(path, ck.SHAPES[name], seed=seed)
    return path


def _within(a, b, what):
    assert np.all(np.isfinite(a)), what
    d, s = float(np.max(np.abs(a - b))), float(np.std(b))
    print(f"TOLBUDGET|engine_logits|{what}|stated-0.15-sigma|fast|{d / (SIGMA_BOUND * s):.4f}")
    assert d <= SIGMA_BOUND * s, (what, d, s)


@pytest.mark.parametrize("name", L2)
def test_fast_engines_are_deterministic_and_flag_variants_agree(q3, oracle, name):
    """Tolerance mode is reordered, not nondeterministic (no float atomics in a sum): two FAST engines on the same inputs, and one
    FAST engine after q3_reset_kv, return identical bits.  FAST + Q3_FLAG_NO_VALUE_T equals plain FAST bit for bit (FAST never
    allocates the transposed copy); FAST + Q3_FLAG_NO_GRAPH meets the stated 0.15 sigma bound against the strict oracle and
    equals the graph-replayed engine bit for bit (same kernels, launched eagerly)."""
    path = _ckpt(q3, name)
    om = oracle.OracleModel(path, 256)
    toks = [3, 17, 4000, 5, 9]
    runs = []
    for build in (lambda b: b, lambda b: b, lambda b: b.with_value_transposed(False), lambda b: b.with_graph(False)):
        with build(q3.TransformerBuilder(path).with_ctx_length(256).with_strict(False)).build() as t:
            runs.append([np.array(t.forward(tok, pos), copy=True) for pos, tok in enumerate(toks)])
            if len(runs) == 1:
                t.reset_kv()
                again = [np.array(t.forward(tok, pos), copy=True) for pos, tok in enumerate(toks)]
                for pos in range(len(toks)):
                    assert_biteq(again[pos], runs[0][pos], f"{name} pos {pos}: the same engine after reset_kv")
    for pos, tok in enumerate(toks):
        b = om.forward(tok, pos)
        for k, what in ((1, "second FAST engine"), (2, "FAST + NO_VALUE_T"), (3, "FAST + NO_GRAPH")):
            assert_biteq(runs[k][pos], runs[0][pos], f"{name} pos {pos}: {what}")
        _within(runs[3][pos], b, f"{name}:no-graph:pos{pos}")


@pytest.mark.parametrize("name", L2)
def test_fast_batch32_decode_within_the_stated_bound(q3, oracle, name):
    """FAST batch-32 decode (k_bquant_split prologues, batched attention): every stream against the strict oracle fed the same
    tokens, 0.15 sigma, finite everywhere; and a second identical batched run returns identical bits."""
    path = _ckpt(q3, name)
    rng = np.random.default_rng(3)
    V = q3.checkpoint.SHAPES[name].vocab_size
    toks = [[int(v) for v in rng.integers(0, V, 32)] for _ in range(3)]
    pos0 = [int(p) for p in rng.integers(0, 4, 32)]
    with q3.TransformerBuilder(path).with_ctx_length(256).with_strict(False).build() as t:
        t.batch_init(32)
        got = [t.forward_batch(toks[k], [p + k for p in pos0])[0].copy() for k in range(3)]
        t.batch_reset_kv()
        for k in range(3):
            assert_biteq(t.forward_batch(toks[k], [p + k for p in pos0])[0], got[k], f"{name} step {k}: second batched run")
    om = oracle.OracleModel(path, 256)
    for i in (0, 1, 13, 31):
        om.reset()
        for k in range(3):
            _within(got[k][i], om.forward(toks[k][i], pos0[i] + k), f"{name}:batch32:stream{i}:step{k}")


@pytest.mark.parametrize("name,n_prompt", [("qwen3-0.6b-dims-l2", 81), ("qwen3-4b-dims-l2", 40), ("small-longctx", 257)])
def test_fast_dense_prefill_then_decode_within_the_stated_bound(q3, oracle, name, n_prompt):
    """FAST q3_prefill_batched (dense prefill; a ragged block) followed by decode: the logits of the next forwards against the
    strict oracle walked through the same tokens."""
    path = _ckpt(q3, name, seed=1235 if name != "small-longctx" else 77)
    shape = q3.checkpoint.SHAPES[name]
    ctx = 512
    prompt = q3.checkpoint.iter_prompt_tokens(shape, 5, n_prompt)
    om = oracle.OracleModel(path, ctx)
    for pos, tok in enumerate(prompt):
        om.forward(tok, pos)
    with q3.TransformerBuilder(path).with_ctx_length(ctx).with_strict(False).build() as t:
        t.prefill(prompt, 0, batched=True)
        tok = 7
        for pos in range(n_prompt, n_prompt + 3):
            a, b = np.array(t.forward(tok, pos), copy=True), om.forward(tok, pos)
            _within(a, b, f"{name}:prefill{n_prompt}:pos{pos}")
            tok = oracle.sample_argmax(b)


def test_fast_engine_past_the_split_and_a_chunk_edge(q3, oracle):
    """A FAST engine past position 256 (the split long-context plan: k_attn_scores_kv / k_attn_out tree sums, no transposed
    value cache) and past 1,024: stated bound against the strict oracle at positions either side of both edges."""
    name = "small-longctx"
    path = _ckpt(q3, name, seed=77)
    shape = q3.checkpoint.SHAPES[name]
    ctx, last = 1100, 1030
    prompt = q3.checkpoint.iter_prompt_tokens(shape, 9, last + 1)
    om = oracle.OracleModel(path, ctx)
    check = {254, 255, 256, 257, 258, 511, 512, 513, 1023, 1024, 1025, last}
    with q3.TransformerBuilder(path).with_ctx_length(ctx).with_strict(False).build() as t:
        for pos, tok in enumerate(prompt):
            b = om.forward(tok, pos)
            if pos in check:
                _within(np.array(t.forward(tok, pos), copy=True), b, f"{name}:pos{pos}")
            else:
                t.forward_argmax(tok, pos)


# ----------------------------------------------------------------------------------------------------------------------
# First-layer value rows, screened: one quantization deep, so the fold budget applies inside an engine
# ----------------------------------------------------------------------------------------------------------------------
SCREEN_SHAPES = ["qwen3-0.6b-dims-l2", "qwen3-4b-dims-l2", "qwen3-8b-dims-l2", "small-longctx"]
SCREEN_SEED = {"small-longctx": 77}
POOL_SIZE, MIN_YIELD = 64, 16


def candidate_pool(shape):
    """the fixed pool of 64 candidate tokens of a shape (inside the first 4,096 rows of the embedding table)"""
    return [(37 * k + 5) % min(shape.vocab_size, 4096) for k in range(POOL_SIZE)]


def layer0_tensors(ck, shape, seed):
    """What a layer-0 value row depends on, regenerated from the synthetic checkpoint's generator (checkpoint.py,
    write_synthetic_checkpoint: tensors are keyed by (seed, tensor, item, chunk)): the first 4,096 embedding rows, the layer-0
    attention RMSNorm weight and the layer-0 value projection.  The GPU tests compare these with the bytes of the file the engine
    loaded (layer0_check_file)."""
    g, dim, kvd = shape.group_size, shape.dim, shape.kv_dim
    rows = min(4096, shape.vocab_size)
    eq, es = ck._synth_chunk(seed, 0, 0, 0, rows * dim, 0.05, g)
    tv = [t[0] for t in shape.quantized_tensors()].index("v_proj")
    assert kvd <= 4096
    vq, vs = ck._synth_chunk(seed, tv, 0, 0, kvd * dim, float(dim) ** -0.5, g)
    w = (1.0 + 0.1 * ck._tensor_rng(seed, 1000, 0, 0).standard_normal(shape.n_layers * dim, dtype=f32)).astype(f32)[:dim]
    return {"eq": eq.reshape(rows, dim), "es": es.reshape(rows, dim // g), "vq": vq.reshape(kvd, dim), "vs": vs.reshape(kvd, dim // g), "w": w}


def layer0_check_file(ck, path, shape, t0):
    off = ck.tensor_offsets(shape)
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    rows, dim, g, kvd = t0["eq"].shape[0], shape.dim, shape.group_size, shape.kv_dim
    q0, s0, _ = off["embed_tokens"]
    assert np.array_equal(mm[q0:q0 + rows * dim].view(np.int8).reshape(rows, dim), t0["eq"])
    assert np.array_equal(np.frombuffer(mm[s0:s0 + 4 * rows * dim // g], dtype="<f4").reshape(rows, -1), t0["es"])
    q0, s0, _ = off["v_proj"]
    assert np.array_equal(mm[q0:q0 + kvd * dim].view(np.int8).reshape(kvd, dim), t0["vq"])
    assert np.array_equal(np.frombuffer(mm[s0:s0 + 4 * kvd * dim // g], dtype="<f4").reshape(kvd, -1), t0["vs"])
    a0 = off["input_layernorm"][0]
    assert np.array_equal(np.frombuffer(mm[a0:a0 + 4 * dim], dtype="<f4"), t0["w"])


def screen_tokens(shape, t0, pool):
    """{token: (S, budget)} for the tokens of the pool that survive screening; float64 and the CPU only.

    x = dequantised embedding row ((f32)q * s, exact to reproduce), y = RMSNorm(x) in float64, quotient q_i = y_i / (max_group |y| /
    127).  A token survives if NO quotient lies within delta of a half-integer, delta = 127 c u with c = ceil(log2 n) + 6, the
    relative budget of a tree RMSNorm in units of u (ref64.rmsnorm_tree_rel_budget).  Why that suffices: the device's quotient is
    fl(y'_i / fl(max|y'| / 127)) with y'_i = fl(w_i fl(f' x_i)) and ONE factor f' for the whole vector, whatever order summed it;
    f' cancels in the quotient up to the two roundings of each y' and the two divisions, 6 u relative, i.e. 127 * 6 u absolute --
    below delta for every n (c >= 14).  So round(q_i) is the same int8 for every legitimate order, and it is round() of the float64
    quotient.  What does NOT cancel is the group scale xs_g = fl(max|y'| / 127): it carries the RMSNorm error of the order used,
    relative ref64.rmsnorm_rel_budget(n) + u (any order: the acceptance budget assumes no tree).  Value row r in float64:
    S_r = sum_g dot_rg ws_rg XS_g with XS_g = max|y| / 127; the device's term fl(fl(dot ws) xs') differs from its float64 term by
    (rmsnorm budget + 3 u) |T_g| and the fold adds gamma(n/G - 1) A:   budget_r = A_r (gamma(n/G - 1) + rmsnorm_rel_budget(n) + 3 u)."""
    n, g = shape.dim, shape.group_size
    ng = n // g
    delta = 127.0 * ref64.rmsnorm_tree_rel_budget(n)
    rel = (ref64.gamma(ng - 1) + ref64.rmsnorm_rel_budget(n) + 3 * U) * ref64.SECOND_ORDER
    vq = t0["vq"].reshape(-1, ng, g).astype(np.int64)
    vs = t0["vs"].astype(np.float64)
    out = {}
    for tok in pool:
        x = (t0["eq"][tok].astype(f32).reshape(ng, g) * t0["es"][tok][:, None]).astype(f32).reshape(-1)
        y = ref64.rmsnorm64(x, t0["w"]).reshape(ng, g)
        m = np.abs(y).max(axis=1)
        if np.any(m == 0):
            continue
        quo = y / (m / 127.0)[:, None]
        frac = np.abs(quo) - np.floor(np.abs(quo))
        if np.any(np.abs(frac - 0.5) <= delta):
            continue
        xq = np.rint(quo).astype(np.int64)
        Tg = (vq * xq[None]).sum(axis=2) * vs * (m / 127.0)[None, :]
        out[tok] = (Tg.sum(axis=1), np.abs(Tg).sum(axis=1) * rel + ref64.TINY)
    return out


def _screened(q3, name):
    ck = q3.checkpoint
    shape = ck.SHAPES[name]
    seed = SCREEN_SEED.get(name, 1235)
    path = _ckpt(q3, name, seed)
    t0 = layer0_tensors(ck, shape, seed)
    layer0_check_file(ck, path, shape, t0)
    ok = screen_tokens(shape, t0, candidate_pool(shape))
    assert len(ok) >= MIN_YIELD
    return path, shape, ok


def _check_vrow(row, ref, what, strict=False):
    S, B = ref
    assert ratio("layer0_value_row", what, "screened", strict, row, S, B) <= 1.0, what


@pytest.mark.parametrize("name", SCREEN_SHAPES)
def test_first_layer_value_rows_forward(q3, name):
    """q3_forward: the layer-0 V row (q3_read_state kind 1) of every screened token, FAST and reference order, at several
    positions, within the budget of screen_tokens() against float64."""
    path, shape, ok = _screened(q3, name)
    kvd = shape.kv_dim
    for strict in (False, True):
        with q3.TransformerBuilder(path).with_ctx_length(320).with_strict(strict).build() as t:
            for k, tok in enumerate(ok):
                pos = (k * 7) % 300 if k else 299           # both plans (pos < 256 and the split plan)
                t.forward(tok, pos)
                _check_vrow(t.read_state("value", pos * kvd, kvd), ok[tok], f"{name}:forward:pos{pos}", strict)


@pytest.mark.parametrize("n_streams", [3, 32])
@pytest.mark.parametrize("name", SCREEN_SHAPES)
def test_first_layer_value_rows_batched_decode(q3, name, n_streams):
    """q3_forward_batch FAST (batch-32 prologue k_bquant_split + MFMA GEMM) with 3 and 32 streams at mixed positions: every
    stream's layer-0 V row (q3_batch_read_state) within the budget."""
    path, shape, ok = _screened(q3, name)
    toks = (list(ok) * 3)[:n_streams]
    kvd, ctx = shape.kv_dim, 64
    with q3.TransformerBuilder(path).with_ctx_length(ctx).with_strict(False).build() as t:
        t.batch_init(n_streams)
        for step in range(2):
            pos = [(5 * i + 11 * step) % (ctx - 2) + step for i in range(n_streams)]
            t.forward_batch(toks, pos, want_logits=False)
            for i in range(n_streams):
                _check_vrow(t.batch_read_state(i, "value", pos[i] * kvd, kvd), ok[toks[i]], f"{name}:batch{n_streams}:stream{i}:pos{pos[i]}")
            toks = toks[1:] + toks[:1]


@pytest.mark.parametrize("n_block", ["full", 81, 257])
@pytest.mark.parametrize("name", SCREEN_SHAPES)
def test_first_layer_value_rows_dense_prefill(q3, name, n_block):
    """q3_prefill_batched FAST: a full-size block (2,048 positions, or the whole context where that is shorter) and the ragged
    blocks 81 and 257, every position fed a screened token: each layer-0 V row of the cache within the budget."""
    path, shape, ok = _screened(q3, name)
    ctx = min(2048, shape.max_seq_len)
    n = ctx if n_block == "full" else n_block
    toks = (list(ok) * (n // len(ok) + 1))[:n]
    kvd = shape.kv_dim
    with q3.TransformerBuilder(path).with_ctx_length(ctx).with_strict(False).build() as t:
        t.prefill(toks, 0, batched=True)
        rows = t.read_state("value", 0, n * kvd).reshape(n, kvd)
    S = np.stack([ok[tk][0] for tk in toks])
    B = np.stack([ok[tk][1] for tk in toks])
    assert ratio("layer0_value_row", f"{name}:prefill{n}", "screened", False, rows, S, B) <= 1.0


def test_fast_4b_dims_past_2300(q3, oracle):
    """The 4B layer dims (dim 2560, head_dim 128, four query heads per kv head, 2 layers) as a FAST engine: a sequential device
    prefill walks the split long-context plan from position 256 on, then the forwards at 2,296 .. 2,306 -- across the
    64-timestep chunk edge at 2,304 -- meet the stated 0.15 sigma bound against the strict oracle fed the same tokens."""
    name = "qwen3-4b-dims-l2"
    path = _ckpt(q3, name)
    shape = q3.checkpoint.SHAPES[name]
    ctx, n_prompt, n_dec = 2400, 2296, 11
    prompt = q3.checkpoint.iter_prompt_tokens(shape, 1235, n_prompt)
    om = oracle.OracleModel(path, ctx)
    for p, tok in enumerate(prompt):
        lg = om.forward(tok, p)
    with q3.TransformerBuilder(path).with_ctx_length(ctx).with_strict(False).build() as t:
        t.prefill(prompt, 0)
        tok = oracle.sample_argmax(lg)
        for pos in range(n_prompt, n_prompt + n_dec):
            a, b = np.array(t.forward(tok, pos), copy=True), om.forward(tok, pos)
            _within(a, b, f"{name}:pos{pos}")
            tok = oracle.sample_argmax(b)


@pytest.mark.parametrize("temperature,topp", [(0.7, 0.9), (1.0, 1.0), (1.3, 0.0)])
def test_sampler_behind_fast_logits(q3, oracle, temperature, topp):
    """The sampler stays in reference order in both modes (csrc/q3_sampler.h takes no strict flag: enqueue_sample() passes
    the same SampleArgs whatever the engine's flags).  So: given the logits a FAST engine returned, q3_forward_sample on a twin
    FAST engine draws exactly the token the oracle's Sampler draws FROM THOSE LOGITS, coin for coin."""
    name = "qwen3-0.6b-dims-l2"
    path = _ckpt(q3, name)
    seed = 0x1234ABCD5678EF01
    smp = oracle.Sampler(q3.checkpoint.SHAPES[name].vocab_size, temperature, topp, seed)
    with q3.TransformerBuilder(path).with_ctx_length(256).with_strict(False).build() as a, \
            q3.TransformerBuilder(path).with_ctx_length(256).with_strict(False).build() as b:
        b.set_sampler(temperature, topp, seed)
        tok = 11
        for pos in range(12):
            lg = np.array(a.forward(tok, pos), copy=True)
            want = smp.sample(lg)
            assert b.forward_sample(tok, pos) == want, f"pos {pos}"
            tok = want
        assert b.sampler_rng_state() == smp.rng_state.value
