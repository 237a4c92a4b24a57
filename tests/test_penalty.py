"""Presence and frequency penalties inside the five q3_generate_many_* loops (include/qwen3_hip.h section 2p).  The yardstick is
tests/pen_ref.py: the rule in numpy float32 and, for the loops, a per-request loop over a single-stream engine -- forward() rows
copied, the penalty applied on the host, then the largest-key argmax or ops.sample / ops.sample_top_k with the request's rng.  With
both penalties 0 that reference has to give the tokens of the existing loops before it judges anything.  There is no tolerance
anywhere.  (The loops' per-slot rng states cannot be read through the ABI; every sampled token depends on every coin in front of
it, and the tokens are compared.)"""
import numpy as np
import pytest

import genlp_ref as gr
import logit_ckpt as lc
import pen_ref as pr
from test_genlp import CTX, LENS, N_NEW, NAME, PREFIX_LEN, SAMPLER, SLOTS, engine, run_loop, slot_rows

pytestmark = pytest.mark.gpu

f32 = np.float32
SLICES = 64
SETTINGS = [(1.5, 0.0), (0.5, 0.5)]


# ---------------------------------------------------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------------------------------------------------
def slice_bounds(n):
    """the slices of k_pen_apply: 64 of them, in units of four entries where n % 4 == 0"""
    unit = 4 if n % 4 == 0 else 1
    units = n // unit
    per = -(-units // SLICES)
    return [(min(s * per, units) * unit, min((s + 1) * per, units) * unit) for s in range(SLICES)]


def special_logits(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    l = (rng.standard_normal(n) * 4).astype(f32)
    tiny = np.finfo(f32).tiny
    special = [0.0, -0.0, np.inf, -np.inf, tiny / 8, -tiny / 8, np.finfo(f32).max, -np.finfo(f32).max, tiny]
    at = rng.permutation(n)[:len(special)]
    for i, v in zip(at, special):
        l[i] = v
    return l


def check_op(q3, l, c, p, f, what):
    got, idx = q3.ops.penalize(l, c, p, f)
    want = pr.penalize(l, c, p, f)
    assert got.tobytes() == want.tobytes(), f"{what}: {np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))} entries differ"
    assert idx == pr.argmax_key(want), what
    return got, idx


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 257, 2000, 151936, 151937])
def test_op_against_the_rule(q3, n):
    l = special_logits(n, 100 + n % 97)
    rng = np.random.Generator(np.random.PCG64(n))
    zero = np.zeros(n, dtype=np.uint32)
    every = rng.integers(1, 5, n).astype(np.uint32)
    first, last = zero.copy(), zero.copy()
    for a, b in slice_bounds(n):
        if b > a:
            first[a], last[b - 1] = 1, 3
    values = zero.copy()
    values[rng.permutation(n)[:min(n, 4)]] = np.array([1, 2, 65536, 2 ** 24 - 1], dtype=np.uint32)[:min(n, 4)]
    got, _ = check_op(q3, l, zero, 1.5, 0.5, f"n {n}, no counts")
    assert got.tobytes() == l.tobytes()
    for p, f in ((1.5, 0.5), (-2.0, 2.0), (0.0, 0.0), (0.3, 0.0)):
        for name, c in (("every entry", every), ("first of every slice", first), ("last of every slice", last), ("1, 2, 65536, 2^24 - 1", values)):
            check_op(q3, l, c, p, f, f"n {n}, ({p}, {f}), {name}")


@pytest.mark.parametrize("n", [65, 2000, 151936])
def test_op_designed_rows(q3, n):
    zero = np.zeros(n, dtype=np.uint32)
    # an all-equal row: the last index; with the last entries produced, the last that was not
    flat = np.full(n, 2.5, dtype=f32)
    assert check_op(q3, flat, zero, 1.0, 0.0, "all equal")[1] == n - 1
    c = zero.copy()
    c[n - 3:] = 1
    assert check_op(q3, flat, c, 1.0, 0.0, "all equal, the last three produced")[1] == n - 4
    # the only maximum penalised below the runner-up
    l = np.linspace(-3.0, 1.0, n).astype(f32)
    l[n // 3], l[n // 2] = 7.0, 6.0
    c = zero.copy()
    c[n // 3] = 2
    assert check_op(q3, l, zero, 0.25, 0.5, "raw")[1] == n // 3
    assert check_op(q3, l, c, 0.25, 0.5, "the maximum penalised by 1.25")[1] == n // 2
    # an exact tie between a penalised lower index and an unpenalised higher one: the higher index
    lo, hi = n // 5, n - 2
    l = np.full(n, -1.0, dtype=f32)
    l[lo], l[hi] = 5.0, 3.75
    d = f32(l[lo] - l[hi])
    assert f32(l[lo] - d) == l[hi] and -2.0 <= d <= 2.0
    c = zero.copy()
    c[lo] = 1
    got, idx = check_op(q3, l, c, float(d), 0.0, "exact tie")
    assert got[lo] == got[hi] and idx == hi
    # ... and the other way round: a penalised higher index ties with an unpenalised lower one and still wins
    l[lo], l[hi] = 3.75, 5.0
    c = zero.copy()
    c[hi] = 1
    assert check_op(q3, l, c, float(d), 0.0, "exact tie, higher index penalised")[1] == hi


def test_op_is_not_fused(q3):
    fr, c, p = pr.fma_triple()
    l = np.zeros(8, dtype=f32)
    counts = np.full(8, c, dtype=np.uint32)
    got, _ = check_op(q3, l, counts, p, fr, "the triple that tells a fused multiply-add apart")
    assert got.tobytes() != pr.penalize_fma(l, counts, p, fr).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the loops
# ---------------------------------------------------------------------------------------------------------------------
LOOPS = ["cols", "dense", "stop", "prefix"]


def loop_name(loop, sampled):
    return {"cols": "sampled" if sampled else "greedy"}.get(loop, loop)


def check_settings(t, ref, loop, prompts, n_new, sampler, settings, what, prefix=(), stop_at=(), must_bite=True):
    """The loop at (0, 0) against the reference first, then at every setting.  stop_at: (request, index) pairs -- the stop tokens are
    those entries of the reference's free-running rows under the setting in force.  Returns the rows per setting."""
    out = {}
    free0 = None
    for p, f in [(0.0, 0.0)] + list(settings):
        free, top, differs = ref.rows(prompts, n_new, p, f, sampler, prefix)
        stop = [free[r][i] for r, i in stop_at]
        want, top, _ = ref.rows(prompts, n_new, p, f, sampler, prefix, stop) if stop else (free, top, differs)
        t.set_penalties(p, f)
        assert t.get_penalties() == (float(f32(p)), float(f32(f)))
        rows, n_out = run_loop(t, loop, prompts, n_new, sampler, stop)
        assert rows == want, f"{what}: ({p}, {f}): other tokens than the reference" + (" -- THE REFERENCE FAILS THE EXISTING LOOP" if (p, f) == (0.0, 0.0) else "")
        if (p, f) == (0.0, 0.0):
            free0 = free
            assert not differs
        elif must_bite:
            # the setting decides something: rows penalised, a token produced twice, other tokens than without it
            assert differs and top >= 2 and free != free0, f"{what}: ({p}, {f}) proves nothing here"
        out[(p, f)] = rows
    t.set_penalties(0.0, 0.0)
    return out


@pytest.fixture(scope="module")
def designed(q3, tmp_path_factory):
    """the designed checkpoints (logits depend on the input token alone) and one single-stream reference engine each"""
    d = tmp_path_factory.mktemp("penalty")
    made = {}

    def get(file):
        if file not in made:
            path = lc.write(str(d / f"{file}.bin"), file)
            made[file] = (path, pr.Engine(q3, path))
        return made[file]
    yield get
    for _, ref in made.values():
        ref.close()


D_PROMPTS = [[0], [1, 2], [3, 0, 1], [2], [7, 5]]
D_NEW = [14, 12, 10, 14, 8]
D_SAMPLER = ([0.7, 1.0, 0.0, 0.7, 1.0], 0.9, [900 + r for r in range(5)])       # request 2 at temperature 0
D_PREFIX = [5, 6, 7]


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("file", ["small_a", "small_b"])
def test_designed_checkpoints(q3, designed, file, loop, sampled):
    """V = 2,000, 5 requests on 3 slots.  Unpenalised greedy output cycles within 4 tokens, so repeats are certain"""
    path, ref = designed(file)
    sampler = D_SAMPLER if sampled else None
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(3)
        prefix = ()
        if loop == "prefix":
            prefix = D_PREFIX
            t.batch_prefix_set(prefix)
        if loop == "dense":
            rows = {}
            for p, f in [(0.0, 0.0)] + SETTINGS:
                want, top, differs = ref.rows(D_PROMPTS, D_NEW, p, f, sampler)
                t.set_penalties(p, f)
                got = [list(r) for r in t.generate_many_dense(D_PROMPTS, D_NEW, sampler, dense_min=2)[0]]
                assert got == want, (file, p, f)
                assert (p, f) == (0.0, 0.0) or (differs and top >= 2 and want != rows[(0.0, 0.0)])
                rows[(p, f)] = got
            return
        # (the stop token is request 3's eleventh token under the setting in force: chosen on the CPU oracle so that in every case
        # a request ends early and a token is still produced twice in front of the stop)
        stop_at = [(3, 10)] if loop == "stop" else ()
        check_settings(t, ref, loop_name(loop, sampled), D_PROMPTS, D_NEW, sampler, SETTINGS, f"{file} {loop}", prefix, stop_at)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_designed_checkpoint_at_the_full_vocabulary(q3, designed, sampled):
    """V = 151,936 (big_a: peaked, uniform, second_try, head_flat): request 0 greedy or at temperature 0, request 1 drawn"""
    path, ref = designed("big_a")
    prompts, n_new = [[0], [2, 1]], [9, 8]
    sampler = ([0.0, 0.7], 0.9, [900, 901]) if sampled else None
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(2)
        check_settings(t, ref, "sampled" if sampled else "greedy", prompts, n_new, sampler, [(0.5, 0.5)], "big_a")


@pytest.fixture(scope="module")
def model(q3, tmp_path_factory):
    """tests/test_genlp.py's shape: 11 prompts of the small synthetic checkpoint, a 6-token prefix, one reference engine"""
    path = str(tmp_path_factory.mktemp("penalty_small") / f"{NAME}.bin")
    shape = q3.checkpoint.SHAPES[NAME]
    q3.checkpoint.write_synthetic_checkpoint(path, shape, seed=2468)
    prompts = [[int(x) for x in np.random.default_rng(6100 + r).integers(0, shape.vocab_size, n)] for r, n in enumerate(LENS)]
    prefix = [int(x) for x in np.random.default_rng(6200).integers(0, shape.vocab_size, PREFIX_LEN)]
    ref = pr.Engine(q3, path, ctx=CTX)
    yield path, prompts, prefix, ref
    ref.close()


# a negative setting raises what was produced: on Gaussian logits that is what changes tokens within six of them
SMALL_SETTINGS = [(1.5, 0.5), (-2.0, -1.0)]


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("loop", LOOPS)
def test_small_synthetic_shape(q3, model, loop, sampled):
    """11 requests on 8 slots: slots are reused, passes with no emitting column, every plan width"""
    path, prompts, prefix, ref = model
    sampler = SAMPLER if sampled else None
    with engine(q3, path) as t:
        if loop == "prefix":
            t.batch_prefix_set(prefix)
        stop_at = [(3, 0), (5, 2)] if loop == "stop" else ()
        check_settings(t, ref, loop_name(loop, sampled), prompts, N_NEW, sampler, SMALL_SETTINGS, loop, prefix if loop == "prefix" else (), stop_at,
                       must_bite=False)


def test_a_reused_slot_starts_empty(q3, designed):
    """identical greedy prompts with different n_new on 2 slots: every row is a prefix of the longest, which a histogram left
    over from the slot's previous request would break"""
    path, ref = designed("small_a")
    n_new = [14, 3, 9, 5, 12, 7, 14, 1]
    prompts = [[0]] * len(n_new)
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(2)
        t.set_penalties(1.5, 0.0)
        longest = ref.rows([[0]], [14], 1.5, 0.0)[0][0]
        assert longest != ref.rows([[0]], [14], 0.0, 0.0)[0][0] and max(np.bincount(longest)) >= 2
        rows = run_loop(t, "greedy", prompts, n_new, None)[0]
        assert rows == [longest[:n] for n in n_new]
        stop = [longest[6]]
        cut = longest.index(stop[0]) + 1
        rows = run_loop(t, "stop", prompts, n_new, None, stop)[0]
        assert rows == [longest[:min(n, cut)] for n in n_new]
        # and after a call that left other counts behind in both slots
        run_loop(t, "greedy", [[1, 2], [3]], [12, 12], None)
        assert run_loop(t, "greedy", prompts, n_new, None)[0] == [longest[:n] for n in n_new]


def test_with_top_k(q3, model):
    path, prompts, prefix, ref = model
    ref.top_k = 5
    try:
        with engine(q3, path) as t:
            t.set_top_k(5)
            check_settings(t, ref, "sampled", prompts, N_NEW, SAMPLER, SMALL_SETTINGS, "top_k 5", must_bite=False)
    finally:
        ref.top_k = 0


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_with_records(q3, model, sampled):
    """set_gen_logprobs(5) under penalties: the tokens and cache rows of the call without records, the records of the RAW rows
    (q3_score_many on prompt + output), zero bytes behind n_out"""
    path, prompts, prefix, ref = model
    sampler = SAMPLER if sampled else None
    p, f = SMALL_SETTINGS[1]
    with engine(q3, path) as t:
        t.set_penalties(p, f)
        free = run_loop(t, "sampled" if sampled else "greedy", prompts, N_NEW, sampler)[0]
        assert free == ref.rows(prompts, N_NEW, p, f, sampler)[0]
        for loop, stop in ((("sampled" if sampled else "greedy"), ()), ("stop", [free[3][0], free[5][2]])):
            t.set_gen_logprobs(-1)
            rows, n_out = run_loop(t, loop, prompts, N_NEW, sampler, stop)
            caches = slot_rows(t, SLOTS)
            got = {}
            for k in (0, 5):
                t.set_gen_logprobs(k)
                assert run_loop(t, loop, prompts, N_NEW, sampler, stop) == (rows, n_out), (loop, k)
                assert slot_rows(t, SLOTS) == caches, (loop, k)
                got[k] = (t.read_gen_logprobs(), t.read_gen_logprobs(N_NEW))
                assert t.get_penalties() == (p, f)
            # (behind the comparisons of the cache rows: the score calls overwrite the slots)
            for k, (cut, full) in got.items():
                gr.assert_same(cut, gr.expected(t, prompts, rows, k), rows, k, f"{loop}, top_n {k}, under penalties")
                gr.assert_zero_behind(full, n_out, f"{loop}, top_n {k}")
            if stop:
                assert any(n < m for n, m in zip(n_out, N_NEW))


def test_off_is_off(q3, model):
    """after a call under (1.5, 0.5) and set_penalties(0, 0): tokens and cache rows of every loop are those of a fresh engine;
    score_many, embed_many and batch_step_cols in between give what they give without the setting; changing the values between
    calls rebuilds nothing that a result depends on"""
    path, prompts, prefix, ref = model
    some, n_new = prompts[:6], N_NEW[:6]
    sampler = (SAMPLER[0][:6], SAMPLER[1], SAMPLER[2][:6])
    calls = [("greedy", None, ()), ("sampled", sampler, ()), ("dense", sampler, ()), ("stop", sampler, [0]), ("prefix", sampler, ())]

    def everything(t):
        got = []
        for loop, smp, stop in calls:
            got.append((run_loop(t, loop, some, n_new, smp, stop), slot_rows(t, 4)))
        return got
    with engine(q3, path, slots=4) as t:
        t.batch_prefix_set(prefix)
        fresh = everything(t)
        scores = [r.tobytes() for r in t.score_many(some)[0]]
        emb = t.embed_many(some)[0].tobytes()
        step = t.batch_step_cols([0, 1], [3, 4], [0, 0])
    with engine(q3, path, slots=4) as t:
        t.batch_prefix_set(prefix)
        t.set_penalties(1.5, 0.5)
        under = everything(t)
        assert [r.tobytes() for r in t.score_many(some)[0]] == scores
        assert t.embed_many(some)[0].tobytes() == emb
        assert t.batch_step_cols([0, 1], [3, 4], [0, 0]) == step
        # other values, the same plans: the reference at both
        t.batch_prefix_set(prefix)
        for p, f in ((-2.0, -1.0), (1.5, 0.5), (-2.0, -1.0)):
            t.set_penalties(p, f)
            assert run_loop(t, "sampled", some, n_new, sampler)[0] == ref.rows(some, n_new, p, f, sampler)[0], (p, f)
        assert run_loop(t, "greedy", some, n_new, None)[0] != fresh[0][0][0]
        # (the calls in between left rows of their own in the slots: the caches start as a fresh engine's do)
        for (p, f), want in (((0.0, 0.0), fresh), ((1.5, 0.5), under)):
            t.set_penalties(p, f)
            t.batch_reset_kv()
            t.batch_prefix_set(prefix)
            got = everything(t)
            assert [g[0] for g in got] == [w[0] for w in want], f"({p}, {f}): other tokens than on a fresh engine"
            assert [g[1] for g in got] == [w[1] for w in want], f"({p}, {f}): other cache rows than on a fresh engine"


def test_the_setting_survives(q3, model):
    path, prompts, prefix, ref = model
    few, n_new = prompts[:3], [4, 5, 3]
    with q3.TransformerBuilder(path).with_ctx_length(CTX).build() as t:
        assert t.get_penalties() == (0.0, 0.0)
        t.set_penalties(-2.0, -1.0)                                  # no batched state yet: the first generate call allocates
        t.batch_init(4, CTX)
        want = ref.rows(few, n_new, -2.0, -1.0)[0]
        assert t.generate_many_greedy(few, n_new)[0] == want
        t.set_sampler(0.7, 0.9, 3)
        t.set_sampler(0.0, 0.9, 3)
        t.set_top_k(7)
        t.set_gen_logprobs(3)
        t.batch_init(4, CTX)
        assert t.get_penalties() == (-2.0, -1.0)
        assert t.generate_many_greedy(few, n_new)[0] == want
        for bad in (2.5, float("nan")):
            assert t._lib.q3_sampler_penalties(t._h, bad, 0.0) == -3 and t.get_penalties() == (-2.0, -1.0)
        assert t.generate_many_greedy(few, n_new)[0] == want


def test_generate_many_arguments(q3, model):
    path, prompts, prefix, ref = model
    some = prompts[:6]
    with engine(q3, path, slots=4) as t:
        t.set_penalties(0.25, 0.0)
        plain = q3.generate_many(t, some, 5)[0]
        assert plain == ref.rows(some, [5] * 6, 0.0, 0.0)[0] and t.get_penalties() == (0.25, 0.0)
        for kw in ({}, dict(sampler=(0.8, 0.9, list(range(11, 17)))), dict(shared_prefix=prefix)):
            rows = q3.generate_many(t, some, 5, presence_penalty=-2.0, frequency_penalty=-1.0, **kw)[0]
            want = ref.rows(some, [5] * 6, -2.0, -1.0, kw.get("sampler"), kw.get("shared_prefix", ()))[0]
            assert rows == want and t.get_penalties() == (0.25, 0.0), kw
        with pytest.raises(IndexError):
            q3.generate_many(t, [[10 ** 9]], 5, presence_penalty=1.0)
        assert t.get_penalties() == (0.25, 0.0)
        with pytest.raises(ValueError):
            q3.generate_many(t, some, 5, presence_penalty=3.0)
        assert t.get_penalties() == (0.25, 0.0)
