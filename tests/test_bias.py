"""Logit bias, banned and allowed tokens, min_tokens inside the five q3_generate_many_* loops (include/qwen3_hip.h section 2q).  The
yardstick is tests/bias_ref.py: the rule in numpy float32 and, for the loops, pen_ref's per-request loop over a single-stream engine
with every forward() row adjusted on the host first -- bias, then penalties, then the largest-key argmax or ops.sample /
ops.sample_top_k with the request's rng.  With no table that reference has to give the tokens of the existing loops before it judges
anything, and every table has to decide something on the reference before the engine is held to it.  There is no tolerance anywhere:
rows are compared as bytes, tokens as integers."""
import numpy as np
import pytest

import bias_ref as br
import logit_ckpt as lc
import pen_ref as pr
from test_genlp import CTX, LENS, N_NEW, NAME, PREFIX_LEN, SAMPLER, SLOTS, engine, slot_rows
from test_penalty import D_NEW, D_PREFIX, D_PROMPTS, D_SAMPLER, slice_bounds, special_logits

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = float("inf")
OFF = ([], [])
PEN = (1.5, 0.5)


# ---------------------------------------------------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------------------------------------------------
UNTIL = 5
BIASES = [1.0, -1.0, 0.0, -0.0, 100.0, -100.0, -INF, 0.37, -7.25, 1e-30, 2.0 ** -20]


def entries_at(rng, l, tokens):
    """one entry per token: biases of every kind, until 0 or UNTIL.  The first bias is finite (an ALLOW list needs one, an ADD list
    must not ban everything), and +inf gets no -inf: their sum is a NaN, which the standard leaves open"""
    out = []
    for i, t in enumerate(tokens):
        b = BIASES[int(rng.integers(len(BIASES)))]
        if b == -INF and (i == 0 or l[t] == np.inf):
            b = 2.5
        out.append((int(t), b, UNTIL if rng.integers(2) else 0))
    return out


def check_op(q3, l, entries, mode, g, counts, what):
    p, f = PEN if counts is not None else (0.0, 0.0)
    got, idx = q3.ops.logit_bias(l, entries, mode, g, counts, p, f)
    want = br.rule(l, entries, mode, g, counts, p, f)
    assert got.tobytes() == want.tobytes(), f"{what}: {np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))} entries differ"
    assert idx == pr.argmax_key(want), what
    return got, idx


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 257, 2000, 151936, 151937])
def test_op_against_the_rule(q3, n):
    l = special_logits(n, 200 + n % 97)
    rng = np.random.Generator(np.random.PCG64(n))
    ends = sorted({a for a, b in slice_bounds(n) if b > a} | {b - 1 for a, b in slice_bounds(n) if b > a})
    lists = {"no entries": [], "the first and the last entry of every slice": entries_at(rng, l, ends),
             "random entries": entries_at(rng, l, rng.permutation(n)[:min(n, 4096)]), "one entry at n - 1": entries_at(rng, l, [n - 1])}
    if n <= 4096:
        lists["every token"] = entries_at(rng, l, range(n))
    counts = rng.integers(0, 4, n).astype(np.uint32)
    for name, entries in lists.items():
        for mode in (br.ADD, br.ALLOW):
            if mode == br.ALLOW and not entries:
                continue                                    # refused: an ALLOW list with no finite bias allows no token
            for g in (UNTIL - 1, UNTIL, UNTIL + 1):
                for c in (None, counts):
                    got, _ = check_op(q3, l, entries, mode, g, c, f"n {n}, {name}, mode {mode}, g {g}, counts {c is not None}")
                    if not entries and c is None:
                        assert got.tobytes() == l.tobytes()


@pytest.mark.parametrize("n", [65, 2000, 151936])
def test_op_designed_rows(q3, n):
    # an all-equal row: the last index; with the last three tokens banned, the last that is not
    flat = np.full(n, 2.5, dtype=f32)
    assert check_op(q3, flat, [], br.ADD, 0, None, "all equal")[1] == n - 1
    ban = [(n - 1, -INF, 0), (n - 3, -INF, 0), (n - 2, -INF, 0)]
    got, idx = check_op(q3, flat, ban, br.ADD, 0, None, "all equal, the last three banned")
    assert idx == n - 4 and (got[n - 3:].view(np.uint32) == 0xFF800000).all()
    # an ALLOW list of two tokens on a row whose maximum is unlisted
    l = np.linspace(-3.0, 1.0, n).astype(f32)
    l[n // 3], l[n // 2], l[n // 7] = 7.0, 6.0, -2.0
    got, idx = check_op(q3, l, [(n // 2, 0.0, 0), (n // 7, 0.0, 0)], br.ALLOW, 0, None, "two allowed")
    assert idx == n // 2 and np.count_nonzero(got.view(np.uint32) != 0xFF800000) == 2
    assert check_op(q3, l, [(n // 2, -5.0, 0), (n // 7, 3.5, 0)], br.ALLOW, 0, None, "two allowed, the lower raised above")[1] == n // 7
    # a bias that produces an exact tie between a lower and a higher index: the higher one, whichever of the two was moved
    lo, hi = n // 5, n - 2
    l = np.full(n, -1.0, dtype=f32)
    l[lo], l[hi] = 5.0, 3.75
    got, idx = check_op(q3, l, [(lo, -1.25, 0)], br.ADD, 0, None, "exact tie, the lower index lowered")
    assert got[lo] == got[hi] and idx == hi
    got, idx = check_op(q3, l, [(hi, 1.25, 0)], br.ADD, 0, None, "exact tie, the higher index raised")
    assert got[lo] == got[hi] and idx == hi
    # the tie stands while the entry is active and goes with it
    assert check_op(q3, l, [(hi, 1.25, 3)], br.ADD, 2, None, "g below until")[1] == hi
    assert check_op(q3, l, [(hi, 1.25, 3)], br.ADD, 3, None, "g at until")[1] == lo
    # a bias of 0 on the row's only -0.0 among +0.0s keeps the order: -0.0 + 0.0 would be a +0.0 at the highest index
    z = np.zeros(n, dtype=f32)
    z[n - 1] = -0.0
    for bias in (0.0, -0.0):
        got, idx = check_op(q3, z, [(n - 1, bias, 0)], br.ADD, 0, None, "the only -0.0")
        assert idx == n - 2 and got.view(np.uint32)[n - 1] == 0x80000000
    # the penalties on top of the bias: +0.5 and then presence 1.5 off a produced token
    l = np.zeros(n, dtype=f32)
    l[lo], l[hi] = 2.0, 1.0
    c = np.zeros(n, dtype=np.uint32)
    c[lo] = 1
    got, idx = check_op(q3, l, [(lo, 0.5, 0)], br.ADD, 0, c, "bias, then penalties")
    assert got[lo] == f32(2.5) - f32(PEN[0] + PEN[1]) and idx == hi


def test_op_applies_the_bias_before_the_penalties(q3):
    l, b, p = br.order_triple()
    row = np.full(8, l, dtype=f32)
    c = np.ones(8, dtype=np.uint32)
    entries = [(t, b, 0) for t in range(8)]
    got, _ = q3.ops.logit_bias(row, entries, br.ADD, 0, c, p, 0.0)
    assert got.tobytes() == br.rule(row, entries, br.ADD, 0, c, p, 0.0).tobytes()
    assert got.tobytes() != br.adjust(pr.penalize(row, c, p, 0.0), entries, br.ADD, 0).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the loops
# ---------------------------------------------------------------------------------------------------------------------
LOOPS = ["cols", "dense", "stop", "prefix"]


def loop_name(loop, sampled):
    return {"cols": "sampled" if sampled else "greedy"}.get(loop, loop)


def run_loop(t, loop, prompts, n_new, sampler, stop=(), dense_min=8):
    if loop == "greedy":
        rows = t.generate_many_greedy(prompts, n_new)[0]
    elif loop == "sampled":
        rows = t.generate_many_sampled(prompts, n_new, *sampler)[0]
    elif loop == "dense":
        rows = t.generate_many_dense(prompts, n_new, sampler, dense_min=dense_min)[0]
    elif loop == "stop":
        rows = t.generate_many_stop(prompts, n_new, stop, sampler)[0]
    else:
        rows = t.generate_many_prefix(prompts, n_new, stop, sampler)[0]
    return [list(r) for r in rows]


def check_tables(t, ref, loop, prompts, n_new, sampler, tables, what, prefix=(), stop_at=(), pen=(0.0, 0.0), dense_min=8):
    """The loop with no table against the reference first, then under every table of `tables` (name -> (lists, modes)).  stop_at:
    (request, index) pairs -- the stop tokens are those entries of the reference's free-running rows under the table in force."""
    t.set_penalties(*pen)
    out = {}
    for name, table in [("no table", OFF)] + list(tables.items()):
        free = br.rows(ref, prompts, n_new, table, *pen, sampler, prefix)
        stop = sorted({free[r][i] for r, i in stop_at})
        want = br.rows(ref, prompts, n_new, table, *pen, sampler, prefix, stop) if stop else free
        t.set_logit_bias(*table)
        assert t.get_logit_bias() == ([sorted(tuple(e) for e in l) for l in table[0]], list(table[1]))
        rows = run_loop(t, loop, prompts, n_new, sampler, stop, dense_min)
        assert rows == want, f"{what}: {name}: other tokens than the reference" + (" -- THE REFERENCE FAILS THE EXISTING LOOP" if table is OFF else "")
        if stop:
            assert any(len(r) < n for r, n in zip(rows, n_new)), f"{what}: {name}: no request ends early"
        out[name] = rows
    t.set_logit_bias([])
    t.set_penalties(0.0, 0.0)
    return out


def bite_tables(ref, prompts, n_new, sampler, prefix, V, seed, pen=(0.0, 0.0), n_add=40):
    """The tables of a case, made from the reference's unconstrained rows and held to DECIDE something on the reference: the banned
    token occurs in an unconstrained row; every token of an ALLOW request is in its list and its unconstrained row leaves the list;
    the ADD lists change every request."""
    rng = np.random.Generator(np.random.PCG64(seed))
    free = br.rows(ref, prompts, n_new, OFF, *pen, sampler, prefix)
    n = len(prompts)
    tables = {}
    # one ban for all requests: the token the unconstrained rows hold most often
    toks, cnt = np.unique([x for row in free for x in row], return_counts=True)
    banned = int(toks[np.argmax(cnt)])
    tables["one ban for all"] = ([[(banned, -INF, 0)]], [br.ADD])
    got = br.rows(ref, prompts, n_new, tables["one ban for all"], *pen, sampler, prefix)
    assert any(banned in row for row in free) and got != free
    # a list per request: its own first token banned (the rule holds for y_0), biases of both signs on others
    add = []
    for r in range(n):
        others = [int(x) for x in rng.permutation(V) if x != free[r][0]][:n_add - 1]
        add.append([(free[r][0], -INF, 0)] + [(x, float(f32(rng.uniform(-6, 6))), 0) for x in others])
    tables["a list per request"] = (add, [br.ADD] * n)
    got = br.rows(ref, prompts, n_new, tables["a list per request"], *pen, sampler, prefix)
    assert all(g[0] != f[0] for g, f in zip(got, free))
    # ALLOW lists of 2 to 5 tokens
    allow = [[(int(x), 0.0, 0) for x in rng.permutation(V)[:2 + r % 4]] for r in range(n)]
    tables["an allow-list per request"] = (allow, [br.ALLOW] * n)
    got = br.rows(ref, prompts, n_new, tables["an allow-list per request"], *pen, sampler, prefix)
    for r in range(n):
        listed = {e[0] for e in allow[r]}
        assert set(got[r]) <= listed and not set(free[r]) <= listed, r
    return tables


@pytest.fixture(scope="module")
def designed(q3, tmp_path_factory):
    """the designed checkpoints (logits depend on the input token alone) and one single-stream reference engine each"""
    d = tmp_path_factory.mktemp("bias")
    made = {}

    def get(file):
        if file not in made:
            path = lc.write(str(d / f"{file}.bin"), file)
            made[file] = (path, pr.Engine(q3, path))
        return made[file]
    yield get
    for _, ref in made.values():
        ref.close()


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("file", ["small_a", "small_b"])
def test_designed_checkpoints(q3, designed, file, loop, sampled):
    """V = 2,000, 5 requests on 3 slots, request 2 at temperature 0 under the sampler"""
    path, ref = designed(file)
    sampler = D_SAMPLER if sampled else None
    prefix = D_PREFIX if loop == "prefix" else ()
    tables = bite_tables(ref, D_PROMPTS, D_NEW, sampler, prefix, lc.V_SMALL, 11)
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(3)
        if prefix:
            t.batch_prefix_set(prefix)
        # (the stop token is request 3's eleventh token under the table in force: a request ends early under every table)
        stop_at = [(3, 10)] if loop == "stop" else ()
        check_tables(t, ref, loop_name(loop, sampled), D_PROMPTS, D_NEW, sampler, tables, f"{file} {loop}", prefix, stop_at, dense_min=2)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("loop", ["stop", "prefix"])
def test_min_tokens_on_the_stop_loop(q3, designed, loop, sampled):
    """{stop, -inf, until = min_tokens}: the stop token stands in a free-running row in front of index min_tokens and ends it there;
    under the entry the request ends later, or runs to n_new"""
    path, ref = designed("small_a")
    sampler = D_SAMPLER if sampled else None
    prefix = D_PREFIX if loop == "prefix" else ()
    free = br.rows(ref, D_PROMPTS, D_NEW, OFF, 0.0, 0.0, sampler, prefix)
    m = 6
    stop = [free[3][1], free[0][2]]
    cut = br.rows(ref, D_PROMPTS, D_NEW, OFF, 0.0, 0.0, sampler, prefix, stop)
    early = [r for r, row in enumerate(cut) if len(row) < m and row[-1] in stop]
    assert {0, 3} <= set(early)
    one = ([[(s, -INF, m) for s in sorted(set(stop))]], [br.ADD])
    # ... and per request: request r must not stop in front of m + r tokens
    per = ([[(s, -INF, m + r) for s in sorted(set(stop))] for r in range(5)], [br.ADD] * 5)
    for table in (one, per):
        want = br.rows(ref, D_PROMPTS, D_NEW, table, 0.0, 0.0, sampler, prefix, stop)
        for r in early:
            least = m if table is one else m + r
            assert len(want[r]) > len(cut[r]) and len(want[r]) >= min(least + 1, D_NEW[r]) and not set(want[r][:least]) & set(stop), r
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(3)
        if prefix:
            t.batch_prefix_set(prefix)
        for name, table in (("no table", OFF), ("min_tokens 6 for all", one), ("min_tokens 6 + r", per), ("no table again", OFF)):
            t.set_logit_bias(*table)
            want = br.rows(ref, D_PROMPTS, D_NEW, table, 0.0, 0.0, sampler, prefix, stop)
            assert run_loop(t, loop, D_PROMPTS, D_NEW, sampler, stop) == want, name
        # the same through generate_many's min_tokens, the table put back
        t.set_logit_bias([[(1, 0.5, 0)]])
        kw = dict(shared_prefix=prefix) if prefix else {}
        rows = q3.generate_many(t, D_PROMPTS, max(D_NEW), stop_tokens=stop, sampler=sampler, stop_on_device=True, min_tokens=m, **kw)[0]
        assert rows == br.rows(ref, D_PROMPTS, [max(D_NEW)] * 5, one, 0.0, 0.0, sampler, prefix, stop)
        assert t.get_logit_bias() == ([[(1, 0.5, 0)]], [0])


@pytest.mark.parametrize("loop", ["greedy", "sampled", "dense", "stop", "prefix"])
def test_a_mixed_table_with_penalties_and_top_k(q3, designed, loop):
    """penalties (1.5, 0.5) on top of the adjusted rows, top_k 20 in front of every draw; ADD and ALLOW lists and until entries in
    one table"""
    path, ref = designed("small_b")
    sampler = None if loop == "greedy" else D_SAMPLER
    prefix = D_PREFIX if loop == "prefix" else ()
    ref.top_k = 20
    try:
        rng = np.random.Generator(np.random.PCG64(77))
        free = br.rows(ref, D_PROMPTS, D_NEW, OFF, *PEN, sampler, prefix)
        lists, modes = [], []
        for r in range(5):
            if r % 2:
                lists.append([(int(x), float(f32(rng.uniform(-2, 2))), 0) for x in rng.permutation(lc.V_SMALL)[:6]])
                modes.append(br.ALLOW)
            else:
                others = [int(x) for x in rng.permutation(lc.V_SMALL) if x != free[r][0]][:30]
                lists.append([(free[r][0], -INF, 3)] + [(x, float(f32(rng.uniform(-6, 6))), int(rng.integers(0, 6))) for x in others])
                modes.append(br.ADD)
        mixed = (lists, modes)
        want = br.rows(ref, D_PROMPTS, D_NEW, mixed, *PEN, sampler, prefix)
        assert all(w != f for w, f in zip(want, free))
        # the penalties decide something on top of the table
        assert want != br.rows(ref, D_PROMPTS, D_NEW, mixed, 0.0, 0.0, sampler, prefix)
        with q3.TransformerBuilder(path).build() as t:
            t.batch_init(3)
            t.set_top_k(20)
            if prefix:
                t.batch_prefix_set(prefix)
            stop_at = [(3, 10)] if loop == "stop" else ()
            check_tables(t, ref, loop, D_PROMPTS, D_NEW, sampler, {"mixed": mixed}, f"{loop}, penalties, top_k 20", prefix, stop_at, PEN, dense_min=2)
            # the table alone, then the penalties alone: the adjusted form with and without counts, then the form under penalties
            check_tables(t, ref, loop, D_PROMPTS, D_NEW, sampler, {"mixed": mixed}, f"{loop}, top_k 20", prefix, stop_at, dense_min=2)
            t.set_penalties(*PEN)
            assert run_loop(t, loop, D_PROMPTS, D_NEW, sampler, [free[3][10]] if stop_at else (), 2) == \
                br.rows(ref, D_PROMPTS, D_NEW, OFF, *PEN, sampler, prefix, [free[3][10]] if stop_at else ())
    finally:
        ref.top_k = 0


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_designed_checkpoint_at_the_full_vocabulary(q3, designed, sampled):
    """V = 151,936 (big_a): request 0 greedy or at temperature 0, request 1 drawn; a 300-entry ADD list and a 12-token ALLOW list"""
    path, ref = designed("big_a")
    prompts, n_new = [[0], [2, 1]], [7, 6]
    sampler = ([0.0, 0.7], 0.9, [900, 901]) if sampled else None
    tables = bite_tables(ref, prompts, n_new, sampler, (), lc.V_BIG, 13, n_add=300)
    rng = np.random.Generator(np.random.PCG64(14))
    tables["an allow-list per request"] = ([[(int(x), 0.0, 0) for x in rng.permutation(lc.V_BIG)[:12]] for _ in prompts], [br.ALLOW] * 2)
    assert all(len(l) == 300 for l in tables["a list per request"][0])
    got = br.rows(ref, prompts, n_new, tables["an allow-list per request"], 0.0, 0.0, sampler)
    assert all(set(g) <= {e[0] for e in l} for g, l in zip(got, tables["an allow-list per request"][0]))
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(2)
        check_tables(t, ref, "sampled" if sampled else "greedy", prompts, n_new, sampler, tables, "big_a")


@pytest.fixture(scope="module")
def model(q3, tmp_path_factory):
    """tests/test_genlp.py's shape: 11 prompts of the small synthetic checkpoint, a 6-token prefix, one reference engine"""
    path = str(tmp_path_factory.mktemp("bias_small") / f"{NAME}.bin")
    shape = q3.checkpoint.SHAPES[NAME]
    q3.checkpoint.write_synthetic_checkpoint(path, shape, seed=2468)
    prompts = [[int(x) for x in np.random.default_rng(6100 + r).integers(0, shape.vocab_size, n)] for r, n in enumerate(LENS)]
    prefix = [int(x) for x in np.random.default_rng(6200).integers(0, shape.vocab_size, PREFIX_LEN)]
    ref = pr.Engine(q3, path, ctx=CTX)
    yield path, shape.vocab_size, prompts, prefix, ref
    ref.close()


def per_request_table(ref, prompts, n_new, sampler, prefix, V, seed):
    """a list for every request, no two alike: its own unconstrained first token banned, and every third request an allow-list"""
    rng = np.random.Generator(np.random.PCG64(seed))
    free = br.rows(ref, prompts, n_new, OFF, 0.0, 0.0, sampler, prefix)
    lists, modes = [], []
    for r in range(len(prompts)):
        if r % 3 == 2:
            lists.append([(int(x), 0.0, 0) for x in rng.permutation(V)[:3 + r % 4] if x != free[r][0]])
            modes.append(br.ALLOW)
        else:
            others = [int(x) for x in rng.permutation(V) if x != free[r][0]][:20]
            lists.append([(free[r][0], -INF, 0)] + [(x, float(f32(rng.uniform(-4, 4))), 0) for x in others])
            modes.append(br.ADD)
    got = br.rows(ref, prompts, n_new, (lists, modes), 0.0, 0.0, sampler, prefix)
    # every request is decided by ITS list: its first token is another one, and under another request's list it would differ again
    assert all(g[0] != f[0] for g, f in zip(got, free))
    shifted = (lists[1:] + lists[:1], modes[1:] + modes[:1])
    other = br.rows(ref, prompts, n_new, shifted, 0.0, 0.0, sampler, prefix)
    assert sum(g != o for g, o in zip(got, other)) >= len(prompts) - 2
    return (lists, modes)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("loop", LOOPS)
def test_a_reused_slot_takes_the_new_occupants_list(q3, model, loop, sampled):
    """11 requests on 8 slots: slots are reused by requests with other lists, passes with no emitting column, every plan width"""
    path, V, prompts, prefix, ref = model
    sampler = SAMPLER if sampled else None
    use = prefix if loop == "prefix" else ()
    table = per_request_table(ref, prompts, N_NEW, sampler, use, V, 21)
    with engine(q3, path) as t:
        if use:
            t.batch_prefix_set(use)
        stop_at = [(3, 0), (5, 2)] if loop == "stop" else ()
        check_tables(t, ref, loop_name(loop, sampled), prompts, N_NEW, sampler, {"a list per request": table}, loop, use, stop_at)


def test_the_setting_leaks_nowhere(q3, model):
    """under a table: batch_step_cols, batch_step_cols_draw, score, choose, embed and single-stream decode give the bytes they give
    with none; a generate call with another number of requests than lists is refused and leaves the caches alone; after
    set_logit_bias([]) tokens and cache rows of every loop are those of an engine that never saw a table"""
    path, V, prompts, prefix, ref = model
    some, n_new = prompts[:6], N_NEW[:6]
    sampler = (SAMPLER[0][:6], SAMPLER[1], SAMPLER[2][:6])
    calls = [("greedy", None, ()), ("sampled", sampler, ()), ("dense", sampler, ()), ("stop", sampler, [0]), ("prefix", sampler, ())]
    cands = [3, 17, 40]

    def loops(t):
        return [(run_loop(t, loop, some, n_new, smp, stop), slot_rows(t, 4)) for loop, smp, stop in calls]

    def others(t):
        got = [t.batch_step_cols([0, 1], [3, 4], [0, 0], want_logits=True)]
        t.set_batch_sampler(0.8, 0.9, [5, 6, 7, 8])
        got.append(t.batch_step_cols_draw([0, 1], [3, 4], [1, 1], want_logits=True))
        t.set_batch_sampler(0.0, 0.9, [5, 6, 7, 8])
        got.append([r.tobytes() for r in t.score_many(some)[0]])
        got.append(np.asarray(t.choice_many(some, cands)[0]).tobytes())
        got.append(t.embed_many(some)[0].tobytes())
        t.reset_kv()
        got.append((t.forward(3, 0).tobytes(), t.generate_greedy(5, 1, 6)))
        return [(g[0].tobytes(), g[1]) if isinstance(g, tuple) and isinstance(g[0], np.ndarray) else g for g in got]
    with engine(q3, path, slots=4) as t:
        t.batch_prefix_set(prefix)
        fresh = loops(t)
        plain = others(t)
    table = per_request_table(ref, some, n_new, sampler, (), V, 22)
    with engine(q3, path, slots=4) as t:
        t.batch_prefix_set(prefix)
        t.set_logit_bias(*table)
        under = loops(t)
        assert under[0][0] != fresh[0][0] and under[1][0] == br.rows(ref, some, n_new, table, 0.0, 0.0, sampler)
        assert others(t) == plain
        # 6 lists, 5 requests: refused before anything runs
        t.batch_reset_kv()
        t.batch_prefix_set(prefix)
        assert loops(t) == under
        caches = slot_rows(t, 4)
        for loop, smp, stop in calls:
            with pytest.raises(IndexError, match="6 lists"):
                run_loop(t, loop, some[:5], n_new[:5], None if smp is None else (smp[0][:5], smp[1], smp[2][:5]), stop)
        assert slot_rows(t, 4) == caches and t.get_logit_bias()[1] == table[1]
        # a token outside the vocabulary, an ADD list that bans all of it: refused with the model at hand, the table stays
        with pytest.raises(q3.Q3Error, match="index out of range"):
            t.set_logit_bias([[(V, 1.0, 0)]])
        if V <= 4096:
            with pytest.raises(q3.Q3Error, match="bans every token"):
                t.set_logit_bias([[(v, -INF, 0) for v in range(V)]])
        assert t.get_logit_bias()[1] == table[1]
        assert run_loop(t, "sampled", some, n_new, sampler) == under[1][0]
        # off: the caches start as a fresh engine's do
        t.set_logit_bias([])
        t.batch_reset_kv()
        t.batch_prefix_set(prefix)
        got = loops(t)
        assert [g[0] for g in got] == [w[0] for w in fresh], "other tokens than on an engine that never saw a table"
        assert [g[1] for g in got] == [w[1] for w in fresh], "other cache rows than on an engine that never saw a table"


def test_the_table_survives(q3, model):
    path, V, prompts, prefix, ref = model
    few, n_new = prompts[:3], [4, 5, 3]
    table = per_request_table(ref, few, n_new, None, (), V, 23)
    one = ([table[0][0]], [br.ADD])
    with q3.TransformerBuilder(path).with_ctx_length(CTX).build() as t:
        assert t.get_logit_bias() == OFF
        t.set_logit_bias(*table)                                     # no batched state yet: the first generate call makes the device side
        t.batch_init(4, CTX)
        want = br.rows(ref, few, n_new, table)
        assert run_loop(t, "greedy", few, n_new, None) == want
        t.set_sampler(0.7, 0.9, 3)
        t.set_sampler(0.0, 0.9, 3)
        t.set_top_k(7)
        t.set_gen_logprobs(3)
        t.set_penalties(1.0, 0.0)
        t.set_penalties(0.0, 0.0)
        t.batch_init(4, CTX)
        assert t.get_logit_bias()[1] == table[1]
        assert run_loop(t, "greedy", few, n_new, None) == want
        # a refused table changes nothing
        with pytest.raises(ValueError):
            t.set_logit_bias([[(3, 1.0, 0), (3, 2.0, 0)]])
        assert run_loop(t, "greedy", few, n_new, None) == want
        # two tables, the same plans: one list for every request, any number of requests; then the per-request one again
        t.set_logit_bias(*one)
        assert run_loop(t, "greedy", prompts[:5], N_NEW[:5], None) == br.rows(ref, prompts[:5], N_NEW[:5], one)
        t.set_logit_bias(*table)
        assert run_loop(t, "greedy", few, n_new, None) == want


def test_records_stay_on_the_raw_rows(q3, model):
    """set_gen_logprobs(5) under a table: the tokens of the call without records, and the records of score_top_many on prompt + row"""
    import genlp_ref as gr
    path, V, prompts, prefix, ref = model
    table = per_request_table(ref, prompts, N_NEW, SAMPLER, (), V, 24)
    with engine(q3, path) as t:
        t.set_logit_bias(*table)
        rows = run_loop(t, "sampled", prompts, N_NEW, SAMPLER)
        assert rows == br.rows(ref, prompts, N_NEW, table, 0.0, 0.0, SAMPLER)
        t.set_gen_logprobs(5)
        assert run_loop(t, "sampled", prompts, N_NEW, SAMPLER) == rows
        got = t.read_gen_logprobs()
        gr.assert_same(got, gr.expected(t, prompts, rows, 5), rows, 5, "under a table")


def test_generate_many_arguments(q3, model):
    path, V, prompts, prefix, ref = model
    some = prompts[:6]
    kept = ([[(1, 0.25, 0)]], [0])
    with engine(q3, path, slots=4) as t:
        t.set_logit_bias(*kept)
        # with none of the arguments the engine's table simply holds
        assert q3.generate_many(t, some, 5)[0] == br.rows(ref, some, [5] * 6, kept)
        free = br.rows(ref, some, [5] * 6)
        banned = [[row[0]] for row in free]
        for kw in ({}, dict(sampler=(0.8, 0.9, list(range(11, 17)))), dict(shared_prefix=prefix)):
            smp, pre = kw.get("sampler"), kw.get("shared_prefix", ())
            first = [[row[0]] for row in br.rows(ref, some, [5] * 6, OFF, 0.0, 0.0, smp, pre)]
            table = q3.merge_logit_bias(6, {7: 2.0}, first, None)
            rows = q3.generate_many(t, some, 5, logit_bias={7: 2.0}, banned_tokens=first, **kw)[0]
            assert rows == br.rows(ref, some, [5] * 6, table, 0.0, 0.0, smp, pre) and t.get_logit_bias() == kept, kw
            allowed = [9, 40, 77, 100]
            rows = q3.generate_many(t, some, 5, allowed_tokens=allowed, presence_penalty=1.5, **kw)[0]
            assert rows == br.rows(ref, some, [5] * 6, q3.merge_logit_bias(6, None, None, allowed), 1.5, 0.0, smp, pre), kw
            assert all(set(r) <= set(allowed) for r in rows) and t.get_logit_bias() == kept
        with pytest.raises(IndexError):
            q3.generate_many(t, [[10 ** 9]], 5, banned_tokens=[3])
        assert t.get_logit_bias() == kept
        with pytest.raises(ValueError):
            q3.generate_many(t, some, 5, logit_bias={3: 200.0})
        assert t.get_logit_bias() == kept and banned
