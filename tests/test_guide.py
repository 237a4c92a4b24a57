"""Guided decoding inside the five q3_generate_many_* loops (include/qwen3_hip.h section 2r).  The yardstick is tests/guide_ref.py:
the mask in numpy on the bits and, for the loops, pen_ref's per-request loop over a single-stream engine with every forward() row
masked in the state the request's own tokens lead to, then adjusted (bias_ref) and penalised, then the largest-key argmax or
ops.sample / ops.sample_top_k with the request's rng.  With no guide that reference has to give the tokens of the existing loops
before it judges anything, and every guide has to DECIDE on the reference -- the reference without the guide's row at that step
commits a token the row forbids, at g == 0 and behind two state changes -- before the engine is held to it.  There is no tolerance
anywhere: rows are compared as bytes, tokens as integers."""
import numpy as np
import pytest

import bias_ref as br
import guide_ref as gr
import logit_ckpt as lc
import pen_ref as pr
from test_bias import LOOPS, OFF, PEN, loop_name, run_loop
from test_genlp import CTX, LENS, N_NEW, NAME, PREFIX_LEN, SAMPLER, engine, slot_rows
from test_penalty import D_NEW, D_PREFIX, D_PROMPTS, D_SAMPLER, slice_bounds, special_logits

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = float("inf")
NO_GUIDE = (None, [])


# ---------------------------------------------------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------------------------------------------------
def state_rows(n, rng):
    """one state's row of a table, in the forms that matter to the kernel: the allowed entries carry state numbers of every size"""
    to = rng.integers(0, 4096, n).astype(np.int16)
    ends = sorted({a for a, b in slice_bounds(n) if b > a} | {b - 1 for a, b in slice_bounds(n) if b > a})
    rows = {"all allowed": to.copy(), "only token 0": np.full(n, -1, dtype=np.int16), "only n - 1": np.full(n, -1, dtype=np.int16),
            "the first and the last entry of every slice": np.full(n, -1, dtype=np.int16), "a random half": np.where(rng.random(n) < 0.5, to, -1).astype(np.int16)}
    rows["only token 0"][0] = 0
    rows["only n - 1"][n - 1] = 4095
    rows["the first and the last entry of every slice"][ends] = to[ends]
    return rows


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 257, 2000, 151936, 151937])
def test_op_against_the_rule(q3, n):
    l = special_logits(n, 300 + n % 97)
    rng = np.random.Generator(np.random.PCG64(1000 + n))
    counts = rng.integers(0, 4, n).astype(np.uint32)
    for name, row in state_rows(n, rng).items():
        allowed = np.flatnonzero(row >= 0)
        listed = rng.permutation(n)[:min(n, 40)]
        # the ADD list bans nothing (a -inf over +inf is a NaN, which the standard leaves open); the ALLOW list names allowed and forbidden tokens
        lists = [("no list", [], br.ADD), ("an ADD list", [(int(t), float(f32(rng.uniform(-6, 6))), int(rng.integers(0, 2)) * 5) for t in listed], br.ADD),
                 ("an ALLOW list", [(int(t), float(rng.integers(0, 2)) * 0.75, 0) for t in sorted(set(listed[:8].tolist()) | set(allowed[:3].tolist()))], br.ALLOW)]
        for lname, entries, mode in lists:
            for c in (None, counts):
                what = f"n {n}, {name}, {lname}, counts {c is not None}"
                p, f = PEN if c is not None else (0.0, 0.0)
                got, idx = q3.ops.guide(l, row, entries, mode, 4, c, p, f)
                want = gr.rule(l, row, entries, mode, 4, c, p, f)
                assert got.tobytes() == want.tobytes(), f"{what}: {np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))} entries differ"
                assert idx == pr.argmax_key(want), what
                if name == "all allowed" and not entries and c is None:
                    assert got.tobytes() == l.tobytes(), what
                if not entries and c is None:
                    assert (got.view(np.uint32)[row < 0] == 0xFF800000).all() and got[row >= 0].tobytes() == l[row >= 0].tobytes(), what


# ---------------------------------------------------------------------------------------------------------------------
# the loops
# ---------------------------------------------------------------------------------------------------------------------
DEPTH = 3               # deciding states per chain: a request is decided at g = 0, 1 and 2, the last behind two state changes


def chain_guide(ref, prompts, n_new, sampler, prefix, V, n_states, chains, seed, eos=None, table=None, pen=(0.0, 0.0)):
    """A guide made of chains.  chains: [(states c_0 .. c_DEPTH, the requests that start in c_0)]; every request in no chain is
    unguided.  State c_i, i < DEPTH, allows a random half of the vocabulary, every token leading to c_{i+1}; c_DEPTH allows everything
    and stays (eos None), or allows eos alone (the accepting state: eos is allowed nowhere else).  Every state in no chain allows
    everything and stays.  Then, depth by depth, every chain state is made to DECIDE: the reference runs with the chains cut at that
    depth (the states from there on allow everything), and the token it commits there is forbidden in the state.  Returns
    (next, start per request, {(request, depth): the token forbidden for it})."""
    rng = np.random.Generator(np.random.PCG64(seed))
    next = np.repeat(np.arange(n_states, dtype=np.int16)[:, None], V, axis=1)
    start = [-1] * len(prompts)
    for states, reqs in chains:
        assert len(states) == DEPTH + 1
        for r in reqs:
            start[r] = states[0]
        for i in range(DEPTH):
            next[states[i]] = np.where(rng.random(V) < 0.5, states[i + 1], -1)
            if eos is not None:
                next[states[i], eos] = -1
        if eos is not None:
            next[states[DEPTH]] = -1
            next[states[DEPTH], eos] = states[DEPTH]
    forced = {}
    for i in range(DEPTH):
        cut = next.copy()
        for states, _ in chains:
            for k in range(i, DEPTH + 1):
                cut[states[k]] = states[min(k + 1, DEPTH)]
        got = gr.rows(ref, prompts, n_new, (cut, start), table, *pen, sampler, prefix)
        for states, reqs in chains:
            for r in reqs:
                forced[(r, i)] = got[r][i]
                next[states[i], got[r][i]] = -1
    assert (next >= 0).any(axis=1).all()
    return next, start, forced


def assert_decides(ref, prompts, n_new, sampler, prefix, guide, chains, forced, table=None, pen=(0.0, 0.0), stop=()):
    """on the reference: every guided request walks its chain, and at every depth the token the reference commits without that
    state's row is one the row forbids -- at g == 0, and at g == 2 behind two state changes"""
    next, start = guide
    want = gr.rows(ref, prompts, n_new, guide, table, *pen, sampler, prefix, stop)
    for states, reqs in chains:
        for r in reqs:
            s0 = gr.start_of(guide, r)
            assert s0 == states[0]
            for i in range(DEPTH):
                assert gr.state_of(next, s0, want[r][:i]) == states[i], (r, i)
                assert next[states[i], forced[(r, i)]] < 0 and want[r][i] != forced[(r, i)] and next[states[i], want[r][i]] >= 0, (r, i)
            assert len({states[0], states[1], states[2]}) == 3
    return want


def check_guides(t, ref, loop, prompts, n_new, sampler, guides, what, prefix=(), stop=(), table=None, pen=(0.0, 0.0), dense_min=2):
    """The loop with no guide against the reference first, then under every guide of `guides` (name -> (next, start))"""
    t.set_penalties(*pen)
    t.set_logit_bias(*(table or OFF))
    out = {}
    for name, guide in [("no guide", None)] + list(guides.items()):
        want = gr.rows(ref, prompts, n_new, guide, table, *pen, sampler, prefix, stop)
        t.set_guide(*(guide or NO_GUIDE))
        got = t.get_guide()
        assert got[1] == ([] if guide is None else [int(s) for s in guide[1]]) and (guide is None or np.array_equal(got[0], guide[0]))
        rows = run_loop(t, loop, prompts, n_new, sampler, stop, dense_min)
        assert rows == want, f"{what}: {name}: other tokens than the reference" + (" -- THE REFERENCE FAILS THE EXISTING LOOP" if guide is None else "")
        out[name] = rows
    t.set_guide(*NO_GUIDE)
    t.set_logit_bias([])
    t.set_penalties(0.0, 0.0)
    return out


@pytest.fixture(scope="module")
def designed(q3, tmp_path_factory):
    """the designed checkpoints (logits depend on the input token alone) and one single-stream reference engine each"""
    d = tmp_path_factory.mktemp("guide")
    made = {}

    def get(file):
        if file not in made:
            path = lc.write(str(d / f"{file}.bin"), file)
            made[file] = (path, pr.Engine(q3, path))
        return made[file]
    yield get
    for _, ref in made.values():
        ref.close()


ONE_CHAIN = [([0, 1, 2, 3], [0, 1, 2, 3, 4])]
# one chain per request in a table of 4096 states: start states 0 and 4095 among them, chains that run down and chains that jump
PER_REQUEST = [([0, 1, 2, 3], [0]), ([4095, 4094, 4093, 4092], [1]), ([2000, 7, 2001, 9], [2]), ([100, 101, 102, 103], [3]), ([50, 49, 48, 47], [4])]
MIXED = [PER_REQUEST[0], PER_REQUEST[2], PER_REQUEST[4]]           # requests 1 and 3 unguided
EOS = 1234


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("file", ["small_a", "small_b"])
def test_designed_checkpoints(q3, designed, file, loop, sampled):
    """V = 2,000, 5 requests on 3 slots (slots are reused), request 2 at temperature 0 under the sampler.  On the stop loop EOS is
    allowed only in the accepting states, and every guided request ends there, short of its n_new"""
    path, ref = designed(file)
    sampler = D_SAMPLER if sampled else None
    prefix = D_PREFIX if loop == "prefix" else ()
    eos, stop = (EOS, [EOS]) if loop == "stop" else (None, ())
    V = lc.V_SMALL
    guides = {}
    for name, n_states, chains, seed in (("one for all", DEPTH + 1, ONE_CHAIN, 31), ("one per request, 4096 states", 4096, PER_REQUEST, 32),
                                         ("two requests unguided", 4096, MIXED, 33)):
        next, start, forced = chain_guide(ref, D_PROMPTS, D_NEW, sampler, prefix, V, n_states, chains, seed, eos)
        guide = (next, [0] if chains is ONE_CHAIN else start)
        assert chains is ONE_CHAIN or (0 in start and 4095 in start or chains is MIXED)
        want = assert_decides(ref, D_PROMPTS, D_NEW, sampler, prefix, guide, chains, forced, stop=stop)
        if eos is not None:
            guided = [r for _, reqs in chains for r in reqs]
            assert all(want[r][DEPTH:] == [eos] and len(want[r]) < D_NEW[r] for r in guided), "no request ends early under the guide"
        guides[name] = guide
    free = gr.rows(ref, D_PROMPTS, D_NEW, None, None, 0.0, 0.0, sampler, prefix, stop)
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(3)
        if prefix:
            t.batch_prefix_set(prefix)
        out = check_guides(t, ref, loop_name(loop, sampled), D_PROMPTS, D_NEW, sampler, guides, f"{file} {loop}", prefix, stop)
        # start -1: the rows of the call with no guide
        assert [out["two requests unguided"][r] for r in (1, 3)] == [out["no guide"][r] for r in (1, 3)] == [free[r] for r in (1, 3)]
        if eos is not None:
            assert any(len(r) < n for r, n in zip(out["one for all"], D_NEW))


@pytest.mark.parametrize("loop", ["greedy", "dense", "prefix"])
def test_a_row_with_no_finite_entry_commits_the_last_token_and_the_state_stays(q3, designed, loop):
    """Defined behaviour, not a fault: a table of section 2q bans the only tokens state 0 allows for g < 3.  Greedy commits V - 1 by
    the key rule, which state 0 forbids: the state stays, so at g == 3 the row is still state 0's -- one of its two tokens comes, and
    only then the request moves on to the state that allows everything."""
    path, ref = designed("small_a")
    V = lc.V_SMALL
    prefix = D_PREFIX if loop == "prefix" else ()
    free = gr.rows(ref, D_PROMPTS, D_NEW, None, None, 0.0, 0.0, None, prefix)
    a, b = 700, 1301
    assert all(a not in row and b not in row for row in free)
    next = np.full((2, V), -1, dtype=np.int16)
    next[0, [a, b]] = 1
    next[1] = 1
    guide, table = (next, [0]), ([[(a, -INF, 3), (b, -INF, 3), (V - 1, -INF, 3)]], [br.ADD])       # (V - 1 is banned too: it comes all the same)
    want = gr.rows(ref, D_PROMPTS, D_NEW, guide, table, 0.0, 0.0, None, prefix)
    for r, row in enumerate(want):
        assert row[:3] == [V - 1] * 3 and row[3] in (a, b) and gr.state_of(next, 0, row[:3]) == 0 and gr.state_of(next, 0, row[:4]) == 1, r
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(3)
        if prefix:
            t.batch_prefix_set(prefix)
        check_guides(t, ref, loop, D_PROMPTS, D_NEW, None, {"two tokens, both banned": guide}, loop, prefix, table=table)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_designed_checkpoint_at_the_full_vocabulary(q3, designed, sampled):
    """V = 151,936 (big_a): state 0 allows only tokens of the last slice, state 1 only tokens of the first"""
    path, ref = designed("big_a")
    V = lc.V_BIG
    prompts, n_new = [[0], [2, 1], [3]], [5, 4, 4]
    sampler = ([0.0, 0.7, 1.0], 0.9, [900, 901, 902]) if sampled else None
    bounds = [(a, b) for a, b in slice_bounds(V) if b > a]
    (f0, f1), (l0, l1) = bounds[0], bounds[-1]
    next = np.full((2, V), -1, dtype=np.int16)
    next[0, l0:l1] = 1
    next[1, f0:f1] = 0
    guide = (next, [0])
    free = gr.rows(ref, prompts, n_new, None, None, 0.0, 0.0, sampler)
    # (the designs peak inside the two slices: what the unconstrained rows hold is forbidden in both states)
    next[:, sorted({tok for row in free for tok in row})] = -1
    want = gr.rows(ref, prompts, n_new, guide, None, 0.0, 0.0, sampler)
    for r, row in enumerate(want):
        assert all((l0 <= tok < l1) if g % 2 == 0 else (f0 <= tok < f1) for g, tok in enumerate(row)), r
        assert not set(row) & set(free[r]), r
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(2)
        check_guides(t, ref, "sampled" if sampled else "greedy", prompts, n_new, sampler, {"last slice, first slice": guide}, "big_a")


@pytest.mark.parametrize("loop", ["greedy", "sampled", "dense", "stop", "prefix"])
def test_a_guide_beside_a_table_penalties_and_top_k(q3, designed, loop):
    """a chain per request, a list per request (ADD and ALLOW), penalties (1.5, 0.5) on top, top_k 20 in front of every draw"""
    path, ref = designed("small_b")
    V = lc.V_SMALL
    sampler = None if loop == "greedy" else D_SAMPLER
    prefix = D_PREFIX if loop == "prefix" else ()
    eos, stop = (EOS, [EOS]) if loop == "stop" else (None, ())
    ref.top_k = 20
    try:
        rng = np.random.Generator(np.random.PCG64(78))
        lists, modes = [], []
        for r in range(5):
            if r % 2:
                # (an ALLOW list wide enough to meet every half of the vocabulary a chain state allows, and the stop token)
                lists.append([(int(x), float(f32(rng.uniform(-2, 2))), 0) for x in sorted(set(rng.permutation(V)[:60].tolist()) | {EOS})])
                modes.append(br.ALLOW)
            else:
                lists.append([(int(x), float(f32(rng.uniform(-6, 6))), int(rng.integers(0, 6))) for x in rng.permutation(V)[:30]])
                modes.append(br.ADD)
        table = (lists, modes)
        next, start, forced = chain_guide(ref, D_PROMPTS, D_NEW, sampler, prefix, V, 4096, PER_REQUEST, 34, eos, table, PEN)
        guide = (next, start)
        want = assert_decides(ref, D_PROMPTS, D_NEW, sampler, prefix, guide, PER_REQUEST, forced, table, PEN, stop)
        # the table and the penalties decide something on top of the guide
        assert want != gr.rows(ref, D_PROMPTS, D_NEW, guide, None, *PEN, sampler, prefix, stop)
        if eos is None:
            assert want != gr.rows(ref, D_PROMPTS, D_NEW, guide, table, 0.0, 0.0, sampler, prefix, stop)
        with q3.TransformerBuilder(path).build() as t:
            t.batch_init(3)
            t.set_top_k(20)
            if prefix:
                t.batch_prefix_set(prefix)
            check_guides(t, ref, loop, D_PROMPTS, D_NEW, sampler, {"a chain per request": guide}, f"{loop}, table, penalties, top_k 20", prefix, stop, table, PEN)
            # the guide beside the table alone, beside the penalties alone, and alone: the masked form with and without lists and counts
            check_guides(t, ref, loop, D_PROMPTS, D_NEW, sampler, {"a chain per request": guide}, f"{loop}, table, top_k 20", prefix, stop, table)
            check_guides(t, ref, loop, D_PROMPTS, D_NEW, sampler, {"a chain per request": guide}, f"{loop}, penalties, top_k 20", prefix, stop, None, PEN)
            check_guides(t, ref, loop, D_PROMPTS, D_NEW, sampler, {"a chain per request": guide}, f"{loop}, top_k 20", prefix, stop)
    finally:
        ref.top_k = 0


@pytest.fixture(scope="module")
def model(q3, tmp_path_factory):
    """tests/test_genlp.py's shape: 11 prompts of the small synthetic checkpoint, a 6-token prefix, one reference engine"""
    path = str(tmp_path_factory.mktemp("guide_small") / f"{NAME}.bin")
    shape = q3.checkpoint.SHAPES[NAME]
    q3.checkpoint.write_synthetic_checkpoint(path, shape, seed=2468)
    prompts = [[int(x) for x in np.random.default_rng(6100 + r).integers(0, shape.vocab_size, n)] for r, n in enumerate(LENS)]
    prefix = [int(x) for x in np.random.default_rng(6200).integers(0, shape.vocab_size, PREFIX_LEN)]
    ref = pr.Engine(q3, path, ctx=CTX)
    yield path, shape.vocab_size, prompts, prefix, ref
    ref.close()


def two_state_guide(ref, prompts, n_new, sampler, prefix, V, seed, unguided=()):
    """two states that each allow a random half of the vocabulary and lead to each other; state 0 forbids every request's
    unconstrained first token; request r starts in state r % 2 (its first token is forbidden there too), or is unguided"""
    rng = np.random.Generator(np.random.PCG64(seed))
    free = gr.rows(ref, prompts, n_new, None, None, 0.0, 0.0, sampler, prefix)
    next = np.stack([np.where(rng.random(V) < 0.5, 1, -1), np.where(rng.random(V) < 0.5, 0, -1)]).astype(np.int16)
    next[:, [row[0] for row in free]] = -1
    start = [-1 if r in unguided else r % 2 for r in range(len(prompts))]
    want = gr.rows(ref, prompts, n_new, (next, start), None, 0.0, 0.0, sampler, prefix)
    assert all((w == f) == (r in unguided) for r, (w, f) in enumerate(zip(want, free)))
    return next, start


def test_the_setting_leaks_nowhere(q3, model):
    """under a guide: batch_step_cols, batch_step_cols_draw, forward_batch, score, choose, embed and single-stream decode give the
    bytes they give with none; a generate call with another number of requests than start states is refused and leaves the caches
    alone; after set_guide(None, []) tokens and cache rows of every loop are those of an engine that never saw a guide"""
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
        got.append(t.forward_batch([3, 4, 5, 6], [2, 2, 2, 2]))
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
    guide = two_state_guide(ref, some, n_new, sampler, (), V, 41)
    with engine(q3, path, slots=4) as t:
        t.batch_prefix_set(prefix)
        t.set_guide(*guide)
        under = loops(t)
        assert under[0][0] != fresh[0][0] and under[1][0] == gr.rows(ref, some, n_new, guide, None, 0.0, 0.0, sampler)
        assert others(t) == plain
        # 6 start states, 5 requests: refused before anything runs
        t.batch_reset_kv()
        t.batch_prefix_set(prefix)
        assert loops(t) == under
        caches = slot_rows(t, 4)
        for loop, smp, stop in calls:
            with pytest.raises(IndexError, match="6 start states"):
                run_loop(t, loop, some[:5], n_new[:5], None if smp is None else (smp[0][:5], smp[1], smp[2][:5]), stop)
        assert slot_rows(t, 4) == caches and t.get_guide()[1] == guide[1]
        # a table over another vocabulary: refused with the model at hand, the guide stays
        with pytest.raises(q3.Q3Error, match="vocab_size"):
            t.set_guide(np.zeros((2, V + 1), dtype=np.int16), [0])
        assert t.get_guide()[1] == guide[1]
        assert run_loop(t, "sampled", some, n_new, sampler) == under[1][0]
        # off: the caches start as a fresh engine's do
        t.set_guide(*NO_GUIDE)
        t.batch_reset_kv()
        t.batch_prefix_set(prefix)
        got = loops(t)
        assert [g[0] for g in got] == [w[0] for w in fresh], "other tokens than on an engine that never saw a guide"
        assert [g[1] for g in got] == [w[1] for w in fresh], "other cache rows than on an engine that never saw a guide"


def test_the_guide_survives(q3, model):
    path, V, prompts, prefix, ref = model
    few, n_new = prompts[:3], [4, 5, 3]
    guide = two_state_guide(ref, few, n_new, None, (), V, 42)
    one = (guide[0], [1])
    with q3.TransformerBuilder(path).with_ctx_length(CTX).build() as t:
        assert t.get_guide() == NO_GUIDE
        t.set_guide(*guide)                                          # no batched state yet: the first generate call makes the device side
        t.batch_init(4, CTX)
        want = gr.rows(ref, few, n_new, guide)
        assert run_loop(t, "greedy", few, n_new, None) == want
        t.set_sampler(0.7, 0.9, 3)
        t.set_sampler(0.0, 0.9, 3)
        t.set_top_k(7)
        t.set_gen_logprobs(3)
        t.set_penalties(1.0, 0.0)
        t.set_penalties(0.0, 0.0)
        t.set_logit_bias([[(1, 0.5, 0)]])
        t.set_logit_bias([])
        t.set_gen_logprobs(-1)
        t.batch_init(4, CTX)                                         # a new batched state: the table goes up again
        assert t.get_guide()[1] == guide[1]
        assert run_loop(t, "greedy", few, n_new, None) == want
        assert run_loop(t, "greedy", few, n_new, None) == want       # and stays there for the next call
        # a refused guide changes nothing
        with pytest.raises(q3.Q3Error, match="allows no token"):
            t.set_guide([[-1] * V], [0])
        assert run_loop(t, "greedy", few, n_new, None) == want
        # two guides, the same plans: one start state for every request, any number of requests; then the per-request one again
        t.set_guide(*one)
        assert run_loop(t, "greedy", prompts[:5], N_NEW[:5], None) == gr.rows(ref, prompts[:5], N_NEW[:5], one)
        t.set_guide(*guide)
        assert run_loop(t, "greedy", few, n_new, None) == want
        # clearing it restores the unguided rows
        t.set_guide(*NO_GUIDE)
        assert run_loop(t, "greedy", few, n_new, None) == gr.rows(ref, few, n_new) != want


def test_records_stay_on_the_raw_rows(q3, model):
    """set_gen_logprobs(5) under a guide: the tokens of the call without records, the records of score_top_many on prompt + row
    everywhere, and the records of the call without a guide wherever the committed tokens agree up to there"""
    import genlp_ref as glr
    path, V, prompts, prefix, ref = model
    guide = two_state_guide(ref, prompts, N_NEW, SAMPLER, (), V, 43, unguided=(1, 4, 10))
    with engine(q3, path) as t:
        t.set_gen_logprobs(5)
        free = run_loop(t, "sampled", prompts, N_NEW, SAMPLER)
        free_recs = t.read_gen_logprobs()
        t.set_gen_logprobs(-1)
        t.set_guide(*guide)
        rows = run_loop(t, "sampled", prompts, N_NEW, SAMPLER)
        assert rows == gr.rows(ref, prompts, N_NEW, guide, None, 0.0, 0.0, SAMPLER)
        t.set_gen_logprobs(5)
        assert run_loop(t, "sampled", prompts, N_NEW, SAMPLER) == rows
        got = t.read_gen_logprobs()
        glr.assert_same(got, glr.expected(t, prompts, rows, 5), rows, 5, "under a guide")
        same = 0
        for r, (a, b) in enumerate(zip(rows, free)):
            for g in range(min(len(a), len(b))):
                if a[:g + 1] != b[:g + 1]:
                    break
                for x, y in zip(got[r], free_recs[r]):
                    assert np.asarray(x[g]).tobytes() == np.asarray(y[g]).tobytes(), (r, g)
                same += 1
        assert same >= sum(N_NEW[r] for r in (1, 4, 10))


def test_generate_many_takes_automata(q3, model):
    path, V, prompts, prefix, ref = model
    some = prompts[:6]
    A = q3.guide.Automaton
    kept = two_state_guide(ref, some, [5] * 6, None, (), V, 44)
    labels = A.from_sequences([[7, 8, 9], [7, 30], [41, 42, 43, 44]], V, eos=0)
    other = A(kept[0], 1)
    with engine(q3, path, slots=4) as t:
        t.set_guide(*kept)
        # with guide=None the engine's guide simply holds
        assert q3.generate_many(t, some, 5)[0] == gr.rows(ref, some, [5] * 6, kept)
        # one automaton for all: every row is one of the labels, then eos, where it ends
        rows = q3.generate_many(t, some, 6, stop_tokens=[0], stop_on_device=True, guide=labels)[0]
        assert rows == gr.rows(ref, some, [6] * 6, (labels.next, [0]), None, 0.0, 0.0, None, (), [0])
        assert all(labels.walk(r)[1] is None and r[-1] == 0 and len(r) < 6 for r in rows)
        g, got = t.get_guide()
        assert np.array_equal(g, kept[0]) and got == kept[1]
        # one per request, None among them; merged behind one another
        per = [labels, None, other, labels, None, other]
        merged = q3.guide.merge_guides(per, 6)
        assert merged[1] == [0, -1, labels.n_states + 1, 0, -1, labels.n_states + 1]
        for kw in ({}, dict(sampler=(0.8, 0.9, list(range(11, 17)))), dict(shared_prefix=prefix)):
            rows = q3.generate_many(t, some, 5, guide=per, **kw)[0]
            assert rows == gr.rows(ref, some, [5] * 6, merged, None, 0.0, 0.0, kw.get("sampler"), kw.get("shared_prefix", ())), kw
            assert t.get_guide()[1] == kept[1]
        with pytest.raises(IndexError):
            q3.generate_many(t, [[10 ** 9]], 5, guide=labels)
        assert t.get_guide()[1] == kept[1]
