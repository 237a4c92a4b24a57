"""Sparse guides inside the five q3_generate_many_* loops (include/qwen3_hip.h section 2s).  The rule is section 2r's, so the
yardstick is tests/guide_ref.py on a DENSE table: the operator against gr.rule on the dense row of the state, the loops against
gr.rows under the dense twin of the guide.  guide_ref.digest casts the table to int16, so where the engine's guide uses state
numbers above 4,095 the reference runs on a compacted dense table with the states in use renumbered (compact_to_big below).  The
designed checkpoints, chain_guide and assert_decides are tests/test_guide.py's: every guide first DECIDES on the reference, then
the engine is held to it in both forms, dense and sparse, in one engine.  No tolerance: rows as bytes, tokens as integers."""
import re

import numpy as np
import pytest

import bias_ref as br
import guide_ref as gr
import logit_ckpt as lc
import pen_ref as pr
from test_bias import LOOPS, OFF, PEN, loop_name, run_loop
from test_genlp import CTX, N_NEW, SAMPLER, engine, slot_rows
from test_guide import (DEPTH, EOS, MIXED, NO_GUIDE, ONE_CHAIN, PER_REQUEST, assert_decides, chain_guide, designed, model,  # noqa: F401 (fixtures)
                        two_state_guide)
from test_penalty import D_NEW, D_PREFIX, D_PROMPTS, D_SAMPLER, slice_bounds, special_logits

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = float("inf")
NO_SPARSE = (None, None, None, None, [])
BIG = 1 << 20


def compress(row, prefer_allowed=False):
    """one dense row as (default, tokens, targets): the default is the row's most frequent value -- or, prefer_allowed, its most
    frequent ALLOWED value, so that a state which forbids half of the vocabulary lists that half as forbidding edges"""
    row = np.asarray(row).astype(np.int64)
    counts = np.bincount(row + 1)
    if prefer_allowed and counts[1:].any():
        counts[0] = 0
    default = int(counts.argmax()) - 1
    tokens = np.flatnonzero(row != default)
    return default, tokens.astype(np.int32), row[tokens].astype(np.int32)


def sparse_of(next, prefer_allowed=False):
    """the arrays of set_guide_sparse for a dense table"""
    rows = [compress(r, prefer_allowed) for r in np.asarray(next)]
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([r[1].size for r in rows], out=offsets[1:])
    return np.array([r[0] for r in rows], dtype=np.int32), offsets, np.concatenate([r[1] for r in rows]), np.concatenate([r[2] for r in rows])


def compact_to_big(next, big_of, n_big=BIG):
    """The helper map for guides with large state numbers.  next: a compact dense table whose state c is state big_of[c] of the
    engine's guide.  Returns the arrays of a sparse guide of n_big states: the states of big_of carry the compact rows with every
    target renamed; every other state allows everything and stays where it is."""
    big_of = np.asarray(big_of, dtype=np.int64)
    assert len(set(big_of.tolist())) == len(big_of) == len(next) and big_of.min() >= 0 and big_of.max() < n_big
    default = np.arange(n_big, dtype=np.int32)
    count = np.zeros(n_big, dtype=np.int64)
    rows = {}
    for c, b in enumerate(big_of):
        d, tokens, targets = compress(next[c], prefer_allowed=c % 2 == 0)
        rename = lambda a: np.where(np.asarray(a) >= 0, big_of[np.maximum(a, 0)], -1)
        default[b] = rename(d)
        rows[int(b)] = (tokens, rename(targets).astype(np.int32))
        count[b] = tokens.size
    offsets = np.zeros(n_big + 1, dtype=np.int64)
    np.cumsum(count, out=offsets[1:])
    order = sorted(rows)
    return default, offsets, np.concatenate([rows[b][0] for b in order]), np.concatenate([rows[b][1] for b in order])


# ---------------------------------------------------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------------------------------------------------
def states(n, rng):
    """one state in the forms that matter to the kernel, as name -> (default, tokens, targets); the dense row is made from them"""
    to = rng.integers(0, BIG, n).astype(np.int32)
    every = np.arange(n, dtype=np.int32)
    ends = np.array(sorted({a for a, b in slice_bounds(n) if b > a} | {b - 1 for a, b in slice_bounds(n) if b > a}), dtype=np.int32)
    half = np.flatnonzero(rng.random(n) < 0.5).astype(np.int32)
    if half.size == 0:
        half = every[:1]
    some = rng.permutation(n)[:max(n // 3, 1)].astype(np.int32)
    some.sort()
    none = np.zeros(0, dtype=np.int32)
    mixed = np.where(rng.random(n) < 0.5, to, -1).astype(np.int32)
    mixed[rng.integers(0, n)] = 7
    forbid = lambda tokens: np.full(tokens.size, -1, dtype=np.int32)
    keep_one = lambda tokens: tokens[:-1] if tokens.size == n else tokens        # (a state has to allow something)
    redundant = np.where(np.arange(some.size) % 2 == 0, to[some], -1).astype(np.int32)
    high = np.where(np.arange(half.size) % 3 == 0, -1, BIG - 1 - np.arange(half.size) % 5).astype(np.int32)
    high[-1] = BIG - 1
    return {
        "default allowed, no edges": (5, none, none),
        "default -1, the single edge at token 0": (-1, every[:1], to[:1]),
        "default -1, the single edge at n - 1": (-1, every[-1:], np.array([BIG - 1], dtype=np.int32)),
        "default -1, edges at the first and last token of every slice": (-1, ends, to[ends]),
        "default allowed, forbidding edges at the first and last token of every slice": (BIG - 1, keep_one(ends), forbid(keep_one(ends))),
        "default -1, a random half allowed": (-1, half, to[half]),
        "default allowed, a random half forbidden": (3, keep_one(half), forbid(keep_one(half))),
        "every token listed": (-1, every, mixed),
        "redundant edges: next -1 under default -1": (-1, some, redundant),
        "targets up to n_states - 1": (BIG - 1, half, high),
    }


def dense_row(n, default, tokens, targets):
    row = np.full(n, default, dtype=np.int64)
    row[tokens] = targets
    return row


def check_state(q3, l, n, name, state, rng, counts):
    default, tokens, targets = state
    row = dense_row(n, default, tokens, targets)
    assert (row >= 0).any(), name
    allowed = np.flatnonzero(row >= 0)
    listed = rng.permutation(n)[:min(n, 40)]
    # the ADD list bans nothing (a -inf over +inf is a NaN, which the standard leaves open); the ALLOW list names allowed and forbidden tokens
    lists = [("no list", [], br.ADD), ("an ADD list", [(int(t), float(f32(rng.uniform(-6, 6))), int(rng.integers(0, 2)) * 5) for t in listed], br.ADD),
             ("an ALLOW list", [(int(t), float(rng.integers(0, 2)) * 0.75, 0) for t in sorted(set(listed[:8].tolist()) | set(allowed[:3].tolist()))], br.ALLOW)]
    for lname, entries, mode in lists:
        for c in (None, counts):
            what = f"n {n}, {name}, {lname}, counts {c is not None}"
            p, f = PEN if c is not None else (0.0, 0.0)
            got, idx = q3.ops.guide_sparse(l, default, tokens, targets, entries, mode, 4, c, p, f)
            want = gr.rule(l, row, entries, mode, 4, c, p, f)
            assert got.tobytes() == want.tobytes(), f"{what}: {np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))} entries differ"
            assert idx == pr.argmax_key(want), what
            if not entries and c is None:
                assert (got.view(np.uint32)[row < 0] == 0xFF800000).all() and got[row >= 0].tobytes() == l[row >= 0].tobytes(), what


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 257, 2000, 151936, 151937])
def test_op_against_the_rule(q3, n):
    l = special_logits(n, 300 + n % 97)
    rng = np.random.Generator(np.random.PCG64(2000 + n))
    counts = rng.integers(0, 4, n).astype(np.uint32)
    forms = states(n, rng)
    assert len(forms) == 10
    for name, state in forms.items():
        check_state(q3, l, n, name, state, rng, counts)


@pytest.mark.parametrize("n", [300000, 300001])
def test_op_on_slices_longer_than_the_flag_array(q3, n):
    """above 64 x 4,096 tokens a slice is walked in more than one chunk of flag bytes: both the 16-byte and the single-entry path"""
    assert (n + 63) // 64 > 4096
    l = special_logits(n, 300 + n % 97)
    rng = np.random.Generator(np.random.PCG64(2000 + n))
    counts = rng.integers(0, 4, n).astype(np.uint32)
    forms = states(n, rng)
    for name in ("default -1, a random half allowed", "default allowed, a random half forbidden",
                 "default -1, edges at the first and last token of every slice", "default -1, the single edge at n - 1"):
        check_state(q3, l, n, name, forms[name], rng, counts)


# ---------------------------------------------------------------------------------------------------------------------
# the loops
# ---------------------------------------------------------------------------------------------------------------------
def check_both_forms(t, ref, loop, prompts, n_new, sampler, guides, what, prefix=(), stop=(), table=None, pen=(0.0, 0.0), dense_min=2):
    """The loop with no guide against the reference first, then under every guide of `guides` (name -> (next, start[, sparse
    arrays])) in its dense form and in its sparse form: the tokens of gr.rows under the dense table, and the getters say which form
    holds."""
    t.set_penalties(*pen)
    t.set_logit_bias(*(table or OFF))
    out = {}
    want = gr.rows(ref, prompts, n_new, None, table, *pen, sampler, prefix, stop)
    t.set_guide(*NO_GUIDE)
    assert run_loop(t, loop, prompts, n_new, sampler, stop, dense_min) == want, f"{what}: no guide -- THE REFERENCE FAILS THE EXISTING LOOP"
    out["no guide"] = want
    for name, guide in guides.items():
        next, start = guide[0], [int(s) for s in guide[1]]
        want = gr.rows(ref, prompts, n_new, (next, start), table, *pen, sampler, prefix, stop)
        forms = [("sparse, most frequent default", sparse_of(next)), ("sparse, allowed default", sparse_of(next, True))] if len(guide) == 2 else [("sparse", guide[2])]
        if len(guide) == 2:
            forms.insert(1, ("dense", None))
        for form, arrays in forms:
            if arrays is None:
                t.set_guide(next, start)
                assert t.get_guide()[1] == start and t.get_guide_sparse() == NO_SPARSE
            else:
                t.set_guide_sparse(*arrays, start)
                got = t.get_guide_sparse()
                assert t.get_guide() == NO_GUIDE and got[4] == start and all(np.array_equal(a, b) for a, b in zip(got[:4], arrays))
            rows = run_loop(t, loop, prompts, n_new, sampler, stop, dense_min)
            assert rows == want, f"{what}: {name}, {form}: other tokens than the reference"
        out[name] = want
    t.set_guide_sparse(None, None, None, None, [])
    assert t.get_guide() == NO_GUIDE and t.get_guide_sparse() == NO_SPARSE
    t.set_logit_bias([])
    t.set_penalties(0.0, 0.0)
    return out


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("file", ["small_a", "small_b"])
def test_designed_checkpoints(q3, designed, file, loop, sampled):
    """V = 2,000, 5 requests on 3 slots (slots are reused).  Every chain state allows a random half of the vocabulary: in the form
    with the allowed default it lists about V / 2 forbidding edges, some in every slice"""
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
        want = assert_decides(ref, D_PROMPTS, D_NEW, sampler, prefix, guide, chains, forced, stop=stop)
        if eos is not None:
            guided = [r for _, reqs in chains for r in reqs]
            assert all(want[r][DEPTH:] == [eos] and len(want[r]) < D_NEW[r] for r in guided), "no request ends early under the guide"
        guides[name] = guide
    d, off, _, targets = sparse_of(guides["one for all"][0], True)
    bounds = [(a, b) for a, b in slice_bounds(V) if b > a]
    for s in range(DEPTH):
        a, b = int(off[s]), int(off[s + 1])
        tokens = sparse_of(guides["one for all"][0], True)[2][a:b]
        assert d[s] >= 0 and V // 3 < b - a < 2 * V // 3 and (targets[a:b] == -1).all(), "a chain state with default allowed and about V / 2 forbidding edges"
        assert all(((tokens >= lo) & (tokens < hi)).any() for lo, hi in bounds), "edges in every slice"
    free = gr.rows(ref, D_PROMPTS, D_NEW, None, None, 0.0, 0.0, sampler, prefix, stop)
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(3)
        if prefix:
            t.batch_prefix_set(prefix)
        out = check_both_forms(t, ref, loop_name(loop, sampled), D_PROMPTS, D_NEW, sampler, guides, f"{file} {loop}", prefix, stop)
        # start -1: the rows of the call with no guide
        assert [out["two requests unguided"][r] for r in (1, 3)] == [out["no guide"][r] for r in (1, 3)] == [free[r] for r in (1, 3)]


BIG_STATES = [0, 1, 2, 32767, 32768, 40000, 65535, 65536, 70000, BIG - 3, BIG - 2, BIG - 1]
BIG_CHAINS = [([0, 32768, 65535, BIG - 1], [0, 3]), ([BIG - 2, 65536, 32767, 1], [1]), ([40000, BIG - 3, 2, 70000], [2, 4])]


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("loop", LOOPS)
def test_a_guide_of_1048576_states(q3, designed, loop, sampled):
    """chains at states 0, 32,768, 65,535 and 1,048,575 (and their neighbours) of a guide with 2^20 states, against the reference on
    the compacted dense table of the twelve states in use"""
    path, ref = designed("small_a")
    sampler = D_SAMPLER if sampled else None
    prefix = D_PREFIX if loop == "prefix" else ()
    eos, stop = (EOS, [EOS]) if loop == "stop" else (None, ())
    small = {b: c for c, b in enumerate(BIG_STATES)}
    chains = [([small[b] for b in states], reqs) for states, reqs in BIG_CHAINS]
    next, start, forced = chain_guide(ref, D_PROMPTS, D_NEW, sampler, prefix, lc.V_SMALL, len(BIG_STATES), chains, 35, eos)
    assert_decides(ref, D_PROMPTS, D_NEW, sampler, prefix, (next, start), chains, forced, stop=stop)
    arrays = compact_to_big(next, BIG_STATES)
    big_start = [-1 if s < 0 else BIG_STATES[s] for s in start]
    assert arrays[0].size == BIG and {0, 32768, 65535, BIG - 1} <= {int(x) for x in arrays[3]} | {int(arrays[0][b]) for b in BIG_STATES} | set(big_start)
    assert big_start == [0, BIG - 2, 40000, 0, 40000]
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(3)
        if prefix:
            t.batch_prefix_set(prefix)
        want = gr.rows(ref, D_PROMPTS, D_NEW, (next, start), None, 0.0, 0.0, sampler, prefix, stop)
        t.set_guide_sparse(*arrays, big_start)
        assert t.get_guide_sparse()[4] == big_start and t.get_guide() == NO_GUIDE
        for _ in range(2):                              # the second call finds the table on the device
            assert run_loop(t, loop_name(loop, sampled), D_PROMPTS, D_NEW, sampler, stop, 2) == want


@pytest.mark.parametrize("loop", ["greedy", "dense", "prefix"])
def test_a_row_with_no_finite_entry_commits_the_last_token_and_the_state_stays(q3, designed, loop):
    """tests/test_guide.py's case in both forms: a table of section 2q bans the only tokens state 0 allows for g < 3; V - 1 comes, which
    state 0 forbids, and the state stays"""
    path, ref = designed("small_a")
    V = lc.V_SMALL
    prefix = D_PREFIX if loop == "prefix" else ()
    free = gr.rows(ref, D_PROMPTS, D_NEW, None, None, 0.0, 0.0, None, prefix)
    a, b = 700, 1301
    assert all(a not in row and b not in row for row in free)
    next = np.full((2, V), -1, dtype=np.int16)
    next[0, [a, b]] = 1
    next[1] = 1
    guide, table = (next, [0]), ([[(a, -INF, 3), (b, -INF, 3), (V - 1, -INF, 3)]], [br.ADD])
    want = gr.rows(ref, D_PROMPTS, D_NEW, guide, table, 0.0, 0.0, None, prefix)
    for r, row in enumerate(want):
        assert row[:3] == [V - 1] * 3 and row[3] in (a, b) and gr.state_of(next, 0, row[:3]) == 0 and gr.state_of(next, 0, row[:4]) == 1, r
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(3)
        if prefix:
            t.batch_prefix_set(prefix)
        check_both_forms(t, ref, loop, D_PROMPTS, D_NEW, None, {"two tokens, both banned": guide}, loop, prefix, table=table)


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
    next[:, sorted({tok for row in free for tok in row})] = -1
    want = gr.rows(ref, prompts, n_new, guide, None, 0.0, 0.0, sampler)
    for r, row in enumerate(want):
        assert all((l0 <= tok < l1) if g % 2 == 0 else (f0 <= tok < f1) for g, tok in enumerate(row)), r
        assert not set(row) & set(free[r]), r
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(2)
        check_both_forms(t, ref, "sampled" if sampled else "greedy", prompts, n_new, sampler, {"last slice, first slice": guide}, "big_a")


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
                lists.append([(int(x), float(f32(rng.uniform(-2, 2))), 0) for x in sorted(set(rng.permutation(V)[:60].tolist()) | {EOS})])
                modes.append(br.ALLOW)
            else:
                lists.append([(int(x), float(f32(rng.uniform(-6, 6))), int(rng.integers(0, 6))) for x in rng.permutation(V)[:30]])
                modes.append(br.ADD)
        table = (lists, modes)
        next, start, forced = chain_guide(ref, D_PROMPTS, D_NEW, sampler, prefix, V, 4096, PER_REQUEST, 34, eos, table, PEN)
        guide = (next, start)
        want = assert_decides(ref, D_PROMPTS, D_NEW, sampler, prefix, guide, PER_REQUEST, forced, table, PEN, stop)
        assert want != gr.rows(ref, D_PROMPTS, D_NEW, guide, None, *PEN, sampler, prefix, stop)
        with q3.TransformerBuilder(path).build() as t:
            t.batch_init(3)
            t.set_top_k(20)
            if prefix:
                t.batch_prefix_set(prefix)
            check_both_forms(t, ref, loop, D_PROMPTS, D_NEW, sampler, {"a chain per request": guide}, f"{loop}, table, penalties, top_k 20", prefix, stop, table, PEN)
            check_both_forms(t, ref, loop, D_PROMPTS, D_NEW, sampler, {"a chain per request": guide}, f"{loop}, table, top_k 20", prefix, stop, table)
            check_both_forms(t, ref, loop, D_PROMPTS, D_NEW, sampler, {"a chain per request": guide}, f"{loop}, penalties, top_k 20", prefix, stop, None, PEN)
    finally:
        ref.top_k = 0


# ---------------------------------------------------------------------------------------------------------------------
# settings
# ---------------------------------------------------------------------------------------------------------------------
def test_the_setting_leaks_nowhere(q3, model):
    """under a sparse guide the non-generate calls give their unguided bytes; a call with another number of requests than start
    states is refused with the caches intact; after clearing, tokens and cache rows of every loop are those of an engine that never
    saw a guide"""
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
    next, start = two_state_guide(ref, some, n_new, sampler, (), V, 41, unguided=(2,))
    arrays = sparse_of(next, True)
    with engine(q3, path, slots=4) as t:
        t.batch_prefix_set(prefix)
        t.set_guide_sparse(*arrays, start)
        under = loops(t)
        want = gr.rows(ref, some, n_new, (next, start), None, 0.0, 0.0, sampler)
        assert under[0][0] != fresh[0][0] and under[1][0] == want
        # start -1: the unguided rows
        assert under[1][0][2] == fresh[1][0][2] and under[0][0][2] == fresh[0][0][2]
        assert others(t) == plain
        t.batch_reset_kv()
        t.batch_prefix_set(prefix)
        assert loops(t) == under
        # 6 start states, 5 requests: refused before anything runs, whichever form holds
        caches = slot_rows(t, 4)
        for loop, smp, stop in calls:
            with pytest.raises(IndexError, match="6 start states"):
                run_loop(t, loop, some[:5], n_new[:5], None if smp is None else (smp[0][:5], smp[1], smp[2][:5]), stop)
        assert slot_rows(t, 4) == caches and t.get_guide_sparse()[4] == start
        # a guide over another vocabulary and a refused guide change nothing
        with pytest.raises(q3.Q3Error, match="allows no token"):
            t.set_guide_sparse([-1], [0, 0], [], [], [0])
        assert t.get_guide_sparse()[4] == start and run_loop(t, "sampled", some, n_new, sampler) == want
        # off: the caches start as a fresh engine's do
        t.set_guide(*NO_GUIDE)
        assert t.get_guide_sparse() == NO_SPARSE
        t.batch_reset_kv()
        t.batch_prefix_set(prefix)
        got = loops(t)
        assert [g[0] for g in got] == [w[0] for w in fresh], "other tokens than on an engine that never saw a guide"
        assert [g[1] for g in got] == [w[1] for w in fresh], "other cache rows than on an engine that never saw a guide"


def test_each_form_replaces_the_other_and_the_guide_survives(q3, model):
    path, V, prompts, prefix, ref = model
    few, n_new = prompts[:3], [4, 5, 3]
    next, start = two_state_guide(ref, few, n_new, None, (), V, 42)
    other = np.ascontiguousarray(next[::-1])                                  # the two states swapped: another guide
    other = np.where(other >= 0, 1 - other, -1).astype(np.int16)
    arrays, other_arrays = sparse_of(next), sparse_of(other, True)
    want, other_want, free = gr.rows(ref, few, n_new, (next, start)), gr.rows(ref, few, n_new, (other, start)), gr.rows(ref, few, n_new)
    assert len({str(want), str(other_want), str(free)}) == 3
    with q3.TransformerBuilder(path).with_ctx_length(CTX).build() as t:
        assert t.get_guide() == NO_GUIDE and t.get_guide_sparse() == NO_SPARSE
        t.set_guide_sparse(*arrays, start)                                    # no batched state yet: the first generate call makes the device side
        t.batch_init(4, CTX)
        assert run_loop(t, "greedy", few, n_new, None) == want
        # sparse, then dense: the dense one holds and the sparse getter reads nothing
        t.set_guide(other, start)
        assert t.get_guide()[1] == start and t.get_guide_sparse() == NO_SPARSE
        assert run_loop(t, "greedy", few, n_new, None) == other_want
        # dense, then sparse
        t.set_guide_sparse(*arrays, start)
        assert t.get_guide() == NO_GUIDE and t.get_guide_sparse()[4] == start
        assert run_loop(t, "greedy", few, n_new, None) == want
        # the other setters and a new batched state
        t.set_sampler(0.7, 0.9, 3)
        t.set_sampler(0.0, 0.9, 3)
        t.set_top_k(7)
        t.set_gen_logprobs(3)
        t.set_penalties(1.0, 0.0)
        t.set_penalties(0.0, 0.0)
        t.set_logit_bias([[(1, 0.5, 0)]])
        t.set_logit_bias([])
        t.set_gen_logprobs(-1)
        t.set_top_k(0)
        t.batch_init(4, CTX)                                                  # a new batched state: the arrays go up again
        assert t.get_guide_sparse()[4] == start
        assert run_loop(t, "greedy", few, n_new, None) == want
        assert run_loop(t, "greedy", few, n_new, None) == want                # and stay there for the next call
        # two sparse guides, the same plans: one start state for every request, any number of requests
        t.set_guide_sparse(*other_arrays, [1])
        assert run_loop(t, "greedy", prompts[:5], N_NEW[:5], None) == gr.rows(ref, prompts[:5], N_NEW[:5], (other, [1]))
        t.set_guide_sparse(*arrays, start)
        assert run_loop(t, "greedy", few, n_new, None) == want
        # clearing through either setter clears both
        t.set_guide_sparse(None, None, None, None, [])
        assert t.get_guide() == NO_GUIDE and t.get_guide_sparse() == NO_SPARSE and run_loop(t, "greedy", few, n_new, None) == free
        t.set_guide_sparse(*arrays, start)
        t.set_guide(*NO_GUIDE)
        assert t.get_guide() == NO_GUIDE and t.get_guide_sparse() == NO_SPARSE and run_loop(t, "greedy", few, n_new, None) == free


# ---------------------------------------------------------------------------------------------------------------------
# generate_many(regex=...)
# ---------------------------------------------------------------------------------------------------------------------
def made_up_vocab(V, eos):
    """token bytes for the small synthetic checkpoint: single bytes, some tokens of several bytes (among them halves of a code point
    and digits in pairs), empty tokens for the rest, and eos"""
    vocab = [b""] * V
    pool = [bytes([b]) for b in list(range(0x20, 0x7f)) + [0x0a, 0xc3, 0xa9, 0xe6, 0x97, 0xa5]]
    pool += [b"12", b"2024", b"-0", b"ab", b"abc", b" x", "é".encode(), "日".encode(), "日".encode()[:2], b"7\xc3", b"\xa9-", b"id_", b"A1", b"__"]
    at = np.random.default_rng(7).permutation(V - 1)[:len(pool)]
    for i, b in zip(at, pool):
        vocab[int(i) if int(i) != eos else V - 1] = b
    vocab[eos] = b"<eos>"
    return vocab


REGEXES = [r"\d{4}-\d{2}", r"[a-c]+_?\d*", r"(ab|é)+x", r"[^a-z ]{2,5}", r"id_\w{1,3}|A1"]


@pytest.mark.parametrize("pattern", REGEXES)
def test_generate_many_regex(q3, model, pattern):
    path, V, prompts, prefix, ref = model
    eos = 0
    vocab = made_up_vocab(V, eos)
    tok = type("Tok", (), {"vocab": vocab})()
    some, n_new = prompts[:6], 7
    dfa = q3.regex_dfa(pattern)
    g = q3.SparseAutomaton.from_regex(pattern, vocab, eos)
    assert g.n_states <= 4096
    twin = g.to_dense()                                                       # small enough: the dense twin is the reference's table
    kept = two_state_guide(ref, some, [n_new] * 6, None, (), V, 44)
    with engine(q3, path, slots=4) as t:
        t.set_guide(*kept)
        for kw in ({}, dict(sampler=(0.9, 0.95, list(range(21, 27))))):
            rows = q3.generate_many(t, some, n_new, stop_tokens=[eos], stop_on_device=True, regex=pattern, tokenizer=tok, **kw)[0]
            assert rows == gr.rows(ref, some, [n_new] * 6, (twin.next, [0]), None, 0.0, 0.0, kw.get("sampler"), (), [eos]), kw
            for row in rows:
                data = b"".join(vocab[v] for v in row if v != eos)
                if row[-1] == eos:
                    assert eos not in row[:-1] and re.fullmatch(pattern, data.decode("utf-8"), re.ASCII), (row, data)
                else:
                    # cut at n_new: a prefix the DFA can still complete (regex_dfa keeps no dead state)
                    s = dfa[1]
                    for b in data:
                        s = int(dfa[0][s, b])
                        assert s >= 0, (row, data)
                    assert len(row) == n_new
            # the engine's previous guide is back
            back = t.get_guide()
            assert np.array_equal(back[0], kept[0]) and back[1] == kept[1] and t.get_guide_sparse() == NO_SPARSE
        # the same through guide=, and beside a sparse guide that is kept
        t.set_guide_sparse(*sparse_of(kept[0]), kept[1])
        assert q3.generate_many(t, some, n_new, stop_tokens=[eos], stop_on_device=True, guide=g)[0] == q3.generate_many(
            t, some, n_new, stop_tokens=[eos], stop_on_device=True, guide=[g, twin, g, twin, g, twin])[0]
        assert t.get_guide_sparse()[4] == kept[1] and t.get_guide() == NO_GUIDE
