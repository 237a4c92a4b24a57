"""Log-probabilities of generated tokens inside the five q3_generate_many_* loops (include/qwen3_hip.h section 2o).  The yardstick
is the engine's own q3_score_many / q3_score_top_many on prompt + output (tests/genlp_ref.py), which tests/test_score.py and
tests/test_score_top.py hold to forward() per position; one test goes to forward() directly.  Tokens and cache rows are compared with
the same call under the setting off.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import genlp_ref as gr
import group_cases
import logit_ckpt as lc
import score_top_ref as tr
from test_embed import NAME

pytestmark = pytest.mark.gpu

SLOTS, CTX = 8, 64
LENS = [1, 2, 5, 9, 31, 32, 33, 40, 3, 1, 7]
N_NEW = [1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 6]
TEMPERATURE = [0.8, 0.8, 0.0, 0.8, 0.8, 0.8, 0.8, 0.0, 0.8, 0.8, 0.8]      # two requests at temperature 0
TOPP = 0.9
SEEDS = [0x9E3779B97F4A7C15 + 1000003 * r for r in range(len(LENS))]
SAMPLER = (TEMPERATURE, TOPP, SEEDS)
PREFIX_LEN = 6


@pytest.fixture(scope="module")
def model(q3, tmp_path_factory):
    """(checkpoint path, shape, the 11 prompts, the 6-token prefix) of the small synthetic shape, written once"""
    path = str(tmp_path_factory.mktemp("genlp") / f"{NAME}.bin")
    shape = q3.checkpoint.SHAPES[NAME]
    q3.checkpoint.write_synthetic_checkpoint(path, shape, seed=2468)
    prompts = [[int(x) for x in np.random.default_rng(6100 + r).integers(0, shape.vocab_size, n)] for r, n in enumerate(LENS)]
    prefix = [int(x) for x in np.random.default_rng(6200).integers(0, shape.vocab_size, PREFIX_LEN)]
    return path, shape, prompts, prefix


def engine(q3, path, slots=SLOTS, ctx=CTX, graph=True):
    b = q3.TransformerBuilder(path).with_ctx_length(ctx)
    t = (b if graph else b.with_graph(False)).build()
    t.batch_init(slots, ctx)
    return t


def slot_rows(t, slots):
    return [(t.batch_read_state(s, "key").tobytes(), t.batch_read_state(s, "value").tobytes()) for s in range(slots)]


def run_loop(t, loop, prompts, n_new, sampler, stop=()):
    """(rows cut to n_out, n_out) of one of the five loops through the engine's own methods"""
    if loop == "greedy":
        rows = t.generate_many_greedy(prompts, n_new)[0]
    elif loop == "sampled":
        rows = t.generate_many_sampled(prompts, n_new, *sampler)[0]
    elif loop == "dense":
        rows = t.generate_many_dense(prompts, n_new, sampler, dense_min=8)[0]
    elif loop == "stop":
        rows = t.generate_many_stop(prompts, n_new, stop, sampler)[0]
    else:
        rows = t.generate_many_prefix(prompts, n_new, stop, sampler)[0]
    return [list(r) for r in rows], [len(r) for r in rows]


def greedy_requests(sampler, n):
    return [r for r in range(n) if sampler is None or (sampler[0] if np.isscalar(sampler[0]) else sampler[0][r]) == 0.0]


def check_loop(t, loop, prompts, n_new, sampler, settings, what, stop=(), use_prefix=False, slots=SLOTS):
    """the loop with the setting off, then at every value of `settings`: the same tokens and cache rows, the records of the score
    calls on prompt + output, zero bytes behind n_out, the identities of the greedy requests.  Returns the rows."""
    t.set_gen_logprobs(-1)
    rows, n_out = run_loop(t, loop, prompts, n_new, sampler, stop)
    caches = slot_rows(t, slots)
    got = {}
    for k in settings:
        t.set_gen_logprobs(k)
        assert t.get_gen_logprobs() == k
        again = run_loop(t, loop, prompts, n_new, sampler, stop)
        assert again == (rows, n_out), f"{what}: setting {k}: other tokens than with the setting off"
        assert slot_rows(t, slots) == caches, f"{what}: setting {k}: other cache rows than with the setting off"
        got[k] = (t.read_gen_logprobs(), t.read_gen_logprobs(n_new))
    t.set_gen_logprobs(-1)
    for k, (cut, full) in got.items():
        w = f"{what}: setting {k}"
        gr.assert_same(cut, gr.expected(t, prompts, rows, k, use_prefix=use_prefix), rows, k, w)
        gr.assert_zero_behind(full, n_out, w)
        for r in greedy_requests(sampler, len(prompts)):
            gr.assert_greedy_identities(cut[r][0], cut[r][2] if k else None, rows[r], f"{w}: greedy request {r}")
    return rows


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("loop", ["cols", "dense", "stop", "prefix"])
def test_every_loop_against_the_score_calls(q3, model, loop, sampled):
    """11 requests on 8 slots (slots are reused); passes with no emitting column, passes whose only emitting column is a prompt's last
    behind decode columns, every plan width; the setting at 0 and at 5"""
    path, shape, prompts, prefix = model
    sampler = SAMPLER if sampled else None
    name = {"cols": "sampled" if sampled else "greedy"}.get(loop, loop)
    with engine(q3, path) as t:
        stop = ()
        if loop == "stop":
            # from the loop's own output without stop tokens: request 3 ends on its first token, request 5 on its third
            free = run_loop(t, "sampled" if sampled else "greedy", prompts, N_NEW, sampler)[0]
            stop = [free[3][0], free[5][2]]
        if loop == "prefix":
            t.batch_prefix_set(prefix)
        rows = check_loop(t, name, prompts, N_NEW, sampler, (0, 5), f"{name}{' sampled' if sampled else ''}", stop, use_prefix=loop == "prefix")
        if loop == "stop":
            early = [r for r in range(len(rows)) if len(rows[r]) < N_NEW[r]]
            assert len(early) >= 2 and len(rows[3]) == 1 and 3 in early, (early, [len(r) for r in rows])
        else:
            assert [len(r) for r in rows] == N_NEW


def test_the_prefix_loop_with_stop_tokens_and_the_eager_plans(q3, model):
    """q3_generate_many_prefix through the stop loop, and the loops on an engine without graphs: the launches as they are"""
    path, shape, prompts, prefix = model
    with engine(q3, path) as t:
        t.batch_prefix_set(prefix)
        free = run_loop(t, "prefix", prompts, N_NEW, SAMPLER)[0]
        rows = check_loop(t, "prefix", prompts, N_NEW, SAMPLER, (5,), "prefix with stop tokens", [free[4][1], free[10][0]], use_prefix=True)
        assert len(rows[4]) <= 2 and len(rows[10]) == 1
    with engine(q3, path, graph=False) as t:
        check_loop(t, "sampled", prompts, N_NEW, SAMPLER, (0, 5), "eager, sampled")
        check_loop(t, "greedy", prompts, N_NEW, None, (5,), "eager, greedy")


def test_against_forward_on_a_single_stream_engine(q3, model):
    """one request, a prompt of 4 tokens and 3 new ones: the records from score_ref.record over forward()'s logits, the tops and
    ranks from a host sort of the keys"""
    path, shape, prompts, _ = model
    p = prompts[3][:4]
    k = 7
    with engine(q3, path) as t:
        t.set_gen_logprobs(k)
        rows = t.generate_many_greedy([p], [3])[0]
        got = t.read_gen_logprobs()
        t.set_gen_logprobs(0)
        assert t.generate_many_greedy([p], [3])[0] == rows
        plain = t.read_gen_logprobs()
    with q3.TransformerBuilder(path).with_ctx_length(CTX).build() as t:
        seq = p + list(rows[0])
        logits = [np.array(t.forward(tok, pos), copy=True) for pos, tok in enumerate(seq[:-1])]
    want = gr.from_logits(logits[len(p) - 1:], rows[0], k)
    gr.assert_same(got, [want], rows, k, "against forward()")
    gr.assert_same(plain, [(want[0], None, None)], rows, 0, "against forward(), records alone")
    gr.assert_greedy_identities(got[0][0], got[0][2], rows[0], "against forward()")
    assert plain[0][0].tobytes() == got[0][0].tobytes()


def test_top_k_sampling_stays_inside_the_listed_tokens(q3, model):
    path, shape, prompts, _ = model
    with engine(q3, path) as t:
        t.set_top_k(20)
        rows = check_loop(t, "sampled", prompts, N_NEW, SAMPLER, (20,), "top_k 20")
        t.set_gen_logprobs(20)
        assert run_loop(t, "sampled", prompts, N_NEW, SAMPLER)[0] == rows
        for row, (recs, tops, ranks) in zip(rows, t.read_gen_logprobs()):
            assert (ranks < 20).all() and np.array_equal(tops["index"][np.arange(len(row)), ranks], np.asarray(row, dtype=np.int32))
        t.set_top_k(1)
        rows = run_loop(t, "sampled", prompts, N_NEW, SAMPLER)[0]
        for row, (recs, tops, ranks) in zip(rows, t.read_gen_logprobs()):
            assert not ranks.any() and np.array_equal(recs["argmax"], np.asarray(row, dtype=np.int32))


def test_designed_logits_at_the_full_vocabulary(q3, tmp_path_factory):
    """V = 151,936, logits that depend on the input token alone (token t: design t % 4 of big_c), 2 requests, 2 new tokens, top_n
    64.  twins: tokens 9 and V - 9 tie at the maximum and the tie goes to the higher index, whose design is ramp_up, the ramp that
    underflows to zeros with its maximum at V - 1"""
    V, names = lc.FILES["big_c"]
    assert V == 151936 and (V - 9) % 4 == names.index("ramp_up") and (V - 1) % 4 == names.index("ramp_up")
    path = lc.write(str(tmp_path_factory.mktemp("genlp_designed") / "big_c.bin"), "big_c")
    prompts = [[lc.token_of("big_c", "twins", 3)], [lc.token_of("big_c", "head_far", 1), lc.token_of("big_c", "ramp_up", 5)]]
    k = 64
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(2)
        rows = check_loop(t, "greedy", prompts, [2, 2], None, (k,), "big_c", slots=2)
        assert rows == [[V - 9, V - 1], [V - 1, V - 1]]
        t.set_gen_logprobs(k)
        sampled = check_loop(t, "sampled", prompts, [2, 2], ([1.0, 0.0], 0.4, [7, 8]), (k,), "big_c sampled", slots=2)
        assert sampled[0][0] == 9 and sampled[1] == rows[1]          # a nucleus of one is the LOWER twin: rank 1, not the argmax
        t.set_gen_logprobs(k)
        run_loop(t, "sampled", prompts, [2, 2], ([1.0, 0.0], 0.4, [7, 8]))
        recs, tops, ranks = t.read_gen_logprobs()[0]
        assert ranks[0] == 1 and recs["argmax"][0] == V - 9 and tops["index"][0, :2].tolist() == [V - 9, 9]
        assert recs["target"][0] == recs["max"][0] and tops["index"][0, 2:10].tolist() == list(range(V - 1, V - 9, -1))


@pytest.mark.parametrize("k", [1, 64])
def test_one_and_sixty_four_alternatives(q3, model, k):
    path, shape, prompts, _ = model
    with engine(q3, path) as t:
        check_loop(t, "sampled", prompts, N_NEW, SAMPLER, (k,), f"top_n {k}")


def test_a_group_size_other_than_64(q3, tmp_path):
    name = "g128-hd128"
    shape = group_cases.SHAPES[name]
    path = str(tmp_path / f"{name}.bin")
    q3.checkpoint.write_synthetic_checkpoint(path, shape, seed=group_cases.CKPT_SEED)
    prompts = group_cases.cols_prompts(shape)
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(group_cases.COLS_SLOTS)
        check_loop(t, "greedy", prompts, [group_cases.COLS_NEW] * len(prompts), None, (5,), name, slots=group_cases.COLS_SLOTS)


def test_thirty_two_emitting_columns_and_one_slot(q3, model):
    path, shape, prompts, _ = model
    ones = [[int(x)] for x in np.random.default_rng(6300).integers(0, shape.vocab_size, 32)]
    with engine(q3, path, slots=32) as t:
        check_loop(t, "greedy", ones, [2] * 32, None, (5,), "32 one-token prompts", slots=32)
        check_loop(t, "sampled", ones, [2] * 32, (0.8, TOPP, list(range(1, 33))), (0,), "32 one-token prompts, sampled", slots=32)
    with engine(q3, path, slots=1) as t:
        check_loop(t, "greedy", [prompts[2]], [4], None, (0, 5), "one slot", slots=1)
        check_loop(t, "stop", [prompts[2], prompts[1]], [4, 3], ([0.8, 0.0], TOPP, [5, 6]), (5,), "one slot, stop loop", stop=[0], slots=1)


def test_state(q3, model):
    """read before any call under the setting and past the total are Q3_ERR_ARG; the setting survives batch_init, set_sampler and
    the calls; after set_gen_logprobs(-1) a call gives the tokens it gave before and leaves nothing to read"""
    path, shape, prompts, _ = model
    few, n_new = prompts[:3], [2, 3, 1]
    with q3.TransformerBuilder(path).with_ctx_length(CTX).build() as t:
        lib, h = t._lib, t._h
        buf = np.zeros(64, dtype=q3.SCORE_DTYPE).ctypes.data_as(C.c_void_p)
        top = np.zeros((64, 64), dtype=q3.TOP_DTYPE).ctypes.data_as(C.c_void_p)
        t.set_gen_logprobs(5)                                        # no batched state yet: the first call allocates
        assert lib.q3_gen_logprobs_read(h, 0, 1, buf, top, None) == -3
        t.batch_init(4, CTX)
        assert t.get_gen_logprobs() == 5
        assert lib.q3_gen_logprobs_read(h, 0, 1, buf, top, None) == -3 and b"no records" in lib.q3_last_error()
        t.set_gen_logprobs(-1)
        before = t.generate_many_greedy(few, n_new)[0]
        assert lib.q3_gen_logprobs_read(h, 0, 1, buf, top, None) == -3
        with pytest.raises(IndexError):
            t.read_gen_logprobs()
        t.set_gen_logprobs(5)
        t.set_sampler(0.7, 0.9, 3)
        t.set_sampler(0.0, 0.9, 3)
        t.batch_init(4, CTX)
        assert t.get_gen_logprobs() == 5
        assert t.generate_many_greedy(few, n_new)[0] == before
        total = sum(n_new)
        assert lib.q3_gen_logprobs_read(h, 0, total, buf, top, None) == 0
        assert lib.q3_gen_logprobs_read(h, total, 0, buf, top, None) == 0
        for first, count, b_, t_ in ((0, total + 1, buf, top), (total, 1, buf, top), (2 ** 63, 2 ** 63, buf, top), (0, 1, None, top), (0, 1, buf, None)):
            assert lib.q3_gen_logprobs_read(h, first, count, b_, t_, None) == -3, (first, count)
        for bad in (-2, 65):
            assert lib.q3_gen_logprobs(h, bad) == -3 and t.get_gen_logprobs() == 5
        got = t.read_gen_logprobs()
        gr.assert_same(got, gr.expected(t, few, before, 5), before, 5, "behind the refused calls")
        # a failed generate call leaves nothing to read
        with pytest.raises(IndexError):
            t.generate_many_greedy([[shape.vocab_size]], [1])
        assert lib.q3_gen_logprobs_read(h, 0, 1, buf, top, None) == -3
        assert t.generate_many_greedy(few, n_new)[0] == before
        t.set_gen_logprobs(-1)
        assert t.generate_many_greedy(few, n_new)[0] == before
        assert lib.q3_gen_logprobs_read(h, 0, 1, buf, top, None) == -3
        # batch_step_cols forms no record under the setting
        t.set_gen_logprobs(0)
        t.generate_many_greedy(few, n_new)
        kept = [x[0].tobytes() for x in t.read_gen_logprobs()]
        t.batch_step_cols([0, 1], [3, 4], [0, 0])
        assert [x[0].tobytes() for x in t.read_gen_logprobs()] == kept


def test_a_sequence_of_calls_on_one_engine(q3, model):
    """plain stop call, logprobs call, score_many, embed_many, plain stop call, logprobs call with another top_n"""
    path, shape, prompts, _ = model
    some = prompts[:6]
    n_new = N_NEW[:6]
    with engine(q3, path, slots=4) as t:
        fresh = [r.tobytes() for r in t.score_many(some)[0]]
    with engine(q3, path, slots=4) as t:
        free = t.generate_many_greedy(some, n_new)[0]
        stop = [free[5][2]]
        a = run_loop(t, "stop", some, n_new, None, stop)
        t.set_gen_logprobs(3)
        b = run_loop(t, "stop", some, n_new, None, stop)
        first = t.read_gen_logprobs()
        assert [r.tobytes() for r in t.score_many(some)[0]] == fresh
        again = t.read_gen_logprobs()                               # the earlier call's records stand behind score_many
        for x, y in zip(first, again):
            assert all(u.tobytes() == v.tobytes() for u, v in zip(x, y))
        t.embed_many(some)
        t.set_gen_logprobs(-1)
        c = run_loop(t, "stop", some, n_new, None, stop)
        t.set_gen_logprobs(64)
        d = run_loop(t, "stop", some, n_new, None, stop)
        second = t.read_gen_logprobs()
        assert a == b == c == d and a[0][5] == free[5][:free[5].index(stop[0]) + 1] and len(a[0][5]) <= 3
        for x, y in zip(first, second):
            assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == np.ascontiguousarray(y[1][:, :3]).tobytes() and np.array_equal(x[2], y[2])
        gr.assert_same(second, gr.expected(t, some, a[0], 64), a[0], 64, "the second logprobs call")


def test_score_top_calls_between_loops_with_records(q3, model):
    """The exps, the part lists and the part counts are one scratch for the score calls and the loops: greedy loop at 64,
    score_top_many with k = 5 (and the loop's records read again), sampled loop at 3, score_top_many with k = 64, score_many, greedy
    loop at 5, all on one engine.  Every result -- tokens, records, tops, ranks -- is, byte for byte, that of the same call made
    first on a fresh engine."""
    path, shape, prompts, _ = model
    some, n_new = prompts[:6], N_NEW[:6]
    sampler = (TEMPERATURE[:6], TOPP, SEEDS[:6])

    def raw(arrays):
        return [None if a is None else a.tobytes() for a in arrays]

    def records(t):
        return [raw(per_request) for per_request in t.read_gen_logprobs()]

    def loop(name, k, smp):
        def call(t):
            t.set_gen_logprobs(k)
            rows = run_loop(t, name, some, n_new, smp)
            return rows, records(t)
        return call

    def score(k):
        def call(t):
            if k:
                recs, tops, ranks, _ = t.score_top_many(some, k)
            else:
                recs, tops, ranks = t.score_many(some)[0], None, None
            return [raw(x) for x in (recs, tops or [], ranks or [])]
        return call

    steps = [("greedy loop at 64", loop("greedy", 64, None)), ("score_top_many, k 5", score(5)), ("sampled loop at 3", loop("sampled", 3, sampler)),
             ("score_top_many, k 64", score(64)), ("score_many", score(0)), ("greedy loop at 5", loop("greedy", 5, None))]
    want = []
    for _, call in steps:
        with engine(q3, path, slots=4) as t:
            want.append(call(t))
    with engine(q3, path, slots=4) as t:
        for i, ((what, call), w) in enumerate(zip(steps, want)):
            assert call(t) == w, f"{what}: other bytes than on a fresh engine"
            if i == 0:
                first = records(t)
            if i == 1:
                assert records(t) == first == want[0][1], "the loop's records behind score_top_many"


def test_generate_many_with_logprobs(q3, model):
    """generation.generate_many(logprobs=) over every option combination: the rows of the call without it, the tuples of
    top_logprobs() on prompt + row, the engine's setting put back"""
    path, shape, prompts, prefix = model
    some = prompts[:6]
    with engine(q3, path, slots=4) as t:
        t.set_gen_logprobs(2)
        free = q3.generate_many(t, some, 5)[0]
        stop = [free[4][2]]
        for kw in ({}, dict(sampler=(0.8, TOPP, SEEDS[:6])), dict(dense_min=8), dict(stop_tokens=stop), dict(stop_tokens=stop, stop_on_device=True),
                   dict(shared_prefix=prefix, sampler=(0.8, TOPP, SEEDS[:6]))):
            plain = q3.generate_many(t, some, 5, **kw)
            for k in (0, 4):
                rows, stats, lps = q3.generate_many(t, some, 5, logprobs=k, **kw)
                assert (rows, stats) == plain and t.get_gen_logprobs() == 2, kw
                full = [list(kw.get("shared_prefix", [])) + p + r for p, r in zip(some, rows)]
                sf = [len(f) - len(r) for f, r in zip(full, rows)]
                want = q3.top_logprobs(t, full, max(k, 1), sf)
                for r, (g, w) in enumerate(zip(lps, want)):
                    assert np.array_equal(g[0], w[0]) and g[0].dtype == np.float64, (kw, k, r)
                    if k:
                        assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(g, w)), (kw, k, r)
                    else:
                        assert g[1].shape == g[2].shape == (len(rows[r]), 0) and g[3].size == 0
            if "stop_tokens" in kw:
                cut = free[4].index(stop[0]) + 1             # the row ends with the first stop token, its tuple with it
                assert rows[4] == free[4][:cut] and cut <= 3 and lps[4][0].size == cut
