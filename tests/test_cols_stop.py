"""Stop tokens in the device loop (include/qwen3_hip.h section 2h): q3_generate_many_stop.  A request that ends at its first stop
token is a request with n_new = n_emit, so the yardstick is the existing loop -- generate_many_greedy / generate_many_sampled --
called at the cap for the tokens and with n_new = n_emit for the passes, and nothing here has a tolerance.

The synthetic checkpoints emit no EOS of their own: cols_stop_cases.pick_stops chooses a stop set from the rows at the cap and the
tests assert that it ends requests at y_0, inside their rows and not at all.  Checked with the CPU oracle for the checkpoint seed
and prompts used here: tiny-g64 greedy picks [187] (n_emit 1, 10, 10, 10, 8, 10, 10), sampled [82] (10, 10, 10, 1, 4, 10, 10);
small-hd128 greedy [11, 80] (10, 10, 1, 10, 4, 10, 10), sampled [3, 834] (10, 1, 4, 10, 10, 10, 10); 9 passes saved in each."""
import ctypes as C

import pytest

import cols_sim
from cols_stop_cases import (CAP, CKPT_SEED, PROMPT_LEN, SEEDS, SHAPES, SLOTS, STOP_MAX, TEMPERATURE, TOPP, kinds, n_emit_of, passes_saved,
                             pick_stops, prompts)
from conftest import assert_biteq

pytestmark = pytest.mark.gpu

SAMPLER = (list(TEMPERATURE), TOPP, list(SEEDS))
N = len(PROMPT_LEN)


class Model:
    """One synthetic checkpoint, its requests and what the existing loops make of them at the cap: computed once, never changed."""

    def __init__(self, q3, name, path):
        self.q3, self.name, self.path, self.ctx = q3, name, path, SHAPES[name]
        self.shape = q3.checkpoint.SHAPES[name]
        q3.checkpoint.write_synthetic_checkpoint(path, self.shape, seed=CKPT_SEED)
        self.prompts = prompts(self.shape.vocab_size)
        self._at_cap = {}

    def engine(self, fast=False):
        b = self.q3.TransformerBuilder(self.path).with_ctx_length(self.ctx or None)
        if fast:
            b = b.with_strict(False)
        return b.build()

    def batch_engine(self, slots=SLOTS):
        t = self.engine()
        t.batch_init(slots)
        return t

    def at_cap(self, sampled):
        """(rows of the existing loop at the cap, the stop set picked from them, n_emit)"""
        if sampled not in self._at_cap:
            with self.batch_engine() as t:
                rows, stats = (t.generate_many_sampled(self.prompts, [CAP] * N, *SAMPLER) if sampled
                               else t.generate_many_greedy(self.prompts, [CAP] * N))
            assert stats.passes == cols_sim.schedule(PROMPT_LEN, [CAP] * N, SLOTS)[1].passes
            stop = pick_stops(rows)
            assert stop is not None and len(stop) <= STOP_MAX, f"no stop set ends the rows in every way: {rows}"
            at_y0, inside, never = kinds(rows, stop)
            assert at_y0 >= 1 and inside >= 1 and never >= 1 and passes_saved(rows, stop) >= 1
            self._at_cap[sampled] = (rows, stop, n_emit_of(rows, stop))
        return self._at_cap[sampled]


@pytest.fixture(scope="module")
def models(q3, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Model(q3, name, str(tmp_path_factory.mktemp("colsstop") / f"{name}.bin"))
        return made[name]
    return get


def tup(stats):
    return (stats.passes, stats.live_columns, stats.prompt_columns, stats.decode_columns)


def check_stop_call(t, m, stop, sampler, rows, emit, what):
    """one generate_many_stop call against the rows at the cap: tokens up to the cut, n_out, -1 behind, and returns the stats"""
    out, n_out, stats = t.generate_many_stop(m.prompts, [CAP] * N, stop, sampler, raw=True)
    assert n_out == emit, what
    for r in range(N):
        got = out[r * CAP:(r + 1) * CAP]
        assert got[:emit[r]] == rows[r][:emit[r]], f"{what}: request {r}"
        assert got[emit[r]:] == [-1] * (CAP - emit[r]), f"{what}: request {r} behind its last token"
    return stats


@pytest.mark.parametrize("name", list(SHAPES))
def test_greedy_equals_the_loop_with_n_emit(q3, models, name):
    m = models(name)
    rows, stop, emit = m.at_cap(False)
    _, wstats = cols_sim.schedule(PROMPT_LEN, emit, SLOTS)
    with m.batch_engine() as t:
        for k in range(2):                                   # the second call finds the slots and the plans as the first left them
            stats = check_stop_call(t, m, stop, None, rows, emit, f"call {k}")
            assert tup(stats) == tuple(wstats)
        want, lstats = t.generate_many_greedy(m.prompts, emit)
        assert want == [r[:e] for r, e in zip(rows, emit)]
        assert tup(lstats) == tuple(wstats)
        cut, cstats = t.generate_many_stop(m.prompts, [CAP] * N, stop)
        assert cut == want and tup(cstats) == tuple(wstats)


@pytest.mark.parametrize("name", ["tiny-g64", "small-hd128"])
def test_under_samplers(q3, models, name):
    """greedy and sampled requests share passes; a request that stops draws no coin behind its stop token, and the next occupant
    of its slot draws from its own seed"""
    m = models(name)
    rows, stop, emit = m.at_cap(True)
    _, wstats = cols_sim.schedule(PROMPT_LEN, emit, SLOTS)
    with m.batch_engine() as t:
        for k in range(2):
            stats = check_stop_call(t, m, stop, SAMPLER, rows, emit, f"call {k}")
            assert tup(stats) == tuple(wstats)
        want, lstats = t.generate_many_sampled(m.prompts, emit, *SAMPLER)
        assert want == [r[:e] for r, e in zip(rows, emit)]
        assert tup(lstats) == tuple(wstats)
        # the greedy stop set on the same engine: the two sets of plans take turns
        grows, gstop, gemit = m.at_cap(False)
        check_stop_call(t, m, gstop, None, grows, gemit, "greedy behind sampled")
        check_stop_call(t, m, stop, SAMPLER, rows, emit, "sampled behind greedy")


@pytest.mark.parametrize("name", ["tiny-g64", "small-hd128"])
def test_cache_rows_of_the_last_occupants(q3, models, name):
    m = models(name)
    rows, stop, emit = m.at_cap(False)
    table, _ = cols_sim.schedule(PROMPT_LEN, emit, SLOTS)
    last = {}
    for _, slot, _, req in table:
        last[slot] = req
    assert sorted(last) == list(range(SLOTS))
    with m.batch_engine() as t, m.engine() as ref:
        check_stop_call(t, m, stop, None, rows, emit, "stop call")
        c = t.get_config()
        kvd = c.n_kv_heads * c.head_dim
        for slot, r in last.items():
            ref.reset_kv()
            y0 = ref.prefill(m.prompts[r], 0)
            if emit[r] > 1:
                ref.generate_greedy(y0, PROMPT_LEN[r], emit[r] - 1)
            n = PROMPT_LEN[r] + emit[r] - 1                  # rows 0 .. prompt_len + n_emit - 2
            for kind in ("key", "value"):
                got = t.batch_read_state(slot, kind).reshape(c.n_layers, t._batch_ctx, kvd)[:, :n]
                want = ref.read_state(kind).reshape(c.n_layers, c.seq_len, kvd)[:, :n]
                assert_biteq(got, want, f"slot {slot}, request {r}: {kind} rows")


@pytest.mark.parametrize("name", ["tiny-g64", "small-hd128"])
def test_no_stop_list_and_all_at_y0(q3, models, name):
    m = models(name)
    rows, _, _ = m.at_cap(False)
    with m.batch_engine() as t:
        stats = check_stop_call(t, m, [], None, rows, [CAP] * N, "n_stop 0")
        assert tup(stats) == tuple(cols_sim.schedule(PROMPT_LEN, [CAP] * N, SLOTS)[1])
        y0 = sorted({r[0] for r in rows})
        assert len(y0) <= STOP_MAX
        stats = check_stop_call(t, m, y0, None, rows, [1] * N, "every request stops at y_0")
        assert tup(stats) == tuple(cols_sim.schedule(PROMPT_LEN, [1] * N, SLOTS)[1])
        # a stop token at index n_new - 1: the request ends there either way
        n_new = [3] * N
        out, n_out, stats = t.generate_many_stop(m.prompts, n_new, [rows[4][2]], None, raw=True)
        want = n_emit_of([r[:3] for r in rows], [rows[4][2]])
        assert n_out == want and want[4] == 3
        assert tup(stats) == tuple(cols_sim.schedule(PROMPT_LEN, want, SLOTS)[1])


@pytest.mark.parametrize("stop_first", [False, True])
@pytest.mark.parametrize("name", ["tiny-g64", "small-hd128"])
def test_kept_plans_survive(q3, models, name, stop_first):
    m = models(name)
    rows, stop, emit = m.at_cap(False)
    toks = [p[0] for p in m.prompts[:SLOTS]]

    def others(t):
        many = t.generate_many_greedy(m.prompts, [4] * N)
        lg, am = t.batch_step_cols([2, 0, 0], [toks[2], toks[0], toks[1]], [0, 0, 1], want_logits=True)
        flg, fam = t.forward_batch(toks, [0] * SLOTS)
        return many, lg, am, flg, fam

    def same(a, b, what):
        assert a[0] == b[0] and a[2] == b[2] and a[4] == b[4], what
        assert_biteq(a[1], b[1], f"{what}: batch_step_cols logits")
        assert_biteq(a[3], b[3], f"{what}: forward_batch logits")

    with m.batch_engine() as t:
        if stop_first:
            check_stop_call(t, m, stop, None, rows, emit, "stop call on a fresh engine")
            before = others(t)
            assert before[0][0] == [r[:4] for r in rows]
            check_stop_call(t, m, stop, None, rows, emit, "stop call behind the others")
            same(others(t), before, "behind a stop call")
        else:
            before = others(t)
            assert before[0][0] == [r[:4] for r in rows]
            check_stop_call(t, m, stop, None, rows, emit, "stop call")
            same(others(t), before, "behind a stop call")
            srows, sstop, semit = m.at_cap(True)
            check_stop_call(t, m, sstop, SAMPLER, srows, semit, "sampled stop call")
            same(others(t), before, "behind a sampled stop call")


def test_errors(q3, models):
    m = models("tiny-g64")
    V = m.shape.vocab_size
    P = [[1, 2, 3], [4]]
    with m.engine() as t:
        with pytest.raises(IndexError, match="q3_batch_init"):
            t.generate_many_stop(P, [2, 2], [5])
        t.batch_init(2, 40)
        assert all(1 <= len(r) <= 2 for r in t.generate_many_stop(P, [2, 2], list(range(V - 8, V)))[0])     # 8 stop tokens: accepted
        with pytest.raises(IndexError, match="stop tokens"):
            t.generate_many_stop(P, [2, 2], list(range(9)))
        with pytest.raises(IndexError, match="stop token"):
            t.generate_many_stop(P, [2, 2], [V])
        with pytest.raises(IndexError):
            t.generate_many_stop(P, [2, 2], [-1])
        for prompts_, n_new in [([[]], [1]), ([[1, 2]], [0]), ([[1] * 30], [12]), ([[1, V]], [1])]:     # what generate_many_greedy rejects
            with pytest.raises(IndexError):
                t.generate_many_stop(prompts_, n_new, [5])
        for sampler in [(-0.5, 0.9, 1), (0.8, 1.5, 1), (float("nan"), 0.9, 1)]:                         # what generate_many_sampled rejects
            with pytest.raises(IndexError):
                t.generate_many_stop(P, [2, 2], [5], sampler)
        L = q3.load_library()
        i32, sz = C.c_int32, C.c_size_t
        out, n_out = (i32 * 4)(), (sz * 2)()
        args = (t._h, (i32 * 4)(1, 2, 3, 4), (sz * 2)(3, 1), (sz * 2)(2, 2), 2, None, None, None)
        assert L.q3_generate_many_stop(*args, None, 1, out, n_out, None) == -3                           # null stop_tokens with n_stop > 0
        assert L.q3_generate_many_stop(*args, (i32 * 1)(5), 1, out, None, None) == -3                    # null n_out
        assert L.q3_generate_many_stop(*args[:5], (C.c_float * 2)(0.5, 0.5), None, None, (i32 * 1)(5), 1, out, n_out, None) == -3
        assert L.q3_generate_many_stop(*args, None, 0, out, n_out, None) == 0 and list(n_out) == [2, 2]  # no stop list at all
        t.set_batch_sampler(0.8, 0.9, [1, 2])
        with pytest.raises(q3.Q3Error) as ei:                # greedy call under a sampling batch, as generate_many_greedy
            t.generate_many_stop(P, [2, 2], [5])
        assert ei.value.code == -5
    with m.engine(fast=True) as t:
        t.batch_init(2)
        with pytest.raises(q3.Q3Error) as ei:
            t.generate_many_stop(P, [2, 2], [5])
        assert ei.value.code == -5 and "Q3_FLAG_FAST" in ei.value.msg


@pytest.mark.parametrize("name", ["tiny-g64", "small-hd128"])
def test_generate_many_front_end(q3, models, name):
    m = models(name)
    with m.batch_engine() as t:
        for sampled in (False, True):
            rows, stop, emit = m.at_cap(sampled)
            sampler = SAMPLER if sampled else None
            want, wstats = q3.generate_many(t, m.prompts, CAP, stop_tokens=stop, sampler=sampler)
            got, stats = q3.generate_many(t, m.prompts, CAP, stop_tokens=stop, sampler=sampler, stop_on_device=True)
            assert got == want == [r[:e] for r, e in zip(rows, emit)]
            assert stats.passes == cols_sim.schedule(PROMPT_LEN, emit, SLOTS)[1].passes < wstats.passes
        none, nstats = q3.generate_many(t, m.prompts, CAP, stop_on_device=True)          # no stop token: today's path
        assert none == m.at_cap(False)[0] and nstats.passes == cols_sim.schedule(PROMPT_LEN, [CAP] * N, SLOTS)[1].passes
        with pytest.raises(ValueError):
            q3.generate_many(t, m.prompts, CAP, stop_tokens=m.at_cap(False)[1], stop_on_device=True, dense_min=8)
