"""Column passes under the sampler (include/qwen3_hip.h section 2f): q3_batch_step_cols_draw and q3_generate_many_sampled.
The yardstick is always a second single-stream engine of the same context seeded like the slot or the request -- set_sampler, then
forward_sample, or prefill + generate_greedy (q3_generate_sampled) -- and every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from cols_draw_cases import CKPT_SEED, GREEDY, N_NEW, PROMPT_LEN, SAMPLERS, SEEDS, SHAPES, SLOT_COUNTS, prompts, request_seeds, sampler_id
from conftest import assert_biteq

pytestmark = pytest.mark.gpu

N_HIST = 64


class Model:
    """One synthetic checkpoint and its single-stream references, computed once and never changed."""

    def __init__(self, q3, name, path):
        self.q3, self.name, self.path, self.ctx = q3, name, path, SHAPES[name]
        self.shape = q3.checkpoint.SHAPES[name]
        q3.checkpoint.write_synthetic_checkpoint(path, self.shape, seed=CKPT_SEED)
        self.prompts = prompts(self.shape.vocab_size)
        self._refs = {}
        self._single = None

    def single(self):
        """the single-stream engine every reference comes from: re-seeded and its cache zeroed for each of them"""
        if self._single is None:
            self._single = self.engine()
        self._single.reset_kv()
        return self._single

    def close(self):
        if self._single is not None:
            self._single.close()
            self._single = None

    def engine(self, fast=False, graph=True):
        b = self.q3.TransformerBuilder(self.path).with_ctx_length(self.ctx or None).with_graph(graph)
        if fast:
            b = b.with_strict(False)
        return b.build()

    def history(self, seed, n=N_HIST):
        return [int(t) for t in np.random.default_rng(seed).integers(0, self.shape.vocab_size, n)]

    def _rows(self, t, n):
        c = t.get_config()
        kvd, S = c.n_kv_heads * c.head_dim, c.seq_len
        return (t.read_state("key").reshape(c.n_layers, S, kvd)[:, :n].copy(), t.read_state("value").reshape(c.n_layers, S, kvd)[:, :n].copy())

    def walk(self, hist_seed, T, p, seed):
        """history(hist_seed) at positions 0 .. N_HIST - 1 through forward_sample on a fresh engine seeded (T, p, seed):
        (tokens, draw of every position, key rows, value rows)"""
        k = ("walk", hist_seed, T, p, seed)
        if k not in self._refs:
            toks = self.history(hist_seed)
            t = self.single()
            t.set_sampler(T, p, seed)
            draws = [t.forward_sample(tok, pos) for pos, tok in enumerate(toks)]
            self._refs[k] = (toks, draws) + self._rows(t, N_HIST)
        return self._refs[k]

    def request(self, r, T, p, seed):
        """request r under (T, p, seed) on an engine of its own: (row, key rows, value rows of the positions it wrote)"""
        k = ("req", r, T, p, seed if T > 0 else 0)
        if k not in self._refs:
            P, n = self.prompts[r], N_NEW[r]
            t = self.single()
            t.set_sampler(T, p, seed)
            y0 = t.prefill(P, 0)
            row = [y0] + (t.generate_greedy(y0, len(P), n - 1) if n > 1 else [])
            self._refs[k] = (row,) + self._rows(t, len(P) + n - 1)
        return self._refs[k]


@pytest.fixture(scope="module")
def models(q3, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Model(q3, name, str(tmp_path_factory.mktemp("colsdraw") / f"{name}.bin"))
        return made[name]
    yield get
    for m in made.values():
        m.close()


def slot_rows(t, slot, n):
    c = t.get_config()
    kvd = c.n_kv_heads * c.head_dim
    return (t.batch_read_state(slot, "key").reshape(c.n_layers, t._batch_ctx, kvd)[:, :n],
            t.batch_read_state(slot, "value").reshape(c.n_layers, t._batch_ctx, kvd)[:, :n])


def check_rows(t, slot, want_k, want_v, n, what):
    k, v = slot_rows(t, slot, n)
    assert_biteq(k, want_k[:, :n], f"{what}: key rows")
    assert_biteq(v, want_v[:, :n], f"{what}: value rows")


@pytest.mark.parametrize("sampler", SAMPLERS, ids=sampler_id)
@pytest.mark.parametrize("name", list(SHAPES))
def test_identity_slots_equal_forward_batch(q3, models, name, sampler):
    """one column per slot, slot i = stream i: the tokens, logits, caches and rng streams of forward_batch under set_batch_sampler --
    all passes through step_cols_draw (engine b), and the two entry points taking turns on one engine (engine c)"""
    m = models(name)
    T, p = sampler
    n, steps = 5, 6
    toks = [m.history(100 + i, steps) for i in range(n)]
    seeds = [SEEDS[i % 2] + i for i in range(n)]
    with m.engine() as a, m.engine() as b, m.engine() as c:
        for t in (a, b, c):
            t.batch_init(n)
            t.set_batch_sampler(T, p, seeds)
        for k in range(steps):
            col, pos = [toks[i][k] for i in range(n)], [k] * n
            want, wdraw = a.forward_batch(col, pos)
            got, gdraw = b.batch_step_cols_draw(list(range(n)), col, pos, want_logits=True)
            assert_biteq(got, want, f"step {k}: logits")
            assert gdraw == wdraw, f"step {k}: draws"
            alt, adraw = c.batch_step_cols_draw(list(range(n)), col, pos, want_logits=True) if k % 2 else c.forward_batch(col, pos)
            assert_biteq(alt, want, f"step {k}: logits, entry points taking turns")
            assert adraw == wdraw, f"step {k}: draws, entry points taking turns"
        assert any(wdraw[i] != q3.sample_argmax(want[i]) for i in range(n)), "every draw is the argmax: the case shows nothing"
        for i in range(n):
            for t in (b, c):
                assert_biteq(t.batch_read_state(i, "key"), a.batch_read_state(i, "key"), f"slot {i} key")
                assert_biteq(t.batch_read_state(i, "value"), a.batch_read_state(i, "value"), f"slot {i} value")


@pytest.mark.parametrize("sampler", SAMPLERS, ids=sampler_id)
@pytest.mark.parametrize("name", list(SHAPES))
def test_runs_walk_a_slot(q3, models, name, sampler):
    """slot 1 walked in runs of 1, 2, 5, 16, 32 and 8 columns: kept draw j is the j-th forward_sample of an engine seeded like the
    slot; a column with keep 0 returns -1 and still takes its coin, so the draws behind it are the reference's"""
    m = models(name)
    T, p = sampler
    toks, draws, rk, rv = m.walk(300, T, p, SEEDS[1])
    keep = [0 if j % 3 == 1 else 1 for j in range(N_HIST)]
    with m.engine() as t:
        t.batch_init(2)
        t.set_batch_sampler(T, p, [SEEDS[0], SEEDS[1]])
        got, at = [], 0
        for c in [1, 2, 5, 16, 32, 8]:
            got += t.batch_step_cols_draw([1] * c, toks[at:at + c], list(range(at, at + c)), keep=keep[at:at + c])
            at += c
        assert got == [d if k else -1 for d, k in zip(draws, keep)]
        check_rows(t, 1, rk, rv, N_HIST, "slot 1")
        assert not t.batch_read_state(0, "key").any()
        # slot 0's stream has not moved: its first draw is the first draw of an engine seeded like it
        toks0, draws0, _, _ = m.walk(301, T, p, SEEDS[0])
        assert t.batch_step_cols_draw([0], toks0[:1], [0]) == draws0[:1]


@pytest.mark.parametrize("width", [3, 11, 32])
@pytest.mark.parametrize("name", list(SHAPES))
def test_mixed_pass(q3, models, name, width):
    """a decode column of slot 2, a prompt run of slot 0 and a decode column of slot 1 in one pass (plan widths 4, 16 and 32: with and
    without pads), only the run's last column and the decode columns kept; then one more column per slot: every rng moved on by
    its run's length"""
    m = models(name)
    T, p = SAMPLERS[{3: 0, 11: 1, 32: 2}[width]]
    seeds = [SEEDS[0], SEEDS[1], SEEDS[0] + 7]
    w0, w1, w2 = m.walk(400, T, p, seeds[0]), m.walk(401, T, p, seeds[1]), m.walk(402, T, p, seeds[2])
    run = width - 2
    with m.engine() as t:
        t.batch_init(3)
        t.set_batch_sampler(T, p, seeds)
        for at, c in ((0, 32), (32, 8)):                     # slot 1: 40 positions of history, every coin taken and dropped
            assert t.batch_step_cols_draw([1] * c, w1[0][at:at + c], list(range(at, at + c)), keep=[0] * c) == [-1] * c
        assert t.batch_step_cols_draw([2] * 5, w2[0][:5], list(range(5))) == w2[1][:5]
        slots = [2] + [0] * run + [1]
        toks = [w2[0][5]] + w0[0][:run] + [w1[0][40]]
        pos = [5] + list(range(run)) + [40]
        keep = [1] + [0] * (run - 1) + [1, 1]
        lg, got = t.batch_step_cols_draw(slots, toks, pos, keep=keep, want_logits=True)
        assert got == [w2[1][5]] + [-1] * (run - 1) + [w0[1][run - 1], w1[1][40]]
        s = m.single()                                       # the raw logits of the run's last column
        for q, tok in enumerate(w0[0][:run]):
            ref = np.array(s.forward(tok, q), copy=True)
        assert_biteq(lg[run], ref, "logits of the run's last column")
        assert t.batch_step_cols_draw([1, 0, 2], [w1[0][41], w0[0][run], w2[0][6]], [41, run, 6]) == [w1[1][41], w0[1][run], w2[1][6]]
        check_rows(t, 0, w0[2], w0[3], run + 1, "slot 0")
        check_rows(t, 1, w1[2], w1[3], 42, "slot 1")
        check_rows(t, 2, w2[2], w2[3], 7, "slot 2")


def run_many(t, m, order, temperature, topp, seeds):
    rows, stats = t.generate_many_sampled([m.prompts[r] for r in order], [N_NEW[r] for r in order], [temperature[r] for r in order],
                                          [topp[r] for r in order], [seeds[r] for r in order])
    return {r: rows[i] for i, r in enumerate(order)}, stats


@pytest.mark.parametrize("sampler", SAMPLERS, ids=sampler_id)
@pytest.mark.parametrize("name", list(SHAPES))
def test_generate_many_sampled(q3, models, name, sampler):
    """every request row equals its own engine's, for both seed assignments, 1, 3 and 8 slots and both request orders; the slots
    are never cleared between calls, and with 1 and 3 slots they change hands inside a call"""
    m = models(name)
    T, p = sampler
    R = len(PROMPT_LEN)
    with m.engine() as t:
        for n_slots in SLOT_COUNTS:
            t.batch_init(n_slots)
            for which in (0, 1):
                seeds = request_seeds(which)
                want = {r: m.request(r, T, p, seeds[r])[0] for r in range(R)}
                for order in (list(range(R)), list(range(R))[::-1]):
                    got, stats = run_many(t, m, order, [T] * R, [p] * R, seeds)
                    assert got == want, f"{n_slots} slots, seeds {which}, order {order}"
                    _, wstats = q3.cols_schedule([PROMPT_LEN[r] for r in order], [N_NEW[r] for r in order], n_slots)
                    assert stats == wstats
        # 8 slots, requests in ascending order last: request r finished in slot r
        got, _ = run_many(t, m, list(range(R)), [T] * R, [p] * R, seeds)
        assert got == want
        for r in range(R):
            _, rk, rv = m.request(r, T, p, seeds[r])
            check_rows(t, r, rk, rv, PROMPT_LEN[r] + N_NEW[r] - 1, f"slot of request {r}")


@pytest.mark.parametrize("name", list(SHAPES))
def test_generate_many_mixed_and_greedy(q3, models, name):
    """greedy and sampled requests in one call; all temperatures 0; an engine without graphs; a context that never set a batch sampler"""
    m = models(name)
    T, p = SAMPLERS[1]
    R = len(PROMPT_LEN)
    order = list(range(R))
    seeds = request_seeds(0)
    temps = [T if r % 2 == 0 else 0.0 for r in order]
    topps = [p if r % 2 == 0 else GREEDY[1] for r in order]
    want = {r: m.request(r, temps[r], topps[r], seeds[r])[0] for r in order}
    with m.engine() as t, m.engine(graph=False) as eager:
        for n_slots in (2, 8):
            t.batch_init(n_slots)
            greedy, gstats = t.generate_many_greedy(m.prompts, list(N_NEW))
            got, _ = run_many(t, m, order, temps, topps, seeds)
            assert got == want, f"{n_slots} slots: mixed requests"
            for r in order:
                if temps[r] == 0.0:
                    assert got[r] == greedy[r], f"{n_slots} slots: greedy request {r}"
            zero, zstats = run_many(t, m, order, [0.0] * R, [GREEDY[1]] * R, seeds)
            assert [zero[r] for r in order] == greedy and zstats == gstats, f"{n_slots} slots: all temperatures 0"
            assert t.generate_many_greedy(m.prompts, list(N_NEW))[0] == greedy          # the greedy plans behind the sampled ones
        eager.batch_init(3)
        got, _ = run_many(eager, m, order, temps, topps, seeds)
        assert got == want, "Q3_FLAG_NO_GRAPH"


def test_errors(q3, models, tmp_path_factory):
    m = models("tiny-g64")
    V = m.shape.vocab_size
    lib = q3.load_library()
    with m.engine() as t:
        with pytest.raises(IndexError, match="q3_batch_init"):
            t.batch_step_cols_draw([0], [1], [0])
        with pytest.raises(IndexError, match="q3_batch_init"):
            t.generate_many_sampled([[1, 2]], [2], 1.0, 0.9, 1)
        t.batch_init(3, 40)
        assert len(t.generate_many_sampled([[1] * 30], [11], 1.0, 0.9, 7)[0][0]) == 11           # no batch sampler was ever set
        # temperature 0, or no batch sampler: q3_batch_step_cols
        assert t.batch_step_cols_draw([0, 0], [1, 2], [0, 1], keep=[0, 0]) == t.batch_step_cols([1, 1], [1, 2], [0, 1])
        t.set_batch_sampler(0.8, 0.9, [1, 2, 3])
        bad = [
            ([], [], []), ([0] * 33, [1] * 33, list(range(33))),                     # n_cols 0 and 33
            ([3], [1], [0]), ([-1], [1], [0]),                                       # slot outside 0 .. max_streams - 1
            ([0, 1, 0], [1, 1, 1], [0, 0, 1]),                                       # a slot in two runs
            ([0, 0], [1, 1], [3, 5]), ([0, 0], [1, 1], [3, 3]),                      # a run must be consecutive and ascending
            ([0], [V], [0]), ([0], [-1], [0]), ([0], [1], [40]), ([0], [1], [-1]),   # token, position out of range
        ]
        for slots, toks, pos in bad:
            with pytest.raises(IndexError):
                t.batch_step_cols_draw(slots, toks, pos)
        i32 = lambda v: (C.c_int32 * len(v))(*v)
        assert lib.q3_batch_step_cols_draw(t._h, None, i32([1]), i32([0]), 1, None, None, None) == -3
        assert lib.q3_batch_step_cols_draw(t._h, i32([0]), None, i32([0]), 1, None, None, None) == -3
        assert lib.q3_batch_step_cols_draw(t._h, i32([0]), i32([1]), None, 1, None, None, None) == -3
        # the two greedy names still refuse a sampling batch
        with pytest.raises(q3.Q3Error) as ei:
            t.batch_step_cols([0], [1], [0])
        assert ei.value.code == -5 and "greedy only" in ei.value.msg
        with pytest.raises(q3.Q3Error) as ei:
            t.generate_many_greedy([[1, 2]], [2])
        assert ei.value.code == -5 and "greedy only" in ei.value.msg
        for prompts_, n_new in [([[]], [1]), ([[1, 2]], [0]), ([[1] * 30], [12]), ([[1, V]], [1])]:
            with pytest.raises(IndexError):
                t.generate_many_sampled(prompts_, n_new, 1.0, 0.9, 1)
        for T, p in [(-1.0, 0.9), (float("nan"), 0.9), (1.0, 1.5), (1.0, -0.1)]:
            with pytest.raises(IndexError):
                t.generate_many_sampled([[1, 2]], [2], T, p, 1)
        # null arrays
        szs = lambda v: (C.c_size_t * len(v))(*v)
        f32 = lambda v: (C.c_float * len(v))(*v)
        u64 = lambda v: (C.c_uint64 * len(v))(*v)
        full = [t._h, i32([1, 2]), szs([2]), szs([2]), 1, f32([1.0]), f32([0.9]), u64([1]), i32([0, 0]), None]
        assert lib.q3_generate_many_sampled(*full) == 0
        for k in (1, 2, 3, 5, 6, 7, 8):
            args = list(full)
            args[k] = None
            assert lib.q3_generate_many_sampled(*args) == -3, f"argument {k} null"
    with m.engine(fast=True) as t:
        t.batch_init(2)
        t.set_batch_sampler(0.8, 0.9, [1, 2])
        with pytest.raises(q3.Q3Error) as ei:
            t.batch_step_cols_draw([0], [1], [0])
        assert ei.value.code == -5 and "Q3_FLAG_FAST" in ei.value.msg
        with pytest.raises(q3.Q3Error) as ei:
            t.generate_many_sampled([[1, 2]], [2], 1.0, 0.9, 1)
        assert ei.value.code == -5 and "Q3_FLAG_FAST" in ei.value.msg
    # 8 query heads per kv head: the shape the short prefill block refuses
    ck = q3.checkpoint
    path = str(tmp_path_factory.mktemp("colsdraw") / "kvmul8.bin")
    ck.write_synthetic_checkpoint(path, ck.ModelShape(256, 384, 2, 8, 1, 512, 96, 64, True, 64), seed=5)
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(2)
        t.set_batch_sampler(0.8, 0.9, [1, 2])
        with pytest.raises(q3.Q3Error) as ei:
            t.batch_step_cols_draw([0], [1], [0])
        assert ei.value.code == -5 and "per-kv-head attention kernel" in ei.value.msg
        with pytest.raises(q3.Q3Error) as ei:
            t.generate_many_sampled([[1, 2]], [2], 1.0, 0.9, 1)
        assert ei.value.code == -5 and "per-kv-head attention kernel" in ei.value.msg


def test_generate_many_cuts_at_stop_tokens(q3, models):
    """generation.generate_many(sampler=...): rows cut behind the first stop token, like the greedy path"""
    m = models("tiny-g64")
    T, p = SAMPLERS[2]
    R = len(PROMPT_LEN)
    seeds = request_seeds(1)
    full = [(m.request(r, T, p, seeds[r])[0] + [None] * 5)[:5] for r in range(R)]
    with m.engine() as t:
        t.batch_init(3)
        # requests 1 .. 4 want >= 5 tokens in the shared cases: their first 5 are the reference's (request 0 is run on its own below)
        stop = full[3][2]
        got, stats = q3.generate_many(t, m.prompts[1:], 5, stop_tokens=[stop], sampler=(T, p, seeds[1:]))
        for r in range(1, R):
            exp = full[r]
            assert got[r - 1] == (exp[:exp.index(stop) + 1] if stop in exp else exp), f"request {r}"
        assert len(got[2]) == full[3].index(stop) + 1 and stats.passes > 0
        got, _ = q3.generate_many(t, m.prompts[:1], 3, sampler=(T, p, seeds[0]))               # scalars: one sampler for all
        assert got == [full[0][:3]]
        assert q3.generate_many(t, m.prompts, 4)[0] == t.generate_many_greedy(m.prompts, [4] * R)[0]   # sampler=None: the greedy path
