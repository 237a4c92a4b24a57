"""The shared prompt prefix in the loops (include/qwen3_hip.h section 2i): q3_batch_prefix_set and q3_generate_many_prefix.  The
yardstick is always the existing loops on the FULL prompts prefix + suffix, run on an engine of their own (so that no slot of the
engine under test ever saw the prefix through the weights), or a fresh single-stream engine.  Nothing here has a tolerance.

Stop sets are picked as in test_cols_stop.py, from the rows of the existing loop at the cap, with the suffix lengths for the
schedule.  Checked with the CPU oracle for the checkpoint seed, prefixes and suffixes used here: tiny-g64 (P 7) greedy picks [348]
(n_emit 10, 10, 1, 10, 3, 10, 10; 9 passes saved), sampled [31, 198] (10, 10, 1, 10, 10, 10, 5; 12 saved); small-hd128 (P 33) greedy
[602] (10, 5, 1, 10, 10, 2, 10; 9 saved), sampled [209] (10, 1, 10, 2, 10, 10, 10; 11 saved)."""
import pytest

import cols_sim
from cols_stop_cases import SEEDS, STOP_MAX, TEMPERATURE, TOPP, kinds, n_emit_of, passes_saved, pick_stops
from conftest import assert_biteq
from prefix_cases import CAP, CKPT_SEED, PREFIX_LENS, PREFIX_ONE, SLOTS, context, prefix, suffixes

pytestmark = pytest.mark.gpu

SAMPLER = (list(TEMPERATURE), TOPP, list(SEEDS))
N = len(TEMPERATURE)
CASES = [(name, P) for name, lens in PREFIX_LENS.items() for P in lens]


class Model:
    """One synthetic checkpoint and what the existing loops make of the full prompts at the cap: computed once, never changed."""

    def __init__(self, q3, name, path):
        self.q3, self.name, self.path = q3, name, path
        self.shape = q3.checkpoint.SHAPES[name]
        self.ctx = context(self.shape, name)
        q3.checkpoint.write_synthetic_checkpoint(path, self.shape, seed=CKPT_SEED)
        self._at_cap = {}

    def engine(self):
        return self.q3.TransformerBuilder(self.path).with_ctx_length(self.ctx).build()

    def batch_engine(self, slots=SLOTS):
        t = self.engine()
        t.batch_init(slots)
        return t

    def prefix(self, P):
        return prefix(self.shape.vocab_size, P)

    def suffixes(self, P):
        return suffixes(self.shape.vocab_size, self.ctx, P)

    def full(self, P):
        return [self.prefix(P) + s for s in self.suffixes(P)]

    def at_cap(self, P, sampled):
        """rows of the existing loop for the full prompts, on an engine of its own"""
        if (P, sampled) not in self._at_cap:
            with self.batch_engine() as t:
                rows, stats = (t.generate_many_sampled(self.full(P), [CAP] * N, *SAMPLER) if sampled
                               else t.generate_many_greedy(self.full(P), [CAP] * N))
            assert stats.passes == cols_sim.schedule([len(p) for p in self.full(P)], [CAP] * N, SLOTS)[1].passes
            self._at_cap[(P, sampled)] = rows
        return self._at_cap[(P, sampled)]

    def stops(self, P, sampled):
        rows = self.at_cap(P, sampled)
        sl = [len(s) for s in self.suffixes(P)]
        stop = pick_stops(rows, sl, SLOTS)
        assert stop is not None and len(stop) <= STOP_MAX, f"no stop set ends the rows in every way: {rows}"
        at_y0, inside, never = kinds(rows, stop)
        assert at_y0 >= 1 and inside >= 1 and never >= 1 and passes_saved(rows, stop, sl, SLOTS) >= 1
        return stop, n_emit_of(rows, stop)


@pytest.fixture(scope="module")
def models(q3, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Model(q3, name, str(tmp_path_factory.mktemp("prefixloop") / f"{name}.bin"))
        return made[name]
    return get


def tup(stats):
    return (stats.passes, stats.live_columns, stats.prompt_columns, stats.decode_columns)


def check_equal_calls(m, P, sampler, want):
    sl = [len(s) for s in m.suffixes(P)]
    wstats = cols_sim.schedule(sl, [CAP] * N, SLOTS)[1]
    with m.batch_engine() as t:
        t.batch_prefix_set(m.prefix(P))
        assert t.batch_prefix_get() == m.prefix(P)
        for k in range(2):                                   # the second call finds the slots dirty above P
            out, n_out, stats = t.generate_many_prefix(m.suffixes(P), [CAP] * N, (), sampler, raw=True)
            assert [out[r * CAP:(r + 1) * CAP] for r in range(N)] == want, f"call {k}"
            assert n_out == [CAP] * N and tup(stats) == tuple(wstats), f"call {k}"


@pytest.mark.parametrize("name, P", CASES)
def test_greedy_equals_the_loop_on_the_full_prompts(q3, models, name, P):
    m = models(name)
    assert all(P + len(s) + CAP - 1 <= m.ctx for s in m.suffixes(P)) and max(len(s) for s in m.suffixes(P)) >= 40
    check_equal_calls(m, P, None, m.at_cap(P, False))


@pytest.mark.parametrize("name, P", CASES)
def test_under_samplers(q3, models, name, P):
    """greedy and sampled requests mixed: a sampled request's rng stands P coins behind its seed at its first column"""
    m = models(name)
    want = m.at_cap(P, True)
    assert want != m.at_cap(P, False)
    check_equal_calls(m, P, SAMPLER, want)


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("name", ["tiny-g64", "small-hd128"])
def test_stop_tokens(q3, models, name, sampled):
    m = models(name)
    P = PREFIX_ONE[name]
    sampler = SAMPLER if sampled else None
    rows = m.at_cap(P, sampled)
    stop, emit = m.stops(P, sampled)
    sl = [len(s) for s in m.suffixes(P)]
    wstats = cols_sim.schedule(sl, emit, SLOTS)[1]
    with m.batch_engine() as ref:
        want_out, want_n, _ = ref.generate_many_stop(m.full(P), [CAP] * N, stop, sampler, raw=True)
    assert want_n == emit
    with m.batch_engine() as t:
        t.batch_prefix_set(m.prefix(P))
        for k in range(2):
            out, n_out, stats = t.generate_many_prefix(m.suffixes(P), [CAP] * N, stop, sampler, raw=True)
            assert out == want_out and n_out == emit, f"call {k}"
            for r in range(N):
                got = out[r * CAP:(r + 1) * CAP]
                assert got[:emit[r]] == rows[r][:emit[r]] and got[emit[r]:] == [-1] * (CAP - emit[r]), f"call {k}: request {r}"
            assert tup(stats) == tuple(wstats), f"call {k}"
        cut, cstats = t.generate_many_prefix(m.suffixes(P), [CAP] * N, stop, sampler)
        assert cut == [r[:e] for r, e in zip(rows, emit)] and tup(cstats) == tuple(wstats)


def kv_rows(c, flat, ctx, n):
    return flat.reshape(c.n_layers, ctx, c.n_kv_heads * c.head_dim)[:, :n]


@pytest.mark.parametrize("name, P", [("tiny-g64", 7), ("tiny-g64", 40), ("small-hd128", 70)])
def test_slot_and_store(q3, models, name, P):
    """slot 0 after batch_prefix_set holds what a single-stream prefill writes; a loop call puts those rows into every slot it uses"""
    m = models(name)
    with m.batch_engine() as t, m.engine() as ref:
        t.set_batch_sampler(0.8, 0.9, [11, 12, 13])          # whatever the batch sampler says, no rng is involved
        t.batch_prefix_set(m.prefix(P))
        ref.prefill(m.prefix(P), 0)
        c = t.get_config()
        want = {kind: kv_rows(c, ref.read_state(kind), c.seq_len, P) for kind in ("key", "value")}
        for kind in ("key", "value"):
            assert_biteq(kv_rows(c, t.batch_read_state(0, kind), t._batch_ctx, P), want[kind], f"slot 0 {kind} rows behind batch_prefix_set")
            for s in range(1, SLOTS):
                assert not kv_rows(c, t.batch_read_state(s, kind), t._batch_ctx, P).any(), f"slot {s} is untouched"
        t.set_batch_sampler(0.0, 0.9, [11, 12, 13])
        t.generate_many_prefix(m.suffixes(P), [CAP] * N)
        for kind in ("key", "value"):
            for s in range(SLOTS):
                assert_biteq(kv_rows(c, t.batch_read_state(s, kind), t._batch_ctx, P), want[kind], f"slot {s} {kind} rows behind a loop call")


@pytest.mark.parametrize("name", ["tiny-g64", "small-hd128"])
def test_residency(q3, models, name):
    """the store is private: calls that overwrite rows 0 .. of every slot, and batch_reset_kv, do not change what the prefix loop returns"""
    m = models(name)
    P = PREFIX_ONE[name]
    want = m.at_cap(P, False)
    other = [[(t + 1) % m.shape.vocab_size for t in p] for p in m.full(P)]
    with m.batch_engine() as t:
        assert t.batch_prefix_get() == []
        with pytest.raises(IndexError, match="prefix"):      # Q3_ERR_ARG: nothing resident
            t.generate_many_prefix(m.suffixes(P), [CAP] * N)
        t.batch_prefix_set(m.prefix(P))
        t.generate_many_greedy(other, [CAP] * N)
        assert t.generate_many_prefix(m.suffixes(P), [CAP] * N)[0] == want
        t.batch_reset_kv()
        assert t.batch_prefix_get() == m.prefix(P)
        assert t.generate_many_prefix(m.suffixes(P), [CAP] * N)[0] == want
        # a new prefix replaces the old one; [] releases it; batch_init drops it
        P2 = PREFIX_LENS[name][-1]
        t.batch_prefix_set(m.prefix(P2))
        assert t.generate_many_prefix(m.suffixes(P2), [CAP] * N)[0] == m.at_cap(P2, False)
        t.batch_prefix_set([])
        assert t.batch_prefix_get() == []
        t.batch_prefix_set(m.prefix(P))
        t.batch_init(SLOTS)
        assert t.batch_prefix_get() == []
        with pytest.raises(IndexError, match="prefix"):
            t.generate_many_prefix(m.suffixes(P), [CAP] * N)


@pytest.mark.parametrize("name", ["tiny-g64", "small-hd128"])
def test_generate_many_shared_prefix(q3, models, name):
    m = models(name)
    P = 33
    sl = [len(s) for s in m.suffixes(P)]
    rows = m.at_cap(P, False)
    stop = [rows[0][CAP // 2]]                               # request 0 ends inside its row at the latest
    emit = n_emit_of(rows, stop)
    assert emit[0] <= CAP // 2 + 1
    assert q3.common_prefix_len(m.full(P)) == P
    with m.batch_engine() as ref:
        want, wstats = q3.generate_many(ref, m.full(P), CAP, stop_tokens=stop)
        want_dev, _ = q3.generate_many(ref, m.full(P), CAP, stop_tokens=stop, stop_on_device=True)
    assert want == want_dev == [r[:e] for r, e in zip(rows, emit)]
    with m.batch_engine() as t:
        got, stats = q3.generate_many(t, m.full(P), CAP, stop_tokens=stop, shared_prefix=True)
        assert got == want and tup(stats) == tuple(cols_sim.schedule(sl, [CAP] * N, SLOTS)[1]) and stats.passes < wstats.passes
        assert t.batch_prefix_get() == m.prefix(P)
        got, stats = q3.generate_many(t, m.full(P), CAP, stop_tokens=stop, shared_prefix=True, stop_on_device=True)
        assert got == want and tup(stats) == tuple(cols_sim.schedule(sl, emit, SLOTS)[1])
        got, _ = q3.generate_many(t, m.suffixes(P), CAP, stop_tokens=stop, shared_prefix=m.prefix(P), sampler=SAMPLER)
        assert got == [r[:e] for r, e in zip(m.at_cap(P, True), n_emit_of(m.at_cap(P, True), stop))]


@pytest.mark.parametrize("name", ["tiny-g64", "small-hd128"])
def test_forking(q3, models, name):
    """one prompt prefilled into slot 0 and copied to slots 1 and 2: three draws of its last token with three seeds"""
    m = models(name)
    prompt = m.full(33)[4]
    n = len(prompt)
    seeds = [SEEDS[0], SEEDS[1], SEEDS[2]]
    with m.batch_engine() as t, m.engine() as ref:
        t.batch_prefill_slots([0], [prompt[:-1]], [0])
        t.batch_copy_rows(0, [1, 2], 0, n - 1)
        t.set_batch_sampler(0.8, 0.9, seeds)
        got = t.batch_step_cols_draw([0, 1, 2], [prompt[-1]] * 3, [n - 1] * 3)
        want = []
        for seed in seeds:
            ref.reset_kv()
            ref.set_sampler(0.0, 0.9, 0)
            ref.prefill(prompt[:-1], 0)
            ref.set_sampler(0.8, 0.9, seed)
            want.append(ref.forward_sample(prompt[-1], n - 1))
        assert got == want


def test_errors(q3, models):
    m = models("tiny-g64")
    V = m.shape.vocab_size
    with m.engine() as t:
        with pytest.raises(IndexError, match="q3_batch_init"):
            t.batch_prefix_set([1, 2])
        with pytest.raises(IndexError, match="q3_batch_init"):
            t.generate_many_prefix([[1]], [1])
        assert t.batch_prefix_get() == []
        t.batch_init(2, 40)
        for bad in ([1] * 40, [1, V], [-1]):                 # n >= the batch context; a token outside the vocabulary
            with pytest.raises(IndexError):
                t.batch_prefix_set(bad)
        assert t.batch_prefix_get() == []
        t.batch_prefix_set([1] * 39)                         # one row is left
        assert t.generate_many_prefix([[2], [3]], [1, 1])[1].passes == 1
        t.batch_prefix_set([1, 2, 3])
        for suffixes_, n_new in [([[1] * 28], [11]), ([[]], [1]), ([[1]], [0]), ([[V]], [1])]:       # 3 + 28 + 11 - 1 > 40
            with pytest.raises(IndexError):
                t.generate_many_prefix(suffixes_, n_new)
        assert len(t.generate_many_prefix([[1] * 28], [10])[0][0]) == 10
        with pytest.raises(IndexError, match="stop tokens"):
            t.generate_many_prefix([[1]], [2], list(range(9)))
        with pytest.raises(IndexError):
            t.generate_many_prefix([[1]], [2], [V])
        for sampler in [(-0.5, 0.9, 1), (0.8, 1.5, 1), (float("nan"), 0.9, 1)]:
            with pytest.raises(IndexError):
                t.generate_many_prefix([[1]], [2], (), sampler)
        t.set_batch_sampler(0.8, 0.9, [1, 2])
        with pytest.raises(q3.Q3Error) as ei:                # a greedy call under a sampling batch, as generate_many_stop
            t.generate_many_prefix([[1]], [2])
        assert ei.value.code == -5
    with q3.TransformerBuilder(m.path).with_strict(False).build() as t:
        t.batch_init(2)
        with pytest.raises(q3.Q3Error) as ei:
            t.batch_prefix_set([1, 2])
        assert ei.value.code == -5 and "Q3_FLAG_FAST" in ei.value.msg
