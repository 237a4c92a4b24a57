"""Ragged column passes over the batched state (include/qwen3_hip.h section 2e): q3_batch_step_cols and q3_generate_many_greedy.
The yardstick is always a second single-stream engine of the same context -- forward / prefill / generate_greedy over a zeroed
cache, read_state against batch_read_state -- and every comparison is bit for bit."""
import numpy as np
import pytest

import cols_sim
from conftest import assert_biteq

pytestmark = pytest.mark.gpu

# shape -> batch context: head_dim 64 (k_attn_gqa); head_dim 128 with 2 query heads per kv head (k_attn_gqa2<2>); 4 per kv head
# and the wide k_dgemm rows of the 4B layer
SHAPES = {"tiny-g64": 0, "small-hd128": 0, "qwen3-4b-dims-l2": 512}
N_HIST = 64


class Model:
    """One synthetic checkpoint and its single-stream references, computed once and never changed."""

    def __init__(self, q3, name, path):
        self.q3, self.name, self.path, self.ctx = q3, name, path, SHAPES[name]
        self.shape = q3.checkpoint.SHAPES[name]
        q3.checkpoint.write_synthetic_checkpoint(path, self.shape, seed=2468)
        self._refs = {}

    def engine(self, **kw):
        b = self.q3.TransformerBuilder(self.path).with_ctx_length(self.ctx or None)
        if kw.get("fast"):
            b = b.with_strict(False)
        return b.build()

    def history(self, seed, n=N_HIST):
        rng = np.random.default_rng(seed)
        return [int(t) for t in rng.integers(0, self.shape.vocab_size, n)]

    def ref(self, seed, n=N_HIST):
        """tokens of history(seed) at positions 0 .. n-1 through forward() on a fresh engine: (tokens, logits [n, V], key, value)"""
        if (seed, n) not in self._refs:
            toks = self.history(seed, n)
            with self.engine() as t:
                lg = np.stack([np.array(t.forward(tok, p), copy=True) for p, tok in enumerate(toks)])
                self._refs[(seed, n)] = (toks, lg, t.read_state("key"), t.read_state("value"))
        return self._refs[(seed, n)]


@pytest.fixture(scope="module")
def models(q3, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Model(q3, name, str(tmp_path_factory.mktemp("cols") / f"{name}.bin"))
        return made[name]
    return get


def feed(t, slot, toks, first_pos, chunks):
    """tokens toks[first_pos:] of one slot in runs of the given lengths; returns the logits of every column"""
    out, p = [], first_pos
    for c in chunks:
        lg, am = t.batch_step_cols([slot] * c, toks[p:p + c], list(range(p, p + c)), want_logits=True)
        out.append((lg, am))
        p += c
    return np.concatenate([lg for lg, _ in out]), [a for _, am in out for a in am]


def check_slot(t, slot, ref, n, what):
    """rows 0 .. n-1 of the slot's caches equal the reference's, the rest of the slot is still zero"""
    _, _, rk, rv = ref
    L, S = t.get_config().n_layers, t._batch_ctx
    kvd = t.get_config().n_kv_heads * t.get_config().head_dim
    k = t.batch_read_state(slot, "key").reshape(L, S, kvd)
    v = t.batch_read_state(slot, "value").reshape(L, S, kvd)
    assert_biteq(k[:, :n], rk.reshape(L, S, kvd)[:, :n], f"{what}: key rows")
    assert_biteq(v[:, :n], rv.reshape(L, S, kvd)[:, :n], f"{what}: value rows")
    assert not k[:, n:].any() and not v[:, n:].any(), f"{what}: rows past {n} written"


@pytest.mark.parametrize("name", list(SHAPES))
def test_identity_slots_equal_forward_batch(q3, models, name):
    m = models(name)
    n, steps = 5, 4
    toks = [m.history(100 + i, steps) for i in range(n)]
    pos0 = [0, 0, 0, 0, 0]
    with m.engine() as a, m.engine() as b:
        a.batch_init(n)
        b.batch_init(n)
        for k in range(steps):
            col = [toks[i][k] for i in range(n)]
            want, wam = a.forward_batch(col, [p + k for p in pos0])
            got, gam = b.batch_step_cols(list(range(n)), col, [p + k for p in pos0], want_logits=True)
            assert_biteq(got, want, f"step {k}")
            assert gam == wam
        for i in range(n):
            assert_biteq(b.batch_read_state(i, "key"), a.batch_read_state(i, "key"), f"slot {i} key")
            assert_biteq(b.batch_read_state(i, "value"), a.batch_read_state(i, "value"), f"slot {i} value")


@pytest.mark.parametrize("name", list(SHAPES))
def test_permuted_and_sparse_slots(q3, models, name):
    m = models(name)
    slots, steps = [3, 0, 2], 6
    refs = [m.ref(200 + i) for i in range(3)]
    with m.engine() as t:
        t.batch_init(4)
        for k in range(steps):
            lg, am = t.batch_step_cols(slots, [r[0][k] for r in refs], [k] * 3, want_logits=True)
            for j, r in enumerate(refs):
                assert_biteq(lg[j], r[1][k], f"slot {slots[j]} step {k}")
                assert am[j] == q3.sample_argmax(r[1][k])
        for j, r in enumerate(refs):
            check_slot(t, slots[j], r, steps, f"slot {slots[j]}")
        assert not t.batch_read_state(1, "key").any() and not t.batch_read_state(1, "value").any()


@pytest.mark.parametrize("name", list(SHAPES))
def test_runs_walk_a_slot(q3, models, name):
    m = models(name)
    ref = m.ref(300)
    with m.engine() as t:
        t.batch_init(2)
        lg, am = feed(t, 1, ref[0], 0, [1, 2, 5, 16, 32, 8])
        assert_biteq(lg, ref[1], "logits of every column")
        assert am == [q3.sample_argmax(r) for r in ref[1]]
        assert_biteq(t.batch_read_state(1, "key"), ref[2], "key cache")
        assert_biteq(t.batch_read_state(1, "value"), ref[3], "value cache")
        assert not t.batch_read_state(0, "key").any()


@pytest.mark.parametrize("name", list(SHAPES))
def test_mixed_pass(q3, models, name):
    m = models(name)
    ra, rb, rc = m.ref(400), m.ref(401), m.ref(402)
    with m.engine() as t:
        t.batch_init(3)
        feed(t, 1, rb[0], 0, [32, 8])                       # slot 1: 40 tokens of history
        feed(t, 2, rc[0], 0, [5])                           # slot 2: 5
        slots = [0] * 7 + [1] + [2] * 3
        toks = ra[0][:7] + [rb[0][40]] + rc[0][5:8]
        pos = list(range(7)) + [40] + [5, 6, 7]
        lg, am = t.batch_step_cols(slots, toks, pos, want_logits=True)
        assert_biteq(lg[:7], ra[1][:7], "run of 7 from position 0")
        assert_biteq(lg[7], rb[1][40], "decode column at position 40")
        assert_biteq(lg[8:], rc[1][5:8], "run of 3 from position 5")
        assert am == [q3.sample_argmax(r) for r in list(ra[1][:7]) + [rb[1][40]] + list(rc[1][5:8])]
        check_slot(t, 0, ra, 7, "slot 0")
        check_slot(t, 1, rb, 41, "slot 1")
        check_slot(t, 2, rc, 8, "slot 2")


@pytest.mark.parametrize("n_cols", [15, 16, 17, 31, 32])
@pytest.mark.parametrize("name", ["tiny-g64", "small-hd128"])
def test_widths(q3, models, name, n_cols):
    """pad and tile boundaries: a run of n_cols - 1 in slot 1 next to one column of slot 0"""
    m = models(name)
    ra, rb = m.ref(500), m.ref(501)
    with m.engine() as t:
        t.batch_init(2)
        r = n_cols - 1
        lg, am = t.batch_step_cols([1] * r + [0], ra[0][:r] + [rb[0][0]], list(range(r)) + [0], want_logits=True)
        assert_biteq(lg[:r], ra[1][:r], "run")
        assert_biteq(lg[r], rb[1][0], "last column")
        assert am[-1] == q3.sample_argmax(rb[1][0])
        check_slot(t, 1, ra, r, "slot 1")
        check_slot(t, 0, rb, 1, "slot 0")


@pytest.mark.parametrize("name", ["tiny-g64", "qwen3-4b-dims-l2"])
def test_slot_reuse_without_reset(q3, models, name):
    m = models(name)
    ra, rb = m.ref(600), m.ref(601)
    with m.engine() as t:
        t.batch_init(1)
        feed(t, 0, ra[0], 0, [32, 19])                      # positions 0 .. 50
        lg, _ = feed(t, 0, rb[0], 0, [9, 1, 1])
        assert_biteq(lg, rb[1][:11], "second occupant of slot 0")
        L, S = t.get_config().n_layers, t._batch_ctx
        k = t.batch_read_state(0, "key").reshape(L, S, -1)
        assert_biteq(k[:, :11], rb[2].reshape(L, S, -1)[:, :11], "rows of the second occupant")
        assert_biteq(k[:, 11:51], ra[2].reshape(L, S, -1)[:, 11:51], "rows the first occupant left behind")


@pytest.mark.parametrize("name", ["tiny-g64", "small-hd128"])
def test_batched_decode_unchanged_by_a_column_pass(q3, models, name):
    m = models(name)
    ref = m.ref(700)
    toks0, pos0 = [3, 9, 27], [0, 2, 1]
    with m.engine() as t:
        t.batch_init(3)
        lg0, am0 = t.forward_batch(toks0, pos0)
        t.batch_reset_kv()
        out0 = t.generate_greedy_batch(toks0, pos0, 6)
        t.batch_reset_kv()
        lg, _ = t.batch_step_cols([2, 2, 2, 0], ref[0][:3] + [ref[0][0]], [0, 1, 2, 0], want_logits=True)
        assert_biteq(lg[:3], ref[1][:3], "column pass")
        t.batch_reset_kv()
        lg1, am1 = t.forward_batch(toks0, pos0)
        assert_biteq(lg1, lg0, "forward_batch after a column pass")
        assert am1 == am0
        t.batch_reset_kv()
        assert np.array_equal(t.generate_greedy_batch(toks0, pos0, 6), out0)
        lg2, _ = t.batch_step_cols([1], [ref[0][0]], [0], want_logits=True)      # and back again: the kept plan
        assert_biteq(lg2[0], ref[1][0], "column pass after batched decode")


def test_errors(q3, models, tmp_path_factory):
    m = models("tiny-g64")
    V = m.shape.vocab_size
    with m.engine() as t:
        with pytest.raises(IndexError, match="q3_batch_init"):
            t.batch_step_cols([0], [1], [0])
        with pytest.raises(IndexError, match="q3_batch_init"):
            t.generate_many_greedy([[1, 2]], [2])
        t.batch_init(3, 40)
        assert t.batch_step_cols([0], [1], [0]) == t.batch_step_cols([1], [1], [0])
        bad = [
            ([], [], []),                                    # n_cols 0
            ([0] * 33, [1] * 33, list(range(33))),           # n_cols 33
            ([3], [1], [0]), ([-1], [1], [0]),               # slot outside 0 .. max_streams - 1
            ([0, 1, 0], [1, 1, 1], [0, 0, 1]),               # a slot in two runs
            ([0, 0], [1, 1], [3, 5]), ([0, 0], [1, 1], [3, 3]), ([0, 0], [1, 1], [3, 2]),   # a run must be consecutive and ascending
            ([0], [V], [0]), ([0], [-1], [0]),               # token outside the vocabulary
            ([0], [1], [40]), ([0], [1], [-1]),              # position >= the batch context
        ]
        for slots, toks, pos in bad:
            with pytest.raises(IndexError):
                t.batch_step_cols(slots, toks, pos)
        for prompts, n_new in [([[]], [1]), ([[1, 2]], [0]), ([[1] * 30], [12]), ([[1, V]], [1])]:
            with pytest.raises(IndexError):
                t.generate_many_greedy(prompts, n_new)
        assert len(t.generate_many_greedy([[1] * 30], [11])[0][0]) == 11         # 30 + 11 - 1 = 40 positions: fits
        t.set_batch_sampler(0.8, 0.9, [1, 2, 3])
        with pytest.raises(q3.Q3Error) as ei:
            t.batch_step_cols([0], [1], [0])
        assert ei.value.code == -5 and "greedy only" in ei.value.msg
        with pytest.raises(q3.Q3Error) as ei:
            t.generate_many_greedy([[1, 2]], [2])
        assert ei.value.code == -5
        t.set_batch_sampler(0.0, 0.9, [1, 2, 3])
        t.batch_step_cols([0], [1], [0])
    with m.engine(fast=True) as t:
        t.batch_init(2)
        with pytest.raises(q3.Q3Error) as ei:
            t.batch_step_cols([0], [1], [0])
        assert ei.value.code == -5 and "Q3_FLAG_FAST" in ei.value.msg
    # 8 query heads per kv head: the shape the short prefill block refuses
    ck = q3.checkpoint
    path = str(tmp_path_factory.mktemp("cols") / "kvmul8.bin")
    ck.write_synthetic_checkpoint(path, ck.ModelShape(256, 384, 2, 8, 1, 512, 96, 64, True, 64), seed=5)
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(2)
        with pytest.raises(q3.Q3Error) as ei:
            t.batch_step_cols([0], [1], [0])
        assert ei.value.code == -5 and "per-kv-head attention kernel" in ei.value.msg


MANY_LEN, MANY_NEW = (1, 3, 33, 40, 7), (4, 1, 20, 9, 33)


def many_ref(m):
    if "many" not in m._refs:
        prompts = [m.history(800 + r, n) for r, n in enumerate(MANY_LEN)]
        rows = []
        with m.engine() as t:
            for p, k in zip(prompts, MANY_NEW):
                t.reset_kv()
                y0 = t.prefill(p, 0)
                rows.append([y0] + (t.generate_greedy(y0, len(p), k - 1) if k > 1 else []))
        m._refs["many"] = (prompts, rows)
    return m._refs["many"]


@pytest.mark.parametrize("max_streams", [2, 32])
@pytest.mark.parametrize("name", list(SHAPES))
def test_generate_many_greedy(q3, models, name, max_streams):
    m = models(name)
    prompts, want = many_ref(m)
    _, wstats = cols_sim.schedule(MANY_LEN, MANY_NEW, max_streams)
    with m.engine() as t:
        t.batch_init(max_streams)
        for _ in range(2):                                  # the second call finds the slots as the first left them
            rows, stats = t.generate_many_greedy(prompts, list(MANY_NEW))
            for r in range(len(prompts)):
                assert rows[r] == want[r], f"request {r}"
            assert (stats.passes, stats.live_columns, stats.prompt_columns, stats.decode_columns) == tuple(wstats)
        stop = want[2][1]
        got, _ = q3.generate_many(t, prompts, 5, stop_tokens=[stop])             # rows cut behind the first stop token
        for r in (2, 3, 4):
            exp = want[r][:5]
            assert got[r] == (exp[:exp.index(stop) + 1] if stop in exp else exp), f"request {r}"
