"""Dense blocks over the slots of the batched state (include/qwen3_hip.h section 2g): q3_batch_prefill_slots and
q3_generate_many_dense.  The yardstick is always the sequential path on a fresh single-stream engine of the same context --
prefill / forward / generate_greedy, the same behind set_sampler -- and every comparison is bit for bit."""
import numpy as np
import pytest

import edge_ckpt
from conftest import assert_biteq

pytestmark = pytest.mark.gpu

NAME, CTX = "qwen3-0.6b-dims-l2", 512
N_MORE = 5


class Model:
    """One checkpoint and its single-stream references, computed once and never changed."""

    def __init__(self, q3, name, path, ctx=CTX):
        self.q3, self.name, self.path, self.ctx = q3, name, path, ctx
        self.shape = q3.checkpoint.SHAPES[name]
        self._refs = {}

    def engine(self, fast=False):
        b = self.q3.TransformerBuilder(self.path).with_ctx_length(self.ctx)
        return (b.with_strict(False) if fast else b).build()

    def prompt(self, seed, n):
        rng = np.random.default_rng(seed)
        return [int(t) for t in rng.integers(0, self.shape.vocab_size, n)]

    def ref(self, seed, n):
        """prompt(seed, n) on a fresh engine: dict(prompt, first = prefill's token, more = N_MORE greedy tokens behind it, key / value
        [L, S, kvd] after the prompt, logits = forward's of the last prompt token)"""
        if (seed, n) not in self._refs:
            p = self.prompt(seed, n)
            with self.engine() as t:
                if n > 1:
                    t.prefill(p[:-1], 0)
                lg = np.array(t.forward(p[-1], n - 1), copy=True)
                cfg = t.get_config()
                kvd = cfg.n_kv_heads * cfg.head_dim
                key = t.read_state("key").reshape(cfg.n_layers, self.ctx, kvd)[:, :n].copy()
                value = t.read_state("value").reshape(cfg.n_layers, self.ctx, kvd)[:, :n].copy()
                t.reset_kv()
                first = t.prefill(p, 0)
                more = [int(v) for v in t.generate_greedy(first, n, N_MORE)]
            assert first == self.q3.sample_argmax(lg)
            self._refs[(seed, n)] = dict(prompt=p, first=first, more=more, key=key, value=value, logits=lg)
        return self._refs[(seed, n)]

    def ref_sampled(self, seed, n, temperature, topp, rng_seed, n_new):
        k = (seed, n, temperature, topp, rng_seed, n_new)
        if k not in self._refs:
            p = self.prompt(seed, n)
            with self.engine() as t:
                t.set_sampler(temperature, topp, rng_seed)
                first = t.prefill(p, 0)
                rest = [int(v) for v in t.generate_greedy(first, n, n_new - 1)] if n_new > 1 else []       # q3_generate_sampled once a sampler is set
            self._refs[k] = [first] + rest
        return self._refs[k]


@pytest.fixture(scope="module")
def models(q3, tmp_path_factory):
    made = {}

    def get(name=NAME, edit=None):
        if (name, edit) not in made:
            path = str(tmp_path_factory.mktemp("dense") / f"{name}-{edit}.bin")
            if edit:
                edge_ckpt.write(path, name, edit)
            else:
                q3.checkpoint.write_synthetic_checkpoint(path, q3.checkpoint.SHAPES[name], seed=1357)
            made[(name, edit)] = Model(q3, name, path)
        return made[(name, edit)]
    return get


def slot_rows(t, slot, ctx=CTX):
    c = t.get_config()
    kvd = c.n_kv_heads * c.head_dim
    return (t.batch_read_state(slot, "key").reshape(c.n_layers, ctx, kvd),
            t.batch_read_state(slot, "value").reshape(c.n_layers, ctx, kvd))


def check_rows(t, slot, ref, n, what):
    """rows 0 .. n-1 of the slot equal the reference's, every later row is still zero"""
    k, v = slot_rows(t, slot)
    assert_biteq(k[:, :n], ref["key"][:, :n], f"{what}: key rows")
    assert_biteq(v[:, :n], ref["value"][:, :n], f"{what}: value rows")
    assert not k[:, n:].any() and not v[:, n:].any(), f"{what}: rows past {n} written"


def finish(q3, t, slots, refs, what):
    """every prompt's last token through one column pass: forward's logits, prefill's token, then N_MORE greedy tokens"""
    n = [len(r["prompt"]) for r in refs]
    lg, am = t.batch_step_cols(slots, [r["prompt"][-1] for r in refs], [k - 1 for k in n], want_logits=True)
    for j, r in enumerate(refs):
        assert_biteq(lg[j], r["logits"], f"{what}: logits of slot {slots[j]}")
        assert am[j] == r["first"]
    rows = [[] for _ in refs]
    for k in range(N_MORE):
        am = t.batch_step_cols(slots, am, [x + k for x in n])
        for j in range(len(refs)):
            rows[j].append(am[j])
    assert rows == [r["more"] for r in refs], what


def several_slots(q3, m):
    """runs of 41, 97 and 8 tokens into slots 2, 0 and 5 of an 8-slot batch, slot 0 from position 5: 160 padded columns"""
    slots = [2, 0, 5]
    refs = [m.ref(11, 42), m.ref(12, 5 + 97 + 1), m.ref(13, 9)]
    first = [0, 5, 0]
    with m.engine() as t:
        t.batch_init(8)
        t.batch_step_cols([0] * 5, refs[1]["prompt"][:5], list(range(5)))
        st = t.batch_prefill_slots(slots, [r["prompt"][f:-1] for r, f in zip(refs, first)], first)
        assert (st.blocks, st.live_columns, st.pad_columns) == (1, 41 + 97 + 8, 160 - 146)
        for s, r in zip(slots, refs):
            check_rows(t, s, r, len(r["prompt"]) - 1, f"slot {s}")
        for s in (1, 3, 4, 6, 7):
            k, v = slot_rows(t, s)
            assert not k.any() and not v.any(), f"slot {s} written"
        finish(q3, t, slots, refs, "several slots")


def test_several_slots_share_one_block(q3, models):
    several_slots(q3, models())


def test_several_slots_on_an_edge_valued_checkpoint(q3, models):
    several_slots(q3, models(NAME, "all"))


# padded columns -> the path: 25: a column pass; 48: per-wave k_pgemm, 3 position tiles; 96: k_pgemm3; 288 over 8 kv heads: k_attn_pf2
# with 8 positions per workgroup (the others take 4)
@pytest.mark.parametrize("lens", [(10, 9), (20, 17), (33,), (50, 40), (70, 70, 70, 70)], ids=lambda v: "+".join(map(str, v)))
def test_switch_points(q3, models, lens):
    m = models()
    slots = [3, 1, 0, 2][:len(lens)]
    refs = [m.ref(20 + i, n + 1) for i, n in enumerate(lens)]
    want, _ = q3.dense_pack(list(lens), 2048)
    with m.engine() as t:
        t.batch_init(4)
        st = t.batch_prefill_slots(slots, [r["prompt"][:-1] for r in refs], [0] * len(lens))
        assert st.blocks == 1 and st.live_columns == sum(lens) and st.live_columns + st.pad_columns == -(-(want[-1][1] + lens[-1]) // 8) * 8
        for s, r, n in zip(slots, refs, lens):
            check_rows(t, s, r, n, f"slot {s}")
        finish(q3, t, slots, refs, str(lens))


def test_a_run_splits_over_blocks_of_128(q3, models, monkeypatch):
    """Q3_PREFILL_M=128: a 301-token run takes three blocks, a second request shares the last one"""
    monkeypatch.setenv("Q3_PREFILL_M", "128")
    m = models()
    refs = [m.ref(31, 302), m.ref(32, 21)]
    with m.engine() as t:
        t.batch_init(2)
        st = t.batch_prefill_slots([1, 0], [r["prompt"][:-1] for r in refs], [0, 0])
        assert (st.blocks, st.live_columns, st.pad_columns) == (3, 321, 72 - 65)
        check_rows(t, 1, refs[0], 301, "the split run")
        check_rows(t, 0, refs[1], 20, "its neighbour")
        finish(q3, t, [1, 0], refs, "blocks of 128")


def test_the_block_width_is_fixed_by_the_first_dense_call(q3, models, monkeypatch):
    """Q3_PREFILL_M changes between two calls on one batched state: the second call still packs for the scratch of the first
    (blocks of 48 columns), in either direction, and a new q3_batch_init reads the variable again"""
    m = models()
    refs = [m.ref(35, 151), m.ref(36, 61)]
    prompts = [r["prompt"][:-1] for r in refs]
    monkeypatch.setenv("Q3_PREFILL_M", "48")
    with m.engine() as t:
        t.batch_init(2)
        want = q3.dense_pack([150, 60], 48)[1]
        assert t.batch_prefill_slots([0, 1], prompts, [0, 0]) == want and want.blocks == 5
        monkeypatch.delenv("Q3_PREFILL_M")
        t.batch_reset_kv()
        assert t.batch_prefill_slots([1, 0], prompts, [0, 0]) == want
        check_rows(t, 1, refs[0], 150, "packed for the first call's scratch")
        check_rows(t, 0, refs[1], 60, "its neighbour")
        monkeypatch.setenv("Q3_PREFILL_M", "4096")
        rows, _, ds = t.generate_many_dense([r["prompt"] for r in refs], [2, 2], None, 8)
        assert rows == [[r["first"], r["more"][0]] for r in refs] and ds == want
        t.batch_init(2)                                          # starts the scratch over
        monkeypatch.setenv("Q3_PREFILL_M", "256")
        assert t.batch_prefill_slots([0, 1], prompts, [0, 0]) == q3.dense_pack([150, 60], 256)[1]
        finish(q3, t, [0, 1], refs, "after a new batch_init")


def test_slot_reuse(q3, models):
    """a slot that held a longer sequence takes a shorter one: rows past the run are never read"""
    m = models()
    long_, short = m.ref(41, 121), m.ref(42, 41)
    with m.engine() as t:
        t.batch_init(2)
        t.batch_prefill_slots([1], [long_["prompt"][:-1]], [0])
        finish(q3, t, [1], [long_], "first occupant")
        t.batch_prefill_slots([1], [short["prompt"][:-1]], [0])
        k, v = slot_rows(t, 1)
        assert_biteq(k[:, :40], short["key"][:, :40], "key rows of the second occupant")
        assert_biteq(v[:, :40], short["value"][:, :40], "value rows of the second occupant")
        assert_biteq(k[:, 46:120], long_["key"][:, 46:120], "rows of the first occupant past the run")
        finish(q3, t, [1], [short], "second occupant")


def test_a_shape_the_dense_kernels_refuse_walks_32_columns(q3, tmp_path_factory):
    """small-longctx: head_dim 64"""
    name = "small-longctx"
    path = str(tmp_path_factory.mktemp("dense64") / "m.bin")
    q3.checkpoint.write_synthetic_checkpoint(path, q3.checkpoint.SHAPES[name], seed=77)
    m = Model(q3, name, path)
    refs = [m.ref(51, 42), m.ref(52, 71)]
    with m.engine() as t:
        t.batch_init(3)
        st = t.batch_prefill_slots([2, 0], [r["prompt"][:-1] for r in refs], [0, 0])
        assert st.live_columns == 41 + 70 and st.blocks == q3.dense_pack([41, 70], 32)[1].blocks
        check_rows(t, 2, refs[0], 41, "slot 2")
        check_rows(t, 0, refs[1], 70, "slot 0")
        k, v = slot_rows(t, 1)
        assert not k.any() and not v.any()
        finish(q3, t, [2, 0], refs, name)


@pytest.mark.parametrize("lens", [(45, 20), (10, 9), (40, 30)], ids=lambda v: "+".join(map(str, v)))
def test_under_the_batch_sampler(q3, models, lens, monkeypatch):
    """(45, 20): one wide block; (10, 9): a column pass; (40, 30) with blocks of 48 columns: a wide block, then a narrow one"""
    m = models()
    T, P, seeds, n_new = 0.8, 0.9, [0x1234567, 0xABCDEF01], 4
    want = [m.ref_sampled(60 + i, n + 1, T, P, seeds[i], n_new) for i, n in enumerate(lens)]
    prompts = [m.prompt(60 + i, n + 1) for i, n in enumerate(lens)]
    if lens == (40, 30):
        monkeypatch.setenv("Q3_PREFILL_M", "48")
    with m.engine() as t:
        t.batch_init(2)
        t.set_batch_sampler(T, P, seeds)
        t.batch_prefill_slots([0, 1], [p[:-1] for p in prompts], [0, 0])
        tok = t.batch_step_cols_draw([0, 1], [p[-1] for p in prompts], list(lens))
        rows = [[tok[0]], [tok[1]]]
        for k in range(1, n_new):
            tok = t.batch_step_cols_draw([0, 1], tok, [n + k for n in lens])
            rows[0].append(tok[0])
            rows[1].append(tok[1])
        assert rows == want
        # temperature 0: the greedy tokens, no coin anywhere
        t.set_batch_sampler(0.0, P, seeds)
        refs = [m.ref(60 + i, n + 1) for i, n in enumerate(lens)]
        t.batch_prefill_slots([1, 0], [p[:-1] for p in prompts], [0, 0])
        tok = t.batch_step_cols_draw([1, 0], [p[-1] for p in prompts], list(lens))
        assert tok == [r["first"] for r in refs]


LOOP_LEN, LOOP_NEW = [3, 40, 90, 1, 130, 33], [2, 6, 1, 4, 3, 5]


@pytest.fixture(scope="module")
def loop_rows(q3, models):
    """the six requests on two slots through the column loops, once"""
    m = models()
    prompts = [m.prompt(70 + r, n) for r, n in enumerate(LOOP_LEN)]
    T, P, S = [0.8, 0.0, 0.7, 0.9, 0.8, 0.6], [0.9, 0.9, 0.95, 1.0, 0.9, 0.8], [11, 12, 13, 14, 15, 16]
    with m.engine() as t:
        t.batch_init(2)
        greedy, _ = t.generate_many_greedy(prompts, LOOP_NEW)
        sampled, _ = t.generate_many_sampled(prompts, LOOP_NEW, T, P, S)
    return prompts, greedy, sampled, (T, P, S)


@pytest.mark.parametrize("dense_min", [0, 1, 32, 64])
def test_the_loop(q3, models, loop_rows, dense_min):
    m = models()
    prompts, greedy, sampled, smp = loop_rows
    assert greedy[1] == [m.ref(71, 40)["first"]] + m.ref(71, 40)["more"]          # the loop's own yardstick is the sequential path
    dense = [r for r, n in enumerate(LOOP_LEN) if dense_min and n - 1 >= dense_min]
    with m.engine() as t:
        t.batch_init(2)
        rows, st, ds = t.generate_many_dense(prompts, LOOP_NEW, None, dense_min)
        assert rows == greedy
        assert ds.live_columns == sum(LOOP_LEN[r] - 1 for r in dense) and (ds.blocks == 0) == (not dense)
        want_st = q3.cols_schedule([1 if r in dense else n for r, n in enumerate(LOOP_LEN)], LOOP_NEW, 2)[1]
        assert st == want_st
        rows, _, ds2 = t.generate_many_dense(prompts, LOOP_NEW, smp, dense_min)
        assert rows == sampled
        assert ds2 == ds
        if dense_min == 32:              # the front end passes it through
            assert q3.generate_many(t, prompts, 3, dense_min=dense_min)[0] == q3.generate_many(t, prompts, 3)[0]


def test_nothing_else_moved(q3, models):
    """after a dense call, the batched decode, a column pass and the single-cache dense prefill of the same engine give their results"""
    m = models()
    a, b, c = m.ref(81, 60), m.ref(82, 45), m.ref(83, 50)
    with m.engine() as t:
        t.batch_init(3)
        t.batch_prefill_slots([0], [a["prompt"][:-1]], [0])                     # nothing but a dense block so far
        lg, am = t.batch_step_cols([0], [a["prompt"][-1]], [59], want_logits=True)
        assert_biteq(lg[0], a["logits"], "column pass behind a dense block")
        out = t.generate_greedy_batch([a["first"]], [60], N_MORE)
        assert [int(v) for v in out[0]] == a["more"]
        t.batch_prefill_slots([2, 1], [b["prompt"][:-1], c["prompt"][:-1]], [0, 0])
        out = t.generate_greedy_batch([a["more"][-1]], [60 + N_MORE], 1)        # slot 0 goes on where it was
        with m.engine() as s:
            s.prefill(a["prompt"], 0)
            assert int(out[0][0]) == [int(v) for v in s.generate_greedy(a["first"], 60, N_MORE + 1)][-1]
        finish(q3, t, [2, 1], [b, c], "two more slots")
        assert t.prefill(c["prompt"], 0, batched=True) == c["first"]
        cfg = t.get_config()
        kvd = cfg.n_kv_heads * cfg.head_dim
        assert_biteq(t.read_state("key").reshape(cfg.n_layers, CTX, kvd)[:, :50], c["key"], "q3_prefill_batched key rows")


def test_errors_leave_the_engine_usable(q3, models):
    m = models()
    r = m.ref(91, 41)
    p = r["prompt"][:-1]
    with m.engine() as t:
        with pytest.raises(IndexError):
            t.batch_prefill_slots([0], [p], [0])                                 # no batch_init
        t.batch_init(2)
        for slots, prompts, first in (([2], [p], [0]), ([-1], [p], [0]), ([0, 0], [p, p], [0, 0]), ([0, 1], [p, []], [0, 0]),
                                      ([0], [p], [CTX - 39]), ([0], [p], [CTX]), ([0], [p], [-1]),
                                      ([0], [p[:5] + [m.shape.vocab_size]], [0]), ([0], [[-1] + p], [0]), ([], [], [])):
            with pytest.raises(IndexError):
                t.batch_prefill_slots(slots, prompts, first)
        k, v = slot_rows(t, 0)
        assert not k.any() and not v.any()
        with pytest.raises(IndexError):
            t.generate_many_dense([p, []], [1, 1], None, 8)
        with pytest.raises(IndexError):
            t.generate_many_dense([p], [0], None, 8)
        t.batch_prefill_slots([1], [p], [0])
        check_rows(t, 1, r, 40, "a correct call behind the refused ones")
        finish(q3, t, [1], [r], "behind the refused calls")
    with m.engine(fast=True) as t:
        t.batch_init(2)
        with pytest.raises(q3.Q3Error) as ei:
            t.batch_prefill_slots([0], [p], [0])
        assert ei.value.code == -5
        with pytest.raises(q3.Q3Error) as ei:
            t.generate_many_dense([p], [2], None, 8)
        assert ei.value.code == -5
