"""The batched paths at 8 and 5 query heads per kv head, head_dim 128 (the layouts of Qwen3-32B and 14B).  8: the per-kv-head
attention kernels as two workgroups of 4 heads per kv group, k_attn_pf2<8, NP> in dense blocks.  5: k_attn_pf2<5, 4> in dense blocks,
its fifth head paired across two positions (column passes stay on the generic k_attn_gqa<0, 0>).  The yardstick is a fresh
single-stream engine (test_dense_slots.Model), itself held to the C oracle here; every comparison is bit for bit."""
import numpy as np
import pytest

import score_ref
from conftest import assert_biteq
from test_dense_slots import CTX, N_MORE, Model, check_rows, finish, slot_rows

pytestmark = pytest.mark.gpu

COL_LENS = (1, 63, 64, 65, 130, 300)        # the 64-timestep chunk and the 256-entry block of the exact sum, from both sides
# name -> (shape, context).  long: score rows that fit k_attn_gqa's LDS and not k_attn_gqa2's two tiles (4,864 < 5,120 <= 6,912:
# attn_gqa_smem_bytes / attn_gqa2_smem_bytes against 150 KB); wide: one layer of Qwen3-32B's widths, longer than any listed model's
SHAPES = {"small": ("small-kvm8", CTX), "small5": ("small-kvm5", CTX), "long": ((512, 1024, 2, 16, 2, 2048, 5120, 128, True, 64), 5120),
          "wide": ((5120, 25600, 1, 64, 8, 4096, 256, 128, False, 64), 256), "wide5": ((5120, 17408, 1, 40, 8, 4096, 256, 128, False, 64), 256)}
SMALL = ("small5", "small")


class ShapeModel(Model):
    """test_dense_slots.Model of a ModelShape"""

    def __init__(self, q3, shape, path, ctx):
        self.q3, self.shape, self.path, self.ctx, self._refs = q3, shape, path, ctx, {}


@pytest.fixture(scope="module")
def models(q3, tmp_path_factory):
    made = {}

    def get(name="small"):
        if name not in made:
            spec, ctx = SHAPES[name]
            shape = q3.checkpoint.SHAPES[spec] if isinstance(spec, str) else q3.checkpoint.ModelShape(*spec)
            path = str(tmp_path_factory.mktemp("heads") / f"{name}.bin")
            q3.checkpoint.write_synthetic_checkpoint(path, shape, seed=8642)
            made[name] = ShapeModel(q3, shape, path, ctx)
        return made[name]
    return get


def load_cols(t, slot, toks):
    """toks into rows 0.. of `slot`, through column passes of up to 32 columns"""
    for i in range(0, len(toks), 32):
        c = toks[i:i + 32]
        t.batch_step_cols([slot] * len(c), c, list(range(i, i + len(c))))


@pytest.mark.parametrize("name", SMALL)
def test_forward_matches_the_oracle(q3, oracle, models, name):
    m = models(name)
    om = oracle.OracleModel(m.path)
    with m.engine() as t:
        for pos, tok in enumerate(m.prompt(1, 3)):
            assert_biteq(np.array(t.forward(tok, pos), copy=True), om.forward(tok, pos), f"logits at position {pos}")


def test_column_passes(q3, models):
    m = models()
    refs = [m.ref(200 + i, n) for i, n in enumerate(COL_LENS)]
    prompts, slots = [r["prompt"] for r in refs], list(range(len(refs)))
    with m.engine() as t:
        t.batch_init(len(refs))
        for s, r in zip(slots, refs):
            load_cols(t, s, r["prompt"][:-1])
            check_rows(t, s, r, len(r["prompt"]) - 1, f"slot {s}")
        finish(q3, t, slots, refs, "column passes")
        t.batch_init(3)                                          # six requests through three slots
        rows, _ = t.generate_many_greedy(prompts, [1 + N_MORE] * len(refs))
        assert rows == [[r["first"]] + r["more"] for r in refs]
        T, P, seeds = 0.8, 0.9, [31, 32, 33, 34, 35, 36]
        rows, _ = t.generate_many_sampled(prompts, [4] * len(refs), T, P, seeds)
        assert rows == [m.ref_sampled(200 + i, n, T, P, seeds[i], 4) for i, n in enumerate(COL_LENS)]


@pytest.mark.parametrize("name, lens", [("small", (65, 130, 300)), ("long", (65, 130))])
def test_batched_decode(q3, models, name, lens):
    """streams at different positions through q3_forward_batch: the attention kernel forms the key row itself and one of the kv
    group's two workgroups stores it.  small: k_attn_gqa2<4>; long (a context of 5,120): k_attn_gqa<128, 4>"""
    m = models(name)
    refs = [m.ref(200 + n, n) for n in lens]
    with m.engine() as t:
        t.batch_init(len(refs))
        for s, r in enumerate(refs):
            load_cols(t, s, r["prompt"][:-1])
        lg, am = t.forward_batch([r["prompt"][-1] for r in refs], [n - 1 for n in lens])
        for s, (r, n) in enumerate(zip(refs, lens)):
            assert_biteq(lg[s], r["logits"], f"stream {s}: logits")
            for rows, kind in zip(slot_rows(t, s, m.ctx), ("key", "value")):     # both kv heads, the row this step wrote included
                assert_biteq(rows[:, :n], r[kind], f"stream {s}: {kind} rows")
                assert not rows[:, n:].any()
        assert am == [r["first"] for r in refs]
        out = t.generate_greedy_batch(am, list(lens), N_MORE)
        assert [[int(v) for v in row] for row in out] == [r["more"] for r in refs]


@pytest.mark.parametrize("n, first", [(33, 0), (127, 0), (128, 0), (129, 0), (257, 0), (300, 0), (300, 1)])
@pytest.mark.parametrize("name", SMALL)
def test_dense_prefill(q3, models, name, n, first):
    """q3_prefill_batched up to position n: the cache rows, then forward's logits and the greedy tokens behind token n + 1.  5 per kv
    head: an odd block ends in a wave alone on its first row; first = 1 pairs positions 127 | 128 and 255 | 256 in one wave -- row a
    ends with a chunk, row b starts the next one"""
    m = models(name)
    r = m.ref(300 + n, n + 1)
    with m.engine() as t:
        if first:
            t.prefill(r["prompt"][:first], 0)
        t.prefill(r["prompt"][first:-1], first, batched=True)
        cfg = t.get_config()
        for kind in ("key", "value"):
            rows = t.read_state(kind).reshape(cfg.n_layers, CTX, cfg.n_kv_heads * cfg.head_dim)
            assert_biteq(rows[:, :n], r[kind][:, :n], f"{kind} rows")
            assert not rows[:, n:].any()
        assert_biteq(np.array(t.forward(r["prompt"][-1], n), copy=True), r["logits"], "logits behind the block")
        assert [int(v) for v in t.generate_greedy(r["first"], n + 1, N_MORE)] == r["more"]


@pytest.mark.parametrize("lens", [(41, 1, 22), (300, 250)], ids=lambda v: "+".join(map(str, v)))
@pytest.mark.parametrize("name", SMALL)
def test_runs_share_a_block(q3, models, name, lens):
    """41 + 1 + 22: columns 0-40, 48 and 56-77 of 80, a run of one column and one that ends on an odd column (k_attn_pf2<8, 2>);
    300 + 250: 554 columns over 2 kv heads, enough workgroups for 4 positions each (k_attn_pf2<8, 4>).  5 per kv head: the pad columns
    repeat a run's last one, so columns 40 | 41 and 48 | 49 are cross-position pairs of equal positions; one block, not 32 columns at
    a time"""
    m = models(name)
    slots = [2, 0, 3][:len(lens)]
    refs = [m.ref(400 + k, k + 1) for k in lens]
    with m.engine() as t:
        t.batch_init(4)
        st = t.batch_prefill_slots(slots, [r["prompt"][:-1] for r in refs], [0] * len(lens))
        assert st == q3.dense_pack(list(lens), 2048)[1] and (st.blocks, st.live_columns) == (1, sum(lens))
        for s, r, k in zip(slots, refs, lens):
            check_rows(t, s, r, k, f"slot {s}")
        k, v = slot_rows(t, 1)
        assert not k.any() and not v.any()
        finish(q3, t, slots, refs, str(lens))


@pytest.mark.parametrize("name", SMALL)
def test_embed_and_score(q3, models, name):
    m = models(name)
    prompts = [m.prompt(500 + i, n) for i, n in enumerate((1, 9, 300, 66))]
    want_x, want_r = [], []
    with m.engine() as t:
        for p in prompts:
            t.reset_kv()
            rows = [np.array(t.forward(tok, i), copy=True) for i, tok in enumerate(p)]
            want_x.append(t.read_state("x").copy())
            want_r.append(score_ref.records(rows[:-1], p[1:]))
    with m.engine() as t:
        t.batch_init(4)
        x, est = t.embed_many(prompts, normalize=False)
        recs, sst = t.score_many(prompts)
        for i in range(len(prompts)):
            assert_biteq(x[i], want_x[i], f"embedding of request {i}")
            score_ref.assert_records(recs[i], want_r[i], f"records of request {i}")
        assert est.blocks == 1 and sst.blocks == 1              # the 300-token prompt and its neighbours: one dense block


@pytest.mark.parametrize("name", ("wide5", "wide"))
def test_real_widths(q3, models, name):
    """dim 5120, hidden 17,408 / 25,600 (the batched quantize prologues past 4,096 elements): a 40-token dense request, two column
    passes"""
    m = models(name)
    r = m.ref(600, 41)
    with m.engine() as t:
        t.batch_init(2)
        t.batch_prefill_slots([1], [r["prompt"][:-1]], [0])
        for rows, kind in zip(slot_rows(t, 1, m.ctx), ("key", "value")):
            assert_biteq(rows[:, :40], r[kind][:, :40], f"{kind} rows")
        lg, am = t.batch_step_cols([1], [r["prompt"][-1]], [40], want_logits=True)
        assert_biteq(lg[0], r["logits"], "logits behind the block")
        assert am == [r["first"]] and t.batch_step_cols([1], am, [41]) == [r["more"][0]]
