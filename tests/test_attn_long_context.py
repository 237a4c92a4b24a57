"""The batched paths at contexts whose score rows no longer fit LDS: k_attn_gqa2g<2 | 4 | 5> (8 query heads per kv head: two parts
of 4), which keeps them in global scratch.  The yardstick is a fresh single-stream engine of the same context walking ONE prompt P of
S tokens (test_dense_slots.Model's sequential path: prefill between the recorded positions, forward at them); every slot holds a
prefix of P, so one walk per shape serves every test.  Every comparison is bit for bit."""
import numpy as np
import pytest

from conftest import assert_biteq
from test_dense_slots import N_MORE, slot_rows
from test_head_groups import ShapeModel, load_cols

pytestmark = pytest.mark.gpu

# name -> (query heads, dim, context).  2 kv heads, head_dim 128, 2 layers, vocabulary 512, group 64.  The context is the smallest
# multiple of 256 at which attn_gqa_smem_bytes(128, heads per workgroup, S) = 4 * ((h + 1) * 384 + h * S + tch * 132) exceeds
# 150 KB = 38,400 floats (tch 64; 32 for h = 2).  Recomputed: h = 4: S <= 7,008 fits, so 6,912 and then 7,168; h = 5: S <= 5,529, so
# 5,376 and then 5,632; h = 2: S <= 16,512, so 16,384 and then 16,640.  k_attn_gqa2 needs more LDS than k_attn_gqa, so neither fits.
SHAPES = {"g4": (8, 512, 7168), "g8": (16, 512, 7168), "g5": (10, 512, 5632), "g2": (4, 256, 16640)}
N_GREEDY = 1 + N_MORE


class LongModel(ShapeModel):
    def positions(self):
        S = self.ctx
        return sorted({0, 63, 64, 256, 300, S - 301, S - 41, S - 3, S - 2, S - 1})

    def walk(self):
        """dict(P, logits[p] = forward(P[p], p) over rows 0 .. p-1 of P, greedy[p] = the N_GREEDY greedy tokens behind P[:p + 1]
        (where they end inside the context), key / value [L, S, kvd] of all of P)"""
        if "walk" not in self._refs:
            S = self.ctx
            P, logits, greedy, at = self.prompt(77, S), {}, {}, 0
            with self.engine() as t:
                for p in self.positions():
                    if p > at:
                        t.prefill(P[at:p], at)
                    if p + N_GREEDY <= S:        # an excursion over rows p ..: the walk writes them again before it reads them
                        greedy[p] = [int(v) for v in t.generate_greedy(P[p], p, N_GREEDY)]
                    logits[p] = np.array(t.forward(P[p], p), copy=True)
                    at = p + 1
                c = t.get_config()
                kv = [t.read_state(k).reshape(c.n_layers, S, c.n_kv_heads * c.head_dim) for k in ("key", "value")]
            self._refs["walk"] = dict(P=P, logits=logits, greedy=greedy, key=kv[0], value=kv[1])
        return self._refs["walk"]


@pytest.fixture(scope="module")
def models(q3, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            heads, dim, ctx = SHAPES[name]
            shape = q3.checkpoint.ModelShape(dim, 2 * dim, 2, heads, 2, 512, ctx, 128, True, 64)
            path = str(tmp_path_factory.mktemp("longctx") / f"{name}.bin")
            q3.checkpoint.write_synthetic_checkpoint(path, shape, seed=9753)
            made[name] = LongModel(q3, shape, path, ctx)
        return made[name]
    return get


def check_slot(t, m, r, slot, n, what):
    """rows 0 .. n-1 of the slot are P's, every later row is still zero"""
    for rows, kind in zip(slot_rows(t, slot, m.ctx), ("key", "value")):
        assert_biteq(rows[:, :n], r[kind][:, :n], f"{what}: {kind} rows")
        assert not rows[:, n:].any(), f"{what}: {kind} rows past {n} written"


@pytest.mark.parametrize("name", list(SHAPES))
def test_column_passes(q3, models, name):
    m = models(name)
    r, S = m.walk(), m.ctx
    P = r["P"]
    assert (S - 300) % 64 and (S - 300) % 256           # the long row ends inside a chunk and inside a block of the exact sum
    lens = (1, 64, 65, 257, S - 300, S)
    with m.engine() as t:
        t.batch_init(7)
        for s, n in enumerate(lens[:4]):
            load_cols(t, s, P[:n - 1])
        t.batch_prefill_slots([4, 5, 6], [P[:S - 301], P[:S - 1], P[:S - 3]], [0, 0, 0])
        lg, am = t.batch_step_cols(list(range(6)), [P[n - 1] for n in lens], [n - 1 for n in lens], want_logits=True)
        for s, n in enumerate(lens):
            assert_biteq(lg[s], r["logits"][n - 1], f"slot {s} ({n} rows): logits")
            assert am[s] == q3.sample_argmax(r["logits"][n - 1])
            check_slot(t, m, r, s, n, f"slot {s}")
        # three consecutive columns of one slot: the later ones attend to rows the earlier ones wrote in this pass
        lg, _ = t.batch_step_cols([6] * 3, P[S - 3:], [S - 3, S - 2, S - 1], want_logits=True)
        for j, p in enumerate((S - 3, S - 2, S - 1)):
            assert_biteq(lg[j], r["logits"][p], f"run column {j}: logits")
        check_slot(t, m, r, 6, S, "run")


@pytest.mark.parametrize("name", ["g4", "g8"])
def test_batched_decode(q3, models, name):
    """q3_forward_batch: the attention kernel forms the position's key row itself, patches it into the staged chunk and (8 heads:
    part 0 alone) stores it.  The parent served this through k_attn_streams."""
    m = models(name)
    r, S = m.walk(), m.ctx
    P, pos = r["P"], (64, 300, S - 1)
    with m.engine() as t:
        t.batch_init(3)
        load_cols(t, 0, P[:64])
        load_cols(t, 1, P[:300])
        t.batch_prefill_slots([2], [P[:S - 1]], [0])
        lg, am = t.forward_batch([P[p] for p in pos], pos)
        for s, p in enumerate(pos):
            assert_biteq(lg[s], r["logits"][p], f"stream {s}: logits")
            check_slot(t, m, r, s, p + 1, f"stream {s}")
        assert am[:2] == [r["greedy"][64][0], r["greedy"][300][0]]
        out = t.generate_greedy_batch(am[:2], [65, 301], N_MORE)
        assert [[int(v) for v in row] for row in out] == [r["greedy"][64][1:], r["greedy"][300][1:]]


@pytest.mark.parametrize("name", ["g4", "g5"])
def test_verify_and_generate_many(q3, models, name):
    m = models(name)
    r, S = m.walk(), m.ctx
    P, g = r["P"], r["greedy"]
    p = S - 41                                          # past the longest context the LDS rows allowed
    with m.engine() as t:
        t.prefill(P[:p], 0, batched=True)               # the prefill-only context
        nxt, n_acc = t.verify([P[p]] + g[p][:3], p)
        assert (list(nxt), n_acc) == (g[p][:4], 3)
        t.batch_init(2)                                 # three requests through two slots
        rows, _ = t.generate_many_greedy([P[:p + 1], P[:65], P[:257]], [4, 4, 4])
        assert rows == [g[p][:4], g[64][:4], g[256][:4]]
