"""k_kv_rows_bcast through q3_batch_copy_rows (include/qwen3_hip.h section 2i): rows of every layer of both caches go from one slot
to several, bit for bit, and nothing else moves.  Every slot gets a history of its own, the whole state of every slot is read
before and after the copy, and the state afterwards must equal the state before with the copied rows put in by numpy."""
import numpy as np
import pytest

from conftest import assert_biteq

pytestmark = pytest.mark.gpu

CKPT_SEED = 97531
HIST = 40            # positions 0 .. 39 of every slot hold a history
TAIL = 3             # ... and so do the last TAIL rows of the context: a copy that ends at the last row moves something


def fill(t, n_slots, vocab, ctx):
    """a different history in every slot: positions 0 .. HIST - 1 and the last TAIL positions of the context"""
    t.batch_reset_kv()
    toks = np.random.default_rng(77).integers(0, vocab, (n_slots, HIST + TAIL))
    step = 32 // n_slots
    for p0 in range(0, HIST, step):
        k = min(step, HIST - p0)
        t.batch_step_cols([s for s in range(n_slots) for _ in range(k)], [int(toks[s, p0 + i]) for s in range(n_slots) for i in range(k)],
                          [p0 + i for _ in range(n_slots) for i in range(k)])
    t.batch_step_cols([s for s in range(n_slots) for _ in range(TAIL)], [int(toks[s, HIST + i]) for s in range(n_slots) for i in range(TAIL)],
                      [ctx - TAIL + i for _ in range(n_slots) for i in range(TAIL)])


def state(t, n_slots):
    """[slot][cache][layer][position][kv_dim]"""
    c = t.get_config()
    kvd = c.n_kv_heads * c.head_dim
    return np.stack([np.stack([t.batch_read_state(s, kind).reshape(c.n_layers, t._batch_ctx, kvd) for kind in ("key", "value")])
                     for s in range(n_slots)])


def check_copy(t, n_slots, src, dst, first_pos, n_rows):
    before = state(t, n_slots)
    rows = before[src, :, :, first_pos:first_pos + n_rows]
    assert np.count_nonzero(rows.view(np.int32)) > rows.size // 2, "the source rows hold a history"
    for d in dst:
        assert not np.array_equal(before[d, :, :, first_pos:first_pos + n_rows].view(np.int32), rows.view(np.int32)), "the copy changes something"
    t.batch_copy_rows(src, dst, first_pos, n_rows)
    want = before.copy()
    for d in dst:
        want[d, :, :, first_pos:first_pos + n_rows] = rows
    after = state(t, n_slots)
    for s in range(n_slots):
        assert_biteq(after[s], want[s], f"slot {s} after copying rows {first_pos}..{first_pos + n_rows - 1} of slot {src} to {dst}")


@pytest.fixture(scope="module")
def ckpt(q3, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = str(tmp_path_factory.mktemp("prefixcopy") / f"{name}.bin")
            q3.checkpoint.write_synthetic_checkpoint(made[name], q3.checkpoint.SHAPES[name], seed=CKPT_SEED)
        return made[name]
    return get


@pytest.mark.parametrize("n_rows, first_pos, src, dst", [
    (1, 0, 0, [1]),
    (1, 39, 0, [3, 1, 2]),                                   # destinations out of order
    (7, 5, 2, [0, 3]),                                       # a tail that is no multiple of any chunk
    (40, 0, 1, [0, 2, 3]),
    (3, 93, 3, [0]),                                         # ends at the last row of the context
])
def test_copy_rows_tiny(q3, ckpt, n_rows, first_pos, src, dst):
    shape = q3.checkpoint.SHAPES["tiny-g64"]
    assert shape.max_seq_len == 96 and shape.kv_dim == 128
    with q3.TransformerBuilder(ckpt("tiny-g64")).build() as t:
        t.batch_init(4)
        fill(t, 4, shape.vocab_size, 96)
        check_copy(t, 4, src, dst, first_pos, n_rows)


def test_copy_rows_three_layers_wide_rows(q3, ckpt):
    shape = q3.checkpoint.SHAPES["small-hd128"]
    assert shape.n_layers == 3 and shape.kv_dim == 512
    with q3.TransformerBuilder(ckpt("small-hd128")).build() as t:
        t.batch_init(3)
        fill(t, 3, shape.vocab_size, shape.max_seq_len)
        check_copy(t, 3, 1, [2, 0], 4, 33)


def test_copy_rows_on_a_fast_engine(q3, ckpt):
    """it only copies: a Q3_FLAG_FAST engine takes it"""
    with q3.TransformerBuilder(ckpt("tiny-g64")).with_strict(False).build() as t:
        t.batch_init(2)
        t.forward_batch([5, 9], [0, 0], want_logits=False)
        t.forward_batch([6, 10], [1, 1], want_logits=False)
        check_copy(t, 2, 1, [0], 0, 2)


def test_errors(q3, ckpt):
    with q3.TransformerBuilder(ckpt("tiny-g64")).build() as t:
        with pytest.raises(IndexError, match="q3_batch_init"):
            t.batch_copy_rows(0, [1], 0, 1)
        t.batch_init(4, 40)
        t.batch_copy_rows(0, [1, 2, 3], 0, 40)               # max_streams - 1 destinations, the whole context: accepted
        for src, dst, first_pos, n_rows in [
                (0, [], 0, 1), (0, [1, 2, 3, 1], 0, 1),      # n_dst outside 1 .. max_streams - 1
                (4, [1], 0, 1), (-1, [1], 0, 1), (0, [4], 0, 1), (0, [-1], 0, 1),     # a slot out of range
                (1, [0, 1], 0, 1),                           # the source among the destinations
                (0, [2, 2], 0, 1),                           # a destination named twice
                (0, [1], 0, 0),                              # no row
                (0, [1], 38, 3), (0, [1], 40, 1), (0, [1], 0, 41), (0, [1], 2 ** 63, 2 ** 63)]:      # past the batch context
            with pytest.raises(IndexError):
                t.batch_copy_rows(src, dst, first_pos, n_rows)
        t.batch_init(1)
        with pytest.raises(IndexError):                      # one slot: nowhere to copy to
            t.batch_copy_rows(0, [0], 0, 1)
