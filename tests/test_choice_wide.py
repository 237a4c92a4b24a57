"""Choice logits at dim > 4096 (q3_choice_many through k_choice_norm and k_choice_stream, csrc/q3_choice.h): the dims of Qwen3-14B and
32B, a row that ends inside a KiB, and 8192 with groups of 256.  The yardstick is test_choice's: forward() of a single-stream engine
of the same context, bit for bit, and on one shape the C oracle.
No refusal test: the form takes every dim up to 16384, and the engine refuses a checkpoint above that when it is loaded."""
import numpy as np
import pytest

from conftest import assert_biteq
from test_choice import ChoiceModel, check

pytestmark = pytest.mark.gpu

CTX, V = 256, 2048
# name -> ModelShape(dim, hidden, layers, heads, kv heads, vocab, context, head_dim, shared classifier, group): one layer each
SHAPES = {"14b": (5120, 2048, 1, 40, 8, V, CTX, 128, False, 64),          # five whole KiB a row, 80 groups
          "32b-g128": (5120, 2048, 1, 64, 8, V, CTX, 128, False, 128),    # 8 lanes share a group
          "4608": (4608, 2048, 1, 16, 8, V, CTX, 128, True, 64),          # 288 pieces of 16 bytes: half of the fifth KiB
          "8192-g256": (8192, 2048, 1, 16, 8, V, CTX, 128, True, 256)}    # eight KiB, 16 lanes share a group, 32 groups
LENS = (40, 3)


@pytest.fixture(scope="module")
def models(q3, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            path = str(tmp_path_factory.mktemp("wide") / f"{name}.bin")
            if name in SHAPES:
                shape = q3.checkpoint.ModelShape(*SHAPES[name])
                q3.checkpoint.write_synthetic_checkpoint(path, shape, seed=8642)
                made[name] = ChoiceModel(q3, name, path, CTX, shape=shape)
            else:
                q3.checkpoint.write_synthetic_checkpoint(path, q3.checkpoint.SHAPES[name], seed=2468)
                made[name] = ChoiceModel(q3, name, path)
        return made[name]
    return get


def ids(m, k):
    """the first and the last row of the matrix in front; k = 256: 128 descending ids, twice"""
    v = m.shape.vocab_size
    return list(range(v - 1, v - 129, -1)) * 2 if k == 256 else ([v - 1, 0] + m.ids(600 + k, k))[:k]


def rows_of(m, refs, cands):
    with m.engine() as t:
        t.batch_init(2)
        return t.choice_many([r["prompt"] for r in refs], cands)[0]


@pytest.mark.parametrize("k", [1, 2, 33, 256])
@pytest.mark.parametrize("name", SHAPES)
def test_one_block(q3, models, name, k):
    """prompts of 40 and 3 tokens in one block (groups of 64; the others walk 32 columns at a time, the long prompt over two blocks);
    k = 33 crosses the part of 32 candidates, 256 is eight parts"""
    m = models(name)
    assert m.shape.dim > 4096
    refs, cands = m.by_len(100, LENS), ids(m, k)
    check(rows_of(m, refs, cands), refs, cands, f"{name}, k = {k}")


@pytest.mark.parametrize("name", SHAPES)
def test_per_request_lists_and_more_requests_than_slots(q3, models, name):
    m = models(name)
    refs = m.by_len(100, LENS + (9,))
    prompts = [r["prompt"] for r in refs]
    cands = [m.ids(700 + i, 5) for i in range(3)]
    with m.engine() as t:
        t.batch_init(2)
        rows, st = t.choice_many(prompts, cands)
        assert st.waves == 2
        check(rows, refs, cands, f"{name}: per-request lists", per_request=True)
        one, _ = t.choice_many(prompts, cands[0])                # the shared form behind it, same buffers
        check(one, refs, cands[0], f"{name}: the shared list")


def test_against_the_cpu_oracle(q3, oracle, models):
    m = models("14b")
    refs, cands = m.by_len(100, LENS), ids(m, 33)
    rows = rows_of(m, refs, cands)
    om = oracle.OracleModel(m.path, m.ctx)
    for i, r in enumerate(refs):
        om.reset()
        for pos, tok in enumerate(r["prompt"]):
            want = np.array(om.forward(tok, pos), copy=True)
        assert_biteq(rows[i], want[cands], f"request {i} against the oracle")


def test_dim_4096_is_unchanged(q3, models):
    """the largest dim of k_choice_rows, which this form leaves alone: forward()'s bits as before"""
    m = models("qwen3-8b-dims-l2")
    assert m.shape.dim == 4096
    refs, cands = m.by_len(100, LENS), ids(m, 33)
    check(rows_of(m, refs, cands), refs, cands, "dim 4096")
