"""A plan the kernels refuse is refused every time it is asked for: a build that fails half-way leaves no plan and no key behind,
so the same call on the same width never finds a half-built launch list to enqueue.  The shape is the one the short prefill
block refuses (8 query heads per kv head: no per-kv-head attention kernel); every call here ends before its first launch."""
import pytest

pytestmark = pytest.mark.gpu


def refused(q3, call):
    with pytest.raises(q3.Q3Error) as ei:
        call()
    assert ei.value.code == -5 and "per-kv-head attention kernel" in ei.value.msg


def test_refused_block_plans_stay_refused(q3, tmp_path):
    ck = q3.checkpoint
    path = str(tmp_path / "kvmul8.bin")
    ck.write_synthetic_checkpoint(path, ck.ModelShape(256, 384, 2, 8, 1, 512, 96, 64, True, 64), seed=5)
    with q3.TransformerBuilder(path).build() as t:
        for _ in range(2):                       # the prefill-only context of the first call, then the batched state
            for _ in range(2):
                refused(q3, lambda: t.verify([1, 2, 3, 4], 0))
            for _ in range(2):
                refused(q3, lambda: t.prefill([1, 2, 3, 4, 5], batched=True))
            t.batch_init(2)
