"""The batched decode matmuls on the nibbles of a Q4 checkpoint (header section 2v: the WB = 4 form of k_bgemm for QKV and W1|W3;
the residual launches run the int8 kernels on the expanded copy).  Everything is bit for bit: the launch alone against the
oracle's matmul on the unpacked nibbles, the engine against its expanded Q8 twin."""
import dataclasses
import functools
import os

import numpy as np
import pytest

from conftest import assert_biteq

pytestmark = pytest.mark.gpu
f32 = np.float32
QKV, SWIGLU, RESID = 0, 1, 2          # ROLE_NORM_QKV, ROLE_NORM_SWIGLU, ROLE_QUANT_RESID: the epilogues
# (role, n, rows, rows_kv, G) -- the smallest shapes that reach each path:
SHAPES = (
    # residual launches (int8 on the expanded nibbles): k_dgemm's ring of 8 in one iteration, ring of 16, ring of 8 in three
    # iterations; n = 256 has no ring: k_bgemm's RESID
    [(RESID, n, rows, 0, 64) for n in (512, 1024, 1536, 256) for rows in (16, 48)]
    # k_bgemm QKV: a short single phase (G 64: 8 groups), two and four MFMA steps per group; q | k | v on tile boundaries, one tile
    # per task (4 tiles) and two (320 tiles: between one and two per CU)
    + [(QKV, 512, rows, kv, G) for G in (64, 128, 256) for rows, kv in ((32, 16), (4096, 512))]
    # k_bgemm SWIGLU: 40 groups = a full phase of 16 and a tail phase of 8 whose upper waves are past the row
    + [(SWIGLU, 2560, 32, 0, 64)]
    # an odd count of 64-byte steps per row: no nibble-packed copy, the int8 kernel on the expanded copy
    + [(RESID, 192, 16, 0, 64)])


@functools.lru_cache(maxsize=None)
def case(role, n, rows, rows_kv, G):
    """operands of 32 columns and the reference output [32][rows (+ 2 rows_kv)], made once per shape"""
    from oracle import q3_oracle as oracle
    dw = rows + 2 * rows_kv if role == QKV else (2 * rows if role == SWIGLU else rows)
    ng = n // G
    rng = np.random.default_rng(n + 7 * rows + role + G)
    idx = np.arange(dw * n, dtype=np.int64).reshape(dw, n)
    wq = ((idx + idx // n * 5) % 16 - 8).astype(np.int8)                       # every nibble value, -8 included, in every column residue
    ws = (10.0 ** rng.uniform(-6, 3, (dw, ng))).astype(f32)
    wq[0, G:2 * G] = 0                                                         # an all-zero group, scale 1.0 as the exporter writes it
    ws[0, 1] = 1.0
    ws[1, :] = f32(2.0 ** -126)                                                # scales that a division by 16 would not survive
    ws[2, :] = f32(2.0 ** -123)
    xq = rng.integers(-127, 128, (32, n)).astype(np.int8)
    xq[:, 0], xq[:, 1] = 127, -127
    xs = (10.0 ** rng.uniform(-6, 3, (32, ng))).astype(f32)
    out0 = rng.standard_normal((32, rows)).astype(f32) if role == RESID else None
    want = np.stack([oracle.matmul(xq[c], xs[c], wq, ws, n, dw, G) for c in range(32)])
    if role == RESID:
        want = out0 + want
    elif role == SWIGLU:
        want = np.stack([oracle.swiglu(w[:rows].copy(), w[rows:].copy()) for w in want])
    return wq, ws, xq, xs, out0, want


@pytest.mark.parametrize("cols", [1, 16, 17, 32])
@pytest.mark.parametrize("role,n,rows,rows_kv,G", SHAPES, ids=[f"role{ro}-n{n}-r{r}-g{G}" for ro, n, r, _, G in SHAPES])
def test_bmatmul_w4(q3, oracle, role, n, rows, rows_kv, G, cols):
    wq, ws, xq, xs, out0, want = case(role, n, rows, rows_kv, G)
    r = q3.ops.bmatmul_w4(role, q3.checkpoint.pack_q4(wq), ws, xq[:cols], xs[:cols], n, rows, G, rows_kv=rows_kv,
                          out=None if out0 is None else out0[:cols])
    # the residual launches keep the int8 kernels on the expanded copy (the 4-bit form of k_dgemm lost its A/B, profiles/w4_batch.md)
    dgemm = role == RESID and G == 64 and (n // G) % 8 == 0
    assert r["info"][:2] == [1 if dgemm else 0, 4 if role != RESID and n % 128 == 0 else 8], r["info"]
    assert_biteq(r["out"], want[:cols], f"{cols} columns")


@pytest.mark.parametrize("name,G", [("small-hd128", 64), ("qwen3-0.6b-dims-l2", 64), ("small-hd128", 128)])
def test_engine_q4_vs_expanded_twin(q3, tmp_ckpt_dir, name, G):
    ck = q3.checkpoint
    s4 = dataclasses.replace(ck.SHAPES[name], weight_bits=4, group_size=G)
    p4, p8 = os.path.join(tmp_ckpt_dir, f"{name}-g{G}.q4.bin"), os.path.join(tmp_ckpt_dir, f"{name}-g{G}.q4x.bin")
    ck.ensure_synthetic_checkpoint(p4, s4, seed=37, sparse_zero_groups=True)
    ck.expand_q4_checkpoint(p4, p8)
    prompt = ck.iter_prompt_tokens(s4, 5, 40)
    ragged = [prompt[:7], prompt[3:22], prompt[10:13]]
    got = []
    for path, bits in ((p4, 4), (p8, 8)):
        with q3.TransformerBuilder(path).with_ctx_length(128).build() as t:
            assert t.batch_weight_bits == 8                                    # no batched context yet
            t.batch_init(4, 128)
            assert t.batch_weight_bits == bits
            res = [t.generate_greedy_batch([1, 2, 3, 4], [0, 0, 0, 0], 8)]
            res += [t.batch_read_state(s, "x") for s in range(4)]
            t.batch_reset_kv()
            res.append(np.concatenate(t.generate_many_greedy(ragged, [6, 3, 5])[0]))
            res += [t.batch_read_state(s, "x") for s in range(4)]
            nxt, acc = t.verify(prompt[:6], 0)
            res += [np.asarray(nxt), np.asarray([acc])]
            got.append(res)
    for i, (a, b) in enumerate(zip(*got)):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), f"result {i} differs between Q4 and its twin"
