"""Embeddings (include/qwen3_hip.h section 2j): what can be checked without a GPU -- the entry point's first refusal, the command
line's parser, and the numpy restatement of the L2 part that tests/test_embed.py holds the kernel to."""
import ctypes as C

import numpy as np

import embed_ref
from conftest import golden_path


def test_a_null_engine_is_refused_before_anything_touches_the_gpu(q3):
    lib = q3.load_library()
    lens = (C.c_size_t * 1)(3)
    toks = (C.c_int32 * 3)(1, 2, 3)
    out = (C.c_float * 8)()
    assert lib.q3_embed_many(None, toks, lens, 1, 0, 0, out, None) == -3
    assert b"null engine" in lib.q3_last_error()
    assert "q3_embed_many" in q3.EXPORTED_SYMBOLS


def test_the_command_line_knows_the_embed_verb(q3):
    from qwen3_rs_amd import cli
    a = cli.build_parser().parse_args(["embed", "model.bin", "-i", "one", "-i", "two", "--instruct", "Given a query", "--dim", "32",
                                       "--no-normalize", "--append-token", "7", "-o", "out.npy", "--streams", "4", "--context", "128"])
    assert (a.cmd, a.checkpoint, a.input, a.instruct, a.dim) == ("embed", "model.bin", ["one", "two"], "Given a query", 32)
    assert (a.no_normalize, a.append_token, a.output, a.streams, a.context) == (True, 7, "out.npy", 4, 128)
    b = cli.build_parser().parse_args(["embed", "model.bin", "-i", "one"])
    assert (b.dim, b.no_normalize, b.append_token, b.output, b.instruct) == (None, False, None, None, None)


def test_embed_ref_on_hand_made_vectors():
    # 64 ones: s2 = 64 and nrm = 8 exactly, every component 0.125; the norm of the result within 2 ulp of 1
    out = embed_ref.l2_row(np.ones(64, dtype=np.float32))
    assert out.dtype == np.float32 and np.array_equal(out, np.full(64, 0.125, dtype=np.float32))
    assert abs(float(np.sqrt(np.sum(out.astype(np.float64) ** 2))) - 1.0) <= 2 * 2.0 ** -23
    # truncation normalises the leading sub-vector alone
    v = np.array([3.0, 4.0, 100.0], dtype=np.float32)
    assert np.array_equal(embed_ref.l2_row(v, 2), np.array([0.6, 0.8], dtype=np.float32))
    # the sum is the left fold from -0.0: an empty or all -0.0 run keeps the sign, and the order is the sequential one
    assert np.signbit(embed_ref.seq_sum(np.zeros(0, dtype=np.float32)))
    t = np.array([1.0, 2.0 ** -24, 2.0 ** -24], dtype=np.float32)
    assert embed_ref.seq_sum(t) == np.float32(1.0) and embed_ref.seq_sum(t[::-1]) > np.float32(1.0)
    # eps: an all-zero vector stays zero (0 / 1e-12); the squares of 1e-30 underflow to 0, so the divisor is the eps
    assert np.array_equal(embed_ref.l2_row(np.zeros(16, dtype=np.float32)), np.zeros(16, dtype=np.float32))
    small = np.full(16, 1e-30, dtype=np.float32)
    assert np.array_equal(embed_ref.l2_row(small), small / np.float32(1e-12))
    # a NaN norm takes the eps as well: the comparison is false
    bad = np.array([np.nan, 1.0], dtype=np.float32)
    got = embed_ref.l2_row(bad)
    assert np.isnan(got[0]) and got[1] == np.float32(1.0) / np.float32(1e-12)


def test_the_oracle_tap_gives_unit_rows(oracle):
    """tap_x() of the tiny golden checkpoint -- the final RMSNorm of the last token forwarded -- through embed_ref: finite rows whose
    norm is 1 up to the rounding of dim sequential adds, one square root and one divide per component"""
    om = oracle.OracleModel(golden_path("tiny.bin"))
    dim = om.get_config().dim
    rows = []
    for prompt in ([5], [1, 2, 3, 4], [200, 17, 17, 3, 90, 41, 8]):
        om.reset()
        for pos, tok in enumerate(prompt):
            om.forward(tok, pos)
        rows.append(om.tap_x())
    out = embed_ref.l2(np.stack(rows))
    assert out.shape == (3, dim) and np.isfinite(out).all()
    norms = np.sqrt(np.sum(out.astype(np.float64) ** 2, axis=1))
    assert np.all(np.abs(norms - 1.0) <= (dim + 2) * 2.0 ** -24)
    cut = embed_ref.l2(np.stack(rows), 24)
    assert cut.shape == (3, 24) and np.all(np.abs(np.sqrt(np.sum(cut.astype(np.float64) ** 2, axis=1)) - 1.0) <= 26 * 2.0 ** -24)
