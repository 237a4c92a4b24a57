"""Q4 checkpoints on the host: nibble layout, quantizer, headers, sizes, expansion and the exporter (no GPU)."""
import dataclasses
import os
import struct

import numpy as np
import pytest

from test_export import build_model_dir

f32 = np.float32

def test_pack_layout_and_inverse(q3):
    ck = q3.checkpoint
    run = np.array([1, 2, 3, 4, 5, 6, 7, -8, -1, -2, -3, -4, -5, -6, -7, 0], np.int8)     # columns c0 .. c15
    want = np.array([0x51, 0x62, 0x73, 0x84, 0xBF, 0xAE, 0x9D, 0x0C], np.uint8)
    assert ck.pack_q4(run).tolist() == want.tolist()
    every = np.array([(i + 3 * k) % 16 - 8 for k in range(16) for i in range(16)], np.int8)   # each value in each column
    assert np.array_equal(ck.unpack_q4(ck.pack_q4(every)), every)

def test_quantize_q40_known_answers(q3):
    ck = q3.checkpoint
    g = np.array([7, -7, 3, 0, 1, -2, 5, -6] * 2, f32)
    q, s, err = ck.quantize_q40(np.concatenate([g, np.zeros(16, f32)]), 16)
    assert s.tolist() == [1.0, 1.0] and q[:16].tolist() == g.tolist() and not q[16:].any() and err == 0.0
    h = np.array([7, 0.5, 1.5, 2.5, -0.5, -1.5, 3.5, 6.5] + [0] * 8, f32)              # quotients at half integers: to even
    assert ck.quantize_q40(h, 16)[0][:8].tolist() == [7, 0, 2, 2, 0, -2, 4, 6]

@pytest.mark.parametrize("name", ["tiny", "small-hd128"])
def test_header_size_and_expansion(q3, oracle, tmp_path, name):
    ck = q3.checkpoint
    s4 = dataclasses.replace(ck.SHAPES[name], weight_bits=4)
    p4, p8 = str(tmp_path / "q4.bin"), str(tmp_path / "q8.bin")
    assert ck.write_synthetic_checkpoint(p4, s4, seed=9, sparse_zero_groups=True) == os.path.getsize(p4) == s4.file_size()
    raw = open(p4, "rb").read()
    assert struct.unpack("<Ii", raw[:8]) == (0x616A6334, 1)
    assert ck.read_header(p4) == s4
    assert q3.engine.parse_header(raw[:256]).dim == s4.dim
    with pytest.raises(Exception, match="magic"):
        oracle.read_config(raw[:256])
    s8 = ck.expand_q4_checkpoint(p4, p8)
    assert s8 == ck.SHAPES[name] and os.path.getsize(p8) == s8.file_size()
    assert oracle.OracleModel(p8).config.dim == s8.dim
    o4, o8 = ck.tensor_offsets(s4), ck.tensor_offsets(s8)
    exp = open(p8, "rb").read()
    for tname, cnt, rows, cols in s4.quantized_tensors():
        size = rows * cols
        (q4o, s4o, st4), (q8o, s8o, st8) = o4[tname], o8[tname]
        for i in (0, cnt - 1):
            assert raw[s4o + i * st4: s4o + i * st4 + 4 * (size // s4.group_size)] == exp[s8o + i * st8: s8o + i * st8 + 4 * (size // s4.group_size)]
            q8 = np.frombuffer(exp, np.int8, size, q8o + i * st8)
            if s4.tensor_bits(tname) == 4:
                assert np.array_equal(q8, ck.unpack_q4(np.frombuffer(raw, np.uint8, size // 2, q4o + i * st4)))
                assert q8.min() >= -7 and q8.max() <= 7
            else:
                assert raw[q4o + i * st4: q4o + i * st4 + size] == q8.tobytes()

def test_export_weight_bits_4(q3, tmp_path):
    from qwen3_rs_amd import export as ex
    ck = q3.checkpoint
    d = str(tmp_path / "hf")
    want = build_model_dir(d, tied=True, with_qk_norm=True)
    p8, p4 = str(tmp_path / "m8.bin"), str(tmp_path / "m4.bin")
    s8 = ex.export_model(d, p8)
    s4 = ex.export_model(d, p4, weight_bits=4)
    assert s4.weight_bits == 4 and ck.read_header(p4) == s4 and os.path.getsize(p4) == s4.file_size()
    b8, b4 = open(p8, "rb").read(), open(p4, "rb").read()
    o8, o4 = ck.tensor_offsets(s8), ck.tensor_offsets(s4)
    n_emb = o8["q_proj"][0] - 256                              # the norms and the embedding: byte for byte the 8-bit export
    assert b4[256:256 + n_emb] == b8[256:256 + n_emb] and o4["q_proj"][0] == o8["q_proj"][0]
    w = np.asarray(want["model.layers.1.mlp.down_proj.weight"], f32).reshape(-1)
    q, s, _ = ck.quantize_q40(w, s4.group_size)
    qo, so, st = o4["down_proj"]
    assert b4[qo + st: qo + st + w.size // 2] == ck.pack_q4(q).tobytes()
    assert b4[so + st: so + st + 4 * s.size] == s.astype("<f4").tobytes()
