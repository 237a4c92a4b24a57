"""Q4 checkpoints on the GPU (header section 2v): a Q4 file computes, bit for bit, what its expanded Q8 file computes."""
import dataclasses
import os

import numpy as np
import pytest

import ref64
from conftest import assert_biteq

pytestmark = pytest.mark.gpu
f32 = np.float32
QKV, SWIGLU, QUANT, PREQR = range(4)
# (n, rows, group): generic and listed contraction lengths, rows that are not a whole number of wave-loads, a tail batch
CASES = [(64, 48, 16), (192, 40, 32), (384, 5, 64), (512, 64, 128), (1024, 64, 256), (1024, 2048, 64), (2560, 512, 64),
         (4096, 256, 64), (2048, 256, 64), (3072, 256, 64), (9728, 128, 64), (12288, 128, 64)]
LISTED = {QKV: (1024, 2560, 4096), SWIGLU: (1024, 2560, 4096), QUANT: (3072, 9728, 12288, 2048, 4096), PREQR: (2048, 4096)}
ROLE_CASES = [(role, n, rows, G) for n, rows, G in CASES for role in (QKV, SWIGLU, QUANT, PREQR) if role != PREQR or n in LISTED[PREQR]]

def q4_pair(ck, name, tmp_ckpt_dir, seed=31):
    s4 = dataclasses.replace(ck.SHAPES[name], weight_bits=4)
    p4, p8 = os.path.join(tmp_ckpt_dir, f"{name}.q4.bin"), os.path.join(tmp_ckpt_dir, f"{name}.q4x.bin")
    ck.ensure_synthetic_checkpoint(p4, s4, seed=seed, sparse_zero_groups=True)
    if not os.path.exists(p8):
        ck.expand_q4_checkpoint(p4, p8)
    return p4, p8

@pytest.mark.parametrize("strict", [True, False], ids=["strict", "fast"])
@pytest.mark.parametrize("role,n,rows,G", ROLE_CASES, ids=[f"role{ro}-n{n}-r{r}-g{G}" for ro, n, r, G in ROLE_CASES])
def test_gemv_role_w4(q3, oracle, role, n, rows, G, strict):
    """W4 launch against the int8 launch on the unpacked weights: bit-equal; tolerance mode: float64 with test_tolerance_mode's budgets"""
    ck, ops = q3.checkpoint, q3.ops
    hd = 8 if rows < 128 else 64
    if role == QKV:
        rows = max(rows, 8)                                    # q | k | v segments are whole heads: no odd row count
    rows_kv = hd * max(1, rows // (2 * hd)) if role == QKV else 0
    dw = rows + 2 * rows_kv if role == QKV else (2 * rows if role == SWIGLU else rows)
    ng = n // G
    rng = np.random.default_rng(n + 7 * rows + role)
    idx = np.arange(dw * n, dtype=np.int64).reshape(dw, n)
    wq = ((idx + idx // n * 5) % 16 - 8).astype(np.int8)                       # every nibble value, -8 included, in every column
    ws = (10.0 ** rng.uniform(-6, 3, (dw, ng))).astype(f32)
    wq[0, G:2 * G] = 0                                                         # an all-zero group, scale 1.0 as the exporter writes it
    ws[0, 1] = 1.0
    x = rng.standard_normal(n).astype(f32)
    kw = dict(rows_kv=rows_kv, head_dim=hd if role == QKV else 0, strict=strict)
    if role in (QKV, SWIGLU):
        kw.update(x=x, norm_w=(1 + 0.1 * rng.standard_normal(n)).astype(f32))
    elif role == QUANT:
        kw.update(x=x, out=rng.standard_normal(rows).astype(f32))
    else:
        pq, ps = oracle.quantize(x, G)
        kw.update(pre_q=pq, pre_s=ps, out=rng.standard_normal(rows).astype(f32))
    r4 = ops.gemv_role_w4(role, ck.pack_q4(wq), ws, n, rows, G, **kw)
    assert r4["info"][0] == (1 if G == 64 and n in LISTED[role] else 0), r4["info"]
    if strict:
        r8 = ops.gemv_role(role, wq, ws, n, rows, G, **kw)
        assert_biteq(r4["out"], r8["out"], "W4 launch against the int8 launch on the unpacked weights")
        if r4["tap"] is not None:
            assert_biteq(r4["tap"], r8["tap"], "normalised vector")
        return
    if role in (QKV, SWIGLU):
        y64 = ref64.rmsnorm64(x, kw["norm_w"])
        assert np.all(np.abs(r4["tap"] - y64) <= np.abs(y64) * ref64.rmsnorm_rel_budget(n) + ref64.TINY)
        xq, xs = oracle.quantize(r4["tap"], G)
    else:
        xq, xs = oracle.quantize(x, G)
    S, A = ref64.gemv_rows(xq, xs, wq, ws, n, dw, G)
    E = ref64.gemv_budget(n, G, A)
    if role in (QUANT, PREQR):
        want = np.asarray(kw["out"], np.float64) + S
        budget = E + ref64.U * (np.abs(want) + E)
    elif role == SWIGLU:
        want, budget = ref64.swiglu64(S[:rows], S[rows:]), ref64.swiglu_budget(S[:rows], S[rows:], E[:rows], E[rows:])
    else:
        want, budget = S, E
    err = np.abs(r4["out"].astype(np.float64) - want)
    assert np.all(err <= budget), (float(np.max(err / np.maximum(budget, 1e-300))))

@pytest.mark.parametrize("name", ["tiny", "tiny-untied", "tiny-g64", "small-hd128"])
def test_forward_q4_vs_oracle_on_the_expanded_file(q3, oracle, tmp_ckpt_dir, name):
    p4, p8 = q4_pair(q3.checkpoint, name, tmp_ckpt_dir)
    om = oracle.OracleModel(p8)
    with q3.TransformerBuilder(p4).build() as t:
        assert t.weight_bits == 4
        tok = 1
        for pos in [0, 1, 2, 3, 1, 7, 8]:
            a, b = np.array(t.forward(tok, pos), copy=True), om.forward(tok, pos)
            assert_biteq(a, b, f"{name} pos {pos}")
            assert t.forward_argmax(tok, pos) == oracle.sample_argmax(b)
            tok = oracle.sample_argmax(b)
        assert_biteq(t.read_state("x"), om.tap_x(), "x after final norm")

@pytest.mark.parametrize("name", ["qwen3-0.6b-dims-l2", "qwen3-4b-dims-l2", "qwen3-8b-dims-l2"])
def test_listed_layer_dims_q4_vs_q8_engine(q3, tmp_ckpt_dir, name):
    p4, p8 = q4_pair(q3.checkpoint, name, tmp_ckpt_dir)
    with q3.TransformerBuilder(p4).with_ctx_length(512).build() as t4, q3.TransformerBuilder(p8).with_ctx_length(512).build() as t8:
        assert (t4.weight_bits, t8.weight_bits) == (4, 8)
        tok = 3
        for pos in [0, 1, 2, 3, 300]:                                          # 300: the long-context plan (attention split at 256)
            a, b = np.array(t4.forward(tok, pos), copy=True), np.array(t8.forward(tok, pos), copy=True)
            assert_biteq(a, b, f"{name} pos {pos}")
            tok = int(np.argmax(b))
        t4.reset_kv(), t8.reset_kv()
        assert t4.generate_greedy(5, 0, 12) == t8.generate_greedy(5, 0, 12)

@pytest.mark.parametrize("name", ["small-hd128", "qwen3-0.6b-dims-l2"])
def test_batched_paths_q4_vs_q8_engine(q3, tmp_ckpt_dir, name):
    ck = q3.checkpoint
    p4, p8 = q4_pair(ck, name, tmp_ckpt_dir)
    prompt = ck.iter_prompt_tokens(ck.SHAPES[name], 5, 40)
    ragged = [prompt[:7], prompt[3:22], prompt[10:13]]
    got = []
    for path in (p4, p8):
        with q3.TransformerBuilder(path).with_ctx_length(128).build() as t:
            t.batch_init(4, 128)
            res = [t.generate_greedy_batch([1, 2, 3, 4], [0, 0, 0, 0], 8).tolist()]
            t.batch_reset_kv()
            res.append(t.generate_many_greedy(ragged, [6, 3, 5])[0])
            first = t.prefill(prompt, 0, batched=True)
            res.append([first] + t.generate_greedy(first, len(prompt), 4))
            got.append(res)
    assert got[0] == got[1]

def test_q4_layer_section_cut_short_is_refused(q3, tmp_ckpt_dir):
    ck = q3.checkpoint
    p4, _ = q4_pair(ck, "tiny", tmp_ckpt_dir)
    cut = os.path.join(tmp_ckpt_dir, "tiny.q4.cut.bin")
    with open(cut, "wb") as f:
        f.write(open(p4, "rb").read()[:ck.tensor_offsets(ck.read_header(p4))["gate_proj"][0] + 16])
    with pytest.raises(q3.Q3Error, match="Failed to read quantized tensor data: Insufficient data"):
        q3.TransformerBuilder(cut).build()
