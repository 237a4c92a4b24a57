"""The shapes of the group-size tests (tests/test_group_sizes.py, and the group-size rows of tests/test_gpu_parity.py) and the CPU-side
models they share.  Every listed model and almost every other test uses quantization group 64; the engine accepts any power of two
in [16, 1024] single-stream (check_supported) and 64 / 128 / 256 batched (q3_batch_init), and the exporter writes whatever
--group-size it is given (model_exporter.rs:39-58).

What each shape reaches (from the planners: plan_role / build_plan in q3_engine.hip, batch_plan in q3_batch_host.inc):

  g128-hd128   NJ = 2 chained MFMAs per group in k_bgemm; head_dim 128 with 2 query heads per kv head: k_attn_gqa2; hd % G == 0, so the
               attention kernel quantizes xb itself (gqa_store), one group per head
  g128-hd64    hd % G != 0: no fused xb quantizer, Wo runs its own PRO_QUANT launch; head_dim 64: k_attn_gqa
  g256-hd128   NJ = 4; hd % G != 0: unfused; its own lm_head (untied classifier)
  g256-hd256   gqa_store with upg = 4: one group is the four 64-lane quarters of a 256-wide head
  dims06-g128  the 0.6B layer dims (1024 / 3072, 16 heads, 8 kv heads): k_bquant_split in its run-time-division form with 4 parts,
  dims06-g256  row-tile pairs, and NT = 2 stream tiles at more than 16 streams; at 256 a part is exactly one group
  g512         single stream only (q3_batch_init refuses): a group is 128 threads = 2 waves of the 256-thread quantizer workgroup
  g1024        single stream only: a group is the whole workgroup (4 waves); lpg = 64 lanes per group in k_gemv; untied classifier

Single stream, G != 64 always takes the generic k_gemv<PRO, EPI, 0, ...> instantiations (find_cfg returns nullptr), whose
prologues quantize through the run-time-lanes path of quantize4_to_lds.
"""
import numpy as np

from oracle import np_oracle
from qwen3_rs_amd import checkpoint as ck

CKPT_SEED = 8642
SHAPES = {
    "g128-hd128": ck.ModelShape(512, 1024, 2, 8, 4, 2048, 96, 128, True, 128),
    "g128-hd64": ck.ModelShape(256, 384, 2, 4, 2, 512, 96, 64, True, 128),
    "g256-hd128": ck.ModelShape(512, 768, 2, 4, 2, 512, 96, 128, False, 256),
    "g256-hd256": ck.ModelShape(512, 1024, 2, 4, 2, 512, 96, 256, True, 256),
    "dims06-g128": ck.ModelShape(1024, 3072, 2, 16, 8, 4096, 96, 128, True, 128),
    "dims06-g256": ck.ModelShape(1024, 3072, 2, 16, 8, 4096, 96, 128, True, 256),
    "g512": ck.ModelShape(512, 1024, 2, 4, 2, 512, 96, 128, True, 512),
    "g1024": ck.ModelShape(1024, 2048, 2, 8, 4, 512, 96, 128, False, 1024),
}
BATCHED = [n for n, s in SHAPES.items() if s.group_size <= 256]
SINGLE_ONLY = [n for n, s in SHAPES.items() if s.group_size > 256]

# ---- the single-stream schedules
N_FORWARD = 10                 # forwards on seeded random tokens at positions 0 .. 9
PROMPT_LEN, N_GREEDY = 9, 8    # prefill of 9 tokens from position 0, then 8 greedy tokens
SAMPLER = (0.8, 0.9, 0x9E3779B97F4A7C15)
N_DRAWS = 8


def forward_tokens(shape):
    return [int(t) for t in np.random.default_rng(3100).integers(0, shape.vocab_size, N_FORWARD)]


def prompt(shape, n=PROMPT_LEN, seed=3200):
    return [int(t) for t in np.random.default_rng(seed).integers(0, shape.vocab_size, n)]


# ---- the batched schedules
STREAM_COUNTS = (3, 17, 32)
BATCH_STEPS = 4
PREFILL_LEN, PREFILL_POS = 70, 3


def streams(shape, n):
    """(first tokens, ragged first positions) of the first n of 32 fixed streams"""
    rng = np.random.default_rng(3300)
    toks = [int(t) for t in rng.integers(0, shape.vocab_size, 32)]
    pos = [int(p) for p in rng.integers(0, 6, 32)]
    return toks[:n], pos[:n]


def checked_streams(n):
    """the streams compared with single-stream runs: the first three, both sides of the 16-stream tile boundary, the last"""
    return sorted({i for i in (0, 1, 2, 15, 16, n - 1) if i < n})


# ---- the column-pass loops: the reduced tables of cols_draw_cases / cols_stop_cases / prefix_cases
COLS_PROMPT_LEN = (1, 2, 5, 33, 40)
COLS_SLOTS, COLS_NEW = 3, 6
COLS_TEMPERATURE = (0.0, 0.8, 1.0, 0.0, 0.6)
COLS_TOPP = 0.9
COLS_SEEDS = tuple(0x9E3779B97F4A7C15 + 1000003 * r for r in range(len(COLS_PROMPT_LEN)))
PREFIX_LEN = 7


def cols_prompts(shape):
    return [[int(t) for t in np.random.default_rng(4100 + r).integers(0, shape.vocab_size, n)] for r, n in enumerate(COLS_PROMPT_LEN)]


def cols_prefix(shape):
    return [int(t) for t in np.random.default_rng(5200).integers(0, shape.vocab_size, PREFIX_LEN)]


# ---- operator vectors
def random_vector(G, n=3072):
    """the vector of test_gpu_parity.test_quantize_bitexact: N(0, 3) with a zero group and a group whose maximum is 1e-30"""
    x = (np.random.default_rng(G).standard_normal(n) * 3).astype(np.float32)
    x[:G] = 0.0
    x[G] = 1e-30
    return x


def max_sweep_vector(G):
    """G/4 groups (repeated until the vector is longer than 1,024 elements, so that the quantizer's threads take several float4
    slots): group i holds its maximum, 3.0 with alternating sign, in float4 slot i, at element i % 4 of the slot, and values below
    2.9 in magnitude everywhere else.  Every thread of a group carries the group's maximum once, so a reduction that leaves out
    any lane -- or any wave -- of the group is seen."""
    ng = G // 4
    reps = max(1, -(-1025 // (ng * G)))
    rng = np.random.default_rng(600 + G)
    x = np.clip(rng.standard_normal((reps * ng, G)), -2.9, 2.9).astype(np.float32)
    for g in range(reps * ng):
        i = g % ng
        x[g, 4 * i + (i % 4)] = 3.0 if g % 2 == 0 else -3.0
    return x.reshape(-1)


# ---- the CPU model of a quantizer that takes its maximum per wave
def quantize_per_wave(x, G, wave_elems=256):
    """tensor.rs:91-119 with the group maximum taken per slice of 256 elements (one 64-lane wave of float4 slots) instead of per
    group: every slice is quantized with its own maximum and the stored scale is the first slice's.  For G <= 256 this IS the
    reference rule.  (What a reduction confined to one wave computes at G = 512 / 1024.)"""
    w = min(G, wave_elems)
    q, s = np_oracle.quantize(np.ascontiguousarray(x, dtype=np.float32), w)
    return q, s.reshape(-1, G // w)[:, 0].copy()


def groups_that_differ(x, G, oracle_quantize):
    """number of groups in which quantize_per_wave and the oracle disagree (int8 values or scale), and the number of groups"""
    qa, sa = quantize_per_wave(x, G)
    qb, sb = oracle_quantize(x, G)
    bad = np.any(qa.reshape(-1, G) != np.asarray(qb).reshape(-1, G), axis=1) | (sa.view(np.int32) != np.asarray(sb, dtype=np.float32).view(np.int32))
    return int(np.count_nonzero(bad)), bad.size


def layer0_inputs(path, shape, rmsnorm, dequantize):
    """the layer-0 quantizer input of every token of the vocabulary: rmsnorm(embedding row, input_layernorm[0]) (qwen3.rs:62-79, 131-135)"""
    raw = np.fromfile(path, dtype=np.uint8)
    off = ck.tensor_offsets(shape)
    V, d, G = shape.vocab_size, shape.dim, shape.group_size
    w = raw[off["input_layernorm"][0]:off["input_layernorm"][0] + 4 * d].view("<f4")
    q_off, s_off, _ = off["embed_tokens"]
    q = raw[q_off:q_off + V * d].view(np.int8)
    s = raw[s_off:s_off + 4 * (V * d // G)].view("<f4")
    x = np.asarray(dequantize(q, s, G), dtype=np.float32).reshape(V, d)
    return np.stack([rmsnorm(x[t], w) for t in range(V)])
