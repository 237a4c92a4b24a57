"""Edge-valued synthetic checkpoints: a synthetic checkpoint (checkpoint.write_synthetic_checkpoint) with named, composable edits
applied in place, chosen so that the REFERENCE ITSELF walks into the special cases a Gaussian model never reaches.  Helper module of
tests/test_edge_checkpoints.py (not a conftest); every edit leaves the file a valid exporter output (a zeroed int8 group carries
scale 1.0, model_exporter.rs:122).

Edits (EDITS maps a name to the list applied):
  hot_scores       q_norm and k_norm of every layer x HOT_SCORES: attention scores differ by more than 88 inside a row, so the exp
                   leaves its main range, underflows to +0 and through the subnormals, and the exact row sums see zeros
  far_scores       the same x FAR_SCORES: differences past -750, where the double inside glibc's expf itself underflows -- the
                   first point at which the exp's main path ALONE returns other bits than the full routine (between -88 and about -708
                   the two agree bit for bit), so that a kernel which wrongly stays on the main path is caught, not merely entered
  hot_gate         post_attention_layernorm x HOT_GATE: W1's outputs pass -88.7 (exp overflows to inf, the SwiGLU product is
                   -0.0) and +88
  zero_groups      a zero group at each activation quantizer: the first group of every input_layernorm (QKV input), gate_proj rows
                   [G, 2G) (silu(0) * u = +-0.0: a group of mixed signed zeros into W2's quantizer), the v_proj rows of kv head 0
                   (zero attention outputs into Wo's quantizer).  Rule: scale 0, NaN quotient, `as i8` gives 0
  zero_keys        the k_proj rows of the last kv head: key rows 0 after the norm, all scores 0, a uniform softmax
  tied_classifier  classifier row 2i+1 := row 2i (int8 and scales; the embedding when the classifier is shared): every logit pair is
                   bit-equal and every greedy step is a tie that the reference resolves to the odd index (last maximum)
  flat_logits      final norm weights 0: every logit +0.0, the greedy token is vocab_size - 1, the sampler's distribution is uniform
  all              hot_scores + hot_gate + zero_groups + tied_classifier

Constants.  HOT_SCORES = 6 on every shape (the factor of test_attention_scores_outside_the_exp_main_range); FAR_SCORES = 16 (scores
grow with the square of the factor: under hot_scores the most negative softmax input of the reference is -190 / -249 on tiny-g64 /
small-hd128, under far_scores -1,463 / -1,828 / -2,091 on tiny-g64 / small-hd128 / small-longctx, with 260 / 20,716 / 99,097 inputs at
or beyond -750 over the single-stream schedule, and logits stay within +-6); HOT_GATE = 64 on every shape: the FFN input is normalised, so W1's outputs are about N(0, 1) x HOT_GATE whatever the row length.  Checkpoint seed 5.

Witness counts of the numpy reference (oracle/np_oracle.py) over each shape's schedules (test_edge_checkpoints.SHAPES /
streams(): greedy decode from token 3 at position 0, and the ragged batched-decode streams), as measured when the constants were
chosen.  Columns: softmax inputs at or beyond -88 below their row maximum / nonzero subnormal probabilities (edit hot_scores); gate
values < -88.8 / > 88 / -0.0 SwiGLU outputs (edit hot_gate); the same five under `all`:

  shape                schedule          hot_scores       hot_gate                 all
  tiny-g64             24 positions      508 / 216        1449 / 1696 / 726        452 / 220 / 1267 / 1373 / 2194
  tiny-g64             17 streams x 4    84 / 52          4288 / 4418 / 2128       106 / 66 / 3731 / 3783 / 6147
  small-hd128          81 positions      34373 / 11907    20849 / 21287 / 10628    34190 / 11966 / 19523 / 19943 / 17698
  small-hd128          17 streams x 4    357 / 229        17378 / 17599 / 8599     337 / 196 / 16454 / 16348 / 14896
  small-longctx        257 positions     143458 / 44198   21042 / 22392 / 10596    139481 / 43697 / 19329 / 19943 / 26052
  small-longctx        3 streams x 6     43 / 25          1564 / 1635 / 788        51 / 41 / 1410 / 1375 / 1858
  qwen3-0.6b-dims-l2   12 positions      401 / 190        5996 / 6078 / 3025       409 / 194 / 6163 / 6178 / 3812
  qwen3-0.6b-dims-l2   17 streams x 4    523 / 330        34995 / 35536 / 17471    539 / 333 / 34223 / 34866 / 21516
  qwen3-4b-dims-l2     17 streams x 2    170 / 119        55405 / 56442 / 27667    198 / 134 / 54884 / 56359 / 29801

tests/test_edge_checkpoints.py asserts the conditions (not the counts) for every (shape, edit, schedule) its GPU part uses.
"""
from __future__ import annotations

import os

import numpy as np

from qwen3_rs_amd import checkpoint as ck

SEED = 5
HOT_SCORES = 6.0
FAR_SCORES = 16.0
HOT_GATE = 64.0
# the shapes of the package plus tiny-g64 with its own lm_head (every listed group-64 test shape shares its classifier)
SHAPES = dict(ck.SHAPES, **{"tiny-g64-untied": ck.ModelShape(256, 384, 2, 4, 2, 512, 96, 64, False, 64)})


def _f32(mm, off, n):
    return mm[off:off + 4 * n].view("<f4")


def _zero_rows(mm, shape, name, layer, r0, r1):
    """rows [r0, r1) of item `layer` of a quantized tensor := 0 with scale 1.0, as quantize_q80 writes an all-zero group"""
    cols = {n: c for n, _, _, c in shape.quantized_tensors()}[name]
    assert cols % shape.group_size == 0
    q_off, s_off, stride = ck.tensor_offsets(shape)[name]
    gpr = cols // shape.group_size
    mm[q_off + layer * stride + r0 * cols: q_off + layer * stride + r1 * cols] = 0
    _f32(mm, s_off + layer * stride + 4 * r0 * gpr, (r1 - r0) * gpr)[:] = 1.0


def _scale_norm(mm, shape, name, k):
    count = dict(shape.norm_tensors())[name]
    _f32(mm, ck.tensor_offsets(shape)[name][0], count)[:] *= np.float32(k)


def hot_scores(mm, shape, k=HOT_SCORES):
    _scale_norm(mm, shape, "q_norm", k)
    _scale_norm(mm, shape, "k_norm", k)


def far_scores(mm, shape):
    hot_scores(mm, shape, FAR_SCORES)


def hot_gate(mm, shape, k=HOT_GATE):
    _scale_norm(mm, shape, "post_attention_layernorm", k)


def zero_groups(mm, shape):
    G = shape.group_size
    w = _f32(mm, ck.tensor_offsets(shape)["input_layernorm"][0], shape.n_layers * shape.dim).reshape(shape.n_layers, shape.dim)
    w[:, :G] = 0.0
    for l in range(shape.n_layers):
        _zero_rows(mm, shape, "gate_proj", l, G, 2 * G)
        _zero_rows(mm, shape, "v_proj", l, 0, shape.head_dim)


def zero_keys(mm, shape):
    for l in range(shape.n_layers):
        _zero_rows(mm, shape, "k_proj", l, shape.kv_dim - shape.head_dim, shape.kv_dim)


def tied_classifier(mm, shape):
    t = "embed_tokens" if shape.shared_classifier else "lm_head"
    q_off, s_off, _ = ck.tensor_offsets(shape)[t]
    V, d = shape.vocab_size, shape.dim
    assert V % 2 == 0
    q = mm[q_off:q_off + V * d].reshape(V // 2, 2, d)
    q[:, 1] = q[:, 0]
    s = _f32(mm, s_off, V * d // shape.group_size).reshape(V // 2, 2, d // shape.group_size)
    s[:, 1] = s[:, 0]


def flat_logits(mm, shape):
    _f32(mm, ck.tensor_offsets(shape)["norm"][0], shape.dim)[:] = 0.0


EDITS = {
    "hot_scores": [hot_scores],
    "far_scores": [far_scores],
    "hot_gate": [hot_gate],
    "zero_groups": [zero_groups],
    "zero_keys": [zero_keys],
    "tied_classifier": [tied_classifier],
    "flat_logits": [flat_logits],
    "all": [hot_scores, hot_gate, zero_groups, tied_classifier],
}


def write(path: str, name: str, edit: str, seed: int = SEED) -> str:
    """checkpoint of SHAPES[name] with EDITS[edit] applied; written once per path"""
    shape = SHAPES[name]
    if os.path.exists(path) and os.path.getsize(path) == shape.file_size():
        return path
    tmp = path + ".edit"
    ck.write_synthetic_checkpoint(tmp, shape, seed=seed)
    mm = np.memmap(tmp, dtype=np.uint8, mode="r+")
    for fn in EDITS[edit]:
        fn(mm, shape)
    mm.flush()
    del mm
    os.replace(tmp, path)
    return path


# ---------------------------------------------------------------------------------------------------------------------
# the witness: what the numpy reference meets on such a checkpoint
# ---------------------------------------------------------------------------------------------------------------------
TINY = np.float32(np.finfo(np.float32).tiny)


class Recorder:
    """Wraps oracle.np_oracle's module-level softmax / swiglu / quantize (install them with pytest's monkeypatch.setattr) and counts,
    per forward() and per layer, the edge values that pass through them.  The call order inside NpQwen3.forward gives the layer:
    n_heads softmax calls and one swiglu per layer; quantize at QKV input, Wo input, FFN input, W2 input per layer, then the
    classifier input."""

    def __init__(self, npo, shape):
        self.npo, self.shape = npo, shape
        self.orig = (npo.softmax, npo.swiglu, npo.quantize)
        self.steps = []

    def install(self, setattr_):
        setattr_(self.npo, "softmax", self.softmax)
        setattr_(self.npo, "swiglu", self.swiglu)
        setattr_(self.npo, "quantize", self.quantize)

    def begin(self):
        L = self.shape.n_layers
        self.cur = {"cold": [0] * L, "cold_rows": [0] * L, "far": [0] * L, "subnormal": 0, "uniform_rows": [0] * L, "gate_lo": 0, "gate_hi": 0,
                    "swiglu_negzero": 0, "zero_groups": [[0] * L for _ in range(4)], "hidden_negzero": [0] * L}
        self.n_sm = self.n_q = 0
        self.steps.append(self.cur)

    def softmax(self, a):
        out = self.orig[0](a)
        layer = self.n_sm // self.shape.n_heads
        self.n_sm += 1
        if layer < self.shape.n_layers:                       # later calls are the sampler's
            a = np.asarray(a, dtype=np.float32)
            cold = int(np.count_nonzero((a - a.max()).astype(np.float32) <= np.float32(-88.0)))
            self.cur["cold"][layer] += cold
            self.cur["cold_rows"][layer] += cold > 0
            self.cur["far"][layer] += int(np.count_nonzero((a - a.max()).astype(np.float32) <= np.float32(-750.0)))
            self.cur["subnormal"] += int(np.count_nonzero((out > 0) & (out < TINY)))
            self.cur["uniform_rows"][layer] += bool(a.size > 1 and np.all(out == out[0]))
        return out

    def swiglu(self, g, u):
        out = self.orig[1](g, u)
        self.cur["gate_lo"] += int(np.count_nonzero(g < np.float32(-88.8)))
        self.cur["gate_hi"] += int(np.count_nonzero(g > np.float32(88.0)))
        self.cur["swiglu_negzero"] += int(np.count_nonzero((out == 0) & np.signbit(out)))
        return out

    def quantize(self, x, group_size):
        layer, site = divmod(self.n_q, 4)
        self.n_q += 1
        if layer < self.shape.n_layers:
            g = np.asarray(x, dtype=np.float32).reshape(-1, group_size)
            zero = np.max(np.abs(g), axis=1) == 0
            self.cur["zero_groups"][site][layer] += int(np.count_nonzero(zero))
            if site == 3:
                self.cur["hidden_negzero"][layer] += int(np.count_nonzero(zero & np.any(np.signbit(g), axis=1)))
        return self.orig[2](x, group_size)

    def forward(self, model, token, pos):
        self.begin()
        lg = model.forward(token, pos)
        self.cur["logits"] = lg
        return lg
