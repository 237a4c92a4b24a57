"""The classifier arithmetic of q3_choice_many (include/qwen3_hip.h section 2k) restated in numpy.  Helper module of
tests/test_choice_host.py (not a conftest).  For the normalised vector y (the final RMSNorm's output), a classifier row c and the
group size G:

    xs_g = max|y_i| / 127 over the group;  xq_i = round-half-away(y_i / xs_g) as i8 (saturating, NaN -> 0);  xs_g == 0: xq_i = 0
    d_g  = sum over the group of wq[c][i] * xq_i      int32, exact
    t_g  = ((float)d_g * ws[c][g]) * xs_g             two float32 roundings
    logit = (((t_0 + t_1) + t_2) + ...)               a strict left fold, groups ascending

Every float32 operation is a single numpy float32 operation (IEEE, no contraction); np.add.accumulate folds strictly from the left."""
import numpy as np

from qwen3_rs_amd import checkpoint as ck


def quantize(y, G):
    """(int8 codes [n], float32 scales [n / G]) of a float32 vector"""
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, G)
    with np.errstate(all="ignore"):
        xs = (np.max(np.abs(y), axis=1) / np.float32(127.0)).astype(np.float32)
        v = (y / xs[:, None]).astype(np.float32).astype(np.float64)       # the IEEE float32 quotient, held exactly
        r = np.trunc(v + np.copysign(0.5, v))                             # half away from zero, exact in float64
        r = np.where(np.isnan(r), 0.0, np.clip(r, -128.0, 127.0))
        q = np.where(xs[:, None] != 0.0, r, 0.0).astype(np.int8)
    return q.reshape(-1), xs


def logits(y, wq, ws, ids, G):
    """wq int8 [V, n], ws float32 [V, n / G]: the logits of the rows `ids`, float32 [len(ids)]"""
    xq, xs = quantize(y, G)
    ng = xs.size
    out = np.zeros(len(ids), dtype=np.float32)
    for j, c in enumerate(ids):
        d = np.sum(wq[c].astype(np.int32).reshape(ng, G) * xq.astype(np.int32).reshape(ng, G), axis=1, dtype=np.int32)
        t = (d.astype(np.float32) * ws[c].astype(np.float32)).astype(np.float32)
        t = (t * xs).astype(np.float32)
        out[j] = np.add.accumulate(t, dtype=np.float32)[-1]
    return out


def classifier(path):
    """(wq int8 [V, dim], ws float32 [V, dim / G], G) of a checkpoint file: lm_head, or the token embedding table when it is shared"""
    shape = ck.read_header(path)
    raw = np.fromfile(path, dtype=np.uint8)
    V, d, G = shape.vocab_size, shape.dim, shape.group_size
    q_off, s_off, _ = ck.tensor_offsets(shape)["embed_tokens" if shape.shared_classifier else "lm_head"]
    wq = raw[q_off:q_off + V * d].view(np.int8).reshape(V, d)
    ws = raw[s_off:s_off + 4 * (V * d // G)].view("<f4").reshape(V, d // G)
    return wq, ws, G
