"""The L2 part of q3_embed_many (include/qwen3_hip.h section 2j) restated in numpy float32.  Helper module of tests/test_embed.py and
tests/test_embed_host.py (not a conftest).

    s2  = (((-0.0 + y0*y0) + y1*y1) + ... )   over the first out_dim components, a strict left fold
    nrm = sqrt(s2);  d = nrm > 1e-12 ? nrm : 1e-12   (torch F.normalize's eps; a NaN nrm takes the eps)
    out = y / d

np.add.accumulate folds strictly from the left (no pairwise blocks), np.sqrt and the divide of float32 operands are IEEE."""
import numpy as np

EPS = np.float32(1e-12)


def seq_sum(terms) -> np.float32:
    """the left fold of float32 terms, started from -0.0"""
    t = np.concatenate((np.array([-0.0], dtype=np.float32), np.ascontiguousarray(terms, dtype=np.float32)))
    return np.add.accumulate(t, dtype=np.float32)[-1]


def l2_row(y, out_dim=None) -> np.ndarray:
    y = np.ascontiguousarray(y, dtype=np.float32)
    v = y if out_dim is None else y[:out_dim]
    with np.errstate(all="ignore"):
        nrm = np.sqrt(seq_sum(v * v), dtype=np.float32)
        d = np.where(nrm > EPS, nrm, EPS).astype(np.float32)
        return (v / d).astype(np.float32)


def l2(rows, out_dim=None) -> np.ndarray:
    """rows [n, dim] -> [n, out_dim]: every row cut to its first out_dim components (None: all) and L2-normalised"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    return np.stack([l2_row(r, out_dim) for r in rows])
