"""The record of q3_score_many (include/qwen3_hip.h section 2l) restated in numpy from a logit vector, the log-probability formed
from it, and the call's schedule counted in Python.  Helper module of tests/test_score_host.py and tests/test_score.py (not a
conftest).  For the logits l[0 .. V) behind a position and the next token t:
    target = l[t]
    max    = fmaxf fold of l from -inf                                              (layers.rs:496)
    sum    = ((-0.0 + expf(l[0] - max)) + expf(l[1] - max)) + ...   in index order   (layers.rs:497-503), expf glibc's
    argmax = the last index of the maximum in total order                           (sampler.rs:57-59)"""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
DTYPE = np.dtype([("target", f32), ("max", f32), ("sum", f32), ("argmax", np.int32)])
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]


def expf(a):
    """glibc's expf of every element (numpy's own SIMD expf differs in the last bit)"""
    a = np.ascontiguousarray(a, dtype=f32)
    return np.fromiter((_libm.expf(float(v)) for v in a.ravel()), dtype=f32, count=a.size).reshape(a.shape)


def total_order_key(l):
    """u32 keys that order floats as f32::total_cmp does: -0.0 below +0.0"""
    b = np.ascontiguousarray(l, dtype=f32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def argmax_last(l) -> int:
    k = total_order_key(l)
    return int(k.size - 1 - np.argmax(k[::-1]))


def fold_max(l):
    return f32(np.fmax.reduce(np.asarray(l, dtype=f32), initial=f32(-np.inf)))


def exps(l):
    l = np.asarray(l, dtype=f32)
    return expf((l - fold_max(l)).astype(f32))


def seq_sum(e):
    """Iterator::sum::<f32>(): a strict left fold from -0.0"""
    return np.add.accumulate(np.concatenate([np.array([-0.0], dtype=f32), np.asarray(e, dtype=f32)]), dtype=f32)[-1]


def record(l, target: int):
    l = np.asarray(l, dtype=f32)
    out = np.zeros((), dtype=DTYPE)
    out["target"], out["max"], out["sum"], out["argmax"] = l[target], fold_max(l), seq_sum(exps(l)), argmax_last(l)
    return out


def records(logit_rows, targets):
    """one record per row of logits"""
    return np.array([record(l, t) for l, t in zip(logit_rows, targets)], dtype=DTYPE).reshape(len(targets))


def prob(l, target: int):
    """softmax(l)[target] as layers.rs:503-505 forms it from the record's numbers: e * (1 / sum)"""
    l = np.asarray(l, dtype=f32)
    r = record(l, target)
    e = expf(np.array([f32(r["target"] - r["max"])], dtype=f32))[0]
    return f32(e * f32(f32(1.0) / r["sum"]))


def logprobs_of(recs):
    """generation.logprobs_of: (target - max) - log(sum) in float64"""
    t, m, s = (np.asarray(recs[k], dtype=f32).astype(np.float64) for k in ("target", "max", "sum"))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (t - m) - np.log(s)


def log_softmax64(l, target: int) -> float:
    z = np.asarray(l, dtype=f32).astype(np.float64)
    z = z - z.max()
    return float(z[target] - np.log(np.exp(z).sum()))


def assert_records(got, want, what):
    """the standard of the header: target and sum by bits, argmax equal, max by value"""
    assert got.dtype == DTYPE and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    for k in ("target", "sum"):
        a, b = np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{what}: {k} differs at records {bad[:8].tolist()} of {a.size}: {got[k][bad[:4]]} vs {want[k][bad[:4]]}"
    bad = np.flatnonzero(got["argmax"] != want["argmax"])
    assert bad.size == 0, f"{what}: argmax differs at records {bad[:8].tolist()}: {got['argmax'][bad[:4]]} vs {want['argmax'][bad[:4]]}"
    bad = np.flatnonzero(~(got["max"] == want["max"]))
    assert bad.size == 0, f"{what}: max differs at records {bad[:8].tolist()}: {got['max'][bad[:4]]} vs {want['max'][bad[:4]]}"


def pack_blocks(lens, cap):
    """q3_dense_pack's rule: the blocks of one wave, each a list of pieces (run, offset in the run, columns, first column)"""
    blocks, cur, end = [], [], 0
    for r, n in enumerate(lens):
        off = 0
        while off < n:
            start = (end + 7) & ~7
            if start >= cap:
                blocks.append(cur)
                cur, start = [], 0
            take = min(n - off, cap - start)
            cur.append((r, off, take, start))
            off += take
            end = start + take
            if off < n:
                blocks.append(cur)
                cur, end = [], 0
    if cur:
        blocks.append(cur)
    return blocks


def schedule(lens, score_from, streams, cap):
    """(waves, blocks, live_columns, pad_columns, chunks, scored) of q3_score_many: a column is scored when its token has a
    successor in its request at or behind score_from; a block's scored columns go 32 at a time"""
    sf = [1] * len(lens) if score_from is None else list(score_from)
    waves = blocks = live = pad = chunks = 0
    for w0 in range(0, len(lens), streams):
        waves += 1
        for blk in pack_blocks(lens[w0:w0 + streams], cap):
            blocks += 1
            cols = sum(p[2] for p in blk)
            live += cols
            pad += ((blk[-1][3] + blk[-1][2] + 7) & ~7) - cols
            scored = sum(1 for r, off, take, _ in blk for i in range(off, off + take)
                         if i + 1 < lens[w0 + r] and i + 1 >= sf[w0 + r])
            chunks += (scored + 31) // 32
    return waves, blocks, live, pad, chunks, sum(n - f for n, f in zip(lens, sf))
