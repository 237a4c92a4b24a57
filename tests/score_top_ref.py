"""The k best tokens and the target's rank of q3_score_top_many (include/qwen3_hip.h section 2m) restated in numpy from a logit
vector.  Helper module of tests/test_score_top_host.py and tests/test_score_top.py (not a conftest).  The key of entry i of a row
l[0 .. V) is (total_order_key(l[i]) << 32) | i; the top k are the k largest keys, largest first; the rank of target t is the number
of keys above key[t].  Keys are distinct integers: there is no tolerance."""
import numpy as np

from score_ref import total_order_key

f32 = np.float32
DTYPE = np.dtype([("logit", f32), ("index", np.int32)])
TOP_MAX = 64


def keys(l):
    l = np.ascontiguousarray(l, dtype=f32)
    return (total_order_key(l).astype(np.uint64) << np.uint64(32)) | np.arange(l.size, dtype=np.uint64)


def top_keys(l, k: int):
    """the k largest keys, descending"""
    return np.sort(keys(l))[::-1][:k].copy()


def pairs(l, sorted_keys):
    """{logit, index} of keys of row l"""
    out = np.zeros(len(sorted_keys), dtype=DTYPE)
    out["index"] = (np.asarray(sorted_keys, dtype=np.uint64) & np.uint64(0xffffffff)).astype(np.int32)
    out["logit"] = np.ascontiguousarray(l, dtype=f32)[out["index"]]
    return out


def top(l, k: int):
    return pairs(l, top_keys(l, k))


def rank(l, t: int) -> int:
    ks = keys(l)
    return int(np.count_nonzero(ks > ks[t]))


def keys_of(tops):
    """the keys of an array of DTYPE, same shape"""
    return (total_order_key(tops["logit"]).astype(np.uint64) << np.uint64(32)) | tops["index"].astype(np.uint32).astype(np.uint64)


def assert_tops(got, want, what):
    """logits by bits, indices equal"""
    assert got.dtype == DTYPE and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    a, b = np.ascontiguousarray(got["logit"]).view(np.uint32), np.ascontiguousarray(want["logit"]).view(np.uint32)
    bad = np.argwhere((a != b) | (got["index"] != want["index"]))
    assert bad.size == 0, f"{what}: differs at {bad[:6].tolist()} of {got.shape}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
