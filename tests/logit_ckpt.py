"""Checkpoints whose logits are chosen: a valid checkpoint in which the logits depend only on the input token and are a designed
vector, so that the sampler sees distributions a Gaussian model never gives.  Helper module of tests/test_designed_logits.py (CPU)
and tests/test_sampler_designed.py (GPU); not a conftest.

Construction (layer dimensions of tiny-g64 with one layer and an untied classifier: dim 256, four groups of 64):
  * every o_proj and down_proj row is zero (zero int8 groups, scale 1.0): the residual stream stays the embedding row;
  * embedding row t holds int8 127 at element (t % 4) * 64, zeros elsewhere, all scales 1.0; every norm weight that matters is 1.0;
  * lm_head row v, group g holds int8 sign(design_g[v]) at the group's first element with scale |design_g[v]| (a zero design value
    is a zero group with scale 1.0), everything else zero.
Then logits(t) = design_{t % 4} x c at every position, c = 16 up to the RMSNorm epsilon and two roundings: token t selects design
t % 4 of the file.  A design is written as the logits wanted AFTER the division by its temperature T0; the file stores
value * T0 / 16.  Equal design values give bit-equal logits and the map is monotone, so ties and order are the table's.

Designs (V = vocabulary size; `settings` are the (temperature, top-p) pairs the tests draw with):
  peaked      token 5: 0, 77: -1, `third`: -2.5, V - 1: -3, the rest -30 - 0.005 (v % 997), all + PEAK; T0 0.7.  4 candidates,
              nucleus of 2
  uniform     all equal.  At V = 151,936 and top-p 0.9985 the histogram finds a threshold but the sequential f32 sum over ALL
              candidates stays below top-p: neither attempt crosses, last = n0 - 1
  second_try  0, except -4 where v % 37 == 7; top-p TOPP_SECOND_TRY.  The histogram's prefix (the upper tokens) sums sequentially to
              less than top-p, the sum over every candidate crosses: the token depends on the second attempt
              (on the pipelined path only: every wave of 64 indices holds both values, so both histogram kernels add value by
              value.  k_sample_norm_hist adds at most 768 values into a workgroup's own partial and then one partial per
              workgroup into the bin: an accurate mass, a threshold.  The single-workgroup kernel adds all 151,936 values into
              one LDS word, drifts like the sequential sum and finds no threshold: its first attempt already sorts everything)
  second_try_block  the same with the -4 tokens at the end of the vocabulary: every wave but one holds a single bin and adds its
              total once, so the single-workgroup kernel's histogram is accurate too and its second attempt decides the token
  head_flat   token 777: 11, the rest 0.  The flat mass lies at the foot of the 64-bin window: no threshold, every candidate sorted
  head_far    token 777: 13, the rest 0: the flat mass lies wholly below the window
  twins       tokens 9 and V - 9 equal, the rest 32 below: a nucleus of one (top-p 0.4) is the lower index
  levels      -0.75 (v % 5): five distinct probabilities, the nucleus ends inside a run of ties
  ramp        RAMP_TOP - step * v: probabilities run through the subnormals to exact zeros
  ramp_up     the ramp reversed: the maximum is the last index and the candidates fill the last two workgroup ranges of the
              chip-wide passes, the last a partial one
  count_K     1.5 on exactly K indices spread evenly, -40 elsewhere: exactly K candidates (K on either side of a kernel switch)

witness() restates, with sequential f32 sums (the histogram's bin masses apart, see there), what the sampler kernels decide on a
logit vector: cutoff and candidate count, the histogram rule (bins key >> 21, window of 64 bins below the maximum,
acc > topp * 1.001 + 1e-6, one bin of margin), whether the first attempt's candidates cross top-p, the nucleus size, the subnormal
and zero counts.  tests/test_designed_logits.py asserts the conditions on the C oracle's logits of the written files, not counts.
What witness() gave at V = 151,936 when the constants were chosen -- candidates / threshold found / n0 / sequential sum of the first
attempt's candidates / sequential sum of all candidates / nucleus:
  peaked (0.7, 0.9)             4 / yes / 2 / 0.91207 / 1.0 / 2
  uniform (1, 0.9985)           151,936 / yes / 151,936 / 0.99832 / 0.99832 / 151,936      neither attempt crosses
  second_try (1, 0.99802)       151,936 / yes / 147,829 / 0.99778 / 0.99827 / 149,883      only the second attempt crosses
  second_try_block (1, 0.99802) 151,936 / yes / 147,829 / 0.99785 / 0.99833 / 149,304
  head_flat (1, 0.9)            151,936 / no / 151,936 / 0.99962 / 0.99962 / 130,780       151,935 candidates in the window's last bin
  head_far (1, 0.9)             151,936 / no / 151,936 / 0.99755 / 0.99755 / 93,488
  levels (1, 0.9)               151,936 / yes / 91,162 / 0.91716 / 1.00044 / 86,866
  levels (0.3, 0.5)             30,388 / yes / 30,388 / 0.91834 / 0.91834 / 16,545
  ramp, ramp_up (1, 0.95)       1,032 / yes / 315 / 0.95715 / 0.99997 / 300                1,663 subnormals, 142,000 zeros
  ramp (0.5, 0.999)             746 / no / 746 / 1.0 / 1.0 / 346                           832 subnormals, 146,933 zeros
  count_2048, count_2049 (1, 0.9)  K / yes / K / 1.0 / 1.0 / 1,844 and 1,845
The scan's accumulator stays 5.0e-4 (uniform), 5.1e-4 (second_try) and 5.5e-4 (second_try_block) away from its limit;
HIST_ORDER_ERROR is 1.5e-4.
"""
from __future__ import annotations

import os

import numpy as np

from edge_ckpt import _f32, _zero_rows
from qwen3_rs_amd import checkpoint as ck

f32 = np.float32
SEED = 7
V_BIG, V_SMALL = 151936, 2000
C_NOMINAL = 16.0
TOPP_SECOND_TRY = float(f32(0.9980208873748779))
RADIX_MIN = 2048                       # kSampRadixMin of q3_sampler.h
TINY = f32(np.finfo(np.float32).tiny)


def shape_of(vocab: int) -> ck.ModelShape:
    return ck.ModelShape(256, 384, 1, 4, 2, vocab, 64, 64, False, 64)


# ---------------------------------------------------------------------------------------------------------------------
# designs: name -> (function V -> wanted logits / T0 as float64, T0, settings)
# ---------------------------------------------------------------------------------------------------------------------
PEAK = 100.0          # the peak is NOT at logit 0: an exp taken against another maximum than the row's overflows (peaked) or
RAMP_TOP = -100.0     # underflows (ramps), so k_sample_exp's maximum -- read from State::argmax, not recomputed -- has to be right


def _peaked(V):
    v = np.arange(V)
    d = -30.0 - 0.005 * (v % 997)
    d[5], d[77], d[4000 if V > 4000 else V // 2], d[V - 1] = 0.0, -1.0, -2.5, -3.0
    return d + PEAK


def _uniform(V):
    return np.full(V, 3.0)


N_LOW = 4107          # tokens of second_try at -4: those with v % 37 == 7 at V = 151,936


def _second_try(V):
    d = np.zeros(V)
    d[np.arange(V) % 37 == 7] = -4.0
    return d


def _second_try_block(V):
    d = np.zeros(V)
    d[V - N_LOW:] = -4.0
    return d


def _head_far(V):
    d = np.zeros(V)
    d[777] = 13.0
    return d


def _twins(V):
    d = np.full(V, -30.0)
    d[9] = d[V - 9] = 2.0
    return d


def _head_flat(V):
    d = np.zeros(V)
    d[777] = 11.0
    return d


def _levels(V):
    return -0.75 * (np.arange(V) % 5)


def _ramp(step):
    return lambda V: RAMP_TOP - step * np.arange(V)


def _ramp_up(V):
    return RAMP_TOP - 0.01 * np.arange(V)[::-1]


def count_indices(V, K):
    idx = np.linspace(0, V - 1, K).astype(np.int64)
    assert np.unique(idx).size == K
    return idx


def _count(K):
    def f(V):
        d = np.full(V, -40.0)
        d[count_indices(V, K)] = 1.5
        return d
    return f


DESIGNS = {
    "peaked": (_peaked, 0.7, [(0.7, 0.9), (0.7, 1.0)]),
    "uniform": (_uniform, 1.0, [(1.0, 0.9985)]),
    "second_try": (_second_try, 1.0, [(1.0, TOPP_SECOND_TRY)]),
    "head_flat": (_head_flat, 1.0, [(1.0, 0.9)]),
    "levels": (_levels, 1.0, [(1.0, 0.9), (0.3, 0.5)]),
    "ramp": (_ramp(0.01), 1.0, [(1.0, 0.95), (0.5, 0.999), (1.0, 1.0)]),
    "ramp_steep": (_ramp(0.5), 1.0, [(1.0, 0.95), (0.5, 0.999), (1.0, 1.0)]),
    "second_try_block": (_second_try_block, 1.0, [(1.0, TOPP_SECOND_TRY)]),
    "head_far": (_head_far, 1.0, [(1.0, 0.9)]),
    "twins": (_twins, 1.0, [(1.0, 0.4), (1.0, 0.9)]),
    "ramp_up": (_ramp_up, 1.0, [(1.0, 0.95), (1.0, 1.0)]),
    "count_2048": (_count(2048), 1.0, [(1.0, 0.9)]),
    "count_2049": (_count(2049), 1.0, [(1.0, 0.9)]),
    "count_64": (_count(64), 1.0, [(1.0, 0.9)]),
    "count_65": (_count(65), 1.0, [(1.0, 0.9)]),
}

# file -> (vocabulary, the four designs: token t draws from design t % 4)
FILES = {
    "big_a": (V_BIG, ["peaked", "uniform", "second_try", "head_flat"]),
    "big_b": (V_BIG, ["levels", "ramp", "count_2048", "count_2049"]),
    "big_c": (V_BIG, ["second_try_block", "head_far", "twins", "ramp_up"]),
    "small_a": (V_SMALL, ["peaked", "levels", "ramp_steep", "count_64"]),
    "small_b": (V_SMALL, ["count_65", "count_64", "levels", "peaked"]),
}
BIG_FILES, SMALL_FILES = ["big_a", "big_b", "big_c"], ["small_a", "small_b"]

SEEDS = [1, 42, 0xC0FFEE, 0x1234ABCD5678EF01, 777777, 2 ** 63 + 12345, 99, 31337]
# xorshift64* seeds whose FIRST coin is below 2^-20 / above 1 - 2^-20 (found by a vectorised search over seeds 1 .. 10^7;
# tests/test_designed_logits.py recomputes the coins): r = coin * cumulative at both ends of the cdf
COIN_LOW_SEEDS = [209226, 4458056]          # coins 8 / 2^24, 2 / 2^24
COIN_HIGH_SEEDS = [1574392, 2137202]        # coins 1 - 1 / 2^24, 1 - 3 / 2^24
COIN_EXTREME_DESIGNS = ("peaked", "levels", "ramp", "ramp_steep", "ramp_up", "twins")


def seeds_for(design, n=len(SEEDS)):
    """the seeds a per-design draw test uses: n ordinary ones, plus the coin extremes on the designs that take them"""
    return SEEDS[:n] + (COIN_LOW_SEEDS + COIN_HIGH_SEEDS if design in COIN_EXTREME_DESIGNS else [])


def cases(file):
    """every (design, group, temperature, top-p) of a file, each design once"""
    seen, out = set(), []
    for g, name in enumerate(FILES[file][1]):
        if name not in seen:
            seen.add(name)
            out += [(name, g, T, p) for T, p in DESIGNS[name][2]]
    return out


def token_of(file, design, k=0):
    """a token whose logits are `design`: the k-th of its residue class (any token t with t % 4 == group will do)"""
    return FILES[file][1].index(design) + 4 * k


def write(path: str, file: str) -> str:
    """the checkpoint FILES[file]; written once per path"""
    V, names = FILES[file]
    shape = shape_of(V)
    if os.path.exists(path) and os.path.getsize(path) == shape.file_size():
        return path
    G, d, ng = shape.group_size, shape.dim, shape.dim // shape.group_size
    assert len(names) == ng
    tmp = path + ".design"
    with open(tmp, "wb") as f:
        f.truncate(shape.file_size())
    mm = np.memmap(tmp, dtype=np.uint8, mode="r+")
    mm[:ck.HEADER_SIZE] = np.frombuffer(ck.header_bytes(shape), dtype=np.uint8)
    off = ck.tensor_offsets(shape)
    for name, count in shape.norm_tensors():
        _f32(mm, off[name][0], count)[:] = 1.0
    rng = np.random.Generator(np.random.PCG64([SEED, V]))
    for name, cnt, rows, cols in shape.quantized_tensors():
        q_off, s_off, stride = off[name]
        if name in ("embed_tokens", "lm_head"):
            continue
        for l in range(cnt):
            if name in ("o_proj", "down_proj"):
                _zero_rows(mm, shape, name, l, 0, rows)
                continue
            q, s, _ = ck.quantize_q80(rng.standard_normal(rows * cols, dtype=np.float32) * f32(cols ** -0.5), G)
            mm[q_off + l * stride: q_off + l * stride + rows * cols] = q.view(np.uint8)
            _f32(mm, s_off + l * stride, rows * cols // G)[:] = s
    # embedding: 127 at the first element of group t % ng
    q_off, s_off, _ = off["embed_tokens"]
    mm[q_off:q_off + V * d] = 0
    t = np.arange(V, dtype=np.int64)
    mm[q_off + t * d + (t % ng) * G] = 127
    _f32(mm, s_off, V * ng)[:] = 1.0
    # classifier: row v, group g = sign and magnitude of design g
    q_off, s_off, _ = off["lm_head"]
    mm[q_off:q_off + V * d] = 0
    sc = _f32(mm, s_off, V * ng).reshape(V, ng)
    for g, name in enumerate(names):
        fn, T0, _ = DESIGNS[name]
        val = (fn(V) * T0 / C_NOMINAL).astype(np.float32)
        mm[q_off + t * d + g * G] = np.sign(val).astype(np.int8).view(np.uint8)
        sc[:, g] = np.where(val != 0, np.abs(val), f32(1.0))
    mm.flush()
    del sc, mm
    os.replace(tmp, path)
    return path


# ---------------------------------------------------------------------------------------------------------------------
# the witness: what the sampler kernels decide on a logit vector (q3_sampler.h: k_sample, samp_threshold), sequential f32 sums
# ---------------------------------------------------------------------------------------------------------------------
def total_order_key(p):
    b = np.ascontiguousarray(p, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def witness(npo, logits, temperature, topp):
    """npo: oracle.np_oracle (its softmax is the reference's).  Returns a dict; the nucleus entries only for 0 < top-p < 1.
    Every running sum is sequential f32 except the histogram's bin masses: the kernels add those with atomics, in no fixed order,
    which is modelled by the correctly rounded sum (what the masses of k_sample_norm_hist, and of the single-workgroup kernel on
    waves of one bin, come close to: see HIST_ORDER_ERROR); `hist_margin` is the smallest distance of the scan's accumulator from
    its limit, to be held against that error."""
    p = npo.softmax((np.asarray(logits, dtype=np.float32) / f32(temperature)).astype(np.float32))
    n = p.size
    w = {"n": n, "subnormal": int(np.count_nonzero((p > 0) & (p < TINY))), "zeros": int(np.count_nonzero(p == 0)),
         "distinct": int(np.unique(p).size), "p": p}
    topp = f32(topp)
    if not (0.0 < topp < 1.0):
        return w
    cutoff = f32(f32(1.0) - topp) / f32(max(n - 1, 1))
    cand = np.nonzero(p >= cutoff)[0]
    key = total_order_key(p)
    # sorted candidates: probability descending, index ascending
    order = cand[np.lexsort((cand, -p[cand].astype(np.float64)))]
    cum = np.cumsum(p[order], dtype=np.float32)
    over = np.nonzero(cum > topp)[0]
    w.update(cutoff=float(cutoff), candidates=int(cand.size), crossed_all=bool(over.size), total_all=float(cum[-1]),
             nucleus=int(over[0]) + 1 if over.size else int(cand.size))
    w["nucleus_in_ties"] = bool(w["nucleus"] < cand.size and p[order[w["nucleus"] - 1]] == p[order[w["nucleus"]]])
    # histogram over the window of 64 bins below the largest probability
    bins = (key >> np.uint32(21)).astype(np.int64)
    bmax = int(bins.max())
    bfloor = max(bmax - 64, 0)
    inw = cand[bins[cand] >= bfloor]
    mass = np.zeros(2048, dtype=np.float32)
    for b in np.unique(bins[inw]):
        mass[b] = f32(np.sum(p[inw][bins[inw] == b], dtype=np.float64))
    limit = f32(f32(topp * f32(1.001)) + f32(1e-6))
    acc, found, b, margin = f32(0.0), False, 2047, np.inf
    while b > bfloor:
        acc = f32(acc + mass[b])
        margin = min(margin, abs(float(acc) - float(limit)))
        if acc > limit:
            found = True
            break
        b -= 1
    tbin = b - 1 if (found and b > 0) else 0
    pre = cand[key[cand] >= np.uint32(tbin << 21)]                       # the first attempt's candidates
    porder = pre[np.lexsort((pre, -p[pre].astype(np.float64)))]
    pcum = np.cumsum(p[porder], dtype=np.float32)
    w.update(threshold_found=found, window_mass=float(acc), hist_margin=margin, n0=int(pre.size), prefix_total=float(pcum[-1]),
             prefix_crossed=bool(np.any(pcum > topp)), below_window=int(np.count_nonzero(bins[cand] <= bfloor)),
             prefix_order=porder, prefix_cum=pcum)
    return w


# How far a kernel's bin mass can lie from the correctly rounded one, in the two cases the designs rely on.  The single-workgroup
# kernel on waves that hold one bin: a wave's total (a tree of 64) is added once, at most n / 64 adds into a mass <= 1, each off by at
# most half an ulp of 1: n / 64 * 2^-24.  k_sample_norm_hist, value by value: a workgroup adds at most 768 values into its own partial
# (<= 768 / n of the mass) and the 256 partials are added into the bin: 256 * 2^-24 + 768 * (768 / n) * 2^-24, less than the first.
# (The single-workgroup kernel on waves of mixed bins adds up to n values into one word: no such bound, and no design relies on one.)
HIST_ORDER_ERROR = (V_BIG / 64 + 64) * 2.0 ** -24


def draw_without_second_attempt(w, coin):
    """the token a sampler draws that stops at the first attempt's candidates although their sum does not cross top-p (what the
    second attempt exists to prevent): last = n0 - 1, cumulative = their total.  w: a witness() with prefix_crossed False"""
    assert not w["prefix_crossed"]
    cum, order = w["prefix_cum"], w["prefix_order"]
    r = f32(f32(coin) * cum[-1])
    hit = np.nonzero(r < cum)[0]
    return int(order[hit[0]]) if hit.size else int(order[-1])


def first_coin(seed):
    """the first uniform of a sampler seeded with `seed` (sampler.rs:44-54), and the state behind it"""
    M = (1 << 64) - 1
    s = int(seed) & M
    s ^= s >> 12
    s ^= (s << 25) & M
    s ^= s >> 27
    return f32(f32((((s * 0x2545F4914F6CDD1D) & M) >> 32) >> 8) / f32(16777216.0)), s
