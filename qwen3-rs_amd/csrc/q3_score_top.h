// q3_score_top.h -- the k best tokens of every scored column and the rank of its target (include/qwen3_hip.h section 2m).
//
// The rows, the arguments and the row sources are those of q3_score.h: l[0 .. V) of the classifier's output, RecordArgs, and a
// source that names every row's record, target, k and destinations.  The key of entry i is
//     ((uint64)total_order_key(l[i]) << 32) | i,
// the key the classifier leaves per workgroup in the argmax slots and spec_col_best folds.  Keys are distinct integers, so the k
// largest of a row and the number of keys above the target's are the same however the row is cut:
//   k_score_top_part   grid (parts, rows): the k largest keys of one slice of a row, sorted, and the slice's count of keys above the target's;
//   k_score_top_merge  grid rows: one wave takes the k largest of the parts' sorted lists, as {logit, index}, and sums the counts.
// Only a thread's own loop index, its own counters and what the source hands out (host-checked table entries; the pass's out[j] and
// its committed token clamped to [0, V)) become addresses: no logit and no key read back from memory does, so a row that holds a NaN
// is wrong but harmless.
#pragma once

namespace q3 {

constexpr int kScoreTopMax = 64;        // Q3_SCORE_TOP_MAX: the largest k, and the lanes of the merge's wave
constexpr int kScoreTopParts = 64;      // the most slices per row: one list per lane of the merge
constexpr int kScoreTopE = 10;          // keys a thread of the part kernel holds: a tile is 256 * 10 entries, V = 151,936 / 64 parts is 2,374

// q3_score_top of the header
struct ScoreTop {
    float logit;
    int index;
};

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    v = max(v, (unsigned)dpp_i<0xB1>((int)v));
    v = max(v, (unsigned)dpp_i<0x4E>((int)v));
    v = max(v, (unsigned)dpp_i<0x141>((int)v));
    v = max(v, (unsigned)dpp_i<0x140>((int)v));
    const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)v, 0), r1 = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
    const unsigned r2 = (unsigned)__builtin_amdgcn_readlane((int)v, 32), r3 = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
    return max(max(r0, r1), max(r2, r3));
}
// the largest key of a wave, in every lane: the largest high word, then the largest low word among the lanes that hold it
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long key) {
    const unsigned hi = (unsigned)(key >> 32), lo = (unsigned)key;
    const unsigned mh = wave_max_u32(hi);
    const unsigned ml = wave_max_u32(hi == mh ? lo : 0u);
    return ((unsigned long long)mh << 32) | ml;
}

// grid = (parts, rows), 256 threads.  Slice p of a row is [p per, min(n, (p + 1) per)), per = ceil(n / parts), walked in tiles of
// 256 * kScoreTopE entries.  A thread holds the high words of its entries of the tile in registers (entry e of thread t is
// tile + 256 e + t: the index is never stored) and, from the second tile on, one key of the best so far.  A round takes the
// workgroup's largest key: every thread keeps the largest it holds, every wave the largest of its threads, and only the wave that
// held the round's winner forms its next one.  The wave maxima change hands in LDS, two sets by turns, one barrier a round.
// A slice or a row shorter than k gives what it has.  Key 0 marks "nothing": only a NaN of all ones at index 0 has it.
// The body is score_top_slice: row l[0 .. n), slice `part` of `parts`, the k largest keys to keys_out[j * parts] (the caller has
// added the part), and with ABOVE the slice's count of keys above tkey to *above_out.  q3_topk.h selects with ABOVE = false.
template <bool ABOVE>
__device__ __forceinline__ void score_top_slice(const float* l, int n, int k, int parts, int part, unsigned long long tkey,
                                                unsigned long long* keys_out, int* above_out) {
    __shared__ unsigned long long best[kScoreTopMax];       // the largest keys so far, descending
    __shared__ unsigned long long wmax[2][4];
    __shared__ int above_lds[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int per = (n + parts - 1) / parts;
    const long long s0 = (long long)part * per;
    const int i0 = (int)(s0 < (long long)n ? s0 : (long long)n), i1 = (int)(s0 + per < (long long)n ? s0 + per : (long long)n);
    int have = 0, above = 0;
    for (int tile = i0; tile < i1; tile += 256 * kScoreTopE) {
        unsigned hi[kScoreTopE];
        float v[kScoreTopE];
        const int cnt = min(i1 - tile, 256 * kScoreTopE);
        // all of the tile's loads in flight at once: an entry past the slice's end reads the slice's last one and is not used
#pragma unroll
        for (int e = 0; e < kScoreTopE; ++e) v[e] = l[min(tile + 256 * e + tid, i1 - 1)];
#pragma unroll
        for (int e = 0; e < kScoreTopE; ++e) {
            const int i = tile + 256 * e + tid;
            const unsigned h = total_order_key(v[e]);
            hi[e] = i < i1 ? h : 0u;
            if (ABOVE) above += (i < i1 && (((unsigned long long)h << 32) | (unsigned)i) > tkey) ? 1 : 0;
        }
        unsigned long long carry = tid < have ? best[tid] : 0ull;
        // the largest key this thread holds and the register it stands in (kScoreTopE: the carry); ties in the high word go to
        // the later entry, the higher index
        unsigned long long mine;
        int at;
        auto rescan = [&] {
            unsigned bh = 0u;
            at = 0;
#pragma unroll
            for (int e = 0; e < kScoreTopE; ++e)
                if (hi[e] >= bh) { bh = hi[e]; at = e; }
            mine = bh ? (((unsigned long long)bh << 32) | (unsigned)(tile + 256 * at + tid)) : 0ull;
            if (carry > mine) { mine = carry; at = kScoreTopE; }
        };
        rescan();
        unsigned long long wbest = wave_max_key(mine);
        if (lane == 0) wmax[0][wave] = wbest;
        __syncthreads();                                    // the carries are read, set 0 stands
        const int rounds = min(k, have + cnt);
        for (int r = 0; r < rounds; ++r) {
            const unsigned long long* w = wmax[r & 1];
            const unsigned long long win = max(max(w[0], w[1]), max(w[2], w[3]));
            if (tid == 0) best[r] = win;
            if (wbest == win) {                             // wave-uniform: this wave held it
                if (mine == win) {
                    if (at == kScoreTopE) carry = 0ull;
#pragma unroll
                    for (int e = 0; e < kScoreTopE; ++e)
                        if (e == at) hi[e] = 0u;
                    rescan();
                }
                wbest = wave_max_key(mine);
            }
            if (lane == 0) wmax[(r + 1) & 1][wave] = wbest;
            __syncthreads();
        }
        have = rounds;
    }
    if (ABOVE) {
        above = group_sum_i32(above, 64);
        if (lane == 0) above_lds[wave] = above;
    }
    __syncthreads();                                        // also: best[] stands when no tile ran
    if (tid < k) keys_out[(size_t)tid * (size_t)parts] = tid < have ? best[tid] : 0ull;
    if (ABOVE && tid == 0) *above_out = (above_lds[0] + above_lds[1]) + (above_lds[2] + above_lds[3]);
}
template <class Src>
__global__ __launch_bounds__(256) void k_score_top_part(const RecordArgs a, const Src src) {
    const int j = blockIdx.y, part = blockIdx.x;
    const int k = src.k();
    if (!src.top_live(j, k)) return;
    const float* l = a.logits + (size_t)j * (size_t)a.n;
    const int target = src.target(a, j, [&] { return record_best(a, j); });
    const unsigned long long tkey = ((unsigned long long)total_order_key(l[target]) << 32) | (unsigned)target;
    score_top_slice<true>(l, a.n, k, a.parts, part, tkey, a.part_keys + (size_t)j * (size_t)k * (size_t)a.parts + (size_t)part,
                          a.part_above + (size_t)j * (size_t)a.parts + (size_t)part);
}

// One wave merges the lists of a row as they stand in LDS, entry j of part p at [j * parts + p]: lane p walks the list of part p
// from its head; a round takes the wave's largest head and the lane that held it steps on (its own counter, below k).  Lane j
// returns the j-th winner (0: none, and in the lanes from k on).
__device__ __forceinline__ unsigned long long score_top_merge_wave(const unsigned long long* lists, int k, int parts, int lane) {
    int h = 0;
    unsigned long long cur = lane < parts ? lists[lane] : 0ull, mine = 0ull;
    for (int r = 0; r < k; ++r) {
        const unsigned long long win = wave_max_key(cur);
        if (lane == r) mine = win;
        if (cur == win && lane < parts) {
            ++h;
            cur = h < k ? lists[h * parts + lane] : 0ull;
        }
    }
    return mine;
}

// grid = rows, 256 threads.  All copy the row's lists into LDS as they stand, entry j of part p at [j][p]; then wave 0 alone goes on.
// Lane p walks the list of part p from its head; a round takes the wave's largest head and the lane that held it steps on (its own
// counter, below k).  Lane j keeps the j-th winner and stores it as {logit, index}; the rank is the sum of the parts' counts.
template <class Src>
__global__ __launch_bounds__(256) void k_score_top_merge(const RecordArgs a, const Src src) {
    __shared__ unsigned long long lists[kScoreTopMax * kScoreTopParts];
    const int lane = threadIdx.x;
    const int j = blockIdx.x;
    const int k = src.k();
    if (!src.top_live(j, k)) return;
    const int total = k * a.parts;
    const unsigned long long* keys = a.part_keys + (size_t)j * (size_t)total;
#pragma unroll 8
    for (int i = threadIdx.x; i < total; i += 256) lists[i] = keys[i];
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int o = src.out(j);
    const unsigned long long mine = score_top_merge_wave(lists, k, a.parts, lane);
    if (lane < k) {
        ScoreTop t;
        t.logit = key_to_float((unsigned)(mine >> 32));
        t.index = (int)(unsigned)(mine & 0xffffffffull);
        src.top()[(size_t)o * (size_t)k + (size_t)lane] = t;
    }
    int* const rank = src.rank();
    if (rank) {
        const int above = group_sum_i32(lane < a.parts ? a.part_above[(size_t)j * (size_t)a.parts + (size_t)lane] : 0, 64);
        if (lane == 0) rank[o] = above;
    }
}

}  // namespace q3
