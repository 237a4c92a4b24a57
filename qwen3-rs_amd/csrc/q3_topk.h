// q3_topk.h -- top-k sampling: Sampler::sample among the k best tokens (include/qwen3_hip.h section 2n).
//
// A draw with top_k = k is the reference's Sampler::sample (q3_sampler.h) on the logits with every entry outside the SURVIVOR SET
// replaced by -inf.  The survivors are the k largest entries under the key of q3_score_top.h,
//     ((uint64)total_order_key(l[i]) << 32) | i,
// so equal logits go to the higher index and k = 1 leaves the argmax.  A masked entry has e = exp(-inf) = +0.0 and p = +0.0: it adds
// an exact zero to every running sum of the reference and fails the nucleus cutoff, so the softmax denominator, the cdf and the
// nucleus are sums over the survivors alone, in the reference's order -- ascending token index, or (probability descending, index
// ascending) -- and at most 64 terms long.  One wave forms them term by term; nothing is guessed, binned or radix sorted.
//   k_topk_part   grid (parts, columns): score_top_slice of q3_score_top.h, the k largest keys of one slice of a column's logits;
//   k_topk_draw   grid columns, one wave: merges the slices' lists, puts the survivors in ascending index order and draws.
// One deviation from the masked reference: a multinomial walk whose cdf ends below the coin returns the highest-index survivor (the
// reference returns index V - 1, which is masked).
// As in q3_score_top.h no logit and no key read back from memory becomes an address; the drawn index is clamped to the vocabulary.
#pragma once
#include "q3_sampler.h"
#include "q3_score_top.h"

namespace q3 {

constexpr int kTopkMax = kScoreTopMax;                          // Q3_TOP_K_MAX
constexpr int kTopkColKeys = kScoreTopMax * kScoreTopParts;     // keys of a column in TopkArgs::part_keys

struct TopkArgs {
    const float* logits;                // column c: logits + c * sb_logits, n entries
    long long sb_logits;
    int n;                              // vocab_size
    int parts;                          // 1 .. kScoreTopParts: gridDim.x of k_topk_part
    const int* k;                       // the engine's top_k, read when the pass runs
    unsigned long long* part_keys;      // [columns][kTopkColKeys]: entry j of slice p of a column at [j * parts + p]
    SamplerState* ss;                   // per column, as SampleArgs::ss
    State* st;
    int32_t* out_tokens;                // column c: out_tokens + c * out_cap
    int out_cap;
};

// the k of this pass: what the host stored, kept inside what the buffers hold whatever the word says
__device__ __forceinline__ int topk_k(const TopkArgs& a) {
    const int k = *a.k;
    return max(1, min(k, min(kTopkMax, a.n)));
}

__device__ __forceinline__ float wave_lane_f32(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// grid = (parts, columns), 256 threads.  A column that does not draw (a discarded prompt-position draw, a temperature-0 slot or a
// pad of a column pass: State::step < State::prompt_len, k_sample_exp's rule) returns at once.
__global__ __launch_bounds__(256) void k_topk_part(const TopkArgs a) {
    const size_t col = blockIdx.y;
    const State* st = a.st + col;
    if (st->step < st->prompt_len) return;
    score_top_slice<false>(a.logits + col * (size_t)a.sb_logits, a.n, topk_k(a), a.parts, (int)blockIdx.x, 0ull,
                           a.part_keys + col * (size_t)kTopkColKeys + blockIdx.x, nullptr);
}

// grid = columns, 64 threads.  k_sample's contract: the column's rng moves on by one coin, also for a discarded draw, which then
// returns; the drawn token replaces State::token and out_tokens[step - 1].
__global__ __launch_bounds__(64) void k_topk_draw(const TopkArgs a) {
    __shared__ unsigned long long lists[kTopkColKeys];
    __shared__ float asc_l[kTopkMax], srt_p[kTopkMax];
    __shared__ int asc_i[kTopkMax], srt_i[kTopkMax];
    const int lane = threadIdx.x;
    const size_t col = blockIdx.x;
    State* st = a.st + col;
    SamplerState* ss = a.ss + col;
    const float temperature = ss->temperature, topp = ss->topp;
    const bool discard = st->step < st->prompt_len;
    unsigned long long rs = ss->rng;
    rs ^= rs >> 12;
    rs ^= rs << 25;
    rs ^= rs >> 27;                                               // sampler.rs:44-49
    const unsigned r32 = (unsigned)((rs * 0x2545F4914F6CDD1Dull) >> 32);
    const float coin = (float)(r32 >> 8) / 16777216.0f;          // sampler.rs:52-54
    if (lane == 0) ss->rng = rs;
    if (discard) return;

    const int n = a.n, k = topk_k(a), parts = a.parts, total = k * parts;
    const unsigned long long* src = a.part_keys + col * (size_t)kTopkColKeys;
    for (int i = lane; i < total; i += 64) lists[i] = src[i];
    __syncthreads();
    // lane j: the j-th largest key of the column
    const unsigned long long mine = score_top_merge_wave(lists, k, parts, lane);
    const bool live = mine != 0ull;
    const float my_l = key_to_float((unsigned)(mine >> 32));
    const int my_i = (int)(unsigned)(mine & 0xffffffffull);
    const unsigned long long live_mask = __builtin_amdgcn_ballot_w64(live);
    const int m = __builtin_popcountll(live_mask);               // survivors
    const float l_max = wave_lane_f32(my_l, 0);

    // ascending token index: a survivor's place is the number of survivors with a lower index (indices are distinct)
    int at = 0;
    for (int b = 0; b < k; ++b) {
        const int ib = __builtin_amdgcn_readlane(my_i, b);
        at += (((live_mask >> b) & 1ull) != 0ull && ib < my_i) ? 1 : 0;
    }
    if (live) { asc_l[at] = my_l; asc_i[at] = my_i; }
    __syncthreads();
    const bool in = lane < m;
    const int idx = in ? asc_i[lane] : 0;
    // e = exp(l / T - max), the maximum being the scaled top survivor; sum from -0.0 in index order; p = e * (1 / sum)
    const float mx = l_max / temperature;
    const float e = in ? q3_expf(asc_l[lane] / temperature - mx) : 0.0f;
    float sum = -0.0f;
    for (int b = 0; b < m; ++b) sum = sum + wave_lane_f32(e, b);
    const float inv = 1.0f / sum;
    const float p = e * inv;

    int result = 0;
    if (topp <= 0.0f || topp >= 1.0f) {
        // sample_mult over the survivors: first i with coin < cdf_i, cdf from 0.0                  sampler.rs:62-71
        float cdf = 0.0f;
        int hit = -1;
        for (int b = 0; b < m; ++b) {
            cdf = cdf + wave_lane_f32(p, b);
            if (coin < cdf) { hit = b; break; }
        }
        if (hit < 0) hit = m - 1;                                  // the walk fell through: the highest-index survivor
        result = m > 0 ? asc_i[hit] : 0;
    } else {
        // sample_topp: the cutoff of the FULL vocabulary, candidates by (probability descending, index ascending)   sampler.rs:74-112
        const float cutoff = (1.0f - topp) / (float)((n - 1) > 1 ? (n - 1) : 1);
        const bool cand = in && p >= cutoff;
        const unsigned pk = total_order_key(p);
        const unsigned long long cand_mask = __builtin_amdgcn_ballot_w64(cand);
        const int n0 = __builtin_popcountll(cand_mask);
        int place = 0;
        for (int b = 0; b < m; ++b) {
            const unsigned pb = (unsigned)__builtin_amdgcn_readlane((int)pk, b);
            place += (((cand_mask >> b) & 1ull) != 0ull && (pb > pk || (pb == pk && b < lane))) ? 1 : 0;
        }
        if (cand) { srt_p[place] = p; srt_i[place] = idx; }
        __syncthreads();
        const float sp = lane < n0 ? srt_p[lane] : 0.0f;
        float cumulative = 0.0f;
        int last_idx = n0 > 0 ? n0 - 1 : 0;
        for (int b = 0; b < n0; ++b) {
            cumulative = cumulative + wave_lane_f32(sp, b);
            if (cumulative > topp) { last_idx = b; break; }
        }
        const float r = coin * cumulative;
        float cdf = 0.0f;
        int hit = last_idx;
        for (int b = 0; b <= last_idx && b < n0; ++b) {
            cdf = cdf + wave_lane_f32(sp, b);
            if (r < cdf) { hit = b; break; }
        }
        result = n0 > 0 ? srt_i[hit] : 0;
    }
    result = max(0, min(result, n - 1));
    if (lane == 0) {
        // k_next already advanced (pos, step) and stored the argmax: the sampled token replaces it
        st->token = result;
        const int s = st->step - 1;
        if (s >= 0 && s < a.out_cap) a.out_tokens[col * (size_t)a.out_cap + (size_t)s] = result;
    }
}

}  // namespace q3
