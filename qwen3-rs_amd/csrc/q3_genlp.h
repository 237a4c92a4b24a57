// q3_genlp.h -- log-probability records of the tokens a q3_generate_many_* loop produces (include/qwen3_hip.h section 2o).
//
// A column pass ends with the classifier's rows l[0 .. V) of its columns in the logits buffer and one argmax key per workgroup in the
// slots; the turn kernel that follows commits a token for every column whose ColEnt::out >= 0.  The launches here sit between the
// two (behind the draws of a sampled plan) and reduce exactly those rows, chosen by the device: row j is column j of the pass, the
// live columns and their destinations are the ColsCtl fields the turn kernel set up (n_live, out[]), and the target is the token
// the turn kernel is about to commit -- cols_commit_token (q3_batch.h), the rule both call.
//   k_genlp_exp, k_genlp_sum             k_score_exp / k_score_sum (q3_score.h) with that row table: the record {l[target], max, sum,
//                                        argmax} goes to recs[out[j]];
//   k_genlp_top_part, k_genlp_top_merge  k_score_top_part / k_score_top_merge (q3_score_top.h): top[out[j] top_n ..] and rank[out[j]].
// A workgroup of a column past n_live or with out[j] < 0 (pads, prompt-interior columns, dense blocks' columns) returns at once.
// The records are taken on the raw logits: temperature 1, the full vocabulary, in front of top-k and top-p.
// Only loop indices, counters, out[j] and the committed token clamped to [0, V) become addresses: no logit and no key read back from
// memory does, so a row that holds a NaN is wrong but harmless.
#pragma once

namespace q3 {

// where a call's results go and how many alternatives it wants: uploaded once per call, read when a pass runs, so plans and graphs
// hold for any top_n and any buffers
struct GenlpCtl {
    ScoreRec* recs;                     // [n_out] of the call
    ScoreTop* top;                      // [n_out][top_n], or null (top_n == 0)
    int* rank;                          // [n_out], or null (top_n == 0)
    int top_n;                          // 0 .. kScoreTopMax
    int pad_;
};

struct GenlpArgs {
    const ColsCtl* cols;                // n_live and out[] of the pass in flight
    const ColsDraw* draw;               // sampled plans: mode[] of the pass in flight; null in a greedy plan
    const State* st;                    // sampled plans: State::token holds the draw, State::argmax the row's largest key
    const GenlpCtl* ctl;
    const float* logits;                // [kColsMax][n]
    const unsigned long long* slots;    // [kColsMax][slot_stride] argmax keys of the classifier launch, nslots of them written per row
    float* probs;                       // [kColsMax][probs_stride] exps scratch (section 2l's)
    unsigned long long* part_keys;      // [kColsMax][top_n][parts]
    int* part_above;                    // [kColsMax][parts]
    long long probs_stride;
    int slot_stride, nslots;
    int n;                              // vocab_size
    int parts;                          // gridDim.x of k_genlp_top_part
};

// the record of column j, or -1: the column emits nothing
__device__ __forceinline__ int genlp_out(const GenlpArgs& a, int j) { return j < a.cols->n_live ? a.cols->out[j] : -1; }

// the token the turn kernel commits for column j (best: the fold of the row's slots, which a sampled plan also holds in
// State::argmax, where k_cols_turn_draw reads it), clamped to the vocabulary
__device__ __forceinline__ int genlp_target(const GenlpArgs& a, int j, unsigned long long best) {
    const int t = a.draw ? cols_commit_token(a.draw->mode[j], a.st[j].argmax, a.st[j].token) : cols_commit_token(kColArgmax, best, 0);
    return min(max(t, 0), a.n - 1);
}

// grid = (kScoreExpParts, width), 256 threads: k_score_exp over the emitting columns
__global__ __launch_bounds__(256) void k_genlp_exp(const GenlpArgs a) {
    const int j = blockIdx.y;
    if (genlp_out(a, j) < 0) return;
    const float mx = key_to_float((unsigned)(spec_col_best(a.slots + (size_t)j * (size_t)a.slot_stride, a.nslots) >> 32));
    const float* l = a.logits + (size_t)j * (size_t)a.n;
    float* p = a.probs + (size_t)j * (size_t)a.probs_stride;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n; i += gridDim.x * 256) p[i] = q3_expf(l[i] - mx);
}

// grid = width, kSampThreads threads: k_score_sum over the emitting columns, the target the committed token
__global__ __launch_bounds__(kSampThreads) void k_genlp_sum(const GenlpArgs a) {
    __shared__ float xch[kSampThreads + 16];
    __shared__ float carry_lds;
    const int j = blockIdx.x;
    const int o = genlp_out(a, j);
    if (o < 0) return;
    const unsigned long long best = spec_col_best(a.slots + (size_t)j * (size_t)a.slot_stride, a.nslots);
    const float sum = wg_walk_segments(a.probs + (size_t)j * (size_t)a.probs_stride, a.n, -0.0f, xch, &carry_lds, nullptr,
                                       [](int, float, float) { return false; });
    if (threadIdx.x == 0) {
        ScoreRec rec;
        rec.target = a.logits[(size_t)j * (size_t)a.n + (size_t)genlp_target(a, j, best)];
        rec.max = key_to_float((unsigned)(best >> 32));
        rec.sum = sum;
        rec.argmax = (int)(unsigned)(best & 0xffffffffull);
        a.ctl->recs[o] = rec;
    }
}

// grid = (parts, width), 256 threads: k_score_top_part over the emitting columns
__global__ __launch_bounds__(256) void k_genlp_top_part(const GenlpArgs a) {
    const int j = blockIdx.y, part = blockIdx.x;
    const int k = a.ctl->top_n;
    if (genlp_out(a, j) < 0 || k < 1 || k > kScoreTopMax) return;
    const float* l = a.logits + (size_t)j * (size_t)a.n;
    const int target = genlp_target(a, j, spec_col_best(a.slots + (size_t)j * (size_t)a.slot_stride, a.nslots));
    const unsigned long long tkey = ((unsigned long long)total_order_key(l[target]) << 32) | (unsigned)target;
    score_top_slice<true>(l, a.n, k, a.parts, part, tkey, a.part_keys + (size_t)j * (size_t)k * (size_t)a.parts + (size_t)part,
                          a.part_above + (size_t)j * (size_t)a.parts + (size_t)part);
}

// grid = width, 256 threads: k_score_top_merge over the emitting columns
__global__ __launch_bounds__(256) void k_genlp_top_merge(const GenlpArgs a) {
    __shared__ unsigned long long lists[kScoreTopMax * kScoreTopParts];
    const int lane = threadIdx.x;
    const int j = blockIdx.x;
    const int o = genlp_out(a, j);
    const int k = a.ctl->top_n;
    if (o < 0 || k < 1 || k > kScoreTopMax) return;
    const int total = k * a.parts;
    const unsigned long long* src = a.part_keys + (size_t)j * (size_t)total;
#pragma unroll 8
    for (int i = threadIdx.x; i < total; i += 256) lists[i] = src[i];
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const unsigned long long mine = score_top_merge_wave(lists, k, a.parts, lane);
    if (lane < k) {
        ScoreTop t;
        t.logit = key_to_float((unsigned)(mine >> 32));
        t.index = (int)(unsigned)(mine & 0xffffffffull);
        a.ctl->top[(size_t)o * (size_t)k + (size_t)lane] = t;
    }
    const int above = group_sum_i32(lane < a.parts ? a.part_above[(size_t)j * (size_t)a.parts + (size_t)lane] : 0, 64);
    if (lane == 0) a.ctl->rank[o] = above;
}

}  // namespace q3
