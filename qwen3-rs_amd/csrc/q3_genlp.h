// q3_genlp.h -- log-probability records of the tokens a q3_generate_many_* loop produces (include/qwen3_hip.h section 2o).
//
// A column pass ends with the classifier's rows l[0 .. V) of its columns in the logits buffer and one argmax key per workgroup in the
// slots; the turn kernel that follows commits a token for every column whose ColEnt::out >= 0.  Between the two (behind the draws of
// a sampled plan) stand the record kernels of q3_score.h and q3_score_top.h over the row source below, PassRows: they reduce exactly
// those rows, chosen by the device.  Row j is column j of the pass, the live columns and their destinations are the ColsCtl fields
// the turn kernel set up (n_live, out[]), and the target is the token the turn kernel is about to commit -- cols_commit_token
// (q3_batch.h), the rule both call.  The record {l[target], max, sum, argmax} goes to recs[out[j]], the alternatives to
// top[out[j] top_n ..] and rank[out[j]].
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

// The rows of a column pass in flight (the source of q3_score.h's kernels): everything is read from device memory when the pass runs.
struct PassRows {
    const ColsCtl* cols;                // n_live and out[] of the pass in flight
    const ColsDraw* draw;               // sampled plans: mode[] of the pass in flight; null in a greedy plan
    const State* st;                    // sampled plans: State::token holds the draw, State::argmax the row's largest key
    const GenlpCtl* ctl;
    int pen;                            // 1: a plan under penalties (q3_penalty.h) -- State::argmax holds the largest key of the PENALISED
                                        // row in a greedy plan too (k_spec_colmax over its slices), and the committed token is that key's
    // the record of column j, or -1: the column emits nothing
    __device__ __forceinline__ int out(int j) const { return j < cols->n_live ? cols->out[j] : -1; }
    __device__ __forceinline__ bool live(int j) const { return out(j) >= 0; }
    __device__ __forceinline__ bool top_live(int j, int k) const { return live(j) && k >= 1 && k <= kScoreTopMax; }
    // the token the turn kernel commits for column j (best(): the fold of the row's slots, which a sampled plan also holds in
    // State::argmax, where k_cols_turn_draw reads it; under penalties the fold of the penalised row's slices), clamped to the vocabulary
    template <class Best>
    __device__ __forceinline__ int target(const RecordArgs& a, int j, Best&& best) const {
        const int t = draw ? cols_commit_token(draw->mode[j], st[j].argmax, st[j].token) : cols_commit_token(kColArgmax, pen ? st[j].argmax : best(), 0);
        return min(max(t, 0), a.n - 1);
    }
    __device__ __forceinline__ int k() const { return ctl->top_n; }
    __device__ __forceinline__ ScoreRec* recs() const { return ctl->recs; }
    __device__ __forceinline__ ScoreTop* top() const { return ctl->top; }
    __device__ __forceinline__ int* rank() const { return ctl->rank; }
};

}  // namespace q3
