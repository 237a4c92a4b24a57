// q3_penalty.h -- presence and frequency penalties inside the q3_generate_many_* loops (include/qwen3_hip.h section 2p).
//
// Request r has produced y_0 .. y_{j-1}; c[v] counts the i < j with y_i == v.  Its next token is taken from the PENALISED row
//     c[v] == 0:  l'[v] = l[v]                                        (the same bits)
//     c[v] >  0:  l'[v] = l[v] - (presence + frequency * (float)c[v])  (multiply, add, subtract: three f32 roundings, nothing fused)
// of its classifier row l[0 .. V).  Two kernels around what a column plan already runs (PlanKey::pen, q3_plan_host.inc):
//   k_pen_apply   grid (kPenSlices, width), behind the classifier: l' of every emitting column into a buffer of its own -- the
//                 classifier's output is never written -- and per slice the largest key ((uint64)total_order_key(l'[v]) << 32) | v, the
//                 key format of the classifier's argmax slots, so spec_col_best folds them as it folds those;
//   k_pen_count   one workgroup in front of the turn kernel: counts[slot][token] += 1 for the token the turn kernel is about to commit
//                 (cols_commit_token, the rule the turn kernels and the records of q3_genlp.h share).
// The counts belong to the KV slot.  The column that emits a request's FIRST token -- the emitting column whose token comes from the
// prompt, ColEnt::src >= 0, read from the table row the pass was set up from -- has all counts zero by the rule: its slices copy the
// row and clear their part of the slot's counts, which is how a reused slot starts empty without a launch of its own.
// Only loop indices, out[], slot numbers and the committed token clamped to [0, V) become addresses: a NaN logit is wrong but harmless.
#pragma once
#include "q3_score_top.h"

namespace q3 {

constexpr int kPenSlices = 64;          // slices per row of k_pen_apply: k_topk_part's grid
constexpr int kPenThreads = 256;

// the engine-wide setting as the passes read it: written by q3_sampler_penalties, read when a pass runs, so two non-zero settings
// share every plan and graph
struct PenCtl {
    float presence, frequency;
};

struct PenArgs {
    const float* logits;                // [columns][n]: the classifier's output, read only
    float* pen_logits;                  // [columns][n]: l' of the emitting columns
    unsigned* counts;                   // [max_streams][n] per KV slot (operator entry: [n], read only)
    unsigned long long* pen_slots;      // [columns][kPenSlices]: the largest key of every slice of l'; 0 where the column emits nothing
    const PenCtl* ctl;
    const ColsCtl* cols;                // the pass in flight; null: the operator entry -- one row, emitting, counts as given
    const ColsDraw* draw;               // sampled plans: mode[] of the pass in flight; null in a greedy plan
    const State* st;                    // sampled plans: State::argmax holds the fold of pen_slots, State::token the draw
    const int* col_slot;                // KV slot of every column of the pass in flight
    int n;                              // vocab_size
    int max_streams;
};

// l' of one entry, on the bits: an entry that was never produced keeps its bits whatever they are
__device__ __forceinline__ unsigned pen_entry(unsigned l_bits, unsigned c, float presence, float frequency) {
    const float p = __fadd_rn(presence, __fmul_rn(frequency, (float)c));
    const unsigned pen = __float_as_uint(__fsub_rn(__uint_as_float(l_bits), p));
    return c ? pen : l_bits;
}
__device__ __forceinline__ unsigned long long pen_key(unsigned bits, int i) {
    return ((unsigned long long)total_order_key(__uint_as_float(bits)) << 32) | (unsigned)i;
}

// the pass's record of column j: does it emit, and is what it emits its request's first token
__device__ __forceinline__ bool pen_emits(const ColsCtl* c, int j) { return j < c->n_live && c->out[j] >= 0; }
__device__ __forceinline__ bool pen_first(const ColsCtl* c, int j) {
    // the turn kernel that set the pass up left the cursor one behind its row
    const int p = c->cursor - 1;
    return p >= 0 && c->table != nullptr && c->table[(size_t)p * kColsMax + j].src >= 0;
}

// grid = (kPenSlices, columns), 256 threads.  Slice s of a row is [s per, min(n, (s + 1) per)) in units of four entries where
// n % 4 == 0 (16-byte loads and stores), of one entry otherwise.
__global__ __launch_bounds__(kPenThreads) void k_pen_apply(const PenArgs a) {
    __shared__ unsigned long long wbest[kPenThreads / 64];
    const int j = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
    unsigned long long* const slot_out = a.pen_slots + (size_t)j * kPenSlices + s;
    bool first = false;
    int kv = 0;
    if (a.cols) {
        if (!pen_emits(a.cols, j)) {
            if (tid == 0) *slot_out = 0ull;
            return;
        }
        first = pen_first(a.cols, j);
        kv = min(max(a.col_slot[j], 0), a.max_streams - 1);
    }
    const float presence = a.ctl->presence, frequency = a.ctl->frequency;
    const int n = a.n;
    const float* l = a.logits + (size_t)j * (size_t)n;
    float* o = a.pen_logits + (size_t)j * (size_t)n;
    unsigned* c = a.counts + (size_t)kv * (size_t)n;
    unsigned long long best = 0ull;
    if ((n & 3) == 0) {
        const int units = n >> 2, per = (units + kPenSlices - 1) / kPenSlices;
        const int u0 = min(s * per, units), u1 = min(u0 + per, units);
        for (int u = u0 + tid; u < u1; u += kPenThreads) {
            const v4u lv = *(const v4u*)(l + 4 * (size_t)u);
            v4u ov = lv;
            if (first) {
                *(v4u*)(c + 4 * (size_t)u) = v4u{0u, 0u, 0u, 0u};
            } else {
                const v4u cv = *(const v4u*)(c + 4 * (size_t)u);
                ov.x = pen_entry(lv.x, cv.x, presence, frequency);
                ov.y = pen_entry(lv.y, cv.y, presence, frequency);
                ov.z = pen_entry(lv.z, cv.z, presence, frequency);
                ov.w = pen_entry(lv.w, cv.w, presence, frequency);
            }
            *(v4u*)(o + 4 * (size_t)u) = ov;
            // ascending index: a later entry of equal value has the larger key
            best = max(best, pen_key(ov.x, 4 * u));
            best = max(best, pen_key(ov.y, 4 * u + 1));
            best = max(best, pen_key(ov.z, 4 * u + 2));
            best = max(best, pen_key(ov.w, 4 * u + 3));
        }
    } else {
        const int per = (n + kPenSlices - 1) / kPenSlices;
        const int i0 = min(s * per, n), i1 = min(i0 + per, n);
        for (int i = i0 + tid; i < i1; i += kPenThreads) {
            const unsigned lb = __float_as_uint(l[i]);
            unsigned ob = lb;
            if (first) c[i] = 0u;
            else ob = pen_entry(lb, c[i], presence, frequency);
            o[i] = __uint_as_float(ob);
            best = max(best, pen_key(ob, i));
        }
    }
    best = wave_max_key(best);
    if ((tid & 63) == 0) wbest[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) *slot_out = max(max(wbest[0], wbest[1]), max(wbest[2], wbest[3]));
}

// one workgroup of kColsMax threads, a thread per column, in front of the turn kernel: the token an emitting column is about to
// commit enters its slot's counts.  A pass has at most one emitting column per slot, so plain loads and stores do.
// (pen_commit_column: that token of emitting column j, clamped to [0, V))
__device__ __forceinline__ int pen_commit_column(const PenArgs& a, int j) {
    unsigned long long best;
    if (a.draw) {
        best = a.st[j].argmax;
    } else {
        best = 0ull;
        const unsigned long long* s = a.pen_slots + (size_t)j * kPenSlices;
        for (int i = 0; i < kPenSlices; ++i) best = max(best, s[i]);
    }
    const int t = cols_commit_token(a.draw ? a.draw->mode[j] : kColArgmax, best, a.st[j].token);
    return min(max(t, 0), a.n - 1);
}
__device__ __forceinline__ void pen_count_column(const PenArgs& a, int j) {
    if (j >= kColsMax || !pen_emits(a.cols, j)) return;
    const int token = pen_commit_column(a, j);
    const int kv = min(max(a.col_slot[j], 0), a.max_streams - 1);
    a.counts[(size_t)kv * (size_t)a.n + (size_t)token] += 1u;
}

__global__ __launch_bounds__(64) void k_pen_count(const PenArgs a) { pen_count_column(a, threadIdx.x); }

}  // namespace q3
