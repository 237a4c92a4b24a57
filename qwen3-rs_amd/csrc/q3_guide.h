// q3_guide.h -- guided decoding: a token automaton inside the q3_generate_many_* loops (include/qwen3_hip.h section 2r).
//
// A guide is a table next[n_states][V] of int16: next[s][v] >= 0, in state s token v may come and leads to that state; -1, it may
// not.  Request r starts in start[r] (start[0] where there is one entry; -1: unguided) and is about to produce y_g from classifier
// row l[0 .. V) in state s_g.  The MASKED row is
//     next[s_g][v] >= 0:  m[v] = l[v]     (the same bits)
//     otherwise:          m[v] = -inf     (0xFF800000)
// section 2q's table, where set, applies to m in place of l, section 2p's penalties on top.  After the commit
//     s_{g+1} = next[s_g][y_g] where that is >= 0, else s_g
// (the sampler's fall-through and a row with no finite entry can commit a token the state forbids).  Two kernels in the places of
// k_bias_apply and k_bias_count (PlanKey::pen == kPenGuide, q3_plan_host.inc), with their grids, slices and outputs, so everything
// behind them runs as it runs under penalties:
//   k_guide_apply  grid (kPenSlices, width), behind the classifier.  Request and output index as in k_bias_apply; the state is
//                  start[r] where g == 0, else the KV slot's; the state's int16 row streams beside the logits, 8-byte loads where
//                  V % 4 == 0 (a row starts at 2 s V bytes: 8-byte aligned), single entries otherwise.  Then bias_entry and
//                  pen_entry as they are.  Without a table of section 2q BiasCtl holds one empty ADD list.
//   k_guide_step   one workgroup in front of the turn kernel, a thread per column: the slot's next state from the token the column
//                  is about to commit (pen_commit_column), then the count where penalties are set.  For g == 0 it starts from
//                  start[r], so a reused slot needs no reset.  k_guide_apply of a pass has run by then, and a pass has at most one
//                  emitting column per slot: plain loads and stores do.
// The table, start[] and the slots' states stand behind GuideCtl in device memory, read when a pass runs: two guides share every
// plan and graph.  Only loop indices, out[], slot numbers, request indices and states clamped to their arrays and the committed token
// clamped to [0, V) become addresses.
#pragma once
#include "q3_bias.h"

namespace q3 {

constexpr int kGuideMaxStates = 4096;   // Q3_GUIDE_MAX_STATES

typedef short v4s __attribute__((ext_vector_type(4)));

// the guide of the call in flight as the passes read it
struct GuideCtl {
    const short* next;                  // [n_states][n]
    const int* start;                   // [n_start]
    int* state;                         // [max_streams]: the state of the request in every KV slot, written by k_guide_step
    int n_states, n_start;              // n_start == 1: the one start state holds for every request; else start[r] is request r's
};

// request and output index of emitting column j: out == o_off[r] + g with 0 <= g < n_new[r], so r is the last request whose offset
// is not above out
__device__ __forceinline__ void guide_request(const BiasCtl& t, int out, int& r, unsigned& g) {
    int lo = 0, hi = t.n_requests;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.o_off[mid] <= out) lo = mid;
        else hi = mid;
    }
    r = lo;
    g = (unsigned)max(out - t.o_off[lo], 0);
}

// s_g of request r in slot kv: -1 (unguided) or a row of the table
__device__ __forceinline__ int guide_state(const GuideCtl& gc, int r, unsigned g, int kv) {
    const int s = g == 0u ? gc.start[gc.n_start == 1 ? 0 : min(r, gc.n_start - 1)] : gc.state[kv];
    return s < 0 ? -1 : min(s, gc.n_states - 1);
}

__device__ __forceinline__ unsigned guide_mask(unsigned l_bits, short nx) { return nx >= 0 ? l_bits : 0xFF800000u; }

// grid = (kPenSlices, columns), 256 threads; the slices are k_pen_apply's.  a.counts is not read: the counts are BiasCtl's.
__global__ __launch_bounds__(kPenThreads) void k_guide_apply(const PenArgs a, const BiasCtl* __restrict__ bc, const GuideCtl* __restrict__ gcp) {
    __shared__ unsigned long long wbest[kPenThreads / 64];
    const int j = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
    unsigned long long* const slot_out = a.pen_slots + (size_t)j * kPenSlices + s;
    const BiasCtl t = *bc;
    const GuideCtl gc = *gcp;
    int r = 0, kv = 0;
    unsigned g = t.g_op;
    if (a.cols) {
        if (!pen_emits(a.cols, j)) {
            if (tid == 0) *slot_out = 0ull;
            return;
        }
        guide_request(t, a.cols->out[j], r, g);
        kv = min(max(a.col_slot[j], 0), a.max_streams - 1);
    }
    const int n = a.n;
    const int state = guide_state(gc, r, g, kv);
    const bool guided = state >= 0;
    const short* const nx = gc.next + (size_t)max(state, 0) * (size_t)n;
    const int li = t.n_lists == 1 ? 0 : min(r, t.n_lists - 1);
    const bool allow = t.modes[li] == kBiasAllow;
    const int l0 = (int)t.list_off[li], l1 = (int)t.list_off[li + 1];
    const BiasEntry* const ent = t.entries;
    const bool pen = t.counts != nullptr;
    const bool first = a.cols != nullptr && g == 0u;          // a request's first output: all counts zero by the rule, the slot's cleared here
    const float presence = a.ctl->presence, frequency = a.ctl->frequency;
    const float* l = a.logits + (size_t)j * (size_t)n;
    float* o = a.pen_logits + (size_t)j * (size_t)n;
    unsigned* c = t.counts + (size_t)kv * (size_t)n;
    unsigned long long best = 0ull;
    if ((n & 3) == 0) {
        const int units = n >> 2, per = (units + kPenSlices - 1) / kPenSlices;
        const int u0 = min(s * per, units), u1 = min(u0 + per, units);
        const int e0 = bias_lower(ent, l0, l1, 4 * u0), e1 = bias_lower(ent, e0, l1, 4 * u1);
        const bool plain = e0 == e1 && !allow;
        for (int u = u0 + tid; u < u1; u += kPenThreads) {
            v4u ov = *(const v4u*)(l + 4 * (size_t)u);
            if (guided) {
                const v4s nv = *(const v4s*)(nx + 4 * (size_t)u);
                ov.x = guide_mask(ov.x, nv.x);
                ov.y = guide_mask(ov.y, nv.y);
                ov.z = guide_mask(ov.z, nv.z);
                ov.w = guide_mask(ov.w, nv.w);
            }
            if (!plain) {
                ov.x = bias_entry(ov.x, 4 * u, ent, e0, e1, allow, g);
                ov.y = bias_entry(ov.y, 4 * u + 1, ent, e0, e1, allow, g);
                ov.z = bias_entry(ov.z, 4 * u + 2, ent, e0, e1, allow, g);
                ov.w = bias_entry(ov.w, 4 * u + 3, ent, e0, e1, allow, g);
            }
            if (pen) {
                if (first) {
                    *(v4u*)(c + 4 * (size_t)u) = v4u{0u, 0u, 0u, 0u};
                } else {
                    const v4u cv = *(const v4u*)(c + 4 * (size_t)u);
                    ov.x = pen_entry(ov.x, cv.x, presence, frequency);
                    ov.y = pen_entry(ov.y, cv.y, presence, frequency);
                    ov.z = pen_entry(ov.z, cv.z, presence, frequency);
                    ov.w = pen_entry(ov.w, cv.w, presence, frequency);
                }
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
        const int e0 = bias_lower(ent, l0, l1, i0), e1 = bias_lower(ent, e0, l1, i1);
        const bool plain = e0 == e1 && !allow;
        for (int i = i0 + tid; i < i1; i += kPenThreads) {
            unsigned ob = __float_as_uint(l[i]);
            if (guided) ob = guide_mask(ob, nx[i]);
            if (!plain) ob = bias_entry(ob, i, ent, e0, e1, allow, g);
            if (pen) {
                if (first) c[i] = 0u;
                else ob = pen_entry(ob, c[i], presence, frequency);
            }
            o[i] = __uint_as_float(ob);
            best = max(best, pen_key(ob, i));
        }
    }
    best = wave_max_key(best);
    if ((tid & 63) == 0) wbest[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) *slot_out = max(max(wbest[0], wbest[1]), max(wbest[2], wbest[3]));
}

// one workgroup of kColsMax threads, a thread per column, in front of the turn kernel: the slot's state steps over the token the
// column is about to commit, and the token enters the slot's counts where penalties are set
__global__ __launch_bounds__(64) void k_guide_step(PenArgs a, const BiasCtl* __restrict__ bc, const GuideCtl* __restrict__ gcp) {
    const int j = threadIdx.x;
    if (j >= kColsMax || !pen_emits(a.cols, j)) return;
    const int token = pen_commit_column(a, j);
    const int kv = min(max(a.col_slot[j], 0), a.max_streams - 1);
    const GuideCtl gc = *gcp;
    int r;
    unsigned g;
    guide_request(*bc, a.cols->out[j], r, g);
    const int state = guide_state(gc, r, g, kv);
    int to = state;
    if (state >= 0) {
        const int nx = gc.next[(size_t)state * (size_t)a.n + (size_t)token];
        if (nx >= 0) to = min(nx, gc.n_states - 1);
    }
    gc.state[kv] = to;
    a.counts = bc->counts;
    if (a.counts) a.counts[(size_t)kv * (size_t)a.n + (size_t)token] += 1u;
}

}  // namespace q3
