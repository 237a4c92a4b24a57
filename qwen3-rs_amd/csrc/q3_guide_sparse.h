// q3_guide_sparse.h -- the sparse guide: section 2r's rule on a compressed token automaton (include/qwen3_hip.h section 2s).
//
// The rule is q3_guide.h's, unchanged: masked row, -inf as 0xFF800000, section 2q's table on m, section 2p's penalties on top, the
// state stays over a forbidden commit, start[r] == -1 is unguided.  Only the statement of next[s][v] differs:
//     dflt[n_states]            what every unlisted token does in state s: -1 forbidden, else the state it leads to
//     row_off[n_states + 1]     state s owns edges[row_off[s] .. row_off[s + 1])
//     edges[n_edges]            (token, next), tokens strictly ascending within a state, next -1 or a state
//     next[s][v] = the edge's next where v is listed in state s, else dflt[s]
// Two kernels in the places of k_guide_apply and k_guide_step (PlanKey::pen == kPenGuideSp, q3_plan_host.inc), with their grids,
// slices and outputs:
//   k_guide_sp_apply  grid (kPenSlices, width).  Request, output index, state and slot as in k_guide_apply.  The workgroup finds the
//                     part [e0, e1) of the state's edges that falls into its slice by two searches.  Where that is empty the
//                     allowed bit is uniform (dflt[s] >= 0) and nothing more is read.  Otherwise the slice is walked in chunks of
//                     kGuideSpChunk tokens: a byte per token in LDS is filled with the default, all threads stream the chunk's edges
//                     (8-byte loads, coalesced) and store one byte each -- distinct addresses, the tokens ascend strictly -- and
//                     behind a barrier the chunk's logits stream as in k_guide_apply with the flag read from LDS.  Every barrier
//                     sits in control flow that depends on the state, the slice and the edge list alone: uniform over the
//                     workgroup.  A slice of V = 151,936 is 2,376 tokens: one chunk.
//   k_guide_sp_step   one workgroup, a thread per column: one search of the state's edges for the token about to be committed, else
//                     dflt; state[slot] = to >= 0 ? to : s; then the count where penalties are set.
// Per emitting column the apply kernel moves 8 V + 8 E_s bytes (E_s the state's edges) against k_guide_apply's 10 V.
// Only clamped values become addresses: states to [-1, n_states), edge indices to the state's range inside [0, n_edges], the token
// of an edge to its chunk, the committed token to [0, V), slots, requests and out[] as in q3_guide.h.
#pragma once
#include "q3_guide.h"

namespace q3 {

constexpr int kGuideSpMaxStates = 1 << 20;      // Q3_GUIDE_SPARSE_MAX_STATES
constexpr int kGuideSpMaxEdges = 1 << 27;       // Q3_GUIDE_SPARSE_MAX_EDGES
constexpr int kGuideSpChunk = 4096;             // tokens per pass over the flag bytes in LDS

struct GuideEdge {                              // q3_guide_edge
    int token;
    int next;
};

// the sparse guide of the call in flight as the passes read it
struct GuideSpCtl {
    const int* dflt;                    // [n_states]
    const unsigned* row_off;            // [n_states + 1]
    const GuideEdge* edges;             // [n_edges]
    const int* start;                   // [n_start]
    int* state;                         // [max_streams]: the state of the request in every KV slot, written by k_guide_sp_step
    int n_states, n_start;              // n_start == 1: the one start state holds for every request; else start[r] is request r's
    int n_edges, pad_;
};

// guide_state over a sparse guide
__device__ __forceinline__ int guide_sp_state(const GuideSpCtl& gc, int r, unsigned g, int kv) {
    const int s = g == 0u ? gc.start[gc.n_start == 1 ? 0 : min(r, gc.n_start - 1)] : gc.state[kv];
    return s < 0 ? -1 : min(s, gc.n_states - 1);
}

// the edges of state s (>= 0) as a range inside [0, n_edges]
__device__ __forceinline__ void guide_sp_range(const GuideSpCtl& gc, int s, int& lo, int& hi) {
    lo = (int)min(gc.row_off[s], (unsigned)gc.n_edges);
    hi = (int)min(max(gc.row_off[s + 1], (unsigned)lo), (unsigned)gc.n_edges);
}

// the first index of e[lo .. hi) whose token is not below `token` (hi where there is none); the host steps the stop sequences of
// q3_stop_seq.h through it too
__host__ __device__ __forceinline__ int guide_sp_lower(const GuideEdge* e, int lo, int hi, int token) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid].token < token) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The flag bytes of tokens [c0, c1), c1 - c0 <= kGuideSpChunk, from the state's edges ed[k0 .. k1) that fall into it: the default,
// then a byte per edge.  Called by the whole workgroup; the barrier in front keeps the readers of the chunk before.
__device__ __forceinline__ void guide_sp_flags(unsigned* flags, const GuideEdge* ed, int k0, int k1, int c0, int c1, bool dflt_ok, int tid) {
    __syncthreads();
    const unsigned fill = dflt_ok ? 0x01010101u : 0u;
    for (int w = tid; 4 * w < c1 - c0; w += kPenThreads) flags[w] = fill;
    __syncthreads();
    unsigned char* const fb = (unsigned char*)flags;
    for (int k = k0 + tid; k < k1; k += kPenThreads) {
        const GuideEdge ge = ed[k];
        fb[min(max(ge.token - c0, 0), kGuideSpChunk - 1)] = ge.next >= 0 ? 1 : 0;
    }
    __syncthreads();
}

__device__ __forceinline__ unsigned guide_sp_mask(unsigned l_bits, unsigned ok) { return ok ? l_bits : 0xFF800000u; }

// grid = (kPenSlices, columns), 256 threads; the slices are k_pen_apply's.  a.counts is not read: the counts are BiasCtl's.
__global__ __launch_bounds__(kPenThreads) void k_guide_sp_apply(const PenArgs a, const BiasCtl* __restrict__ bc, const GuideSpCtl* __restrict__ gcp) {
    __shared__ unsigned long long wbest[kPenThreads / 64];
    __shared__ unsigned flags[kGuideSpChunk / 4];
    const int j = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
    unsigned long long* const slot_out = a.pen_slots + (size_t)j * kPenSlices + s;
    const BiasCtl t = *bc;
    const GuideSpCtl gc = *gcp;
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
    const int state = guide_sp_state(gc, r, g, kv);
    // an unguided request: everything allowed, no edges
    const bool dflt_ok = state < 0 || gc.dflt[state] >= 0;
    int s0 = 0, s1 = 0;
    if (state >= 0) guide_sp_range(gc, state, s0, s1);
    const GuideEdge* const ed = gc.edges;
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
    const unsigned char* const fb = (const unsigned char*)flags;
    unsigned long long best = 0ull;
    if ((n & 3) == 0) {
        const int units = n >> 2, per = (units + kPenSlices - 1) / kPenSlices;
        const int u0 = min(s * per, units), u1 = min(u0 + per, units);
        const int e0 = bias_lower(ent, l0, l1, 4 * u0), e1 = bias_lower(ent, e0, l1, 4 * u1);
        const bool plain = e0 == e1 && !allow;
        const int g0 = guide_sp_lower(ed, s0, s1, 4 * u0), g1 = guide_sp_lower(ed, g0, s1, 4 * u1);
        for (int c0 = u0, k0 = g0; c0 < u1; c0 += kGuideSpChunk / 4) {
            const int c1 = min(c0 + kGuideSpChunk / 4, u1);
            const int k1 = g0 == g1 ? g1 : guide_sp_lower(ed, k0, g1, 4 * c1);
            const bool listed = k0 != k1;
            if (listed) guide_sp_flags(flags, ed, k0, k1, 4 * c0, 4 * c1, dflt_ok, tid);
            const unsigned same = dflt_ok ? 0x01010101u : 0u;
            for (int u = c0 + tid; u < c1; u += kPenThreads) {
                v4u ov = *(const v4u*)(l + 4 * (size_t)u);
                const unsigned f = listed ? flags[u - c0] : same;
                ov.x = guide_sp_mask(ov.x, f & 0xffu);
                ov.y = guide_sp_mask(ov.y, f & 0xff00u);
                ov.z = guide_sp_mask(ov.z, f & 0xff0000u);
                ov.w = guide_sp_mask(ov.w, f & 0xff000000u);
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
            k0 = k1;
        }
    } else {
        const int per = (n + kPenSlices - 1) / kPenSlices;
        const int i0 = min(s * per, n), i1 = min(i0 + per, n);
        const int e0 = bias_lower(ent, l0, l1, i0), e1 = bias_lower(ent, e0, l1, i1);
        const bool plain = e0 == e1 && !allow;
        const int g0 = guide_sp_lower(ed, s0, s1, i0), g1 = guide_sp_lower(ed, g0, s1, i1);
        for (int c0 = i0, k0 = g0; c0 < i1; c0 += kGuideSpChunk) {
            const int c1 = min(c0 + kGuideSpChunk, i1);
            const int k1 = g0 == g1 ? g1 : guide_sp_lower(ed, k0, g1, c1);
            const bool listed = k0 != k1;
            if (listed) guide_sp_flags(flags, ed, k0, k1, c0, c1, dflt_ok, tid);
            for (int i = c0 + tid; i < c1; i += kPenThreads) {
                unsigned ob = guide_sp_mask(__float_as_uint(l[i]), listed ? (unsigned)fb[i - c0] : (unsigned)dflt_ok);
                if (!plain) ob = bias_entry(ob, i, ent, e0, e1, allow, g);
                if (pen) {
                    if (first) c[i] = 0u;
                    else ob = pen_entry(ob, c[i], presence, frequency);
                }
                o[i] = __uint_as_float(ob);
                best = max(best, pen_key(ob, i));
            }
            k0 = k1;
        }
    }
    best = wave_max_key(best);
    if ((tid & 63) == 0) wbest[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) *slot_out = max(max(wbest[0], wbest[1]), max(wbest[2], wbest[3]));
}

// one workgroup of kColsMax threads, a thread per column, in front of the turn kernel: the slot's state steps over the token the
// column is about to commit, and the token enters the slot's counts where penalties are set
__global__ __launch_bounds__(64) void k_guide_sp_step(PenArgs a, const BiasCtl* __restrict__ bc, const GuideSpCtl* __restrict__ gcp) {
    const int j = threadIdx.x;
    if (j >= kColsMax || !pen_emits(a.cols, j)) return;
    const int token = pen_commit_column(a, j);
    const int kv = min(max(a.col_slot[j], 0), a.max_streams - 1);
    const GuideSpCtl gc = *gcp;
    int r;
    unsigned g;
    guide_request(*bc, a.cols->out[j], r, g);
    const int state = guide_sp_state(gc, r, g, kv);
    int to = state;
    if (state >= 0) {
        int lo, hi;
        guide_sp_range(gc, state, lo, hi);
        const int k = guide_sp_lower(gc.edges, lo, hi, token);
        const int nx = k < hi && gc.edges[k].token == token ? gc.edges[k].next : gc.dflt[state];
        if (nx >= 0) to = min(nx, gc.n_states - 1);
    }
    gc.state[kv] = to;
    a.counts = bc->counts;
    if (a.counts) a.counts[(size_t)kv * (size_t)a.n + (size_t)token] += 1u;
}

}  // namespace q3
