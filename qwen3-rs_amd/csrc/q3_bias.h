// q3_bias.h -- logit bias, banned and allowed tokens inside the q3_generate_many_* loops (include/qwen3_hip.h section 2q).
//
// Request r is about to produce its output y_g from classifier row l[0 .. V).  Its list -- at most kBiasMax entries (token, bias, until),
// sorted by token on the host, tokens distinct -- and its mode give the ADJUSTED row
//     listed, active (until == 0 || g < until), bias != +-0:  a[v] = l[v] + bias      (one f32 rounding; bias -inf gives -inf)
//     listed otherwise, or unlisted under kBiasAdd:           a[v] = l[v]             (the same bits)
//     unlisted under kBiasAllow:                              a[v] = -inf             (0xFF800000)
// and section 2p's penalties, where set, then apply to a in place of l.  One kernel in the place of k_pen_apply (PlanKey::pen ==
// kPenAdj, q3_plan_host.inc), with its grid, its slices and its two outputs -- the adjusted rows in the buffer of the penalised ones,
// the slices' largest keys in the key format of the classifier's argmax slots -- so everything behind it (k_spec_colmax, the draws,
// the top-k selection, the turn kernels) runs as it runs under penalties:
//   k_bias_apply  grid (kPenSlices, width), behind the classifier.  A column that emits nothing stores key 0 and returns.  An emitting
//                 column finds its request and output index from ColsCtl::out[j] == o_off[r] + g by a search over o_off, then the
//                 sub-range of its list that falls into the slice; a slice with an empty sub-range under kBiasAdd copies.
//   k_bias_count  k_pen_count over the counts BiasCtl names; nothing where it names none (no penalties).
// The tables and the counts pointer stand behind BiasCtl in device memory, written per call and read when a pass runs: two tables,
// and penalties on or off, share every plan and graph.
// Only loop indices, out[], slot numbers, request and entry indices clamped to their arrays and the committed token clamped to [0, V)
// become addresses: a NaN logit (+inf + -inf) is wrong but harmless.
#pragma once
#include "q3_penalty.h"

namespace q3 {

constexpr int kBiasMax = 4096;          // Q3_BIAS_MAX
enum { kBiasAdd = 0, kBiasAllow = 1 };  // Q3_BIAS_ADD, Q3_BIAS_ALLOW

// the forms of a column plan on the PlanKey::pen axis (q3_batch_host.inc): the classifier's rows as they are, section 2p's penalised
// rows, the adjusted rows of this header with or without penalties on top, or the masked rows of q3_guide.h (section 2r) or of
// q3_guide_sparse.h (section 2s) with or without a table of this header and penalties on top
enum { kPenOff = 0, kPenOn = 1, kPenAdj = 2, kPenGuide = 3, kPenGuideSp = 4, kPenForms = 5 };

struct BiasEntry {                      // q3_bias_entry
    int token;
    float bias;
    unsigned until;
};

// the table of the call in flight as the passes read it
struct BiasCtl {
    const BiasEntry* entries;           // the lists, one behind the other, each sorted by token
    const unsigned* list_off;           // [n_lists + 1]: list i is entries[list_off[i] .. list_off[i + 1])
    const unsigned char* modes;         // [n_lists]
    const int* o_off;                   // [n_requests + 1]: ColsCtl::out of request r's y_0, and the call's n_out behind the last
    unsigned* counts;                   // section 2p's counts [max_streams][n], or null: no penalties (operator entry: [n], read only)
    int n_lists, n_requests;            // n_lists == 1: the one list holds for every request; else list r is request r's
    unsigned g_op;                      // the operator entry's output index
    int pad_;
};

// the first index of e[lo .. hi) whose token is not below `token` (hi where there is none)
__device__ __forceinline__ int bias_lower(const BiasEntry* e, int lo, int hi, int token) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid].token < token) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// a[v] of one entry, on the bits, from the slice's part e[e0 .. e1) of the list
__device__ __forceinline__ unsigned bias_entry(unsigned l_bits, int v, const BiasEntry* e, int e0, int e1, bool allow, unsigned g) {
    const int k = bias_lower(e, e0, e1, v);
    if (k < e1 && e[k].token == v) {
        const float bias = e[k].bias;
        const unsigned until = e[k].until;
        const bool active = until == 0u || g < until;
        if (!active || bias == 0.0f) return l_bits;
        return __float_as_uint(__fadd_rn(__uint_as_float(l_bits), bias));
    }
    return allow ? 0xFF800000u : l_bits;
}

// grid = (kPenSlices, columns), 256 threads; the slices are k_pen_apply's.  a.counts is not read: the counts are BiasCtl's.
__global__ __launch_bounds__(kPenThreads) void k_bias_apply(const PenArgs a, const BiasCtl* __restrict__ bc) {
    __shared__ unsigned long long wbest[kPenThreads / 64];
    const int j = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
    unsigned long long* const slot_out = a.pen_slots + (size_t)j * kPenSlices + s;
    const BiasCtl t = *bc;
    int r = 0, kv = 0;
    unsigned g = t.g_op;
    if (a.cols) {
        if (!pen_emits(a.cols, j)) {
            if (tid == 0) *slot_out = 0ull;
            return;
        }
        // out == o_off[r] + g with 0 <= g < n_new[r]: r is the last request whose offset is not above out
        const int out = a.cols->out[j];
        int lo = 0, hi = t.n_requests;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (t.o_off[mid] <= out) lo = mid;
            else hi = mid;
        }
        r = lo;
        g = (unsigned)max(out - t.o_off[r], 0);
        kv = min(max(a.col_slot[j], 0), a.max_streams - 1);
    }
    const int li = t.n_lists == 1 ? 0 : min(r, t.n_lists - 1);
    const bool allow = t.modes[li] == kBiasAllow;
    const int l0 = (int)t.list_off[li], l1 = (int)t.list_off[li + 1];
    const BiasEntry* const ent = t.entries;
    const bool pen = t.counts != nullptr;
    const bool first = a.cols != nullptr && g == 0u;          // a request's first output: all counts zero by the rule, the slot's cleared here
    const float presence = a.ctl->presence, frequency = a.ctl->frequency;
    const int n = a.n;
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
            const v4u lv = *(const v4u*)(l + 4 * (size_t)u);
            v4u ov = lv;
            if (!plain) {
                ov.x = bias_entry(lv.x, 4 * u, ent, e0, e1, allow, g);
                ov.y = bias_entry(lv.y, 4 * u + 1, ent, e0, e1, allow, g);
                ov.z = bias_entry(lv.z, 4 * u + 2, ent, e0, e1, allow, g);
                ov.w = bias_entry(lv.w, 4 * u + 3, ent, e0, e1, allow, g);
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
            const unsigned lb = __float_as_uint(l[i]);
            unsigned ob = plain ? lb : bias_entry(lb, i, ent, e0, e1, allow, g);
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

// k_pen_count of a plan in the adjusted form: the counts are BiasCtl's, and there are none without penalties
__global__ __launch_bounds__(64) void k_bias_count(PenArgs a, const BiasCtl* __restrict__ bc) {
    a.counts = bc->counts;
    if (!a.counts) return;
    pen_count_column(a, threadIdx.x);
}

}  // namespace q3
