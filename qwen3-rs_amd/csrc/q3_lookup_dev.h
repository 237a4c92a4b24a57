// q3_lookup_dev.h -- prompt-lookup drafts inside the stop loop (include/qwen3_hip.h section 2u): the drafter of q3_lookup.h on the
// device, the accept walk over a slot's run, and the scheduler step that hands a pass's spare columns to decode-phase slots.
//
// Between two passes of q3_generate_many_lookup two kernels stand where k_cols_sched stands alone:
//   k_lookup_draft       one workgroup per KV slot.  Thread 0 first walks the slot's run of the pass just committed (lookup_accept):
//                        the drafts that equal the argmax in front of them become output tokens.  Then the workgroup searches the
//                        slot's sequence S -- the request's prompt and the tokens it has produced, read where they lie in
//                        ColsCtl::prompts and ColsCtl::out_tokens -- for the draft of the NEXT pass and leaves it in the scratch
//                        tail behind the call's prompts, where k_cols_turn reads any prompt token.
//   k_cols_sched_lookup  one workgroup, one thread steps cols_sched_step_lookup: rules 4 and 5 with g moved by the tokens the walk
//                        committed, rules 1 to 3 as cols_sched_step states them, and rule 6 -- the columns between the pass's base
//                        columns and its plan width go to decode-phase slots, in slot order, as draft columns.
// The accept walk runs in the drafter's workgroups and not in the step: the draft of the next pass continues the sequence WITH the
// tokens just accepted, so the walk has to come first, and per slot it is independent work.
// The search (lookup_find): candidate starts are walked from the end of S in chunks of kLookupChunk; a chunk's tokens are staged in
// LDS once (plus the overlap of a window that begins in it), thread t tests starts hi - 1 - t, hi - 1 - t - 256, ... against the
// suffix, last token of the window first, and stops at its first -- largest -- match; a butterfly over the wave's lanes and one LDS
// word per wave give the workgroup's largest match, and the first chunk that holds one ends the search.  LDS holds the last
// kLookupGram tokens of every window; where ngram is longer the tokens in front are compared from device memory, only for the
// starts that passed in LDS.  No floating point arithmetic anywhere in this file.
//
// Under the sampler (section 2w) the same two kernels run next to the sampled plans' ColsDraw.  The step also writes the ColAux
// row: column j of a decode-phase slot's run -- its decode column and the drafts behind it -- is drawn with the slot's rng advanced
// j coins, keep set, last clear, so the plan's draw launches draw every column of the run, a workgroup each, and the turn kernel
// leaves the slot's rng alone.  ColsCtl::next then holds the DRAWN token of every column (the argmax for a temperature-0 slot), the
// walk reads it as it reads the argmaxes, and commits the slot's rng itself: the state the last standing column left behind its
// coin, 1 + standing drafts coins past the slot's state.  The coins of rejected columns are not spent.
#pragma once

namespace q3 {

constexpr int kLookupDraftMax = 31;     // Q3_LOOKUP_DRAFT_MAX: a run is the decode column and at most 31 drafts
constexpr int kLookupThreads = 256;
constexpr int kLookupChunk = 4096;      // candidate starts per staged chunk (Q3_LOOKUP_CHUNK)
constexpr int kLookupGram = 32;         // tokens of a window compared in LDS

// S = a[0 .. na) ++ b[0 .. n - na)
struct LookupSeq {
    const int* a;
    const int* b;
    int na, n;
};
__device__ __forceinline__ int lookup_tok(const LookupSeq& s, int j) { return j < s.na ? s.a[j] : s.b[j - s.na]; }

// The largest i < n - g with S[i .. i + g) == S[n - g .. n), or -1; the same value in every thread.  Every thread of the workgroup
// calls it with the same arguments.
__device__ inline int lookup_find(const LookupSeq& s, int g) {
    __shared__ int stage[kLookupChunk + kLookupGram - 1];
    __shared__ int suf[kLookupGram];
    __shared__ int wave_best[kLookupThreads / 64];
    const int t = threadIdx.x, n = s.n;
    if (n <= g) return -1;
    const int gl = g < kLookupGram ? g : kLookupGram;       // the window's last gl tokens are compared in LDS,
    const int head = g - gl;                                // the head tokens in front of them in device memory
    if (t < gl) suf[t] = lookup_tok(s, n - gl + t);
    for (int hi = n - g; hi > 0; hi -= kLookupChunk) {      // starts [lo, hi)
        const int lo = hi > kLookupChunk ? hi - kLookupChunk : 0;
        const int m = hi - lo + gl - 1;                     // staged: S[lo + head .. lo + head + m), which ends at or before S[n - 2]
        __syncthreads();
        for (int j = t; j < m; j += kLookupThreads) stage[j] = lookup_tok(s, lo + head + j);
        __syncthreads();
        int best = -1;
        for (int i = hi - 1 - t; i >= lo; i -= kLookupThreads) {
            const int* w = stage + (i - lo);
            int k = gl - 1;
            while (k >= 0 && w[k] == suf[k]) --k;
            if (k >= 0) continue;
            int h = 0;
            while (h < head && lookup_tok(s, i + h) == lookup_tok(s, n - g + h)) ++h;
            if (h == head) {
                best = i;
                break;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const int other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        if ((t & 63) == 0) wave_best[t >> 6] = best;
        __syncthreads();
        for (int w = 0; w < kLookupThreads / 64; ++w) best = wave_best[w] > best ? wave_best[w] : best;
        if (best >= 0) return best;
    }
    return -1;
}

// The draft over S, at most cap tokens, to draft[0 ..); returns its length (the same value in every thread)
__device__ inline int lookup_draft_dev(const LookupSeq& s, int g, int cap, int* draft) {
    const int i = lookup_find(s, g);
    if (i < 0) return 0;
    int len = s.n - (i + g);
    if (len > cap) len = cap;
    if ((int)threadIdx.x < len) draft[threadIdx.x] = lookup_tok(s, i + g + (int)threadIdx.x);
    return len;
}

// q3_op_lookup_draft: the drafter over one sequence.  One workgroup.
__global__ __launch_bounds__(kLookupThreads) void k_op_lookup_draft(const int* seq, int n, int g, int cap, int* draft, int* len) {
    const LookupSeq s{seq, seq, n, n};
    const int l = lookup_draft_dev(s, g, cap, draft);
    if (threadIdx.x == 0) *len = l;
}

// What the loop keeps per KV slot besides SchedSlot, and its arguments
struct LookupSlot {
    int col0;                           // the pass in flight: index of the slot's decode column in the row,
    int nd;                             // and the draft columns behind it
    int committed;                      // tokens the pass just committed produced for the slot: 1 + accepted drafts (0: no decode column)
    int dlen;                           // length of the draft in the scratch tail, cut to what the request and the context leave room for
};
struct LookupDev {
    LookupSlot slot[kColsMax];
    int ngram, draft_len, fill_width, ctx;
    int draft_src0;                     // index of the scratch tail in ColsCtl::prompts: slot i's draft k is prompts[draft_src0 + i * 31 + k]
    int pad_;
    q3_lookup_stats stats;
};

// The accept walk of one decode-phase slot over the pass just committed.  The turn kernel has stored the decode column's own token,
// next[col0], at out[t.g] and in *last.  Draft k stands while it equals the argmax of the column in front of it; the argmax behind an
// accepted draft is the next output token.  The walk ends at a stop token and at nnew.  Returns the tokens committed, 1 at least.
__host__ __device__ inline int lookup_accept(const SchedSlot& t, const LookupSlot& ls, const int* stop, int n_stop, const int* next, const int* draft,
                                             int* out, int* last) {
    int n = 1, y = next[ls.col0];
    for (int k = 0; k < ls.nd; ++k) {
        bool end = t.g + n >= t.nnew;
        for (int j = 0; j < n_stop; ++j) end = end || y == stop[j];
        if (end || draft[k] != next[ls.col0 + k]) break;
        y = next[ls.col0 + 1 + k];
        out[t.g + n] = y;
        ++n;
    }
    *last = y;
    return n;
}

// One workgroup per KV slot, between two passes: the accept walk, then the draft of the next pass.  tail: the scratch behind the
// call's prompts.  dr: null, or the loop draws (section 2w): cs[j] is the sampler state of column j behind its coin, and the walk
// commits the rng of a slot that draws -- a temperature-0 slot spends no coin, as in the plain loop.
__global__ __launch_bounds__(kLookupThreads) void k_lookup_draft(const ColsStopDev* d, ColsCtl* ctl, LookupDev* lk, int* tail, const ColsDraw* dr,
                                                                 const SamplerState* cs) {
    __shared__ int sh_g;
    const int i = blockIdx.x;
    const SchedSlot t = d->sched.slot[i];
    int* draft = tail + i * kLookupDraftMax;
    if (threadIdx.x == 0) {
        const LookupSlot ls = lk->slot[i];
        int g = 0, committed = 0;                           // g: tokens produced once the walk is done; 0: no decode column next pass
        if (t.req >= 0 && t.took < 0) {
            committed = lookup_accept(t, ls, d->sched.stop, d->sched.n_stop, ctl->next, draft, ctl->out_tokens + t.ooff, &ctl->slot_last[i]);
            g = t.g + committed;
            if (dr != nullptr) {
                SamplerState* ss = dr->slot_ss + i;
                if (ss->temperature != 0.0f) ss->rng = cs[ls.col0 + committed - 1].rng;
            }
        } else if (sched_slot_emitted(t)) {
            g = 1;                                          // a prompt run that produced y_0
        }
        lk->slot[i].committed = committed;
        sh_g = g;
    }
    __syncthreads();                                        // the tokens the walk stored are part of S
    const int g = sh_g;
    int cap = lk->draft_len;
    if (cap > t.nnew - g - 1) cap = t.nnew - g - 1;         // the decode column produces token g, draft k verifies token g + 1 + k
    if (cap > lk->ctx - (t.plen + g)) cap = lk->ctx - (t.plen + g);
    int len = 0;
    if (g > 0 && cap > 0) {
        const LookupSeq s{ctl->prompts + t.poff, ctl->out_tokens + t.ooff, t.plen, t.plen + g};
        len = lookup_draft_dev(s, lk->ngram, cap, draft);
    }
    if (threadIdx.x == 0) lk->slot[i].dlen = len;
}

// cols_sched_step (q3_stop.h) with drafts.  Rules 4 and 5 read the walk's count where the slot had a decode column; rules 1 to 3 lay
// out the same base columns; rule 6 puts up to max(plan width of the base columns, fill_width) - base columns draft columns directly
// behind the decode columns of their slots, in slot order, at most dlen each.  Draft columns emit nothing.  aux: null, or the ColAux
// row of the sampled plans: prompt runs as cols_sched_step writes them, the columns of a decode-phase slot's run by their index in
// the run, every one drawn, none last (k_lookup_draft commits that slot's rng).
__host__ __device__ inline void cols_sched_step_lookup(ColsSched& s, LookupDev& lk, const int* slot_last, ColEnt* row, ColAux* aux) {
    const int ms = s.max_streams;
    for (int i = 0; i < ms; ++i) {
        SchedSlot& t = s.slot[i];
        LookupSlot& ls = lk.slot[i];
        if (t.req < 0) continue;
        const bool kept = sched_slot_emitted(t);
        if (t.took < 0) {
            t.g += ls.committed;
            lk.stats.drafted += (uint64_t)ls.nd;
            lk.stats.accepted += (uint64_t)(ls.committed - 1);
        } else if (t.took > 0) {
            t.fed += t.took;
            if (kept) t.g = 1;
        }
        t.took = 0;
        ls.nd = 0;
        if (!kept) continue;
        bool end = t.g == t.nnew;
        const int tok = slot_last[i];
        for (int k = 0; k < s.n_stop; ++k) end = end || tok == s.stop[k];
        if (end) {
            s.n_out[t.req] = t.g;
            t.req = -1;
        }
    }
    // 1. admit
    int held = 0;
    for (int i = 0; i < ms; ++i) {
        SchedSlot& t = s.slot[i];
        if (t.req < 0) lk.slot[i].dlen = 0;                 // a draft belongs to the request it was made for
        if (t.req < 0 && s.next < s.n_requests) {
            const int r = s.next++;
            t = SchedSlot{r, 0, 0, 0, s.prompt_len[r], s.n_new[r], s.p_off[r], s.o_off[r]};
        }
        if (t.req >= 0) ++held;
    }
    if (held == 0) {
        s.status = SchedStatus{0, 1};
        return;
    }
    // the base columns of rules 2 and 3, counted: a prompt run's length goes to took as in cols_sched_step
    int base = 0;
    for (int i = 0; i < ms; ++i)
        if (s.slot[i].req >= 0 && s.slot[i].fed == s.slot[i].plen) {
            s.slot[i].took = -1;
            ++base;
        }
    for (int i = 0; i < ms && base < kColsMax; ++i) {
        SchedSlot& t = s.slot[i];
        if (t.req < 0 || t.took < 0) continue;
        const int left = t.plen - t.fed;
        t.took = left < kColsMax - base ? left : kColsMax - base;
        base += t.took;
    }
    if (base == 0) {
        s.status = SchedStatus{0, 0};
        return;
    }
    int width = 1;
    while (width < base) width *= 2;                        // the plan widths are the powers of two up to kColsMax
    int spare = (width > lk.fill_width ? width : lk.fill_width) - base;
    int cols = 0;
    // 2. one column per decode-phase slot, 6. its drafts behind it
    for (int i = 0; i < ms; ++i) {
        SchedSlot& t = s.slot[i];
        if (t.req < 0 || t.took >= 0) continue;
        LookupSlot& ls = lk.slot[i];
        const int pos = s.pos_base + t.fed + t.g - 1;
        row[cols] = ColEnt{i, pos, -1, t.ooff + t.g};
        if (aux) aux[cols] = ColAux{-1, 0, 1, 0};
        ls.col0 = cols++;
        ls.nd = ls.dlen < spare ? ls.dlen : spare;
        spare -= ls.nd;
        for (int k = 0; k < ls.nd; ++k) {
            row[cols] = ColEnt{i, pos + 1 + k, lk.draft_src0 + i * kLookupDraftMax + k, -1};
            if (aux) aux[cols] = ColAux{-1, 1 + k, 1, 0};
            ++cols;
        }
        ++s.stats.decode_columns;
    }
    // 3. prompt-phase slots
    for (int i = 0; i < ms; ++i) {
        SchedSlot& t = s.slot[i];
        if (t.req < 0 || t.took <= 0) continue;
        for (int k = 0; k < t.took; ++k) {
            const int pos = t.fed + k;
            const int out = pos + 1 == t.plen ? t.ooff : -1;
            row[cols] = ColEnt{i, s.pos_base + pos, t.poff + pos, out};
            if (aux) aux[cols] = ColAux{pos == 0 ? t.req : -1, k, out >= 0 ? 1 : 0, k == t.took - 1 ? 1 : 0};
            ++cols;
        }
        s.stats.prompt_columns += (uint64_t)t.took;
    }
    ColEnt pad = row[cols - 1];
    pad.out = -1;
    for (int j = cols; j < kColsMax; ++j) {
        row[j] = pad;
        if (aux) aux[j] = ColAux{-1, aux[cols - 1].k, 0, 0};
    }
    s.stats.live_columns += (uint64_t)cols;
    ++s.stats.passes;
    s.status = SchedStatus{cols, 0};
}

// k_cols_sched with the step above: the scheduler state, the lookup state and ColsCtl::slot_last are staged in LDS, one thread
// steps, and the states, the row and (draw) the ColAux row go back.  One workgroup, behind k_lookup_draft.
__global__ __launch_bounds__(64) void k_cols_sched_lookup(ColsStopDev* d, ColsCtl* ctl, LookupDev* lk, int draw) {
    static_assert(sizeof(ColsSched) % 4 == 0 && sizeof(LookupDev) % 4 == 0 && sizeof(ColEnt) == 16 && sizeof(ColAux) == 16, "copied as words");
    __shared__ ColsSched s;
    __shared__ LookupDev l;
    __shared__ ColEnt row[kColsMax];
    __shared__ ColAux aux[kColsMax];
    __shared__ int last[kColsMax];
    const int t = threadIdx.x;
    constexpr int nw = (int)(sizeof(ColsSched) / 4), nl = (int)(sizeof(LookupDev) / 4);
    int* sw = reinterpret_cast<int*>(&s);
    int* gw = reinterpret_cast<int*>(&d->sched);
    int* lw = reinterpret_cast<int*>(&l);
    int* glw = reinterpret_cast<int*>(lk);
    for (int i = t; i < nw; i += 64) sw[i] = gw[i];
    for (int i = t; i < nl; i += 64) lw[i] = glw[i];
    if (t < kColsMax) last[t] = ctl->slot_last[t];
    __syncthreads();
    if (t == 0) cols_sched_step_lookup(s, l, last, row, draw ? aux : nullptr);
    __syncthreads();
    for (int i = t; i < nw; i += 64) gw[i] = sw[i];
    for (int i = t; i < nl; i += 64) glw[i] = lw[i];
    const SchedStatus st = s.status;
    if (t < kColsMax && st.n_live > 0) {
        d->row[t] = row[t];
        if (draw) d->aux[t] = aux[t];
    }
    if (t == 0) {
        d->ncols = st.n_live;
        ctl->cursor = 0;
        ctl->n_passes = st.done || st.n_live == 0 ? 0 : 1;
        ctl->n_live = 0;
        d->status = st;
    }
}

}  // namespace q3
