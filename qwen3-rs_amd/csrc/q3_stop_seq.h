// q3_stop_seq.h -- stop sequences: a token automaton beside every slot whose "match" ends the request where a stop token would
// (include/qwen3_hip.h section 2t).
//
// The tables are section 2s's compressed statement (q3_guide_sparse.h): dflt[n_states], row_off[n_states + 1], edges[n_edges] of
// (token, next) with the tokens ascending strictly within a state, start[n_start].  Only the reading of next[s][v] == -1 differs:
// here it means "the sequence is complete, the request ends with this token".
//   stop_seq_next     one state step: one search of the state's edges for the token, else dflt.  __host__ __device__: the kernel, the
//                     host twin q3_cols_schedule_stop_seq and q3_op_stop_seq all call this one function.
//   stop_seq_slot     the automaton phase of one slot between two passes: nothing where the slot did not emit in the pass just
//                     committed (sched_slot_emitted, q3_stop.h: the scheduler step decides with the same helper), else the step from
//                     the request's start state on its first output or from the slot's stored state; returns the "sequence complete"
//                     flag cols_sched_step takes.
//   k_cols_sched_seq  k_cols_sched with that phase in front of the step: thread i < max_streams steps slot i -- the searches of the
//                     slots run in parallel lanes, log2(E_s) dependent loads each -- a barrier, then thread 0 runs cols_sched_step
//                     with the flags.  One workgroup, one launch per pass, in k_cols_sched's place.
// The per-slot states live in StopSeqDev, a struct of its own beside ColsStopDev: ColsSched, ColsStopDev and k_cols_sched are what
// they were.  Only clamped values become addresses: states to [-1, n_states), edge indices to the state's range inside [0, n_edges],
// the token to [0, vocab), the request to [0, n_start).
#pragma once
#include "q3_guide_sparse.h"

namespace q3 {

constexpr int kStopSeqMaxStates = 1 << 16;      // Q3_STOP_SEQ_MAX_STATES
constexpr int kStopSeqMaxEdges = 1 << 24;       // Q3_STOP_SEQ_MAX_EDGES

// the stop automaton as the step reads it: device pointers in StopSeqDev, host pointers in the host twin and q3_op_stop_seq
struct StopSeqCtl {
    const int* dflt;                    // [n_states]
    const unsigned* row_off;            // [n_states + 1]
    const GuideEdge* edges;             // [n_edges]
    const int* start;                   // [n_start]
    int n_states, n_start;              // n_start == 1: the one start state holds for every request; else start[r] is request r's
    int n_edges, vocab;
};

// what the stop loop keeps in device memory under a stop automaton, beside ColsStopDev
struct StopSeqDev {
    StopSeqCtl ctl;
    int state[kColsMax];                // per slot: the state of the request it holds, -1 none; written by k_cols_sched_seq
};

__host__ __device__ inline int stop_seq_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// guide_sp_range, host-callable: the edges of state s (in [0, n_states)) as a range inside [0, n_edges]
__host__ __device__ inline void stop_seq_range(const StopSeqCtl& c, int s, int& lo, int& hi) {
    const unsigned ne = (unsigned)c.n_edges, a = c.row_off[s], b = c.row_off[s + 1];
    lo = (int)(a < ne ? a : ne);
    const unsigned b1 = b > (unsigned)lo ? b : (unsigned)lo;
    hi = (int)(b1 < ne ? b1 : ne);
}

// next[state][token]: -1 the sequence is complete, else the state behind the token
__host__ __device__ inline int stop_seq_next(const StopSeqCtl& c, int state, int token) {
    const int s = stop_seq_clamp(state, 0, c.n_states - 1), v = stop_seq_clamp(token, 0, c.vocab - 1);
    int lo, hi;
    stop_seq_range(c, s, lo, hi);
    const int k = guide_sp_lower(c.edges, lo, hi, v);
    int nx = c.dflt[s];
    if (k < hi) {
        const GuideEdge ge = c.edges[k];
        if (ge.token == v) nx = ge.next;
    }
    return nx < 0 ? -1 : (nx < c.n_states ? nx : c.n_states - 1);
}

// Slot t between two passes, `token` what it produced in the pass just committed: 1 where that token completes a sequence.
// *state: the slot's stored state, read from the second output on and written whenever the slot emitted.
__host__ __device__ inline int stop_seq_slot(const StopSeqCtl& c, const SchedSlot& t, int* state, int token) {
    if (!sched_slot_emitted(t)) return 0;
    // a prompt run that reached its last token produced y_0: the request starts in its own start state, whatever the slot held
    int s = t.took > 0 ? c.start[c.n_start == 1 ? 0 : stop_seq_clamp(t.req, 0, c.n_start - 1)] : *state;
    s = s < 0 ? -1 : (s < c.n_states ? s : c.n_states - 1);
    int done = 0;
    if (s >= 0) {
        s = stop_seq_next(c, s, token);
        done = s < 0 ? 1 : 0;
    }
    *state = s;
    return done;
}

// k_cols_sched under a stop automaton (q3_stop.h states what is staged and written back): the automaton phase stands between the
// staging and the step.
__global__ __launch_bounds__(64) void k_cols_sched_seq(ColsStopDev* d, ColsCtl* ctl, StopSeqDev* q, int draw) {
    static_assert(sizeof(ColsSched) % 4 == 0 && sizeof(ColEnt) == 16 && sizeof(ColAux) == 16, "copied as words");
    static_assert(kMaxStreams <= kColsMax && kColsMax <= 64, "a thread per slot");
    __shared__ ColsSched s;
    __shared__ ColEnt row[kColsMax];
    __shared__ ColAux aux[kColsMax];
    __shared__ int last[kColsMax];
    __shared__ int done[kColsMax];
    const int t = threadIdx.x;
    constexpr int nw = (int)(sizeof(ColsSched) / 4);
    int* sw = reinterpret_cast<int*>(&s);
    int* gw = reinterpret_cast<int*>(&d->sched);
    for (int i = t; i < nw; i += 64) sw[i] = gw[i];
    if (t < kColsMax) {
        last[t] = ctl->slot_last[t];
        done[t] = 0;
    }
    __syncthreads();
    if (t < kColsMax && t < s.max_streams) done[t] = stop_seq_slot(q->ctl, s.slot[t], &q->state[t], last[t]);
    __syncthreads();
    if (t == 0) cols_sched_step(s, last, row, draw ? aux : nullptr, done);
    __syncthreads();
    for (int i = t; i < nw; i += 64) gw[i] = sw[i];
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
