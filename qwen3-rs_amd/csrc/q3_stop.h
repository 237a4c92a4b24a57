// q3_stop.h -- the scheduler of every loop over column passes (include/qwen3_hip.h sections 2e to 2i), and the device side of the
// stop-token loop (section 2h).
//
// cols_sched_step is the one statement of the header's five rules: it applies them to a state that lives next to the table, once
// per pass, and writes the pass as one row of the table.  Where every request's n_new is known in advance (sections 2e / 2f / 2g
// and section 2i without stop tokens) the host steps it with an empty stop list before the first launch and uploads the rows as
// one table (cols_generate); q3_cols_schedule and q3_cols_schedule_stop step it on the host too, which is how the CPU tests reach
// it.  A request that ends at a stop token is a request whose n_new is not known in advance, so there the table is made one pass
// at a time, behind the pass whose tokens decide it: the same function runs in k_cols_sched on the device (one thread, between
// two passes).  Under a stop automaton (section 2t) k_cols_sched_seq of q3_stop_seq.h stands in its place: the slots' automata step
// in parallel lanes first, and the step takes their "sequence complete" flags as its last argument.
#pragma once

namespace q3 {

constexpr int kStopMax = 8;             // Q3_STOP_MAX

struct SchedSlot {
    int req;                            // request held, -1: free
    int fed, g;                         // prompt tokens through a pass / tokens produced
    int took;                           // columns in the pass laid out last: -1 one decode column, k > 0 a prompt run of k, 0 none
    int plen, nnew, poff, ooff;         // the request's records, copied when it is admitted: the passes in between read no request array
};
struct SchedStatus { int n_live, done; };   // live columns of the pass laid out (0 with done = 1: no request queued or held)
struct ColsSched {
    SchedSlot slot[kColsMax];
    int max_streams, n_requests;
    int next;                           // queue head: the next request to admit
    int n_stop;
    int stop[kStopMax];
    int pos_base;                       // added to every column's position: the rows in front of it hold a shared prefix (section 2i)
    int pad_;
    const int* p_off;                   // per request: offset of the prompt in ColsCtl::prompts
    const int* prompt_len;
    const int* n_new;
    const int* o_off;                   // per request: offset of y_0 in ColsCtl::out_tokens
    int* n_out;                         // per request: tokens produced, written when the request ends
    q3_cols_stats stats;                // of the passes laid out so far
    SchedStatus status;
};

// Whether slot t produced a token in the pass laid out last (rule 4): a decode column, or a prompt run that reaches the prompt's
// last token.  Asked before the step has taken the pass into fed and g; the step and the automaton phase of the stop sequences
// (q3_stop_seq.h) both ask here, so they cannot disagree.
__host__ __device__ inline bool sched_slot_emitted(const SchedSlot& t) {
    return t.req >= 0 && (t.took < 0 || (t.took > 0 && t.fed + t.took == t.plen));
}

// One step: rules 4 and 5 for the pass just committed (slot_last[i] = the token slot i produced in it), then rules 1 to 3 for the
// next pass, written as one row of kColsMax entries -- pads as cols_job_run makes them -- and, where aux is not null, the
// ColAux row of the sampled plans.  With n_stop == 0 the values of slot_last decide nothing.  No arrays of its own: the per-slot
// record of the pass in flight is SchedSlot::took.  seq_done: null, or per slot whether the token it produced completes a stop
// sequence (section 2t; read where the slot emitted).
__host__ __device__ inline void cols_sched_step(ColsSched& s, const int* slot_last, ColEnt* row, ColAux* aux, const int* seq_done) {
    const int ms = s.max_streams;
    // 4. a run that reached its prompt's last token produced y_0; 5. a request ends at n_new tokens, at a stop token or where a
    // stop sequence is complete
    for (int i = 0; i < ms; ++i) {
        SchedSlot& t = s.slot[i];
        if (t.req < 0) continue;
        const bool kept = sched_slot_emitted(t);
        if (t.took < 0) {
            ++t.g;
        } else if (t.took > 0) {
            t.fed += t.took;
            if (kept) t.g = 1;
        }
        t.took = 0;
        if (!kept) continue;
        bool end = t.g == t.nnew || (seq_done && seq_done[i] != 0);
        const int tok = slot_last[i];
        for (int k = 0; k < s.n_stop; ++k) end = end || tok == s.stop[k];
        if (end) {
            s.n_out[t.req] = t.g;
            t.req = -1;
        }
    }
    // 1. admit: the next request, in ascending index, takes the lowest free slot
    int held = 0;
    for (int i = 0; i < ms; ++i) {
        SchedSlot& t = s.slot[i];
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
    int cols = 0;
    // 2. one column per decode-phase slot
    for (int i = 0; i < ms; ++i) {
        SchedSlot& t = s.slot[i];
        if (t.req < 0 || t.fed != t.plen) continue;
        row[cols] = ColEnt{i, s.pos_base + t.fed + t.g - 1, -1, t.ooff + t.g};
        if (aux) aux[cols] = ColAux{-1, 0, 1, 1};
        t.took = -1;
        ++cols;
        ++s.stats.decode_columns;
    }
    // 3. prompt-phase slots share what is left of the pass
    for (int i = 0; i < ms && cols < kColsMax; ++i) {
        SchedSlot& t = s.slot[i];
        if (t.req < 0 || t.took < 0) continue;
        const int pl = t.plen, left = pl - t.fed;
        const int n = left < kColsMax - cols ? left : kColsMax - cols;
        for (int k = 0; k < n; ++k) {
            const int pos = t.fed + k;
            const int out = pos + 1 == pl ? t.ooff : -1;       // the run's last column emits y_0
            row[cols] = ColEnt{i, s.pos_base + pos, t.poff + pos, out};
            if (aux) aux[cols] = ColAux{pos == 0 ? t.req : -1, k, out >= 0 ? 1 : 0, k == n - 1 ? 1 : 0};
            ++cols;
        }
        t.took = n;
        s.stats.prompt_columns += (uint64_t)n;
    }
    if (cols == 0) {                    // cannot happen: a held request always gets a column (the header's note to rule 5).  The host
        s.status = SchedStatus{0, 0};   // loop answers a pass of no columns with Q3_ERR_INTERNAL
        return;
    }
    // pads repeat the pass's last live column and emit nothing
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

// What the stop loop keeps in device memory besides the buffers of sections 2e / 2f: the scheduler state, the one-row table the
// turn kernels read and the status word the host waits for.
struct ColsStopDev {
    ColsSched sched;
    ColEnt row[kColsMax];
    ColAux aux[kColsMax];
    int ncols;
    int pad_;
    SchedStatus status;
};

// Between two passes, behind the turn kernel that committed the last one (it found cursor == n_passes and set nothing up): the
// scheduler state and ColsCtl::slot_last are staged in LDS, one thread runs the step there, and the state, the row and (draw)
// the ColAux row go back to device memory.  The row is a table of one pass -- cursor 0 of 1, nothing to commit -- and a launch of
// the turn kernel behind this one sets the pass up, as for pass 0 of the kept loops.  done: n_passes = 0, that launch sets
// nothing up.  One workgroup.
__global__ __launch_bounds__(64) void k_cols_sched(ColsStopDev* d, ColsCtl* ctl, int draw) {
    static_assert(sizeof(ColsSched) % 4 == 0 && sizeof(ColEnt) == 16 && sizeof(ColAux) == 16, "copied as words");
    __shared__ ColsSched s;
    __shared__ ColEnt row[kColsMax];
    __shared__ ColAux aux[kColsMax];
    __shared__ int last[kColsMax];
    const int t = threadIdx.x;
    constexpr int nw = (int)(sizeof(ColsSched) / 4);
    int* sw = reinterpret_cast<int*>(&s);
    int* gw = reinterpret_cast<int*>(&d->sched);
    for (int i = t; i < nw; i += 64) sw[i] = gw[i];
    if (t < kColsMax) last[t] = ctl->slot_last[t];
    __syncthreads();
    if (t == 0) cols_sched_step(s, last, row, draw ? aux : nullptr, nullptr);
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
