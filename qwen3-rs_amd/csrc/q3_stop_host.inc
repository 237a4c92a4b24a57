// q3_stop_host.inc -- host side of the stop-token loop (include/qwen3_hip.h section 2h; included by q3_engine.hip behind
// q3_cols_host.inc, same translation unit).
//
// The loops of sections 2e / 2f know every pass before the first one runs.  Here a pass depends on the tokens of the pass before
// it: k_cols_sched (q3_stop.h) lays it out on the device, the kept plans and their turn kernels run it unchanged from a table of
// one row, and the host learns one thing per pass -- how many live columns it has, which picks the plan width -- from an 8-byte
// status word.  That is one synchronisation per pass.

namespace {

int stop_list_check(const int32_t* stop_tokens, size_t n_stop) {
    if (n_stop > (size_t)Q3_STOP_MAX) return fail(Q3_ERR_ARG, "%zu stop tokens, at most %d", n_stop, Q3_STOP_MAX);
    if (n_stop > 0 && !stop_tokens) return fail(Q3_ERR_ARG, "null stop_tokens with n_stop %zu", n_stop);
    return Q3_OK;
}

// The stop automaton of q3_stop_seq_set on the device (q3_stop_seq.h, section 2t), on the stream in front of a call's first pass:
// the control block with the slots' states, made once and cleared to -1 then -- a later call finds the states its predecessor left,
// and a request's first output never reads them; the three arrays where the device does not hold this automaton yet -- once per
// q3_stop_seq_set and per batched state, never per call; start[] and the control block with every call.
int stop_seq_call_begin(q3_engine* e) {
    BatchCtx* b = e->batch;
    const GuideSparse& t = e->stop_seq;
    int rc;
    if (!b->stop_seq_dev) {
        DevMem<StopSeqDev> dev;
        if ((rc = dev.alloc(1))) return rc;
        HIP_TRY(hipMemsetAsync(dev, 0xff, sizeof(StopSeqDev), e->stream));
        b->stop_seq_dev = std::move(dev);
    }
    if (b->stop_seq_serial != t.serial) {
        b->stop_seq_serial = 0;
        if ((rc = b->stop_seq_dflt.grow(t.dflt.size(), e->stream)) || (rc = b->stop_seq_off.grow(t.row_off.size(), e->stream)) ||
            (rc = b->stop_seq_edges.grow(std::max(t.edges.size(), (size_t)1), e->stream)))
            return rc;
        HIP_TRY(hipMemcpyAsync(b->stop_seq_dflt, t.dflt.data(), sizeof(int) * t.dflt.size(), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(b->stop_seq_off, t.row_off.data(), sizeof(uint32_t) * t.row_off.size(), hipMemcpyHostToDevice, e->stream));
        if (!t.edges.empty())
            HIP_TRY(hipMemcpyAsync(b->stop_seq_edges, t.edges.data(), sizeof(GuideEdge) * t.edges.size(), hipMemcpyHostToDevice, e->stream));
        b->stop_seq_serial = t.serial;
    }
    if ((rc = b->stop_seq_start.grow(t.start.size(), e->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(b->stop_seq_start, t.start.data(), sizeof(int) * t.start.size(), hipMemcpyHostToDevice, e->stream));
    StopSeqCtl h{};
    h.dflt = b->stop_seq_dflt;
    h.row_off = b->stop_seq_off;
    h.edges = b->stop_seq_edges;
    h.start = b->stop_seq_start;
    h.n_states = (int)t.n_states;
    h.n_start = (int)t.start.size();
    h.n_edges = (int)t.edges.size();
    h.vocab = (int)t.vocab;
    StopSeqDev* dev = b->stop_seq_dev;
    HIP_TRY(hipMemcpyAsync(&dev->ctl, &h, sizeof(StopSeqCtl), hipMemcpyHostToDevice, e->stream));
    return Q3_OK;
}

// rq: checked by cols_requests_check, with the prefix in front of the prompts as its pos_base
int cols_generate_stop(q3_engine* e, const ColsRequests& rq, const int32_t* stop_tokens, size_t n_stop, int32_t* out_tokens, size_t* n_out,
                       q3_cols_stats* stats) {
    int rc;
    const bool draw = rq.draw();
    const size_t n_requests = rq.size();
    BatchCtx* b = e->batch;
    if (!n_out) return fail(Q3_ERR_ARG, "null argument");
    if ((rc = stop_list_check(stop_tokens, n_stop))) return rc;
    for (size_t k = 0; k < n_stop; ++k)
        if (stop_tokens[k] < 0 || stop_tokens[k] >= e->cfg.vocab_size)
            return fail(Q3_ERR_ARG, "index out of range: stop token %d (vocab_size %d)", stop_tokens[k], e->cfg.vocab_size);

    if (draw && (rc = cols_draw_alloc(e))) return rc;
    const int lp = e->gen_logprobs;                         // >= 0: the passes run the plans with records (section 2o)
    if (lp >= 0 && (rc = genlp_alloc(e))) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));              // nothing in flight reads the buffers that may be re-allocated
    if (!b->cols_stop && (rc = b->cols_stop.alloc(1))) return rc;
    if (!b->h_cols_stop && (rc = b->h_cols_stop.alloc(1))) return rc;
    if ((rc = b->cols_req.grow(5 * n_requests, e->stream))) return rc;
    if ((rc = b->cols_prompts.grow(rq.n_prompt, e->stream))) return rc;
    if ((rc = b->cols_out.grow(rq.n_out, e->stream))) return rc;
    if (lp >= 0 && (rc = genlp_call_begin(e, lp, rq.n_out))) return rc;
    const int pen = e->pen_form();
    if (pen == kPenAdj && (rc = bias_call_begin(e, rq.o_off.data(), n_requests, rq.n_out))) return rc;     // the call's table (section 2q)
    if (pen == kPenGuide && (rc = guide_call_begin(e, rq.o_off.data(), n_requests, rq.n_out))) return rc;  // the call's guide and table (section 2r)
    if (pen == kPenGuideSp && (rc = guide_sp_call_begin(e, rq.o_off.data(), n_requests, rq.n_out))) return rc;  // ... in its sparse form (section 2s)
    const bool seq = e->stop_seq.n_states != 0;            // a stop automaton holds (section 2t): k_cols_sched_seq stands for k_cols_sched
    if (seq && (rc = stop_seq_call_begin(e))) return rc;

    // uploaded once: the prompts, the per-request records, the sampler parameters, the scheduler state with the stop list
    int* dreq = b->cols_req;
    HIP_TRY(hipMemcpyAsync(b->cols_prompts, rq.prompts, 4 * rq.n_prompt, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(dreq + 0 * n_requests, rq.p_off.data(), 4 * n_requests, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(dreq + 1 * n_requests, rq.prompt_len.data(), 4 * n_requests, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(dreq + 2 * n_requests, rq.n_new.data(), 4 * n_requests, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(dreq + 3 * n_requests, rq.o_off.data(), 4 * n_requests, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(dreq + 4 * n_requests, 0, 4 * n_requests, e->stream));
    HIP_TRY(hipMemsetAsync(b->cols_out, 0xFF, 4 * rq.n_out, e->stream));          // -1 behind every request's last token
    ColsStopDev* d = b->cols_stop;
    ColsSched sched;
    cols_sched_init(sched, b->max_streams, rq, stop_tokens, n_stop, dreq + 4 * n_requests);
    sched.p_off = dreq;                                    // the records as the device holds them
    sched.prompt_len = dreq + n_requests;
    sched.n_new = dreq + 2 * n_requests;
    sched.o_off = dreq + 3 * n_requests;
    HIP_TRY(hipMemsetAsync(d, 0, sizeof(ColsStopDev), e->stream));
    HIP_TRY(hipMemcpyAsync(&d->sched, &sched, sizeof(ColsSched), hipMemcpyHostToDevice, e->stream));
    if (draw && (rc = cols_sampler_upload(e, b->cols_slot_samp, d->aux, rq.temperature, rq.topp, rq.seeds, n_requests))) return rc;
    // the control block of the turn kernels: a table of one row, empty until k_cols_sched fills it
    ColsHost* h = b->h_cols;
    memset(&h->ctl, 0, sizeof(ColsCtl));
    h->ctl.table = d->row;
    h->ctl.ncols = &d->ncols;
    h->ctl.prompts = b->cols_prompts;
    h->ctl.out_tokens = b->cols_out;
    HIP_TRY(hipMemcpyAsync(b->cols_ctl, &h->ctl, sizeof(ColsCtl), hipMemcpyHostToDevice, e->stream));
    // the shared prefix in front of every request: rows 0 .. pos_base - 1 of the slots the scheduler can use
    if (rq.pos_base && (rc = prefix_bcast_slots(e, (int)std::min<size_t>(n_requests, (size_t)b->max_streams)))) return rc;

    // every pass advances at least one column of a request that has prompt_len + n_new - 1 of them at the most: a scheduler that
    // asks for more passes than that is wrong, and the call ends with an error code
    const size_t pass_cap = rq.n_prompt + rq.n_out;
    SchedStatus* hs = b->h_cols_stop;
    size_t passes = 0;
    for (;;) {
        if (seq) rc = launch_now(e->stream, k_cols_sched_seq, dim3(1), dim3(64), 0, d, b->cols_ctl, (StopSeqDev*)b->stop_seq_dev, draw ? 1 : 0);
        else rc = launch_now(e->stream, k_cols_sched, dim3(1), dim3(64), 0, d, b->cols_ctl, draw ? 1 : 0);
        if (rc) return rc;
        // the pass is set up by a launch of its own, like pass 0 of the kept loops (n_live is 0: nothing to commit)
        if ((rc = cols_turn_setup(e, draw))) return rc;
        HIP_TRY(hipMemcpyAsync(hs, &d->status, sizeof(SchedStatus), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (hs->done) break;
        if (hs->n_live < 1 || hs->n_live > kColsMax) return fail(Q3_ERR_INTERNAL, "the scheduler laid out a pass of %d columns", hs->n_live);
        if (++passes > pass_cap) return fail(Q3_ERR_INTERNAL, "the scheduler asks for more than %zu passes", pass_cap);
        Plan* plan;                                        // built on first use of a width: the stream is idle here
        if ((rc = plan_get(e, cols_key(hs->n_live, draw, lp, pen), &plan))) return rc;
        if ((rc = plan_enqueue(e, *plan))) return rc;      // ends with the turn kernel: cursor == n_passes, it commits and sets nothing up
    }
    std::vector<int> got(n_requests);
    q3_cols_stats st;
    HIP_TRY(hipMemcpyAsync(out_tokens, b->cols_out, 4 * rq.n_out, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(got.data(), dreq + 4 * n_requests, 4 * n_requests, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(&st, &d->sched.stats, sizeof(q3_cols_stats), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (st.passes != passes) return fail(Q3_ERR_INTERNAL, "the scheduler counted %llu passes, the host ran %zu", (unsigned long long)st.passes, passes);
    for (size_t r = 0; r < n_requests; ++r) n_out[r] = (size_t)got[r];
    if (stats) *stats = st;
    if (lp >= 0) genlp_call_end(e, lp, rq.n_out);
    return Q3_OK;
}

}  // namespace

extern "C" {

int q3_generate_many_stop(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, const size_t* n_new, size_t n_requests,
                          const float* temperature, const float* topp, const uint64_t* seeds, const int32_t* stop_tokens, size_t n_stop,
                          int32_t* out_tokens, size_t* n_out, q3_cols_stats* stats) {
    g_err[0] = 0;
    genlp_call_enter(e);
    if (stats) *stats = q3_cols_stats{0, 0, 0, 0};
    int rc;
    ColsRequests rq;
    const bool draw = temperature || topp || seeds;
    if ((rc = cols_prepare(e, "q3_generate_many_stop", draw))) return rc;
    if ((rc = cols_requests_check(e, prompts, prompt_len, n_new, n_requests, draw, temperature, topp, seeds, 0, out_tokens, rq))) return rc;
    return cols_generate_stop(e, rq, stop_tokens, n_stop, out_tokens, n_out, stats);
}

int q3_cols_schedule_stop(const size_t* prompt_len, const size_t* n_new, size_t n_requests, int max_streams, const int32_t* rows,
                          const int32_t* stop_tokens, size_t n_stop, int32_t* table, size_t cap, size_t* n_entries, size_t* n_out,
                          q3_cols_stats* stats) {
    g_err[0] = 0;
    int rc;
    if (!rows) return fail(Q3_ERR_ARG, "null rows");
    if ((rc = stop_list_check(stop_tokens, n_stop))) return rc;
    return cols_schedule_table(prompt_len, n_new, n_requests, max_streams, rows, stop_tokens, n_stop, table, cap, n_entries, n_out, stats);
}

/* ---- section 2t: the host twin of the loop under a stop automaton, and one token stream over the tables ---- */

int q3_cols_schedule_stop_seq(const size_t* prompt_len, const size_t* n_new, size_t n_requests, int max_streams, const int32_t* rows,
                              const int32_t* stop_tokens, size_t n_stop, const int32_t* dflt, const uint32_t* row_off, const q3_guide_edge* edges,
                              size_t n_states, size_t n_edges, size_t vocab, const int32_t* start, size_t n_start, int32_t* table, size_t cap,
                              size_t* n_entries, size_t* n_out, q3_cols_stats* stats) {
    g_err[0] = 0;
    int rc;
    if (!rows) return fail(Q3_ERR_ARG, "null rows");
    if ((rc = stop_list_check(stop_tokens, n_stop))) return rc;
    if ((rc = stop_seq_check(dflt, row_off, edges, n_states, n_edges, vocab, start, n_start))) return rc;
    static_assert(sizeof(GuideEdge) == sizeof(q3_guide_edge), "one layout");
    const StopSeqCtl c{dflt, row_off, reinterpret_cast<const GuideEdge*>(edges), start, (int)n_states, (int)n_start, (int)n_edges, (int)vocab};
    return cols_schedule_table(prompt_len, n_new, n_requests, max_streams, rows, stop_tokens, n_stop, table, cap, n_entries, n_out, stats,
                               n_states ? &c : nullptr);
}

int q3_op_stop_seq(const int32_t* dflt, const uint32_t* row_off, const q3_guide_edge* edges, size_t n_states, size_t n_edges, size_t vocab,
                   int32_t start_state, const int32_t* tokens, size_t n_tokens, size_t* n_emit, int32_t* end_state) {
    g_err[0] = 0;
    int rc;
    if ((rc = stop_seq_check(dflt, row_off, edges, n_states, n_edges, vocab, &start_state, 1))) return rc;
    if (n_states == 0) return fail(Q3_ERR_ARG, "a stop automaton of no states");
    if (!tokens && n_tokens) return fail(Q3_ERR_ARG, "null tokens with %zu tokens", n_tokens);
    if (!n_emit || !end_state) return fail(Q3_ERR_ARG, "null argument");
    const StopSeqCtl c{dflt, row_off, reinterpret_cast<const GuideEdge*>(edges), &start_state, (int)n_states, 1, (int)n_edges, (int)vocab};
    int s = start_state;
    size_t g = 0;
    for (; s >= 0 && g < n_tokens; ++g) s = stop_seq_next(c, s, tokens[g]);
    // a match ends the walk behind the completing token; start -1 steps nothing
    *n_emit = start_state < 0 ? n_tokens : g;
    *end_state = s;
    return Q3_OK;
}

}  // extern "C"
