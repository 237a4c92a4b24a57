// q3_lookup_host.inc -- host side of prompt-lookup drafts in the stop loop (include/qwen3_hip.h sections 2u and 2w; included by
// q3_engine.hip behind q3_stop_host.inc, same translation unit).
//
// The loop is cols_generate_stop's: it takes a LookupArgs and calls the three hooks below where the lookup loop differs -- room for
// the drafts behind the prompts and the lookup state at the start of the call, k_lookup_draft and k_cols_sched_lookup
// (q3_lookup_dev.h) where k_cols_sched stands, the counts at its end.  Status read-back, plan lookup, pass cap and error checks are
// that loop's own.

namespace {

// in front of the first pass, on the stream: the lookup state, cleared, with the call's arguments
int lookup_call_begin(q3_engine* e, const LookupArgs& a, size_t n_prompt) {
    BatchCtx* b = e->batch;
    int rc;
    if (!b->lookup_dev && (rc = b->lookup_dev.alloc(1))) return rc;
    LookupDev h;
    memset(&h, 0, sizeof h);
    h.ngram = a.ngram;
    h.draft_len = a.draft_len;
    h.fill_width = a.fill_width;
    h.ctx = b->ctx;
    h.draft_src0 = (int)n_prompt;
    HIP_TRY(hipMemcpyAsync(b->lookup_dev, &h, sizeof h, hipMemcpyHostToDevice, e->stream));     // pageable: the copy is staged before the call returns
    return Q3_OK;
}

// between two passes: accept and draft per slot, then the step.  draw (section 2w; cols_draw_alloc has run): the walk reads the column
// sampler states the pass's draws left and commits the slots' rng, the step writes the ColAux row of the next pass
int lookup_sched_launch(q3_engine* e, size_t n_prompt, bool draw) {
    BatchCtx* b = e->batch;
    ColsStopDev* d = b->cols_stop;
    int rc;
    if ((rc = launch_now(e->stream, k_lookup_draft, dim3(b->max_streams), dim3(kLookupThreads), 0, (const ColsStopDev*)d, (ColsCtl*)b->cols_ctl,
                         (LookupDev*)b->lookup_dev, (int*)(b->cols_prompts + n_prompt), draw ? (const ColsDraw*)b->cols_draw : nullptr,
                         draw ? (const SamplerState*)b->draw_cols.ss : nullptr)))
        return rc;
    return launch_now(e->stream, k_cols_sched_lookup, dim3(1), dim3(64), 0, d, (ColsCtl*)b->cols_ctl, (LookupDev*)b->lookup_dev, draw ? 1 : 0);
}

// behind the last pass: the counts (the caller synchronises)
int lookup_call_end(q3_engine* e, q3_lookup_stats* out) {
    HIP_TRY(hipMemcpyAsync(out, &e->batch->lookup_dev->stats, sizeof(q3_lookup_stats), hipMemcpyDeviceToHost, e->stream));
    return Q3_OK;
}

// what both entry points refuse about their draft arguments, and about the engine's settings (sections 2u and 2w)
int lookup_args_check(int ngram, int draft_len, int fill_width) {
    if (ngram < 1) return fail(Q3_ERR_ARG, "ngram %d must be >= 1", ngram);
    if (draft_len < 1 || draft_len > kLookupDraftMax) return fail(Q3_ERR_ARG, "draft_len %d out of range (1..%d)", draft_len, kLookupDraftMax);
    if (fill_width != 0 && (fill_width < 1 || fill_width > kColsMax || (fill_width & (fill_width - 1))))
        return fail(Q3_ERR_ARG, "fill_width %d is not 0 or a pass width (1, 2, 4, 8, 16, 32)", fill_width);
    return Q3_OK;
}
int lookup_refusals(q3_engine* e, const char* who) {
    static const char* const kPenNames[] = {"", "q3_sampler_penalties", "q3_logit_bias_set", "q3_guide_set", "q3_guide_set_sparse"};
    static_assert(kPenOff == 0 && kPenOn == 1 && kPenAdj == 2 && kPenGuide == 3 && kPenGuideSp == 4, "kPenNames is indexed by the form");
    const char* name = nullptr;
    if (e->pen_form() != kPenOff) name = kPenNames[e->pen_form()];
    else if (e->gen_logprobs >= 0) name = "q3_gen_logprobs";
    else if (e->stop_seq.n_states) name = "q3_stop_seq_set";
    else if (e->batch->prefix_n) name = "q3_batch_prefix_set";
    if (name) return fail(Q3_ERR_UNSUPPORTED, "%s does not draft under %s: clear it, or call q3_generate_many_stop", who, name);
    return Q3_OK;
}

}  // namespace

extern "C" {

int q3_generate_many_lookup_draw(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, const size_t* n_new, size_t n_requests,
                                 const float* temperature, const float* topp, const uint64_t* seeds, const int32_t* stop_tokens, size_t n_stop,
                                 int ngram, int draft_len, int fill_width, int32_t* out_tokens, size_t* n_out, q3_cols_stats* stats,
                                 q3_lookup_stats* lookup_stats) {
    g_err[0] = 0;
    genlp_call_enter(e);
    if (stats) *stats = q3_cols_stats{0, 0, 0, 0};
    if (lookup_stats) *lookup_stats = q3_lookup_stats{0, 0};
    int rc;
    if ((rc = lookup_args_check(ngram, draft_len, fill_width))) return rc;          // in front of the engine: no device is touched
    if ((rc = cols_prepare(e, "q3_generate_many_lookup_draw", true))) return rc;
    if ((rc = lookup_refusals(e, "q3_generate_many_lookup_draw"))) return rc;
    ColsRequests rq;
    if ((rc = cols_requests_check(e, prompts, prompt_len, n_new, n_requests, true, temperature, topp, seeds, 0, out_tokens, rq))) return rc;
    if (rq.n_prompt > (size_t)INT32_MAX - (size_t)kColsMax * kLookupDraftMax) return fail(Q3_ERR_ARG, "more than 2^31 tokens in one call");
    q3_lookup_stats ls{0, 0};
    const LookupArgs a{ngram, draft_len, fill_width, &ls};
    if ((rc = cols_generate_stop(e, rq, stop_tokens, n_stop, out_tokens, n_out, stats, &a))) return rc;
    if (lookup_stats) *lookup_stats = ls;
    return Q3_OK;
}

int q3_batch_slot_rng(q3_engine* e, int slot, uint64_t* rng_state) {
    g_err[0] = 0;
    if (!e || !rng_state) return fail(Q3_ERR_ARG, "null argument");
    if (!e->batch || !e->batch->cols_slot_samp) return fail(Q3_ERR_ARG, "no sampled q3_generate_many_* loop has run on this batched state");
    if (slot < 0 || slot >= e->batch->max_streams) return fail(Q3_ERR_ARG, "slot %d out of range (0..%d)", slot, e->batch->max_streams - 1);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    SamplerState h;
    HIP_TRY(hipMemcpy(&h, e->batch->cols_slot_samp + slot, sizeof(h), hipMemcpyDeviceToHost));
    *rng_state = h.rng;
    return Q3_OK;
}

int q3_generate_many_lookup(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, const size_t* n_new, size_t n_requests,
                            const int32_t* stop_tokens, size_t n_stop, int ngram, int draft_len, int fill_width, int32_t* out_tokens, size_t* n_out,
                            q3_cols_stats* stats, q3_lookup_stats* lookup_stats) {
    g_err[0] = 0;
    genlp_call_enter(e);
    if (stats) *stats = q3_cols_stats{0, 0, 0, 0};
    if (lookup_stats) *lookup_stats = q3_lookup_stats{0, 0};
    int rc;
    if ((rc = cols_prepare(e, "q3_generate_many_lookup"))) return rc;
    if ((rc = lookup_args_check(ngram, draft_len, fill_width))) return rc;
    if ((rc = lookup_refusals(e, "q3_generate_many_lookup"))) return rc;             // greedy and plain only
    ColsRequests rq;
    if ((rc = cols_requests_check(e, prompts, prompt_len, n_new, n_requests, false, nullptr, nullptr, nullptr, 0, out_tokens, rq))) return rc;
    if (rq.n_prompt > (size_t)INT32_MAX - (size_t)kColsMax * kLookupDraftMax) return fail(Q3_ERR_ARG, "more than 2^31 tokens in one call");
    q3_lookup_stats ls{0, 0};
    const LookupArgs a{ngram, draft_len, fill_width, &ls};
    if ((rc = cols_generate_stop(e, rq, stop_tokens, n_stop, out_tokens, n_out, stats, &a))) return rc;
    if (lookup_stats) *lookup_stats = ls;
    return Q3_OK;
}

int q3_op_lookup_draft(const int32_t* seq, size_t n, int ngram, int draft_len, int32_t* draft_out, int32_t* len_out, int device) {
    int rc = op_begin(device);
    if (rc) return rc;
    if ((!seq && n) || !draft_out || !len_out) return fail(Q3_ERR_ARG, "null argument");
    if (n > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 tokens");
    if (ngram < 1) return fail(Q3_ERR_ARG, "ngram %d must be >= 1", ngram);
    if (draft_len < 1 || draft_len > kLookupDraftMax) return fail(Q3_ERR_ARG, "draft_len %d out of range (1..%d)", draft_len, kLookupDraftMax);
    OpBuf dseq, ddraft, dlen;
    if ((rc = dseq.upload(seq, 4 * n)) || (rc = ddraft.alloc(4 * (size_t)kLookupDraftMax)) || (rc = dlen.alloc(4))) return rc;
    if ((rc = launch_now(0, k_op_lookup_draft, dim3(1), dim3(kLookupThreads), 0, (const int*)dseq.as<int>(), (int)n, ngram, draft_len, ddraft.as<int>(),
                         dlen.as<int>())) ||
        (rc = op_end()))
        return rc;
    int32_t len = 0;
    HIP_TRY(hipMemcpy(&len, dlen.p, 4, hipMemcpyDeviceToHost));
    if (len > 0) HIP_TRY(hipMemcpy(draft_out, ddraft.p, 4 * (size_t)len, hipMemcpyDeviceToHost));
    *len_out = len;
    return Q3_OK;
}

}  // extern "C"
