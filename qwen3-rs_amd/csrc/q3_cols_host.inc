// q3_cols_host.inc -- host side of the column passes (include/qwen3_hip.h sections 2e and 2f; included by q3_engine.hip behind
// q3_batch_host.inc, same translation unit).
//
// A pass is up to 32 columns of (slot, token, position) over the per-stream KV caches of the batched state: decode columns of some
// slots next to runs of consecutive prompt positions of others, one pass over the packed weights (PlanKind::Cols).  The loop
// q3_generate_many_greedy walks a pass table that is a pure function of the request lengths (cols_sched_step of q3_stop.h, stepped
// here on the host): the host knows every pass's width in advance, the device resolves every pass's tokens itself (k_cols_turn).
// Section 2f is the same under the sampler: a second set of plans whose classifier is followed by the per-column draws and
// k_cols_turn_draw (q3_sampler.h), the greedy plans and their launches untouched.
// Section 2o is a third axis on both: under q3_gen_logprobs the loops run plans whose turn kernel is preceded by the record launches
// of q3_score.h / q3_score_top.h over the pass in flight (q3_genlp.h), and the call's records, tops and ranks stay in the batched state for q3_gen_logprobs_read.

namespace {

// q3_prefix_host.inc: one launch on the stream that copies the resident prefix into rows 0 .. P - 1 of slots 0 .. n_slots - 1
int prefix_bcast_slots(q3_engine* e, int n_slots);

int cols_schedule_check(const size_t* prompt_len, const size_t* n_new, size_t n_requests, int max_streams) {
    if (!prompt_len || !n_new || n_requests == 0) return fail(Q3_ERR_ARG, "null or empty request list");
    if (max_streams < 1 || max_streams > kMaxStreams) return fail(Q3_ERR_ARG, "max_streams %d out of range (1..%d)", max_streams, kMaxStreams);
    for (size_t r = 0; r < n_requests; ++r)
        if (prompt_len[r] == 0 || n_new[r] == 0) return fail(Q3_ERR_ARG, "request %zu: empty prompt or n_new 0", r);
    return Q3_OK;
}

// The checked requests of a call: the per-request records of the scheduler (q3_stop.h keeps them as int) and, for the loops, the
// arrays they index.  draw: the three sampler arrays, all given.
struct ColsRequests {
    std::vector<int> p_off, prompt_len, n_new, o_off;
    size_t n_prompt = 0, n_out = 0;
    const int32_t* prompts = nullptr;
    size_t pos_base = 0;
    const float *temperature = nullptr, *topp = nullptr;
    const uint64_t* seeds = nullptr;
    size_t size() const { return prompt_len.size(); }
    bool draw() const { return temperature != nullptr; }
};

// the lengths alone: what q3_cols_schedule and q3_cols_schedule_stop check
int cols_requests_lengths(const size_t* prompt_len, const size_t* n_new, size_t n_requests, int max_streams, ColsRequests& rq) {
    int rc;
    if ((rc = cols_schedule_check(prompt_len, n_new, n_requests, max_streams))) return rc;
    rq.p_off.resize(n_requests);
    rq.prompt_len.resize(n_requests);
    rq.n_new.resize(n_requests);
    rq.o_off.resize(n_requests);
    for (size_t r = 0; r < n_requests; ++r) {
        if (prompt_len[r] > (size_t)INT32_MAX || n_new[r] > (size_t)INT32_MAX || rq.n_prompt + prompt_len[r] > (size_t)INT32_MAX ||
            rq.n_out + n_new[r] > (size_t)INT32_MAX)
            return fail(Q3_ERR_ARG, "more than 2^31 tokens in one call");
        rq.p_off[r] = (int)rq.n_prompt;
        rq.o_off[r] = (int)rq.n_out;
        rq.prompt_len[r] = (int)prompt_len[r];
        rq.n_new[r] = (int)n_new[r];
        rq.n_prompt += prompt_len[r];
        rq.n_out += n_new[r];
    }
    return Q3_OK;
}

// everything the five q3_generate_many_* entry points refuse about their requests (cols_prepare has run).  draw: the call is a
// sampled one, which needs all three sampler arrays.  pos_base: the rows in front of every prompt (section 2i)
int cols_requests_check(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, const size_t* n_new, size_t n_requests, bool draw,
                        const float* temperature, const float* topp, const uint64_t* seeds, size_t pos_base, const int32_t* out_tokens, ColsRequests& rq) {
    int rc;
    const BatchCtx* b = e->batch;
    if (!prompts || !out_tokens || (draw && (!temperature || !topp || !seeds))) return fail(Q3_ERR_ARG, "null argument");
    if ((rc = cols_requests_lengths(prompt_len, n_new, n_requests, b->max_streams, rq))) return rc;
    for (size_t r = 0; r < n_requests; ++r)
        if (pos_base + prompt_len[r] + n_new[r] - 1 > (size_t)b->ctx)
            return fail(Q3_ERR_ARG, "request %zu: prompt of %zu + %zu new tokens exceeds seq_len %d", r, pos_base + prompt_len[r], n_new[r], b->ctx);
    for (size_t i = 0; i < rq.n_prompt; ++i)
        if (prompts[i] < 0 || prompts[i] >= e->cfg.vocab_size)
            return fail(Q3_ERR_ARG, "index out of range: token %d (vocab_size %d)", prompts[i], e->cfg.vocab_size);
    if (n_requests > (size_t)INT32_MAX / 5) return fail(Q3_ERR_ARG, "more than 2^31 / 5 requests in one call");
    if (e->bias.n_lists() > 1 && e->bias.n_lists() != n_requests)
        return fail(Q3_ERR_ARG, "q3_logit_bias_set holds %zu lists, one per request, and the call has %zu requests", e->bias.n_lists(), n_requests);
    if (e->guide.n_states && e->guide.start.size() > 1 && e->guide.start.size() != n_requests)
        return fail(Q3_ERR_ARG, "q3_guide_set holds %zu start states, one per request, and the call has %zu requests", e->guide.start.size(), n_requests);
    if (e->guide_sp.n_states && e->guide_sp.start.size() > 1 && e->guide_sp.start.size() != n_requests)
        return fail(Q3_ERR_ARG, "q3_guide_set_sparse holds %zu start states, one per request, and the call has %zu requests", e->guide_sp.start.size(), n_requests);
    if (e->stop_seq.n_states && e->stop_seq.start.size() > 1 && e->stop_seq.start.size() != n_requests)
        return fail(Q3_ERR_ARG, "q3_stop_seq_set holds %zu start states, one per request, and the call has %zu requests", e->stop_seq.start.size(), n_requests);
    for (size_t r = 0; draw && r < n_requests; ++r)
        if ((rc = sampler_check(temperature[r], topp[r], (long)r))) return rc;
    rq.prompts = prompts;
    rq.pos_base = pos_base;
    rq.temperature = temperature;
    rq.topp = topp;
    rq.seeds = seeds;
    return Q3_OK;
}

// a scheduler state over the records of rq, nothing admitted yet.  n_out: per request, written when the request ends
void cols_sched_init(ColsSched& s, int max_streams, const ColsRequests& rq, const int32_t* stop_tokens, size_t n_stop, int* n_out) {
    memset(&s, 0, sizeof(ColsSched));
    for (int i = 0; i < kColsMax; ++i) s.slot[i] = SchedSlot{-1, 0, 0, 0, 0, 0, 0, 0};
    s.max_streams = max_streams;
    s.n_requests = (int)rq.size();
    s.n_stop = (int)n_stop;
    for (size_t k = 0; k < n_stop; ++k) s.stop[k] = stop_tokens[k];
    s.pos_base = (int)rq.pos_base;
    s.p_off = rq.p_off.data();
    s.prompt_len = rq.prompt_len.data();
    s.n_new = rq.n_new.data();
    s.o_off = rq.o_off.data();
    s.n_out = n_out;
}

// The schedule on the host: cols_sched_step (q3_stop.h) pass after pass until no request is queued or held.  on_pass(pass, row,
// aux, slot_last) sees every pass as the step wrote it and may set slot_last[i], the token slot i produced in it (zero unless set:
// with an empty stop list no value of it is looked at).  Every pass advances at least one column of a request that has
// prompt_len + n_new - 1 of them at the most: a scheduler that asks for more passes than that is wrong.
// seq: null, or the stop automaton of section 2t over host arrays: the automaton phase of k_cols_sched_seq (stop_seq_slot,
// q3_stop_seq.h) runs in front of every step, over slot states kept here
template <class OnPass>
int cols_sched_walk(ColsSched& s, const ColsRequests& rq, OnPass&& on_pass, const StopSeqCtl* seq = nullptr) {
    const size_t pass_cap = rq.n_prompt + rq.n_out;
    ColEnt row[kColsMax];
    ColAux aux[kColsMax];
    int slot_last[kColsMax] = {0};
    int seq_state[kColsMax], seq_done[kColsMax] = {0};
    for (int i = 0; i < kColsMax; ++i) seq_state[i] = -1;
    for (size_t pass = 0;; ++pass) {
        for (int i = 0; seq && i < s.max_streams; ++i) seq_done[i] = stop_seq_slot(*seq, s.slot[i], &seq_state[i], slot_last[i]);
        cols_sched_step(s, slot_last, row, aux, seq ? seq_done : nullptr);
        if (s.status.done) return Q3_OK;
        if (s.status.n_live < 1) return fail(Q3_ERR_INTERNAL, "the scheduler laid out a pass of %d columns", s.status.n_live);
        if (pass >= pass_cap) return fail(Q3_ERR_INTERNAL, "the scheduler asks for more than %zu passes", pass_cap);
        on_pass(pass, row, aux, slot_last);
    }
}

// q3_cols_schedule (rows == nullptr, no stop list) and q3_cols_schedule_stop: the table of the walk above
int cols_schedule_table(const size_t* prompt_len, const size_t* n_new, size_t n_requests, int max_streams, const int32_t* rows,
                        const int32_t* stop_tokens, size_t n_stop, int32_t* table, size_t cap, size_t* n_entries, size_t* n_out, q3_cols_stats* stats,
                        const StopSeqCtl* seq = nullptr) {
    int rc;
    ColsRequests rq;
    if ((rc = cols_requests_lengths(prompt_len, n_new, n_requests, max_streams, rq))) return rc;
    if (seq && seq->n_start != 1 && (size_t)seq->n_start != n_requests)
        return fail(Q3_ERR_ARG, "the stop automaton holds %d start states, one per request, and the schedule has %zu requests", seq->n_start, n_requests);
    std::vector<int> got(n_requests, 0);
    ColsSched s;
    cols_sched_init(s, max_streams, rq, stop_tokens, n_stop, got.data());
    size_t n = 0;
    if ((rc = cols_sched_walk(s, rq, [&](size_t pass, const ColEnt* row, const ColAux*, int* slot_last) {
            for (int j = 0; j < s.status.n_live; ++j) {
                const ColEnt& c = row[j];
                if (table && n < cap) {
                    table[4 * n + 0] = (int32_t)pass;
                    table[4 * n + 1] = c.slot;
                    table[4 * n + 2] = c.pos;
                    table[4 * n + 3] = s.slot[c.slot].req;
                }
                ++n;
                if (rows && c.out >= 0) slot_last[c.slot] = rows[c.out];       // what the turn kernel commits: the token this column produces
            }
        }, seq)))
        return rc;
    if (n_entries) *n_entries = n;
    if (n_out)
        for (size_t r = 0; r < n_requests; ++r) n_out[r] = (size_t)got[r];
    if (stats) *stats = s.stats;
    if (table && n > cap) return fail(Q3_ERR_ARG, "the schedule has %zu entries, the table holds %zu", n, cap);
    return Q3_OK;
}

// what every entry point of section 2e refuses.  draw: the names of section 2f, which hold for any batch sampler
int cols_prepare(q3_engine* e, const char* who, bool draw = false) {
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    if (!e->batch || !e->batch->has_kv) return fail(Q3_ERR_ARG, "q3_batch_init has not been called");
    if (e->flags & Q3_FLAG_FAST)
        return fail(Q3_ERR_UNSUPPORTED, "%s needs a reference-order engine: with Q3_FLAG_FAST the block kernels and the decode kernels are not bit-equal", who);
    if (e->batch->sampling && !draw)
        return fail(Q3_ERR_UNSUPPORTED, "%s is greedy only: the batch sampler is set to a temperature > 0", who);
    return Q3_OK;
}

// the key of the column plan a pass of n live columns runs: the narrowest width that holds it.  draw: the sampled plan of that
// width (cols_draw_alloc has run by the time it is built: its launches carry the buffers allocated there).
// lp: the q3_gen_logprobs value a q3_generate_many_* loop runs under (-1 off, 0 records, > 0 records and top): the plan's third axis.
// pen: kPenOn, the loop runs under a non-zero q3_sampler_penalties (section 2p); kPenAdj, under a table of q3_logit_bias_set (section
// 2q), with or without penalties: the plan's fourth axis (q3_engine::pen_form).
// Every other caller keeps the plans without records and without penalties.
PlanKey cols_key(int n, bool draw, int lp = -1, int pen = kPenOff) {
    return PlanKey{PlanKind::Cols, kColsWidths[cols_width_index(n)], draw, false, lp < 0 ? kGenlpOff : (lp == 0 ? kGenlpRecs : kGenlpTop), pen};
}

// What the plans with records carry of section 2o's own, on first use: the control block and its pinned copy (the scratch of the
// record launches is record_args', q3_plan_host.inc).  One group, committed whole.  Freed with the context.
int genlp_alloc(q3_engine* e) {
    BatchCtx* b = e->batch;
    int rc;
    if (b->genlp_ctl) return Q3_OK;
    HIP_TRY(hipSetDevice(e->device));
    DevMem<GenlpCtl> ctl; PinMem<GenlpCtl> h;
    if ((rc = ctl.alloc(1)) || (rc = h.alloc(1))) return rc;
    HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(GenlpCtl), e->stream));
    b->genlp_ctl = std::move(ctl); b->h_genlp = std::move(h);
    return Q3_OK;
}

// The per-call side of the records, behind the call's synchronisation and in front of its first pass: room for n_out records (and
// tops and ranks with lp > 0), cleared on the stream -- a request that ends early leaves zero bytes behind its last token -- and the
// control block.  The pinned copy is free: the call before ended with a synchronisation.
int genlp_call_begin(q3_engine* e, int lp, size_t n_out) {
    int rc;
    BatchCtx* b = e->batch;
    const size_t k = (size_t)lp;
    if ((rc = b->genlp_recs.grow(n_out, e->stream))) return rc;
    if (lp > 0 && ((rc = b->genlp_top.grow(n_out * k, e->stream)) || (rc = b->genlp_rank.grow(n_out, e->stream)))) return rc;
    if (n_out) {
        HIP_TRY(hipMemsetAsync(b->genlp_recs, 0, sizeof(ScoreRec) * n_out, e->stream));
        if (lp > 0) {
            HIP_TRY(hipMemsetAsync(b->genlp_top, 0, sizeof(ScoreTop) * n_out * k, e->stream));
            HIP_TRY(hipMemsetAsync(b->genlp_rank, 0, sizeof(int) * n_out, e->stream));
        }
    }
    GenlpCtl* h = b->h_genlp;
    *h = GenlpCtl{b->genlp_recs, lp > 0 ? (ScoreTop*)b->genlp_top : nullptr, lp > 0 ? (int*)b->genlp_rank : nullptr, lp, 0};
    HIP_TRY(hipMemcpyAsync(b->genlp_ctl, h, sizeof(GenlpCtl), hipMemcpyHostToDevice, e->stream));
    return Q3_OK;
}
// the call has succeeded: its records are what q3_gen_logprobs_read hands out
void genlp_call_end(q3_engine* e, int lp, size_t n_out) {
    BatchCtx* b = e->batch;
    b->genlp_count = n_out;
    b->genlp_top_n = lp;
    b->genlp_valid = true;
}
// every q3_generate_many_* call starts here: the records of the call before are gone
void genlp_call_enter(q3_engine* e) {
    if (e && e->batch) e->batch->genlp_valid = false;
}

// The buffers of the sampled passes, on first use: the column sampler states and the draw scratch of the verify pass
// (spec_draw_alloc, 32 columns wide whatever max_streams is), the control block of k_cols_turn_draw, the one-pass table of a
// host-made pass and the loop's per-slot sampler states.  Freed with the context.
int cols_draw_alloc(q3_engine* e) {
    BatchCtx* b = e->batch;
    int rc;
    if (!b->draw_cols && (rc = spec_draw_alloc(e))) return rc;
    if (b->h_cols_draw) return Q3_OK;
    HIP_TRY(hipSetDevice(e->device));
    // one group, committed whole (DrawSite::alloc)
    DevMem<ColsDraw> draw; DevMem<ColsStep> step; DevMem<SamplerState> slot_samp; PinMem<ColsDrawHost> h_draw;
    if ((rc = draw.alloc(1)) || (rc = step.alloc(1)) || (rc = slot_samp.alloc(kMaxStreams)) || (rc = h_draw.alloc(1))) return rc;
    HIP_TRY(hipMemsetAsync(draw, 0, sizeof(ColsDraw), e->stream));
    HIP_TRY(hipMemsetAsync(slot_samp, 0, sizeof(SamplerState) * kMaxStreams, e->stream));
    b->cols_draw = std::move(draw); b->cols_step = std::move(step); b->cols_slot_samp = std::move(slot_samp); b->h_cols_draw = std::move(h_draw);
    return Q3_OK;
}

// The sampler side of a loop's passes, on the stream: the per-request parameters (temperature null: none, no request is loaded from
// them) and the control block of k_cols_turn_draw over the per-slot states slot_ss and the ColAux table aux.
int cols_sampler_upload(q3_engine* e, SamplerState* slot_ss, const ColAux* aux, const float* temperature, const float* topp, const uint64_t* seeds,
                        size_t n_requests) {
    int rc;
    BatchCtx* b = e->batch;
    if (temperature) {
        if ((rc = b->cols_temp.grow(n_requests, e->stream))) return rc;
        if ((rc = b->cols_topp.grow(n_requests, e->stream))) return rc;
        if ((rc = b->cols_seeds.grow(n_requests, e->stream))) return rc;
        HIP_TRY(hipMemcpyAsync(b->cols_temp, temperature, 4 * n_requests, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(b->cols_topp, topp, 4 * n_requests, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(b->cols_seeds, seeds, 8 * n_requests, hipMemcpyHostToDevice, e->stream));
    }
    ColsDraw& dr = b->h_cols_draw->dr;
    memset(&dr, 0, sizeof(ColsDraw));
    dr.slot_ss = slot_ss;
    dr.aux = aux;
    dr.temperature = b->cols_temp;
    dr.topp = b->cols_topp;
    dr.seeds = b->cols_seeds;
    HIP_TRY(hipMemcpyAsync(b->cols_draw, &dr, sizeof(ColsDraw), hipMemcpyHostToDevice, e->stream));
    return Q3_OK;
}

// The launch that sets up the pass at the table's cursor with nothing to commit: pass 0 of a table, or the one pass of a table
// of one row.  Every later pass of a table is set up by the turn kernel that ends the pass before it.
int cols_turn_setup(q3_engine* e, bool draw) {
    BatchCtx* b = e->batch;
    if (draw) return launch_now(e->stream, k_cols_turn_draw, dim3(1), dim3(kWG), 0, b->cols_ctl, b->cols_draw, b->draw_cols.ss, b->st, b->col_slot);
    return launch_now(e->stream, k_cols_turn, dim3(1), dim3(kWG), 0, b->cols_ctl, b->slots, b->nslots, 0, b->st, b->col_slot);
}

// One host-made pass.  draw = false: the states and the slot table are written here and the greedy plan commits the argmaxes.
// draw = true: the pass goes through a one-pass table, set up by a k_cols_turn_draw launch in front of the sampled plan -- the
// column sampler states derive from the slot states in device memory (the batch sampler's draw_decode.ss: slot i = stream i).
int cols_step(q3_engine* e, const int32_t* slots, const int32_t* tokens, const int32_t* pos, int n_cols, const uint8_t* keep, float* logits_out,
              int32_t* next_out, bool draw) {
    int rc;
    BatchCtx* b = e->batch;
    if (!slots || !tokens || !pos) return fail(Q3_ERR_ARG, "null argument");
    if (n_cols < 1 || n_cols > kColsMax) return fail(Q3_ERR_ARG, "n_cols %d out of range (1..%d)", n_cols, kColsMax);
    bool seen[kMaxStreams] = {false};
    for (int j = 0; j < n_cols; ++j) {
        if (slots[j] < 0 || slots[j] >= b->max_streams) return fail(Q3_ERR_ARG, "column %d: slot %d out of range (0..%d)", j, slots[j], b->max_streams - 1);
        if (tokens[j] < 0 || tokens[j] >= e->cfg.vocab_size || pos[j] < 0 || pos[j] >= b->ctx)
            return fail(Q3_ERR_ARG, "index out of range: column %d token %d (vocab_size %d), pos %d (seq_len %d)", j, tokens[j], e->cfg.vocab_size,
                        pos[j], b->ctx);
        if (j > 0 && slots[j] == slots[j - 1]) {
            if (pos[j] != pos[j - 1] + 1)
                return fail(Q3_ERR_ARG, "column %d: the positions of a slot's run must be consecutive (%d behind %d)", j, pos[j], pos[j - 1]);
        } else {
            if (seen[slots[j]]) return fail(Q3_ERR_ARG, "column %d: slot %d is in two runs", j, slots[j]);
            seen[slots[j]] = true;
        }
    }
    if (draw && (rc = cols_draw_alloc(e))) return rc;
    Plan* plan;
    if ((rc = plan_get(e, cols_key(n_cols, draw), &plan))) return rc;
    HIP_TRY(hipSetDevice(e->device));
    ColsHost* h = b->h_cols;
    memset(&h->ctl, 0, sizeof(ColsCtl));
    if (draw) {
        ColsDrawHost* hd = b->h_cols_draw;
        h->ctl.n_passes = 1;
        h->ctl.table = b->cols_step->table;
        h->ctl.ncols = &b->cols_step->ncols;
        h->ctl.prompts = b->cols_step->tokens;
        memset(&hd->dr, 0, sizeof(ColsDraw));
        hd->dr.slot_ss = b->draw_decode.ss;
        hd->dr.aux = b->cols_step->aux;
        hd->step.ncols = n_cols;
        for (int j = 0; j < kColsMax; ++j) {
            const int i = j < n_cols ? j : n_cols - 1;       // pads repeat the last live column and neither draw nor commit
            hd->step.table[j] = ColEnt{slots[i], pos[i], i, -1};
            hd->step.tokens[j] = tokens[i];
            ColAux& x = hd->step.aux[j];
            x.req = -1;
            x.k = (i > 0 && slots[i] == slots[i - 1]) ? hd->step.aux[i - 1].k + 1 : 0;
            x.keep = j < n_cols && (!keep || keep[j]) ? 1 : 0;
            x.last = j < n_cols && (j == n_cols - 1 || slots[j + 1] != slots[j]) ? 1 : 0;
        }
        HIP_TRY(hipMemcpyAsync(b->cols_ctl, &h->ctl, sizeof(ColsCtl), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(b->cols_draw, &hd->dr, sizeof(ColsDraw), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(b->cols_step, &hd->step, sizeof(ColsStep), hipMemcpyHostToDevice, e->stream));
        if ((rc = cols_turn_setup(e, true))) return rc;
    } else {
        h->ctl.n_live = n_cols;
        for (int j = 0; j < kColsMax; ++j) {
            const int i = j < n_cols ? j : n_cols - 1;           // pads repeat the last live column: the same bits to the same rows
            h->ctl.out[j] = -1;
            h->st[j].token = tokens[i];
            h->st[j].pos = pos[i];
            h->st[j].step = 0;
            h->st[j].prompt_len = 0;
            h->st[j].argmax = 0ull;
            h->slot[j] = slots[i];
        }
        HIP_TRY(hipMemcpyAsync(b->cols_ctl, &h->ctl, sizeof(ColsCtl), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(b->st, h->st, sizeof(State) * kColsMax, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(b->col_slot, h->slot, 4 * kColsMax, hipMemcpyHostToDevice, e->stream));
    }
    if ((rc = plan_enqueue(e, *plan))) return rc;
    const size_t V = e->cfg.vocab_size;
    if (logits_out) HIP_TRY(hipMemcpyAsync(b->h_logits, b->logits, 4 * V * (size_t)n_cols, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(&h->ctl, b->cols_ctl, sizeof(ColsCtl), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (logits_out) memcpy(logits_out, b->h_logits, 4 * V * (size_t)n_cols);
    if (next_out)
        for (int j = 0; j < n_cols; ++j) next_out[j] = h->ctl.next[j];
    return Q3_OK;
}

// What a call enqueues, in stream order: column passes from a pass table and dense blocks over the slots (q3_dense_host.inc) in
// between.  The table is walked by the turn kernels on the device, one pass per step that is not wide; a wide step is the block
// of n columns over runs [r0, r0 + nr) of the run table.
struct ColsJobStep { bool wide; int n; size_t r0, nr; };
struct ColsJob {
    std::vector<ColEnt> table;          // [passes][kColsMax]
    std::vector<ColAux> aux;            // under the sampler: next to the table
    std::vector<int> ncols;             // live columns of every pass
    std::vector<DenseRun> runs;
    std::vector<ColsJobStep> steps;
    size_t max_end = 0;                 // the largest position + 1 a wide block attends over
    int bcast_slots = 0;                // > 0: the resident prefix goes into the lowest bcast_slots slots in front of the first pass (section 2i)
    // a new pass of the table; returns its index
    size_t add_pass(bool draw) {
        ncols.push_back(0);
        table.resize(table.size() + kColsMax);
        if (draw) aux.resize(table.size());
        steps.push_back(ColsJobStep{false, 0, 0, 0});
        return ncols.size() - 1;
    }
};
struct ColsJobSampler {                 // the sampler side of a job (draw)
    SamplerState* slot_ss;              // per-slot states the passes draw from and commit to
    const float *temperature, *topp;    // per request (loaded where ColAux::req >= 0), or nullptr
    const uint64_t* seeds;
    size_t n_requests;
    bool skip_wide;                     // the wide blocks' runs advance slot_ss of their slots by their lengths (k_dense_rng_skip), ahead of the passes
};

// pads of every pass (they repeat the pass's last live column and emit nothing), then the whole job on the stream: the only
// uploads of the call are the table, the run table, the prompts and the per-request sampler parameters; one synchronisation.
// lp >= 0 (the generate loops under q3_gen_logprobs): the passes run the plans with records, which fill the call's n_out records.
// pen (the generate loops under a non-zero q3_sampler_penalties, or kPenAdj under a table of q3_logit_bias_set, whose bias_call_begin
// has run): the passes run the plans of that form.
int cols_job_run(q3_engine* e, ColsJob& job, bool draw, const ColsJobSampler& smp, const int32_t* prompts, size_t n_prompt, int32_t* out_tokens, size_t n_out,
                 int lp = -1, int pen = kPenOff) {
    int rc;
    BatchCtx* b = e->batch;
    const size_t n_passes = job.ncols.size();
    bool width_used[kColsNW] = {false};
    for (size_t p = 0; p < n_passes; ++p) {
        ColEnt pad = job.table[p * kColsMax + job.ncols[p] - 1];
        pad.out = -1;
        for (int j = job.ncols[p]; j < kColsMax; ++j) job.table[p * kColsMax + j] = pad;
        if (draw)
            for (int j = job.ncols[p]; j < kColsMax; ++j) job.aux[p * kColsMax + j] = ColAux{-1, job.aux[p * kColsMax + job.ncols[p] - 1].k, 0, 0};
        width_used[cols_width_index(job.ncols[p])] = true;
    }
    // every plan and buffer the call needs exists before the first launch is enqueued
    if (draw && n_passes && (rc = cols_draw_alloc(e))) return rc;
    if (lp >= 0 && (rc = genlp_alloc(e))) return rc;
    Plan* plans[kColsNW] = {nullptr};
    for (int w = 0; w < kColsNW; ++w)
        if (width_used[w] && (rc = plan_get(e, cols_key(kColsWidths[w], draw, lp, pen), &plans[w]))) return rc;
    std::vector<Plan*> wide_plans(job.steps.size(), nullptr);
    if (!job.runs.empty()) {
        if ((rc = dense_scratch_get(e))) return rc;
        if ((rc = dense_att_grow(e, job.max_end))) return rc;
        for (size_t i = 0; i < job.steps.size(); ++i)
            if (job.steps[i].wide && (rc = plan_get(e, PlanKey{PlanKind::SlotPrefill, job.steps[i].n, false}, &wide_plans[i]))) return rc;
    }

    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));              // nothing in flight reads the buffers that may be re-allocated
    if ((rc = b->cols_table.grow(n_passes * kColsMax, e->stream))) return rc;
    if ((rc = b->cols_ncols.grow(n_passes, e->stream))) return rc;
    if ((rc = b->cols_prompts.grow(n_prompt, e->stream))) return rc;
    if ((rc = b->cols_out.grow(n_out, e->stream))) return rc;
    if ((rc = b->dense_runs.grow(job.runs.size(), e->stream))) return rc;
    if (lp >= 0 && (rc = genlp_call_begin(e, lp, n_out))) return rc;
    if (n_passes) {
        HIP_TRY(hipMemcpyAsync(b->cols_table, job.table.data(), sizeof(ColEnt) * n_passes * kColsMax, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(b->cols_ncols, job.ncols.data(), 4 * n_passes, hipMemcpyHostToDevice, e->stream));
    }
    HIP_TRY(hipMemcpyAsync(b->cols_prompts, prompts, 4 * n_prompt, hipMemcpyHostToDevice, e->stream));
    if (!job.runs.empty()) HIP_TRY(hipMemcpyAsync(b->dense_runs, job.runs.data(), sizeof(DenseRun) * job.runs.size(), hipMemcpyHostToDevice, e->stream));
    if (draw && n_passes) {
        if ((rc = b->cols_aux.grow(n_passes * kColsMax, e->stream))) return rc;
        HIP_TRY(hipMemcpyAsync(b->cols_aux, job.aux.data(), sizeof(ColAux) * n_passes * kColsMax, hipMemcpyHostToDevice, e->stream));
        if ((rc = cols_sampler_upload(e, smp.slot_ss, b->cols_aux, smp.temperature, smp.topp, smp.seeds, smp.n_requests))) return rc;
    }
    // the coins of the wide blocks first: a turn kernel reads a slot's rng when it sets a pass up, one pass ahead of the stream, so
    // a skip enqueued next to its block would be overwritten by the commit of a pass of the same slot set up before it.  One
    // launch per block: the pieces of a run that spans blocks are the same slot's
    if (job.bcast_slots && (rc = prefix_bcast_slots(e, job.bcast_slots))) return rc;
    if (draw && smp.skip_wide)
        for (const ColsJobStep& s : job.steps)
            if (s.wide && (rc = launch_now(e->stream, k_dense_rng_skip, dim3(1), dim3(64), 0, smp.slot_ss, (const DenseRun*)(b->dense_runs + s.r0), (int)s.nr))) return rc;
    if (n_passes) {
        ColsHost* h = b->h_cols;
        memset(&h->ctl, 0, sizeof(ColsCtl));
        h->ctl.n_passes = (int)n_passes;
        h->ctl.table = b->cols_table;
        h->ctl.ncols = b->cols_ncols;
        h->ctl.prompts = b->cols_prompts;
        h->ctl.out_tokens = b->cols_out;
        HIP_TRY(hipMemcpyAsync(b->cols_ctl, &h->ctl, sizeof(ColsCtl), hipMemcpyHostToDevice, e->stream));
        if ((rc = cols_turn_setup(e, draw))) return rc;
    }
    size_t p = 0;
    for (size_t i = 0; i < job.steps.size(); ++i) {
        const ColsJobStep& s = job.steps[i];
        if (!s.wide) {
            if ((rc = plan_enqueue(e, *plans[cols_width_index(job.ncols[p++])]))) return rc;
            continue;
        }
        if ((rc = dense_enqueue_block(e, *wide_plans[i], b->dense_runs + s.r0, (int)s.nr, s.n, b->cols_prompts))) return rc;
    }
    HIP_TRY(hipGetLastError());
    if (n_out) HIP_TRY(hipMemcpyAsync(out_tokens, b->cols_out, 4 * n_out, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (lp >= 0) genlp_call_end(e, lp, n_out);
    return Q3_OK;
}

// One set of runs that enter their slots together, packed into blocks (dense_blocks, q3_dense_host.inc) and added to the job: a
// wide block is a wide step; a narrower one (and every block of a shape the dense kernels refuse: its cap is 32) is a
// column pass of its live columns, which emit nothing and under the sampler consume their coins (keep = 0).
// runs: slot, first position, prompt offset and length of every run.  first_req (sampled loop only, else nullptr): run i belongs
// to request first_req[i]; loaded / wide_coins are the loop's per-request records of whether a pass has loaded the request's
// sampler into its slot and how many coins its wide pieces stand for.
struct DenseIn { int slot, pos0, src0; size_t len; };
void dense_job_add(q3_engine* e, ColsJob& job, const std::vector<DenseIn>& in, bool draw, const size_t* first_req, std::vector<char>* loaded,
                   std::vector<size_t>* wide_coins, q3_dense_stats& total) {
    std::vector<size_t> lens(in.size());
    for (size_t i = 0; i < in.size(); ++i) lens[i] = in[i].len;
    const DenseBlocks db = dense_blocks(lens.data(), lens.size(), dense_block_cap(e));
    total.blocks += db.stats.blocks;
    total.live_columns += db.stats.live_columns;
    total.pad_columns += db.stats.pad_columns;
    for (const DenseBlock& bl : db.blocks) {
        const size_t i0 = bl.p0, i1 = bl.p0 + bl.np;
        if (bl.wide) {
            job.steps.push_back(ColsJobStep{true, bl.n, job.runs.size(), bl.np});
            for (size_t i = i0; i < i1; ++i) {
                const DensePiece& pc = db.pieces[i];
                const DenseIn& r = in[pc.run];
                job.runs.push_back(DenseRun{pc.col0, r.slot, r.pos0 + (int)pc.off, r.src0 + (int)pc.off, pc.len});
                job.max_end = std::max(job.max_end, (size_t)r.pos0 + pc.off + (size_t)pc.len);
                if (wide_coins) (*wide_coins)[first_req[pc.run]] += (size_t)pc.len;
            }
        } else {
            const size_t p = job.add_pass(draw);
            for (size_t i = i0; i < i1; ++i) {
                const DensePiece& pc = db.pieces[i];
                const DenseIn& r = in[pc.run];
                for (int k = 0; k < pc.len; ++k) {
                    const size_t at = p * kColsMax + job.ncols[p]++;
                    job.table[at] = ColEnt{r.slot, r.pos0 + (int)pc.off + k, r.src0 + (int)pc.off + k, -1};
                    if (!draw) continue;
                    int req = -1;
                    if (loaded && k == 0 && !(*loaded)[first_req[pc.run]]) {
                        req = (int)first_req[pc.run];
                        (*loaded)[first_req[pc.run]] = 1;
                    }
                    job.aux[at] = ColAux{req, k, 0, k == pc.len - 1 ? 1 : 0};
                }
            }
        }
    }
}

// The device-resident loop of q3_generate_many_greedy and (rq.draw) q3_generate_many_sampled: the table is the schedule's rows,
// stepped on the host before the first launch; under the sampler the ColAux rows next to it, the per-request sampler parameters
// and the sampled plans.
// dense_min > 0 (q3_generate_many_dense): a request with prompt_len - 1 >= dense_min enters the schedule with a prompt of one
// column, its last prompt token; the tokens in front of it go through dense blocks enqueued in front of the pass that holds it.
// rq.pos_base > 0 (q3_generate_many_prefix, dense_min 0): the prompts are suffixes behind the resident prefix of pos_base tokens,
// which is copied into the slots in front of the first pass; the scheduler moves every position up by pos_base.
int cols_generate(q3_engine* e, const ColsRequests& rq, int32_t* out_tokens, q3_cols_stats* stats, size_t dense_min = 0, q3_dense_stats* dstats = nullptr) {
    int rc;
    const bool draw = rq.draw();
    BatchCtx* b = e->batch;
    const size_t n_requests = rq.size();
    // what the scheduler sees of a dense request; shift: the positions its blocks take, which the step function does not know of
    ColsRequests seen = rq;
    std::vector<int> shift(n_requests, 0);
    for (size_t r = 0; r < n_requests; ++r)
        if (dense_min > 0 && (size_t)rq.prompt_len[r] - 1 >= dense_min) {
            shift[r] = rq.prompt_len[r] - 1;
            seen.p_off[r] += shift[r];
            seen.prompt_len[r] = 1;
        }
    std::vector<int> got(n_requests, 0);
    ColsSched s;
    cols_sched_init(s, b->max_streams, seen, nullptr, 0, got.data());
    ColsJob job;
    if (rq.pos_base) job.bcast_slots = (int)std::min<size_t>(n_requests, (size_t)b->max_streams);
    q3_dense_stats dst{0, 0, 0};
    std::vector<char> loaded(n_requests, 0);
    std::vector<size_t> wide_coins(n_requests, 0);
    if ((rc = cols_sched_walk(s, seen, [&](size_t, const ColEnt* row, const ColAux* aux, int*) {
            const int n_live = s.status.n_live;
            const auto req_of = [&](const ColEnt& c) { return (size_t)s.slot[c.slot].req; };
            // in front of the pass, the blocks of the dense requests it admits (their one prompt column: src >= 0), in admission order
            std::vector<std::pair<size_t, int>> enter;
            for (int j = 0; j < n_live; ++j)
                if (shift[req_of(row[j])] && row[j].src >= 0) enter.emplace_back(req_of(row[j]), row[j].slot);
            if (!enter.empty()) {
                std::sort(enter.begin(), enter.end());
                std::vector<DenseIn> in;
                std::vector<size_t> in_req;
                for (const auto& en : enter) {
                    in_req.push_back(en.first);
                    in.push_back(DenseIn{en.second, 0, rq.p_off[en.first], (size_t)shift[en.first]});
                }
                dense_job_add(e, job, in, draw, in_req.data(), draw ? &loaded : nullptr, draw ? &wide_coins : nullptr, dst);
            }
            // the pass as the step wrote it (cols_job_run makes the pads), but for what a dense request's blocks have done
            const size_t p = job.add_pass(draw);
            job.ncols[p] = n_live;
            for (int j = 0; j < n_live; ++j) {
                const size_t at = p * kColsMax + j, r = req_of(row[j]);
                job.table[at] = row[j];
                job.table[at].pos += shift[r];
                if (!draw) continue;
                job.aux[at] = aux[j];
                if (shift[r] && row[j].src >= 0) {
                    // the column stands wide_coins coins into its rng (the discarded samples of the positions its wide blocks took),
                    // and a narrow block may have loaded the request's sampler already
                    job.aux[at].k = (int)wide_coins[r];
                    if (loaded[r]) job.aux[at].req = -1;
                }
            }
        })))
        return rc;
    if (draw && (rc = cols_draw_alloc(e))) return rc;        // the loop's per-slot sampler states are allocated there
    const ColsJobSampler smp{b->cols_slot_samp, rq.temperature, rq.topp, rq.seeds, n_requests, false};
    const int pen = e->pen_form();
    if (pen == kPenAdj && (rc = bias_call_begin(e, rq.o_off.data(), n_requests, rq.n_out))) return rc;     // the call's table, on the stream in front of its passes
    if (pen == kPenGuide && (rc = guide_call_begin(e, rq.o_off.data(), n_requests, rq.n_out))) return rc;  // the call's guide and table (section 2r)
    if (pen == kPenGuideSp && (rc = guide_sp_call_begin(e, rq.o_off.data(), n_requests, rq.n_out))) return rc;  // ... in its sparse form (section 2s)
    if ((rc = cols_job_run(e, job, draw, smp, rq.prompts, rq.n_prompt, out_tokens, rq.n_out, e->gen_logprobs, pen))) return rc;
    if (stats) *stats = s.stats;
    if (dstats) *dstats = dst;
    return Q3_OK;
}

}  // namespace

extern "C" {

int q3_batch_step_cols(q3_engine* e, const int32_t* slots, const int32_t* tokens, const int32_t* pos, int n_cols, float* logits_out,
                       int32_t* next_out) {
    g_err[0] = 0;
    int rc;
    if ((rc = cols_prepare(e, "q3_batch_step_cols"))) return rc;
    return cols_step(e, slots, tokens, pos, n_cols, nullptr, logits_out, next_out, false);
}

int q3_batch_step_cols_draw(q3_engine* e, const int32_t* slots, const int32_t* tokens, const int32_t* pos, int n_cols, const uint8_t* keep,
                            float* logits_out, int32_t* next_out) {
    g_err[0] = 0;
    int rc;
    if ((rc = cols_prepare(e, "q3_batch_step_cols_draw", true))) return rc;
    return cols_step(e, slots, tokens, pos, n_cols, keep, logits_out, next_out, e->batch->sampling);   // temperature 0: the greedy pass
}

int q3_cols_schedule(const size_t* prompt_len, const size_t* n_new, size_t n_requests, int max_streams, int32_t* table, size_t cap,
                     size_t* n_entries, q3_cols_stats* stats) {
    g_err[0] = 0;
    return cols_schedule_table(prompt_len, n_new, n_requests, max_streams, nullptr, nullptr, 0, table, cap, n_entries, nullptr, stats);
}

int q3_generate_many_greedy(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, const size_t* n_new, size_t n_requests,
                            int32_t* out_tokens, q3_cols_stats* stats) {
    g_err[0] = 0;
    genlp_call_enter(e);
    if (stats) *stats = q3_cols_stats{0, 0, 0, 0};
    int rc;
    ColsRequests rq;
    if ((rc = cols_prepare(e, "q3_generate_many_greedy"))) return rc;
    if ((rc = cols_requests_check(e, prompts, prompt_len, n_new, n_requests, false, nullptr, nullptr, nullptr, 0, out_tokens, rq))) return rc;
    return cols_generate(e, rq, out_tokens, stats);
}

int q3_generate_many_sampled(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, const size_t* n_new, size_t n_requests,
                             const float* temperature, const float* topp, const uint64_t* seeds, int32_t* out_tokens, q3_cols_stats* stats) {
    g_err[0] = 0;
    genlp_call_enter(e);
    if (stats) *stats = q3_cols_stats{0, 0, 0, 0};
    int rc;
    ColsRequests rq;
    if ((rc = cols_prepare(e, "q3_generate_many_sampled", true))) return rc;
    if ((rc = cols_requests_check(e, prompts, prompt_len, n_new, n_requests, true, temperature, topp, seeds, 0, out_tokens, rq))) return rc;
    return cols_generate(e, rq, out_tokens, stats);
}

/* ---- section 2g: dense blocks over the slots ---- */

int q3_batch_prefill_slots(q3_engine* e, const int32_t* slots, const int32_t* tokens, const size_t* run_len, const int32_t* first_pos, size_t n_runs,
                           q3_dense_stats* stats) {
    g_err[0] = 0;
    if (stats) *stats = q3_dense_stats{0, 0, 0};
    int rc;
    if ((rc = cols_prepare(e, "q3_batch_prefill_slots", true))) return rc;
    BatchCtx* b = e->batch;
    if (!slots || !tokens || !run_len || !first_pos || n_runs == 0) return fail(Q3_ERR_ARG, "null or empty run list");
    bool seen[kMaxStreams] = {false};
    std::vector<DenseIn> in;
    size_t n_tok = 0;
    for (size_t r = 0; r < n_runs; ++r) {
        if (slots[r] < 0 || slots[r] >= b->max_streams) return fail(Q3_ERR_ARG, "run %zu: slot %d out of range (0..%d)", r, slots[r], b->max_streams - 1);
        if (seen[slots[r]]) return fail(Q3_ERR_ARG, "run %zu: slot %d is named twice", r, slots[r]);
        seen[slots[r]] = true;
        if (run_len[r] == 0) return fail(Q3_ERR_ARG, "run %zu is empty", r);
        if (first_pos[r] < 0 || run_len[r] > (size_t)b->ctx || (size_t)first_pos[r] + run_len[r] > (size_t)b->ctx)
            return fail(Q3_ERR_ARG, "run %zu: first_pos %d + %zu tokens exceeds seq_len %d", r, first_pos[r], run_len[r], b->ctx);
        in.push_back(DenseIn{slots[r], first_pos[r], (int)n_tok, run_len[r]});
        n_tok += run_len[r];
    }
    for (size_t i = 0; i < n_tok; ++i)
        if (tokens[i] < 0 || tokens[i] >= e->cfg.vocab_size)
            return fail(Q3_ERR_ARG, "index out of range: token %d (vocab_size %d)", tokens[i], e->cfg.vocab_size);
    const bool draw = b->sampling;                  // temperature 0, or no batch sampler: no rng is touched
    ColsJob job;
    q3_dense_stats dst{0, 0, 0};
    dense_job_add(e, job, in, draw, nullptr, nullptr, nullptr, dst);
    const ColsJobSampler smp{b->draw_decode.ss, nullptr, nullptr, nullptr, 0, true};
    if ((rc = cols_job_run(e, job, draw, smp, tokens, n_tok, nullptr, 0))) return rc;
    if (stats) *stats = dst;
    return Q3_OK;
}

int q3_generate_many_dense(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, const size_t* n_new, size_t n_requests,
                           const float* temperature, const float* topp, const uint64_t* seeds, size_t dense_min, int32_t* out_tokens,
                           q3_cols_stats* stats, q3_dense_stats* dstats) {
    g_err[0] = 0;
    genlp_call_enter(e);
    if (stats) *stats = q3_cols_stats{0, 0, 0, 0};
    if (dstats) *dstats = q3_dense_stats{0, 0, 0};
    int rc;
    ColsRequests rq;
    const bool draw = temperature || topp || seeds;
    if ((rc = cols_prepare(e, "q3_generate_many_dense", draw))) return rc;
    if ((rc = cols_requests_check(e, prompts, prompt_len, n_new, n_requests, draw, temperature, topp, seeds, 0, out_tokens, rq))) return rc;
    return cols_generate(e, rq, out_tokens, stats, dense_min, dstats);
}

/* ---- section 2o: log-probability records of the generated tokens ---- */

int q3_gen_logprobs(q3_engine* e, int top_n) {
    g_err[0] = 0;
    if (top_n < -1 || top_n > kScoreTopMax) return fail(Q3_ERR_ARG, "top_n %d out of range (-1..%d)", top_n, kScoreTopMax);
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    if (top_n > e->cfg.vocab_size) return fail(Q3_ERR_ARG, "top_n %d exceeds vocab_size %d", top_n, e->cfg.vocab_size);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    // a batched state that is not there yet gets its buffers from the first generate call that runs under the setting
    int rc;
    if (top_n >= 0 && e->batch && e->batch->has_kv && (rc = genlp_alloc(e))) return rc;
    e->gen_logprobs = top_n;
    return Q3_OK;
}

int q3_gen_logprobs_get(const q3_engine* e, int* top_n) {
    g_err[0] = 0;
    if (!e || !top_n) return fail(Q3_ERR_ARG, "null argument");
    *top_n = e->gen_logprobs;
    return Q3_OK;
}

/* ---- section 2p: presence and frequency penalties ---- */

int q3_sampler_penalties(q3_engine* e, float presence, float frequency) {
    g_err[0] = 0;
    if (int rc = penalties_check(presence, frequency)) return rc;
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const float p0 = e->pen_presence, f0 = e->pen_frequency;
    e->pen_presence = presence;
    e->pen_frequency = frequency;
    // a batched state that is not there yet gets the penalty state from the first generate call that runs under the setting
    int rc = Q3_OK;
    if (e->batch && e->batch->has_kv) {
        // (the rows, keys and setting may stand there without counts: a table of section 2q made them)
        if (e->pen_on()) rc = pen_alloc(e);
        if (!rc && e->batch->pen_ctl) rc = pen_ctl_upload(e);
    }
    if (rc) { e->pen_presence = p0; e->pen_frequency = f0; }
    return rc;
}

int q3_sampler_get_penalties(const q3_engine* e, float* presence, float* frequency) {
    g_err[0] = 0;
    if (!e || !presence || !frequency) return fail(Q3_ERR_ARG, "null argument");
    *presence = e->pen_presence;
    *frequency = e->pen_frequency;
    return Q3_OK;
}

/* ---- section 2q: logit bias, banned and allowed tokens ---- */

int q3_logit_bias_set(q3_engine* e, const q3_bias_entry* entries, const size_t* n_entries, const uint8_t* mode, size_t n_lists) {
    g_err[0] = 0;
    BiasTable t;
    if (int rc = bias_check(entries, n_entries, mode, n_lists, -1, t)) return rc;
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    if (int rc = bias_check(entries, n_entries, mode, n_lists, (long)e->cfg.vocab_size, t)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->bias = std::move(t);
    return Q3_OK;
}

int q3_logit_bias_get(const q3_engine* e, size_t* n_lists, size_t* n_entries_total) {
    g_err[0] = 0;
    if (!e || !n_lists || !n_entries_total) return fail(Q3_ERR_ARG, "null argument");
    *n_lists = e->bias.n_lists();
    *n_entries_total = e->bias.entries.size();
    return Q3_OK;
}

/* ---- section 2r: guided decoding ---- */

int q3_guide_set(q3_engine* e, const int16_t* next, size_t n_states, size_t vocab, const int32_t* start, size_t n_start) {
    g_err[0] = 0;
    if (int rc = guide_check(next, n_states, vocab, start, n_start)) return rc;
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    if (n_states && vocab != (size_t)e->cfg.vocab_size) return fail(Q3_ERR_ARG, "a guide over %zu tokens (vocab_size %d)", vocab, e->cfg.vocab_size);
    GuideTable t;
    if (n_states) {
        t.next.assign(next, next + n_states * vocab);
        t.start.assign(start, start + n_start);
        t.n_states = n_states;
        t.vocab = vocab;
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    t.serial = ++e->guide_serial;
    e->guide = std::move(t);
    e->guide_sp = GuideSparse{};         // one guide holds at a time (section 2s)
    return Q3_OK;
}

int q3_guide_get(const q3_engine* e, size_t* n_states, size_t* n_start) {
    g_err[0] = 0;
    if (!e || !n_states || !n_start) return fail(Q3_ERR_ARG, "null argument");
    *n_states = e->guide.n_states;
    *n_start = e->guide.start.size();
    return Q3_OK;
}

/* ---- section 2s: sparse guides ---- */

int q3_guide_set_sparse(q3_engine* e, const int32_t* dflt, const uint32_t* row_off, const q3_guide_edge* edges, size_t n_states, size_t n_edges, size_t vocab,
                        const int32_t* start, size_t n_start) {
    g_err[0] = 0;
    if (int rc = guide_sparse_check(dflt, row_off, edges, n_states, n_edges, vocab, start, n_start)) return rc;
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    if (n_states && vocab != (size_t)e->cfg.vocab_size) return fail(Q3_ERR_ARG, "a guide over %zu tokens (vocab_size %d)", vocab, e->cfg.vocab_size);
    GuideSparse t;
    if (n_states) {
        t.dflt.assign(dflt, dflt + n_states);
        t.row_off.assign(row_off, row_off + n_states + 1);
        t.edges.resize(n_edges);
        if (n_edges) memcpy(t.edges.data(), edges, sizeof(GuideEdge) * n_edges);
        t.start.assign(start, start + n_start);
        t.n_states = n_states;
        t.vocab = vocab;
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    t.serial = ++e->guide_serial;
    e->guide_sp = std::move(t);
    e->guide = GuideTable{};             // one guide holds at a time
    return Q3_OK;
}

int q3_guide_get_sparse(const q3_engine* e, size_t* n_states, size_t* n_edges, size_t* n_start) {
    g_err[0] = 0;
    if (!e || !n_states || !n_edges || !n_start) return fail(Q3_ERR_ARG, "null argument");
    *n_states = e->guide_sp.n_states;
    *n_edges = e->guide_sp.edges.size();
    *n_start = e->guide_sp.start.size();
    return Q3_OK;
}

/* ---- section 2t: stop sequences (the loop and the host twin: q3_stop_host.inc) ---- */

int q3_stop_seq_set(q3_engine* e, const int32_t* dflt, const uint32_t* row_off, const q3_guide_edge* edges, size_t n_states, size_t n_edges, size_t vocab,
                    const int32_t* start, size_t n_start) {
    g_err[0] = 0;
    if (int rc = stop_seq_check(dflt, row_off, edges, n_states, n_edges, vocab, start, n_start)) return rc;
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    if (n_states && vocab != (size_t)e->cfg.vocab_size) return fail(Q3_ERR_ARG, "a stop automaton over %zu tokens (vocab_size %d)", vocab, e->cfg.vocab_size);
    GuideSparse t;
    if (n_states) {
        t.dflt.assign(dflt, dflt + n_states);
        t.row_off.assign(row_off, row_off + n_states + 1);
        t.edges.resize(n_edges);
        if (n_edges) memcpy(t.edges.data(), edges, sizeof(GuideEdge) * n_edges);
        t.start.assign(start, start + n_start);
        t.n_states = n_states;
        t.vocab = vocab;
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    t.serial = ++e->guide_serial;
    e->stop_seq = std::move(t);
    return Q3_OK;
}

int q3_stop_seq_get(const q3_engine* e, size_t* n_states, size_t* n_edges, size_t* n_start) {
    g_err[0] = 0;
    if (!e || !n_states || !n_edges || !n_start) return fail(Q3_ERR_ARG, "null argument");
    *n_states = e->stop_seq.n_states;
    *n_edges = e->stop_seq.edges.size();
    *n_start = e->stop_seq.start.size();
    return Q3_OK;
}

int q3_gen_logprobs_read(q3_engine* e, size_t first, size_t count, q3_score_rec* recs, q3_score_top* top, int32_t* rank) {
    g_err[0] = 0;
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    const BatchCtx* b = e->batch;
    if (!b || !b->genlp_valid) return fail(Q3_ERR_ARG, "the last q3_generate_many_* call left no records: none has run with q3_gen_logprobs on, or it failed");
    if (first > b->genlp_count || count > b->genlp_count - first)
        return fail(Q3_ERR_ARG, "records %zu .. %zu of %zu", first, first + count, b->genlp_count);
    const size_t k = (size_t)b->genlp_top_n;
    if (!recs) return fail(Q3_ERR_ARG, "null recs");
    if (k > 0 && !top) return fail(Q3_ERR_ARG, "null top: the call ran with top_n %zu", k);
    HIP_TRY(hipSetDevice(e->device));
    if (count) {
        HIP_TRY(hipMemcpyAsync(recs, b->genlp_recs + first, sizeof(ScoreRec) * count, hipMemcpyDeviceToHost, e->stream));
        if (k > 0) HIP_TRY(hipMemcpyAsync(top, b->genlp_top + first * k, sizeof(ScoreTop) * count * k, hipMemcpyDeviceToHost, e->stream));
        if (k > 0 && rank) HIP_TRY(hipMemcpyAsync(rank, b->genlp_rank + first, sizeof(int32_t) * count, hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return Q3_OK;
}

}  // extern "C"
