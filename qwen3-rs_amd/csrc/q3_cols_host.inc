// q3_cols_host.inc -- host side of the column passes (include/qwen3_hip.h sections 2e and 2f; included by q3_engine.hip behind
// q3_batch_host.inc, same translation unit).
//
// A pass is up to 32 columns of (slot, token, position) over the per-stream KV caches of the batched state: decode columns of some
// slots next to runs of consecutive prompt positions of others, one pass over the packed weights (PlanKind::Cols).  The loop
// q3_generate_many_greedy walks a pass table that is a pure function of the request lengths (cols_schedule_run): the host
// knows every pass's width in advance, the device resolves every pass's tokens itself (k_cols_turn).
// Section 2f is the same under the sampler: a second set of plans whose classifier is followed by the per-column draws and
// k_cols_turn_draw (q3_sampler.h), the greedy plans and their launches untouched.

namespace {

// The schedule of q3_generate_many_greedy (stated in the header): emit(pass, slot, pos, request) for every column, in column order.
template <class Emit>
void cols_schedule_run(const size_t* prompt_len, const size_t* n_new, size_t n_requests, int max_streams, Emit&& emit, q3_cols_stats& st) {
    struct Slot { long req = -1; size_t fed = 0, g = 0; };
    Slot s[kColsMax];
    size_t next = 0, active = 0;
    st = q3_cols_stats{0, 0, 0, 0};
    while (next < n_requests || active > 0) {
        // 1. admit: the next request, in ascending index, takes the lowest free slot
        for (int i = 0; i < max_streams && next < n_requests; ++i)
            if (s[i].req < 0) {
                s[i] = Slot{(long)next++, 0, 0};
                ++active;
            }
        int cols = 0, took[kColsMax] = {0};
        bool dec[kColsMax] = {false};
        // 2. one column per decode-phase slot
        for (int i = 0; i < max_streams; ++i)
            if (s[i].req >= 0 && s[i].fed == prompt_len[s[i].req]) {
                emit(st.passes, i, s[i].fed + s[i].g - 1, (size_t)s[i].req);
                dec[i] = true;
                ++cols;
                ++st.decode_columns;
            }
        // 3. prompt-phase slots share what is left of the pass
        for (int i = 0; i < max_streams && cols < kColsMax; ++i)
            if (s[i].req >= 0 && !dec[i]) {
                const size_t left = prompt_len[s[i].req] - s[i].fed;
                took[i] = (int)std::min<size_t>(left, (size_t)(kColsMax - cols));
                for (int k = 0; k < took[i]; ++k) emit(st.passes, i, s[i].fed + k, (size_t)s[i].req);
                cols += took[i];
                st.prompt_columns += took[i];
            }
        // 4. / 5. phase changes and finished requests
        for (int i = 0; i < max_streams; ++i) {
            if (s[i].req < 0) continue;
            if (dec[i]) ++s[i].g;
            else if (took[i]) {
                s[i].fed += took[i];
                if (s[i].fed == prompt_len[s[i].req]) s[i].g = 1;      // the run's last column emitted y_0
            }
            if (s[i].g == n_new[s[i].req]) {
                s[i].req = -1;
                --active;
            }
        }
        st.live_columns += cols;
        ++st.passes;
    }
}

int cols_schedule_check(const size_t* prompt_len, const size_t* n_new, size_t n_requests, int max_streams) {
    if (!prompt_len || !n_new || n_requests == 0) return fail(Q3_ERR_ARG, "null or empty request list");
    if (max_streams < 1 || max_streams > kMaxStreams) return fail(Q3_ERR_ARG, "max_streams %d out of range (1..%d)", max_streams, kMaxStreams);
    for (size_t r = 0; r < n_requests; ++r)
        if (prompt_len[r] == 0 || n_new[r] == 0) return fail(Q3_ERR_ARG, "request %zu: empty prompt or n_new 0", r);
    return Q3_OK;
}

int cols_width_index(int n) {
    int w = 0;
    while (kColsWidths[w] < n) ++w;
    return w;
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

// the plan of width kColsWidths[wi], built on first use.  batch_build_plan leaves it in b->plan / b->graph: it moves to the
// cache, and the shared plan is marked stale (the next decode / prefill / verify call rebuilds its own, as after any change of kind).
// draw: the sampled plan of that width (cols_draw_alloc has run: its launches carry the buffers allocated there).
int cols_plan_get(q3_engine* e, int wi, ColsPlan** out, bool draw = false) {
    BatchCtx* b = e->batch;
    ColsPlan& p = draw ? b->cols_plans_draw[wi] : b->cols_plans[wi];
    if (p.plan.empty()) {
        HIP_TRY(hipSetDevice(e->device));
        const int rc = batch_build_plan(e, kColsWidths[wi], PlanKind::Cols, draw);
        if (rc == Q3_OK) {
            p.plan.swap(b->plan);
            p.graph.swap(b->graph);
        }
        b->plan.clear();
        b->graph.reset();
        b->plan_streams = 0;
        if (rc) return rc;
    }
    *out = &p;
    return Q3_OK;
}

int cols_enqueue(q3_engine* e, const ColsPlan& p) {
    if (p.graph) return p.graph.launch(e->stream);
    for (const Launch& Ln : p.plan) launch(Ln, e->stream);
    HIP_TRY(hipGetLastError());
    return Q3_OK;
}

template <class T>
int cols_grow(T*& ptr, size_t& cap, size_t need) {
    if (need <= cap) return Q3_OK;
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
    HIP_TRY(hipMalloc((void**)&ptr, sizeof(T) * need));
    cap = need;
    return Q3_OK;
}

// The buffers of the sampled passes, on first use: the column sampler states and the draw scratch of the verify pass
// (spec_draw_alloc, 32 columns wide whatever max_streams is), the control block of k_cols_turn_draw, the one-pass table of a
// host-made pass and the loop's per-slot sampler states.  Freed with the context.
int cols_draw_alloc(q3_engine* e) {
    BatchCtx* b = e->batch;
    int rc;
    if (!b->spec_samp && (rc = spec_draw_alloc(e))) return rc;
    if (b->h_cols_draw) return Q3_OK;
    HIP_TRY(hipSetDevice(e->device));
    if (!b->cols_draw) HIP_TRY(hipMalloc((void**)&b->cols_draw, sizeof(ColsDraw)));
    HIP_TRY(hipMemsetAsync(b->cols_draw, 0, sizeof(ColsDraw), e->stream));
    if (!b->cols_step) HIP_TRY(hipMalloc((void**)&b->cols_step, sizeof(ColsStep)));
    if (!b->cols_slot_samp) HIP_TRY(hipMalloc((void**)&b->cols_slot_samp, sizeof(SamplerState) * kMaxStreams));
    HIP_TRY(hipMemsetAsync(b->cols_slot_samp, 0, sizeof(SamplerState) * kMaxStreams, e->stream));
    HIP_TRY(hipHostMalloc((void**)&b->h_cols_draw, sizeof(ColsDrawHost), hipHostMallocDefault));
    return Q3_OK;
}

// One host-made pass.  draw = false: the states and the slot table are written here and the greedy plan commits the argmaxes.
// draw = true: the pass goes through a one-pass table, set up by a k_cols_turn_draw launch in front of the sampled plan -- the
// column sampler states derive from the slot states in device memory (the batch sampler's d_sampler: slot i = stream i).
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
    ColsPlan* plan;
    if ((rc = cols_plan_get(e, cols_width_index(n_cols), &plan, draw))) return rc;
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
        hd->dr.slot_ss = b->d_sampler;
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
        if ((rc = launch_now(e->stream, k_cols_turn_draw, dim3(1), dim3(kWG), 0, b->cols_ctl, b->cols_draw, b->spec_samp, b->st, b->col_slot))) return rc;
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
    if ((rc = cols_enqueue(e, *plan))) return rc;
    const size_t V = e->cfg.vocab_size;
    if (logits_out) HIP_TRY(hipMemcpyAsync(b->h_logits, b->logits, 4 * V * (size_t)n_cols, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(&h->ctl, b->cols_ctl, sizeof(ColsCtl), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (logits_out) memcpy(logits_out, b->h_logits, 4 * V * (size_t)n_cols);
    if (next_out)
        for (int j = 0; j < n_cols; ++j) next_out[j] = h->ctl.next[j];
    return Q3_OK;
}

// The device-resident loop of q3_generate_many_greedy (temperature == nullptr) and q3_generate_many_sampled: the same schedule and
// table; under the sampler a parallel table of ColAux, the per-request sampler parameters and the sampled plans.
int cols_generate(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, const size_t* n_new, size_t n_requests, const float* temperature,
                  const float* topp, const uint64_t* seeds, int32_t* out_tokens, q3_cols_stats* stats) {
    int rc;
    const bool draw = temperature != nullptr;
    BatchCtx* b = e->batch;
    if (!prompts || !out_tokens) return fail(Q3_ERR_ARG, "null argument");
    if ((rc = cols_schedule_check(prompt_len, n_new, n_requests, b->max_streams))) return rc;
    std::vector<size_t> p_off(n_requests), o_off(n_requests);
    size_t n_prompt = 0, n_out = 0;
    for (size_t r = 0; r < n_requests; ++r) {
        if (prompt_len[r] + n_new[r] - 1 > (size_t)b->ctx)
            return fail(Q3_ERR_ARG, "request %zu: prompt of %zu + %zu new tokens exceeds seq_len %d", r, prompt_len[r], n_new[r], b->ctx);
        p_off[r] = n_prompt;
        o_off[r] = n_out;
        n_prompt += prompt_len[r];
        n_out += n_new[r];
    }
    for (size_t i = 0; i < n_prompt; ++i)
        if (prompts[i] < 0 || prompts[i] >= e->cfg.vocab_size)
            return fail(Q3_ERR_ARG, "index out of range: token %d (vocab_size %d)", prompts[i], e->cfg.vocab_size);
    if (n_prompt > (size_t)INT32_MAX || n_out > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 tokens in one call");

    // the pass table: kColsMax entries per pass, pads repeat the pass's last live column and emit nothing
    std::vector<ColEnt> table;
    std::vector<ColAux> aux;
    std::vector<int> ncols;
    q3_cols_stats st;
    cols_schedule_run(prompt_len, n_new, n_requests, b->max_streams, [&](uint64_t pass, int slot, size_t pos, size_t req) {
        if (pass == ncols.size()) {
            ncols.push_back(0);
            table.resize(table.size() + kColsMax);
            if (draw) aux.resize(table.size());
        }
        ColEnt c;
        c.slot = slot;
        c.pos = (int)pos;
        c.src = pos < prompt_len[req] ? (int)(p_off[req] + pos) : -1;
        c.out = pos + 1 >= prompt_len[req] ? (int)(o_off[req] + (pos + 1 - prompt_len[req])) : -1;
        const size_t at = (size_t)pass * kColsMax + ncols[pass]++;
        table[at] = c;
        if (draw) {          // a request enters at position 0; the run's earlier column is the entry in front (one run per slot)
            const bool in_run = ncols[pass] > 1 && table[at - 1].slot == slot;
            aux[at] = ColAux{pos == 0 ? (int)req : -1, in_run ? aux[at - 1].k + 1 : 0, c.out >= 0 ? 1 : 0, 1};
            if (in_run) aux[at - 1].last = 0;
        }
    }, st);
    const size_t n_passes = ncols.size();
    bool width_used[kColsNW] = {false};
    for (size_t p = 0; p < n_passes; ++p) {
        ColEnt pad = table[p * kColsMax + ncols[p] - 1];
        pad.out = -1;
        for (int j = ncols[p]; j < kColsMax; ++j) table[p * kColsMax + j] = pad;
        if (draw)
            for (int j = ncols[p]; j < kColsMax; ++j) aux[p * kColsMax + j] = ColAux{-1, aux[p * kColsMax + ncols[p] - 1].k, 0, 0};
        width_used[cols_width_index(ncols[p])] = true;
    }
    // every plan the call needs exists before the first pass is enqueued
    if (draw && (rc = cols_draw_alloc(e))) return rc;
    ColsPlan* plans[kColsNW] = {nullptr};
    for (int w = 0; w < kColsNW; ++w)
        if (width_used[w] && (rc = cols_plan_get(e, w, &plans[w], draw))) return rc;

    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));              // nothing in flight reads the buffers that may be re-allocated
    if ((rc = cols_grow(b->cols_table, b->cols_table_cap, n_passes * kColsMax))) return rc;
    if ((rc = cols_grow(b->cols_ncols, b->cols_ncols_cap, n_passes))) return rc;
    if ((rc = cols_grow(b->cols_prompts, b->cols_prompts_cap, n_prompt))) return rc;
    if ((rc = cols_grow(b->cols_out, b->cols_out_cap, n_out))) return rc;
    // the only uploads of the call
    HIP_TRY(hipMemcpyAsync(b->cols_table, table.data(), sizeof(ColEnt) * n_passes * kColsMax, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(b->cols_ncols, ncols.data(), 4 * n_passes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(b->cols_prompts, prompts, 4 * n_prompt, hipMemcpyHostToDevice, e->stream));
    if (draw) {
        if ((rc = cols_grow(b->cols_aux, b->cols_aux_cap, n_passes * kColsMax))) return rc;
        if ((rc = cols_grow(b->cols_temp, b->cols_temp_cap, n_requests))) return rc;
        if ((rc = cols_grow(b->cols_topp, b->cols_topp_cap, n_requests))) return rc;
        if ((rc = cols_grow(b->cols_seeds, b->cols_seeds_cap, n_requests))) return rc;
        HIP_TRY(hipMemcpyAsync(b->cols_aux, aux.data(), sizeof(ColAux) * n_passes * kColsMax, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(b->cols_temp, temperature, 4 * n_requests, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(b->cols_topp, topp, 4 * n_requests, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(b->cols_seeds, seeds, 8 * n_requests, hipMemcpyHostToDevice, e->stream));
        ColsDraw& dr = b->h_cols_draw->dr;
        memset(&dr, 0, sizeof(ColsDraw));
        dr.slot_ss = b->cols_slot_samp;
        dr.aux = b->cols_aux;
        dr.temperature = b->cols_temp;
        dr.topp = b->cols_topp;
        dr.seeds = b->cols_seeds;
        HIP_TRY(hipMemcpyAsync(b->cols_draw, &dr, sizeof(ColsDraw), hipMemcpyHostToDevice, e->stream));
    }
    ColsHost* h = b->h_cols;
    memset(&h->ctl, 0, sizeof(ColsCtl));
    h->ctl.n_passes = (int)n_passes;
    h->ctl.table = b->cols_table;
    h->ctl.ncols = b->cols_ncols;
    h->ctl.prompts = b->cols_prompts;
    h->ctl.out_tokens = b->cols_out;
    HIP_TRY(hipMemcpyAsync(b->cols_ctl, &h->ctl, sizeof(ColsCtl), hipMemcpyHostToDevice, e->stream));
    // pass 0 is set up by a launch of its own (nothing to commit); every later pass by the k_cols_turn that ends the pass before it
    if (draw) {
        if ((rc = launch_now(e->stream, k_cols_turn_draw, dim3(1), dim3(kWG), 0, b->cols_ctl, b->cols_draw, b->spec_samp, b->st, b->col_slot))) return rc;
    } else if ((rc = launch_now(e->stream, k_cols_turn, dim3(1), dim3(kWG), 0, b->cols_ctl, b->slots, b->nslots, 0, b->st, b->col_slot))) return rc;
    for (size_t p = 0; p < n_passes; ++p)
        if ((rc = cols_enqueue(e, *plans[cols_width_index(ncols[p])]))) return rc;
    HIP_TRY(hipMemcpyAsync(out_tokens, b->cols_out, 4 * n_out, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (stats) *stats = st;
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
    int rc;
    if ((rc = cols_schedule_check(prompt_len, n_new, n_requests, max_streams))) return rc;
    size_t n = 0;
    q3_cols_stats st;
    cols_schedule_run(prompt_len, n_new, n_requests, max_streams, [&](uint64_t pass, int slot, size_t pos, size_t req) {
        if (table && n < cap) {
            table[4 * n + 0] = (int32_t)pass;
            table[4 * n + 1] = slot;
            table[4 * n + 2] = (int32_t)pos;
            table[4 * n + 3] = (int32_t)req;
        }
        ++n;
    }, st);
    if (n_entries) *n_entries = n;
    if (stats) *stats = st;
    if (table && n > cap) return fail(Q3_ERR_ARG, "the schedule has %zu entries, the table holds %zu", n, cap);
    return Q3_OK;
}

int q3_generate_many_greedy(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, const size_t* n_new, size_t n_requests,
                            int32_t* out_tokens, q3_cols_stats* stats) {
    g_err[0] = 0;
    if (stats) *stats = q3_cols_stats{0, 0, 0, 0};
    int rc;
    if ((rc = cols_prepare(e, "q3_generate_many_greedy"))) return rc;
    return cols_generate(e, prompts, prompt_len, n_new, n_requests, nullptr, nullptr, nullptr, out_tokens, stats);
}

int q3_generate_many_sampled(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, const size_t* n_new, size_t n_requests,
                             const float* temperature, const float* topp, const uint64_t* seeds, int32_t* out_tokens, q3_cols_stats* stats) {
    g_err[0] = 0;
    if (stats) *stats = q3_cols_stats{0, 0, 0, 0};
    int rc;
    if ((rc = cols_prepare(e, "q3_generate_many_sampled", true))) return rc;
    if (!temperature || !topp || !seeds) return fail(Q3_ERR_ARG, "null argument");
    if (!prompt_len || !n_new || n_requests == 0) return fail(Q3_ERR_ARG, "null or empty request list");
    for (size_t r = 0; r < n_requests; ++r) {
        if (!(temperature[r] >= 0.0f)) return fail(Q3_ERR_ARG, "request %zu: Temperature must be non-negative", r);
        if (!(topp[r] >= 0.0f && topp[r] <= 1.0f)) return fail(Q3_ERR_ARG, "request %zu: Top-p must be between 0.0 and 1.0", r);
    }
    return cols_generate(e, prompts, prompt_len, n_new, n_requests, temperature, topp, seeds, out_tokens, stats);
}

}  // extern "C"
