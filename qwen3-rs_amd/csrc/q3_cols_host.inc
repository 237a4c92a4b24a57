// q3_cols_host.inc -- host side of the column passes (include/qwen3_hip.h section 2e; included by q3_engine.hip behind
// q3_batch_host.inc, same translation unit).
//
// A pass is up to 32 columns of (slot, token, position) over the per-stream KV caches of the batched state: decode columns of some
// slots next to runs of consecutive prompt positions of others, one pass over the packed weights (PlanKind::Cols).  The loop
// q3_generate_many_greedy walks a pass table that is a pure function of the request lengths (cols_schedule_run): the host
// knows every pass's width in advance, the device resolves every pass's tokens itself (k_cols_turn).

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

// what every entry point of section 2e refuses
int cols_prepare(q3_engine* e, const char* who) {
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    if (!e->batch || !e->batch->has_kv) return fail(Q3_ERR_ARG, "q3_batch_init has not been called");
    if (e->flags & Q3_FLAG_FAST)
        return fail(Q3_ERR_UNSUPPORTED, "%s needs a reference-order engine: with Q3_FLAG_FAST the block kernels and the decode kernels are not bit-equal", who);
    if (e->batch->sampling)
        return fail(Q3_ERR_UNSUPPORTED, "%s is greedy only: the batch sampler is set to a temperature > 0", who);
    return Q3_OK;
}

// the plan of width kColsWidths[wi], built on first use.  batch_build_plan leaves it in b->plan / b->graph: it moves to the
// cache, and the shared plan is marked stale (the next decode / prefill / verify call rebuilds its own, as after any change of kind).
int cols_plan_get(q3_engine* e, int wi, ColsPlan** out) {
    BatchCtx* b = e->batch;
    ColsPlan& p = b->cols_plans[wi];
    if (p.plan.empty()) {
        HIP_TRY(hipSetDevice(e->device));
        const int rc = batch_build_plan(e, kColsWidths[wi], PlanKind::Cols);
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

}  // namespace

extern "C" {

int q3_batch_step_cols(q3_engine* e, const int32_t* slots, const int32_t* tokens, const int32_t* pos, int n_cols, float* logits_out,
                       int32_t* next_out) {
    g_err[0] = 0;
    int rc;
    if ((rc = cols_prepare(e, "q3_batch_step_cols"))) return rc;
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
    ColsPlan* plan;
    if ((rc = cols_plan_get(e, cols_width_index(n_cols), &plan))) return rc;
    HIP_TRY(hipSetDevice(e->device));
    ColsHost* h = b->h_cols;
    memset(&h->ctl, 0, sizeof(ColsCtl));
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
    std::vector<int> ncols;
    q3_cols_stats st;
    cols_schedule_run(prompt_len, n_new, n_requests, b->max_streams, [&](uint64_t pass, int slot, size_t pos, size_t req) {
        if (pass == ncols.size()) {
            ncols.push_back(0);
            table.resize(table.size() + kColsMax);
        }
        ColEnt c;
        c.slot = slot;
        c.pos = (int)pos;
        c.src = pos < prompt_len[req] ? (int)(p_off[req] + pos) : -1;
        c.out = pos + 1 >= prompt_len[req] ? (int)(o_off[req] + (pos + 1 - prompt_len[req])) : -1;
        table[(size_t)pass * kColsMax + ncols[pass]++] = c;
    }, st);
    const size_t n_passes = ncols.size();
    bool width_used[kColsNW] = {false};
    for (size_t p = 0; p < n_passes; ++p) {
        ColEnt pad = table[p * kColsMax + ncols[p] - 1];
        pad.out = -1;
        for (int j = ncols[p]; j < kColsMax; ++j) table[p * kColsMax + j] = pad;
        width_used[cols_width_index(ncols[p])] = true;
    }
    // every plan the call needs exists before the first pass is enqueued
    ColsPlan* plans[kColsNW] = {nullptr};
    for (int w = 0; w < kColsNW; ++w)
        if (width_used[w] && (rc = cols_plan_get(e, w, &plans[w]))) return rc;

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
    ColsHost* h = b->h_cols;
    memset(&h->ctl, 0, sizeof(ColsCtl));
    h->ctl.n_passes = (int)n_passes;
    h->ctl.table = b->cols_table;
    h->ctl.ncols = b->cols_ncols;
    h->ctl.prompts = b->cols_prompts;
    h->ctl.out_tokens = b->cols_out;
    HIP_TRY(hipMemcpyAsync(b->cols_ctl, &h->ctl, sizeof(ColsCtl), hipMemcpyHostToDevice, e->stream));
    // pass 0 is set up by a launch of its own (nothing to commit); every later pass by the k_cols_turn that ends the pass before it
    if ((rc = launch_now(e->stream, k_cols_turn, dim3(1), dim3(kWG), 0, b->cols_ctl, b->slots, b->nslots, 0, b->st, b->col_slot))) return rc;
    for (size_t p = 0; p < n_passes; ++p)
        if ((rc = cols_enqueue(e, *plans[cols_width_index(ncols[p])]))) return rc;
    HIP_TRY(hipMemcpyAsync(out_tokens, b->cols_out, 4 * n_out, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (stats) *stats = st;
    return Q3_OK;
}

}  // extern "C"
