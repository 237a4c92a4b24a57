// q3_prefix_host.inc -- host side of the shared prompt prefix (include/qwen3_hip.h section 2i; included by q3_engine.hip behind
// q3_stop_host.inc, same translation unit).
//
// A prefix that many requests share is prefilled once (q3_batch_prefix_set), kept in a store beside the per-stream caches, and copied
// into rows 0 .. P - 1 of the slots a loop call can use by ONE launch of k_kv_rows_bcast (q3_prefix.h) in front of its first pass.
// The loops are the kept ones with every position moved up by P (cols_generate / cols_generate_stop, ColsRequests::pos_base): the attention
// kernels read the copied rows as they read any other row of the slot.

namespace {

// Rows of n_rows positions of every layer of both caches, from one source block to n_dst destination blocks, one launch on the
// engine's stream.  The pointers are those of the first copied row of layer 0; strides in floats.
int kv_rows_bcast(q3_engine* e, const float* src_key, const float* src_value, size_t src_layer_stride, const KvBcastDst& dst, int n_dst,
                  size_t dst_layer_stride, size_t n_rows) {
    const q3_config& c = e->cfg;
    const size_t kvd = (size_t)c.n_kv_heads * c.head_dim, run = n_rows * kvd;
    const bool wide = kvd % 4 == 0;                          // every shape batch_alloc accepts (kv_dim % 16 == 0)
    const size_t n = wide ? run / 4 : run;                   // accesses per layer and cache
    // the grid follows the bytes to move, not n_dst: 8 workgroups per CU over all layers of both caches, kBcastUnroll accesses a thread
    const size_t rows_y = 2 * (size_t)c.n_layers;
    const size_t want_x = (n + (size_t)kWG * kBcastUnroll - 1) / ((size_t)kWG * kBcastUnroll);
    const size_t cap_x = (8 * (size_t)e->n_cu + rows_y - 1) / rows_y;
    const dim3 grid((unsigned)std::max<size_t>(1, std::min(want_x, cap_x)), (unsigned)rows_y);
    // launched directly: the by-value table makes the arguments larger than a plan's launch record
    if (wide)
        hipLaunchKernelGGL(k_kv_rows_bcast<v4u>, grid, dim3(kWG), 0, e->stream, src_key, src_value, src_layer_stride, dst, n_dst, dst_layer_stride,
                           c.n_layers, run);
    else
        hipLaunchKernelGGL(k_kv_rows_bcast<unsigned>, grid, dim3(kWG), 0, e->stream, src_key, src_value, src_layer_stride, dst, n_dst, dst_layer_stride,
                           c.n_layers, run);
    HIP_TRY(hipGetLastError());
    return Q3_OK;
}

int prefix_bcast_slots(q3_engine* e, int n_slots) {
    BatchCtx* b = e->batch;
    const size_t kvd = (size_t)e->cfg.n_kv_heads * e->cfg.head_dim, P = b->prefix_n;
    if (!b->prefix_store || P == 0 || n_slots < 1 || n_slots > b->max_streams) return fail(Q3_ERR_INTERNAL, "no resident prefix to copy into %d slots", n_slots);
    KvBcastDst dst{};
    for (int i = 0; i < n_slots; ++i) {
        dst.key[i] = b->key + (size_t)i * b->kv_stream;
        dst.value[i] = b->value + (size_t)i * b->kv_stream;
    }
    const float* sk = b->prefix_store;
    return kv_rows_bcast(e, sk, sk + (size_t)e->cfg.n_layers * P * kvd, P * kvd, dst, n_slots, (size_t)b->ctx * kvd, P);
}

void prefix_release(q3_engine* e) {
    BatchCtx* b = e->batch;
    b->prefix_store.reset();
    b->prefix_n = 0;
    b->prefix_tokens.clear();
}

// one xorshift64* state step per coin (sampler.rs:44-49): what k_rng_skip does on the device
uint64_t rng_skip(uint64_t rs, size_t coins) {
    for (size_t i = 0; i < coins; ++i) {
        rs ^= rs >> 12;
        rs ^= rs << 25;
        rs ^= rs >> 27;
    }
    return rs;
}

}  // namespace

extern "C" {

int q3_batch_copy_rows(q3_engine* e, int src_slot, const int32_t* dst_slots, int n_dst, size_t first_pos, size_t n_rows) {
    g_err[0] = 0;
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    BatchCtx* b = e->batch;
    if (!b || !b->has_kv) return fail(Q3_ERR_ARG, "q3_batch_init has not been called");
    if (!dst_slots) return fail(Q3_ERR_ARG, "null argument");
    if (n_dst < 1 || n_dst > b->max_streams - 1) return fail(Q3_ERR_ARG, "n_dst %d out of range (1..%d)", n_dst, b->max_streams - 1);
    if (src_slot < 0 || src_slot >= b->max_streams) return fail(Q3_ERR_ARG, "source slot %d out of range (0..%d)", src_slot, b->max_streams - 1);
    bool seen[kMaxStreams] = {false};
    for (int i = 0; i < n_dst; ++i) {
        const int s = dst_slots[i];
        if (s < 0 || s >= b->max_streams) return fail(Q3_ERR_ARG, "destination %d: slot %d out of range (0..%d)", i, s, b->max_streams - 1);
        if (s == src_slot) return fail(Q3_ERR_ARG, "destination %d: slot %d is the source", i, s);
        if (seen[s]) return fail(Q3_ERR_ARG, "destination %d: slot %d is named twice", i, s);
        seen[s] = true;
    }
    if (n_rows == 0) return fail(Q3_ERR_ARG, "no row to copy");
    if (first_pos >= (size_t)b->ctx || n_rows > (size_t)b->ctx - first_pos)
        return fail(Q3_ERR_ARG, "rows %zu .. %zu + %zu exceed seq_len %d", first_pos, first_pos, n_rows, b->ctx);
    const size_t kvd = (size_t)e->cfg.n_kv_heads * e->cfg.head_dim, at = first_pos * kvd;
    KvBcastDst dst{};
    for (int i = 0; i < n_dst; ++i) {
        dst.key[i] = b->key + (size_t)dst_slots[i] * b->kv_stream + at;
        dst.value[i] = b->value + (size_t)dst_slots[i] * b->kv_stream + at;
    }
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = kv_rows_bcast(e, b->key + (size_t)src_slot * b->kv_stream + at, b->value + (size_t)src_slot * b->kv_stream + at, (size_t)b->ctx * kvd, dst, n_dst,
                            (size_t)b->ctx * kvd, n_rows))) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return Q3_OK;
}

int q3_batch_prefix_set(q3_engine* e, const int32_t* tokens, size_t n) {
    g_err[0] = 0;
    int rc;
    if ((rc = cols_prepare(e, "q3_batch_prefix_set", true))) return rc;
    BatchCtx* b = e->batch;
    HIP_TRY(hipSetDevice(e->device));
    if (n == 0) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        prefix_release(e);
        return Q3_OK;
    }
    if (!tokens) return fail(Q3_ERR_ARG, "null argument");
    if (n >= (size_t)b->ctx) return fail(Q3_ERR_ARG, "a prefix of %zu tokens leaves no room in a context of %d", n, b->ctx);
    for (size_t i = 0; i < n; ++i)
        if (tokens[i] < 0 || tokens[i] >= e->cfg.vocab_size)
            return fail(Q3_ERR_ARG, "index out of range: token %d (vocab_size %d)", tokens[i], e->cfg.vocab_size);
    HIP_TRY(hipStreamSynchronize(e->stream));
    prefix_release(e);                                       // a call that fails leaves no prefix resident
    // rows 0 .. n - 1 of slot 0, by the blocks and passes of q3_batch_prefill_slots in their greedy form: no slot rng is touched,
    // whatever q3_batch_sampler_set says
    ColsJob job;
    q3_dense_stats dst{0, 0, 0};
    dense_job_add(e, job, std::vector<DenseIn>{DenseIn{0, 0, 0, n}}, false, nullptr, nullptr, nullptr, dst);
    const ColsJobSampler smp{nullptr, nullptr, nullptr, nullptr, 0, false};
    if ((rc = cols_job_run(e, job, false, smp, tokens, n, nullptr, 0))) return rc;
    // slot 0 -> the store: the same kernel, one destination whose layers are n rows apart
    const q3_config& c = e->cfg;
    const size_t kvd = (size_t)c.n_kv_heads * c.head_dim, half = (size_t)c.n_layers * n * kvd;
    DevMem<float> store;                                     // moved in once its rows have arrived
    if (store.alloc(2 * half)) {
        (void)hipGetLastError();
        return fail(Q3_ERR_HIP, "the prefix store of %zu MiB for %zu tokens does not fit", (4 * 2 * half) >> 20, n);
    }
    KvBcastDst d{};
    d.key[0] = store;
    d.value[0] = store + half;
    if ((rc = kv_rows_bcast(e, b->key, b->value, (size_t)b->ctx * kvd, d, 1, n * kvd, n)) == Q3_OK) {
        const hipError_t err = hipStreamSynchronize(e->stream);
        if (err != hipSuccess) rc = fail(Q3_ERR_HIP, "%s", hipGetErrorString(err));
    }
    if (rc) return rc;
    b->prefix_store = std::move(store);
    b->prefix_n = n;
    b->prefix_tokens.assign(tokens, tokens + n);
    return Q3_OK;
}

int q3_batch_prefix_get(const q3_engine* e, size_t* n, int32_t* tokens, size_t cap) {
    g_err[0] = 0;
    if (!e || !n) return fail(Q3_ERR_ARG, "null argument");
    const BatchCtx* b = e->batch;
    *n = b ? b->prefix_n : 0;
    if (tokens && b)
        for (size_t i = 0; i < std::min(cap, b->prefix_n); ++i) tokens[i] = b->prefix_tokens[i];
    return Q3_OK;
}

int q3_generate_many_prefix(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, const size_t* n_new, size_t n_requests,
                            const float* temperature, const float* topp, const uint64_t* seeds, const int32_t* stop_tokens, size_t n_stop,
                            int32_t* out_tokens, size_t* n_out, q3_cols_stats* stats) {
    g_err[0] = 0;
    genlp_call_enter(e);
    if (stats) *stats = q3_cols_stats{0, 0, 0, 0};
    int rc;
    ColsRequests rq;
    const bool draw = temperature || topp || seeds;
    if ((rc = cols_prepare(e, "q3_generate_many_prefix", draw))) return rc;
    const size_t P = e->batch->prefix_n;
    if (P == 0) return fail(Q3_ERR_ARG, "no prefix is resident: call q3_batch_prefix_set first");
    if (!n_out) return fail(Q3_ERR_ARG, "null argument");
    if ((rc = stop_list_check(stop_tokens, n_stop))) return rc;
    if ((rc = cols_requests_check(e, prompts, prompt_len, n_new, n_requests, draw, temperature, topp, seeds, P, out_tokens, rq))) return rc;
    // the prompt loop draws and discards one sample per prompt position (section 2f): a sampled request enters its first column
    // with its seed state P coins on.  A greedy request draws no coin
    std::vector<uint64_t> seeds_p;
    if (draw) {
        seeds_p.assign(seeds, seeds + n_requests);
        for (size_t r = 0; r < n_requests; ++r)
            if (temperature[r] > 0.0f) seeds_p[r] = rng_skip(seeds[r], P);
        rq.seeds = seeds_p.data();
    }
    if (n_stop > 0 || e->stop_seq.n_states) return cols_generate_stop(e, rq, stop_tokens, n_stop, out_tokens, n_out, stats);
    // no stop token and no stop automaton (section 2t): the tabled, device-resident loop of sections 2e / 2f
    if ((rc = cols_generate(e, rq, out_tokens, stats))) return rc;
    for (size_t r = 0; r < n_requests; ++r) n_out[r] = n_new[r];
    return Q3_OK;
}

}  // extern "C"
