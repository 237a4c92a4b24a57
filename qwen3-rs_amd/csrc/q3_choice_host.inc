// q3_choice_host.inc -- host side of the choice logits (include/qwen3_hip.h section 2k; included by q3_engine.hip behind
// q3_embed_host.inc, same translation unit).
//
// The walk is q3_embed_many's (embed_walk, q3_embed_host.inc): the same waves, blocks, runs and row table, the same plans.  Behind
// each block k_choice_rows (q3_choice.h) computes, for every prompt that ends in it, the classifier's rows of its candidates.

extern "C" {

int q3_choice_many(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, size_t n_requests, const int32_t* cand, size_t k, uint32_t flags,
                   float* out, q3_embed_stats* stats) {
    g_err[0] = 0;
    if (stats) *stats = q3_embed_stats{0, 0, 0, 0};
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    int rc;
    if ((rc = cols_prepare(e, "q3_choice_many", true))) return rc;
    BatchCtx* b = e->batch;
    if (!prompts || !prompt_len || !out || n_requests == 0) return fail(Q3_ERR_ARG, "null or empty request list");
    if (flags & ~(uint32_t)(Q3_CHOICE_PREFIX | Q3_CHOICE_PER_REQUEST)) return fail(Q3_ERR_ARG, "unknown flag bits 0x%x", flags);
    if (!cand) return fail(Q3_ERR_ARG, "null candidate list");
    if (k == 0 || k > (size_t)Q3_CHOICE_MAX) return fail(Q3_ERR_ARG, "k %zu out of range (1..%d)", k, Q3_CHOICE_MAX);
    if (n_requests > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 requests in one call");
    const bool per_request = (flags & Q3_CHOICE_PER_REQUEST) != 0;
    const size_t n_cand = per_request ? n_requests * k : k, n_out = n_requests * k;
    for (size_t i = 0; i < n_cand; ++i)
        if (cand[i] < 0 || cand[i] >= e->cfg.vocab_size)
            return fail(Q3_ERR_ARG, "index out of range: candidate %d (vocab_size %d)", cand[i], e->cfg.vocab_size);
    const int dim = e->cfg.dim, G = e->cfg.group_size;
    if (dim > 4 * kWG * kProSlots)
        return fail(Q3_ERR_UNSUPPORTED, "q3_choice_many: dim %d exceeds the %d elements the RMSNorm prologue holds", dim, 4 * kWG * kProSlots);

    ChoiceArgs a{};
    a.norm_w = e->rms_final;
    a.wq = e->wcls.q;
    a.ws = e->wcls.s;
    a.cand_stride = per_request ? (long long)k : 0;
    a.n = dim;
    a.group = G;
    a.k = (int)k;
    const size_t smem = choice_smem_bytes(dim, G);
    const unsigned parts = (unsigned)((k + kChoicePart - 1) / kChoicePart);
    q3_embed_stats st;
    if ((rc = embed_walk(e, prompts, prompt_len, n_requests, (flags & Q3_CHOICE_PREFIX) != 0,
                         [&](const std::vector<DenseRun>&, const std::vector<EmbedStep>&) {
                             int rc2;
                             if ((rc2 = b->choice_cand.grow(n_cand, e->stream))) return rc2;
                             if ((rc2 = b->choice_out.grow(n_out, e->stream))) return rc2;
                             HIP_TRY(hipMemcpyAsync(b->choice_cand, cand, 4 * n_cand, hipMemcpyHostToDevice, e->stream));
                             a.cand = b->choice_cand;
                             a.out = b->choice_out;
                             return (int)Q3_OK;
                         },
                         [&](const EmbedRow* rows, size_t n_rows, const float* x, size_t) {
                             a.rows = rows;
                             a.x = x;
                             return launch_now(e->stream, k_choice_rows, dim3((unsigned)n_rows, parts), dim3(kWG), smem, a);
                         }, st)))
        return rc;
    // one copy back, one synchronisation
    HIP_TRY(hipMemcpyAsync(out, b->choice_out, 4 * n_out, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (stats) *stats = st;
    return Q3_OK;
}

}  // extern "C"
