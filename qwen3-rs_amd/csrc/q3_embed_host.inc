// q3_embed_host.inc -- host side of the embeddings (include/qwen3_hip.h section 2j; included by q3_engine.hip behind
// q3_prefix_host.inc, same translation unit).
//
// The prompts of a call go through the slots of the batched state in waves of max_streams, every wave packed into blocks by the
// rule of q3_dense_pack.  A block runs the layers and nothing behind them: a wide one is the kept PlanKind::SlotPrefill plan of
// its width (q3_dense_host.inc), one of 32 columns or fewer the launches [0, Plan::head) of the kept column plan that holds
// its live columns, with the states and the slot table written by k_dense_states as for a wide block.  Behind each block
// k_embed_rows (q3_embed.h) turns the residuals of the prompts that end in it into their output rows.
// The walk itself is embed_walk, which takes the launch behind a block as a callable: q3_choice_many (q3_choice_host.inc) runs the
// same walk with k_choice_rows in that place, q3_score_many (q3_score_host.inc) with the classifier chunks of a block's scored columns.

namespace {

// n: the columns of a wide block, pads included; the live columns of a narrow one, which stand side by side from column 0
struct EmbedStep { bool wide; int n; size_t r0, nr, g0, ng; };

// The walk q3_embed_many and q3_choice_many (q3_choice_host.inc) share: the lengths become waves, blocks, runs and a row table; the
// plans and the buffers of the walk are made; the prompts and tables go up, the prefix rows into the slots, and block after block is
// enqueued, each followed by the caller's tail launch.  Nothing is copied back and nothing is waited for: that is the caller's.
//   grow(runs, steps): called once, behind the walk's own allocations and in front of the first enqueue: the caller's buffers and
//                          uploads (a buffer that re-allocates waits for the stream itself: DevMem::grow).  It sees the schedule:
//                          steps[i] is block i, runs[steps[i].r0 .. + steps[i].nr) ALL of its runs in column order (q3_score_many,
//                          q3_score_host.inc, makes its table of scored columns from them)
//   tail(rows, n_rows, x, i): the rows {column, request} of the prompts that end in block i, just enqueued (device table), and the
//                          block's residuals x[column][dim]: enqueue the kernel that reads them.  Called for a block in which a
//                          prompt ends (n_rows > 0); with every_block, for every block
// st: the schedule's stats, valid when the walk returns Q3_OK.
template <class Grow, class Tail>
int embed_walk(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, size_t n_requests, bool use_prefix, Grow grow, Tail tail,
               q3_embed_stats& st, bool every_block = false) {
    BatchCtx* b = e->batch;
    int rc;
    st = q3_embed_stats{0, 0, 0, 0};
    const size_t P = use_prefix ? b->prefix_n : 0;
    if (use_prefix && P == 0) return fail(Q3_ERR_ARG, "no prefix is resident: call q3_batch_prefix_set first");
    if (n_requests > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 requests in one call");
    std::vector<size_t> off(n_requests);
    size_t n_tok = 0;
    for (size_t r = 0; r < n_requests; ++r) {
        if (prompt_len[r] == 0) return fail(Q3_ERR_ARG, "request %zu: empty prompt", r);
        if (prompt_len[r] > (size_t)b->ctx || P + prompt_len[r] > (size_t)b->ctx)
            return fail(Q3_ERR_ARG, "request %zu: prompt of %zu tokens exceeds seq_len %d", r, P + prompt_len[r], b->ctx);
        off[r] = n_tok;
        n_tok += prompt_len[r];
        if (n_tok > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 tokens in one call");
    }
    for (size_t i = 0; i < n_tok; ++i)
        if (prompts[i] < 0 || prompts[i] >= e->cfg.vocab_size)
            return fail(Q3_ERR_ARG, "index out of range: token %d (vocab_size %d)", prompts[i], e->cfg.vocab_size);

    // the schedule, a pure function of the lengths: wave w holds requests [w S, (w + 1) S), its i-th request in slot i from position P
    const size_t S = (size_t)b->max_streams;
    const int cap = dense_block_cap(e);
    std::vector<DenseRun> runs;
    std::vector<EmbedRow> rows;
    std::vector<EmbedStep> steps;
    size_t max_end = 0;
    bool width_used[kColsNW] = {false};
    for (size_t w0 = 0; w0 < n_requests; w0 += S) {
        const size_t nw = std::min(S, n_requests - w0);
        const DenseBlocks db = dense_blocks(prompt_len + w0, nw, cap);
        st.waves++;
        st.blocks += db.stats.blocks;
        st.live_columns += db.stats.live_columns;
        st.pad_columns += db.stats.pad_columns;
        for (const DenseBlock& bl : db.blocks) {
            EmbedStep s{bl.wide, bl.n, runs.size(), bl.np, rows.size(), 0};
            int col = 0;
            for (size_t i = bl.p0; i < bl.p0 + bl.np; ++i) {
                const DensePiece& pc = db.pieces[i];
                const size_t r = w0 + pc.run;
                const int c0 = s.wide ? pc.col0 : col;
                runs.push_back(DenseRun{c0, (int)pc.run, (int)(P + pc.off), (int)(off[r] + pc.off), pc.len});
                if (s.wide) max_end = std::max(max_end, P + pc.off + (size_t)pc.len);
                // a run whose last piece lies in a later block has no row here
                if (pc.off + (size_t)pc.len == prompt_len[r]) rows.push_back(EmbedRow{c0 + pc.len - 1, (int)r});
                col += pc.len;
            }
            if (!s.wide) {
                s.n = col;
                width_used[cols_width_index(col)] = true;
            }
            s.ng = rows.size() - s.g0;
            steps.push_back(s);
        }
    }

    // every plan and buffer the call needs exists before the first launch is enqueued; a shape the kernels refuse ends here
    Plan* plans[kColsNW] = {nullptr};
    for (int w = 0; w < kColsNW; ++w)
        if (width_used[w] && (rc = plan_get(e, cols_key(kColsWidths[w], false), &plans[w]))) return rc;
    std::vector<Plan*> wide_plans(steps.size(), nullptr);
    if (max_end) {
        if ((rc = dense_scratch_get(e))) return rc;
        if ((rc = dense_att_grow(e, max_end))) return rc;
        for (size_t i = 0; i < steps.size(); ++i)
            if (steps[i].wide && (rc = plan_get(e, PlanKey{PlanKind::SlotPrefill, steps[i].n, false}, &wide_plans[i]))) return rc;
    }
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = b->cols_prompts.grow(n_tok, e->stream))) return rc;
    if ((rc = b->dense_runs.grow(runs.size(), e->stream))) return rc;
    if ((rc = b->embed_rows.grow(rows.size(), e->stream))) return rc;
    if ((rc = grow(runs, steps))) return rc;

    // the call on the stream: three uploads, the prefix rows, block after block with its tail
    HIP_TRY(hipMemcpyAsync(b->cols_prompts, prompts, 4 * n_tok, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(b->dense_runs, runs.data(), sizeof(DenseRun) * runs.size(), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(b->embed_rows, rows.data(), sizeof(EmbedRow) * rows.size(), hipMemcpyHostToDevice, e->stream));
    if (P && (rc = prefix_bcast_slots(e, (int)std::min(n_requests, S)))) return rc;
    for (size_t i = 0; i < steps.size(); ++i) {
        const EmbedStep& s = steps[i];
        const float* x = nullptr;
        if (s.wide) {
            if ((rc = dense_enqueue_block(e, *wide_plans[i], b->dense_runs + s.r0, (int)s.nr, s.n, b->cols_prompts))) return rc;
            x = b->dense.x;
        } else {
            // the layers of the column plan and nothing behind them: no classifier, no turn kernel.  The plan's columns past the
            // live ones repeat the last live column, as k_dense_states lays out the columns behind a block's last run
            const int wi = cols_width_index(s.n);
            hipLaunchKernelGGL(k_dense_states, dim3(1), dim3(256), 0, e->stream, b->st, b->col_slot, (const DenseRun*)(b->dense_runs + s.r0), (int)s.nr,
                               (const int32_t*)b->cols_prompts, kColsWidths[wi]);
            if ((rc = plan_enqueue(e, *plans[wi], plans[wi]->head))) return rc;
            x = b->x;
        }
        if ((s.ng || every_block) && (rc = tail((const EmbedRow*)(b->embed_rows + s.g0), s.ng, x, i))) return rc;
    }
    HIP_TRY(hipGetLastError());
    return Q3_OK;
}

}  // namespace

extern "C" {

int q3_embed_many(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, size_t n_requests, uint32_t flags, size_t out_dim, float* out,
                  q3_embed_stats* stats) {
    g_err[0] = 0;
    if (stats) *stats = q3_embed_stats{0, 0, 0, 0};
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    int rc;
    if ((rc = cols_prepare(e, "q3_embed_many", true))) return rc;
    BatchCtx* b = e->batch;
    if (!prompts || !prompt_len || !out || n_requests == 0) return fail(Q3_ERR_ARG, "null or empty request list");
    if (flags & ~(uint32_t)(Q3_EMBED_L2 | Q3_EMBED_PREFIX)) return fail(Q3_ERR_ARG, "unknown flag bits 0x%x", flags);
    const size_t dim = (size_t)e->cfg.dim;
    if (out_dim > dim) return fail(Q3_ERR_ARG, "out_dim %zu exceeds dim %zu", out_dim, dim);
    if (out_dim == 0) out_dim = dim;
    const size_t n_out = n_requests * out_dim;
    const size_t smem = 4 * (size_t)term_floats((int)dim);
    q3_embed_stats st;
    if ((rc = embed_walk(e, prompts, prompt_len, n_requests, (flags & Q3_EMBED_PREFIX) != 0,
                         [&](const std::vector<DenseRun>&, const std::vector<EmbedStep>&) { return b->embed_out.grow(n_out, e->stream); },
                         [&](const EmbedRow* rows, size_t n_rows, const float* x, size_t) {
                             return launch_now(e->stream, k_embed_rows, dim3((unsigned)n_rows), dim3(kWG), smem, rows, x, (const float*)e->rms_final,
                                               (int)dim, (int)out_dim, (flags & Q3_EMBED_L2) ? kEmbedL2 : 0u, b->embed_out);
                         }, st)))
        return rc;
    // one copy back, one synchronisation
    HIP_TRY(hipMemcpyAsync(out, b->embed_out, 4 * n_out, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (stats) *stats = st;
    return Q3_OK;
}

}  // extern "C"
