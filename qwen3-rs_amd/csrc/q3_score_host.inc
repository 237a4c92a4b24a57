// q3_score_host.inc -- host side of the scores (include/qwen3_hip.h sections 2l and 2m; included by q3_engine.hip behind
// q3_choice_host.inc, same translation unit).
//
// The walk is q3_embed_many's (embed_walk, q3_embed_host.inc): the same waves, blocks, runs and plans.  Behind each block its scored
// columns go through the classifier of a kept column plan, up to 32 at a time, between k_score_gather and k_score_exp / k_score_sum
// (q3_score.h).  What the two classifier launches read: k_bquant<PRO_NORM> (and k_bquant_split) forms a pointer into the column
// states and reads it for PRO_EMBED_NORM only; k_bgemm reads State::pos and the slot table in its QKV epilogue only.  Neither
// consults per-column state for the classifier, so none is set up here.
// q3_score_many and q3_score_top_many are one body (score_run): with k > 0 every chunk runs k_score_top_part and k_score_top_merge
// (q3_score_top.h) behind k_score_sum, over the same rows; with k == 0 nothing of that is allocated, enqueued or copied.
// The launches behind the classifier and the scratch they work on are record_launches and record_scratch / record_args
// (q3_plan_host.inc), which the plans with records of the q3_generate_many_* loops use as well; here the rows are the call's table
// (TableRows, q3_score.h).

namespace {

// a chunk of a block: rows [row0, row0 + m) of the call's table, 1 <= m <= kScoreCols
struct ScoreChunk {
    size_t row0;
    int m;
    bool identity;      // column j of the block is row j of the chunk
};

// Q3_DEBUG_TIMING: event pairs around the launch groups of every chunk (gather | classifier | exps | sum and record, and with the
// k best | the selection), summed and printed to stderr behind the call's synchronisation.  Off: no event is made or recorded.
struct ScoreTiming {
    bool on = false;
    bool top = false;                   // a fifth group
    std::vector<hipEvent_t> ev;         // five per chunk, six with the k best
    ~ScoreTiming() {
        for (hipEvent_t x : ev) (void)hipEventDestroy(x);
    }
    int mark(hipStream_t st) {
        if (!on) return Q3_OK;
        hipEvent_t x;
        HIP_TRY(hipEventCreate(&x));
        ev.push_back(x);
        HIP_TRY(hipEventRecord(x, st));
        return Q3_OK;
    }
    void report() const {
        const size_t per = top ? 6 : 5;
        if (!on || ev.size() < per) return;
        double us[5] = {0, 0, 0, 0, 0};
        for (size_t c = 0; c + per <= ev.size(); c += per)
            for (size_t g = 0; g + 1 < per; ++g) {
                float ms = 0.0f;
                if (hipEventElapsedTime(&ms, ev[c + g], ev[c + g + 1]) == hipSuccess) us[g] += 1e3 * ms;
            }
        const double n = (double)(ev.size() / per);
        if (top)
            fprintf(stderr, "[q3_score_top_many] %zu chunks, us per chunk: gather %.2f classifier %.2f exp %.2f sum %.2f top %.2f\n", ev.size() / per,
                    us[0] / n, us[1] / n, us[2] / n, us[3] / n, us[4] / n);
        else
            fprintf(stderr, "[q3_score_many] %zu chunks, us per chunk: gather %.2f classifier %.2f exp %.2f sum %.2f\n", ev.size() / per, us[0] / n,
                    us[1] / n, us[2] / n, us[3] / n);
    }
};

// is token i of a request of n tokens scored, with score_from sf?  It has a successor, and that successor is at or behind sf
inline bool score_live(size_t i, size_t n, size_t sf) { return i + 1 < n && i + 1 >= sf; }

// the arguments q3_score_many and q3_score_pack check alike; n_rec: the records of the call
int score_check(const size_t* prompt_len, size_t n_requests, const size_t* score_from, size_t& n_rec) {
    if (!prompt_len || n_requests == 0) return fail(Q3_ERR_ARG, "null or empty request list");
    if (n_requests > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 requests in one call");
    size_t n_tok = 0;
    n_rec = 0;
    for (size_t r = 0; r < n_requests; ++r) {
        const size_t n = prompt_len[r], sf = score_from ? score_from[r] : 1;
        if (n == 0) return fail(Q3_ERR_ARG, "request %zu: empty prompt", r);
        if (sf < 1 || sf > n) return fail(Q3_ERR_ARG, "request %zu: score_from %zu out of range (1..%zu)", r, sf, n);
        n_tok += n;
        if (n_tok > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 tokens in one call");
        n_rec += n - sf;
    }
    return Q3_OK;
}

}  // namespace

extern "C" {

int q3_score_pack(const size_t* prompt_len, size_t n_requests, const size_t* score_from, int max_streams, int block_cap, q3_score_stats* stats) {
    g_err[0] = 0;
    if (stats) *stats = q3_score_stats{0, 0, 0, 0, 0, 0};
    int rc;
    size_t n_rec;
    if ((rc = score_check(prompt_len, n_requests, score_from, n_rec))) return rc;
    if (max_streams < 1 || max_streams > kMaxStreams) return fail(Q3_ERR_ARG, "max_streams %d out of range (1..%d)", max_streams, kMaxStreams);
    if ((rc = dense_pack_check(prompt_len, n_requests, block_cap))) return rc;
    q3_score_stats st{0, 0, 0, 0, 0, 0};
    const size_t S = (size_t)max_streams;
    for (size_t w0 = 0; w0 < n_requests; w0 += S) {
        const size_t nw = std::min(S, n_requests - w0);
        q3_dense_stats ds;
        uint64_t cur = 0, in_block = 0;
        auto close = [&] {
            st.chunks += (in_block + kScoreCols - 1) / kScoreCols;
            in_block = 0;
        };
        dense_pack_run(prompt_len + w0, nw, block_cap, [&](uint64_t block, int, size_t run, size_t off, int len) {
            if (block != cur) { close(); cur = block; }
            const size_t r = w0 + run, n = prompt_len[r], sf = score_from ? score_from[r] : 1;
            for (int k = 0; k < len; ++k) in_block += score_live(off + (size_t)k, n, sf) ? 1 : 0;
        }, ds);
        close();
        st.waves++;
        st.blocks += ds.blocks;
        st.live_columns += ds.live_columns;
        st.pad_columns += ds.pad_columns;
    }
    st.scored = n_rec;
    if (stats) *stats = st;
    return Q3_OK;
}

}  // extern "C"

namespace {

// the slices per row of k_score_top_part: kScoreTopParts; in the developer build Q3_SCORE_TOP_PARTS (1 .. 64) as every call reads
// it.  The results do not depend on it (keys are distinct integers); the time does, and fewer parts walk a slice in several tiles.
int score_top_parts() {
    const int v = dev_knob("Q3_SCORE_TOP_PARTS", kScoreTopParts);
    return v >= 1 && v <= kScoreTopParts ? v : kScoreTopParts;
}

// The body of q3_score_many (k == 0: top and rank are not looked at, and nothing of section 2m is allocated, enqueued or copied)
// and of q3_score_top_many (1 <= k <= kScoreTopMax, the caller's check).  e is not null.
int score_run(q3_engine* e, const char* who, const int32_t* prompts, const size_t* prompt_len, size_t n_requests, const size_t* score_from,
              uint32_t flags, int k, q3_score_rec* out, q3_score_top* top, int32_t* rank, q3_score_stats* stats) {
    static_assert(sizeof(ScoreRec) == sizeof(q3_score_rec) && offsetof(ScoreRec, argmax) == offsetof(q3_score_rec, argmax), "the device record is the header's");
    static_assert(sizeof(ScoreTop) == sizeof(q3_score_top) && offsetof(ScoreTop, index) == offsetof(q3_score_top, index), "the device pair is the header's");
    static_assert(kScoreTopMax == Q3_SCORE_TOP_MAX && kScoreTopMax <= 64 && kScoreTopParts <= 64, "a lane of the merge per list and per winner");
    int rc;
    if ((rc = cols_prepare(e, who, true))) return rc;
    BatchCtx* b = e->batch;
    if (!prompts || !prompt_len || n_requests == 0) return fail(Q3_ERR_ARG, "null or empty request list");
    if (flags & ~(uint32_t)Q3_SCORE_PREFIX) return fail(Q3_ERR_ARG, "unknown flag bits 0x%x", flags);
    size_t n_rec;
    if ((rc = score_check(prompt_len, n_requests, score_from, n_rec))) return rc;
    if (n_rec && !out) return fail(Q3_ERR_ARG, "null output for %zu records", n_rec);

    const int dim = e->cfg.dim, V = e->cfg.vocab_size;
    if (k > V) return fail(Q3_ERR_ARG, "k %d exceeds vocab_size %d", k, V);
    if (k && n_rec && !top) return fail(Q3_ERR_ARG, "null top for %zu records", n_rec);
    const int parts = score_top_parts();
    const size_t n_top = k ? n_rec * (size_t)k : 0, n_rank = k && rank ? n_rec : 0;
    std::vector<ScoreRow> rows;
    std::vector<ScoreChunk> chunks;
    std::vector<size_t> step_chunk0;            // chunks [step_chunk0[i], step_chunk0[i + 1]) are block i's
    Plan* plans[kColsNW] = {nullptr};
    RecordArgs args[kColsNW];                   // of the record launches behind plans[w]'s classifier
    q3_embed_stats st;
    ScoreTiming tm;
    tm.on = getenv("Q3_DEBUG_TIMING") != nullptr;
    tm.top = k > 0;
    rc = embed_walk(e, prompts, prompt_len, n_requests, (flags & Q3_SCORE_PREFIX) != 0,
                    [&](const std::vector<DenseRun>& runs, const std::vector<EmbedStep>& steps) {
                        // the record of every token of the call (-1: not scored); the walk has checked the lengths and the tokens
                        std::vector<int32_t> rec_of;
                        int32_t next = 0;
                        for (size_t r = 0; r < n_requests; ++r) {
                            const size_t n = prompt_len[r], sf = score_from ? score_from[r] : 1;
                            for (size_t i = 0; i < n; ++i) rec_of.push_back(score_live(i, n, sf) ? next++ : -1);
                        }
                        // the table: block after block, the scored columns in column order, cut into chunks
                        rows.reserve(n_rec);
                        bool width_used[kColsNW] = {false};
                        for (const EmbedStep& s : steps) {
                            step_chunk0.push_back(chunks.size());
                            const size_t first = rows.size();
                            for (size_t q = s.r0; q < s.r0 + s.nr; ++q)
                                for (int k = 0; k < runs[q].len; ++k) {
                                    const size_t g = (size_t)runs[q].src0 + (size_t)k;
                                    if (rec_of[g] < 0) continue;
                                    const ScoreRow R{runs[q].col0 + k, rec_of[g], prompts[g + 1]};
                                    if (R.col < 0 || R.col >= s.n || (size_t)R.out >= n_rec || R.target < 0 || R.target >= V)
                                        return fail(Q3_ERR_INTERNAL, "%s: table entry {%d, %d, %d} out of range", who, R.col, R.out, R.target);
                                    rows.push_back(R);
                                }
                            for (size_t r0 = first; r0 < rows.size(); r0 += kScoreCols) {
                                ScoreChunk c{r0, (int)std::min<size_t>(kScoreCols, rows.size() - r0), true};
                                for (int j = 0; j < c.m; ++j) c.identity = c.identity && rows[r0 + (size_t)j].col == j;
                                chunks.push_back(c);
                                width_used[cols_width_index(c.m)] = true;
                            }
                        }
                        step_chunk0.push_back(chunks.size());
                        if (rows.size() != n_rec) return fail(Q3_ERR_INTERNAL, "%s: %zu table rows for %zu records", who, rows.size(), n_rec);
                        // the column plans whose classifier the chunks run, kept as the walk's own are
                        int rc2;
                        if ((rc2 = record_scratch(e, k > 0))) return rc2;
                        for (int w = 0; w < kColsNW; ++w) {
                            if (!width_used[w]) continue;
                            if ((rc2 = plan_get(e, cols_key(kColsWidths[w], false), &plans[w]))) return rc2;
                            if (plans[w]->launches.size() < plans[w]->head + 2) return fail(Q3_ERR_INTERNAL, "%s: a column plan without a classifier", who);
                            // one argmax key per workgroup of the classifier launch
                            if ((rc2 = record_args(e, k > 0, (int)plans[w]->launches[plans[w]->head + 1].grid.x, parts, args[w]))) return rc2;
                        }
                        if ((rc2 = b->score_rows.grow(n_rec, e->stream))) return rc2;
                        if ((rc2 = b->score_out.grow(n_rec, e->stream))) return rc2;
                        if ((rc2 = b->score_top.grow(n_top, e->stream))) return rc2;
                        if ((rc2 = b->score_rank.grow(n_rank, e->stream))) return rc2;
                        if (n_rec) HIP_TRY(hipMemcpyAsync(b->score_rows, rows.data(), sizeof(ScoreRow) * n_rec, hipMemcpyHostToDevice, e->stream));
                        return (int)Q3_OK;
                    },
                    [&](const EmbedRow*, size_t, const float* x, size_t i) {
                        int rc2;
                        for (size_t ci = step_chunk0[i]; ci < step_chunk0[i + 1]; ++ci) {
                            const ScoreChunk& c = chunks[ci];
                            const int wi = cols_width_index(c.m), width = kColsWidths[wi];
                            const Plan& p = *plans[wi];
                            const ScoreRow* tab = b->score_rows + c.row0;
                            if ((rc2 = tm.mark(e->stream))) return rc2;
                            // a block of 32 columns or fewer already stands in b->x: nothing to move when column j is row j
                            if (!(x == b->x && c.identity) &&
                                (rc2 = launch_now(e->stream, k_score_gather, dim3((unsigned)((dim / 4 + kScoreGatherT - 1) / kScoreGatherT)), dim3(kScoreGatherT), 0,
                                                  tab, c.m, width, x, b->x, dim)))
                                return rc2;
                            if ((rc2 = tm.mark(e->stream))) return rc2;
                            if ((rc2 = plan_enqueue_range(e, p, p.head, p.head + 2))) return rc2;
                            if ((rc2 = tm.mark(e->stream))) return rc2;
                            const TableRows src{tab, b->score_out, b->score_top, rank ? (int*)b->score_rank : nullptr, k};
                            if ((rc2 = record_launches(args[wi], src, c.m, [&](bool ends_group, auto kernel, dim3 grid, dim3 blk, const RecordArgs& a, const TableRows& s) {
                                    const int rc3 = launch_now(e->stream, kernel, grid, blk, 0, a, s);
                                    return rc3 || !ends_group ? rc3 : tm.mark(e->stream);
                                })))
                                return rc2;
                        }
                        return (int)Q3_OK;
                    }, st, true);
    if (rc) return rc;
    // the copies back, one synchronisation
    if (n_rec) HIP_TRY(hipMemcpyAsync(out, b->score_out, sizeof(ScoreRec) * n_rec, hipMemcpyDeviceToHost, e->stream));
    if (n_top) HIP_TRY(hipMemcpyAsync(top, b->score_top, sizeof(ScoreTop) * n_top, hipMemcpyDeviceToHost, e->stream));
    if (n_rank) HIP_TRY(hipMemcpyAsync(rank, b->score_rank, sizeof(int32_t) * n_rank, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    tm.report();
    if (stats) *stats = q3_score_stats{st.waves, st.blocks, st.live_columns, st.pad_columns, (uint64_t)chunks.size(), (uint64_t)n_rec};
    return Q3_OK;
}

}  // namespace

extern "C" {

int q3_score_many(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, size_t n_requests, const size_t* score_from, uint32_t flags,
                  q3_score_rec* out, q3_score_stats* stats) {
    g_err[0] = 0;
    if (stats) *stats = q3_score_stats{0, 0, 0, 0, 0, 0};
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    return score_run(e, "q3_score_many", prompts, prompt_len, n_requests, score_from, flags, 0, out, nullptr, nullptr, stats);
}

int q3_score_top_many(q3_engine* e, const int32_t* prompts, const size_t* prompt_len, size_t n_requests, const size_t* score_from, uint32_t flags, int k,
                      q3_score_rec* out, q3_score_top* top, int32_t* rank, q3_score_stats* stats) {
    g_err[0] = 0;
    if (stats) *stats = q3_score_stats{0, 0, 0, 0, 0, 0};
    if (k < 1 || k > Q3_SCORE_TOP_MAX) return fail(Q3_ERR_ARG, "k %d out of range (1..%d)", k, Q3_SCORE_TOP_MAX);
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    return score_run(e, "q3_score_top_many", prompts, prompt_len, n_requests, score_from, flags, k, out, top, rank, stats);
}

}  // extern "C"
