// q3_batch_host.inc -- host side of the batched decode path (included by q3_engine.hip, same translation unit).
//
// B <= 32 independent streams, each with its own KV cache and (token, pos) state, advance one token per step; the
// weights are streamed once per step through the int8 matrix cores (q3_batch.h).  The caller pattern this serves is
// N concurrent `generate` loops (generation.rs:9-48) -- the reference runs them as N processes.

// what a plan is built for.  Decode: n streams, each over its own KV cache.  Prefill: n positions of one sequence over
// the engine's own KV cache, layers only (the classifier runs once, on the last position, through the single-stream launch).
// Verify: the prefill layers between k_spec_snapshot and the n-column classifier + k_spec_commit + k_spec_restore; with the
// sampler on (PlanKey::draw), the per-column draws of the batched decode and k_spec_commit_draw stand in for k_spec_commit.
// Cols: n columns of (slot, token, position) over the per-stream caches (q3_batch_step_cols): the prefill layers with the cache base
// of every column taken from the slot table, the n-column classifier and k_cols_turn.  Its plans live in BatchCtx::cols_plans.
// SlotPrefill: the dense Prefill layers over the per-stream caches, n > 32 columns of runs of several slots with a slot table as
// long as the block (q3_batch_prefill_slots), on a scratch of their own (BatchCtx::dense); no classifier.  Its plans live in
// BatchCtx::dense_plans.
enum class PlanKind { Decode, Prefill, Verify, Cols, SlotPrefill };
// n: streams, block positions or columns; grids and the stream-tile count are baked in.  draw: Verify and Cols under the sampler
// (the plan samples every column); the sampler of a Decode plan is not part of its key: q3_batch_sampler_set drops the plan.
// topk: the draws of the plan are the top-k form (q3_topk.h); plan_get sets it from the engine's top_k wherever the plan draws
// genlp: Cols plans of the q3_generate_many_* loops only (cols_key sets it from the engine's q3_gen_logprobs): kGenlpRecs, the record
// launches (record_launches, q3_plan_host.inc) stand in front of the turn kernel; kGenlpTop, the top launches behind them
// pen: Cols plans of the q3_generate_many_* loops only (cols_key sets it from the engine's q3_sampler_penalties): k_pen_apply stands
// behind the classifier, the draws and the turn kernel take the penalised rows, k_pen_count stands in front of the turn kernel
// (q3_penalty.h); the values of the setting are read from device memory when a pass runs.  kPenAdj (cols_key sets it where a table
// of q3_logit_bias_set holds, section 2q): k_bias_apply and k_bias_count (q3_bias.h) stand in their places, and whether penalties apply
// on top is read from device memory when a pass runs (kPenOff / kPenOn / kPenAdj: q3_bias.h).  kPenGuide (where a guide of q3_guide_set
// holds, section 2r, whatever the table and the penalties): k_guide_apply and k_guide_step (q3_guide.h) stand in those places.
// kPenGuideSp (where a sparse guide of q3_guide_set_sparse holds, section 2s): k_guide_sp_apply and k_guide_sp_step (q3_guide_sparse.h)
enum { kGenlpOff = 0, kGenlpRecs = 1, kGenlpTop = 2, kGenlpForms = 3 };
struct PlanKey {
    PlanKind kind = PlanKind::Decode;
    int n = 0;
    bool draw = false;
    bool topk = false;
    int genlp = kGenlpOff;
    int pen = kPenOff;
    bool operator==(const PlanKey& o) const {
        return kind == o.kind && n == o.n && draw == o.draw && topk == o.topk && genlp == o.genlp && pen == o.pen;
    }
};
// The launches of one key, built by batch_build_plan (q3_plan_host.inc): a value, moved to where its kind is kept.
struct Plan {
    std::vector<Launch> launches;
    Graph graph;                 // captured for the kinds that end in a classifier, unless Q3_FLAG_NO_GRAPH
    size_t head = 0;             // index of the first launch behind the layers (q3_embed_many launches [0, head) of a column plan alone)
};

// the per-column buffers the layers of a SlotPrefill plan work on: the dense block scratch, beside the context's own
struct BlockScratch {
    DevMem<float> x, q, qn, kraw, xb, hb;
    DevMem<int8_t> xq_p;
    DevMem<float> xs_p;
    DevMem<State> st;
    DevMem<int> col_slot;
    DevMem<float> att_pf;
    int att_pf_stride = 0;
    int cap = 0;                 // columns (0: not allocated)
};

// the plan widths of a column pass: a pass of n live columns runs the narrowest plan that holds it, padded with repeats of
// its last column
constexpr int kColsWidths[] = {1, 2, 4, 8, 16, 32};
constexpr int kColsNW = 6;
struct ColsHost {               // pinned staging of one host-made pass
    ColsCtl ctl;
    State st[kColsMax];
    int slot[kColsMax];
};
struct ColsStep {               // the one-pass table of a host-made sampled pass (q3_batch_step_cols_draw), device and pinned copy
    ColEnt table[kColsMax];
    ColAux aux[kColsMax];
    int32_t tokens[kColsMax];
    int ncols;
};
struct ColsDrawHost {           // pinned staging of the sampled passes
    ColsDraw dr;
    ColsStep step;
};

struct BatchCtx {
    int max_streams = 0, ctx = 0;
    int cap = 0;                 // columns the scratch buffers hold: max_streams, or the dense prefill block (Q3_PREFILL_M)
    DevMem<float> att_pf;        // k_attn_pf2 score rows [cap][n_heads][att_pf_stride]
    int att_pf_stride = 0;
    DevMem<int8_t> pq;           // packed weights, all matrices
    DevMem<float> ps;
    DevMem<float> qn;            // k_attn_pf2: normalised + rotated queries of the block, head pairs interleaved [cap][n_heads/2][hd][2]
    DevMem<float> x, q, kraw, xb, hb, logits;
    DevMem<float> key, value, att;
    DevMem<int8_t> xq_p;
    DevMem<float> xs_p;
    DevMem<State> st;
    DevMem<unsigned long long> slots;
    int nslots = 0;
    DevMem<unsigned long long> stamps;      // developer timeline (Q3_STAMPS=1, dev build)
    DevMem<int32_t> out_tokens;
    int out_cap = 0;
    PinMem<State> h_st;
    PinMem<int32_t> h_tokens;
    PinMem<float> h_logits;
    Plan step;                   // the one plan of Decode, Prefill and Verify: replaced whenever step_key changes (empty: none)
    PlanKey step_key;
    // draft verification (q3_verify / q3_generate_lookup)
    DevMem<SpecIO> spec_io;      // device: block input and result
    PinMem<SpecIO> h_spec;       // pinned staging of the same
    DevMem<float> spec_snap;     // key / value rows a rejected draft would leave behind, [2][layers][kSpecMax - 1][kv_dim]
    // ... under the sampler (q3_verify_draw / q3_generate_lookup_draw, and the sampled column passes): the draw site of kSpecMax
    // columns, allocated by the first sampled pass (spec_draw_alloc); draw_cols.ss are the column sampler states
    DrawSite draw_cols;
    bool has_kv = false;         // per-stream KV caches allocated (q3_batch_init); prefill-only contexts have none
    // per-stream device samplers (q3_batch_sampler_set)
    bool sampling = false;
    DrawSite draw_decode;        // max_streams columns, allocated by the first q3_batch_sampler_set; draw_decode.ss: slot i = stream i
    size_t kv_stream = 0;        // floats per stream in key / value
    // column passes (q3_batch_step_cols / q3_generate_many_greedy)
    DevMem<int> col_slot;        // device [kColsMax]: KV slot of every column of the pass in flight
    DevMem<ColsCtl> cols_ctl;    // device
    PinMem<ColsHost> h_cols;
    Plan cols_plans[kPenForms][kGenlpForms][3][kColsNW];   // [plain | under penalties | adjusted rows | masked rows | masked rows, sparse][no records | records | records and top][greedy |
                                                        // sampled | sampled with top-k][width], built on first use (q3_batch_init
                                                        // starts over); the sampled ones: the same layers and classifier, then the
                                                        // draws and k_cols_turn_draw; with records: the record launches in front of
                                                        // the turn kernel; under penalties: k_pen_apply behind the classifier and
                                                        // k_pen_count in front of the turn kernel; adjusted rows: k_bias_apply and
                                                        // k_bias_count in their places; masked rows: k_guide_apply and k_guide_step,
                                                        // or k_guide_sp_apply and k_guide_sp_step under a sparse guide
    DevMem<ColEnt> cols_table;                          // the loop's pass table, prompts and output: grow-only device buffers
    DevMem<int> cols_ncols;
    DevMem<int32_t> cols_prompts, cols_out;
    // ... under the sampler (q3_batch_step_cols_draw / q3_generate_many_sampled): allocated by the first sampled pass (cols_draw_alloc),
    // the column sampler states and the draw scratch are draw_cols'
    DevMem<ColsDraw> cols_draw;                         // device
    PinMem<ColsDrawHost> h_cols_draw;
    DevMem<ColsStep> cols_step;                         // device
    DevMem<SamplerState> cols_slot_samp;                // [kMaxStreams] the loop's per-slot states (a single pass uses draw_decode.ss)
    DevMem<ColAux> cols_aux;                            // the loop's table of ColAux and per-request sampler parameters: grow-only
    DevMem<float> cols_temp, cols_topp;
    DevMem<unsigned long long> cols_seeds;
    // ... with stop tokens (q3_generate_many_stop): the scheduler state and its one-row table, the per-request records (grow-only),
    // the pinned status word the host reads after every pass; allocated by the first call
    DevMem<ColsStopDev> cols_stop;                      // device
    PinMem<SchedStatus> h_cols_stop;
    DevMem<int> cols_req;
    // dense blocks over the per-stream caches (q3_batch_prefill_slots / q3_generate_many_dense): scratch of prefill_block_cap()
    // columns beside the 32-column one, allocated on first use; plans by block width, kept (no graph: the launches are enqueued
    // as they are, like q3_prefill_batched's); the run tables of a call, grow-only
    BlockScratch dense;
    int dense_cap = 0;           // columns per block, fixed by the first dense call (Q3_PREFILL_M as read then): packing and scratch agree
    std::map<int, Plan> dense_plans;
    DevMem<DenseRun> dense_runs;
    // the resident shared prefix (q3_batch_prefix_set): key and value rows 0 .. prefix_n - 1 of every layer, [2][n_layers][prefix_n][kv_dim],
    // beside the per-stream caches and private to section 2i; the tokens they were computed from
    DevMem<float> prefix_store;
    size_t prefix_n = 0;
    std::vector<int32_t> prefix_tokens;
    // embeddings (q3_embed_many): the gather tables of a call's blocks and its output rows [n_requests][out_dim], grow-only
    DevMem<EmbedRow> embed_rows;
    DevMem<float> embed_out;
    // choice logits (q3_choice_many): the uploaded candidate ids and the output rows [n_requests][k], grow-only
    DevMem<int32_t> choice_cand;
    DevMem<float> choice_out;
    // the scratch of the record kernels (q3_score.h), shared by the score calls and the plans with records and made by record_scratch
    // (q3_plan_host.inc) alone, on first use at its full size, never replaced while the context lives: the exps of 32 rows, and -- from
    // the first use with k > 0 on -- the parts' lists and counts of 32 rows ([32][64][64] keys, [32][64] counts)
    DevMem<float> record_exps;
    DevMem<unsigned long long> record_part_keys;
    DevMem<int> record_part_above;
    // scores (q3_score_many): the table of a call's scored columns and its records, grow-only
    DevMem<ScoreRow> score_rows;
    DevMem<ScoreRec> score_out;
    // ... with the k best (q3_score_top_many): the call's [records][k] pairs and ranks, grow-only
    DevMem<ScoreTop> score_top;
    DevMem<int> score_rank;
    // log-probabilities of generated tokens (q3_gen_logprobs, section 2o).  Allocated by genlp_alloc, once: the control block the
    // pass source of q3_genlp.h reads and its pinned copy.  Per call, grow-only: the records, tops and ranks, indexed as the call's
    // out_tokens.  genlp_valid: the last q3_generate_many_* call ran with the setting on and succeeded; it left genlp_count records
    // with genlp_top_n alternatives
    DevMem<GenlpCtl> genlp_ctl;
    PinMem<GenlpCtl> h_genlp;
    DevMem<ScoreRec> genlp_recs;
    DevMem<ScoreTop> genlp_top;
    DevMem<int> genlp_rank;
    size_t genlp_count = 0;
    int genlp_top_n = 0;
    bool genlp_valid = false;
    // presence and frequency penalties (q3_sampler_penalties, section 2p), made by pen_alloc (q3_plan_host.inc) on the first non-zero
    // setting or by the first generate call under one, never replaced while the context lives: the produced-token counts of every KV
    // slot [max_streams][V], and -- a group of their own (adj_alloc), which the adjusted rows of section 2q share and a table without
    // penalties makes alone -- the penalised rows of a pass [kColsMax][V], their slices' largest keys [kColsMax][kPenSlices] and the
    // setting as the passes read it
    DevMem<unsigned> pen_counts;
    DevMem<float> pen_logits;
    DevMem<unsigned long long> pen_slots;
    DevMem<PenCtl> pen_ctl;
    // the table of q3_logit_bias_set as the call in flight reads it (section 2q; bias_call_begin, q3_plan_host.inc): the control block
    // the plans of the adjusted form point at, made once, and behind it the grow-only buffers every generate call under a table fills
    DevMem<BiasCtl> bias_ctl;
    DevMem<BiasEntry> bias_entries;
    DevMem<unsigned> bias_off;
    DevMem<unsigned char> bias_modes;
    DevMem<int> bias_ooff;
    // the guide of q3_guide_set (section 2r; guide_alloc and guide_call_begin, q3_plan_host.inc): the control block the plans of the
    // masked form point at and the state of the request in every KV slot [max_streams], made once; the table, uploaded when
    // guide_serial is not the serial of the engine's guide (a new q3_guide_set, or this context is new); start[] of the call in flight
    DevMem<GuideCtl> guide_ctl;
    DevMem<int> guide_state;
    DevMem<short> guide_next;
    DevMem<int> guide_start;
    unsigned long long guide_serial = 0;
    // the sparse guide of q3_guide_set_sparse (section 2s; guide_sp_alloc and guide_sp_call_begin): the same, with the three arrays
    // of the compressed table in the table's place
    DevMem<GuideSpCtl> guide_sp_ctl;
    DevMem<int> guide_sp_state;
    DevMem<int> guide_sp_dflt;
    DevMem<unsigned> guide_sp_off;
    DevMem<GuideEdge> guide_sp_edges;
    DevMem<int> guide_sp_start;
    unsigned long long guide_sp_serial = 0;
    // the stop automaton of q3_stop_seq_set (section 2t; stop_seq_call_begin, q3_stop_host.inc): the control block and the slots'
    // states beside cols_stop, made once; the three arrays, uploaded when stop_seq_serial is not the serial of the engine's
    // automaton; start[] of the call in flight
    DevMem<StopSeqDev> stop_seq_dev;
    DevMem<int> stop_seq_dflt;
    DevMem<unsigned> stop_seq_off;
    DevMem<GuideEdge> stop_seq_edges;
    DevMem<int> stop_seq_start;
    unsigned long long stop_seq_serial = 0;
    // packed-matrix directory
    struct PM { size_t q_off, s_off; int ntiles, ng; };
    std::vector<PM> m_qkv, m_wo, m_w13, m_w2;
    PM m_cls{};
};

namespace {

// q3_plan_host.inc
int plan_get(q3_engine* e, PlanKey key, Plan** out);
int plan_enqueue(q3_engine* e, const Plan& p, size_t n_launches = SIZE_MAX);
int plan_enqueue_range(q3_engine* e, const Plan& p, size_t first, size_t end);
enum class PlanDrop { Step, Dense };
void plans_drop(BatchCtx* b, PlanDrop what);

// every buffer, plan and graph of the context goes with it
void batch_free(q3_engine* e) {
    delete e->batch;
    e->batch = nullptr;
}

// the states of a decode step of n streams on their way to the device, and the step's plan
int batch_set_state(q3_engine* e, const int32_t* tokens, const int32_t* pos, int n, Plan** plan) {
    BatchCtx* b = e->batch;
    if (!b || !b->has_kv) return fail(Q3_ERR_ARG, "q3_batch_init has not been called");
    if (!tokens || !pos || n <= 0 || n > b->max_streams)
        return fail(Q3_ERR_ARG, "n_streams %d out of range (1..%d)", n, b->max_streams);
    for (int i = 0; i < n; ++i) {
        if (tokens[i] < 0 || tokens[i] >= e->cfg.vocab_size || pos[i] < 0 || pos[i] >= b->ctx)
            return fail(Q3_ERR_ARG, "index out of range: stream %d token %d (vocab_size %d), pos %d (seq_len %d)", i, tokens[i],
                        e->cfg.vocab_size, pos[i], b->ctx);
        b->h_st[i].token = tokens[i];
        b->h_st[i].pos = pos[i];
        b->h_st[i].step = 0;
        b->h_st[i].prompt_len = 0;
        b->h_st[i].argmax = 0ull;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = plan_get(e, PlanKey{PlanKind::Decode, n, false}, plan)) return rc;
    HIP_TRY(hipMemcpyAsync(b->st, b->h_st, sizeof(State) * (size_t)n, hipMemcpyHostToDevice, e->stream));
    return Q3_OK;
}

// with_kv = false: prefill-only context (packed weights + per-position scratch, no per-stream KV caches)
// cap: columns the scratch buffers hold (>= max_streams; the dense prefill walks the prompt in blocks of `cap` positions)
int batch_alloc(q3_engine* e, int max_streams, uint32_t ctx_len, bool with_kv, int cap = 0) {
    g_err[0] = 0;
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    if (max_streams < 1 || max_streams > kMaxStreams) return fail(Q3_ERR_ARG, "max_streams %d out of range (1..%d)", max_streams, kMaxStreams);
    if (cap < max_streams) cap = max_streams;
    const q3_config& c = e->cfg;
    const int dim = c.dim, L = c.n_layers, hd = c.head_dim, V = c.vocab_size, H = c.hidden_dim, G = c.group_size;
    const int ahd = c.n_heads * hd, kvd = c.n_kv_heads * hd;
    if (G % 64 != 0 || G > 256)
        return fail(Q3_ERR_UNSUPPORTED, "batched decode needs group_size 64, 128 or 256 (one quantization group = 1, 2 or 4 64-byte MFMA steps), got %d", G);
    if (dim % 16 || ahd % 16 || kvd % 16 || H % 16 || V % 16)
        return fail(Q3_ERR_UNSUPPORTED, "batched decode needs every matrix height to be a multiple of the 16-row MFMA tile");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    batch_free(e);
    BatchCtx* b = new BatchCtx();
    e->batch = b;
    b->max_streams = max_streams;
    b->cap = cap;
    b->ctx = (ctx_len != 0 && (int64_t)ctx_len < (int64_t)c.seq_len) ? (int)ctx_len : c.seq_len;
    // scratch columns: a verify pass (q3_verify) is up to kSpecMax positions wide whatever max_streams is
    const size_t S = b->ctx, B = max_streams, C = (size_t)(cap > kSpecMax ? cap : kSpecMax), BL = kSpecMax;

    // ---- packed weight directory
    size_t qbytes = 0, sfloats = 0;
    auto reserve = [&](int rows, int n) {
        BatchCtx::PM m;
        m.q_off = qbytes;
        m.s_off = sfloats;
        m.ntiles = rows / 16;
        m.ng = n / G;
        qbytes += (size_t)rows * n;
        sfloats += (size_t)rows * (n / G);
        return m;
    };
    for (int l = 0; l < L; ++l) {
        b->m_qkv.push_back(reserve(ahd + 2 * kvd, dim));
        b->m_wo.push_back(reserve(dim, ahd));
        b->m_w13.push_back(reserve(2 * H, dim));
        b->m_w2.push_back(reserve(dim, H));
    }
    b->m_cls = reserve(V, dim);
    int rc;
    if ((rc = b->pq.alloc(qbytes)) || (rc = b->ps.alloc(sfloats))) return rc;
    auto pack = [&](const QT& t, int rows, int n, const BatchCtx::PM& m, int tile0, int tile_stride) {
        hipLaunchKernelGGL(k_pack_weights, dim3(e->n_cu * 8), dim3(kWG), 0, e->stream, t.q, t.s, b->pq + m.q_off, b->ps + m.s_off,
                           rows, n, G, tile0, tile_stride);
    };
    for (int l = 0; l < L; ++l) {
        pack(e->wq[l], ahd, dim, b->m_qkv[l], 0, 1);
        pack(e->wk[l], kvd, dim, b->m_qkv[l], ahd / 16, 1);
        pack(e->wv[l], kvd, dim, b->m_qkv[l], (ahd + kvd) / 16, 1);
        pack(e->wo[l], dim, ahd, b->m_wo[l], 0, 1);
        pack(e->w1[l], H, dim, b->m_w13[l], 0, 2);
        pack(e->w3[l], H, dim, b->m_w13[l], 1, 2);
        pack(e->w2[l], dim, H, b->m_w2[l], 0, 1);
    }
    pack(e->wcls, V, dim, b->m_cls, 0, 1);
    HIP_TRY(hipGetLastError());

    // ---- per-stream run state (qwen3.rs:414-445 per stream); KV caches zero-filled
    b->kv_stream = (size_t)L * S * kvd;
    const size_t maxn = (size_t)(H > ahd ? (H > dim ? H : dim) : (ahd > dim ? ahd : dim));
    const size_t nt_max = (C + 15) / 16;
    if ((rc = b->x.alloc(C * dim)) || (rc = b->q.alloc(C * ahd)) || (rc = b->qn.alloc(C * ahd)) || (rc = b->kraw.alloc(C * kvd)) ||
        (rc = b->xb.alloc(C * ahd)) || (rc = b->hb.alloc(C * H)) || (rc = b->logits.alloc(BL * V)))
        return rc;
    b->has_kv = with_kv;
    if (with_kv) {
        if ((rc = b->key.alloc(B * b->kv_stream)) || (rc = b->value.alloc(B * b->kv_stream))) return rc;
        HIP_TRY(hipMemsetAsync(b->key, 0, 4 * B * b->kv_stream, e->stream));
        HIP_TRY(hipMemsetAsync(b->value, 0, 4 * B * b->kv_stream, e->stream));
    }
    HIP_TRY(hipMemsetAsync(b->x, 0, 4 * C * dim, e->stream));
    if ((rc = b->xq_p.alloc(nt_max * 16 * maxn)) || (rc = b->xs_p.alloc(nt_max * 16 * (maxn / G)))) return rc;
    HIP_TRY(hipMemsetAsync(b->xq_p, 0, nt_max * 16 * maxn, e->stream));          // idle stream columns: finite operands
    HIP_TRY(hipMemsetAsync(b->xs_p, 0, 4 * nt_max * 16 * (maxn / G), e->stream));
    if (S > (size_t)dev_knob("Q3_ATT_LDS_MAX", 4096) && (rc = b->att.alloc(B * c.n_heads * S))) return rc;
    if ((rc = b->st.alloc(C))) return rc;
    HIP_TRY(hipMemsetAsync(b->st, 0, sizeof(State) * C, e->stream));
    if (dev_knob("Q3_STAMPS", 0)) {
        const size_t nst = 96 * (size_t)(10 * L + 8);
        if ((rc = b->stamps.alloc(nst))) return rc;
        HIP_TRY(hipMemset(b->stamps, 0, 8 * nst));
    }
    b->nslots = e->n_cu * 4 * kWaves;
    if ((rc = b->slots.alloc(BL * (size_t)b->nslots))) return rc;
    HIP_TRY(hipMemsetAsync(b->slots, 0, 8 * BL * (size_t)b->nslots, e->stream));
    if ((rc = b->spec_io.alloc(1))) return rc;
    HIP_TRY(hipMemsetAsync(b->spec_io, 0, sizeof(SpecIO), e->stream));
    if ((rc = b->spec_snap.alloc(2 * (size_t)L * (kSpecMax - 1) * kvd)) || (rc = b->h_spec.alloc(1))) return rc;
    b->out_cap = (int)S;
    if ((rc = b->out_tokens.alloc(B * S))) return rc;
    HIP_TRY(hipMemsetAsync(b->out_tokens, 0, 4 * B * S, e->stream));
    if ((rc = b->h_st.alloc(B)) || (rc = b->h_tokens.alloc(B * S))) return rc;
    if ((rc = b->h_logits.alloc(BL * V))) return rc;     // a column pass is kColsMax rows whatever max_streams is
    if ((rc = b->col_slot.alloc(kColsMax))) return rc;
    HIP_TRY(hipMemsetAsync(b->col_slot, 0, 4 * kColsMax, e->stream));
    if ((rc = b->cols_ctl.alloc(1))) return rc;
    HIP_TRY(hipMemsetAsync(b->cols_ctl, 0, sizeof(ColsCtl), e->stream));
    if ((rc = b->h_cols.alloc(1))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return Q3_OK;
}

// Score rows of k_attn_pf2, [columns][n_heads][stride floats], for a context of `need` positions (a multiple of 256): grow-only.
// Nothing may outlive the old buffer: pointer, stride and the kept plans (their launches carry both) go first, so a failed
// allocation leaves a state the next call rebuilds from instead of replaying launches on freed memory.
// drop: the plans that carry this buffer; who, noun: the words of the message.
int att_rows_grow(q3_engine* e, DevMem<float>& att_pf, int& stride, size_t columns, int need, PlanDrop drop, const char* who, const char* noun) {
    if (need <= stride) return Q3_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    att_pf.reset();
    stride = 0;
    plans_drop(e->batch, drop);
    const size_t floats = columns * (size_t)e->cfg.n_heads * (size_t)need;
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    if (4 * floats > free_b)
        return fail(Q3_ERR_HIP, "%s: %zu MiB of score rows for blocks of %zu %s over %d positions of context do not fit "
                    "(%zu MiB free): lower Q3_PREFILL_M", who, (4 * floats) >> 20, columns, noun, need, free_b >> 20);
    if (int rc = att_pf.alloc(floats)) return rc;
    stride = need;
    return Q3_OK;
}

// positions per weight pass of a prefill-only context (Q3_PREFILL_M)
int prefill_block_cap(const q3_engine* e) {
    int M = env_int("Q3_PREFILL_M", 2048);
    if (M < 16) M = 16;
    if (M > 4096) M = 4096;
    M = (M + 15) & ~15;
    if (e->cfg.group_size != 64 && M > kMaxStreams) M = kMaxStreams;
    return M;
}

}  // namespace

extern "C" {

int q3_batch_init(q3_engine* e, int max_streams, uint32_t ctx_len) { return batch_alloc(e, max_streams, ctx_len, true); }

/* q3_prefill with the prompt walked in blocks of up to 32 consecutive positions: each block is ONE pass over the
 * weights on the matrix cores (the positions of the block play the role of the streams of q3_forward_batch, all
 * reading and writing the engine's own KV cache).  Sequential-equivalent: the cache rows and the returned token are
 * bit-identical to q3_prefill / to n calls of q3_forward (generation.rs:116-123).  The per-position logits the
 * reference computes and discards are only formed for the last position. */
int q3_prefill_batched(q3_engine* e, const int32_t* tokens, size_t n_tokens, size_t first_pos, int32_t* next_token) {
    g_err[0] = 0;
    if (!e || !tokens || n_tokens == 0) return fail(Q3_ERR_ARG, "null or empty prompt");
    if (first_pos + n_tokens > (size_t)e->cfg.seq_len)
        return fail(Q3_ERR_ARG, "first_pos %zu + n_tokens %zu exceeds seq_len %d", first_pos, n_tokens, e->cfg.seq_len);
    for (size_t i = 0; i < n_tokens; ++i)
        if (tokens[i] < 0 || tokens[i] >= e->cfg.vocab_size)
            return fail(Q3_ERR_ARG, "index out of range: token %d (vocab_size %d)", tokens[i], e->cfg.vocab_size);
    int rc;
    // prefill-only context: scratch for blocks of Q3_PREFILL_M positions (default 2,048: dense path, k_pgemm3 + k_attn_pf2; 32 or less: the batched
    // decode kernels).  A context created by q3_batch_init keeps its 32-column scratch and walks 32 positions per pass.
    // Round 4: default 2,048 (was 256, and capped there by a 256-thread state kernel): the launches of a block cover more tiles -- 4B
    // shape, 2,048-token prompt: 23.5k tok/s at 256, 25.5k at 512, 30.6k at 1,024, 32.3k at 2,048 (profiles/r04_prefill_ab.txt).
    // The score rows of k_attn_pf2 take 4 * M * n_heads * context bytes (1 GiB at M = 2,048, 32 heads, 4,096 positions).
    if (!e->batch && (rc = batch_alloc(e, kMaxStreams, 0, false, prefill_block_cap(e)))) return rc;
    BatchCtx* b = e->batch;
    HIP_TRY(hipSetDevice(e->device));
    const size_t B = (size_t)b->cap;
    // score rows of k_attn_pf2: [block position][head][context so far, rounded up]
    if (B > (size_t)kMaxStreams &&
        (rc = att_rows_grow(e, b->att_pf, b->att_pf_stride, B, (int)(((first_pos + n_tokens) + 255) & ~(size_t)255), PlanDrop::Step, "dense prefill", "positions")))
        return rc;
    memcpy(e->h_tokens, tokens, 4 * n_tokens);
    HIP_TRY(hipMemcpyAsync(e->d_prompt, e->h_tokens, 4 * n_tokens, hipMemcpyHostToDevice, e->stream));
    int n_last = 0;
    for (size_t base = 0; base < n_tokens; base += B) {
        const int n = (int)((n_tokens - base < B) ? n_tokens - base : B);
        n_last = n;
        Plan* plan;
        if ((rc = plan_get(e, PlanKey{PlanKind::Prefill, n, false}, &plan))) return rc;
        hipLaunchKernelGGL(k_set_prefill_states, dim3((n + 255) / 256), dim3(256), 0, e->stream, b->st, e->d_prompt, (int)base, (int)first_pos, n);
        if ((rc = plan_enqueue(e, *plan))) return rc;
    }
    // the matmul epilogues of the blocks wrote value rows into the row-major cache only: the transposed copy the long-context output
    // kernel streams is brought up to date for the prompt's positions in one launch (~0.3 GB of traffic for a 2,048-token 4B prompt)
    if (e->d_value_t) {
        const int kvd_ = e->cfg.n_kv_heads * e->cfg.head_dim;
        hipLaunchKernelGGL(k_value_transpose, dim3((unsigned)((kvd_ + 63) / 64), (unsigned)((n_tokens + 63) / 64), (unsigned)e->cfg.n_layers), dim3(kWG), 0,
                           e->stream, e->d_value, e->d_value_t, e->cfg.seq_len, kvd_, (int)first_pos, (int)n_tokens);
    }
    // The per-position logits the reference computes and discards are only formed for the LAST position: its residual
    // stream goes through the single-stream classifier launch (final RMSNorm + lm_head + argmax + state update, qwen3.rs:72-76)
    HIP_TRY(hipMemcpyAsync(e->d_x, b->x + (size_t)(n_last - 1) * e->cfg.dim, 4 * (size_t)e->cfg.dim, hipMemcpyDeviceToDevice, e->stream));
    if ((rc = e->set_state((size_t)tokens[n_tokens - 1], first_pos + n_tokens - 1))) return rc;
    for (const Launch& L : e->plan)
        if (L.fam == F_LMHEAD) launch(L, e->stream);
    HIP_TRY(hipGetLastError());
    if (e->sampling) {
        // the reference draws one (discarded) sample per prompt position: n_tokens - 1 coins, then the real draw
        if (n_tokens > 1) hipLaunchKernelGGL(k_rng_skip, dim3(1), dim3(1), 0, e->stream, e->draw.ss, (int)(n_tokens - 1));
        if ((rc = e->enqueue_sample())) return rc;
    }
    HIP_TRY(hipMemcpyAsync(e->h_tokens, e->d_out_tokens, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (next_token) *next_token = e->h_tokens[0];
    return Q3_OK;
}

int q3_forward_batch(q3_engine* e, const int32_t* tokens, const int32_t* pos, int n_streams, float* logits_out, int32_t* argmax_out) {
    g_err[0] = 0;
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    Plan* plan;
    int rc = batch_set_state(e, tokens, pos, n_streams, &plan);
    if (rc) return rc;
    BatchCtx* b = e->batch;
    if ((rc = plan_enqueue(e, *plan))) return rc;
    const size_t V = e->cfg.vocab_size;
    if (logits_out) HIP_TRY(hipMemcpyAsync(b->h_logits, b->logits, 4 * V * n_streams, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(b->h_st, b->st, sizeof(State) * (size_t)n_streams, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (logits_out) memcpy(logits_out, b->h_logits, 4 * V * n_streams);
    if (argmax_out)
        for (int i = 0; i < n_streams; ++i) argmax_out[i] = b->h_st[i].token;    // k_next_batch stored the argmax as the next token
    return Q3_OK;
}

int q3_generate_greedy_batch(q3_engine* e, const int32_t* first_tokens, const int32_t* first_pos, int n_streams, size_t n_steps,
                             int32_t* out_tokens) {
    g_err[0] = 0;
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    if (!out_tokens || n_steps == 0) return fail(Q3_ERR_ARG, "null output or zero steps");
    Plan* plan;
    int rc = batch_set_state(e, first_tokens, first_pos, n_streams, &plan);
    if (rc) return rc;
    BatchCtx* b = e->batch;
    for (int i = 0; i < n_streams; ++i)
        if ((size_t)first_pos[i] + n_steps > (size_t)b->ctx)
            return fail(Q3_ERR_ARG, "stream %d: first_pos %d + n_steps %zu exceeds seq_len %d", i, first_pos[i], n_steps, b->ctx);
    for (size_t k = 0; k < n_steps; ++k)
        if ((rc = plan_enqueue(e, *plan))) return rc;
    for (int i = 0; i < n_streams; ++i)
        HIP_TRY(hipMemcpyAsync(b->h_tokens + (size_t)i * n_steps, b->out_tokens + (size_t)i * b->out_cap, 4 * n_steps,
                               hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    memcpy(out_tokens, b->h_tokens, 4 * n_steps * (size_t)n_streams);
    return Q3_OK;
}

int q3_batch_sampler_set(q3_engine* e, float temperature, float topp, const uint64_t* rng_seeds) {
    g_err[0] = 0;
    if (!e || !e->batch || !e->batch->has_kv) return fail(Q3_ERR_ARG, "q3_batch_init has not been called");
    if (int rc = sampler_check(temperature, topp)) return rc;
    if (!rng_seeds && temperature != 0.0f) return fail(Q3_ERR_ARG, "null seeds");
    BatchCtx* b = e->batch;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const int B = b->max_streams;
    int rc;
    if (!b->draw_decode && (rc = b->draw_decode.alloc(e->cfg.vocab_size, B, false))) return rc;
    std::vector<SamplerState> h(B);
    for (int i = 0; i < B; ++i) h[i] = SamplerState{rng_seeds ? rng_seeds[i] : 0ull, temperature, topp, {0, 0, 0, 0}};
    HIP_TRY(hipMemcpy(b->draw_decode.ss, h.data(), sizeof(SamplerState) * B, hipMemcpyHostToDevice));
    draw_args(b->draw_decode, DrawForm::Decode, b->logits, b->st, b->out_tokens, b->out_cap);
    const bool on = temperature != 0.0f;
    plans_drop(b, PlanDrop::Step);                        // the step's launches carry these arguments: re-plan on the next call
    b->sampling = on;
    return Q3_OK;
}

int q3_batch_reset_kv(q3_engine* e) {
    g_err[0] = 0;
    if (!e || !e->batch) return fail(Q3_ERR_ARG, "q3_batch_init has not been called");
    BatchCtx* b = e->batch;
    if (!b->has_kv) return fail(Q3_ERR_ARG, "q3_batch_init has not been called");   // prefill-only context: no per-stream caches
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemsetAsync(b->key, 0, 4 * (size_t)b->max_streams * b->kv_stream, e->stream));
    HIP_TRY(hipMemsetAsync(b->value, 0, 4 * (size_t)b->max_streams * b->kv_stream, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return Q3_OK;
}

/* kind: 0 key cache, 1 value cache, 2 residual stream x of `stream` (parity taps, like q3_read_state) */
int q3_batch_read_state(q3_engine* e, int stream, int kind, size_t offset, size_t count, float* out) {
    g_err[0] = 0;
    if (!e || !e->batch || !out) return fail(Q3_ERR_ARG, "q3_batch_init has not been called");
    BatchCtx* b = e->batch;
    if (stream < 0 || stream >= b->max_streams) return fail(Q3_ERR_ARG, "stream %d out of range", stream);
    if (!b->has_kv) return fail(Q3_ERR_ARG, "q3_batch_init has not been called");
    const float* src;
    size_t total;
    if (kind == 0) { src = b->key + (size_t)stream * b->kv_stream; total = b->kv_stream; }
    else if (kind == 1) { src = b->value + (size_t)stream * b->kv_stream; total = b->kv_stream; }
    else if (kind == 2) { src = b->x + (size_t)stream * e->cfg.dim; total = e->cfg.dim; }
    else return fail(Q3_ERR_ARG, "unknown state kind %d", kind);
    if (offset + count > total) return fail(Q3_ERR_ARG, "range out of bounds");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out, src + offset, 4 * count, hipMemcpyDeviceToHost));
    return Q3_OK;
}

}  // extern "C"

namespace {

// The column site: sampler states and the draw scratch of up to kSpecMax columns (probs / sp / keys: ~5.3 MB per column at a
// 151,936-entry vocabulary), allocated by the first pass that samples -- greedy users of the context never pay for it -- and freed
// with it.  Its states are cleared on the stream before the context sees any of it.
int spec_draw_alloc(q3_engine* e) {
    BatchCtx* b = e->batch;
    HIP_TRY(hipSetDevice(e->device));
    DrawSite site;
    if (int rc = site.alloc(e->cfg.vocab_size, kSpecMax, false)) return rc;
    HIP_TRY(hipMemsetAsync(site.ss, 0, sizeof(SamplerState) * kSpecMax, e->stream));
    // out_tokens is never written: a column's State::step stays 0, and out_cap 0 closes the window
    draw_args(site, DrawForm::Columns, b->logits, b->st, e->d_out_tokens, 0);
    if (b->pen_logits) draw_args_pen(site, b->pen_logits);
    b->draw_cols = std::move(site);
    return Q3_OK;
}

// what every entry point of section 2c refuses, and the shared context (packed weights + block scratch, q3_prefill_batched's)
// draw: the entry points of section 2d, which hold for any sampler setting
int spec_prepare(q3_engine* e, const char* who, bool draw = false) {
    if (e->flags & Q3_FLAG_FAST)
        return fail(Q3_ERR_UNSUPPORTED, "%s needs a reference-order engine: with Q3_FLAG_FAST the block kernels and the single-stream kernels are not bit-equal, "
                    "so a verified token need not be the token the greedy loop produces", who);
    if (e->sampling && !draw)
        return fail(Q3_ERR_UNSUPPORTED, "%s is greedy only: the engine's sampler is set to a temperature > 0 (speculative sampling is not implemented)", who);
    int rc;
    if (!e->batch && (rc = batch_alloc(e, kMaxStreams, 0, false, prefill_block_cap(e)))) return rc;
    if (e->sampling && !e->batch->draw_cols && (rc = spec_draw_alloc(e))) return rc;
    return Q3_OK;
}

// One verify pass over a plan of n_plan columns, n_real <= n_plan of them live.  The result is left in b->h_spec.
int spec_pass(q3_engine* e, const int32_t* tokens, int n_real, int n_plan, size_t first_pos, float* logits_out) {
    BatchCtx* b = e->batch;
    int rc;
    HIP_TRY(hipSetDevice(e->device));
    Plan* plan;
    if ((rc = plan_get(e, PlanKey{PlanKind::Verify, n_plan, e->sampling}, &plan))) return rc;
    b->h_spec->first_pos = (int)first_pos;
    b->h_spec->n_real = n_real;
    for (int i = 0; i < kSpecMax; ++i) b->h_spec->tokens[i] = i < n_real ? tokens[i] : 0;
    HIP_TRY(hipMemcpyAsync(b->spec_io, b->h_spec, offsetof(SpecIO, n_accepted), hipMemcpyHostToDevice, e->stream));
    if ((rc = plan_enqueue(e, *plan))) return rc;
    HIP_TRY(hipMemcpyAsync(&b->h_spec->n_accepted, &b->spec_io->n_accepted, sizeof(SpecIO) - offsetof(SpecIO, n_accepted), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (logits_out) HIP_TRY(hipMemcpy(logits_out, b->logits, 4 * (size_t)e->cfg.vocab_size * (size_t)n_real, hipMemcpyDeviceToHost));
    return Q3_OK;
}

int verify_block(q3_engine* e, const int32_t* tokens, size_t n_tokens, size_t first_pos, int32_t* next_tokens, size_t* n_accepted, float* logits_out,
                 const char* who, bool draw) {
    g_err[0] = 0;
    if (!e || !tokens || !next_tokens || !n_accepted) return fail(Q3_ERR_ARG, "null argument");
    if (n_tokens == 0 || n_tokens > (size_t)kSpecMax) return fail(Q3_ERR_ARG, "n_tokens %zu out of range (1..%d)", n_tokens, kSpecMax);
    if (first_pos >= (size_t)e->cfg.seq_len || first_pos + n_tokens > (size_t)e->cfg.seq_len)
        return fail(Q3_ERR_ARG, "first_pos %zu + n_tokens %zu exceeds seq_len %d", first_pos, n_tokens, e->cfg.seq_len);
    for (size_t i = 0; i < n_tokens; ++i)
        if (tokens[i] < 0 || tokens[i] >= e->cfg.vocab_size)
            return fail(Q3_ERR_ARG, "index out of range: token %d (vocab_size %d)", tokens[i], e->cfg.vocab_size);
    int rc;
    if ((rc = spec_prepare(e, who, draw))) return rc;
    if ((rc = spec_pass(e, tokens, (int)n_tokens, (int)n_tokens, first_pos, logits_out))) return rc;
    const SpecIO* r = e->batch->h_spec;
    *n_accepted = (size_t)r->n_accepted;
    for (size_t i = 0; i < n_tokens; ++i) next_tokens[i] = r->next[i];
    return Q3_OK;
}

}  // namespace

extern "C" {

int q3_verify(q3_engine* e, const int32_t* tokens, size_t n_tokens, size_t first_pos, int32_t* next_tokens, size_t* n_accepted, float* logits_out) {
    return verify_block(e, tokens, n_tokens, first_pos, next_tokens, n_accepted, logits_out, "q3_verify", false);
}

int q3_verify_draw(q3_engine* e, const int32_t* tokens, size_t n_tokens, size_t first_pos, int32_t* next_tokens, size_t* n_accepted, float* logits_out) {
    return verify_block(e, tokens, n_tokens, first_pos, next_tokens, n_accepted, logits_out, "q3_verify_draw", true);
}

size_t q3_lookup_draft(const int32_t* seq, size_t n, int ngram, int draft_len, int32_t* draft) {
    if (!draft) return 0;
    return lookup_draft_rescan(seq, n, ngram, draft_len, draft);
}

int q3_lookup_trace(const int32_t* seq, size_t n, size_t n_corpus, int ngram, int draft_len, int32_t* drafts, int32_t* lens) {
    g_err[0] = 0;
    if ((!seq && n) || !drafts || !lens || n_corpus > n) return fail(Q3_ERR_ARG, "null argument or n_corpus > n");
    if (ngram < 1 || draft_len < 0) return fail(Q3_ERR_ARG, "ngram %d must be >= 1 and draft_len %d >= 0", ngram, draft_len);
    LookupIndex idx(ngram);
    idx.reserve(n);
    for (size_t i = 0; i < n_corpus; ++i) idx.push(seq[i]);
    for (size_t m = n_corpus; m <= n; ++m) {
        lens[m - n_corpus] = (int32_t)idx.draft(draft_len, drafts + (m - n_corpus) * (size_t)draft_len);
        if (m < n) idx.push(seq[m]);
    }
    return Q3_OK;
}

}  // extern "C"

namespace {

int generate_lookup(q3_engine* e, const int32_t* corpus, size_t n_corpus, size_t first_token, size_t first_pos, size_t n_tokens, int ngram,
                    int draft_len, int32_t* out_tokens, q3_spec_stats* stats, const char* who, bool draw) {
    g_err[0] = 0;
    if (stats) *stats = q3_spec_stats{0, 0, 0, 0};
    if (!e || (!out_tokens && n_tokens) || (!corpus && n_corpus)) return fail(Q3_ERR_ARG, "null argument");
    if (ngram < 1) return fail(Q3_ERR_ARG, "ngram %d must be at least 1", ngram);
    if (draft_len < 0 || draft_len > kSpecMax - 1) return fail(Q3_ERR_ARG, "draft_len %d out of range (0..%d)", draft_len, kSpecMax - 1);
    if (n_tokens == 0) return Q3_OK;
    if (first_token >= (size_t)e->cfg.vocab_size || first_pos >= (size_t)e->cfg.seq_len)
        return fail(Q3_ERR_ARG, "index out of range: token %zu (vocab_size %d), pos %zu (seq_len %d)", first_token, e->cfg.vocab_size, first_pos, e->cfg.seq_len);
    if (first_pos + n_tokens > (size_t)e->cfg.seq_len)
        return fail(Q3_ERR_ARG, "first_pos %zu + n_tokens %zu exceeds seq_len %d", first_pos, n_tokens, e->cfg.seq_len);
    int rc;
    if ((rc = spec_prepare(e, who, draw))) return rc;
    HIP_TRY(hipSetDevice(e->device));
    q3_spec_stats st{0, 0, 0, 0};
    LookupIndex idx(ngram);
    idx.reserve(n_corpus + 1 + n_tokens);
    for (size_t i = 0; i < n_corpus; ++i) idx.push(corpus[i]);
    idx.push((int32_t)first_token);
    // one block width per call: a shorter draft leaves the trailing columns as repeats of its last one (k_spec_snapshot)
    const int n_plan = draft_len + 1;
    int32_t block[kSpecMax];
    int32_t cur = (int32_t)first_token;
    size_t done = 0;
    while (done < n_tokens) {
        const size_t pos = first_pos + done, left = n_tokens - done;
        // a pass with d drafts yields up to d + 1 tokens: never more than are still wanted (which also keeps it inside seq_len)
        size_t d = idx.draft(draft_len, block + 1);
        if (d > left - 1) d = left - 1;
        // a drafted token outside the vocabulary (the corpus is the caller's) can never be accepted: the draft ends in front of it
        for (size_t k = 0; k < d; ++k)
            if (block[1 + k] < 0 || block[1 + k] >= e->cfg.vocab_size) { d = k; break; }
        if (d == 0) {
            // no draft: an ordinary single-stream step through the decode graph (and, with the sampler on, its draw)
            if ((rc = e->set_state((size_t)cur, pos))) return rc;
            if ((rc = e->enqueue_forward(pos))) return rc;
            HIP_TRY(hipMemcpyAsync(e->h_tokens, e->d_out_tokens, 4, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            cur = e->h_tokens[0];
            out_tokens[done++] = cur;
            idx.push(cur);
            st.single_steps++;
            continue;
        }
        block[0] = cur;
        if ((rc = spec_pass(e, block, (int)d + 1, n_plan, pos, nullptr))) return rc;
        const SpecIO* r = e->batch->h_spec;
        const size_t a = (size_t)r->n_accepted;
        for (size_t i = 0; i <= a; ++i) {
            out_tokens[done++] = r->next[i];
            idx.push(r->next[i]);
        }
        cur = r->next[a];
        st.verify_passes++;
        st.drafted += d;
        st.accepted += a;
    }
    if (stats) *stats = st;
    return Q3_OK;
}

}  // namespace

extern "C" {

int q3_generate_lookup(q3_engine* e, const int32_t* corpus, size_t n_corpus, size_t first_token, size_t first_pos, size_t n_tokens, int ngram,
                       int draft_len, int32_t* out_tokens, q3_spec_stats* stats) {
    return generate_lookup(e, corpus, n_corpus, first_token, first_pos, n_tokens, ngram, draft_len, out_tokens, stats, "q3_generate_lookup", false);
}

int q3_generate_lookup_draw(q3_engine* e, const int32_t* corpus, size_t n_corpus, size_t first_token, size_t first_pos, size_t n_tokens, int ngram,
                            int draft_len, int32_t* out_tokens, q3_spec_stats* stats) {
    return generate_lookup(e, corpus, n_corpus, first_token, first_pos, n_tokens, ngram, draft_len, out_tokens, stats, "q3_generate_lookup_draw", true);
}

#ifdef Q3_DEV
/* developer: copy the batched-matmul timeline of launch `idx` of the plan (12 phases x 8 stamps); -DQ3_DEV build only */
int q3_dev_batch_stamps(q3_engine* e, int idx, unsigned long long* out) {
    if (!e || !e->batch || !e->batch->stamps || !out) return Q3_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out, e->batch->stamps + 96 * (size_t)idx, 8 * 96, hipMemcpyDeviceToHost));
    return Q3_OK;
}

#endif  // Q3_DEV

}  // extern "C"
