// q3_batch_host.inc -- host side of the batched decode path (included by q3_engine.hip, same translation unit).
//
// B <= 32 independent streams, each with its own KV cache and (token, pos) state, advance one token per step; the
// weights are streamed once per step through the int8 matrix cores (q3_batch.h).  The caller pattern this serves is
// N concurrent `generate` loops (generation.rs:9-48) -- the reference runs them as N processes.

// what a BatchCtx's plan was built for.  Decode: n streams, each over its own KV cache.  Prefill: n positions of one sequence over
// the engine's own KV cache, layers only (the classifier runs once, on the last position, through the single-stream launch).
// Verify: the prefill layers between k_spec_snapshot and the n-column classifier + k_spec_commit + k_spec_restore; with the
// sampler on (plan_draw), the per-column draws of the batched decode and k_spec_commit_draw stand in for k_spec_commit.
// Cols: n columns of (slot, token, position) over the per-stream caches (q3_batch_step_cols): the prefill layers with the cache base
// of every column taken from the slot table, the n-column classifier and k_cols_turn.  Its plans live in BatchCtx::cols_plans.
// SlotPrefill: the dense Prefill layers over the per-stream caches, n > 32 columns of runs of several slots with a slot table as
// long as the block (q3_batch_prefill_slots), on a scratch of their own (BatchCtx::dense); no classifier.  Its plans live in
// BatchCtx::dense_plans.
enum class PlanKind { Decode, Prefill, Verify, Cols, SlotPrefill };

// the per-column buffers the layers of a plan work on: the context's own, or the dense block scratch of SlotPrefill
struct BlockScratch {
    float *x = nullptr, *q = nullptr, *qn = nullptr, *kraw = nullptr, *xb = nullptr, *hb = nullptr;
    int8_t* xq_p = nullptr;
    float* xs_p = nullptr;
    State* st = nullptr;
    int* col_slot = nullptr;
    float* att_pf = nullptr;
    int att_pf_stride = 0;
    int cap = 0;                 // columns (SlotPrefill scratch; 0: not allocated)
};

// the plan widths of a column pass: a pass of n live columns runs the narrowest plan that holds it, padded with repeats of
// its last column
constexpr int kColsWidths[] = {1, 2, 4, 8, 16, 32};
constexpr int kColsNW = 6;
struct ColsPlan {
    std::vector<Launch> plan;
    Graph graph;
    size_t head = 0;             // index of the first launch behind the layers (q3_embed_many launches [0, head) alone)
};
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
    float* att_pf = nullptr;     // k_attn_pf2 score rows [cap][n_heads][att_pf_stride]
    int att_pf_stride = 0;
    int8_t* pq = nullptr;        // packed weights, all matrices
    float* ps = nullptr;
    float* qn = nullptr;         // k_attn_pf2: normalised + rotated queries of the block, head pairs interleaved [cap][n_heads/2][hd][2]
    float *x = nullptr, *q = nullptr, *kraw = nullptr, *xb = nullptr, *hb = nullptr, *logits = nullptr;
    float *key = nullptr, *value = nullptr, *att = nullptr;
    int8_t* xq_p = nullptr;
    float* xs_p = nullptr;
    State* st = nullptr;
    unsigned long long* slots = nullptr;
    int nslots = 0, nslots_used = 0;
    unsigned long long* stamps = nullptr;   // developer timeline (Q3_STAMPS=1, dev build)
    int32_t* out_tokens = nullptr;
    int out_cap = 0;
    State* h_st = nullptr;
    int32_t* h_tokens = nullptr;
    float* h_logits = nullptr;
    std::vector<Launch> plan;    // grids and the stream-tile count are baked in: rebuilt whenever plan_streams or plan_kind changes
    int plan_streams = 0;        // number of streams the plan / graph were built for
    PlanKind plan_kind = PlanKind::Decode;
    bool plan_draw = false;      // Verify only: the plan samples every column (part of the plan key: sampler on / off)
    // draft verification (q3_verify / q3_generate_lookup)
    SpecIO* spec_io = nullptr;   // device: block input and result
    SpecIO* h_spec = nullptr;    // pinned staging of the same
    float* spec_snap = nullptr;  // key / value rows a rejected draft would leave behind, [2][layers][kSpecMax - 1][kv_dim]
    // ... under the sampler (q3_verify_draw / q3_generate_lookup_draw): allocated by the first sampled pass (spec_draw_alloc)
    SamplerState* spec_samp = nullptr;   // [kSpecMax] column sampler states
    float *spec_probs = nullptr, *spec_sp = nullptr;
    unsigned long long* spec_keys = nullptr;
    SampleArgs spec_sargs{};
    size_t plan_head = 0;        // index of the first launch of the classifier tail (prefill blocks before the last skip it)
    bool has_kv = false;         // per-stream KV caches allocated (q3_batch_init); prefill-only contexts have none
    // per-stream device samplers (q3_batch_sampler_set)
    bool sampling = false;
    SamplerState* d_sampler = nullptr;
    float *d_probs = nullptr, *d_sp = nullptr;
    unsigned long long* d_keys = nullptr;
    SampleArgs sargs{};
    Graph graph;
    size_t kv_stream = 0;        // floats per stream in key / value
    // column passes (q3_batch_step_cols / q3_generate_many_greedy)
    int* col_slot = nullptr;     // device [kColsMax]: KV slot of every column of the pass in flight
    ColsCtl* cols_ctl = nullptr; // device
    ColsHost* h_cols = nullptr;
    ColsPlan cols_plans[kColsNW];                       // by width, built on first use (q3_batch_init starts over)
    ColEnt* cols_table = nullptr;                       // the loop's pass table, prompts and output: grow-only device buffers
    int* cols_ncols = nullptr;
    int32_t *cols_prompts = nullptr, *cols_out = nullptr;
    size_t cols_table_cap = 0, cols_ncols_cap = 0, cols_prompts_cap = 0, cols_out_cap = 0;
    // ... under the sampler (q3_batch_step_cols_draw / q3_generate_many_sampled): allocated by the first sampled pass (cols_draw_alloc),
    // the column sampler states and the draw scratch are those of spec_draw_alloc
    ColsPlan cols_plans_draw[kColsNW];                  // the same layers and classifier, then the draws and k_cols_turn_draw
    ColsDraw* cols_draw = nullptr;                      // device
    ColsDrawHost* h_cols_draw = nullptr;
    ColsStep* cols_step = nullptr;                      // device
    SamplerState* cols_slot_samp = nullptr;             // [kMaxStreams] the loop's per-slot states (a single pass uses d_sampler)
    ColAux* cols_aux = nullptr;                         // the loop's table of ColAux and per-request sampler parameters: grow-only
    float *cols_temp = nullptr, *cols_topp = nullptr;
    unsigned long long* cols_seeds = nullptr;
    size_t cols_aux_cap = 0, cols_temp_cap = 0, cols_topp_cap = 0, cols_seeds_cap = 0;
    // ... with stop tokens (q3_generate_many_stop): the scheduler state and its one-row table, the per-request records (grow-only),
    // the pinned status word the host reads after every pass; allocated by the first call
    ColsStopDev* cols_stop = nullptr;                   // device
    SchedStatus* h_cols_stop = nullptr;
    int* cols_req = nullptr;
    size_t cols_req_cap = 0;
    // dense blocks over the per-stream caches (q3_batch_prefill_slots / q3_generate_many_dense): scratch of prefill_block_cap()
    // columns beside the 32-column one, allocated on first use; plans by block width, kept (no graph: the launches are enqueued
    // as they are, like q3_prefill_batched's); the run tables of a call, grow-only
    BlockScratch dense;
    int dense_cap = 0;           // columns per block, fixed by the first dense call (Q3_PREFILL_M as read then): packing and scratch agree
    std::map<int, std::vector<Launch>> dense_plans;
    DenseRun* dense_runs = nullptr;
    size_t dense_runs_cap = 0;
    // the resident shared prefix (q3_batch_prefix_set): key and value rows 0 .. prefix_n - 1 of every layer, [2][n_layers][prefix_n][kv_dim],
    // beside the per-stream caches and private to section 2i; the tokens they were computed from
    float* prefix_store = nullptr;
    size_t prefix_n = 0;
    std::vector<int32_t> prefix_tokens;
    // embeddings (q3_embed_many): the gather tables of a call's blocks and its output rows [n_requests][out_dim], grow-only
    EmbedRow* embed_rows = nullptr;
    float* embed_out = nullptr;
    size_t embed_rows_cap = 0, embed_out_cap = 0;
    // packed-matrix directory
    struct PM { size_t q_off, s_off; int ntiles, ng; };
    std::vector<PM> m_qkv, m_wo, m_w13, m_w2;
    PM m_cls{};
};

namespace {

typedef void (*BGemmFn)(const BGemmArgs);
typedef void (*BQuantFn)(const GemvArgs, const BQuantArgs);

// ---- one resolver per kernel family
// k_bquant (parts == 1) / k_bquant_split: prologue x vector length x parts.  spec: the listed models' vector lengths at group 64 as
// compile-time n (everything that is a division in the generic kernel folds)
BQuantFn bquant_fn(int pro, int nn, int parts, bool spec) {
#define Q3_BQ_PICK(PRO_, N_) if (nn == N_) return (BQuantFn)k_bquant<PRO_, N_>
#define Q3_BQS_PICK(PRO_, N_, P_) if (nn == N_) return (BQuantFn)k_bquant_split<PRO_, N_, P_>
    if (parts == 1) {
        if (spec && pro == PRO_QUANT) { Q3_BQ_PICK(PRO_QUANT, 2048); Q3_BQ_PICK(PRO_QUANT, 3072); Q3_BQ_PICK(PRO_QUANT, 4096); Q3_BQ_PICK(PRO_QUANT, 9728); Q3_BQ_PICK(PRO_QUANT, 12288); }
        else if (spec && pro == PRO_EMBED_NORM) { Q3_BQ_PICK(PRO_EMBED_NORM, 1024); Q3_BQ_PICK(PRO_EMBED_NORM, 2560); Q3_BQ_PICK(PRO_EMBED_NORM, 4096); }
        else if (spec) { Q3_BQ_PICK(PRO_NORM, 1024); Q3_BQ_PICK(PRO_NORM, 2560); Q3_BQ_PICK(PRO_NORM, 4096); }
        return pro == PRO_QUANT ? (BQuantFn)k_bquant<PRO_QUANT> : (pro == PRO_EMBED_NORM ? (BQuantFn)k_bquant<PRO_EMBED_NORM> : (BQuantFn)k_bquant<PRO_NORM>);
    }
    if (spec && pro == PRO_NORM && parts == 4) { Q3_BQS_PICK(PRO_NORM, 1024, 4); Q3_BQS_PICK(PRO_NORM, 2560, 4); Q3_BQS_PICK(PRO_NORM, 4096, 4); }
    if (spec && pro == PRO_QUANT && parts == 8) { Q3_BQS_PICK(PRO_QUANT, 2048, 8); Q3_BQS_PICK(PRO_QUANT, 3072, 8); Q3_BQS_PICK(PRO_QUANT, 4096, 8); Q3_BQS_PICK(PRO_QUANT, 9728, 8); Q3_BQS_PICK(PRO_QUANT, 12288, 8); }
    return pro == PRO_QUANT ? (BQuantFn)k_bquant_split<PRO_QUANT> : (BQuantFn)k_bquant_split<PRO_NORM>;
#undef Q3_BQ_PICK
#undef Q3_BQS_PICK
}

// the matmul families are templates over the epilogue: F<EPI>(shape...) for the run-time epi (nullptr: not instantiated)
#define Q3_BY_EPI(epi, F, ...)                                                                     \
    ((epi) == EPI_QKV ? F<EPI_QKV>(__VA_ARGS__) : (epi) == EPI_RESID ? F<EPI_RESID>(__VA_ARGS__) : \
     (epi) == EPI_SWIGLU ? F<EPI_SWIGLU>(__VA_ARGS__) : F<EPI_LOGITS>(__VA_ARGS__))
template <int EPI, int RT, int NT>
BGemmFn pick_bgemm_nj(int NJ) {
    if (NJ == 1) return (BGemmFn)k_bgemm<EPI, RT, NT, 1>;
    if (NJ == 2) return (BGemmFn)k_bgemm<EPI, RT, NT, 2>;
    if (NJ == 4) return (BGemmFn)k_bgemm<EPI, RT, NT, 4>;
    return nullptr;
}
template <int EPI>
BGemmFn pick_bgemm(int RT, int NT, int NJ) {
    if (RT == 2) return NT == 1 ? pick_bgemm_nj<EPI, 2, 1>(NJ) : pick_bgemm_nj<EPI, 2, 2>(NJ);
    if constexpr (EPI != EPI_SWIGLU) return NT == 1 ? pick_bgemm_nj<EPI, 1, 1>(NJ) : pick_bgemm_nj<EPI, 1, 2>(NJ);
    return nullptr;
}
// the dense prefill kernels have no classifier form
template <int EPI>
BGemmFn pick_pgemm(int RT, int PT) {
    if constexpr (EPI != EPI_LOGITS) {
        if (RT == 2) return PT == 2 ? (BGemmFn)k_pgemm<EPI, 2, 2, 6> : (PT == 1 ? (BGemmFn)k_pgemm<EPI, 2, 1, 8> : nullptr);
        if constexpr (EPI != EPI_SWIGLU) {
            if (RT == 1) return PT == 2 ? (BGemmFn)k_pgemm<EPI, 1, 2, 8> : (PT == 1 ? (BGemmFn)k_pgemm<EPI, 1, 1, 8> : nullptr);
        }
    }
    return nullptr;
}
template <int EPI>
BGemmFn pick_pgemm3(int ptw, int gs) {      // quantization groups per barrier: 2 for 4 x 8 tiles; 4 for 4 x 4, 2 where ng % 8 != 0
    if constexpr (EPI != EPI_LOGITS) {
        if (ptw == 8) return (BGemmFn)k_pgemm3<EPI, 8, 2>;
        return gs == 4 ? (BGemmFn)k_pgemm3<EPI, 4, 4> : (BGemmFn)k_pgemm3<EPI, 4, 2>;
    }
    return nullptr;
}
// k_dgemm of a residual launch (Wo, W2) at group 64: the 16-group ring where the row length allows it, else 8; nullptr: k_bgemm
BGemmFn pick_dgemm(int ng, int& depth) {
    depth = ng % 16 == 0 ? 16 : (ng % 8 == 0 ? 8 : 0);
    return depth == 16 ? (BGemmFn)k_dgemm<16> : (depth == 8 ? (BGemmFn)k_dgemm<8> : nullptr);
}
// per-kv-head decode attention: k_attn_gqa2 (staging and arithmetic on separate waves; head_dim 128, 2 or 4 query heads per kv head)
// or k_attn_gqa, specialised for head_dim 128 with the same two ratios
AttnFn attn_gqa_fn(bool gqa2, int hd, int kvm) {
    if (gqa2) return kvm == 4 ? (AttnFn)k_attn_gqa2<4> : (AttnFn)k_attn_gqa2<2>;
    if (hd == 128 && kvm == 4) return (AttnFn)k_attn_gqa<128, 4>;
    if (hd == 128 && kvm == 2) return (AttnFn)k_attn_gqa<128, 2>;
    return (AttnFn)k_attn_gqa<0, 0>;
}
// dense prefill attention: query heads per kv head (2 | 4) x positions per workgroup (4 | 8)
AttnFn attn_pf2_fn(int kvm, int np) {
    if (np == 8) return kvm == 4 ? (AttnFn)k_attn_pf2<4, 8> : (AttnFn)k_attn_pf2<2, 8>;
    return kvm == 4 ? (AttnFn)k_attn_pf2<4, 4> : (AttnFn)k_attn_pf2<2, 4>;
}

void batch_free(q3_engine* e) {
    BatchCtx* b = e->batch;
    if (!b) return;
    void* dptrs[] = {b->att_pf, b->qn, b->pq, b->ps, b->x, b->q, b->kraw, b->xb, b->hb, b->logits, b->key, b->value, b->att, b->xq_p, b->xs_p,
                     b->st, b->slots, b->out_tokens, b->stamps, b->d_sampler, b->d_probs, b->d_sp, b->d_keys, b->spec_io, b->spec_snap,
                     b->spec_samp, b->spec_probs, b->spec_sp, b->spec_keys, b->col_slot, b->cols_ctl, b->cols_table, b->cols_ncols, b->cols_prompts,
                     b->cols_out, b->cols_draw, b->cols_step, b->cols_slot_samp, b->cols_aux, b->cols_temp, b->cols_topp, b->cols_seeds, b->cols_stop, b->cols_req,
                     b->dense.x, b->dense.q, b->dense.qn, b->dense.kraw, b->dense.xb, b->dense.hb, b->dense.xq_p, b->dense.xs_p, b->dense.st,
                     b->dense.col_slot, b->dense.att_pf, b->dense_runs, b->prefix_store, b->embed_rows, b->embed_out};
    for (void* p : dptrs)
        if (p) (void)hipFree(p);
    if (b->h_st) (void)hipHostFree(b->h_st);
    if (b->h_tokens) (void)hipHostFree(b->h_tokens);
    if (b->h_logits) (void)hipHostFree(b->h_logits);
    if (b->h_spec) (void)hipHostFree(b->h_spec);
    if (b->h_cols) (void)hipHostFree(b->h_cols);
    if (b->h_cols_draw) (void)hipHostFree(b->h_cols_draw);
    if (b->h_cols_stop) (void)hipHostFree(b->h_cols_stop);
    delete b;
    e->batch = nullptr;
}

// (re)build the launch list for n streams (Decode), n block positions (Prefill, Verify; draw: Verify under the sampler) or n
// columns (Cols; draw: the sampled column plan) or n columns of a dense block over the slots (SlotPrefill)
int batch_build_plan(q3_engine* e, int n, PlanKind kind, bool draw = false) {
    BatchCtx* b = e->batch;
    const bool cols = kind == PlanKind::Cols, slotpf = kind == PlanKind::SlotPrefill;
    const bool prefill = kind == PlanKind::Prefill || kind == PlanKind::Verify, verify = kind == PlanKind::Verify;
    const bool block = prefill || cols || slotpf;   // columns may share a cache: all key rows enter it before any column attends
    BlockScratch sc = b->dense;
    if (!slotpf) {
        sc.x = b->x; sc.q = b->q; sc.qn = b->qn; sc.kraw = b->kraw; sc.xb = b->xb; sc.hb = b->hb;
        sc.xq_p = b->xq_p; sc.xs_p = b->xs_p; sc.st = b->st;
        sc.col_slot = cols ? b->col_slot : nullptr;
        sc.att_pf = b->att_pf; sc.att_pf_stride = b->att_pf_stride;
    }
    const q3_config& c = e->cfg;
    const int dim = c.dim, L = c.n_layers, hd = c.head_dim, V = c.vocab_size, H = c.hidden_dim, G = c.group_size;
    const int ahd = c.n_heads * hd, kvd = c.n_kv_heads * hd, S = prefill ? c.seq_len : b->ctx;
    float* key_base = prefill ? e->d_key : b->key;
    float* value_base = prefill ? e->d_value : b->value;
    const long long kv_stride = prefill ? 0 : (long long)b->kv_stream;
    const int strict = (e->flags & Q3_FLAG_FAST) ? 0 : 1;
    const int NT = n <= 16 ? 1 : 2, NJ = G / 64;
    // dense prefill (round 3): more than 32 positions per weight pass -> every wave owns an output tile (k_pgemm)
    const bool dense = (prefill || slotpf) && n > 32;
    // batched decode / short prefill blocks at group 64: in-lane accumulation for the residual launches (k_dgemm, round 4);
    // Q3_BATCH_DGEMM=0 keeps k_bgemm
    const bool dgemm = !dense && G == 64 && dev_knob("Q3_BATCH_DGEMM", 1) != 0;
    if (dense && G != 64) return fail(Q3_ERR_UNSUPPORTED, "dense prefill needs group_size 64");
    const int nptiles = (n + 15) / 16;
    const int att_tch = dev_knob("Q3_BATCH_ATT_TCH", 32);
    const int att_lds_max = dev_knob("Q3_ATT_LDS_MAX", 4096);
    const bool bq_spec = G == 64 && dev_knob("Q3_BQUANT_SPEC", 1) != 0;
    b->graph.reset();
    b->plan.clear();
    b->plan_streams = n;
    b->plan_kind = kind;
    b->plan_draw = draw;
    int rc;
    Launch Ln;
    // developer timeline: the cells of the launch about to be appended
    auto stamp_cells = [&]() -> unsigned long long* { return b->stamps ? b->stamps + 96 * (size_t)b->plan.size() : nullptr; };
    // the copies of k_spec_snapshot / k_spec_restore: up to (n - 1) rows of kv_dim floats per layer and cache, a float4 per thread
    const unsigned spec_grid = (unsigned)std::min<long>(8L * e->n_cu, std::max<long>(1, ((long)L * (kSpecMax - 1) * (kvd / 4) + kWG - 1) / kWG));
    if (verify) {
        if ((rc = make_launch(Ln, F_NEXT, k_spec_snapshot, dim3(spec_grid), dim3(kWG), 0, b->st, b->spec_io, n, e->d_key, e->d_value, b->spec_snap,
                              L, c.seq_len, kvd))) return rc;
        b->plan.push_back(Ln);
        if (draw) {
            if ((rc = make_launch(Ln, F_NEXT, k_spec_sampler_states, dim3(1), dim3(64), 0, b->spec_io, n, e->d_sampler, b->spec_samp, b->st))) return rc;
            b->plan.push_back(Ln);
        }
    }

    auto quant = [&](Family fam, int pro, const float* in, long long in_stride, int nn, const float* norm_w) -> int {
        const bool embed = pro == PRO_EMBED_NORM, stage = pro != PRO_QUANT;
        GemvArgs a{};
        a.n = nn;
        a.group = G;
        a.strict = strict;
        a.st = sc.st;
        a.seq_len = S;
        a.in = in;
        a.norm_w = norm_w;
        if (embed) { a.emb_q = e->tok.q; a.emb_s = e->tok.s; a.x_out = sc.x; }
        BQuantArgs qa{};
        qa.in_stride = in_stride;
        qa.x_out_stride = dim;
        qa.xq_p = sc.xq_p;
        qa.xs_p = sc.xs_p;
        qa.n_streams = n;
        // several workgroups per stream (k_bquant_split): 4 parts for the RMSNorm prologues, 8 for the plain quantize --
        // as long as a part is a whole number of quantization groups and at most two float4 slots per thread
        // (not for position blocks of 256 and more: the parts repeat the exact sum and a block that size fills the chip with one
        // workgroup per position -- 4B prefill, same box, split -> unsplit: 22,960 -> 23,140 tok/s at 256-position blocks, 26,480 ->
        // 26,720 at 512, 29,090 -> 29,520 at 1,024, 31,330 -> 32,100 at 2,048 (r04); the 32-stream decode step keeps the split)
        int parts = 1;
        if (!embed && dev_knob("Q3_BQUANT_SPLIT", 1) && n < dev_knob("Q3_BQUANT_SPLIT_MAX_N", 256)) {
            for (int c = (pro == PRO_QUANT ? 8 : 4); c > 1; c >>= 1)
                if (nn % (c * G) == 0 && nn / c >= 256 && nn / c <= 8 * kWG) { parts = c; break; }
        }
        size_t smem = gemv_smem_bytes(nn, G, 1, stage);
        if (parts > 1) {
            a.stamps = stamp_cells();
            const size_t slice = align16((size_t)(nn / parts)) + align16(4 * (size_t)(nn / parts / G));
            smem = slice + (stage ? 4 * (size_t)(term_floats(nn) + 128) : 0);
        }
        if ((rc = make_launch(Ln, fam, bquant_fn(pro, nn, parts, bq_spec), dim3((unsigned)parts, (unsigned)n), dim3(kWG), smem, a, qa))) return rc;
        b->plan.push_back(Ln);
        return Q3_OK;
    };
    auto gemm = [&](Family fam, int epi, const BatchCtx::PM& m, BGemmArgs a) -> int {
        a.wq = b->pq + m.q_off;
        a.ws = b->ps + m.s_off;
        a.xq = sc.xq_p;
        a.xs = sc.xs_p;
        a.ng = m.ng;
        a.ntiles = m.ntiles;
        a.n_streams = n;
        a.st = sc.st;
        BGemmFn fn = nullptr;
        unsigned grid = 1, block = 0;
        size_t smem = 0;
        int depth = 0;
        // LDS-staged workgroup tiles of 4 row tiles x 8 or 4 position tiles (k_pgemm3, round 4), two workgroups per CU, the grid walks
        // the (row block, position block) list.  Tile width by measurement (4B shape, us per 256 positions, profiles/r04_prefill_ab.txt):
        // W1|W3 (608 tiles of 4 x 8) 45.5 vs 50.8 for 4 x 4 vs 53.2 k_pgemm; Wo / W2 (80 tiles of 4 x 8) 46.5 vs 33.9 vs 39.0; QKV 22.2 vs
        // 22.6 vs 25.2 -- 4 x 8 where that fills the resident slots, 4 x 4 otherwise.  Q3_PGEMM2_PT = 8 / 4 forces a width,
        // Q3_PGEMM2=0 keeps k_pgemm.
        if (dense && nptiles >= 6 && (m.ntiles % kP2RT) == 0 && (m.ng % 4) == 0 && epi != EPI_LOGITS && dev_knob("Q3_PGEMM2", 1) != 0) {
            const long nrb = m.ntiles / kP2RT;
            const long t8 = nrb * ((nptiles + 7) / 8), t4 = nrb * ((nptiles + 3) / 4), slots = 2L * e->n_cu;
            int ptw = dev_knob("Q3_PGEMM2_PT", 0);
            if (ptw != 4 && ptw != 8) ptw = t8 >= slots ? 8 : 4;
            const long nblk = ptw == 8 ? t8 : t4;
            // (2 row tiles x 4 position tiles per workgroup, Wo / W2 of the 4B shape: 36.1 vs 34.5 us; 8 x 8 tiles: 30.1-30.9k tok/s
            // against 32.1k for 4 x 8 -- neither kept)
            // quantization groups per barrier (the kernel walks stage pairs: ng % (2 gs) == 0): 2 for 4 x 8 tiles; 4 for 4 x 4, or 2
            // where the row has an odd number of 4-group stages (ng % 8 == 4; Q3_PGEMM3_GS=2 forces that form on 4 x 4 tiles -- 2 is the only value with a meaning, any other keeps the choice above)
            const int gs = ptw == 8 ? 2 : ((m.ng % 8) == 0 && dev_knob("Q3_PGEMM3_GS", 4) != 2 ? 4 : 2);
            fn = Q3_BY_EPI(epi, pick_pgemm3, ptw, gs);
            grid = (unsigned)(nblk < slots ? nblk : slots);
            block = kP2Threads;
            smem = pgemm3_smem_bytes(ptw, gs);
        } else if (dense) {
            // wave tasks of RT row tiles x PT position tiles; smaller tiles for the small matrices so that every SIMD has work
            // (r03 sweep, 4B shape: 2 x 2 tiles with a 6-deep ring for the big matrices, 1 x 2 / 8-deep for the 160-tile ones)
            int RT = 2, PT = nptiles >= 2 ? 2 : 1;
            auto tasks = [&](int rt, int pt) { return (long)(m.ntiles / rt) * ((nptiles + pt - 1) / pt); };
            if (epi != EPI_SWIGLU && ((m.ntiles & 1) || tasks(RT, PT) < 8L * e->n_cu)) RT = 1;
            const long nt_ = tasks(RT, PT);
            if (epi == EPI_LOGITS) return fail(Q3_ERR_UNSUPPORTED, "dense prefill has no classifier launch");
            if (!(fn = Q3_BY_EPI(epi, pick_pgemm, RT, PT))) return fail(Q3_ERR_UNSUPPORTED, "no dense prefill kernel for tile %d x %d", RT, PT);
            grid = (unsigned)std::min<long>((nt_ + 3) / 4, 3L * e->n_cu);
            block = kPgThreads;
        } else if ((fn = (dgemm && epi == EPI_RESID) ? pick_dgemm(m.ng, depth) : nullptr)) {
            // decode, group 64, residual launches (Wo, W2): every wave owns a (row tile, stream tile) accumulator tile for the whole
            // contraction (k_dgemm).  Same-box A/B on the 8B shape (profiles/r04_batch32_dgemm.md): the residual launches gain 3-4 % of
            // the step; QKV (11.6 vs 12.9 us), W1|W3 with the fused quantizer (27.7 vs 22.5 + 4.8 us) and the classifier (131-136 vs
            // 130 us) in this form do not beat k_bgemm
            grid = (unsigned)(((long)m.ntiles * NT + kDgWaves - 1) / kDgWaves);
            block = (unsigned)kDgWaves * 64;
            smem = dgemm_smem_bytes(depth);
        } else {
            a.stamps = stamp_cells();
            // one workgroup per row task (RT tiles), two workgroups per CU (64 KiB term tile each).  Two tiles per task
            // share the activation fragments (cost ~1.7x one tile) -- worth it once that saves rounds over the CUs.
            const long slots = (long)e->n_cu * dev_knob("Q3_BATCH_WG_PER_CU", 2);
            int RT = 2;
            if (epi != EPI_SWIGLU) {
                const long r1 = (m.ntiles + slots - 1) / slots, r2 = (m.ntiles / 2 + slots - 1) / slots;
                RT = (m.ntiles % 2 == 0 && r2 * 17 < r1 * 10) ? 2 : 1;
                // between one and two row tiles per CU (QKV of the 4B / 8B shapes: 384 tiles) single-tile tasks put two workgroups
                // on half of the CUs and one on the rest; pairs give 192 CUs one task each (r04 same-box A/B: 3.376 -> 3.358 ms / step)
                if (m.ntiles % 2 == 0 && m.ntiles > e->n_cu && m.ntiles / 2 <= e->n_cu) RT = 2;
                const int force_rt = dev_knob("Q3_BATCH_RT", 0);
                if (force_rt && (m.ntiles % force_rt) == 0) RT = force_rt;
            }
            const long ntasks = m.ntiles / RT;
            grid = (unsigned)(ntasks < slots ? ntasks : slots);
            block = kBThreads;
            smem = bgemm_smem_bytes(RT, NT);
            if (epi == EPI_LOGITS) {
                if ((int)grid > b->nslots) return fail(Q3_ERR_HIP, "argmax slot capacity");
                a.slots = b->slots;
                a.nslots = b->nslots;
                b->nslots_used = (int)grid;
            }
            if (!(fn = Q3_BY_EPI(epi, pick_bgemm, RT, NT, NJ))) return fail(Q3_ERR_UNSUPPORTED, "no batched kernel for group size %d", G);
        }
        if ((rc = make_launch(Ln, fam, fn, dim3(grid), dim3(block), smem, a))) return rc;
        b->plan.push_back(Ln);
        return Q3_OK;
    };

    for (int l = 0; l < L; ++l) {
        const size_t kv_off = (size_t)l * S * kvd;
        bool fused_xb_quant = false;
        if ((rc = quant(F_QKV, l == 0 ? PRO_EMBED_NORM : PRO_NORM, sc.x, dim, dim, e->rms_att + (size_t)l * dim))) return rc;
        {
            BGemmArgs a{};
            a.out0 = sc.q; a.out0_stride = ahd;
            a.out1 = sc.kraw; a.out1_stride = kvd;
            a.out2 = value_base + kv_off; a.out2_stride = kv_stride;
            a.rows0 = ahd; a.rows1 = kvd; a.pos_stride = kvd;
            a.col_slot = sc.col_slot;
            if ((rc = gemm(F_QKV, EPI_QKV, b->m_qkv[l], a))) return rc;
        }
        {
            AttnArgs a{};
            a.q = sc.q;
            a.key_cache = key_base + kv_off;
            a.k_raw = sc.kraw;
            a.value_cache = value_base + kv_off;
            a.q_norm_w = e->q_ln + (size_t)l * hd;
            a.k_norm_w = e->k_ln + (size_t)l * hd;
            a.rope = e->d_rope;
            a.xb = sc.xb;
            a.att_global = S > att_lds_max ? b->att : nullptr;
            a.st = sc.st;
            a.pos_override = -1;
            a.n_heads = c.n_heads;
            a.n_kv_heads = c.n_kv_heads;
            a.hd = hd;
            a.seq_len = S;
            a.strict = strict;
            a.sb_q = ahd; a.sb_kraw = kvd; a.sb_kv = kv_stride; a.sb_xb = ahd;
            a.sb_att = (long long)c.n_heads * S;
            a.col_slot = sc.col_slot;
            a.tch = att_tch < attn_tch(hd) ? att_tch : attn_tch(hd);
            const int kv_mul = c.n_heads / c.n_kv_heads;
            const bool gqa = kv_mul <= 7 && hd <= 256 && (hd & (hd - 1)) == 0 && hd >= 16 &&
                             attn_gqa_smem_bytes(hd, kv_mul, S) <= 150 * 1024 && dev_knob("Q3_BATCH_ATT_GQA", 1);
            // dense prefill, head_dim 128 with 2 or 4 query heads per kv head: k_attn_pf2 (Q3_PREFILL_ATT_PF=0: k_attn_gqa2)
            const bool use_pf = dense && hd == kG2Hd && (kv_mul == 2 || kv_mul == 4) && sc.att_pf != nullptr && dev_knob("Q3_PREFILL_ATT_PF", 1);
            if (slotpf && !use_pf) return fail(Q3_ERR_UNSUPPORTED, "a dense block over the slots needs k_attn_pf2 (head_dim 128, 2 or 4 query heads per kv head)");
            if (block && !gqa && !use_pf) return fail(Q3_ERR_UNSUPPORTED, "batched prefill needs the per-kv-head attention kernel");
            if (block) {   // all key rows of the block enter the cache before any position attends
                if (use_pf) a.q_out = sc.qn;                        // the same launch normalises + rotates the block's query heads
                // long blocks of head_dim-128 models: 64 vectors per workgroup, one chain per lane (k_knorm_rope_blk); Q3_KNORM_BLK=0: one wave per vector
                if (n >= 64 && hd == kG2Hd && dev_knob("Q3_KNORM_BLK", 1)) {
                    const long nvec = (long)n * (c.n_kv_heads + (use_pf ? c.n_heads : 0));
                    rc = make_launch(Ln, F_ATTN, k_knorm_rope_blk, dim3((unsigned)((nvec + kKnbVec - 1) / kKnbVec)), dim3(256), knorm_blk_smem_bytes(), a, n, use_pf ? 1 : 0);
                } else {
                    rc = make_launch(Ln, F_ATTN, k_knorm_rope, dim3((unsigned)(c.n_kv_heads + (use_pf ? c.n_heads : 0)), (unsigned)n), dim3(64), 0, a);
                }
                if (rc) return rc;
                b->plan.push_back(Ln);
                a.k_in_cache = 1;
            }
            if (use_pf) {
                // NP consecutive positions x the kv head's query heads per workgroup, one wave per (position, head pair)
                a.att_global = sc.att_pf;
                a.att_stride = sc.att_pf_stride;
                a.n_pos = n;
                a.pack_q = sc.xq_p;
                a.pack_s = sc.xs_p;
                a.group = G;
                fused_xb_quant = true;
                a.stamps = stamp_cells();
                // 8 positions per workgroup once that still gives every CU a workgroup
                const int npw = (dev_knob("Q3_PREFILL_ATT_NP", 0) == 8 || (dev_knob("Q3_PREFILL_ATT_NP", 0) == 0 && (long)c.n_kv_heads * ((n + 7) / 8) >= e->n_cu)) ? 8 : 4;
                rc = make_launch(Ln, F_ATTN, attn_pf2_fn(kv_mul, npw), dim3((unsigned)c.n_kv_heads, (unsigned)((n + npw - 1) / npw)),
                                 dim3((unsigned)attn_pf2_threads(kv_mul, npw)), attn_pf2_smem_bytes(), a);
            } else if (gqa) {
                // one workgroup per (stream, kv head): K/V staged once for the kv_mul query heads sharing it
                a.att_global = nullptr;
                if (hd % G == 0 && dev_knob("Q3_BATCH_FUSE_XB_QUANT", 1)) {   // Wo's activation prologue rides in the epilogue
                    a.pack_q = sc.xq_p;
                    a.pack_s = sc.xs_p;
                    a.group = G;
                    fused_xb_quant = true;
                }
                a.stamps = stamp_cells();
                // head_dim 128 with 2 or 4 query heads per kv head: staging and arithmetic on separate waves, two LDS tiles
                const bool gqa2 = hd == kG2Hd && (kv_mul == 2 || kv_mul == 4) && attn_gqa2_smem_bytes(kv_mul, S) <= 150 * 1024 && dev_knob("Q3_BATCH_ATT_GQA2", 1);
                rc = make_launch(Ln, F_ATTN, attn_gqa_fn(gqa2, hd, kv_mul), dim3((unsigned)c.n_kv_heads, (unsigned)n),
                                 dim3(gqa2 ? (unsigned)kG2Threads : (unsigned)(kv_mul + 1) * 64),
                                 gqa2 ? attn_gqa2_smem_bytes(kv_mul, S) : attn_gqa_smem_bytes(hd, kv_mul, S), a);
            } else {
                rc = make_launch(Ln, F_ATTN, k_attn_streams, dim3((unsigned)c.n_heads, (unsigned)n), dim3(kWG), attn_smem_bytes(hd, a.att_global ? 0 : S, a.tch), a);
            }
            if (rc) return rc;
            b->plan.push_back(Ln);
        }
        if (!fused_xb_quant && (rc = quant(F_WO, PRO_QUANT, sc.xb, ahd, ahd, nullptr))) return rc;
        {
            BGemmArgs a{};
            a.out0 = sc.x; a.out0_stride = dim;
            if ((rc = gemm(F_WO, EPI_RESID, b->m_wo[l], a))) return rc;
        }
        if ((rc = quant(F_W13, PRO_NORM, sc.x, dim, dim, e->rms_ffn + (size_t)l * dim))) return rc;
        {
            BGemmArgs a{};
            a.out0 = sc.hb; a.out0_stride = H;
            if ((rc = gemm(F_W13, EPI_SWIGLU, b->m_w13[l], a))) return rc;
        }
        if ((rc = quant(F_W2, PRO_QUANT, sc.hb, H, H, nullptr))) return rc;
        {
            BGemmArgs a{};
            a.out0 = sc.x; a.out0_stride = dim;
            if ((rc = gemm(F_W2, EPI_RESID, b->m_w2[l], a))) return rc;
        }
    }
    b->plan_head = b->plan.size();
    if ((prefill && !verify) || slotpf) return Q3_OK;   // Prefill: the classifier runs once, on the last position, through the single-stream launch; SlotPrefill: cache rows only
    if ((rc = quant(F_LMHEAD, PRO_NORM, b->x, dim, dim, e->rms_final))) return rc;
    {
        BGemmArgs a{};
        a.out0 = b->logits; a.out0_stride = V;
        if ((rc = gemm(F_LMHEAD, EPI_LOGITS, b->m_cls, a))) return rc;
    }
    if (verify && draw) {
        // Sampler::sample of every column on the block's logits, exactly the batched decode's launches (one workgroup per column
        // behind the element-wise passes spread over the chip), between the per-column maximum they read and the sampled commit
        if ((rc = make_launch(Ln, F_NEXT, k_spec_colmax, dim3(1), dim3(kWG), 0, b->st, b->slots, b->nslots, b->nslots_used, n))) return rc;
        b->plan.push_back(Ln);
        if ((rc = make_launch(Ln, F_NEXT, k_sample_exp, dim3(64, (unsigned)n), dim3(256), 0, b->spec_sargs))) return rc;
        b->plan.push_back(Ln);
        if ((rc = make_launch(Ln, F_NEXT, k_sample, dim3((unsigned)n), dim3(kSampThreads), 4 * kSegFloats, b->spec_sargs))) return rc;
        b->plan.push_back(Ln);
        if ((rc = make_launch(Ln, F_NEXT, k_spec_commit_draw, dim3(1), dim3(64), 0, b->spec_io, b->st, b->spec_samp, e->d_state, e->d_sampler,
                              e->d_out_tokens, e->out_cap))) return rc;
        b->plan.push_back(Ln);
        if ((rc = make_launch(Ln, F_NEXT, k_spec_restore, dim3(spec_grid), dim3(kWG), 0, b->spec_io, e->d_key, e->d_value, e->d_value_t, b->spec_snap,
                              L, c.seq_len, kvd))) return rc;
        b->plan.push_back(Ln);
    } else if (cols && draw) {
        // the draws of the verify pass above over the column sampler states k_cols_turn_draw set up; columns that do not draw
        // (interior prompt positions, pads, temperature-0 slots) return at once in both sampler launches
        if ((rc = make_launch(Ln, F_NEXT, k_spec_colmax, dim3(1), dim3(kWG), 0, b->st, b->slots, b->nslots, b->nslots_used, n))) return rc;
        b->plan.push_back(Ln);
        if ((rc = make_launch(Ln, F_NEXT, k_sample_exp, dim3(64, (unsigned)n), dim3(256), 0, b->spec_sargs))) return rc;
        b->plan.push_back(Ln);
        if ((rc = make_launch(Ln, F_NEXT, k_sample, dim3((unsigned)n), dim3(kSampThreads), 4 * kSegFloats, b->spec_sargs))) return rc;
        b->plan.push_back(Ln);
        if ((rc = make_launch(Ln, F_NEXT, k_cols_turn_draw, dim3(1), dim3(kWG), 0, b->cols_ctl, b->cols_draw, b->spec_samp, b->st, b->col_slot))) return rc;
        b->plan.push_back(Ln);
    } else if (cols) {
        if ((rc = make_launch(Ln, F_NEXT, k_cols_turn, dim3(1), dim3(kWG), 0, b->cols_ctl, b->slots, b->nslots, b->nslots_used, b->st, b->col_slot))) return rc;
        b->plan.push_back(Ln);
    } else if (verify) {
        if ((rc = make_launch(Ln, F_NEXT, k_spec_commit, dim3(1), dim3(kWG), 0, b->spec_io, b->slots, b->nslots, b->nslots_used, e->d_state,
                              e->d_out_tokens, e->out_cap))) return rc;
        b->plan.push_back(Ln);
        if ((rc = make_launch(Ln, F_NEXT, k_spec_restore, dim3(spec_grid), dim3(kWG), 0, b->spec_io, e->d_key, e->d_value, e->d_value_t, b->spec_snap,
                              L, c.seq_len, kvd))) return rc;
        b->plan.push_back(Ln);
    } else {
        if ((rc = make_launch(Ln, F_NEXT, k_next_batch, dim3((unsigned)n), dim3(kWG), 0, b->st, b->slots, b->nslots, b->nslots_used, b->out_tokens, b->out_cap))) return rc;
        b->plan.push_back(Ln);
    }
    if (b->sampling && !block) {      // Sampler::sample per stream on the logits of this step (one workgroup per stream)
        if (b->sargs.pre_exp) {         // ... behind its element-wise passes spread over the chip
            if ((rc = make_launch(Ln, F_NEXT, k_sample_exp, dim3(64, (unsigned)n), dim3(256), 0, b->sargs))) return rc;
            b->plan.push_back(Ln);
        }
        if ((rc = make_launch(Ln, F_NEXT, k_sample, dim3((unsigned)n), dim3(kSampThreads), 4 * kSegFloats, b->sargs))) return rc;
        b->plan.push_back(Ln);
    }
    if (!(e->flags & Q3_FLAG_NO_GRAPH) && kind != PlanKind::Prefill)
        return b->graph.capture(e->stream, [&] {
            for (const Launch& K : b->plan) launch(K, e->stream);
            return Q3_OK;
        });
    return Q3_OK;
}

int batch_enqueue_step(q3_engine* e) {
    BatchCtx* b = e->batch;
    if (b->graph) return b->graph.launch(e->stream);
    for (const Launch& Ln : b->plan) launch(Ln, e->stream);
    HIP_TRY(hipGetLastError());
    return Q3_OK;
}

int batch_set_state(q3_engine* e, const int32_t* tokens, const int32_t* pos, int n) {
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
    if (b->plan_streams != n || b->plan_kind != PlanKind::Decode) {
        int rc = batch_build_plan(e, n, PlanKind::Decode);
        if (rc) return rc;
    }
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
    HIP_TRY(hipMalloc((void**)&b->pq, qbytes));
    HIP_TRY(hipMalloc((void**)&b->ps, 4 * sfloats));
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
    HIP_TRY(hipMalloc((void**)&b->x, 4 * C * dim));
    HIP_TRY(hipMalloc((void**)&b->q, 4 * C * ahd));
    HIP_TRY(hipMalloc((void**)&b->qn, 4 * C * ahd));
    HIP_TRY(hipMalloc((void**)&b->kraw, 4 * C * kvd));
    HIP_TRY(hipMalloc((void**)&b->xb, 4 * C * ahd));
    HIP_TRY(hipMalloc((void**)&b->hb, 4 * C * H));
    HIP_TRY(hipMalloc((void**)&b->logits, 4 * BL * V));
    b->has_kv = with_kv;
    if (with_kv) {
        HIP_TRY(hipMalloc((void**)&b->key, 4 * B * b->kv_stream));
        HIP_TRY(hipMalloc((void**)&b->value, 4 * B * b->kv_stream));
        HIP_TRY(hipMemsetAsync(b->key, 0, 4 * B * b->kv_stream, e->stream));
        HIP_TRY(hipMemsetAsync(b->value, 0, 4 * B * b->kv_stream, e->stream));
    }
    HIP_TRY(hipMemsetAsync(b->x, 0, 4 * C * dim, e->stream));
    HIP_TRY(hipMalloc((void**)&b->xq_p, nt_max * 16 * maxn));
    HIP_TRY(hipMalloc((void**)&b->xs_p, 4 * nt_max * 16 * (maxn / G)));
    HIP_TRY(hipMemsetAsync(b->xq_p, 0, nt_max * 16 * maxn, e->stream));          // idle stream columns: finite operands
    HIP_TRY(hipMemsetAsync(b->xs_p, 0, 4 * nt_max * 16 * (maxn / G), e->stream));
    if (S > (size_t)dev_knob("Q3_ATT_LDS_MAX", 4096)) HIP_TRY(hipMalloc((void**)&b->att, 4 * B * c.n_heads * S));
    HIP_TRY(hipMalloc((void**)&b->st, sizeof(State) * C));
    HIP_TRY(hipMemsetAsync(b->st, 0, sizeof(State) * C, e->stream));
    if (dev_knob("Q3_STAMPS", 0)) {
        const size_t nst = 96 * (size_t)(10 * L + 8);
        HIP_TRY(hipMalloc((void**)&b->stamps, 8 * nst));
        HIP_TRY(hipMemset(b->stamps, 0, 8 * nst));
    }
    b->nslots = e->n_cu * 4 * kWaves;
    HIP_TRY(hipMalloc((void**)&b->slots, 8 * BL * (size_t)b->nslots));
    HIP_TRY(hipMemsetAsync(b->slots, 0, 8 * BL * (size_t)b->nslots, e->stream));
    HIP_TRY(hipMalloc((void**)&b->spec_io, sizeof(SpecIO)));
    HIP_TRY(hipMemsetAsync(b->spec_io, 0, sizeof(SpecIO), e->stream));
    HIP_TRY(hipMalloc((void**)&b->spec_snap, 4 * 2 * (size_t)L * (kSpecMax - 1) * kvd));
    HIP_TRY(hipHostMalloc((void**)&b->h_spec, sizeof(SpecIO), hipHostMallocDefault));
    b->out_cap = (int)S;
    HIP_TRY(hipMalloc((void**)&b->out_tokens, 4 * B * S));
    HIP_TRY(hipMemsetAsync(b->out_tokens, 0, 4 * B * S, e->stream));
    HIP_TRY(hipHostMalloc((void**)&b->h_st, sizeof(State) * B, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void**)&b->h_tokens, 4 * B * S, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void**)&b->h_logits, 4 * BL * V, hipHostMallocDefault));     // a column pass is kColsMax rows whatever max_streams is
    HIP_TRY(hipMalloc((void**)&b->col_slot, 4 * kColsMax));
    HIP_TRY(hipMemsetAsync(b->col_slot, 0, 4 * kColsMax, e->stream));
    HIP_TRY(hipMalloc((void**)&b->cols_ctl, sizeof(ColsCtl)));
    HIP_TRY(hipMemsetAsync(b->cols_ctl, 0, sizeof(ColsCtl), e->stream));
    HIP_TRY(hipHostMalloc((void**)&b->h_cols, sizeof(ColsHost), hipHostMallocDefault));
    HIP_TRY(hipStreamSynchronize(e->stream));
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
    if (B > (size_t)kMaxStreams) {
        const int need = (int)(((first_pos + n_tokens) + 255) & ~(size_t)255);
        if (need > b->att_pf_stride) {
            HIP_TRY(hipStreamSynchronize(e->stream));
            if (b->att_pf) (void)hipFree(b->att_pf);
            // nothing may outlive the old buffer: pointer, stride and the cached plan (its launches carry both) go first, so a
            // failed allocation leaves a state the next call rebuilds from instead of replaying launches on freed memory
            b->att_pf = nullptr;
            b->att_pf_stride = 0;
            b->plan_streams = 0;
            const size_t bytes = 4 * B * (size_t)e->cfg.n_heads * (size_t)need;
            size_t free_b = 0, total_b = 0;
            (void)hipMemGetInfo(&free_b, &total_b);
            if (bytes > free_b)
                return fail(Q3_ERR_HIP, "dense prefill: %zu MiB of score rows for blocks of %zu positions over %d positions of context do not fit "
                            "(%zu MiB free): lower Q3_PREFILL_M", bytes >> 20, B, need, free_b >> 20);
            HIP_TRY(hipMalloc((void**)&b->att_pf, bytes));
            b->att_pf_stride = need;
        }
    }
    memcpy(e->h_tokens, tokens, 4 * n_tokens);
    HIP_TRY(hipMemcpyAsync(e->d_prompt, e->h_tokens, 4 * n_tokens, hipMemcpyHostToDevice, e->stream));
    int n_last = 0;
    for (size_t base = 0; base < n_tokens; base += B) {
        const int n = (int)((n_tokens - base < B) ? n_tokens - base : B);
        n_last = n;
        if (b->plan_streams != n || b->plan_kind != PlanKind::Prefill)
            if ((rc = batch_build_plan(e, n, PlanKind::Prefill))) return rc;
        hipLaunchKernelGGL(k_set_prefill_states, dim3((n + 255) / 256), dim3(256), 0, e->stream, b->st, e->d_prompt, (int)base, (int)first_pos, n);
        for (size_t i = 0; i < b->plan_head; ++i) launch(b->plan[i], e->stream);
        HIP_TRY(hipGetLastError());
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
        if (n_tokens > 1) hipLaunchKernelGGL(k_rng_skip, dim3(1), dim3(1), 0, e->stream, e->d_sampler, (int)(n_tokens - 1));
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
    int rc = batch_set_state(e, tokens, pos, n_streams);
    if (rc) return rc;
    BatchCtx* b = e->batch;
    if ((rc = batch_enqueue_step(e))) return rc;
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
    int rc = batch_set_state(e, first_tokens, first_pos, n_streams);
    if (rc) return rc;
    BatchCtx* b = e->batch;
    for (int i = 0; i < n_streams; ++i)
        if ((size_t)first_pos[i] + n_steps > (size_t)b->ctx)
            return fail(Q3_ERR_ARG, "stream %d: first_pos %d + n_steps %zu exceeds seq_len %d", i, first_pos[i], n_steps, b->ctx);
    for (size_t k = 0; k < n_steps; ++k)
        if ((rc = batch_enqueue_step(e))) return rc;
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
    const int n = e->cfg.vocab_size, B = b->max_streams;
    const int blen = 4 * ((n + 4095) / 4096);
    size_t n2 = 1;
    while (n2 < (size_t)n) n2 <<= 1;
    const size_t scratch = (size_t)kSampThreads * blen;
    if (!b->d_sampler) {
        HIP_TRY(hipMalloc((void**)&b->d_sampler, sizeof(SamplerState) * B));
        HIP_TRY(hipMalloc((void**)&b->d_probs, 4 * scratch * B));
        HIP_TRY(hipMalloc((void**)&b->d_sp, 4 * scratch * B));
        HIP_TRY(hipMalloc((void**)&b->d_keys, 2 * 8 * n2 * B));
    }
    std::vector<SamplerState> h(B);
    for (int i = 0; i < B; ++i) h[i] = SamplerState{rng_seeds ? rng_seeds[i] : 0ull, temperature, topp, {0, 0, 0, 0}};
    HIP_TRY(hipMemcpy(b->d_sampler, h.data(), sizeof(SamplerState) * B, hipMemcpyHostToDevice));
    SampleArgs a{};
    a.logits = b->logits;
    a.n = n;
    a.blen = blen;
    a.probs = b->d_probs;
    a.keys = b->d_keys;
    a.sp = b->d_sp;
    a.ss = b->d_sampler;
    a.st = b->st;
    a.out_tokens = b->out_tokens;
    a.out_cap = b->out_cap;
    a.sb_logits = n;
    a.sb_scratch = (long long)scratch;
    a.sb_keys = 2 * (long long)n2;
    a.keys2_off = (long long)n2;
    a.pre_exp = dev_knob("Q3_SAMPLER_PRE_EXP", 1);
    b->sargs = a;
    const bool on = temperature != 0.0f;
    b->plan_streams = 0;                                  // the step's launches carry these arguments: re-plan on the next call
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

// Column sampler states and the draw scratch of up to kSpecMax columns (probs / sp / keys: ~5.3 MB per column at a 151,936-entry
// vocabulary), allocated by the first pass that samples -- greedy users of the context never pay for it -- and freed with it.
int spec_draw_alloc(q3_engine* e) {
    BatchCtx* b = e->batch;
    HIP_TRY(hipSetDevice(e->device));
    const int n = e->cfg.vocab_size;
    const int blen = 4 * ((n + 4095) / 4096);
    size_t n2 = 1;
    while (n2 < (size_t)n) n2 <<= 1;
    const size_t scratch = (size_t)kSampThreads * blen;
    HIP_TRY(hipMalloc((void**)&b->spec_samp, sizeof(SamplerState) * kSpecMax));
    HIP_TRY(hipMemsetAsync(b->spec_samp, 0, sizeof(SamplerState) * kSpecMax, e->stream));
    HIP_TRY(hipMalloc((void**)&b->spec_probs, 4 * scratch * kSpecMax));
    HIP_TRY(hipMalloc((void**)&b->spec_sp, 4 * scratch * kSpecMax));
    HIP_TRY(hipMalloc((void**)&b->spec_keys, 2 * 8 * n2 * kSpecMax));
    SampleArgs a{};
    a.logits = b->logits;
    a.n = n;
    a.blen = blen;
    a.probs = b->spec_probs;
    a.keys = b->spec_keys;
    a.sp = b->spec_sp;
    a.ss = b->spec_samp;
    a.st = b->st;
    a.out_tokens = e->d_out_tokens;      // never written: a column's State::step stays 0, and out_cap 0 closes the window
    a.out_cap = 0;
    a.sb_logits = n;
    a.sb_scratch = (long long)scratch;
    a.sb_keys = 2 * (long long)n2;
    a.keys2_off = (long long)n2;
    a.pre_exp = 1;
    b->spec_sargs = a;
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
    if (e->sampling && !e->batch->spec_samp && (rc = spec_draw_alloc(e))) return rc;
    return Q3_OK;
}

// One verify pass over a plan of n_plan columns, n_real <= n_plan of them live.  The result is left in b->h_spec.
int spec_pass(q3_engine* e, const int32_t* tokens, int n_real, int n_plan, size_t first_pos, float* logits_out) {
    BatchCtx* b = e->batch;
    int rc;
    HIP_TRY(hipSetDevice(e->device));
    if (b->plan_streams != n_plan || b->plan_kind != PlanKind::Verify || b->plan_draw != e->sampling)
        if ((rc = batch_build_plan(e, n_plan, PlanKind::Verify, e->sampling))) return rc;
    b->h_spec->first_pos = (int)first_pos;
    b->h_spec->n_real = n_real;
    for (int i = 0; i < kSpecMax; ++i) b->h_spec->tokens[i] = i < n_real ? tokens[i] : 0;
    HIP_TRY(hipMemcpyAsync(b->spec_io, b->h_spec, offsetof(SpecIO, n_accepted), hipMemcpyHostToDevice, e->stream));
    if ((rc = batch_enqueue_step(e))) return rc;
    HIP_TRY(hipMemcpyAsync(&b->h_spec->n_accepted, &b->spec_io->n_accepted, sizeof(SpecIO) - offsetof(SpecIO, n_accepted), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (logits_out) HIP_TRY(hipMemcpy(logits_out, b->logits, 4 * (size_t)e->cfg.vocab_size * (size_t)n_real, hipMemcpyDeviceToHost));
    return Q3_OK;
}

}  // namespace

extern "C" {

}  // extern "C"

namespace {

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
