// q3_plan_host.inc -- the launch lists of the batched entry points (included by q3_engine.hip, same translation unit).
//
// A Plan (q3_batch_host.inc) is a value.  batch_build_plan() makes one from the engine and the context without writing to either;
// plan_get() keeps the plans where their kind lives and builds on a miss; plan_enqueue() puts one on the stream; plans_drop() drops them.

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

// ---- the record launches (q3_score.h, q3_score_top.h): what q3_score_many / q3_score_top_many enqueue behind the classifier of a
// chunk and what a plan with records holds in front of its turn kernel.
// The scratch the four kernels work on, made here and nowhere else: on first use, at its full size (kScoreCols rows of exps; with
// `lists`, the k > 0 launches' part lists and counts at kScoreTopMax and kScoreTopParts), and never again while the context lives --
// so a captured plan's pointers hold whatever call comes next, and a call without lists makes none.
size_t record_exps_stride(const q3_engine* e) { return ((size_t)e->cfg.vocab_size + 3) & ~(size_t)3; }
int record_scratch(q3_engine* e, bool lists) {
    static_assert(kScoreCols == kColsMax, "a chunk and a pass are as wide as the classifier's output");
    BatchCtx* b = e->batch;
    int rc;
    HIP_TRY(hipSetDevice(e->device));
    if (!b->record_exps && (rc = b->record_exps.alloc((size_t)kScoreCols * record_exps_stride(e)))) return rc;
    if (lists && !b->record_part_keys) {
        // one group, committed whole
        DevMem<unsigned long long> keys; DevMem<int> above;
        if ((rc = keys.alloc((size_t)kScoreCols * kScoreTopMax * kScoreTopParts)) || (rc = above.alloc((size_t)kScoreCols * kScoreTopParts))) return rc;
        b->record_part_keys = std::move(keys); b->record_part_above = std::move(above);
    }
    return Q3_OK;
}
// The arguments of the four kernels over the classifier's output of the context and that scratch (record_scratch has run; nothing is
// written here).  nslots: the argmax keys the classifier launch leaves per row; parts: the slices per row of k_score_top_part.
int record_args(const q3_engine* e, bool lists, int nslots, int parts, RecordArgs& a) {
    const BatchCtx* b = e->batch;
    if (nslots < 1 || nslots > b->nslots) return fail(Q3_ERR_INTERNAL, "%d argmax slots of %d", nslots, b->nslots);
    if (parts < 1 || parts > kScoreTopParts) return fail(Q3_ERR_INTERNAL, "%d slices per row of %d", parts, kScoreTopParts);
    if (!b->record_exps || (lists && !b->record_part_keys)) return fail(Q3_ERR_INTERNAL, "record launches before record_scratch");
    a = RecordArgs{};
    a.logits = b->logits;
    a.slots = b->slots;
    a.exps = b->record_exps;
    a.part_keys = lists ? (unsigned long long*)b->record_part_keys : nullptr;
    a.part_above = lists ? (int*)b->record_part_above : nullptr;
    a.exps_stride = (long long)record_exps_stride(e);
    a.slot_stride = b->nslots;
    a.nslots = nslots;
    a.n = e->cfg.vocab_size;
    a.parts = parts;
    return Q3_OK;
}

// The launches over `rows` rows of source `src`, the top pair where a.part_keys stands, stated once.  put(ends_group, kernel, grid,
// block, a, src) enqueues or appends one; ends_group: the launch is the last of a group Q3_DEBUG_TIMING times (exps | sum | top).
template <class Src, class Put>
int record_launches(const RecordArgs& a, const Src& src, int rows, Put&& put) {
    int rc;
    if ((rc = put(true, k_score_exp<Src>, dim3(kScoreExpParts, (unsigned)rows), dim3(256), a, src))) return rc;
    if ((rc = put(true, k_score_sum<Src>, dim3((unsigned)rows), dim3(kSampThreads), a, src))) return rc;
    if (!a.part_keys) return Q3_OK;
    if ((rc = put(false, k_score_top_part<Src>, dim3((unsigned)a.parts, (unsigned)rows), dim3(256), a, src))) return rc;
    return put(true, k_score_top_merge<Src>, dim3((unsigned)rows), dim3(256), a, src);
}

// ---- the penalty state (q3_penalty.h, section 2p): what a plan under penalties points at, made here and nowhere else: on first use,
// at its full size, and never again while the context lives -- so a captured plan's pointers hold whatever call comes next.  Two
// groups, each committed whole: the rows, their keys and the setting (adj_alloc), which a table of section 2q needs too, and the
// counts on top (pen_alloc), which only penalties need.  The counts need no clearing: a request's first output clears its slot's.
// The setting goes to the device with the first group; q3_sampler_penalties rewrites that word alone.
int pen_ctl_upload(q3_engine* e) {
    const PenCtl h{e->pen_presence, e->pen_frequency};
    HIP_TRY(hipMemcpy(e->batch->pen_ctl, &h, sizeof(PenCtl), hipMemcpyHostToDevice));
    return Q3_OK;
}
// the rows, their slices' keys and the setting: what a table without penalties needs of it (section 2q), and no counts
int adj_alloc(q3_engine* e) {
    BatchCtx* b = e->batch;
    if (b->pen_ctl) return Q3_OK;
    int rc;
    HIP_TRY(hipSetDevice(e->device));
    const size_t V = (size_t)e->cfg.vocab_size;
    DevMem<float> rows; DevMem<unsigned long long> keys; DevMem<PenCtl> ctl;
    if ((rc = rows.alloc((size_t)kColsMax * V)) || (rc = keys.alloc((size_t)kColsMax * kPenSlices)) || (rc = ctl.alloc(1))) return rc;
    HIP_TRY(hipMemsetAsync(keys, 0, 8 * (size_t)kColsMax * kPenSlices, e->stream));
    b->pen_logits = std::move(rows); b->pen_slots = std::move(keys); b->pen_ctl = std::move(ctl);
    if (b->draw_cols) draw_args_pen(b->draw_cols, b->pen_logits);
    return pen_ctl_upload(e);
}
int pen_alloc(q3_engine* e) {
    BatchCtx* b = e->batch;
    if (b->pen_counts) return Q3_OK;
    int rc;
    if ((rc = adj_alloc(e))) return rc;
    DevMem<unsigned> counts;
    if ((rc = counts.alloc((size_t)b->max_streams * (size_t)e->cfg.vocab_size))) return rc;
    b->pen_counts = std::move(counts);
    return Q3_OK;
}
// The arguments of k_pen_apply and k_pen_count over the pass in flight (pen_alloc has run; nothing is written here), and of
// k_bias_apply and k_bias_count (bias_alloc has run: counts may be null here, those two take the counts from BiasCtl).  draw: the
// plan is a sampled one, whose columns carry a mode
PenArgs pen_args(const q3_engine* e, bool draw) {
    const BatchCtx* b = e->batch;
    PenArgs a{};
    a.logits = b->logits;
    a.pen_logits = b->pen_logits;
    a.counts = b->pen_counts;
    a.pen_slots = b->pen_slots;
    a.ctl = b->pen_ctl;
    a.cols = b->cols_ctl;
    a.draw = draw ? (const ColsDraw*)b->cols_draw : nullptr;
    a.st = b->st;
    a.col_slot = b->col_slot;
    a.n = e->cfg.vocab_size;
    a.max_streams = b->max_streams;
    return a;
}

// ---- the table of q3_logit_bias_set on the device (q3_bias.h, section 2q).  bias_alloc: what a plan of the adjusted form points at,
// made once -- the rows and keys it shares with the penalties, and the control block.  bias_call_begin: every generate call under a
// table, on the stream in front of its passes: the lists, their offsets and modes, the call's o_off with n_out behind it, the counts
// where penalties are set (null otherwise: none is allocated or read), and the control block that names them all.
int bias_alloc(q3_engine* e) {
    BatchCtx* b = e->batch;
    int rc;
    if ((rc = adj_alloc(e))) return rc;
    if (b->bias_ctl) return Q3_OK;
    DevMem<BiasCtl> ctl;
    if ((rc = ctl.alloc(1))) return rc;
    HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(BiasCtl), e->stream));
    b->bias_ctl = std::move(ctl);
    return Q3_OK;
}
int bias_call_begin(q3_engine* e, const int* o_off, size_t n_requests, size_t n_out_total) {
    BatchCtx* b = e->batch;
    // (a guide without a table, section 2r: one empty ADD list)
    static const BiasTable none{{}, {0u, 0u}, {(unsigned char)kBiasAdd}};
    const BiasTable& t = e->bias.n_lists() ? e->bias : none;
    int rc;
    const size_t n_lists = t.n_lists(), n_ent = t.entries.size();
    if ((rc = bias_alloc(e))) return rc;
    if (e->pen_on() && (rc = pen_alloc(e))) return rc;
    if ((rc = b->bias_entries.grow(std::max<size_t>(n_ent, 1), e->stream)) || (rc = b->bias_off.grow(n_lists + 1, e->stream)) ||
        (rc = b->bias_modes.grow(n_lists, e->stream)) || (rc = b->bias_ooff.grow(n_requests + 1, e->stream)))
        return rc;
    const int n_out = (int)n_out_total;
    if (n_ent) HIP_TRY(hipMemcpyAsync(b->bias_entries, t.entries.data(), sizeof(BiasEntry) * n_ent, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(b->bias_off, t.off.data(), 4 * (n_lists + 1), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(b->bias_modes, t.modes.data(), n_lists, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(b->bias_ooff, o_off, 4 * n_requests, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(b->bias_ooff + n_requests, &n_out, 4, hipMemcpyHostToDevice, e->stream));
    BiasCtl h{};
    h.entries = b->bias_entries;
    h.list_off = b->bias_off;
    h.modes = b->bias_modes;
    h.o_off = b->bias_ooff;
    h.counts = e->pen_on() ? (unsigned*)b->pen_counts : nullptr;
    h.n_lists = (int)n_lists;
    h.n_requests = (int)n_requests;
    HIP_TRY(hipMemcpyAsync(b->bias_ctl, &h, sizeof(BiasCtl), hipMemcpyHostToDevice, e->stream));
    return Q3_OK;
}

// ---- the guide of q3_guide_set on the device (q3_guide.h, section 2r).  guide_alloc: what a plan of the masked form points at on
// top of the adjusted form's, made once -- the control block and the slots' states.  guide_call_begin: every generate call under a
// guide, on the stream in front of its passes: bias_call_begin (the table of section 2q or one empty ADD list, o_off, the counts),
// the guide's table where the device does not hold it yet -- once per q3_guide_set and per batched state, never per call -- then
// start[] and the control block.
int guide_alloc(q3_engine* e) {
    BatchCtx* b = e->batch;
    int rc;
    if ((rc = bias_alloc(e))) return rc;
    if (b->guide_ctl) return Q3_OK;
    DevMem<GuideCtl> ctl; DevMem<int> state;
    if ((rc = ctl.alloc(1)) || (rc = state.alloc((size_t)b->max_streams))) return rc;
    HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(GuideCtl), e->stream));
    HIP_TRY(hipMemsetAsync(state, 0xff, sizeof(int) * (size_t)b->max_streams, e->stream));
    b->guide_ctl = std::move(ctl); b->guide_state = std::move(state);
    return Q3_OK;
}
int guide_call_begin(q3_engine* e, const int* o_off, size_t n_requests, size_t n_out_total) {
    BatchCtx* b = e->batch;
    const GuideTable& t = e->guide;
    int rc;
    if ((rc = guide_alloc(e)) || (rc = bias_call_begin(e, o_off, n_requests, n_out_total))) return rc;
    if (b->guide_serial != t.serial) {
        b->guide_serial = 0;
        if ((rc = b->guide_next.grow(t.next.size(), e->stream))) return rc;
        HIP_TRY(hipMemcpyAsync(b->guide_next, t.next.data(), sizeof(int16_t) * t.next.size(), hipMemcpyHostToDevice, e->stream));
        b->guide_serial = t.serial;
    }
    if ((rc = b->guide_start.grow(t.start.size(), e->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(b->guide_start, t.start.data(), sizeof(int) * t.start.size(), hipMemcpyHostToDevice, e->stream));
    GuideCtl h{};
    h.next = b->guide_next;
    h.start = b->guide_start;
    h.state = b->guide_state;
    h.n_states = (int)t.n_states;
    h.n_start = (int)t.start.size();
    HIP_TRY(hipMemcpyAsync(b->guide_ctl, &h, sizeof(GuideCtl), hipMemcpyHostToDevice, e->stream));
    return Q3_OK;
}

// ---- the sparse guide of q3_guide_set_sparse on the device (q3_guide_sparse.h, section 2s): guide_alloc and guide_call_begin over
// the compressed table.  The three arrays go up where the device does not hold this guide yet, start[] and the control block with
// every call.
int guide_sp_alloc(q3_engine* e) {
    BatchCtx* b = e->batch;
    int rc;
    if ((rc = bias_alloc(e))) return rc;
    if (b->guide_sp_ctl) return Q3_OK;
    DevMem<GuideSpCtl> ctl; DevMem<int> state;
    if ((rc = ctl.alloc(1)) || (rc = state.alloc((size_t)b->max_streams))) return rc;
    HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(GuideSpCtl), e->stream));
    HIP_TRY(hipMemsetAsync(state, 0xff, sizeof(int) * (size_t)b->max_streams, e->stream));
    b->guide_sp_ctl = std::move(ctl); b->guide_sp_state = std::move(state);
    return Q3_OK;
}
int guide_sp_call_begin(q3_engine* e, const int* o_off, size_t n_requests, size_t n_out_total) {
    BatchCtx* b = e->batch;
    const GuideSparse& t = e->guide_sp;
    int rc;
    if ((rc = guide_sp_alloc(e)) || (rc = bias_call_begin(e, o_off, n_requests, n_out_total))) return rc;
    if (b->guide_sp_serial != t.serial) {
        b->guide_sp_serial = 0;
        if ((rc = b->guide_sp_dflt.grow(t.dflt.size(), e->stream)) || (rc = b->guide_sp_off.grow(t.row_off.size(), e->stream)) ||
            (rc = b->guide_sp_edges.grow(std::max(t.edges.size(), (size_t)1), e->stream)))
            return rc;
        HIP_TRY(hipMemcpyAsync(b->guide_sp_dflt, t.dflt.data(), sizeof(int) * t.dflt.size(), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(b->guide_sp_off, t.row_off.data(), sizeof(uint32_t) * t.row_off.size(), hipMemcpyHostToDevice, e->stream));
        if (!t.edges.empty())
            HIP_TRY(hipMemcpyAsync(b->guide_sp_edges, t.edges.data(), sizeof(GuideEdge) * t.edges.size(), hipMemcpyHostToDevice, e->stream));
        b->guide_sp_serial = t.serial;
    }
    if ((rc = b->guide_sp_start.grow(t.start.size(), e->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(b->guide_sp_start, t.start.data(), sizeof(int) * t.start.size(), hipMemcpyHostToDevice, e->stream));
    GuideSpCtl h{};
    h.dflt = b->guide_sp_dflt;
    h.row_off = b->guide_sp_off;
    h.edges = b->guide_sp_edges;
    h.start = b->guide_sp_start;
    h.state = b->guide_sp_state;
    h.n_states = (int)t.n_states;
    h.n_start = (int)t.start.size();
    h.n_edges = (int)t.edges.size();
    HIP_TRY(hipMemcpyAsync(b->guide_sp_ctl, &h, sizeof(GuideSpCtl), hipMemcpyHostToDevice, e->stream));
    return Q3_OK;
}

// ---- the builder: the launches of key.n streams (Decode), block positions (Prefill, Verify; draw: Verify under the sampler),
// columns (Cols; draw: the sampled column plan) or columns of a dense block over the slots (SlotPrefill), appended to `out`.
// It reads the engine and the context and writes neither.
struct BlockView {              // the per-column buffers the layers of a plan work on
    float *x, *q, *qn, *kraw, *xb, *hb;
    int8_t* xq_p; float* xs_p; State* st; int* col_slot;
    float* att_pf; int att_pf_stride;
};
struct PlanBuilder {
    const q3_engine* const e;
    const PlanKey key;
    Plan& out;
    PlanBuilder(const q3_engine* e_, PlanKey key_, Plan& out_) : e(e_), key(key_), out(out_) {}

    const BatchCtx* const b = e->batch;
    const q3_config& c = e->cfg;
    const int n = key.n;
    // what the kind decides, once
    const bool cols = key.kind == PlanKind::Cols, slotpf = key.kind == PlanKind::SlotPrefill, verify = key.kind == PlanKind::Verify;
    const bool own_cache = key.kind == PlanKind::Prefill || verify;          // the positions of one sequence over the engine's own KV cache
    const bool block = own_cache || cols || slotpf;                          // columns may share a cache: all key rows enter it before any column attends
    const bool classifier = !(key.kind == PlanKind::Prefill || slotpf);      // Prefill: the classifier runs once, on the last position, through the single-stream launch; SlotPrefill: cache rows only
    const bool captured = classifier && !(e->flags & Q3_FLAG_NO_GRAPH);      // the layer-only plans are enqueued as they are
    float* const key_base = own_cache ? e->d_key : b->key;
    float* const value_base = own_cache ? e->d_value : b->value;
    const int S = own_cache ? c.seq_len : b->ctx;
    const long long kv_stride = own_cache ? 0 : (long long)b->kv_stream;
    const BlockView sc = scratch();

    const int dim = c.dim, L = c.n_layers, hd = c.head_dim, V = c.vocab_size, H = c.hidden_dim, G = c.group_size;
    const int ahd = c.n_heads * hd, kvd = c.n_kv_heads * hd;
    const int strict = (e->flags & Q3_FLAG_FAST) ? 0 : 1;
    const int NT = n <= 16 ? 1 : 2, NJ = G / 64;
    // dense prefill (round 3): more than 32 positions per weight pass -> every wave owns an output tile (k_pgemm)
    const bool dense = (own_cache || slotpf) && n > 32;
    // batched decode / short prefill blocks at group 64: in-lane accumulation for the residual launches (k_dgemm, round 4);
    // Q3_BATCH_DGEMM=0 keeps k_bgemm
    const bool dgemm = !dense && G == 64 && dev_knob("Q3_BATCH_DGEMM", 1) != 0;
    const int nptiles = (n + 15) / 16;
    const int att_tch = dev_knob("Q3_BATCH_ATT_TCH", 32);
    const int att_lds_max = dev_knob("Q3_ATT_LDS_MAX", 4096);
    const bool bq_spec = G == 64 && dev_knob("Q3_BQUANT_SPEC", 1) != 0;
    // the copies of k_spec_snapshot / k_spec_restore: up to (n - 1) rows of kv_dim floats per layer and cache, a float4 per thread
    const unsigned spec_grid = (unsigned)std::min<long>(8L * e->n_cu, std::max<long>(1, ((long)L * (kSpecMax - 1) * (kvd / 4) + kWG - 1) / kWG));
    int nslots_used = 0;         // argmax slots the classifier launch fills: what the tail launches read

    // the per-column buffers the layers work on: the context's own, or the dense block scratch of SlotPrefill
    BlockView scratch() const {
        // one list of names for both sources: BatchCtx and BlockScratch call their buffers alike
        const auto view = [](const auto& m) {
            BlockView s{};
            s.x = m.x; s.q = m.q; s.qn = m.qn; s.kraw = m.kraw; s.xb = m.xb; s.hb = m.hb;
            s.xq_p = m.xq_p; s.xs_p = m.xs_p; s.st = m.st; s.col_slot = m.col_slot;
            s.att_pf = m.att_pf; s.att_pf_stride = m.att_pf_stride;
            return s;
        };
        BlockView s = slotpf ? view(b->dense) : view(*b);
        if (!slotpf && !cols) s.col_slot = nullptr;
        return s;
    }

    template <class... KA, class... A>
    int add(Family fam, void (*kernel)(KA...), dim3 grid, dim3 blk, size_t smem, const A&... args) {
        Launch Ln;
        if (int rc = make_launch(Ln, fam, kernel, grid, blk, smem, args...)) return rc;
        out.launches.push_back(Ln);
        return Q3_OK;
    }
    // developer timeline: the cells of the launch about to be appended
    unsigned long long* stamp_cells() const { return b->stamps ? b->stamps + 96 * out.launches.size() : nullptr; }

    int quant(Family fam, int pro, const float* in, long long in_stride, int nn, const float* norm_w) {
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
            for (int p = (pro == PRO_QUANT ? 8 : 4); p > 1; p >>= 1)
                if (nn % (p * G) == 0 && nn / p >= 256 && nn / p <= 8 * kWG) { parts = p; break; }
        }
        size_t smem = gemv_smem_bytes(nn, G, 1, stage);
        if (parts > 1) {
            a.stamps = stamp_cells();
            const size_t slice = align16((size_t)(nn / parts)) + align16(4 * (size_t)(nn / parts / G));
            smem = slice + (stage ? 4 * (size_t)(term_floats(nn) + 128) : 0);
        }
        return add(fam, bquant_fn(pro, nn, parts, bq_spec), dim3((unsigned)parts, (unsigned)n), dim3(kWG), smem, a, qa);
    }

    int gemm(Family fam, int epi, const BatchCtx::PM& m, BGemmArgs a) {
        a.wq = b->pq + m.q_off;
        a.ws = b->ps + m.s_off;
        a.xq = sc.xq_p;
        a.xs = sc.xs_p;
        a.ng = m.ng;
        a.ntiles = m.ntiles;
        a.n_streams = n;
        a.st = sc.st;
        BGemmFn fn = nullptr;
        unsigned grid = 1, blk = 0;
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
            blk = kP2Threads;
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
            blk = kPgThreads;
        } else if ((fn = (dgemm && epi == EPI_RESID) ? pick_dgemm(m.ng, depth) : nullptr)) {
            // decode, group 64, residual launches (Wo, W2): every wave owns a (row tile, stream tile) accumulator tile for the whole
            // contraction (k_dgemm).  Same-box A/B on the 8B shape (profiles/r04_batch32_dgemm.md): the residual launches gain 3-4 % of
            // the step; QKV (11.6 vs 12.9 us), W1|W3 with the fused quantizer (27.7 vs 22.5 + 4.8 us) and the classifier (131-136 vs
            // 130 us) in this form do not beat k_bgemm
            grid = (unsigned)(((long)m.ntiles * NT + kDgWaves - 1) / kDgWaves);
            blk = (unsigned)kDgWaves * 64;
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
            blk = kBThreads;
            smem = bgemm_smem_bytes(RT, NT);
            if (epi == EPI_LOGITS) {
                if ((int)grid > b->nslots) return fail(Q3_ERR_HIP, "argmax slot capacity");
                a.slots = b->slots;
                a.nslots = b->nslots;
                nslots_used = (int)grid;
            }
            if (!(fn = Q3_BY_EPI(epi, pick_bgemm, RT, NT, NJ))) return fail(Q3_ERR_UNSUPPORTED, "no batched kernel for group size %d", G);
        }
        return add(fam, fn, dim3(grid), dim3(blk), smem, a);
    }

    // the attention of layer l: key rows into the cache (block plans), then the scores and the weighted values.  *packed: the
    // launch left Wo's quantized operand behind (the activation prologue rides in its epilogue)
    int attention(int l, bool* packed) {
        const size_t kv_off = (size_t)l * S * kvd;
        int rc;
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
                rc = add(F_ATTN, k_knorm_rope_blk, dim3((unsigned)((nvec + kKnbVec - 1) / kKnbVec)), dim3(256), knorm_blk_smem_bytes(), a, n, use_pf ? 1 : 0);
            } else {
                rc = add(F_ATTN, k_knorm_rope, dim3((unsigned)(c.n_kv_heads + (use_pf ? c.n_heads : 0)), (unsigned)n), dim3(64), 0, a);
            }
            if (rc) return rc;
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
            *packed = true;
            a.stamps = stamp_cells();
            // 8 positions per workgroup once that still gives every CU a workgroup
            const int npw = (dev_knob("Q3_PREFILL_ATT_NP", 0) == 8 || (dev_knob("Q3_PREFILL_ATT_NP", 0) == 0 && (long)c.n_kv_heads * ((n + 7) / 8) >= e->n_cu)) ? 8 : 4;
            return add(F_ATTN, attn_pf2_fn(kv_mul, npw), dim3((unsigned)c.n_kv_heads, (unsigned)((n + npw - 1) / npw)),
                       dim3((unsigned)attn_pf2_threads(kv_mul, npw)), attn_pf2_smem_bytes(), a);
        }
        if (gqa) {
            // one workgroup per (stream, kv head): K/V staged once for the kv_mul query heads sharing it
            a.att_global = nullptr;
            if (hd % G == 0 && dev_knob("Q3_BATCH_FUSE_XB_QUANT", 1)) {   // Wo's activation prologue rides in the epilogue
                a.pack_q = sc.xq_p;
                a.pack_s = sc.xs_p;
                a.group = G;
                *packed = true;
            }
            a.stamps = stamp_cells();
            // head_dim 128 with 2 or 4 query heads per kv head: staging and arithmetic on separate waves, two LDS tiles
            const bool gqa2 = hd == kG2Hd && (kv_mul == 2 || kv_mul == 4) && attn_gqa2_smem_bytes(kv_mul, S) <= 150 * 1024 && dev_knob("Q3_BATCH_ATT_GQA2", 1);
            return add(F_ATTN, attn_gqa_fn(gqa2, hd, kv_mul), dim3((unsigned)c.n_kv_heads, (unsigned)n),
                       dim3(gqa2 ? (unsigned)kG2Threads : (unsigned)(kv_mul + 1) * 64),
                       gqa2 ? attn_gqa2_smem_bytes(kv_mul, S) : attn_gqa_smem_bytes(hd, kv_mul, S), a);
        }
        return add(F_ATTN, k_attn_streams, dim3((unsigned)c.n_heads, (unsigned)n), dim3(kWG), attn_smem_bytes(hd, a.att_global ? 0 : S, a.tch), a);
    }

    int layer(int l) {
        const size_t kv_off = (size_t)l * S * kvd;
        int rc;
        if ((rc = quant(F_QKV, l == 0 ? PRO_EMBED_NORM : PRO_NORM, sc.x, dim, dim, e->rms_att + (size_t)l * dim))) return rc;
        BGemmArgs qkv{};
        qkv.out0 = sc.q; qkv.out0_stride = ahd;
        qkv.out1 = sc.kraw; qkv.out1_stride = kvd;
        qkv.out2 = value_base + kv_off; qkv.out2_stride = kv_stride;
        qkv.rows0 = ahd; qkv.rows1 = kvd; qkv.pos_stride = kvd;
        qkv.col_slot = sc.col_slot;
        if ((rc = gemm(F_QKV, EPI_QKV, b->m_qkv[l], qkv))) return rc;
        bool packed = false;
        if ((rc = attention(l, &packed))) return rc;
        if (!packed && (rc = quant(F_WO, PRO_QUANT, sc.xb, ahd, ahd, nullptr))) return rc;
        BGemmArgs resid{};
        resid.out0 = sc.x; resid.out0_stride = dim;
        if ((rc = gemm(F_WO, EPI_RESID, b->m_wo[l], resid))) return rc;
        if ((rc = quant(F_W13, PRO_NORM, sc.x, dim, dim, e->rms_ffn + (size_t)l * dim))) return rc;
        BGemmArgs ffn{};
        ffn.out0 = sc.hb; ffn.out0_stride = H;
        if ((rc = gemm(F_W13, EPI_SWIGLU, b->m_w13[l], ffn))) return rc;
        if ((rc = quant(F_W2, PRO_QUANT, sc.hb, H, H, nullptr))) return rc;
        return gemm(F_W2, EPI_RESID, b->m_w2[l], resid);
    }

    int classify() {
        if (int rc = quant(F_LMHEAD, PRO_NORM, b->x, dim, dim, e->rms_final)) return rc;
        BGemmArgs a{};
        a.out0 = b->logits; a.out0_stride = V;
        return gemm(F_LMHEAD, EPI_LOGITS, b->m_cls, a);
    }

    // Sampler::sample of every column on the block's logits, exactly the batched decode's launches (one workgroup per column
    // behind the element-wise passes spread over the chip), behind the per-column maximum they read.  Columns that do not draw
    // (interior prompt positions, pads, temperature-0 slots of a column pass) return at once in both sampler launches
    int draw_columns() {
        if (int rc = colmax()) return rc;
        return draw(b->draw_cols);
    }
    // State::argmax of every column: the fold of the classifier's argmax slots, or under penalties of the penalised row's slices
    int colmax() {
        if (key.pen) return add(F_NEXT, k_spec_colmax, dim3(1), dim3(kWG), 0, b->st, b->pen_slots, kPenSlices, kPenSlices, n);
        return add(F_NEXT, k_spec_colmax, dim3(1), dim3(kWG), 0, b->st, b->slots, b->nslots, nslots_used, n);
    }
    // the draws of a site's first n columns, plain or top-k as the key says (draw_launches); under penalties over the penalised rows
    int draw(const DrawSite& site) {
        if (key.pen && !site.pen.logits) return fail(Q3_ERR_INTERNAL, "a sampled plan under penalties before draw_args_pen");
        const TopkArgs t = e->topk_args(draw_site_args(site, key.pen));
        return draw_launches(site, n, kDrawExpParts, key.topk ? &t : nullptr, [&](auto kernel, dim3 grid, dim3 blk, size_t smem, const auto& a) {
            return add(F_NEXT, kernel, grid, blk, smem, a);
        }, key.pen);
    }
    // the penalised rows of the emitting columns and their slices' largest keys, behind the classifier (pen_alloc has run)
    // (kPenAdj: the adjusted rows of section 2q in their place, bias_alloc has run)
    // (kPenGuide: the masked rows of section 2r, guide_alloc has run; kPenGuideSp: of section 2s, guide_sp_alloc has run)
    int penalize() {
        if (!b->pen_ctl) return fail(Q3_ERR_INTERNAL, "a plan under penalties before pen_alloc");
        if (key.pen == kPenGuide) {
            if (!b->bias_ctl || !b->guide_ctl) return fail(Q3_ERR_INTERNAL, "a plan of the masked form before guide_alloc");
            return add(F_NEXT, k_guide_apply, dim3(kPenSlices, (unsigned)n), dim3(kPenThreads), 0, pen_args(e, key.draw), (const BiasCtl*)b->bias_ctl,
                       (const GuideCtl*)b->guide_ctl);
        }
        if (key.pen == kPenGuideSp) {
            if (!b->bias_ctl || !b->guide_sp_ctl) return fail(Q3_ERR_INTERNAL, "a plan of the sparse masked form before guide_sp_alloc");
            return add(F_NEXT, k_guide_sp_apply, dim3(kPenSlices, (unsigned)n), dim3(kPenThreads), 0, pen_args(e, key.draw), (const BiasCtl*)b->bias_ctl,
                       (const GuideSpCtl*)b->guide_sp_ctl);
        }
        if (key.pen == kPenAdj) {
            if (!b->bias_ctl) return fail(Q3_ERR_INTERNAL, "a plan of the adjusted form before bias_alloc");
            return add(F_NEXT, k_bias_apply, dim3(kPenSlices, (unsigned)n), dim3(kPenThreads), 0, pen_args(e, key.draw), (const BiasCtl*)b->bias_ctl);
        }
        return add(F_NEXT, k_pen_apply, dim3(kPenSlices, (unsigned)n), dim3(kPenThreads), 0, pen_args(e, key.draw));
    }

    // the records of the columns the turn kernel is about to commit (PassRows, q3_genlp.h; genlp_alloc has run, and plan_get has
    // made the scratch): the draws are done, the pass's ColsCtl::n_live / out[] and, sampled, ColsDraw::mode[] still stand
    int gen_logprobs() {
        if (!b->genlp_ctl) return fail(Q3_ERR_INTERNAL, "a plan with records before genlp_alloc");
        RecordArgs a;
        if (int rc = record_args(e, key.genlp == kGenlpTop, nslots_used, kScoreTopParts, a)) return rc;
        const PassRows src{b->cols_ctl, key.draw ? (const ColsDraw*)b->cols_draw : nullptr, b->st, b->genlp_ctl, key.pen != kPenOff ? 1 : 0};
        return record_launches(a, src, n, [&](bool, auto kernel, dim3 grid, dim3 blk, const RecordArgs& ra, const PassRows& rs) {
            return add(F_NEXT, kernel, grid, blk, 0, ra, rs);
        });
    }

    // what follows the classifier
    int tail() {
        int rc;
        if (verify) {
            // greedy: the accepted prefix from the argmax slots; sampled: from the draws, over the column sampler states
            // k_spec_sampler_states set up
            if (key.draw) {
                if ((rc = draw_columns())) return rc;
                rc = add(F_NEXT, k_spec_commit_draw, dim3(1), dim3(64), 0, b->spec_io, b->st, b->draw_cols.ss, e->d_state, e->draw.ss, e->d_out_tokens, e->out_cap);
            } else {
                rc = add(F_NEXT, k_spec_commit, dim3(1), dim3(kWG), 0, b->spec_io, b->slots, b->nslots, nslots_used, e->d_state, e->d_out_tokens, e->out_cap);
            }
            if (rc) return rc;
            return add(F_NEXT, k_spec_restore, dim3(spec_grid), dim3(kWG), 0, b->spec_io, e->d_key, e->d_value, e->d_value_t, b->spec_snap, L, c.seq_len, kvd);
        }
        if (cols) {
            // sampled: the draws over the column sampler states k_cols_turn_draw set up
            // under penalties (section 2p): the draws and the turn kernel take the penalised rows and their slices' keys; the records
            // stay on the raw rows, their target alone is the token committed from the penalised ones (a greedy plan with records
            // gets it from State::argmax as a sampled one does)
            if (key.pen && (rc = penalize())) return rc;
            if (key.draw && (rc = draw_columns())) return rc;
            if (key.pen && key.genlp && !key.draw && (rc = colmax())) return rc;
            if (key.genlp && (rc = gen_logprobs())) return rc;
            if (key.pen == kPenOn && (rc = add(F_NEXT, k_pen_count, dim3(1), dim3(64), 0, pen_args(e, key.draw)))) return rc;
            if (key.pen == kPenAdj && (rc = add(F_NEXT, k_bias_count, dim3(1), dim3(64), 0, pen_args(e, key.draw), (const BiasCtl*)b->bias_ctl))) return rc;
            if (key.pen == kPenGuide &&
                (rc = add(F_NEXT, k_guide_step, dim3(1), dim3(64), 0, pen_args(e, key.draw), (const BiasCtl*)b->bias_ctl, (const GuideCtl*)b->guide_ctl)))
                return rc;
            if (key.pen == kPenGuideSp &&
                (rc = add(F_NEXT, k_guide_sp_step, dim3(1), dim3(64), 0, pen_args(e, key.draw), (const BiasCtl*)b->bias_ctl, (const GuideSpCtl*)b->guide_sp_ctl)))
                return rc;
            if (!key.draw && key.pen) return add(F_NEXT, k_cols_turn, dim3(1), dim3(kWG), 0, b->cols_ctl, b->pen_slots, kPenSlices, kPenSlices, b->st, b->col_slot);
            if (!key.draw) return add(F_NEXT, k_cols_turn, dim3(1), dim3(kWG), 0, b->cols_ctl, b->slots, b->nslots, nslots_used, b->st, b->col_slot);
            return add(F_NEXT, k_cols_turn_draw, dim3(1), dim3(kWG), 0, b->cols_ctl, b->cols_draw, b->draw_cols.ss, b->st, b->col_slot);
        }
        if ((rc = add(F_NEXT, k_next_batch, dim3((unsigned)n), dim3(kWG), 0, b->st, b->slots, b->nslots, nslots_used, b->out_tokens, b->out_cap))) return rc;
        if (!b->sampling) return Q3_OK;
        // Sampler::sample per stream on the logits of this step (one workgroup per stream), behind its element-wise passes spread
        // over the chip
        return draw(b->draw_decode);
    }

    int build() {
        if (dense && G != 64) return fail(Q3_ERR_UNSUPPORTED, "dense prefill needs group_size 64");
        int rc;
        if (verify) {
            if ((rc = add(F_NEXT, k_spec_snapshot, dim3(spec_grid), dim3(kWG), 0, b->st, b->spec_io, n, e->d_key, e->d_value, b->spec_snap, L, c.seq_len, kvd))) return rc;
            if (key.draw && (rc = add(F_NEXT, k_spec_sampler_states, dim3(1), dim3(64), 0, b->spec_io, n, e->draw.ss, b->draw_cols.ss, b->st))) return rc;
        }
        for (int l = 0; l < L; ++l)
            if ((rc = layer(l))) return rc;
        out.head = out.launches.size();
        if (!classifier) return Q3_OK;
        if ((rc = classify())) return rc;
        if ((rc = tail())) return rc;
        if (!captured) return Q3_OK;
        return out.graph.capture(e->stream, [&] {
            for (const Launch& K : out.launches) launch(K, e->stream);
            return Q3_OK;
        });
    }
};

// A failed build, a failed capture included, leaves `out` empty.
int batch_build_plan(const q3_engine* e, PlanKey key, Plan& out) {
    out = Plan{};
    const int rc = PlanBuilder(e, key, out).build();
    if (rc) out = Plan{};
    return rc;
}

int cols_width_index(int n) {
    int w = 0;
    while (kColsWidths[w] < n) ++w;
    return w;
}

// The plan of `key`, from where its kind lives: the one step slot (Decode, Prefill, Verify: replaced when the key changes -- the
// tail widths of a prefill are arbitrary), the column plans by records form, sampler and width (key.n is one of kColsWidths; kept
// until q3_batch_init starts over) or the dense block plans by width (kept until dense_att_grow drops them).  Built on a miss, stored
// only on success: a shape the kernels refuse is refused again by the next call.
int plan_get(q3_engine* e, PlanKey key, Plan** out) {
    BatchCtx* b = e->batch;
    Plan* home = &b->step;
    bool hit;
    // the engine's top_k holds wherever the plan draws: the sampled Verify and Cols plans, and the Decode plan under the batch sampler
    key.topk = e->top_k > 0 && (key.draw || (key.kind == PlanKind::Decode && b->sampling));
    if (key.kind != PlanKind::Cols) { key.genlp = kGenlpOff; key.pen = kPenOff; }
    if (key.genlp < kGenlpOff || key.genlp >= kGenlpForms) return fail(Q3_ERR_INTERNAL, "plan form %d", key.genlp);
    if (key.pen < kPenOff || key.pen >= kPenForms) return fail(Q3_ERR_INTERNAL, "plan form %d", key.pen);
    if (key.kind == PlanKind::Cols) {
        home = &b->cols_plans[key.pen][key.genlp][key.draw ? (key.topk ? 2 : 1) : 0][cols_width_index(key.n)];
        hit = !home->launches.empty();
    } else if (key.kind == PlanKind::SlotPrefill) {
        if (key.n <= kColsMax || key.n > b->dense.cap)
            return fail(Q3_ERR_ARG, "a dense block of %d columns does not fit the block scratch (33..%d columns)", key.n, b->dense.cap);
        auto it = b->dense_plans.find(key.n);
        if ((hit = it != b->dense_plans.end())) home = &it->second;
    } else {
        hit = !home->launches.empty() && b->step_key == key;
    }
    if (!hit) {
        HIP_TRY(hipSetDevice(e->device));
        // the scratch a plan with records points at exists before the plan does
        if (key.genlp != kGenlpOff)
            if (int rc = record_scratch(e, key.genlp == kGenlpTop)) return rc;
        // ... and so does the penalty state a plan under penalties points at
        if (key.pen)
            if (int rc = key.pen == kPenGuideSp ? guide_sp_alloc(e) : key.pen == kPenGuide ? guide_alloc(e) : (key.pen == kPenAdj ? bias_alloc(e) : pen_alloc(e)))
                return rc;
        Plan built;
        if (int rc = batch_build_plan(e, key, built)) return rc;
        if (key.kind == PlanKind::SlotPrefill) home = &b->dense_plans[key.n];
        *home = std::move(built);
        if (home == &b->step) b->step_key = key;
    }
    *out = home;
    return Q3_OK;
}

// the first n_launches launches of a plan (all of them: its graph, where it has one) on the engine's stream
int plan_enqueue(q3_engine* e, const Plan& p, size_t n_launches) {
    if (p.graph && n_launches >= p.launches.size()) return p.graph.launch(e->stream);
    for (size_t i = 0; i < n_launches && i < p.launches.size(); ++i) launch(p.launches[i], e->stream);
    HIP_TRY(hipGetLastError());
    return Q3_OK;
}

// the launches [first, end) of a plan as they are, never its graph: q3_score_many runs the classifier of a column plan,
// [Plan::head, Plan::head + 2), behind a block that ran other layers
int plan_enqueue_range(q3_engine* e, const Plan& p, size_t first, size_t end) {
    if (first > end || end > p.launches.size()) return fail(Q3_ERR_INTERNAL, "launches [%zu, %zu) of a plan of %zu", first, end, p.launches.size());
    for (size_t i = first; i < end; ++i) launch(p.launches[i], e->stream);
    HIP_TRY(hipGetLastError());
    return Q3_OK;
}

// Plans carry the pointers and strides they were built with: whoever replaces what the step plan's launches carry (the batch sampler's
// arguments, the score rows of a prefill-only context) drops the step plan; whoever frees the dense scratch's score rows, the dense plans.
void plans_drop(BatchCtx* b, PlanDrop what) {
    if (what == PlanDrop::Step) b->step = Plan{};
    else b->dense_plans.clear();
}

}  // namespace
