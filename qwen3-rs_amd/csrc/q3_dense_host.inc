// q3_dense_host.inc -- dense blocks over the per-stream KV caches (include/qwen3_hip.h section 2g; included by q3_engine.hip between
// q3_batch_host.inc and q3_cols_host.inc, same translation unit).
//
// q3_prefill_batched moves a prompt through the dense kernels (k_bquant, k_pgemm / k_pgemm3, k_knorm_rope_blk, k_attn_pf2) in blocks
// of up to Q3_PREFILL_M positions, into the engine's single cache.  Here the columns of such a block are runs of several slots of
// the batched state: every column's cache base comes from a slot table as long as the block (PlanKind::SlotPrefill), so a server
// holding eight 256-token prompts runs them as one 2,048-column block.  This file is the block itself: how runs are packed into
// blocks (dense_pack_run, the rule the header states), the scratch of a block beside the 32-column one, the plans by block width
// and the launch of one block.  The entry points and the loop that mixes blocks with column passes are in q3_cols_host.inc.

namespace {

// The packing rule of q3_dense_pack: emit(block, first column, run, offset in the run, columns) for every piece, in order.
template <class Emit>
void dense_pack_run(const size_t* run_len, size_t n_runs, int block_cap, Emit&& emit, q3_dense_stats& st) {
    st = q3_dense_stats{0, 0, 0};
    uint64_t block = 0;
    int end = 0, live = 0;                       // of the current block: the column behind its last piece, its live columns
    auto close = [&]() {
        if (live == 0) return;
        st.blocks++;
        st.live_columns += (uint64_t)live;
        st.pad_columns += (uint64_t)(((end + 7) & ~7) - live);
        ++block;
        end = live = 0;
    };
    for (size_t r = 0; r < n_runs; ++r) {
        size_t off = 0;
        while (off < run_len[r]) {
            int start = (end + 7) & ~7;
            if (start >= block_cap) {            // nothing left in the block
                close();
                start = 0;
            }
            const int take = (int)std::min<size_t>(run_len[r] - off, (size_t)(block_cap - start));
            emit(block, start, r, off, take);
            off += (size_t)take;
            end = start + take;
            live += take;
            if (off < run_len[r]) close();       // the rest of the run is the first piece of the next block
        }
    }
    close();
}

// The blocks of dense_pack_run as values: what the walks that enqueue them consume (embed_walk, q3_embed_host.inc; dense_job_add,
// q3_cols_host.inc).  A piece: columns [col0, col0 + len) of its block hold positions [off, off + len) of run `run`.  A block: its
// columns up to a multiple of 8 behind its last piece, whether that is more than a column pass holds (wide: a PlanKind::SlotPrefill
// block; otherwise a pass of its live columns), and its pieces [p0, p0 + np) in column order.
struct DensePiece { int col0; size_t run, off; int len; };
struct DenseBlock { int n; bool wide; size_t p0, np; };
struct DenseBlocks {
    std::vector<DensePiece> pieces;
    std::vector<DenseBlock> blocks;
    q3_dense_stats stats;
};
DenseBlocks dense_blocks(const size_t* run_len, size_t n_runs, int block_cap) {
    DenseBlocks d;
    dense_pack_run(run_len, n_runs, block_cap, [&](uint64_t block, int col0, size_t run, size_t off, int len) {
        if (block == d.blocks.size()) d.blocks.push_back(DenseBlock{0, false, d.pieces.size(), 0});
        DenseBlock& bl = d.blocks.back();
        bl.n = (col0 + len + 7) & ~7;
        bl.wide = bl.n > kColsMax;
        bl.np++;
        d.pieces.push_back(DensePiece{col0, run, off, len});
    }, d.stats);
    return d;
}

int dense_pack_check(const size_t* run_len, size_t n_runs, int block_cap) {
    if (!run_len || n_runs == 0) return fail(Q3_ERR_ARG, "null or empty run list");
    if (block_cap < 16 || block_cap % 16 != 0) return fail(Q3_ERR_ARG, "block_cap %d must be a multiple of 16 and at least 16", block_cap);
    for (size_t r = 0; r < n_runs; ++r)
        if (run_len[r] == 0) return fail(Q3_ERR_ARG, "run %zu is empty", r);
    return Q3_OK;
}

// the shapes the dense kernels take: what q3_prefill_batched needs for k_pgemm and k_attn_pf2
bool dense_capable(const q3_engine* e) {
    const q3_config& c = e->cfg;
    const int kv_mul = c.n_heads / c.n_kv_heads;
    return c.group_size == 64 && c.head_dim == kG2Hd && (kv_mul == 2 || kv_mul == 4);
}
// columns per block: Q3_PREFILL_M as for q3_prefill_batched; a shape the dense kernels refuse is walked 32 columns at a time.
// Read once per batched state, by its first dense call: every later call packs for the width the scratch was (or will be)
// allocated with, whatever the variable says by then -- as q3_prefill_batched walks by the cap of its allocation.
int dense_block_cap(q3_engine* e) {
    BatchCtx* b = e->batch;
    if (!b->dense_cap) {
        const int M = prefill_block_cap(e);
        b->dense_cap = dense_capable(e) ? M : std::min(M, (int)kColsMax);
    }
    return b->dense_cap;
}

// The scratch of a dense block over the slots, on first use: the per-column buffers of batch_alloc for dense_block_cap() columns.
// The 32-column scratch, the kept decode / column plans and their graphs are not touched.
int dense_scratch_get(q3_engine* e) {
    BatchCtx* b = e->batch;
    if (b->dense.cap) return Q3_OK;
    const q3_config& c = e->cfg;
    const size_t C = (size_t)dense_block_cap(e), dim = c.dim, H = c.hidden_dim, G = c.group_size;
    const size_t ahd = (size_t)c.n_heads * c.head_dim, kvd = (size_t)c.n_kv_heads * c.head_dim;
    const size_t maxn = std::max(std::max(H, ahd), dim), nt = (C + 15) / 16;
    const size_t bytes = 4 * C * (dim + 3 * ahd + kvd + H) + nt * 16 * maxn + 4 * nt * 16 * (maxn / G) + (sizeof(State) + 4) * C;
    HIP_TRY(hipSetDevice(e->device));
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    if (bytes > free_b)
        return fail(Q3_ERR_HIP, "dense slot prefill: %zu MiB of block scratch for blocks of %zu columns do not fit (%zu MiB free): lower Q3_PREFILL_M",
                    bytes >> 20, C, free_b >> 20);
    BlockScratch d;              // built here, committed whole: a failure frees what it got on the way out
    if (d.x.alloc(C * dim) || d.q.alloc(C * ahd) || d.qn.alloc(C * ahd) || d.kraw.alloc(C * kvd) || d.xb.alloc(C * ahd) || d.hb.alloc(C * H) ||
        d.xq_p.alloc(nt * 16 * maxn) || d.xs_p.alloc(nt * 16 * (maxn / G)) || d.st.alloc(C) || d.col_slot.alloc(C)) {
        (void)hipGetLastError();
        return fail(Q3_ERR_HIP, "dense slot prefill: allocating %zu MiB of block scratch for blocks of %zu columns failed: lower Q3_PREFILL_M", bytes >> 20, C);
    }
    d.cap = (int)C;
    b->dense = std::move(d);
    HIP_TRY(hipMemsetAsync(b->dense.x, 0, 4 * C * dim, e->stream));
    HIP_TRY(hipMemsetAsync(b->dense.xq_p, 0, nt * 16 * maxn, e->stream));           // columns past a block's end: finite operands
    HIP_TRY(hipMemsetAsync(b->dense.xs_p, 0, 4 * nt * 16 * (maxn / G), e->stream));
    HIP_TRY(hipMemsetAsync(b->dense.st, 0, sizeof(State) * C, e->stream));
    HIP_TRY(hipMemsetAsync(b->dense.col_slot, 0, 4 * C, e->stream));
    return Q3_OK;
}

// score rows of k_attn_pf2 for blocks whose columns attend over up to `max_end` positions: [column][head][context, rounded up],
// grown as q3_prefill_batched grows its own.  The kept block plans carry pointer and stride: they go with the old buffer.
int dense_att_grow(q3_engine* e, size_t max_end) {
    BlockScratch& d = e->batch->dense;
    return att_rows_grow(e, d.att_pf, d.att_pf_stride, (size_t)d.cap, (int)((max_end + 255) & ~(size_t)255), PlanDrop::Dense, "dense slot prefill", "columns");
}

// one block: the states and the slot table of its n columns from the device run table, then the layers (the kept
// PlanKind::SlotPrefill plan of its width)
int dense_enqueue_block(q3_engine* e, const Plan& plan, const DenseRun* d_runs, int n_runs, int n, const int32_t* d_prompts) {
    const BlockScratch& d = e->batch->dense;
    if (n > d.cap) return fail(Q3_ERR_ARG, "a dense block of %d columns does not fit the block scratch (%d columns)", n, d.cap);
    hipLaunchKernelGGL(k_dense_states, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, d.st, d.col_slot, d_runs, n_runs, d_prompts, n);
    return plan_enqueue(e, plan);
}

}  // namespace

extern "C" {

int q3_dense_pack(const size_t* run_len, size_t n_runs, int block_cap, int32_t* table, size_t cap, size_t* n_entries, q3_dense_stats* stats) {
    g_err[0] = 0;
    int rc;
    if ((rc = dense_pack_check(run_len, n_runs, block_cap))) return rc;
    size_t n = 0;
    q3_dense_stats st;
    dense_pack_run(run_len, n_runs, block_cap, [&](uint64_t block, int col0, size_t run, size_t off, int) {
        if (table && n < cap) {
            table[4 * n + 0] = (int32_t)block;
            table[4 * n + 1] = col0;
            table[4 * n + 2] = (int32_t)run;
            table[4 * n + 3] = (int32_t)off;
        }
        ++n;
    }, st);
    if (n_entries) *n_entries = n;
    if (stats) *stats = st;
    if (table && n > cap) return fail(Q3_ERR_ARG, "the packing has %zu pieces, the table holds %zu", n, cap);
    return Q3_OK;
}

}  // extern "C"
