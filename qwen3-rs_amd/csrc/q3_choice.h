// q3_choice.h -- the logits of a few candidate tokens behind the prompts that end in a block (include/qwen3_hip.h section 2k).
//
// A block of PlanKind::SlotPrefill, or the layers of a column plan, leaves the last layer's residual of every column in the block
// scratch x[column][dim].  A reranker or a multiple-choice evaluator reads k rows of the classifier behind a prompt's last token and
// nothing else: one workgroup per (prompt that ENDS in the block, part of its candidate list) restates the single-stream classifier
// launch (k_gemv<PRO_NORM, EPI_LOGITS>, q3_gemv.h) for those rows.  No row of the classifier that is not a candidate is read.
#pragma once

namespace q3 {

constexpr int kChoicePart = 32;     // candidates per workgroup (grid y); profiles/choice.md says what was tried
constexpr int kChoiceRows = 4;      // rows of the matrix a wave holds in flight: 4 rows x kChoiceJ loads of 16 bytes per lane
constexpr int kChoiceJ = kProSlots; // 1 KiB chunks of a row: dim <= 1024 * kProSlots, what the PRO_NORM prologue holds in registers

struct ChoiceArgs {
    const EmbedRow* rows;    // {column of the prompt's last token, request}: the gather table of the block
    const float* x;          // the block's residuals, stride n
    const float* norm_w;     // the final norm's weight
    const int8_t* wq;        // the classifier matrix [vocab][n] and its scales [vocab][n / group]
    const float* ws;
    const int32_t* cand;     // the candidate ids, checked by the host: [k], or [n_requests][k] with cand_stride == k
    float* out;              // [n_requests][k]
    long long cand_stride;
    int n, group, k;
};
inline size_t choice_smem_bytes(int n, int group) { return gemv_smem_bytes(n, group, kChoiceRows, true); }

// grid = (rows of the table, parts of kChoicePart candidates).  For its row {col, req} and the candidates j of its part, c = cand_req[j]:
//   xq, xs   = the PRO_NORM prologue of k_gemv over x[col]: exact sequential sum of squares, f = 1 / sqrt(ss / n + eps),
//              y_i = w_i * (f * x_i), per group of G  xs = max|y| / 127, xq_i = quant_round_i8(y_i / xs), zeros under a zero scale
//              -- gemv_prologue_issue / finish themselves, called as k_bquant calls them; every part repeats it (k_bquant_split)
//   d_g      = sum over the group of wq[c][i] * xq[i], int32, exact                                  (sdot4, lpg_sum)
//   t_g      = ((float)d_g * ws[c][g]) * xs[g]                                                       (q3_gemv.h compute_tile)
//   out[req][j] = ordered_row_sum(t, n / G): groups ascending from t_0
// which is what q3_forward puts at logits[c].  The four waves take the part's candidates round-robin, kChoiceRows of them at a time:
// a lane reads 16 consecutive bytes of every 1 KiB chunk of a row, so a wave's load is one coalesced KiB, and the loads of the
// kChoiceRows rows (independent of each other and of the prologue) are requested together, in front of the prologue.
// Bounds: col, req and the candidate ids come from the host (col < the block's columns, req < n_requests, 0 <= c < vocab); nothing
// the model computed becomes an address.  A workgroup reads x[col][0 .. n), w[0 .. n), wq[c][0 .. n), ws[c][0 .. n / G) and writes
// out[req][j] for j < k.  Dynamic LDS: choice_smem_bytes(n, group).
__global__ __launch_bounds__(kWG) void k_choice_rows(const ChoiceArgs c) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const EmbedRow R = c.rows[blockIdx.x];
    const int n = c.n, G = c.group, ng = n / G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nchunks = n >> 4, lpg = G >> 4;                // 16-byte pieces of a row; lanes that share a quantization group
    const int lpg_shift = __builtin_ctz(lpg);
    const int32_t* cand = c.cand + (size_t)R.req * c.cand_stride;
    float* out = c.out + (size_t)R.req * c.k;
    const int j_end = min(c.k, ((int)blockIdx.y + 1) * kChoicePart);
    const GemvSmem sm = gemv_carve(smem_raw, n, G, kChoiceRows, true);
    float* term = sm.term + (size_t)wave * kChoiceRows * ng;

    v4i w[kChoiceRows][kChoiceJ];
    float sc[kChoiceRows][kChoiceJ];
    // candidate r of the wave's batch that begins at j0 is j0 + kWaves * r; one past the end re-reads the last live row (nothing is stored)
    auto load = [&](int j0) {
#pragma unroll
        for (int r = 0; r < kChoiceRows; ++r) {
            const size_t row = (size_t)cand[min(j0 + kWaves * r, j_end - 1)];
            const int8_t* wr = c.wq + row * (size_t)n;
            const float* sr = c.ws + row * (size_t)ng;
#pragma unroll
            for (int j = 0; j < kChoiceJ; ++j) {
                const int cc = min(lane + 64 * j, nchunks - 1);
                if (64 * j < nchunks) {                      // wave-uniform
                    w[r][j] = ((const v4i*)wr)[cc];
                    sc[r][j] = sr[cc >> lpg_shift];
                }
            }
        }
    };

    int j0 = (int)blockIdx.y * kChoicePart + wave;
    const bool any = j0 < j_end;
    if (any) load(j0);

    GemvArgs a{};
    a.in = c.x + (size_t)R.col * n;
    a.norm_w = c.norm_w;
    a.n = n;
    a.group = G;
    a.strict = 1;
    ProRegs<PRO_NORM> pr;
    gemv_prologue_issue<PRO_NORM>(a, pr);
    gemv_prologue_finish<PRO_NORM, 0>(a, sm, pr);            // ends with __syncthreads(): sm.xq / sm.xs complete
    if (!any) return;

    for (; j0 < j_end; j0 += kWaves * kChoiceRows) {
#pragma unroll
        for (int j = 0; j < kChoiceJ; ++j) {
            const int ch = lane + 64 * j;
            const int cc = min(ch, nchunks - 1);
            if (64 * j < nchunks) {
                const v4i xv = ((const v4i*)sm.xq)[cc];
                const float xsc = sm.xs[cc >> lpg_shift];
#pragma unroll
                for (int r = 0; r < kChoiceRows; ++r) {
                    int d = __builtin_amdgcn_sdot4(w[r][j].x, xv.x, 0, false);
                    d = __builtin_amdgcn_sdot4(w[r][j].y, xv.y, d, false);
                    d = __builtin_amdgcn_sdot4(w[r][j].z, xv.z, d, false);
                    d = __builtin_amdgcn_sdot4(w[r][j].w, xv.w, d, false);
                    d = lpg_sum<0>(d, lpg);
                    if (ch < nchunks && (ch & (lpg - 1)) == 0) {
                        float t = (float)d * sc[r][j];       // tensor.rs:59  ((dot as f32) * ws) * xs
                        t = t * xsc;
                        term[r * ng + (ch >> lpg_shift)] = t;
                    }
                }
            }
        }
        wave_lds_sync();
        const int jr = j0 + kWaves * lane;                   // lane r folds row r
        float acc = 0.0f;
        if (lane < kChoiceRows && jr < j_end) acc = ordered_row_sum(term + lane * ng, ng);
        wave_lds_sync();                                     // the terms are read before the next batch overwrites them
        const int jn = j0 + kWaves * kChoiceRows;
        if (jn < j_end) load(jn);
        if (lane < kChoiceRows && jr < j_end) out[jr] = acc;
    }
}

// ------------------------------------------------------------------------------------------------
// dim > 1024 * kChoiceJ (Qwen3-14B and 32B: 5120): the same logits from two launches behind a block.  k_choice_rows holds whole rows in
// registers and repeats the prologue in every part; here the prologue runs once per prompt and a row is streamed.
//   k_choice_norm    grid = rows of the table: the PRO_NORM prologue of k_choice_rows, word for word, and then a copy of sm.xq / sm.xs to
//                    row blockIdx.x of the owned scratch xq[rows][n], xs[rows][n / G]
//   k_choice_stream  grid = (rows of the table, parts of kChoicePart candidates): stages its row of xq / xs in LDS and walks, per wave, the
//                    (batch of kChoiceRows candidates, 1 KiB piece) steps of its candidates in order through kChoiceDepth register
//                    buffers: step s lives in buffer s % kChoiceDepth, is reduced -- d_g, t_g into the wave's LDS term rows, as above --
//                    and its buffer is at once requested for step s + kChoiceDepth, across the end of a batch too, so a wave has
//                    kChoiceRows * kChoiceDepth KiB in flight whatever n is.  Behind a batch's last piece lane r folds row r.
// A piece past a whole number of KiB (n = 4608: 288 sixteen-byte pieces, lanes 32..63 of the fifth have none) clamps its address to
// the row's last piece and owns no group: n is a multiple of G, so the lanes of a group are live together or not at all.
// Bounds: as above; blockIdx.x < the rows the host grew the scratch for; a workgroup of k_choice_stream reads xq / xs of its row,
// wq[c][0 .. n), ws[c][0 .. n / G) for its candidates c and writes out[req][j] for j < k.
// ------------------------------------------------------------------------------------------------
constexpr int kChoiceDepth = 4;                           // pieces of each of a wave's kChoiceRows rows in flight: 16 loads of 16 bytes per lane
constexpr int kChoiceWaveCands = kChoicePart / kWaves;    // candidates of a part that one wave serves
constexpr int kChoiceMaxDim = 16384;                      // the longest vector the exact sum of squares walks in blocks (spec_ok), the engine's own bound
static_assert(kChoiceWaveCands % kChoiceRows == 0, "a wave's candidates are whole batches");

struct ChoiceNormArgs {
    const EmbedRow* rows;
    const float* x;          // the block's residuals, stride n
    const float* norm_w;
    int8_t* xq;              // [rows][n]
    float* xs;               // [rows][n / group]
    int n, group;
};
inline size_t choice_norm_smem_bytes(int n, int group) { return gemv_smem_bytes(n, group, 1, true); }

__global__ __launch_bounds__(kWG) void k_choice_norm(const ChoiceNormArgs c) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const EmbedRow R = c.rows[blockIdx.x];
    const int n = c.n, G = c.group, ng = n / G;
    const GemvSmem sm = gemv_carve(smem_raw, n, G, 1, true);
    GemvArgs a{};
    a.in = c.x + (size_t)R.col * n;
    a.norm_w = c.norm_w;
    a.n = n;
    a.group = G;
    a.strict = 1;
    ProRegs<PRO_NORM> pr;
    gemv_prologue_issue<PRO_NORM>(a, pr);
    gemv_prologue_finish<PRO_NORM, 0>(a, sm, pr);            // ends with __syncthreads(): sm.xq / sm.xs complete
    v4i* xq = (v4i*)(c.xq + (size_t)blockIdx.x * n);
    float* xs = c.xs + (size_t)blockIdx.x * ng;
    for (int i = threadIdx.x; i < (n >> 4); i += kWG) xq[i] = ((const v4i*)sm.xq)[i];
    for (int i = threadIdx.x; i < ng; i += kWG) xs[i] = sm.xs[i];
}

struct ChoiceStreamArgs {
    const EmbedRow* rows;
    const int8_t* xq;        // what k_choice_norm left for the rows of this block
    const float* xs;
    const int8_t* wq;        // the classifier matrix [vocab][n] and its scales [vocab][n / group]
    const float* ws;
    const int32_t* cand;     // as ChoiceArgs
    float* out;
    long long cand_stride;
    int n, group, k;
};
// LDS: xq[n] | xs[n / G] | term[kWaves][kChoiceRows][n / G]
inline size_t choice_stream_smem_bytes(int n, int group) {
    return align16((size_t)n) + align16(4 * (size_t)(n / group)) + 4 * (size_t)kWaves * kChoiceRows * (n / group);
}

__global__ __launch_bounds__(kWG) void k_choice_stream(const ChoiceStreamArgs c) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const EmbedRow R = c.rows[blockIdx.x];
    const int n = c.n, G = c.group, ng = n / G;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nchunks = n >> 4, lpg = G >> 4;                // 16-byte pieces of a row; lanes that share a quantization group
    const int lpg_shift = __builtin_ctz(lpg);
    const int np = (nchunks + 63) >> 6;                      // 1 KiB pieces of a row, the last one may be partial
    const int32_t* cand = c.cand + (size_t)R.req * c.cand_stride;
    float* out = c.out + (size_t)R.req * c.k;
    const int j_end = min(c.k, ((int)blockIdx.y + 1) * kChoicePart);
    int j0 = (int)blockIdx.y * kChoicePart + wave;           // candidate r of the batch at j0 is j0 + kWaves * r
    v4i* xq = (v4i*)smem_raw;
    float* xs = (float*)(smem_raw + align16((size_t)n));
    float* term = (float*)(smem_raw + align16((size_t)n) + align16(4 * (size_t)ng)) + (size_t)wave * kChoiceRows * ng;

    // the wave's rows of the matrix, wave-uniform; one past the end repeats the last live candidate (read, never stored)
    int rid[kChoiceWaveCands];
#pragma unroll
    for (int i = 0; i < kChoiceWaveCands; ++i) rid[i] = __builtin_amdgcn_readfirstlane(cand[min(j0 + kWaves * i, j_end - 1)]);
    const int steps = j0 < j_end ? (j_end - j0 + kWaves * kChoiceRows - 1) / (kWaves * kChoiceRows) * np : 0;

    v4i w[kChoiceDepth][kChoiceRows];
    float sc[kChoiceDepth][kChoiceRows];
    int ls = 0, lp = 0;                                      // the next step to request and its piece; rid[0 .. kChoiceRows) are its rows
    // No branch around the loads: behind a conditional request the compiler's wait counts assume the shorter path and drain the
    // other buffers at every use.  Past the wave's last step the last piece is requested again (cache hits, never reduced).
    auto request = [&](v4i (&wb)[kChoiceRows], float (&sb)[kChoiceRows]) {
        const int cc = min(lane + 64 * lp, nchunks - 1);
#pragma unroll
        for (int r = 0; r < kChoiceRows; ++r) {
            wb[r] = ((const v4i*)(c.wq + (size_t)rid[r] * (size_t)n))[cc];
            sb[r] = (c.ws + (size_t)rid[r] * (size_t)ng)[cc >> lpg_shift];
        }
        if (++ls < steps && ++lp == np) {                    // wave-uniform, scalar
            lp = 0;
#pragma unroll
            for (int i = 0; i + kChoiceRows < kChoiceWaveCands; ++i) rid[i] = rid[i + kChoiceRows];
        }
    };
#pragma unroll
    for (int d = 0; d < kChoiceDepth; ++d) request(w[d], sc[d]);     // in front of the staging: they depend on the arguments alone

    const v4i* gq = (const v4i*)(c.xq + (size_t)blockIdx.x * n);
    const float* gs = c.xs + (size_t)blockIdx.x * ng;
    for (int i = threadIdx.x; i < nchunks; i += kWG) xq[i] = gq[i];
    for (int i = threadIdx.x; i < ng; i += kWG) xs[i] = gs[i];
    __syncthreads();

    int p = 0;
    for (int s = 0; s < steps; s += kChoiceDepth) {
#pragma unroll
        for (int d = 0; d < kChoiceDepth; ++d) {
            if (s + d < steps) {                             // wave-uniform
                const int ch = lane + 64 * p;
                const int cc = min(ch, nchunks - 1);
                const v4i xv = xq[cc];
                const float xsc = xs[cc >> lpg_shift];
                const bool own = ch < nchunks && (ch & (lpg - 1)) == 0;
#pragma unroll
                for (int r = 0; r < kChoiceRows; ++r) {
                    const int dg = lpg_sum<0>(dot16<8>(w[d][r], xv), lpg);
                    if (own) {
                        float t = (float)dg * sc[d][r];      // tensor.rs:59  ((dot as f32) * ws) * xs
                        t = t * xsc;
                        term[r * ng + (ch >> lpg_shift)] = t;
                    }
                }
            }
            request(w[d], sc[d]);                            // step s + d + kChoiceDepth into the buffer just reduced
            if (s + d < steps && ++p == np) {                // the batch's last piece
                p = 0;
                wave_lds_sync();
                const int jr = j0 + kWaves * lane;           // lane r folds row r
                if (lane < kChoiceRows && jr < j_end) out[jr] = ordered_row_sum(term + lane * ng, ng);
                wave_lds_sync();                             // the terms are read before the next batch overwrites them
                j0 += kWaves * kChoiceRows;
            }
        }
    }
}

}  // namespace q3
