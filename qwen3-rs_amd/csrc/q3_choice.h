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

}  // namespace q3
