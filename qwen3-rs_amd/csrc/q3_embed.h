// q3_embed.h -- the last-token vectors of the prompts that end in a block (include/qwen3_hip.h section 2j).
//
// A block of PlanKind::SlotPrefill, or the layers of a column plan, leaves the last layer's residual of every column in the block
// scratch x[column][dim].  An embedding model's output is the final RMSNorm of the column that holds a prompt's last token,
// optionally cut to its leading out_dim components and L2-normalised: one workgroup per such column, behind the block.
#pragma once

namespace q3 {

constexpr unsigned kEmbedL2 = 1u;       // Q3_EMBED_L2

// one prompt that ends in the block: its last token's column, and the output row (the request's index in the call)
struct EmbedRow {
    int col, req;
};

// grid = the rows of the table; x: the block's residuals, stride dim; out: [n_requests][out_dim].  In f32, uncontracted:
//   ss = (((-0.0 + x0*x0) + x1*x1) + ...) over dim terms;  f = 1 / sqrt(ss / dim + eps);  y_i = w_i * (f * x_i)      (k_op_rmsnorm)
//   kEmbedL2:  s2 = (((-0.0 + y0*y0) + y1*y1) + ...) over the first out_dim terms;  d = max(sqrt(s2), 1e-12), a NaN taking the
//   1e-12 (torch F.normalize);  out_i = y_i / d.   Otherwise out_i = y_i.   i < out_dim <= dim.
// Both sums are seq_sum_terms over the term layout k_op_rmsnorm uses; dynamic LDS: term_floats(dim) floats, which holds the
// second sum's term_floats(out_dim) as well.  Bounds: a workgroup reads x[col][0 .. dim), w[0 .. dim) and writes
// out[req][0 .. out_dim); col and req come from the host's table (col < the block's columns, req < n_requests), never from the model.
__global__ __launch_bounds__(kWG) void k_embed_rows(const EmbedRow* __restrict__ rows, const float* __restrict__ x, const float* __restrict__ w,
                                                    int dim, int out_dim, unsigned flags, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* sq = (float*)smem_raw;               // term_floats(dim)
    const EmbedRow R = rows[blockIdx.x];
    const float* in = x + (size_t)R.col * dim;
    float* o = out + (size_t)R.req * out_dim;
    for (int i = threadIdx.x; i < dim; i += kWG) {
        const float v = in[i];
        sq[term_index(i, dim)] = v * v;
    }
    __syncthreads();
    const float ss = seq_sum_terms(sq, dim);
    const float f = 1.0f / sqrtf(ss / (float)dim + kEps);
    if (!(flags & kEmbedL2)) {
        for (int i = threadIdx.x; i < out_dim; i += kWG) o[i] = w[i] * (f * in[i]);
        return;
    }
    __syncthreads();                            // every wave has read the squares: the terms of the second sum take their place
    for (int i = threadIdx.x; i < out_dim; i += kWG) {
        const float y = w[i] * (f * in[i]);
        sq[term_index(i, out_dim)] = y * y;
    }
    __syncthreads();
    const float s2 = seq_sum_terms(sq, out_dim);
    const float nrm = sqrtf(s2);
    const float d = nrm > 1e-12f ? nrm : 1e-12f;
    for (int i = threadIdx.x; i < out_dim; i += kWG) o[i] = (w[i] * (f * in[i])) / d;
}

}  // namespace q3
