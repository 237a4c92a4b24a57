// q3_score.h -- per-position scores of many prompts: every scored column's classifier row reduced to four numbers on the device
// (include/qwen3_hip.h section 2l).
//
// A block of PlanKind::SlotPrefill, or the layers of a column plan, leaves the last layer's residual of every column in the block
// scratch x[column][dim].  The block's SCORED columns go, up to 32 at a time, through the classifier of a column plan (classify(),
// q3_plan_host.inc: k_bquant<PRO_NORM> and k_bgemm<EPI_LOGITS>, the logits q3_forward computes), and three kernels around it:
//   k_score_gather  copies the chunk's residual rows into columns 0 .. m - 1 of the 32-column scratch the classifier reads;
//   k_score_exp     e_i = expf(l_i - max) for every logit of every row, spread over the chip as k_sample_exp is;
//   k_score_sum     one workgroup per row: the sequential f32 sum of the e_i in index order (wg_walk_segments, q3_sampler.h), and the
//                   record {l[target], max, sum, argmax}.
// The maximum and the argmax of a row come from the argmax slots the classifier launch leaves, one key per workgroup: the keys
// k_spec_colmax and k_cols_turn fold (spec_col_best).  No logit leaves the device, and none becomes an address.
// k_score_exp and k_score_sum, and the two top kernels of q3_score_top.h, are the one reduction of a classifier row on the device.
// They are templates over the source of their rows: the host table of a chunk (TableRows, here) or the column pass in flight of a
// q3_generate_many_* loop (PassRows, q3_genlp.h).
#pragma once

namespace q3 {

constexpr int kScoreCols = 32;          // columns per chunk: the widest column plan
constexpr int kScoreGatherT = 64;       // threads per workgroup of k_score_gather, a float4 of every column each
constexpr int kScoreExpParts = 64;      // workgroups per row of k_score_exp (k_sample_exp's grid)

// one scored column of a chunk: its column in the block, the record it fills, the token whose logit is the record's target.
// All three are the host's (q3_score_host.inc checks col < the block's columns, out < the call's records, 0 <= target < vocab_size).
struct ScoreRow {
    int col, out, target;
};
// q3_score_rec of the header
struct ScoreRec {
    float target, max, sum;
    int argmax;
};

// grid = ceil(dim / 4 / kScoreGatherT).  dst[j][..] = src[rows[min(j, m - 1)].col][..] for j < width: the plan's columns past the
// chunk's m repeat the last one, the rule k_dense_states uses.  A thread owns one float4 of every column: it requests all of its
// `width` source pieces, then stores them, so src == dst (a block of 32 columns or fewer, gathered in place) is safe: no thread reads
// a piece another thread writes.  dim % 4 == 0 (group_size is a multiple of 16).  Vector loads and stores only.
__global__ __launch_bounds__(kScoreGatherT) void k_score_gather(const ScoreRow* __restrict__ rows, int m, int width, const float* src, float* dst, int dim) {
    const int v = blockIdx.x * kScoreGatherT + threadIdx.x;
    if (4 * v >= dim) return;
    v4f r[kScoreCols];
#pragma unroll
    for (int j = 0; j < kScoreCols; ++j) {
        const int col = rows[min(j, m - 1)].col;
        if (j < width) r[j] = *(const v4f*)(src + (size_t)col * dim + 4 * (size_t)v);
    }
#pragma unroll
    for (int j = 0; j < kScoreCols; ++j)
        if (j < width) *(v4f*)(dst + (size_t)j * dim + 4 * (size_t)v) = r[j];
}

// What the four record kernels (k_score_exp and k_score_sum here, k_score_top_part and k_score_top_merge of q3_score_top.h) read
// whatever their rows are: row j of a launch is row j of the classifier's output.
struct RecordArgs {
    const float* logits;                // [kScoreCols][n]: the classifier's output
    const unsigned long long* slots;    // [kScoreCols][slot_stride] argmax keys of the classifier launch, nslots of them written per row
    float* exps;                        // [kScoreCols][exps_stride] scratch, exps_stride % 4 == 0
    unsigned long long* part_keys;      // [kScoreCols][k][parts]: entry j of every slice's largest keys, descending, 0 behind the last
    int* part_above;                    // [kScoreCols][parts]: keys of the slice above the target's key
    long long exps_stride;
    int slot_stride, nslots;
    int n;                              // vocab_size
    int parts;                          // 1 .. kScoreTopParts: gridDim.x of k_score_top_part
};

// The kernels are templates over the source of their rows, which answers for row j of the launch:
//   live(j)             does the row emit?  A workgroup of a row that does not returns at once;
//   out(j)              the record of a live row;
//   target(a, j, best)  the token whose logit is the record's target; best() folds the row's argmax slots (spec_col_best);
//   k(), recs(), top(), rank()   the alternatives asked for and where the results go: recs[out], top[out k ..], rank[out] (rank may
//                       be null);
//   top_live(j, k)      does the row take part in the top launches?  live(j), and 1 <= k <= kScoreTopMax: the host's check for a
//                       k that comes by value, the source's own for one read from device memory.
// Only loop indices, counters and what a source hands out become addresses: no logit and no key read back from memory does, so a
// row that holds a NaN is wrong but harmless.
struct ScoreTop;

// The rows of q3_score_many / q3_score_top_many: a host table of m entries, every row of the grid live; k and the destinations by
// value in the kernel arguments.
struct TableRows {
    const ScoreRow* rows;               // the chunk's table, m entries
    ScoreRec* recs_;                    // the call's records
    ScoreTop* top_;                     // the call's [records][k]
    int* rank_;                         // the call's [records], or null
    int k_;                             // 0, or 1 .. kScoreTopMax, <= n
    __device__ __forceinline__ bool live(int) const { return true; }
    __device__ __forceinline__ bool top_live(int, int) const { return true; }
    __device__ __forceinline__ int out(int j) const { return rows[j].out; }
    template <class Best>
    __device__ __forceinline__ int target(const RecordArgs&, int j, Best&&) const { return rows[j].target; }
    __device__ __forceinline__ int k() const { return k_; }
    __device__ __forceinline__ ScoreRec* recs() const { return recs_; }
    __device__ __forceinline__ ScoreTop* top() const { return top_; }
    __device__ __forceinline__ int* rank() const { return rank_; }
};

// the fold of row j's argmax slots: the row's largest key
__device__ __forceinline__ unsigned long long record_best(const RecordArgs& a, int j) {
    return spec_col_best(a.slots + (size_t)j * (size_t)a.slot_stride, a.nslots);
}

// grid = (kScoreExpParts, rows), 256 threads.  exps[row][i] = expf(l_i - max), max the float of the row's largest key (layers.rs:496-501).
// Element-wise: any split over workgroups gives the same bits.  Every wave folds the row's keys itself (<= 2 per lane and CU).
template <class Src>
__global__ __launch_bounds__(256) void k_score_exp(const RecordArgs a, const Src src) {
    const int j = blockIdx.y;
    if (!src.live(j)) return;
    const float mx = key_to_float((unsigned)(record_best(a, j) >> 32));
    const float* l = a.logits + (size_t)j * (size_t)a.n;
    float* p = a.exps + (size_t)j * (size_t)a.exps_stride;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n; i += gridDim.x * 256) p[i] = q3_expf(l[i] - mx);
}

// grid = rows, kSampThreads threads.  sum = ((-0.0 + e_0) + e_1) + ... in index order (layers.rs:502), exact: wg_walk_segments verifies
// every link bitwise.  Thread 0 stores the record {l[target], max, sum, argmax}.
template <class Src>
__global__ __launch_bounds__(kSampThreads) void k_score_sum(const RecordArgs a, const Src src) {
    __shared__ float xch[kSampThreads + 16];
    __shared__ float carry_lds;
    const int j = blockIdx.x;
    if (!src.live(j)) return;
    const unsigned long long best = record_best(a, j);
    const float sum = wg_walk_segments(a.exps + (size_t)j * (size_t)a.exps_stride, a.n, -0.0f, xch, &carry_lds, nullptr,
                                       [](int, float, float) { return false; });
    if (threadIdx.x == 0) {
        ScoreRec rec;
        rec.target = a.logits[(size_t)j * (size_t)a.n + (size_t)src.target(a, j, [&] { return best; })];
        rec.max = key_to_float((unsigned)(best >> 32));
        rec.sum = sum;
        rec.argmax = (int)(unsigned)(best & 0xffffffffull);
        src.recs()[src.out(j)] = rec;
    }
}

}  // namespace q3
