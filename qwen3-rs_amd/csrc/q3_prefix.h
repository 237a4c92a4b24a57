// q3_prefix.h -- copying key / value rows between slots and the prefix store (include/qwen3_hip.h section 2i).
//
// Sections 2e to 2h make a slot's cache rows bit-identical whichever slot a request lands in, so the rows of a prompt prefix that
// many requests share are the same bits in every slot: they are computed once and copied.  The batched caches are plain f32
// [stream][layer][ctx][kv_dim] with no transposed value copy, so rows [first_pos, first_pos + n_rows) of one layer of one slot are
// one contiguous run in the key cache and one in the value cache.
#pragma once

namespace q3 {

constexpr int kBcastMax = 32;           // destinations of one launch
constexpr int kBcastUnroll = 4;         // loads a thread has in flight before its first store

// destination bases, by value in the kernel arguments (512 bytes): the first copied row of layer 0, per cache
struct KvBcastDst {
    float* key[kBcastMax];
    float* value[kBcastMax];
};

typedef unsigned int v4u __attribute__((ext_vector_type(4)));

// One launch copies the run of every layer of both caches from one source block to n_dst destination blocks: every source word is
// loaded once and stored n_dst times.  W is the access: v4u (16 bytes, kv_dim % 4 == 0: every shape the batched state accepts) or
// unsigned (dwords).  Raw 32-bit words, no float arithmetic: NaN payloads, -0.0 and denormals pass through.
// src_key / src_value and the table's pointers point at the first copied row of layer 0; layer strides and `run` (the words of
// one layer's rows, n_rows * kv_dim) are in floats.  blockIdx.y = cache * n_layers + layer, so no index is ever divided;
// blockIdx.x strides over the run, kBcastUnroll accesses of a thread apart by the grid's width.  Bounds: a thread touches words
// [0, run) of a layer's run and nothing else; layer < n_layers by the grid.
template <class W>
__global__ __launch_bounds__(kWG) void k_kv_rows_bcast(const float* __restrict__ src_key, const float* __restrict__ src_value, size_t src_layer_stride,
                                                       const KvBcastDst dst, int n_dst, size_t dst_layer_stride, int n_layers, size_t run) {
    constexpr size_t per = sizeof(W) / 4;
    const int cache = (int)blockIdx.y / n_layers, layer = (int)blockIdx.y - cache * n_layers;
    const W* __restrict__ src = reinterpret_cast<const W*>((cache ? src_value : src_key) + (size_t)layer * src_layer_stride);
    const size_t n = run / per, width = (size_t)gridDim.x * kWG, doff = (size_t)layer * dst_layer_stride;
    for (size_t i0 = (size_t)blockIdx.x * kWG + threadIdx.x; i0 < n; i0 += kBcastUnroll * width) {
        W w[kBcastUnroll];
#pragma unroll
        for (int u = 0; u < kBcastUnroll; ++u)
            if (i0 + u * width < n) w[u] = src[i0 + u * width];
        for (int d = 0; d < n_dst; ++d) {
            W* __restrict__ out = reinterpret_cast<W*>((cache ? dst.value[d] : dst.key[d]) + doff);
#pragma unroll
            for (int u = 0; u < kBcastUnroll; ++u)
                if (i0 + u * width < n) out[i0 + u * width] = w[u];
        }
    }
}

}  // namespace q3
