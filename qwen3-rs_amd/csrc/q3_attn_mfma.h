// q3_attn_mfma.h -- k_attn_pf_mfma<KVM>: causal dense-prefill attention of Q3_FLAG_FAST engines on the bf16 matrix cores
// (head_dim 128; KVM = 2, 4, 5 or 8 query heads per kv head).  DESIGN.md 4.24.
//
// Tolerance mode only: the sums run in the order the MFMA hardware picks, so nothing here is bit-equal to the reference; the
// budget it is held to is derived in DESIGN.md 4.24 and tests/test_attn_block_mfma.py.  Reference-order engines never reach it.
//
// Split precision.  Every f32 operand a goes to the matrix cores as two bf16 values, hi = bf16(a) and lo = bf16(a - hi)
// (a - hi is exact in f32), and a product a * b as three MFMAs hi*hi + hi*lo + lo*hi whose bf16 products are exact in the f32
// accumulator: 16 bits per operand are kept, lo*lo and the two split remainders (<= 2^-16 relative each) are dropped.
//
// Work split.  One workgroup of 8 waves per kv head and tile of block columns, heavy tiles (the highest columns) first; a wave
// owns the 32 x 128 output of one query head and 32 consecutive columns, and all waves share the staged K / V chunks, so a
// cache row crosses HBM once per kv group and tile.  The tile is 32 columns x (8 / KVM) column blocks: 8 heads x 32 columns,
// 4 x 64, 2 x 128; 5 heads x 32 with three waves that only stage.  (The proposal's KVM-wave workgroups: with 2 or 4 waves a
// thread stages 32 or 16 float4 per chunk ahead and the kernel needs more than 256 VGPRs, with 5 waves it spilled 50; with 8
// waves every form stages 8 float4 per thread and fits 256 VGPRs without scratch.)  A wave whose columns all lie behind a
// chunk skips its arithmetic, not its barriers.
//
// Data movement.  Chunks of 64 keys: the f32 cache rows are fetched into registers one chunk ahead (the loads of chunk i + 1
// travel under the arithmetic of chunk i) and split on their way into LDS -- 4 bytes per element, the footprint of the f32
// tile: K as [t][d] (row stride 136 bf16: the 16-byte operand reads of 16 lanes cover all 64 banks), V TRANSPOSED as [d][t']
// (row stride 72 bf16, t' the operand order below).  One buffer, two barriers per chunk, 72 KB.
//
// Arithmetic.  S^T = K Q^T with v_mfma_f32_32x32x16_bf16: the chunk's keys are the rows (A, from LDS), the tile's query
// columns the columns (B: the wave's Q, split once into 64 registers).  The accumulator then holds, per lane, ONE query column
// c = lane % 32 and 16 keys per 32-key block, t = 8 (r / 4) + 4 (lane / 32) + r % 4 -- which is the B-operand layout of
// O^T = V^T P^T (one column per lane, 8 reduction slots per lane half) up to the order of the reduction slots.  That order is
// free as long as A agrees, so V^T is staged with its 16-key groups permuted to it (slot 8 g + j of a group holds key
// 4 g + j % 4 + 8 (j / 4)) and P never leaves the registers.  Online softmax in f32 per column: the running maximum and sum live
// in both lanes of a column (lane, lane ^ 32), the chunk's maximum and sum cross once each by a lane swap, the accumulators
// are rescaled per chunk; exp is the project's expf.  The causal mask comes from the columns' positions and is applied on the
// chunks that reach past the tile's first position only; chunks wholly behind the tile's last position are never staged.
// Deterministic: no atomics, one fixed order per launch shape.
#pragma once

namespace q3 {

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef __bf16 v4bf __attribute__((ext_vector_type(4)));

constexpr int kMfCols = 32;                  // block columns per workgroup
constexpr int kMfTch = 64;                   // keys per staged chunk
constexpr int kMfKld = kG2Hd + 8;            // bf16 per staged K row
constexpr int kMfVld = kMfTch + 8;           // bf16 per staged V^T row
__host__ __device__ constexpr size_t attn_pf_mfma_smem_bytes() {
    return 2 * 2 * ((size_t)kMfTch * kMfKld + (size_t)kG2Hd * kMfVld) + 32 * 8;
}

// a = hi + lo + r, |r| <= 2^-16 |a| (round to nearest even both times; a - hi is exact)
__device__ __forceinline__ void mf_split(float a, __bf16& hi, __bf16& lo) {
    hi = (__bf16)a;
    lo = (__bf16)(a - (float)hi);
}
__device__ __forceinline__ void mf_split4(const v4f a, v4bf& hi, v4bf& lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        __bf16 h_, l_;
        mf_split(a[i], h_, l_);
        hi[i] = h_;
        lo[i] = l_;
    }
}
// acc += a * b at split precision: hi*hi + hi*lo + lo*hi
__device__ __forceinline__ v16f mf_mma3(const v8bf ah, const v8bf al, const v8bf bh, const v8bf bl, v16f acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}
// 16 exps of x - m (their f64 chains interleave); glibc's main path alone unless some lane is outside |x| < 88 (masked scores)
__device__ __forceinline__ v16f mf_exp16(const v16f x, float m, const unsigned long long* etab) {
    v16f d, e;
    bool sp = false;
#pragma unroll
    for (int r = 0; r < 16; ++r) { d[r] = x[r] - m; sp = sp || q3_expf_special(d[r]); }
    // (eight chains at a time: all sixteen in flight hold ~50 registers more than the kernel has)
    if (__builtin_expect(__any(sp), 0)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            e[r] = q3_expf_t(d[r], etab);
            if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // (the rare path with its selects: four)
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            e[r] = q3_expf_main(d[r], etab);
            if (r == 7) __builtin_amdgcn_sched_barrier(0);
        }
    }
    return e;
}

// columns per workgroup: 8 waves = KVM heads x column blocks of 32
__host__ __device__ constexpr int attn_pf_mfma_cols(int kvm) { return kMfCols * (8 / kvm); }

template <int KVM>
__global__ __launch_bounds__(512) void k_attn_pf_mfma(const AttnArgs a0) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int hd = kG2Hd, TCH = kMfTch, KLD = kMfKld, VLD = kMfVld, NTHR = 512, COLS = attn_pf_mfma_cols(KVM);
    constexpr int NKF4 = TCH * (hd / 4), NSLK = (NKF4 + NTHR - 1) / NTHR;          // K: one float4 per slot
    constexpr int NVTASK = (TCH / 4) * (hd / 4), NSLV = (NVTASK + NTHR - 1) / NTHR; // V: 4 keys x 4 dims per task (transposed in registers)
    static_assert(hd == 128 && TCH == 64 && NSLK * NTHR == NKF4 && NSLV * NTHR == NVTASK && (KVM == 2 || KVM == 4 || KVM == 5 || KVM == 8), "");
    __bf16* k_hi = (__bf16*)smem_raw;                              // [TCH][KLD]
    __bf16* k_lo = k_hi + TCH * KLD;
    __bf16* v_hi = k_lo + TCH * KLD;                               // [hd][VLD], keys of a 16-group in operand order
    __bf16* v_lo = v_hi + hd * VLD;
    unsigned long long* etab = (unsigned long long*)(v_lo + hd * VLD);

    const int kvh = blockIdx.x;
    const int tile = (int)gridDim.y - 1 - (int)blockIdx.y;         // heavy tiles (long contexts) first
    const int tid = threadIdx.x, lane = tid & 63, cl = lane & 31, g = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int head = kvh * KVM + wave % KVM;
    const int n_pos = a0.n_pos, pt = tile * COLS, p0 = min(pt + kMfCols * (wave / KVM), n_pos - 1);
    const bool live = wave < KVM * (8 / KVM) && pt + kMfCols * (wave / KVM) < n_pos;       // wave-uniform: the wave has a head and columns
    const size_t kvd = (size_t)a0.n_kv_heads * hd;
    // the block is one ascending run of positions (q3_prefill_batched): a column block's first column holds its smallest position,
    // its last column the largest, and rows 0 .. np_max - 1 of the cache are all the tile reads
    const int pos_min = __builtin_amdgcn_readfirstlane(a0.st[p0].pos);
    const int np_w = __builtin_amdgcn_readfirstlane(a0.st[min(p0 + kMfCols - 1, n_pos - 1)].pos) + 1;     // the wave's context
    const int np_max = __builtin_amdgcn_readfirstlane(a0.st[min(pt + COLS - 1, n_pos - 1)].pos) + 1;       // the tile's
    const int pc = min(p0 + cl, n_pos - 1);                        // this lane's column (past the block: the last one, nothing stored)
    const int pos_c = a0.st[pc].pos;
    const float* kbase = a0.key_cache + (size_t)kvh * hd;
    const float* vbase = a0.value_cache + (size_t)kvh * hd;
    if (tid < 32) etab[tid] = kExp2Tab[tid];

    // ---- staging: global -> registers (issue), registers -> split bf16 in LDS (commit)
    v4f kr[NSLK], vr[NSLV][4];
    auto issue_k = [&](int c0) {
#pragma unroll
        for (int u = 0; u < NSLK; ++u) {
            const int idx = tid + u * NTHR;
            const int row = min(c0 + (idx >> 5), np_max - 1);
            kr[u] = *(const v4f*)(kbase + (size_t)row * kvd + 4 * (idx & 31));
        }
    };
    auto issue_v = [&](int c0) {
#pragma unroll
        for (int u = 0; u < NSLV; ++u) {
            // task bits, low to high: key quad & 3 (2), key quad bit 2 (1), dim quad & 7 (3), dim quad >> 3 (2), key quad bit 3 (1): the
            // lanes of one load instruction read 8 rows x 128 contiguous bytes, and their 8-byte LDS writes below fall on distinct banks
            const int task = tid + u * NTHR;
            const int tq = (task & 7) | ((task >> 5) & 8), dq = (task >> 3) & 31;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = min(c0 + 4 * tq + i, np_max - 1);
                vr[u][i] = *(const v4f*)(vbase + (size_t)row * kvd + 4 * dq);
            }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int u = 0; u < NSLK; ++u) {
            const int idx = tid + u * NTHR;
            v4bf hi, lo;
            mf_split4(kr[u], hi, lo);
            const int o = (idx >> 5) * KLD + 4 * (idx & 31);
            *(v4bf*)(k_hi + o) = hi;
            *(v4bf*)(k_lo + o) = lo;
        }
#pragma unroll
        for (int u = 0; u < NSLV; ++u) {
            const int task = tid + u * NTHR;
            const int tq = (task & 7) | ((task >> 5) & 8), dq = (task >> 3) & 31;
            // keys 4 tq .. 4 tq + 3 of the chunk: quad q of 16-group tq / 4 lies at slot 8 (q & 1) + 4 (q / 2) of the group
            const int q = tq & 3, slot = 16 * (tq >> 2) + 8 * (q & 1) + 4 * (q >> 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const v4f col = {vr[u][0][e], vr[u][1][e], vr[u][2][e], vr[u][3][e]};
                v4bf hi, lo;
                mf_split4(col, hi, lo);
                const int o = (4 * dq + e) * VLD + slot;
                *(v4bf*)(v_hi + o) = hi;
                *(v4bf*)(v_lo + o) = lo;
            }
        }
    };
    issue_k(0);
    issue_v(0);

    // ---- the wave's queries, split once: B operand of S^T = K Q^T, column c = lane % 32, dims 16 ks + 8 g + j
    v8bf qh[hd / 16], ql[hd / 16];
#pragma unroll
    for (int ks = 0; ks < hd / 16; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            __bf16 h_, l_;
            mf_split(a0.q_out[attn_pf2_q_index(pc, head, 16 * ks + 8 * g + j, a0.n_heads, KVM)], h_, l_);
            qh[ks][j] = h_;
            ql[ks][j] = l_;
        }

    const float scale = 1.0f / sqrtf((float)hd);
    v16f o[hd / 32];                                               // O^T: dims 32 db + 8 (r / 4) + 4 g + r % 4 of column c
#pragma unroll
    for (int db = 0; db < hd / 32; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;
    float m_run = -__builtin_inff(), l_run = 0.0f;

    for (int c0 = 0; c0 < np_max; c0 += TCH) {
        __syncthreads();                                           // every wave is done with the previous chunk
        commit();
        __syncthreads();
        // the next chunk's rows travel under this chunk's arithmetic: K from here, V from behind the softmax (all 32 staging registers
        // held across the exps spilled)
        const bool more = c0 + TCH < np_max;
        if (more) issue_k(c0 + TCH);
        if (!live || c0 >= np_w) {                                 // (wave-uniform) a staging wave, or a chunk behind the wave's last column
            if (more) issue_v(c0 + TCH);
            continue;
        }

        // ---- S^T: keys 32 tb + 8 (r / 4) + 4 g + r % 4 of the chunk against column c
        v16f s[2];
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[tb][r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < hd / 16; ++ks)
#pragma unroll
            for (int tb = 0; tb < 2; ++tb) {
                const int off = (32 * tb + cl) * KLD + 16 * ks + 8 * g;
                s[tb] = mf_mma3(*(const v8bf*)(k_hi + off), *(const v8bf*)(k_lo + off), qh[ks], ql[ks], s[tb]);
            }
        const bool diag = c0 + TCH - 1 > pos_min;                  // wave-uniform: some key of the chunk lies ahead of some column
        float cmax = -__builtin_inff();
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int t = c0 + 32 * tb + 8 * (r >> 2) + 4 * g + (r & 3);
                const float v = s[tb][r] * scale;
                s[tb][r] = (diag && t > pos_c) ? -__builtin_inff() : v;
                cmax = fmaxf(cmax, s[tb][r]);
            }
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
        // chunk 0 holds key 0, which no column masks: m_new is finite from the first chunk on
        const float m_new = fmaxf(m_run, cmax);
        const float alpha = q3_expf_t(m_run - m_new, etab);
        m_run = m_new;
        float csum = 0.0f;
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) {
            s[tb] = mf_exp16(s[tb], m_new, etab);
#pragma unroll
            for (int r = 0; r < 16; ++r) csum += s[tb][r];
        }
        csum += __shfl_xor(csum, 32);
        l_run = l_run * alpha + csum;
#pragma unroll
        for (int db = 0; db < hd / 32; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] *= alpha;

        if (more) issue_v(c0 + TCH);

        // ---- O^T += V^T P^T: 16-key group sg = registers 8 (sg & 1) .. + 7 of s[sg / 2], already in B-operand order
        v8bf ph[4], pl[4];
#pragma unroll
        for (int sg = 0; sg < 4; ++sg)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                __bf16 h_, l_;
                mf_split(s[sg >> 1][8 * (sg & 1) + j], h_, l_);
                ph[sg][j] = h_;
                pl[sg][j] = l_;
            }
#pragma unroll
        for (int db = 0; db < hd / 32; ++db)
#pragma unroll
            for (int sg = 0; sg < 4; ++sg) {
                const int off = (32 * db + cl) * VLD + 16 * sg + 8 * g;
                o[db] = mf_mma3(*(const v8bf*)(v_hi + off), *(const v8bf*)(v_lo + off), ph[sg], pl[sg], o[db]);
            }
    }

    if (live && p0 + cl < n_pos) {
        const float inv = 1.0f / l_run;
        float* out = a0.xb + (size_t)pc * a0.sb_xb + (size_t)head * hd + 4 * g;
#pragma unroll
        for (int db = 0; db < hd / 32; ++db)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const v4f v = {o[db][4 * rq] * inv, o[db][4 * rq + 1] * inv, o[db][4 * rq + 2] * inv, o[db][4 * rq + 3] * inv};
                *(v4f*)(out + 32 * db + 8 * rq) = v;
            }
    }
}

// launch shape: grid (kv heads, tiles of attn_pf_mfma_cols columns), 512 threads
typedef void (*AttnMfmaFn)(const AttnArgs);
inline AttnMfmaFn attn_pf_mfma_fn(int kvm) {
    return kvm == 2 ? k_attn_pf_mfma<2> : kvm == 4 ? k_attn_pf_mfma<4> : kvm == 5 ? k_attn_pf_mfma<5> : kvm == 8 ? k_attn_pf_mfma<8> : nullptr;
}
inline dim3 attn_pf_mfma_grid(int n_kv_heads, int kvm, int n_pos) { return dim3((unsigned)n_kv_heads, (unsigned)((n_pos + attn_pf_mfma_cols(kvm) - 1) / attn_pf_mfma_cols(kvm))); }

}  // namespace q3
