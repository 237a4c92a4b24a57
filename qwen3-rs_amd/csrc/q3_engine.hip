// q3_engine.hip -- host side of libqwen3_hip.so: checkpoint loader, launch plan, hipGraph, C ABI.
//
// Mirrors, for the hot path only, what qwen3-inference does around `Transformer::forward`:
//   TransformerBuilder::build            models/mod.rs:55-73      -> q3_create
//   read_config / validate_config        configuration.rs:77-146  -> parse_header
//   MemoryMapper + load_weights          utils.rs, qwen3.rs:199-277 -> Engine::load (mmap -> one HBM blob)
//   TransformerBlockBuffers::new         qwen3.rs:414-445         -> device scratch + zero-filled f32 KV cache
//   Qwen3Transformer::forward            qwen3.rs:62-79           -> Engine::enqueue_forward (kernel chain)
// There is deliberately no CPU fallback anywhere in this file.
#include <hip/hip_runtime.h>
#if !defined(__HIP_DEVICE_COMPILE__)
#include <immintrin.h>
#endif

#include <errno.h>
#include <fcntl.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <map>
#include <new>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/qwen3_hip.h"
#include "q3_kernels.h"
#include "q3_batch.h"
#include "q3_sampler.h"
#include "q3_stop.h"
#include "q3_prefix.h"
#include "q3_embed.h"
#include "q3_choice.h"
#include "q3_score.h"
#include "q3_score_top.h"
#include "q3_topk.h"
#include "q3_genlp.h"
#include "q3_penalty.h"
#include "q3_bias.h"
#include "q3_guide.h"
#include "q3_guide_sparse.h"
#include "q3_stop_seq.h"
#include "q3_lookup.h"

namespace {

using namespace q3;

thread_local char g_err[1024] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(Q3_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// Sampler::new's refusals (sampler.rs:32-33), for every entry point that takes sampler parameters.  req >= 0: they are request req's
int sampler_check(float temperature, float topp, long req = -1) {
    const bool bad_t = !(temperature >= 0.0f), bad_p = !(topp >= 0.0f && topp <= 1.0f);
    if (!bad_t && !bad_p) return Q3_OK;
    char who[40] = "";
    if (req >= 0) snprintf(who, sizeof who, "request %ld: ", req);
    return bad_t ? fail(Q3_ERR_ARG, "%sTemperature must be non-negative", who) : fail(Q3_ERR_ARG, "%sTop-p must be between 0.0 and 1.0", who);
}

// what q3_sampler_penalties and q3_op_penalize refuse about their values (section 2p): finite, inside [-2, 2]
int penalties_check(float presence, float frequency) {
    const auto ok = [](float v) { return v >= -2.0f && v <= 2.0f; };      // false for a NaN
    if (ok(presence) && ok(frequency)) return Q3_OK;
    return fail(Q3_ERR_ARG, "penalties (%g, %g) out of range: finite values in -2 .. 2", (double)presence, (double)frequency);
}

// The table of q3_logit_bias_set as the engine keeps it (section 2q): the lists one behind the other, each sorted by token.
struct BiasTable {
    std::vector<BiasEntry> entries;
    std::vector<unsigned> off;           // [n_lists + 1]; empty: no table
    std::vector<unsigned char> modes;    // [n_lists]
    size_t n_lists() const { return modes.size(); }
};
static_assert(sizeof(BiasEntry) == sizeof(q3_bias_entry) && sizeof(BiasEntry) == 12, "BiasEntry is q3_bias_entry");
static_assert(sizeof(GuideEdge) == sizeof(q3_guide_edge) && sizeof(GuideEdge) == 8, "GuideEdge is q3_guide_edge");

// What q3_logit_bias_set and q3_op_logit_bias refuse about a table, the engine and the GPU untouched: a null array with a non-zero
// count, a list of more than kBiasMax entries, a negative token, a bias that is NaN, +inf or finite outside [-100, 100], a mode other
// than 0 or 1, a token twice in one list, an ALLOW list with no finite bias.  vocab >= 0, the checks that need a model: a token >=
// vocab, an ADD list that bans every token.  On success `out` holds the table, every list sorted by token.
int bias_check(const q3_bias_entry* entries, const size_t* n_entries, const uint8_t* mode, size_t n_lists, long vocab, BiasTable& out) {
    out = BiasTable{};
    if (n_lists == 0) return Q3_OK;
    if (!n_entries) return fail(Q3_ERR_ARG, "null n_entries with %zu lists", n_lists);
    if (n_lists > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 lists");
    size_t total = 0;
    for (size_t i = 0; i < n_lists; ++i) {
        if (n_entries[i] > (size_t)kBiasMax) return fail(Q3_ERR_ARG, "list %zu: %zu entries, at most %d", i, n_entries[i], kBiasMax);
        if (mode && mode[i] != kBiasAdd && mode[i] != kBiasAllow) return fail(Q3_ERR_ARG, "list %zu: mode %d is neither ADD (0) nor ALLOW (1)", i, (int)mode[i]);
        total += n_entries[i];
    }
    if (total > 0 && !entries) return fail(Q3_ERR_ARG, "null entries with %zu of them", total);
    out.entries.resize(total);
    out.off.resize(n_lists + 1);
    out.modes.resize(n_lists);
    size_t at = 0;
    for (size_t i = 0; i < n_lists; ++i) {
        const size_t n = n_entries[i];
        out.off[i] = (unsigned)at;
        out.modes[i] = mode ? mode[i] : (unsigned char)kBiasAdd;
        size_t finite = 0, banned = 0;
        for (size_t k = 0; k < n; ++k) {
            const q3_bias_entry& x = entries[at + k];
            if (x.token < 0) return fail(Q3_ERR_ARG, "list %zu: negative token %d", i, x.token);
            if (vocab >= 0 && x.token >= vocab) return fail(Q3_ERR_ARG, "index out of range: list %zu token %d (vocab_size %ld)", i, x.token, vocab);
            const bool ninf = x.bias == -INFINITY;
            if (!ninf && !(x.bias >= -100.0f && x.bias <= 100.0f))      // false for a NaN
                return fail(Q3_ERR_ARG, "list %zu token %d: bias %g is neither -inf nor a finite value in -100 .. 100", i, x.token, (double)x.bias);
            if (ninf) ++banned; else ++finite;
            out.entries[at + k] = BiasEntry{x.token, x.bias, x.until};
        }
        std::sort(out.entries.begin() + at, out.entries.begin() + at + n, [](const BiasEntry& a, const BiasEntry& b) { return a.token < b.token; });
        for (size_t k = 1; k < n; ++k)
            if (out.entries[at + k].token == out.entries[at + k - 1].token)
                return fail(Q3_ERR_ARG, "list %zu: token %d twice", i, out.entries[at + k].token);
        if (out.modes[i] == kBiasAllow && finite == 0) return fail(Q3_ERR_ARG, "list %zu: an ALLOW list without a finite bias allows no token", i);
        if (out.modes[i] == kBiasAdd && vocab >= 0 && banned >= (size_t)vocab) return fail(Q3_ERR_ARG, "list %zu bans every token of the vocabulary", i);
        at += n;
    }
    out.off[n_lists] = (unsigned)at;
    return Q3_OK;
}

// The guide of q3_guide_set as the engine keeps it (section 2r).  serial: which q3_guide_set made it, so the batched state knows
// whether the table it holds on the device is this one (guide_call_begin, q3_plan_host.inc).
struct GuideTable {
    std::vector<int16_t> next;           // [n_states][vocab]; empty: no guide
    std::vector<int> start;              // [n_start]
    size_t n_states = 0, vocab = 0;
    unsigned long long serial = 0;
};

// What q3_guide_set refuses about a guide, the engine and the GPU untouched: a null array with a non-zero count, more than
// kGuideMaxStates states, states without a start entry, vocab == 0 or >= 2^31, a start or an entry of next outside [-1, n_states),
// a state whose row allows no token.
int guide_check(const int16_t* next, size_t n_states, size_t vocab, const int32_t* start, size_t n_start) {
    if (!next && n_states) return fail(Q3_ERR_ARG, "null next with %zu states", n_states);
    if (!start && n_start) return fail(Q3_ERR_ARG, "null start with %zu entries", n_start);
    if (n_states == 0) return Q3_OK;
    if (n_states > (size_t)kGuideMaxStates) return fail(Q3_ERR_ARG, "%zu states, at most %d", n_states, kGuideMaxStates);
    if (vocab == 0 || vocab > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "a guide over %zu tokens: 1 .. 2^31 - 1", vocab);
    if (n_start == 0) return fail(Q3_ERR_ARG, "%zu states and no start state", n_states);
    if (n_start > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 start states");
    for (size_t r = 0; r < n_start; ++r)
        if (start[r] < -1 || start[r] >= (int32_t)n_states)
            return fail(Q3_ERR_ARG, "start[%zu] = %d: -1 (unguided) or a state below %zu", r, start[r], n_states);
    for (size_t s = 0; s < n_states; ++s) {
        const int16_t* row = next + s * vocab;
        bool any = false;
        for (size_t v = 0; v < vocab; ++v) {
            if (row[v] < -1 || (size_t)(row[v] + 1) > n_states)
                return fail(Q3_ERR_ARG, "next[%zu][%zu] = %d: -1 (forbidden) or a state below %zu", s, v, (int)row[v], n_states);
            any |= row[v] >= 0;
        }
        if (!any) return fail(Q3_ERR_ARG, "state %zu allows no token", s);
    }
    return Q3_OK;
}

// The sparse guide of q3_guide_set_sparse as the engine keeps it (section 2s); serial as in GuideTable, from the same counter.
struct GuideSparse {
    std::vector<int> dflt;               // [n_states]; empty: no sparse guide
    std::vector<uint32_t> row_off;       // [n_states + 1]
    std::vector<GuideEdge> edges;        // [n_edges]
    std::vector<int> start;              // [n_start]
    size_t n_states = 0, vocab = 0;
    unsigned long long serial = 0;
};

// What q3_guide_set_sparse refuses about a guide, the engine and the GPU untouched: a null array with a non-zero count, the caps,
// states without a start entry, vocab == 0 or >= 2^31, row_off[0] != 0, offsets that decrease or do not end at n_edges, a token
// outside [0, vocab) or not strictly ascending within its state, a next, dflt or start outside [-1, n_states), a state that allows
// no token.  The stop automaton of section 2t is stated in the same arrays and checked here too (sparse_table_check with its own
// caps and dead_ok: there -1 ends the request, and a state whose every token does so is legal).
int sparse_table_check(const int32_t* dflt, const uint32_t* row_off, const q3_guide_edge* edges, size_t n_states, size_t n_edges, size_t vocab,
                       const int32_t* start, size_t n_start, int max_states, int max_edges, bool dead_ok, const char* what) {
    if (!dflt && n_states) return fail(Q3_ERR_ARG, "null dflt with %zu states", n_states);
    if (!row_off && n_states) return fail(Q3_ERR_ARG, "null row_off with %zu states", n_states);
    if (!edges && n_edges) return fail(Q3_ERR_ARG, "null edges with %zu edges", n_edges);
    if (!start && n_start) return fail(Q3_ERR_ARG, "null start with %zu entries", n_start);
    if (n_states == 0) {
        if (n_edges) return fail(Q3_ERR_ARG, "%zu edges and no state", n_edges);
        return Q3_OK;
    }
    if (n_states > (size_t)max_states) return fail(Q3_ERR_ARG, "%zu states, at most %d", n_states, max_states);
    if (n_edges > (size_t)max_edges) return fail(Q3_ERR_ARG, "%zu edges, at most %d", n_edges, max_edges);
    if (vocab == 0 || vocab > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "a %s over %zu tokens: 1 .. 2^31 - 1", what, vocab);
    if (n_start == 0) return fail(Q3_ERR_ARG, "%zu states and no start state", n_states);
    if (n_start > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 start states");
    for (size_t r = 0; r < n_start; ++r)
        if (start[r] < -1 || start[r] >= (int32_t)n_states)
            return fail(Q3_ERR_ARG, "start[%zu] = %d: -1 (unguided) or a state below %zu", r, start[r], n_states);
    if (row_off[0] != 0u) return fail(Q3_ERR_ARG, "row_off[0] = %u, not 0", row_off[0]);
    for (size_t s = 0; s < n_states; ++s)
        if (row_off[s + 1] < row_off[s]) return fail(Q3_ERR_ARG, "row_off[%zu] = %u below row_off[%zu] = %u", s + 1, row_off[s + 1], s, row_off[s]);
    if ((size_t)row_off[n_states] != n_edges) return fail(Q3_ERR_ARG, "row_off[%zu] = %u does not end at the %zu edges", n_states, row_off[n_states], n_edges);
    for (size_t s = 0; s < n_states; ++s) {
        if (dflt[s] < -1 || dflt[s] >= (int32_t)n_states) return fail(Q3_ERR_ARG, "dflt[%zu] = %d: -1 (forbidden) or a state below %zu", s, dflt[s], n_states);
        size_t ok = 0;                 // listed tokens that are allowed
        for (size_t k = row_off[s]; k < row_off[s + 1]; ++k) {
            const q3_guide_edge& ge = edges[k];
            if (ge.token < 0 || (size_t)ge.token >= vocab) return fail(Q3_ERR_ARG, "edges[%zu].token = %d of state %zu outside the %zu tokens", k, ge.token, s, vocab);
            if (k > row_off[s] && ge.token <= edges[k - 1].token)
                return fail(Q3_ERR_ARG, "edges[%zu].token = %d of state %zu is not above its predecessor %d: tokens ascend strictly", k, ge.token, s, edges[k - 1].token);
            if (ge.next < -1 || ge.next >= (int32_t)n_states)
                return fail(Q3_ERR_ARG, "edges[%zu].next = %d of state %zu: -1 (forbidden) or a state below %zu", k, ge.next, s, n_states);
            ok += ge.next >= 0;
        }
        const size_t listed = row_off[s + 1] - row_off[s];
        if (!dead_ok && ok == 0 && (dflt[s] < 0 || listed == vocab)) return fail(Q3_ERR_ARG, "state %zu allows no token", s);
    }
    return Q3_OK;
}
int guide_sparse_check(const int32_t* dflt, const uint32_t* row_off, const q3_guide_edge* edges, size_t n_states, size_t n_edges, size_t vocab,
                       const int32_t* start, size_t n_start) {
    return sparse_table_check(dflt, row_off, edges, n_states, n_edges, vocab, start, n_start, kGuideSpMaxStates, kGuideSpMaxEdges, false, "guide");
}
// what q3_stop_seq_set, q3_op_stop_seq and q3_cols_schedule_stop_seq refuse about a stop automaton (section 2t)
int stop_seq_check(const int32_t* dflt, const uint32_t* row_off, const q3_guide_edge* edges, size_t n_states, size_t n_edges, size_t vocab,
                   const int32_t* start, size_t n_start) {
    return sparse_table_check(dflt, row_off, edges, n_states, n_edges, vocab, start, n_start, kStopSeqMaxStates, kStopSeqMaxEdges, true, "stop automaton");
}

constexpr int32_t kMagic = 0x616a6331;   // configuration.rs:8
constexpr int32_t kVersion = 1;          // configuration.rs:10
constexpr size_t kHeaderSize = 256;      // configuration.rs:12
constexpr size_t kConfigSize = 52;       // 13 x i32

int32_t rd_i32(const uint8_t* p) {
    return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

// configuration.rs:77-146
int parse_header(const uint8_t* d, size_t len, q3_config* c) {
    if (!d || !c) return fail(Q3_ERR_ARG, "null argument");
    if (len < kConfigSize)
        return fail(Q3_ERR_FORMAT, "Insufficient data: need %zu bytes, have %zu remaining", kConfigSize, len);
    if (len < kHeaderSize)
        return fail(Q3_ERR_FORMAT, "Cannot skip %zu bytes: insufficient data", kHeaderSize - kConfigSize);
    const int32_t magic = rd_i32(d), version = rd_i32(d + 4);
    if (magic != kMagic)
        return fail(Q3_ERR_FORMAT, "Invalid model configuration: Invalid checkpoint magic number: expected %#x, got %#x",
                    kMagic, (unsigned)magic);
    if (version != kVersion)
        return fail(Q3_ERR_FORMAT, "Invalid model configuration: Unsupported checkpoint version: expected %d, got %d",
                    kVersion, version);
    c->architecture_id = rd_i32(d + 8);
    c->dim = rd_i32(d + 12);
    c->hidden_dim = rd_i32(d + 16);
    c->n_layers = rd_i32(d + 20);
    c->n_heads = rd_i32(d + 24);
    c->n_kv_heads = rd_i32(d + 28);
    c->vocab_size = rd_i32(d + 32);
    c->seq_len = rd_i32(d + 36);
    c->head_dim = rd_i32(d + 40);
    c->shared_classifier = rd_i32(d + 44) != 0;
    c->group_size = rd_i32(d + 48);
    const char* names[8] = {"architecture_id", "dim", "n_layers", "n_heads", "n_kv_heads", "vocab_size", "seq_len", "head_dim"};
    const int32_t vals[8] = {c->architecture_id, c->dim, c->n_layers, c->n_heads, c->n_kv_heads, c->vocab_size, c->seq_len, c->head_dim};
    for (int i = 0; i < 8; ++i)
        if (vals[i] <= 0)
            return fail(Q3_ERR_FORMAT, "Invalid model configuration: Invalid %s: must be positive, got %d", names[i], vals[i]);
    return Q3_OK;
}

bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// shapes the kernels cover (everything the reference README lists, plus small test shapes)
int check_supported(const q3_config& c) {
    const int G = c.group_size;
    if (G < 16 || G > 1024 || !is_pow2(G))
        return fail(Q3_ERR_UNSUPPORTED, "group_size %d unsupported: must be a power of two in [16,1024]", G);
    const int ahd = c.n_heads * c.head_dim;
    if (c.hidden_dim <= 0) return fail(Q3_ERR_FORMAT, "Invalid hidden_dim %d", c.hidden_dim);
    if (c.dim % G || ahd % G || c.hidden_dim % G)
        return fail(Q3_ERR_UNSUPPORTED, "dim/all_heads_dim/hidden_dim must be multiples of group_size %d", G);
    if (c.head_dim % 8 || c.head_dim > 256 || !is_pow2(c.head_dim))
        return fail(Q3_ERR_UNSUPPORTED, "head_dim %d unsupported: power of two in [8,256] required", c.head_dim);
    if (c.n_heads % c.n_kv_heads) return fail(Q3_ERR_UNSUPPORTED, "n_heads must be a multiple of n_kv_heads");
    if (c.dim > 16384 || c.hidden_dim > 65536 || ahd > 16384)
        return fail(Q3_ERR_UNSUPPORTED, "dimension too large for the LDS-staged activation");
    return Q3_OK;
}

struct QT {  // QuantizedTensor view (tensor.rs:5-8) in device memory
    const int8_t* q = nullptr;
    const float* s = nullptr;
};

enum Family { F_QKV = 0, F_ATTN, F_WO, F_W13, F_W2, F_LMHEAD, F_NEXT, F_COUNT };
const char* kFamilyNames[F_COUNT] = {"qkv", "attn", "wo", "w13", "w2", "lm_head", "next"};

typedef void (*GemvFn)(const GemvArgs);
typedef void (*AttnFn)(const AttnArgs);

// One kernel launch of a plan, resolved when the plan is built: the kernel, its grid, block and dynamic LDS bytes, and the
// kernel's own arguments (a std::tuple of its parameter types in `args`, built and read back by the typed `thunk`).
// Copyable: plans are std::vectors.  make_launch() fills one, launch() enqueues it without looking at what it is.
constexpr size_t kLaunchArgBytes = 512;
struct Launch {
    Family fam = F_QKV;
    void (*thunk)(const Launch&, hipStream_t) = nullptr;
    void (*kernel)() = nullptr;
    dim3 grid, block;
    size_t smem = 0;
    alignas(16) unsigned char args[kLaunchArgBytes] = {};
};
inline void launch(const Launch& L, hipStream_t st) { L.thunk(L, st); }

}  // namespace

// GEMV kernel instantiations live in their own translation unit (q3_gemv_inst.hip: compiled in parallel with this one)
namespace q3inst {
typedef void (*GemvFn)(const q3::GemvArgs);
struct GemvCfg { int pro, epi, n, wgt, ept, ru, ju, pf; GemvFn fn; };
GemvFn gemv_pick(int pro, int epi, int G, int RU, int JU, int FIN, int PF);       // generic run-time-n kernels
const GemvCfg* find_cfg(int pro, int epi, int n, int G, bool fast = false);              // shape-specialised kernels
}
using q3inst::GemvCfg;
using q3inst::find_cfg;

namespace {
template <int PRO, int EPI>
GemvFn pick(int G, int RU, int JU, int FIN = 0, int PF = 0) { return q3inst::gemv_pick(PRO, EPI, G, RU, JU, FIN, PF); }

int set_max_smem(const void* fn, size_t bytes) {
    if (bytes > 48 * 1024) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return Q3_OK;
}

template <class... KA>
struct LaunchThunk {
    typedef std::tuple<KA...> Args;
    static_assert(sizeof(Args) <= kLaunchArgBytes && alignof(Args) <= 16, "kernel arguments do not fit the launch record");
    static_assert(std::is_trivially_copy_constructible<Args>::value && std::is_trivially_destructible<Args>::value,
                  "launch records are copied as plain bytes");
    static void run(const Launch& L, hipStream_t st) {
        std::apply([&](const KA&... a) { hipLaunchKernelGGL(reinterpret_cast<void (*)(KA...)>(L.kernel), L.grid, L.block, L.smem, st, a...); },
                   *reinterpret_cast<const Args*>(L.args));
    }
};
// The one place a launch record is made: the arguments are checked against the kernel's signature here, and the kernel's
// dynamic-LDS limit is raised here (nowhere else).
template <class... KA, class... A>
int make_launch(Launch& L, Family fam, void (*kernel)(KA...), dim3 grid, dim3 block, size_t smem, const A&... args) {
    static_assert(sizeof...(KA) == sizeof...(A), "argument count differs from the kernel's");
    L = Launch{};
    L.fam = fam;
    L.thunk = &LaunchThunk<KA...>::run;
    L.kernel = reinterpret_cast<void (*)()>(kernel);
    L.grid = grid;
    L.block = block;
    L.smem = smem;
    new (L.args) std::tuple<KA...>(args...);
    return set_max_smem(reinterpret_cast<const void*>(kernel), smem);
}
// launches outside any plan (operator entry points, weight packing, state setup)
template <class... KA, class... A>
int launch_now(hipStream_t st, void (*kernel)(KA...), dim3 grid, dim3 block, size_t smem, const A&... args) {
    Launch L;
    const int rc = make_launch(L, F_NEXT, kernel, grid, block, smem, args...);
    if (rc == Q3_OK) launch(L, st);
    return rc;
}

// A captured stream graph and its executable instance.
struct Graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    Graph() = default;
    Graph(const Graph&) = delete;
    Graph& operator=(const Graph&) = delete;
    ~Graph() { reset(); }
    Graph(Graph&& o) noexcept { swap(o); }
    Graph& operator=(Graph&& o) noexcept {
        if (this != &o) {
            reset();
            swap(o);
        }
        return *this;
    }
    explicit operator bool() const { return exec != nullptr; }
    void swap(Graph& o) {
        std::swap(graph, o.graph);
        std::swap(exec, o.exec);
    }
    void reset() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        exec = nullptr;
        graph = nullptr;
    }
    // body() enqueues on `st` and returns a Q3 status
    template <class Body>
    int capture(hipStream_t st, Body body) {
        reset();
        HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        const int rc = body();
        const hipError_t end = hipStreamEndCapture(st, &graph);
        if (rc) return rc;
        HIP_TRY(end);
        HIP_TRY(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        return Q3_OK;
    }
    int launch(hipStream_t st) const {
        HIP_TRY(hipGraphLaunch(exec, st));
        return Q3_OK;
    }
};

// The engine's stream: a member declared in front of every buffer and graph that lives on it, so it is destroyed behind them.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

// Environment variables.  The product library reads only the documented ones (include/qwen3_hip.h, "Environment"):
// env_int().  Everything else -- A/B switches between kernel forms that are product code for other shapes, workgroup overrides, timeline
// switches -- exists in the developer build only (make dev, -DQ3_DEV): dev_knob() is its default in the product.
int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}
#ifdef Q3_DEV
#define dev_knob(name, dflt) env_int(name, dflt)
#else
#define dev_knob(name, dflt) (dflt)
#endif

// slices per column of the top-k selection (k_topk_part's gridDim.x): one list per lane of the draw's merge.  A slice of the
// 151,936-entry vocabulary is then 2,374 entries, one tile of the part kernel (Q3_TOPK_PARTS, developer build: another split, the same draws)
int topk_parts() {
    const int p = dev_knob("Q3_TOPK_PARTS", kScoreTopParts);
    return p < 1 ? 1 : (p > kScoreTopParts ? kScoreTopParts : p);
}


}  // namespace

#include "q3_mem.h"
#include "q3_draw_host.inc"

struct BatchCtx;
struct q3_engine;
namespace { void batch_free(q3_engine* e); }

struct q3_engine {
    q3_config cfg{};
    uint32_t flags = 0;
    int device = 0;
    int n_cu = 256;
    Stream stream;
    // device memory
    DevMem<uint8_t> d_blob;
    size_t blob_bytes = 0;
    const float *rms_att = nullptr, *rms_ffn = nullptr, *rms_final = nullptr, *q_ln = nullptr, *k_ln = nullptr;
    QT tok, wcls;
    std::vector<QT> wq, wk, wv, wo, w1, w2, w3;
    DevMem<float> d_x, d_q, d_kraw, d_xb, d_hb, d_logits;
    DevMem<float> d_tap, d_key, d_value, d_rope, d_att;
    DevMem<float> d_value_t;                   // transposed copy of the value cache, [L][kv_dim][seq_len]: what k_attn_out streams (long contexts)
    DevMem<int8_t> d_xbq;                      // attention output quantized by k_attn_short (operand of the PRO_PREQR Wo launch)
    DevMem<float> d_xbs;
    DevMem<State> d_state;
    DevMem<int32_t> d_out_tokens;
    DevMem<int32_t> d_prompt;                  // chat-mode prefill: prompt token ids (capacity out_cap)
    int out_cap = 0;
    DevMem<unsigned long long> d_stamps;      // developer timeline (Q3_STAMPS=1) / kernel begin-end cells (Q3_KSTAMPS=1)
    DevMem<unsigned long long> d_kacc;        // Q3_KSTAMPS=1: per-launch duration / gap sums (k_kstamp_fold)
    DevMem<unsigned long long> d_kslots;      //   per-wave begin / end slots of every launch, [launch][kKstampSlots][2]
    DevMem<unsigned long long> d_kcells;      //   per-launch {begin, end} of the current token (k_kstamp_reduce)
    DevMem<int> d_knslots;                    //   live wave slots of every launch
    bool kstamps = false;
    DevMem<unsigned long long> d_argmax_slots;
    DevMem<unsigned long long> d_next_cell;      // {argmax cell, ticket counter} of the classifier launch with k_next folded in
    int n_argmax_slots = 0;
    // pinned host staging
    PinMem<float> h_logits;
    PinMem<State> h_state;
    PinMem<int32_t> h_tokens;
    // launch plans: `plan` (one attention kernel per layer) for short contexts, `plan_long` (scores + out
    // kernels over many workgroups) once pos >= split_pos; the host knows pos of every forward it enqueues
    std::vector<Launch> plan, plan_long;
    Launch lm_plain;                           // the classifier launch without the folded bookkeeping (q3_profile replays launches without advancing the state)
    size_t n_token_launches = 0;               // launches of a token in `plan` (the developer Q3_KSTAMPS reduce / fold launches follow them)
    // captured chains, indexed [short, long]: `decode` is the token's kernels; `forward` is q3_forward as ONE graph launch -- state
    // upload (pinned h_state) -> the token's kernels -> logits download (pinned h_logits)
    Graph decode[2], forward[2];
    DevMem<float> d_att_priv;
    int split_pos = 256;
    // the transposed value cache exists iff the long-context output kernel will read it: reference-order mode (k_attn_out reads it
    // only when strict), a context that reaches split_pos, rows of whole float4, and the caller did not opt out
    bool wants_value_t() const {
        return !(flags & (Q3_FLAG_FAST | Q3_FLAG_NO_VALUE_T)) && (cfg.seq_len % 4) == 0 && (int64_t)cfg.seq_len > (int64_t)split_pos &&
               dev_knob("Q3_VALUE_T", 1) != 0;
    }
    BatchCtx* batch = nullptr;                 // batched decode state (q3_batch_init), see q3_batch_host.inc
    // device-side Sampler (q3_sampler_set): temperature > 0 makes every token draw go through the draw site's launches
    bool sampling = false;
    DrawSite draw;                       // one column, with the pipelined draw's hist / counts: allocated by the first q3_sampler_set
    std::vector<Launch> sample_plan;     // the draw behind a forward (build_sample_plans)
    // top-k sampling (q3_sampler_top_k, section 2n): engine-wide, 0 = off.  The value also stands in device memory, where every
    // top-k pass reads it; the slices' lists hold the columns of the widest pass (kSpecMax).  Allocated by the first k > 0.
    int top_k = 0;
    DevMem<int> d_top_k;
    DevMem<unsigned long long> d_topk_keys;
    std::vector<Launch> sample_plan_topk;    // the second form of sample_plan: the top-k launches, once both exist
    TopkArgs topk_args(const SampleArgs& s) const { return ::topk_args(s, d_top_k, d_topk_keys); }
    int build_sample_plans();
    // log-probabilities of generated tokens (q3_gen_logprobs, section 2o): engine-wide, -1 = off; 0: a record per token the
    // q3_generate_many_* loops produce; 1 .. kScoreTopMax: also that many best tokens and the rank.  What it needs on the device
    // belongs to the batched state (genlp_alloc, q3_cols_host.inc)
    int gen_logprobs = -1;
    // presence and frequency penalties (q3_sampler_penalties, section 2p): engine-wide, (0, 0) = off.  The values also stand in device
    // memory, in the batched state (pen_alloc, q3_cols_host.inc), where every pass under the setting reads them
    float pen_presence = 0.0f, pen_frequency = 0.0f;
    bool pen_on() const { return pen_presence != 0.0f || pen_frequency != 0.0f; }
    // logit bias, banned and allowed tokens (q3_logit_bias_set, section 2q): engine-wide, no list = off.  Every generate call under a
    // table sends it to the device (bias_call_begin, q3_plan_host.inc)
    BiasTable bias;
    // the guide (q3_guide_set, section 2r): engine-wide, no state = off.  Its table goes to the device once, start[] with every
    // generate call under it (guide_call_begin, q3_plan_host.inc)
    GuideTable guide;
    unsigned long long guide_serial = 0;
    // the sparse guide (q3_guide_set_sparse, section 2s): the same rule on a compressed table; at most one of the two forms holds
    GuideSparse guide_sp;
    // the stop automaton (q3_stop_seq_set, section 2t): section 2s's arrays, read by the scheduler of the stop loop and by nothing else
    GuideSparse stop_seq;
    // the form of the column plans the q3_generate_many_* loops run (PlanKey::pen): under a guide the masked one of its form, whatever
    // the table and the penalties; under a table the adjusted one, whatever the penalties
    int pen_form() const { return guide_sp.n_states ? kPenGuideSp : guide.n_states ? kPenGuide : (bias.n_lists() ? kPenAdj : (pen_on() ? kPenOn : kPenOff)); }
    int enqueue_sample();

    int load(const char* path, uint32_t ctx_len);
    int build_plan();
    int capture();
    int enqueue_forward(size_t pos, bool draw = true);
    int set_state(size_t token, size_t pos);
    ~q3_engine() { batch_free(this); }       // the batched state, then the members in reverse order: the stream last
};

namespace {

// ---- attention: one resolver per kernel family (the only place an instantiation is named), and the launch shape that goes with it
struct AttnShape { AttnFn fn; dim3 grid, block; size_t smem; int kvm; };

AttnFn attn_out_fn(int slice_w, bool p_lds) {
    switch (slice_w) {
        case 8: return p_lds ? (AttnFn)k_attn_out<8, true> : (AttnFn)k_attn_out<8, false>;
        case 16: return p_lds ? (AttnFn)k_attn_out<16, true> : (AttnFn)k_attn_out<16, false>;
        case 32: return p_lds ? (AttnFn)k_attn_out<32, true> : (AttnFn)k_attn_out<32, false>;
        default: return p_lds ? (AttnFn)k_attn_out<0, true> : (AttnFn)k_attn_out<0, false>;
    }
}
AttnFn attn_scores_fn(int kvm) { return kvm == 4 ? (AttnFn)k_attn_scores_kv<4> : kvm == 2 ? (AttnFn)k_attn_scores_kv<2> : (AttnFn)k_attn_scores; }

// k_attn_scores_kv applies to head_dim 128 with 2 or 4 query heads per kv head (every listed Qwen3 size up to 8B)
AttnShape attn_scores_shape(int hd, int n_heads, int n_kv_heads, int S) {
    const int kv_mul = n_heads / n_kv_heads;
    AttnShape r;
    r.kvm = (hd != kSgHd || (kv_mul != 2 && kv_mul != 4) || !dev_knob("Q3_ATT_SCORES_KV", 1)) ? 0 : kv_mul;
    const int tch = r.kvm == 4 ? sg_tch<4>() : r.kvm == 2 ? sg_tch<2>() : attn_tch(hd);
    r.fn = attn_scores_fn(r.kvm);
    r.grid = dim3((unsigned)(r.kvm ? n_kv_heads : n_heads), (unsigned)((S + tch - 1) / tch));
    r.block = dim3(kWG);
    r.smem = r.kvm == 4 ? attn_scores_kv_smem_bytes<4>() : r.kvm == 2 ? attn_scores_kv_smem_bytes<2>() : attn_scores_smem_bytes(hd);
    return r;
}
AttnShape attn_out_shape(int hd, int n_heads, int S, int slice_w) {
    return AttnShape{attn_out_fn(slice_w, attn_out_p_in_lds(S)), dim3((unsigned)n_heads, (unsigned)(hd / slice_w)), dim3(kAoThreads),
                     attn_out_smem_bytes(hd, S, slice_w), 0};
}
// Short-context attention (pos < 256): k_attn_short2 (round 5: coalesced key / value staging, product tile, 8 waves) for
// head_dim 128 on caches of a whole number of 8-row steps; k_attn_short (head_dim 64, odd test contexts) otherwise.
AttnShape attn_short_shape(int hd, int n_heads, int S) {
    if (hd == 128 && S >= 8 && (S % 8) == 0)
        return AttnShape{(AttnFn)k_attn_short2<128>, dim3((unsigned)n_heads, 2), dim3(kS2Threads), attn_short2_smem_bytes(128, kS2MaxT), 0};
    return AttnShape{hd == 128 ? (AttnFn)k_attn_short<128> : (AttnFn)k_attn_short<64>, dim3((unsigned)n_heads), dim3(kWG), 0, 0};
}

inline int att_stride_for(size_t S) { return (int)((S + 255) & ~(size_t)255); }                    // floats per score row
inline int cmax_stride_for(size_t S) { return (int)(((S + 63) / 64 + 63) & ~(size_t)63); }         // 64-block maxima per score row

// Long-context split of one attention launch `a`: A = k_attn_scores[_kv] over (heads | kv heads) x T-chunks, B = k_attn_out over
// heads x slices.  att: [n_heads][att_stride] score rows; cmax: [n_heads][cmax_stride] their 64-block maxima (k_attn_scores_kv only);
// att_priv: [n_heads][slices][att_stride].  The engine's long plan and q3_op_attention both build the pair here.
int make_split_attn(Launch& A, Launch& B, AttnArgs a, float* att, float* cmax, float* att_priv, int n_cu) {
    const AttnShape ss = attn_scores_shape(a.hd, a.n_heads, a.n_kv_heads, a.seq_len);
    a.xbq = nullptr;                  // the split kernels write f32 xb only; Wo quantizes in its prologue
    a.att_global = att;
    a.att_stride = att_stride_for(a.seq_len);
    a.att_cmax = (ss.kvm && dev_knob("Q3_ATT_CMAX", 1)) ? cmax : nullptr;
    a.cmax_stride = cmax_stride_for(a.seq_len);
    AttnArgs sa = a, oa = a;
    // developer timeline of the long plan: k_attn_out's (Q3_STAMP_SCORES=1: k_attn_scores')
    if (dev_knob("Q3_STAMP_SCORES", 0)) oa.stamps = nullptr;
    else sa.stamps = nullptr;
    oa.att_priv = att_priv;
    oa.slice_w = attn_slice_w(a.hd, a.n_heads, n_cu);
    const AttnShape os = attn_out_shape(a.hd, a.n_heads, a.seq_len, oa.slice_w);
    int rc;
    if ((rc = make_launch(A, F_ATTN, ss.fn, ss.grid, ss.block, ss.smem, sa))) return rc;
    return make_launch(B, F_ATTN, os.fn, os.grid, os.block, os.smem, oa);
}

// Tile shape + grid for one GEMV launch.  units = output rows (SwiGLU: hidden units, each 2 weight rows).
// JU follows the row length (1 KiB chunks per row); RU is the largest row count per wave batch that keeps
// every wave of the grid busy and minimises max rows per wave; larger kernels grid-stride over batches.
struct GemvShape { int RU, JU; unsigned grid; int FIN, PF; };
GemvShape plan_gemv(int units, int n, int G, bool swiglu, int row_align, int n_cu, int wg_per_cu, bool allow_fin = true) {
    GemvShape g;
    g.FIN = 0;
    g.PF = 0;
    // launches that stream >= 16 MB are bandwidth- rather than latency-bound: give them a second workgroup per CU
    const size_t launch_bytes = (size_t)units * (swiglu ? 2 : 1) * (size_t)n;
    if (launch_bytes >= (16u << 20) && wg_per_cu < 2) wg_per_cu = 2;
    // chunks (1 KiB wave-loads) per tile row: the largest JU <= 4 that tiles the row exactly (every lane of every load
    // inside the row: the kernel's clamp-free fast path); rows that are not a whole number of wave-loads (2560, 9728)
    // take the JU that wastes the fewest clamped loads
    const int nchunks = n / 16, nj = (n + 1023) / 1024;
    g.JU = 0;
    for (int ju = 4; ju >= 1; --ju)
        if (nchunks % (64 * ju) == 0) { g.JU = ju; break; }
    if (g.JU == 0) {
        int best_waste = 1 << 30;
        for (int ju = 4; ju >= 1; --ju) {
            const int waste = ((nj + ju - 1) / ju) * ju * 64 - nchunks;
            if (waste < best_waste) { best_waste = waste; g.JU = ju; }
        }
    }
    const int ru_max = 8 / g.JU, ru_min = swiglu ? 2 : 1;
    const int waves = n_cu * wg_per_cu * kWaves;
    // rows that are a whole number of tiles fold the group terms in registers (k_gemv FIN = 1)
    if (allow_fin && dev_knob("Q3_GEMV_FIN", 1) && G == 64 && (nchunks % 4) == 0 &&
        launch_bytes < ((size_t)dev_knob("Q3_GEMV_FIN_MAXMB", 1 << 20) << 20)) g.FIN = 1;
    int best_ru = ru_min;
    long best_cost = -1;
    for (int ru = ru_max; ru >= ru_min; ru >>= 1) {
        if (G != 64 && ru != ru_min) continue;
        const int hu = swiglu ? ru / 2 : ru;
        if (row_align > 1 && row_align % hu) continue;   // QKV: batches must not straddle q|k|v segments
        const long nb = (units + hu - 1) / hu;
        const long per_wave = (nb + waves - 1) / waves;
        // latency-bound launches (<= 2 batches per wave): fewest sequential rows per wave wins;
        // streaming launches: the largest tile (most bytes in flight per wave) wins.
        const long cost = per_wave <= 2 ? per_wave * ru * 1000 + (ru_max - ru) : 1000000 + (ru_max - ru);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_ru = ru; }
    }
    g.RU = best_ru;
    const int hu = swiglu ? g.RU / 2 : g.RU;
    const long nb = (units + hu - 1) / hu;
    long grid = (nb + kWaves - 1) / kWaves;
    if (grid > (long)n_cu * wg_per_cu) grid = (long)n_cu * wg_per_cu;
    if (grid < 1) grid = 1;
    g.grid = (unsigned)grid;
    // streaming launches (every wave owns at least two tiles): request the second tile before the prologue too
    const long njt_h = (nj + g.JU - 1) / g.JU;
    if (dev_knob("Q3_GEMV_PF", 1) && G == 64 && nb * njt_h >= 2 * grid * kWaves && (g.FIN || !allow_fin)) g.PF = 1;
    return g;
}

// grid / block / LDS of a specialised launch: one row batch (hu rows or hidden units) per wave and round; at least one
// workgroup per CU as long as there are batches for it (fewer batches than waves: see k_gemv's wave numbering)
struct GemvLaunch { GemvFn fn = nullptr; unsigned grid = 1, block = kWG; size_t smem = 0; };
void apply_cfg(GemvLaunch& Ln, GemvArgs& a, const GemvCfg& c, int units, int n_cu) {
    const int waves = c.wgt / 64;
    const int hu = (c.epi == EPI_SWIGLU) ? c.ru / 2 : c.ru;
    const long nb = ((long)units + hu - 1) / hu;
    const int wg_per_cu = c.wgt >= 1024 ? 1 : (c.wgt >= 512 ? 2 : 4);
    long grid = (nb + waves - 1) / waves;
    const long lower = nb < n_cu ? nb : n_cu;
    if (grid < lower) grid = lower;
    if (grid > (long)n_cu * wg_per_cu) grid = (long)n_cu * wg_per_cu;
    a.vr = c.ru;
    Ln.fn = c.fn;
    Ln.grid = (unsigned)grid;
    Ln.block = (unsigned)c.wgt;
    // f32 staging only for the long vectors' block transpose (wave 0 sums out of registers)
    const bool stage = (c.pro == PRO_NORM || c.pro == PRO_EMBED_NORM) && c.n >= 1024;
    Ln.smem = gemv_smem_bytes(c.n, 64, c.ru, stage, waves, true);
}

// Kernel, grid, block and LDS size of one fused GEMV role (prologue, epilogue) at contraction length n: the shape-specialised
// table entry when there is one, the generic run-time-n kernel otherwise.  units = output rows (SwiGLU: hidden units);
// hd = head_dim for EPI_QKV (row batches must not straddle the q|k|v segments), 1 otherwise.  build_plan and the operator
// entry point q3_op_gemv_role both select through this function.
int plan_role(GemvLaunch& Ln, GemvArgs& a, int pro, int epi, int n, int units, int G, bool fast_fold, int hd, int n_cu) {
    const int small_cap = dev_knob("Q3_WG_PER_CU_SMALL", 2);   // two workgroups per CU: half the rows (and fold chains) per wave
    const int big_cap = dev_knob("Q3_WG_PER_CU_LMHEAD", 2);   // all workgroups resident at once (the NORM prologue keeps ~190 VGPRs live)
    const bool norm = pro == PRO_NORM || pro == PRO_EMBED_NORM;
    const GemvCfg* cfg = find_cfg(pro, epi, n, G, fast_fold);
    if (cfg && epi == EPI_QKV && (hd % cfg->ru) != 0) cfg = nullptr;           // batches must not straddle the q|k|v segments
    if (cfg) {
        apply_cfg(Ln, a, *cfg, units, n_cu);
        if (epi == EPI_LOGITS) {
            // streaming launch: cap the grid at the resident set (grid-stride over the row batches)
            const unsigned cap = (unsigned)(n_cu * (cfg->wgt >= 512 ? 1 : 2));
            if (Ln.grid > cap) Ln.grid = cap;
        }
    } else {
        const GemvShape gs = epi == EPI_LOGITS ? plan_gemv(units, n, G, false, 1, n_cu, big_cap, false)
                                               : plan_gemv(units, n, G, epi == EPI_SWIGLU, epi == EPI_QKV ? hd : 1, n_cu, small_cap);
        Ln.fn = q3inst::gemv_pick(pro, epi, G, gs.RU, gs.JU, epi == EPI_LOGITS ? 0 : gs.FIN, gs.PF);
        a.vr = gs.RU;
        Ln.grid = gs.grid;
        Ln.smem = gemv_smem_bytes(n, G, a.vr, norm);
    }
    if (!Ln.fn) return fail(Q3_ERR_UNSUPPORTED, "no kernel instantiated for this tile shape");
    return Q3_OK;
}

}  // namespace

// utils.rs MemoryMapper + qwen3.rs:199-277 load_weights: walk the file with a cursor, upload it once.
int q3_engine::load(const char* path, uint32_t ctx_len) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(Q3_ERR_IO, "Failed to open checkpoint: %s: %s", path, strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size <= 0) {
        close(fd);
        return fail(Q3_ERR_IO, "Failed to create memory mapping: %s", path);
    }
    const size_t flen = (size_t)st.st_size;
    void* map = mmap(nullptr, flen, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (map == MAP_FAILED) return fail(Q3_ERR_IO, "Failed to create memory mapping: %s", path);
    struct Unmap {
        void* p;
        size_t n;
        ~Unmap() { munmap(p, n); }
    } unmap{map, flen};
    const uint8_t* base = (const uint8_t*)map;

    int rc = parse_header(base, flen, &cfg);
    if (rc) return rc;
    if (ctx_len != 0 && (int64_t)ctx_len < (int64_t)cfg.seq_len) cfg.seq_len = (int32_t)ctx_len;  // models/mod.rs:65-67
    if (cfg.architecture_id != 1) return fail(Q3_ERR_FORMAT, "Unknown architecture_id: %d", cfg.architecture_id);
    if ((rc = check_supported(cfg))) return rc;

    const size_t dim = cfg.dim, L = cfg.n_layers, hd = cfg.head_dim, V = cfg.vocab_size, H = cfg.hidden_dim;
    const size_t G = cfg.group_size, ahd = (size_t)cfg.n_heads * hd, kvd = (size_t)cfg.n_kv_heads * hd;

    // cursor walk (offsets only), mirroring get_f32_slice / get_bytes bounds errors (utils.rs:21-56)
    size_t off = kHeaderSize;
    bool ok = true;
    auto take = [&](size_t bytes, const char* what) -> size_t {
        if (!ok) return 0;
        if (off + bytes > flen) {
            fail(Q3_ERR_FORMAT, "Failed to read %s: Insufficient data: need %zu bytes, have %zu remaining", what, bytes, flen - off);
            ok = false;
            return 0;
        }
        const size_t o = off;
        off += bytes;
        return o;
    };
    struct QOff { size_t q, s; };
    auto take_q = [&](size_t count, size_t size_each, std::vector<QOff>& out) {   // models/mod.rs:83-110
        for (size_t i = 0; i < count; ++i) {
            QOff o;
            o.q = take(size_each, "quantized tensor data");
            o.s = take(4 * (size_each / G), "scale factors");
            out.push_back(o);
        }
    };
    const size_t o_rms_att = take(4 * L * dim, "attention normalization weights");
    const size_t o_rms_ffn = take(4 * L * dim, "FFN normalization weights");
    const size_t o_rms_final = take(4 * dim, "final normalization weights");
    const size_t o_q_ln = take(4 * L * hd, "query layer norm weights");
    const size_t o_k_ln = take(4 * L * hd, "key layer norm weights");
    std::vector<QOff> otok, owq, owk, owv, owo, ow1, ow2, ow3, ocls;
    take_q(1, V * dim, otok);
    take_q(L, dim * ahd, owq);
    take_q(L, dim * kvd, owk);
    take_q(L, dim * kvd, owv);
    take_q(L, ahd * dim, owo);
    take_q(L, dim * H, ow1);
    take_q(L, H * dim, ow2);
    take_q(L, dim * H, ow3);
    if (!cfg.shared_classifier) take_q(1, dim * V, ocls);
    if (!ok) return Q3_ERR_FORMAT;

    // every tensor must start 16-byte aligned for dwordx4 loads (true for all listed models: the header
    // is 256 B and every section size is a multiple of 16)
    auto aligned = [](size_t o) { return (o & 15) == 0; };
    bool all_aligned = aligned(o_rms_att) && aligned(o_rms_ffn) && aligned(o_rms_final) && aligned(o_q_ln) && aligned(o_k_ln);
    for (auto* v : {&otok, &owq, &owk, &owv, &owo, &ow1, &ow2, &ow3, &ocls})
        for (auto& o : *v) all_aligned = all_aligned && aligned(o.q) && aligned(o.s);
    if (!all_aligned) return fail(Q3_ERR_UNSUPPORTED, "checkpoint sections are not 16-byte aligned");

    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIP_TRY(hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking));

    // the whole file becomes one resident HBM blob, layout unchanged (zero repack)
    blob_bytes = off;
    if ((rc = d_blob.alloc(blob_bytes))) return rc;
    HIP_TRY(hipMemcpy(d_blob, base, blob_bytes, hipMemcpyHostToDevice));
    auto fp = [&](size_t o) { return (const float*)(d_blob + o); };
    auto qt = [&](const QOff& o) {
        QT t;
        t.q = (const int8_t*)(d_blob + o.q);
        t.s = (const float*)(d_blob + o.s);
        return t;
    };
    rms_att = fp(o_rms_att);
    rms_ffn = fp(o_rms_ffn);
    rms_final = fp(o_rms_final);
    q_ln = fp(o_q_ln);
    k_ln = fp(o_k_ln);
    tok = qt(otok[0]);
    for (size_t l = 0; l < L; ++l) {
        wq.push_back(qt(owq[l]));
        wk.push_back(qt(owk[l]));
        wv.push_back(qt(owv[l]));
        wo.push_back(qt(owo[l]));
        w1.push_back(qt(ow1[l]));
        w2.push_back(qt(ow2[l]));
        w3.push_back(qt(ow3[l]));
    }
    wcls = cfg.shared_classifier ? tok : qt(ocls[0]);   // qwen3.rs:252-253

    // run state (qwen3.rs:414-445); KV cache zero-filled: generate mode attends over never-written rows
    const size_t S = cfg.seq_len;
    const size_t kv_elems = L * S * kvd;
    if ((rc = d_x.alloc(dim)) || (rc = d_q.alloc(ahd)) || (rc = d_kraw.alloc(kvd)) || (rc = d_xb.alloc(ahd)) || (rc = d_hb.alloc(H)) ||
        (rc = d_logits.alloc(V)) || (rc = d_tap.alloc(dim)) || (rc = d_key.alloc(kv_elems)) || (rc = d_value.alloc(kv_elems)))
        return rc;
    HIP_TRY(hipMemset(d_key, 0, 4 * kv_elems));
    HIP_TRY(hipMemset(d_value, 0, 4 * kv_elems));
    // the long-context plan streams a transposed copy of the value rows (k_attn_out, strict mode only; contexts that can reach the
    // split position only -- split_pos is set here, once, and build_plan uses the same value)
    split_pos = dev_knob("Q3_ATT_SPLIT_POS", 256);
    if (wants_value_t()) {
        if ((rc = d_value_t.alloc(kv_elems))) return rc;
        HIP_TRY(hipMemset(d_value_t, 0, 4 * kv_elems));
    }
    HIP_TRY(hipMemset(d_x, 0, 4 * dim));
    if ((rc = d_state.alloc(1))) return rc;
    HIP_TRY(hipMemset(d_state, 0, sizeof(State)));
    out_cap = (int)S;
    if ((rc = d_out_tokens.alloc((size_t)out_cap))) return rc;
    HIP_TRY(hipMemset(d_out_tokens, 0, 4 * (size_t)out_cap));
    if ((rc = d_prompt.alloc((size_t)out_cap))) return rc;
    HIP_TRY(hipMemset(d_prompt, 0, 4 * (size_t)out_cap));
    if ((rc = h_logits.alloc(V)) || (rc = h_state.alloc(1)) || (rc = h_tokens.alloc((size_t)out_cap))) return rc;

    // RoPE table with the host libm, exactly RoPE::compute_freqs (layers.rs:161-171)
    {
        const size_t half = hd / 2;
        std::vector<float> tab(S * hd);
        std::vector<float> freq(half);
        for (size_t i = 0; i < half; ++i) freq[i] = powf(1e6f, -((float)i) / (float)half);
        for (size_t p = 0; p < S; ++p)
            for (size_t i = 0; i < half; ++i) {
                const float angle = (float)p * freq[i];
                tab[p * hd + 2 * i] = cosf(angle);
                tab[p * hd + 2 * i + 1] = sinf(angle);
            }
        if ((rc = d_rope.alloc(tab.size()))) return rc;
        HIP_TRY(hipMemcpy(d_rope, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice));
    }
    return Q3_OK;
}

// The per-token kernel chain, in the order of TransformerBlock::forward (qwen3.rs:131-176)
int q3_engine::build_plan() {
    const int dim = cfg.dim, L = cfg.n_layers, hd = cfg.head_dim, V = cfg.vocab_size, H = cfg.hidden_dim;
    const int G = cfg.group_size, ahd = cfg.n_heads * hd, kvd = cfg.n_kv_heads * hd, S = cfg.seq_len;
    const int strict = (flags & Q3_FLAG_FAST) ? 0 : 1;
    const bool fast_fold = !strict && dev_knob("Q3_FAST_FOLD", 1) != 0;   // tolerance mode: tree fold of the GEMV group terms too
    const int att_lds_max = dev_knob("Q3_ATT_LDS_MAX", 4096);

    const int att_stride = att_stride_for(S), cmax_stride = cmax_stride_for(S);
    const int slice_w = attn_slice_w(hd, cfg.n_heads, n_cu);
    const int nsl = hd / slice_w;
    const bool use_att_global = S > att_lds_max;
    int rc;
    if ((rc = d_att.alloc((size_t)cfg.n_heads * ((size_t)att_stride + cmax_stride)))) return rc;   // score rows, then their 64-block maxima
    if ((rc = d_att_priv.alloc((size_t)cfg.n_heads * nsl * att_stride))) return rc;
    kstamps = dev_knob("Q3_KSTAMPS", 0) != 0;
    if (dev_knob("Q3_STAMPS", 0) || kstamps) {
        if ((rc = d_stamps.alloc(16 * (size_t)(5 * L + 4)))) return rc;
        HIP_TRY(hipMemset(d_stamps, 0, 8 * 16 * (size_t)(5 * L + 4)));
    }
#ifdef Q3_DEV
    if (kstamps) {
        const size_t nl = (size_t)(5 * L + 4);
        if ((rc = d_kslots.alloc(2 * (size_t)kKstampSlots * nl))) return rc;
        HIP_TRY(hipMemset(d_kslots, 0, 16 * (size_t)kKstampSlots * nl));
        if ((rc = d_kcells.alloc(2 * nl)) || (rc = d_knslots.alloc(nl))) return rc;
        HIP_TRY(hipMemset(d_knslots, 0, 4 * nl));
        if ((rc = d_kacc.alloc(2 + 2 * nl))) return rc;
        HIP_TRY(hipMemset(d_kacc, 0, 8 * (2 + 2 * nl)));
    }
#endif

    auto base_args = [&](int n) {
        GemvArgs a{};
        a.n = n;
        a.group = G;
        a.strict = strict;
        a.debug = kstamps ? 64 : 0;
        a.st = d_state;
        a.seq_len = S;
        return a;
    };
    // developer timelines: the cells of the launch about to be appended to `plan` (tools/kstamps.py and the *_stamps.py tools index by it)
    auto stamp_cells = [&]() -> unsigned long long* {
        if (!d_stamps) return nullptr;
        return kstamps ? d_kslots + 2 * (size_t)kKstampSlots * plan.size() : d_stamps + 16 * plan.size();
    };
    auto stamp = [&](GemvArgs& a) {
        if (d_stamps) { a.stamps = stamp_cells(); a.stamp_block = dev_knob("Q3_STAMP_BLOCK", 7); }
    };
    // one fused GEMV role: resolve kernel and shape (plan_role), stamp, record
    auto gemv = [&](Launch& Ln, Family fam, GemvArgs a, int pro, int epi, int n, int units, int qkv_hd, bool stamped) -> int {
        GemvLaunch g;
        if ((rc = plan_role(g, a, pro, epi, n, units, G, fast_fold, qkv_hd, n_cu))) return rc;
        if (stamped) stamp(a);
        return make_launch(Ln, fam, g.fn, dim3(g.grid), dim3(g.block), g.smem, a);
    };
    auto push_both = [&](const Launch& Ln) { plan.push_back(Ln); plan_long.push_back(Ln); };
    if ((rc = d_xbq.alloc((size_t)ahd)) || (rc = d_xbs.alloc((size_t)(ahd / G)))) return rc;
    Launch Ln;
    for (int l = 0; l < L; ++l) {
        const size_t kv_off = (size_t)l * S * kvd;
        {   // xb = RMSNorm_att(x); xq = quantize(xb); q,k,v = W{q,k,v} xq         qwen3.rs:134-136, layers.rs:334-337
            GemvArgs a = base_args(dim);
            a.seg[0] = Seg{wq[l].q, wq[l].s, d_q, ahd, 0};
            a.seg[1] = Seg{wk[l].q, wk[l].s, d_kraw, kvd, 0};
            a.seg[2] = Seg{wv[l].q, wv[l].s, d_value + kv_off, kvd, kvd};
            a.v_t = d_value_t ? d_value_t + kv_off : nullptr;
            a.total_rows = ahd + 2 * kvd;
            for (int k = 0; k < 2; ++k) {
                a.qkv_dw[k] = (const char*)a.seg[k + 1].wq - (const char*)a.seg[k].wq;
                a.qkv_ds[k] = (const char*)a.seg[k + 1].ws - (const char*)a.seg[k].ws;
                a.qkv_do[k] = (const char*)a.seg[k + 1].out - (const char*)a.seg[k].out;
            }
            a.norm_w = rms_att + (size_t)l * dim;
            a.in = d_x;
            if (l == 0) {
                a.emb_q = tok.q;
                a.emb_s = tok.s;
                a.x_out = d_x;
            }
            if ((rc = gemv(Ln, F_QKV, a, l == 0 ? PRO_EMBED_NORM : PRO_NORM, EPI_QKV, dim, a.total_rows, hd, true))) return rc;
            push_both(Ln);
        }
        // the short plan only ever runs at pos < split_pos
        const bool att_short = (hd == 64 || hd == 128) && split_pos <= kShortMaxT && dev_knob("Q3_ATT_SHORT", 1);
        // k_attn_short can hand Wo its operand quantized (qwen3.rs:152 fused into the attention epilogue)
        const GemvCfg* wo_preq = att_short ? find_cfg(PRO_PREQR, EPI_RESID, ahd, G, fast_fold) : nullptr;
        {   // QK-norm + RoPE + attention                                        layers.rs:346-419
            AttnArgs a{};
            a.q = d_q;
            a.key_cache = d_key + kv_off;
            a.k_raw = d_kraw;
            a.value_cache = d_value + kv_off;
            a.value_t = d_value_t ? d_value_t + kv_off : nullptr;
            a.q_norm_w = q_ln + (size_t)l * hd;
            a.k_norm_w = k_ln + (size_t)l * hd;
            a.rope = d_rope;
            a.xb = d_xb;
            a.att_global = use_att_global ? d_att : nullptr;
            a.st = d_state;
            a.pos_override = -1;
            attn_set_heads(a, cfg.n_heads, cfg.n_kv_heads);
            a.hd = hd;
            a.seq_len = S;
            a.strict = strict;
            a.write_q = 0;
            a.debug = kstamps ? 64 : 0;
            a.stamps = stamp_cells();
            if (wo_preq) {
                a.xbq = d_xbq;
                a.xbs = d_xbs;
                a.xb_group = G;
            }
            // long-context plan: the attention launch becomes k_attn_scores (heads x T-chunks) + k_attn_out (heads x slices)
            Launch A, B;
            if ((rc = make_split_attn(A, B, a, d_att, d_att + (size_t)cfg.n_heads * att_stride, d_att_priv, n_cu))) return rc;
            plan_long.push_back(A);
            plan_long.push_back(B);
            if (att_short) {
                const AttnShape sh = attn_short_shape(hd, cfg.n_heads, S);
                rc = make_launch(Ln, F_ATTN, sh.fn, sh.grid, sh.block, sh.smem, a);
            } else {
                rc = make_launch(Ln, F_ATTN, k_attn, dim3((unsigned)cfg.n_heads), dim3(kWG), attn_smem_bytes(hd, use_att_global ? 0 : S), a);
            }
            if (rc) return rc;
            plan.push_back(Ln);
        }
        {   // xq = quantize(xb); x += Wo xq                                      qwen3.rs:152-156
            GemvArgs a = base_args(ahd);
            a.seg[0] = Seg{wo[l].q, wo[l].s, d_x, dim, 0};
            a.total_rows = dim;
            a.in = d_xb;
            a.pre_q = d_xbq;
            a.pre_s = d_xbs;
            // quantize-in-prologue form: the long-context plan always (k_attn_out emits no quantized operand; no timeline), the short
            // plan when attention emits no int8
            if ((rc = gemv(Ln, F_WO, a, PRO_QUANT, EPI_RESID, ahd, dim, 1, false))) return rc;
            plan_long.push_back(Ln);
            if ((rc = gemv(Ln, F_WO, a, wo_preq ? PRO_PREQR : PRO_QUANT, EPI_RESID, ahd, dim, 1, true))) return rc;
            plan.push_back(Ln);
        }
        {   // xb = RMSNorm_ffn(x); xq = quantize(xb); hb = silu(W1 xq) * (W3 xq)   qwen3.rs:159-161, layers.rs:468-475
            GemvArgs a = base_args(dim);
            a.seg[0] = Seg{w1[l].q, w1[l].s, d_hb, H, 0};
            a.seg[1] = Seg{w3[l].q, w3[l].s, nullptr, H, 0};
            a.total_rows = 2 * H;
            a.norm_w = rms_ffn + (size_t)l * dim;
            a.in = d_x;
            if ((rc = gemv(Ln, F_W13, a, PRO_NORM, EPI_SWIGLU, dim, H, 1, true))) return rc;
            push_both(Ln);
        }
        {   // hq = quantize(hb); x += W2 hq                                      layers.rs:478-479, qwen3.rs:175
            GemvArgs a = base_args(H);
            a.seg[0] = Seg{w2[l].q, w2[l].s, d_x, dim, 0};
            a.total_rows = dim;
            a.in = d_hb;
            if ((rc = gemv(Ln, F_W2, a, PRO_QUANT, EPI_RESID, H, dim, 1, true))) return rc;
            push_both(Ln);
        }
    }
    {   // x = RMSNorm_final(x); xq = quantize(x); logits = Wcls xq + argmax, state update and token store (qwen3.rs:72-76, generation.rs)
        GemvArgs a = base_args(dim);
        a.seg[0] = Seg{wcls.q, wcls.s, d_logits, V, 0};
        a.total_rows = V;
        a.norm_w = rms_final;
        a.in = d_x;
        a.tap_out = d_tap;
        GemvLaunch g;
        if ((rc = plan_role(g, a, PRO_NORM, EPI_LOGITS, dim, V, G, fast_fold, 1, n_cu))) return rc;
        n_argmax_slots = (int)g.grid;
        if ((rc = d_argmax_slots.alloc((size_t)n_argmax_slots))) return rc;
        HIP_TRY(hipMemset(d_argmax_slots, 0, 8 * (size_t)n_argmax_slots));
        a.argmax_slots = d_argmax_slots;
        stamp(a);
        if ((rc = d_next_cell.alloc(2))) return rc;
        HIP_TRY(hipMemset(d_next_cell, 0, 16));
        a.next_cell = d_next_cell;
        a.out_tokens = d_out_tokens;
        a.out_cap = out_cap;
        a.prompt = d_prompt;
        if ((rc = make_launch(Ln, F_LMHEAD, g.fn, dim3(g.grid), dim3(g.block), g.smem, a))) return rc;
        push_both(Ln);
        a.next_cell = nullptr;
        if ((rc = make_launch(lm_plain, F_LMHEAD, g.fn, dim3(g.grid), dim3(g.block), g.smem, a))) return rc;
    }
    n_token_launches = plan.size();
#ifdef Q3_DEV
    if (kstamps) {
        // per launch: live wave slots; behind the token's last launch: k_kstamp_reduce + k_kstamp_fold
        const int nl = (int)n_token_launches;
        std::vector<int> ns(plan.size(), 0);
        for (size_t i = 0; i < plan.size(); ++i) {
            const long w = (long)plan[i].grid.x * plan[i].grid.y * (plan[i].block.x / 64);
            ns[i] = (int)(w < kKstampSlots ? w : kKstampSlots);
        }
        HIP_TRY(hipMemcpy(d_knslots, ns.data(), 4 * ns.size(), hipMemcpyHostToDevice));
        if ((rc = make_launch(Ln, F_NEXT, k_kstamp_reduce, dim3((unsigned)nl), dim3(256), 0, d_kslots, d_knslots, d_kcells))) return rc;
        push_both(Ln);
        if ((rc = make_launch(Ln, F_NEXT, k_kstamp_fold, dim3(1), dim3(256), 0, d_kcells, nl, d_kacc))) return rc;
        push_both(Ln);
    }
#endif
    return Q3_OK;
}

int q3_engine::capture() {
    const size_t lbytes = 4 * (size_t)cfg.vocab_size;
    const bool fwd = dev_knob("Q3_FWD_GRAPH", 1) != 0;
    for (int lng = 0; lng < 2; ++lng) {
        const std::vector<Launch>& P = lng ? plan_long : plan;
        int rc = decode[lng].capture(stream, [&] {
            for (const Launch& L : P) launch(L, stream);
            return Q3_OK;
        });
        if (rc == Q3_OK && fwd)
            rc = forward[lng].capture(stream, [&]() -> int {
                HIP_TRY(hipMemcpyAsync(d_state, h_state, sizeof(State), hipMemcpyHostToDevice, stream));
                for (const Launch& L : P) launch(L, stream);
                HIP_TRY(hipMemcpyAsync(h_logits, d_logits, lbytes, hipMemcpyDeviceToHost, stream));
                return Q3_OK;
            });
        if (rc) return rc;
    }
    return Q3_OK;
}

// draw = false: logits only (q3_forward: the caller samples, the device sampler must not consume a coin)
int q3_engine::enqueue_forward(size_t pos, bool draw) {
    const int lng = (int64_t)pos >= (int64_t)split_pos ? 1 : 0;
    if (decode[lng]) {
        int rc = decode[lng].launch(stream);
        if (rc) return rc;
    } else {
        for (const Launch& L : (lng ? plan_long : plan)) launch(L, stream);
        HIP_TRY(hipGetLastError());
    }
    return draw ? enqueue_sample() : Q3_OK;
}

// Sampler::sample on the logits of the forward just enqueued (after the classifier launch has advanced the state)
int q3_engine::enqueue_sample() {
    if (!sampling) return Q3_OK;
    for (const Launch& L : (top_k > 0 ? sample_plan_topk : sample_plan)) launch(L, stream);
    HIP_TRY(hipGetLastError());
    return Q3_OK;
}

// sample_plan and, once the top-k lists exist too, its second form, from the site's arguments as the last q3_sampler_set left
// them (q3_sampler_set / q3_sampler_top_k, in either order)
int q3_engine::build_sample_plans() {
    sample_plan.clear();
    sample_plan_topk.clear();
    if (!draw) return Q3_OK;
    const auto into = [](std::vector<Launch>& plan) {
        return [&plan](auto kernel, dim3 grid, dim3 block, size_t smem, const auto& a) {
            Launch L;
            const int rc = make_launch(L, F_NEXT, kernel, grid, block, smem, a);
            if (rc == Q3_OK) plan.push_back(L);
            return rc;
        };
    };
    if (int rc = draw_launches(draw, 1, (unsigned)n_cu, nullptr, into(sample_plan))) return rc;
    if (!d_top_k) return Q3_OK;
    const TopkArgs t = topk_args(draw.args);
    return draw_launches(draw, 1, (unsigned)n_cu, &t, into(sample_plan_topk));
}

int q3_engine::set_state(size_t token, size_t pos) {
    if (token >= (size_t)cfg.vocab_size || pos >= (size_t)cfg.seq_len)
        return fail(Q3_ERR_ARG, "index out of range: token %zu (vocab_size %d), pos %zu (seq_len %d)", token,
                    cfg.vocab_size, pos, cfg.seq_len);
    h_state->token = (int)token;
    h_state->pos = (int)pos;
    h_state->step = 0;
    h_state->prompt_len = 0;
    h_state->argmax = 0ull;
    HIP_TRY(hipMemcpyAsync(d_state, h_state, sizeof(State), hipMemcpyHostToDevice, stream));
    return Q3_OK;
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

const char* q3_last_error(void) { return g_err; }
uint32_t q3_abi_version(void) { return Q3_ABI_VERSION; }
// q3_build_id(): csrc/q3_build_id.cpp (its own object, rebuilt whenever any source changes)

int q3_parse_header(const uint8_t* data, size_t len, q3_config* out) {
    g_err[0] = 0;
    return parse_header(data, len, out);
}

int q3_create(const char* checkpoint_path, uint32_t ctx_len, int device, uint32_t flags, q3_engine** out) {
    g_err[0] = 0;
    if (!checkpoint_path || !out) return fail(Q3_ERR_ARG, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(Q3_ERR_HIP, "no HIP device available (libqwen3_hip has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(Q3_ERR_ARG, "device %d out of range (%d devices)", device, ndev);
    q3_engine* e = new q3_engine();
    e->flags = flags;
    e->device = device;
    int rc = e->load(checkpoint_path, ctx_len);
    if (rc == Q3_OK) rc = e->build_plan();
    if (rc == Q3_OK && !(flags & Q3_FLAG_NO_GRAPH)) rc = e->capture();
    if (rc != Q3_OK) {
        delete e;
        return rc;
    }
    *out = e;
    return Q3_OK;
}

void q3_destroy(q3_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    delete e;
}

int q3_get_config(const q3_engine* e, q3_config* out) {
    if (!e || !out) return fail(Q3_ERR_ARG, "null argument");
    *out = e->cfg;
    return Q3_OK;
}

const float* q3_forward(q3_engine* e, size_t token, size_t pos) {
    g_err[0] = 0;
    if (!e) {
        fail(Q3_ERR_ARG, "null engine");
        return nullptr;
    }
    static const bool dbg = getenv("Q3_DEBUG_TIMING") != nullptr;
    struct timespec t0, t1, t2, t3, t4;
    if (dbg) clock_gettime(CLOCK_MONOTONIC, &t0);
    if (hipSetDevice(e->device) != hipSuccess) { fail(Q3_ERR_HIP, "hipSetDevice failed"); return nullptr; }
    const int lng = (int64_t)pos >= (int64_t)e->split_pos ? 1 : 0;
    if (e->forward[lng] && !e->sampling) {
        // one graph launch: state upload, kernels, logits download (the three separate enqueues cost ~25 us of host time)
        if (token >= (size_t)e->cfg.vocab_size || pos >= (size_t)e->cfg.seq_len) {
            fail(Q3_ERR_ARG, "index out of range: token %zu (vocab_size %d), pos %zu (seq_len %d)", token, e->cfg.vocab_size, pos, e->cfg.seq_len);
            return nullptr;
        }
        e->h_state->token = (int)token;
        e->h_state->pos = (int)pos;
        e->h_state->step = 0;
        e->h_state->prompt_len = 0;
        e->h_state->argmax = 0ull;
        hipError_t ge = hipGraphLaunch(e->forward[lng].exec, e->stream);
        if (ge == hipSuccess) ge = hipStreamSynchronize(e->stream);
        if (ge != hipSuccess) {
            fail(Q3_ERR_HIP, "forward failed: %s", hipGetErrorString(ge));
            return nullptr;
        }
        return e->h_logits;
    }
    if (e->set_state(token, pos) != Q3_OK) return nullptr;
    if (dbg) clock_gettime(CLOCK_MONOTONIC, &t1);
    if (e->enqueue_forward(pos, false) != Q3_OK) return nullptr;
    if (dbg) clock_gettime(CLOCK_MONOTONIC, &t2);
    hipError_t err = hipMemcpyAsync(e->h_logits, e->d_logits, 4 * (size_t)e->cfg.vocab_size, hipMemcpyDeviceToHost, e->stream);
    if (dbg) clock_gettime(CLOCK_MONOTONIC, &t3);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err != hipSuccess) {
        fail(Q3_ERR_HIP, "forward failed: %s", hipGetErrorString(err));
        return nullptr;
    }
    if (dbg) {
        clock_gettime(CLOCK_MONOTONIC, &t4);
        auto us = [](const timespec& a, const timespec& b) { return (b.tv_sec - a.tv_sec) * 1e6 + (b.tv_nsec - a.tv_nsec) * 1e-3; };
        static int n = 0;
        if (++n % 16 == 0)
            fprintf(stderr, "[q3] forward: set_state %.1f us, graph launch %.1f us, D2H enqueue %.1f us, sync %.1f us\n",
                    us(t0, t1), us(t1, t2), us(t2, t3), us(t3, t4));
    }
    return e->h_logits;
}

int q3_forward_argmax(q3_engine* e, size_t token, size_t pos, int32_t* next_token) {
    g_err[0] = 0;
    if (!e || !next_token) return fail(Q3_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    int rc = e->set_state(token, pos);
    if (rc) return rc;
    if ((rc = e->enqueue_forward(pos))) return rc;
    HIP_TRY(hipMemcpyAsync(e->h_tokens, e->d_out_tokens, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *next_token = e->h_tokens[0];
    return Q3_OK;
}

int q3_generate_greedy(q3_engine* e, size_t first_token, size_t first_pos, size_t n_tokens, int32_t* out_tokens) {
    g_err[0] = 0;
    if (!e || (!out_tokens && n_tokens)) return fail(Q3_ERR_ARG, "null argument");
    if (n_tokens == 0) return Q3_OK;
    if (first_pos + n_tokens > (size_t)e->cfg.seq_len)
        return fail(Q3_ERR_ARG, "first_pos %zu + n_tokens %zu exceeds seq_len %d", first_pos, n_tokens, e->cfg.seq_len);
    HIP_TRY(hipSetDevice(e->device));
    int rc = e->set_state(first_token, first_pos);
    if (rc) return rc;
    struct timespec t0, t1, t2;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (size_t k = 0; k < n_tokens; ++k)
        if ((rc = e->enqueue_forward(first_pos + k))) return rc;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    HIP_TRY(hipMemcpyAsync(e->h_tokens, e->d_out_tokens, 4 * n_tokens, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    clock_gettime(CLOCK_MONOTONIC, &t2);
    if (e->d_stamps && !e->kstamps) {
        const size_t nl = e->plan.size();
        std::vector<unsigned long long> h(16 * nl);
        HIP_TRY(hipMemcpy(h.data(), e->d_stamps, 8 * 16 * nl, hipMemcpyDeviceToHost));
        double acc[F_COUNT][16] = {}; int cnt[F_COUNT] = {};
        for (size_t i = 0; i < nl; ++i) {
            if (e->plan[i].fam == F_NEXT || h[16 * i] == 0) continue;
            for (int k = 1; k < 16; ++k)
                if (h[16 * i + k] >= h[16 * i]) acc[e->plan[i].fam][k] += (double)(h[16 * i + k] - h[16 * i]);
            cnt[e->plan[i].fam]++;
        }
        for (int f = 0; f < F_COUNT; ++f)
            if (cnt[f]) fprintf(stderr, "[q3 stamps] %-8s n=%d  issue %.0f  prologue %.0f  tile %.0f  finish %.0f  end %.0f  (s_memtime ticks after entry)\n", kFamilyNames[f], cnt[f], acc[f][1] / cnt[f], acc[f][2] / cnt[f], acc[f][3] / cnt[f], acc[f][4] / cnt[f], acc[f][5] / cnt[f]);
        for (int f = 0; f < F_COUNT; ++f) if (cnt[f] && acc[f][7] > 0 && f != F_ATTN) fprintf(stderr, "[q3 stamps] %-8s prologue detail: x/sum start %.0f  sum end %.0f  quantized %.0f\n", kFamilyNames[f], acc[f][6] / cnt[f], acc[f][7] / cnt[f], acc[f][8] / cnt[f]);
        if (e->sampling) {
            unsigned long long hs[16];
            HIP_TRY(hipMemcpy(hs, e->d_stamps + 16 * (size_t)(5 * e->cfg.n_layers + 3), sizeof(hs), hipMemcpyDeviceToHost));
            if (hs[0]) fprintf(stderr, "[q3 stamps] sample (last draw): sum %llu  normalise %llu  histogram %llu  compaction %llu  sort %llu  cumulative walk %llu  cdf walk %llu  total %llu ticks, %llu candidates, %llu rounds of the exact denominator\n",
                               hs[1] - hs[0], hs[2] - hs[1], hs[3] - hs[2], hs[4] - hs[3], hs[5] - hs[4], hs[6] - hs[5], hs[7] - hs[6], hs[7] - hs[0], hs[9], hs[10]);
        }
        if (cnt[F_ATTN] && acc[F_ATTN][7] > 0) {           // k_attn_out: the chain wave in front of each chunk's barrier
            fprintf(stderr, "[q3 stamps] attn chain wave at the chunk barriers:");
            for (int k = 7; k < 16; ++k) fprintf(stderr, " %.0f", acc[F_ATTN][k] / cnt[F_ATTN]);
            fprintf(stderr, "\n");
        }
        if (cnt[F_ATTN]) fprintf(stderr, "[q3 stamps] attn: issued %.0f  norm %.0f  staged %.0f  scores %.0f  softmax %.0f  vsum %.0f\n", acc[F_ATTN][1] / cnt[F_ATTN], acc[F_ATTN][2] / cnt[F_ATTN], acc[F_ATTN][3] / cnt[F_ATTN], acc[F_ATTN][4] / cnt[F_ATTN], acc[F_ATTN][5] / cnt[F_ATTN], acc[F_ATTN][6] / cnt[F_ATTN]);
    }
#ifdef Q3_DEV
    if (e->kstamps && e->d_kacc) {
        // per family: average duration of a launch (first wave in .. last wave out) and average gap to its predecessor's end,
        // both from the in-kernel 100 MHz clock, averaged over every token folded so far; the sum over a token against the
        // host's wall clock for this call
        const size_t nl = e->n_token_launches;
        std::vector<unsigned long long> h(2 + 2 * nl);
        HIP_TRY(hipMemcpy(h.data(), e->d_kacc, 8 * h.size(), hipMemcpyDeviceToHost));
        const double ntok = (double)h[0];
        double dur[F_COUNT] = {}, gap[F_COUNT] = {}; int cnt[F_COUNT] = {};
        double tot = 0.0;
        for (size_t i = 0; i < nl; ++i) {
            const int f = e->plan[i].fam;
            dur[f] += (double)h[2 + 2 * i] * 0.01 / ntok;      // 10 ns ticks -> us
            gap[f] += (double)h[3 + 2 * i] * 0.01 / ntok;
            cnt[f]++;
            tot += ((double)h[2 + 2 * i] + (double)h[3 + 2 * i]) * 0.01 / ntok;
        }
        const double wall_us = ((t2.tv_sec - t0.tv_sec) * 1e6 + (t2.tv_nsec - t0.tv_nsec) * 1e-3) / (double)n_tokens;
        fprintf(stderr, "[q3 kstamps] {\"tokens_folded\": %.0f, \"sum_duration_plus_gap_us_per_token\": %.2f, \"wall_us_per_token_this_call\": %.2f, \"families\": {", ntok, tot, wall_us);
        bool first = true;
        for (int f = 0; f < F_COUNT; ++f)
            if (cnt[f] && f != F_NEXT) {
                fprintf(stderr, "%s\"%s\": {\"launches_per_token\": %d, \"avg_duration_us\": %.3f, \"avg_gap_to_predecessor_us\": %.3f}", first ? "" : ", ",
                        kFamilyNames[f], cnt[f], dur[f] / cnt[f], gap[f] / cnt[f]);
                first = false;
            }
        fprintf(stderr, "}}\n");
    }
#endif
    if (getenv("Q3_DEBUG_TIMING"))
        fprintf(stderr, "[q3] generate_greedy n=%zu enqueue %.1f us, drain %.1f us\n", n_tokens,
                (t1.tv_sec - t0.tv_sec) * 1e6 + (t1.tv_nsec - t0.tv_nsec) * 1e-3,
                (t2.tv_sec - t1.tv_sec) * 1e6 + (t2.tv_nsec - t1.tv_nsec) * 1e-3);
    memcpy(out_tokens, e->h_tokens, 4 * n_tokens);
    return Q3_OK;
}

int q3_prefill(q3_engine* e, const int32_t* tokens, size_t n_tokens, size_t first_pos, int32_t* next_token) {
    g_err[0] = 0;
    if (!e || !tokens || n_tokens == 0) return fail(Q3_ERR_ARG, "null or empty prompt");
    if (first_pos + n_tokens > (size_t)e->cfg.seq_len)
        return fail(Q3_ERR_ARG, "first_pos %zu + n_tokens %zu exceeds seq_len %d", first_pos, n_tokens, e->cfg.seq_len);
    for (size_t i = 0; i < n_tokens; ++i)
        if (tokens[i] < 0 || tokens[i] >= e->cfg.vocab_size)
            return fail(Q3_ERR_ARG, "index out of range: token %d (vocab_size %d)", tokens[i], e->cfg.vocab_size);
    HIP_TRY(hipSetDevice(e->device));
    memcpy(e->h_tokens, tokens, 4 * n_tokens);
    HIP_TRY(hipMemcpyAsync(e->d_prompt, e->h_tokens, 4 * n_tokens, hipMemcpyHostToDevice, e->stream));
    int rc = e->set_state((size_t)tokens[0], first_pos);
    if (rc) return rc;
    // set_state queued {token, pos, step 0, prompt_len 0}; patch prompt_len before anything runs
    e->h_state->prompt_len = (int)n_tokens;
    HIP_TRY(hipMemcpyAsync(e->d_state, e->h_state, sizeof(State), hipMemcpyHostToDevice, e->stream));
    for (size_t k = 0; k < n_tokens; ++k)
        if ((rc = e->enqueue_forward(first_pos + k))) return rc;
    HIP_TRY(hipMemcpyAsync(e->h_tokens, e->d_out_tokens + (n_tokens - 1), 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (next_token) *next_token = e->h_tokens[0];
    return Q3_OK;
}

int q3_sampler_set(q3_engine* e, float temperature, float topp, uint64_t rng_seed) {
    g_err[0] = 0;
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    if (int rc = sampler_check(temperature, topp)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    int rc;
    if (!e->draw && (rc = e->draw.alloc(e->cfg.vocab_size, 1, true))) return rc;
    SamplerState h{};
    h.rng = rng_seed; h.temperature = temperature; h.topp = topp;
    HIP_TRY(hipMemcpy(e->draw.ss, &h, sizeof(h), hipMemcpyHostToDevice));
    draw_args(e->draw, DrawForm::Engine, e->d_logits, e->d_state, e->d_out_tokens, e->out_cap,
              e->d_stamps ? e->d_stamps + 16 * (size_t)(5 * e->cfg.n_layers + 3) : nullptr);
    if ((rc = e->build_sample_plans())) return rc;
    e->sampling = temperature != 0.0f;                       // sampler.rs:119-120: temperature 0 is the argmax path
    return Q3_OK;
}

int q3_sampler_top_k(q3_engine* e, int top_k) {
    g_err[0] = 0;
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    if (top_k < 0 || top_k > kTopkMax || top_k > e->cfg.vocab_size)
        return fail(Q3_ERR_ARG, "top_k %d out of range (0..%d, at most vocab_size %d)", top_k, kTopkMax, e->cfg.vocab_size);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (top_k > 0 && !e->d_top_k) {
        // one group, committed whole (DrawSite::alloc)
        DevMem<int> k; DevMem<unsigned long long> keys;
        int rc;
        if ((rc = k.alloc(1)) || (rc = keys.alloc((size_t)kSpecMax * kTopkColKeys))) return rc;
        e->d_top_k = std::move(k); e->d_topk_keys = std::move(keys);
        if ((rc = e->build_sample_plans())) return rc;
    }
    // 0 is never read: the plans without top-k run.  Two non-zero values share every plan and graph
    if (top_k > 0) HIP_TRY(hipMemcpy(e->d_top_k, &top_k, sizeof(int), hipMemcpyHostToDevice));
    e->top_k = top_k;
    return Q3_OK;
}

int q3_sampler_get_top_k(const q3_engine* e, int* top_k) {
    g_err[0] = 0;
    if (!e || !top_k) return fail(Q3_ERR_ARG, "null argument");
    *top_k = e->top_k;
    return Q3_OK;
}

int q3_sampler_get_rng(q3_engine* e, uint64_t* rng_state) {
    g_err[0] = 0;
    if (!e || !rng_state || !e->draw) return fail(Q3_ERR_ARG, "q3_sampler_set has not been called");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    SamplerState h;
    HIP_TRY(hipMemcpy(&h, e->draw.ss, sizeof(h), hipMemcpyDeviceToHost));
    *rng_state = h.rng;
    return Q3_OK;
}

int q3_forward_sample(q3_engine* e, size_t token, size_t pos, int32_t* next_token) { return q3_forward_argmax(e, token, pos, next_token); }

int q3_generate_sampled(q3_engine* e, size_t first_token, size_t first_pos, size_t n_tokens, int32_t* out_tokens) {
    return q3_generate_greedy(e, first_token, first_pos, n_tokens, out_tokens);
}

int q3_reset_kv(q3_engine* e) {
    if (!e) return fail(Q3_ERR_ARG, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    const size_t bytes = 4 * (size_t)e->cfg.n_layers * e->cfg.seq_len * e->cfg.n_kv_heads * e->cfg.head_dim;
    HIP_TRY(hipMemsetAsync(e->d_key, 0, bytes, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_value, 0, bytes, e->stream));
    if (e->d_value_t) HIP_TRY(hipMemsetAsync(e->d_value_t, 0, bytes, e->stream));
    // the classifier's {argmax cell, ticket} pair is self-clearing per token; a reset also recovers it after a launch that
    // did not run to completion
    HIP_TRY(hipMemsetAsync(e->d_next_cell, 0, 16, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return Q3_OK;
}

int q3_read_state(q3_engine* e, int kind, size_t offset, size_t count, float* out) {
    if (!e || !out) return fail(Q3_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    const size_t kv = (size_t)e->cfg.n_layers * e->cfg.seq_len * e->cfg.n_kv_heads * e->cfg.head_dim;
    const float* src = nullptr;
    size_t lim = 0;
    if (kind == 0) { src = e->d_key; lim = kv; }
    else if (kind == 1) { src = e->d_value; lim = kv; }
    else if (kind == 2) { src = e->d_tap; lim = (size_t)e->cfg.dim; }
    else return fail(Q3_ERR_ARG, "unknown state kind %d", kind);
    if (offset + count > lim) return fail(Q3_ERR_ARG, "state range out of bounds");
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out, src + offset, 4 * count, hipMemcpyDeviceToHost));
    return Q3_OK;
}

const char* q3_profile_name(int family) { return (family >= 0 && family < F_COUNT) ? kFamilyNames[family] : nullptr; }

int q3_profile(q3_engine* e, size_t token, size_t pos, int reps, float* ms, int32_t* launches, int cap) {
    g_err[0] = 0;
    if (!e || !ms || !launches || cap < F_COUNT || reps <= 0) return fail(Q3_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(e->device));
    for (int i = 0; i < cap; ++i) { ms[i] = 0.f; launches[i] = 0; }
    const std::vector<Launch>& P = ((int64_t)pos >= (int64_t)e->split_pos) ? e->plan_long : e->plan;
    const size_t nl = P.size();
    // events are released on every return path (RAII); the replayed launches overwrite x, the logits and KV row `pos`
    // exactly as a forward(token, pos) would -- callers treat q3_profile as a forward that returns timings
    struct Events {
        std::vector<hipEvent_t> ev;
        ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
    } evs;
    evs.ev.assign(2 * F_COUNT, nullptr);
    std::vector<hipEvent_t>& ev = evs.ev;
    for (auto& x : ev) HIP_TRY(hipEventCreate(&x));
    for (int r = 0; r < reps; ++r) {
        int rc = e->set_state(token, pos);
        if (rc) return rc;
        // one full forward first so every family runs on live data, then each family's launches back to back
        // between ONE pair of events: the average is the launch period (kernel + boundary), the same quantity
        // rocprofv3's per-dispatch durations sum to on a serialised stream.
        auto replay = [&](const Launch& L) { launch(L.fam == F_LMHEAD ? e->lm_plain : L, e->stream); };
        for (size_t i = 0; i < nl; ++i) replay(P[i]);
        for (int f = 0; f < F_COUNT; ++f) {
            HIP_TRY(hipEventRecord(ev[2 * f], e->stream));
            for (size_t i = 0; i < nl; ++i)
                if (P[i].fam == f) { replay(P[i]); launches[f] += 1; }
            HIP_TRY(hipEventRecord(ev[2 * f + 1], e->stream));
        }
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (int f = 0; f < F_COUNT; ++f) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, ev[2 * f], ev[2 * f + 1]));
            ms[f] += t;
        }
    }
    return F_COUNT;
}

// The reference's decode loop as its host runs it (generation.rs:31-46,153-162 with temperature 0), in compiled host
// code on top of q3_forward: forward -> `logits.to_vec()` (a 4*vocab byte copy) -> Sampler::sample_argmax on the host
// (last maximum under total_cmp, sampler.rs:57-59) -> feed back.  *seconds follows TokenMetrics (generation.rs:198-233):
// the clock starts before the first forward and stops after the last sample.  This is what a Rust caller of the
// Transformers::Qwen3Hip shim observes; the logits cross PCIe every token.
}  // extern "C"

namespace {
// copy n floats and return the index of the LAST maximum under f32::total_cmp (key = bits ^ ((bits >> 31) & 0x7fffffff) as
// int32: negative floats order reversed).  AVX2 when the host has it (8 keys per step, streaming loads of the pinned
// buffer), scalar otherwise.
#if !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("avx2"))) size_t copy_argmax_last_avx2(const float* src, float* dst, size_t n) {
    // ONE pass: 8 lanes each keep (best key, index of its last occurrence); `key >= best` replaces, so a later equal key wins.
    // dst is 32-byte aligned (caller): non-temporal stores, the copy is not read again here.
    const __m256i m7f = _mm256_set1_epi32(0x7fffffff);
    __m256i best = _mm256_set1_epi32(INT32_MIN), bidx = _mm256_setzero_si256();
    __m256i cur = _mm256_setr_epi32(0, 1, 2, 3, 4, 5, 6, 7);
    const __m256i step = _mm256_set1_epi32(8);
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        const __m256i b = _mm256_loadu_si256((const __m256i*)(src + i));
        _mm256_stream_si256((__m256i*)(dst + i), b);
        const __m256i key = _mm256_xor_si256(b, _mm256_and_si256(_mm256_srai_epi32(b, 31), m7f));
        const __m256i lt = _mm256_cmpgt_epi32(best, key);             // best > key: keep
        best = _mm256_max_epi32(best, key);
        bidx = _mm256_blendv_epi8(cur, bidx, lt);
        cur = _mm256_add_epi32(cur, step);
    }
    _mm_sfence();
    alignas(32) int32_t kk[8], ii[8];
    _mm256_store_si256((__m256i*)kk, best);
    _mm256_store_si256((__m256i*)ii, bidx);
    int32_t best_key = INT32_MIN;
    size_t best_i = 0;
    for (int l = 0; l < 8; ++l)
        if (kk[l] > best_key || (kk[l] == best_key && (size_t)ii[l] > best_i)) { best_key = kk[l]; best_i = (size_t)ii[l]; }
    for (; i < n; ++i) {
        int32_t b;
        memcpy(&b, src + i, 4);
        dst[i] = src[i];
        const int32_t key = b ^ ((b >> 31) & 0x7fffffff);
        if (key >= best_key) { best_key = key; best_i = i; }
    }
    return best_i;
}
#endif
size_t host_copy_argmax_last(const float* src, float* dst, size_t n) {
#if !defined(__HIP_DEVICE_COMPILE__)
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) return copy_argmax_last_avx2(src, dst, n);
#endif
    const int32_t* sb = (const int32_t*)src;
    int32_t best_key = INT32_MIN;
    size_t best_i = 0;
    for (size_t i = 0; i < n; ++i) {
        const int32_t b = sb[i];
        dst[i] = src[i];
        const int32_t key = b ^ ((b >> 31) & 0x7fffffff);
        if (key >= best_key) { best_key = key; best_i = i; }
    }
    return best_i;
}
}  // namespace

extern "C" {

size_t q3_host_sample_argmax(const float* logits, size_t n, float* copy) {
    if (!logits || n == 0) return 0;
    if (copy && ((uintptr_t)copy & 31) == 0) return host_copy_argmax_last(logits, copy, n);
    // no (or an unaligned) destination: the same pass into a scratch block, then a plain copy
    std::vector<float> tmp(n + 16);
    float* al = (float*)(((uintptr_t)tmp.data() + 31) & ~(uintptr_t)31);
    const size_t r = host_copy_argmax_last(logits, al, n);
    if (copy) memcpy(copy, al, 4 * n);
    return r;
}

int q3_host_generate(q3_engine* e, size_t first_token, size_t first_pos, size_t n_tokens, int32_t* out_tokens, double* seconds) {
    g_err[0] = 0;
    if (!e || (!out_tokens && n_tokens)) return fail(Q3_ERR_ARG, "null argument");
    if (first_pos + n_tokens > (size_t)e->cfg.seq_len)
        return fail(Q3_ERR_ARG, "first_pos %zu + n_tokens %zu exceeds seq_len %d", first_pos, n_tokens, e->cfg.seq_len);
    const size_t V = (size_t)e->cfg.vocab_size;
    std::vector<float> copy_store(V + 16);
    float* const copy = (float*)(((uintptr_t)copy_store.data() + 31) & ~(uintptr_t)31);      // 32-byte aligned (non-temporal stores)
    static const bool dbg = getenv("Q3_DEBUG_TIMING") != nullptr;
    double t_fwd = 0.0, t_host = 0.0;
    struct timespec t0, t1, ta, tb, tc;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    size_t token = first_token;
    for (size_t k = 0; k < n_tokens; ++k) {
        if (dbg) clock_gettime(CLOCK_MONOTONIC, &ta);
        const float* lg = q3_forward(e, token, first_pos + k);
        if (!lg) return Q3_ERR_HIP;
        if (dbg) clock_gettime(CLOCK_MONOTONIC, &tb);
        // generation.rs:160 `logits.to_vec()` and Sampler::sample_argmax in ONE pass over the pinned buffer: copy + the maximum
        // total_cmp key (sampler.rs:57-59: Iterator::max_by keeps the LAST maximum under the IEEE total order), then a scan
        // from the END of the copy for its first match
        const size_t best = host_copy_argmax_last(lg, copy, V);
        out_tokens[k] = (int32_t)best;
        token = best;
        if (dbg) {
            clock_gettime(CLOCK_MONOTONIC, &tc);
            t_fwd += (tb.tv_sec - ta.tv_sec) * 1e6 + (tb.tv_nsec - ta.tv_nsec) * 1e-3;
            t_host += (tc.tv_sec - tb.tv_sec) * 1e6 + (tc.tv_nsec - tb.tv_nsec) * 1e-3;
        }
    }
    if (dbg && n_tokens) fprintf(stderr, "[q3] host_generate: q3_forward %.1f us/token, copy + argmax %.1f us/token\n", t_fwd / n_tokens, t_host / n_tokens);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    if (seconds) *seconds = (t1.tv_sec - t0.tv_sec) + (t1.tv_nsec - t0.tv_nsec) * 1e-9;
    return Q3_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// operator-level entry points
// ------------------------------------------------------------------------------------------------
namespace {
// a buffer of an operator entry point, in bytes (a zero-byte request still gets 16)
struct OpBuf : DevMem<unsigned char> {
    int alloc(size_t bytes) { return DevMem<unsigned char>::alloc(bytes ? bytes : 16); }
    int upload(const void* src, size_t bytes) {
        int rc = alloc(bytes);
        if (rc) return rc;
        if (bytes) HIP_TRY(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
        return Q3_OK;
    }
    template <class T> T* as() { return (T*)p; }
};
int op_begin(int device) {
    g_err[0] = 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(Q3_ERR_HIP, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(Q3_ERR_ARG, "device %d out of range", device);
    HIP_TRY(hipSetDevice(device));
    return Q3_OK;
}
int op_end() {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return Q3_OK;
}
bool group_ok(size_t G) { return G >= 16 && G <= 1024 && (G & (G - 1)) == 0; }

// what q3_op_sample and q3_op_sample_top_k check alike, in front of the top-k entry point's own checks
int op_draw_check(const float* logits, size_t n, float temperature, float topp, const uint64_t* rng_state, const int32_t* index, int device) {
    int rc = op_begin(device);
    if (rc) return rc;
    if (!logits || !rng_state || !index || n == 0) return fail(Q3_ERR_ARG, "null argument");
    if (!(temperature > 0.0f)) return fail(Q3_ERR_ARG, "temperature must be positive (0 is q3_op_argmax)");
    return sampler_check(temperature, topp);
}
// The body of q3_op_sample (top_k == 0) and of q3_op_sample_top_k (1 <= top_k <= kTopkMax, the caller's check): one draw of a
// temporary one-column site over the caller's logits.  The top-k launches read none of the site's scratch, so only its state is made.
int op_draw(const float* logits, size_t n, float temperature, float topp, int top_k, uint64_t* rng_state, int32_t* index) {
    int rc;
    DrawSite site;
    OpBuf dl, dk, dkeys, dst, dout;
    SamplerState h{*rng_state, temperature, topp, {0, 0, 0, 0}};
    State st{};
    st.step = 1;                                            // "one forward done": the draw is stored in out_tokens[0]
    site.n = (int)n;
    if ((rc = dl.upload(logits, 4 * n)) || (rc = top_k ? site.ss.alloc(1) : site.alloc((int)n, 1, false)) ||
        (top_k && ((rc = dk.upload(&top_k, sizeof(int))) || (rc = dkeys.alloc(8 * (size_t)kTopkColKeys)))) ||
        (rc = dst.upload(&st, sizeof(st))) || (rc = dout.alloc(16)))
        return rc;
    HIP_TRY(hipMemcpy(site.ss, &h, sizeof(h), hipMemcpyHostToDevice));
    draw_args(site, DrawForm::Operator, dl.as<float>(), dst.as<State>(), dout.as<int32_t>(), 4);
    const TopkArgs t = topk_args(site.args, dk.as<int>(), dkeys.as<unsigned long long>());
    rc = draw_launches(site, 1, 0, top_k ? &t : nullptr, [](auto kernel, dim3 grid, dim3 block, size_t smem, const auto& a) {
        return launch_now(0, kernel, grid, block, smem, a);
    });
    if (rc || (rc = op_end())) return rc;
    HIP_TRY(hipMemcpy(&h, site.ss, sizeof(h), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(index, dout.p, 4, hipMemcpyDeviceToHost));
    *rng_state = h.rng;
    return Q3_OK;
}
}  // namespace

extern "C" {

int q3_op_quantize(int8_t* q, float* s, const float* x, size_t size, size_t group_size, int device) {
    int rc = op_begin(device);
    if (rc) return rc;
    if (!group_ok(group_size) || size % group_size) return fail(Q3_ERR_UNSUPPORTED, "unsupported size/group_size");
    OpBuf dx, dq, ds;
    if ((rc = dx.upload(x, 4 * size)) || (rc = dq.alloc(size)) || (rc = ds.alloc(4 * (size / group_size)))) return rc;
    hipLaunchKernelGGL(k_op_quantize, dim3(1), dim3(kWG), 0, 0, dq.as<int8_t>(), ds.as<float>(), dx.as<float>(), (int)size, (int)group_size);
    if ((rc = op_end())) return rc;
    HIP_TRY(hipMemcpy(q, dq.p, size, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(s, ds.p, 4 * (size / group_size), hipMemcpyDeviceToHost));
    return Q3_OK;
}

int q3_op_dequantize(const int8_t* q, const float* s, float* x, size_t size, size_t group_size, int device) {
    int rc = op_begin(device);
    if (rc) return rc;
    if (group_size == 0 || size % group_size) return fail(Q3_ERR_ARG, "size must be a multiple of group_size");
    OpBuf dx, dq, ds;
    if ((rc = dq.upload(q, size)) || (rc = ds.upload(s, 4 * (size / group_size))) || (rc = dx.alloc(4 * size))) return rc;
    hipLaunchKernelGGL(k_op_dequantize, dim3(256), dim3(256), 0, 0, dq.as<int8_t>(), ds.as<float>(), dx.as<float>(), size, (int)group_size);
    if ((rc = op_end())) return rc;
    HIP_TRY(hipMemcpy(x, dx.p, 4 * size, hipMemcpyDeviceToHost));
    return Q3_OK;
}

int q3_op_matmul(float* xout, const int8_t* xq, const float* xs, const int8_t* wq, const float* ws, size_t n, size_t d,
                 size_t group_size, int device) {
    int rc = op_begin(device);
    if (rc) return rc;
    if (!group_ok(group_size) || n % group_size || n % 16 || n == 0 || d == 0 || n > 65536)
        return fail(Q3_ERR_UNSUPPORTED, "unsupported n/group_size");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    OpBuf dxq, dxs, dwq, dws, dout;
    if ((rc = dxq.upload(xq, n)) || (rc = dxs.upload(xs, 4 * (n / group_size))) || (rc = dwq.upload(wq, n * d)) ||
        (rc = dws.upload(ws, 4 * (n * d / group_size))) || (rc = dout.alloc(4 * d)))
        return rc;
    GemvArgs a{};
    a.n = (int)n;
    a.group = (int)group_size;
    a.seg[0] = Seg{dwq.as<int8_t>(), dws.as<float>(), dout.as<float>(), (int)d, 0};
    a.total_rows = (int)d;
    a.pre_q = dxq.as<int8_t>();
    a.pre_s = dxs.as<float>();
    const GemvShape gs = plan_gemv((int)d, (int)n, (int)group_size, false, 1, prop.multiProcessorCount, 4);
    a.vr = gs.RU;
    const unsigned grid = gs.grid;
    const size_t smem = gemv_smem_bytes((int)n, (int)group_size, a.vr, false);
    GemvFn fn = pick<PRO_PREQ, EPI_STORE>((int)group_size, gs.RU, gs.JU, gs.FIN, gs.PF);
    if (!fn) return fail(Q3_ERR_UNSUPPORTED, "no kernel for tile %dx%d", gs.RU, gs.JU);
    if ((rc = launch_now(0, fn, dim3(grid), dim3(kWG), smem, a)) || (rc = op_end())) return rc;
    HIP_TRY(hipMemcpy(xout, dout.p, 4 * d, hipMemcpyDeviceToHost));
    return Q3_OK;
}

int q3_op_gemv_role(int role, float* out, float* tap_out, int32_t* argmax_index, int32_t* launch_info, const float* in,
                    const float* norm_w, const int8_t* pre_q, const float* pre_s, const int8_t* wq, const float* ws, size_t n,
                    size_t rows, size_t rows_kv, size_t head_dim, size_t group_size, uint32_t flags, int device) {
    int rc = op_begin(device);
    if (rc) return rc;
    int pro, epi;
    switch (role) {
        case Q3_ROLE_NORM_QKV: pro = PRO_NORM; epi = EPI_QKV; break;
        case Q3_ROLE_NORM_SWIGLU: pro = PRO_NORM; epi = EPI_SWIGLU; break;
        case Q3_ROLE_QUANT_RESID: pro = PRO_QUANT; epi = EPI_RESID; break;
        case Q3_ROLE_PREQR_RESID: pro = PRO_PREQR; epi = EPI_RESID; break;
        case Q3_ROLE_NORM_LOGITS: pro = PRO_NORM; epi = EPI_LOGITS; break;
        default: return fail(Q3_ERR_ARG, "unknown GEMV role %d", role);
    }
    const bool norm = pro == PRO_NORM, qkv = epi == EPI_QKV;
    if (!out || !wq || !ws || (pro == PRO_PREQR ? (!pre_q || !pre_s) : !in) || (norm && !norm_w) ||
        (epi == EPI_LOGITS && !argmax_index))
        return fail(Q3_ERR_ARG, "null pointer");
    if (flags & ~Q3_FLAG_FAST) return fail(Q3_ERR_ARG, "unknown flag bits 0x%x (0 or Q3_FLAG_FAST expected)", (unsigned)flags);
    // the limits of check_supported() for the vector this role contracts over
    if (!group_ok(group_size) || n == 0 || n % group_size || n % 16 || n > (norm ? 16384u : 65536u) || rows == 0 ||
        rows > (1u << 22))
        return fail(Q3_ERR_UNSUPPORTED, "unsupported n/group_size/rows");
    if (qkv && (rows_kv == 0 || rows_kv > (1u << 22) || head_dim % 8 || head_dim > 256 || (head_dim & (head_dim - 1)) ||
                rows % head_dim || rows_kv % head_dim))
        return fail(Q3_ERR_UNSUPPORTED, "unsupported q/k/v segment shape");
    // (build_plan additionally gates the tree fold on the developer knob Q3_FAST_FOLD, 1 in every build's default; the operator
    // follows the flag alone, i.e. the product's selection)
    const bool fast = (flags & Q3_FLAG_FAST) != 0;
    const int G = (int)group_size;
    if (pro == PRO_PREQR && !find_cfg(pro, epi, (int)n, G, fast))     // the planner falls back to PRO_QUANT: no generic kernel reads xq into registers
        return fail(Q3_ERR_UNSUPPORTED, "PRO_PREQR has no kernel for n = %zu, group %d", n, G);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    const size_t wrows = qkv ? rows + 2 * rows_kv : (epi == EPI_SWIGLU ? 2 * rows : rows);   // weight rows
    const size_t orows = qkv ? rows + 2 * rows_kv : rows;                                    // output floats
    OpBuf din, dnw, dpq, dps, dwq, dws, dout, dtap, dst, dcell, dslots, dtok;
    if ((rc = dwq.upload(wq, wrows * n)) || (rc = dws.upload(ws, 4 * (wrows * n / group_size)))) return rc;
    if (pro == PRO_PREQR) {
        if ((rc = dpq.upload(pre_q, n)) || (rc = dps.upload(pre_s, 4 * (n / group_size)))) return rc;
    } else if ((rc = din.upload(in, 4 * n))) return rc;
    if (norm && ((rc = dnw.upload(norm_w, 4 * n)) || (rc = dtap.alloc(4 * n)))) return rc;
    if (epi == EPI_RESID) rc = dout.upload(out, 4 * orows);      // x += W xq
    else rc = dout.alloc(4 * orows);
    if (rc) return rc;
    State st0{};                                                 // token 0, position 0, no prompt
    if ((rc = dst.upload(&st0, sizeof(State)))) return rc;

    GemvLaunch Ln;
    GemvArgs a{};
    a.n = (int)n;
    a.group = G;
    a.strict = fast ? 0 : 1;
    a.st = dst.as<State>();
    a.seq_len = 1;
    a.in = din.as<float>();
    a.norm_w = dnw.as<float>();
    a.pre_q = dpq.as<int8_t>();
    a.pre_s = dps.as<float>();
    if (norm && tap_out) a.tap_out = dtap.as<float>();
    const size_t ng = n / group_size;
    int units = (int)rows;
    if (qkv) {
        const int8_t* w0 = dwq.as<int8_t>();
        const float* s0 = dws.as<float>();
        float* o0 = dout.as<float>();
        a.seg[0] = Seg{w0, s0, o0, (int)rows, 0};
        a.seg[1] = Seg{w0 + rows * n, s0 + rows * ng, o0 + rows, (int)rows_kv, 0};
        a.seg[2] = Seg{w0 + (rows + rows_kv) * n, s0 + (rows + rows_kv) * ng, o0 + rows + rows_kv, (int)rows_kv, (int)rows_kv};
        a.total_rows = units = (int)orows;
        for (int k = 0; k < 2; ++k) {
            a.qkv_dw[k] = (const char*)a.seg[k + 1].wq - (const char*)a.seg[k].wq;
            a.qkv_ds[k] = (const char*)a.seg[k + 1].ws - (const char*)a.seg[k].ws;
            a.qkv_do[k] = (const char*)a.seg[k + 1].out - (const char*)a.seg[k].out;
        }
    } else if (epi == EPI_SWIGLU) {
        a.seg[0] = Seg{dwq.as<int8_t>(), dws.as<float>(), dout.as<float>(), (int)rows, 0};
        a.seg[1] = Seg{dwq.as<int8_t>() + rows * n, dws.as<float>() + rows * ng, nullptr, (int)rows, 0};
        a.total_rows = 2 * (int)rows;
    } else {
        a.seg[0] = Seg{dwq.as<int8_t>(), dws.as<float>(), dout.as<float>(), (int)rows, 0};
        a.total_rows = (int)rows;
    }
    if ((rc = plan_role(Ln, a, pro, epi, (int)n, units, G, fast, qkv ? (int)head_dim : 1, prop.multiProcessorCount))) return rc;
    if (epi == EPI_LOGITS) {    // the engine's form: the argmax bookkeeping of k_next folded into the classifier launch
        if ((rc = dslots.alloc(8 * (size_t)Ln.grid)) || (rc = dcell.alloc(16)) || (rc = dtok.alloc(4))) return rc;
        HIP_TRY(hipMemset(dcell.p, 0, 16));
        a.argmax_slots = dslots.as<unsigned long long>();
        a.next_cell = dcell.as<unsigned long long>();
        a.out_tokens = dtok.as<int32_t>();
        a.out_cap = 1;
    }
    if ((rc = launch_now(0, Ln.fn, dim3(Ln.grid), dim3(Ln.block), Ln.smem, a)) || (rc = op_end())) return rc;
    HIP_TRY(hipMemcpy(out, dout.p, 4 * orows, hipMemcpyDeviceToHost));
    if (a.tap_out) HIP_TRY(hipMemcpy(tap_out, dtap.p, 4 * n, hipMemcpyDeviceToHost));
    if (epi == EPI_LOGITS) {
        HIP_TRY(hipMemcpy(&st0, dst.p, sizeof(State), hipMemcpyDeviceToHost));
        *argmax_index = (int32_t)(unsigned)(st0.argmax & 0xffffffffull);
    }
    if (launch_info) {
        const GemvCfg* c = find_cfg(pro, epi, (int)n, G, fast);
        launch_info[0] = (c != nullptr && Ln.fn == c->fn) ? 1 : 0;
        launch_info[1] = (int32_t)Ln.grid;
        launch_info[2] = (int32_t)Ln.block;
        launch_info[3] = a.vr;
    }
    return Q3_OK;
}

int q3_op_rmsnorm(float* out, const float* in, const float* weight, size_t n, uint32_t flags, int device) {
    int rc = op_begin(device);
    if (rc) return rc;
    if (n == 0 || n > 32768) return fail(Q3_ERR_UNSUPPORTED, "unsupported n");
    OpBuf di, dw, dout;
    if ((rc = di.upload(in, 4 * n)) || (rc = dw.upload(weight, 4 * n)) || (rc = dout.alloc(4 * n))) return rc;
    const size_t smem = 4 * (size_t)term_floats((int)n) + 512;
    if ((rc = launch_now(0, k_op_rmsnorm, dim3(1), dim3(kWG), smem, dout.as<float>(), di.as<float>(), dw.as<float>(), (int)n,
                         (flags & Q3_FLAG_FAST) ? 0 : 1)) || (rc = op_end())) return rc;
    HIP_TRY(hipMemcpy(out, dout.p, 4 * n, hipMemcpyDeviceToHost));
    return Q3_OK;
}

int q3_op_softmax(float* x, size_t n, uint32_t flags, int device) {
    int rc = op_begin(device);
    if (rc) return rc;
    if (n == 0) return Q3_OK;
    OpBuf dx;
    if ((rc = dx.upload(x, 4 * n))) return rc;
    hipLaunchKernelGGL(k_op_softmax, dim3(1), dim3(kWG), 0, 0, dx.as<float>(), (int)n, (flags & Q3_FLAG_FAST) ? 0 : 1);
    if ((rc = op_end())) return rc;
    HIP_TRY(hipMemcpy(x, dx.p, 4 * n, hipMemcpyDeviceToHost));
    return Q3_OK;
}

int q3_op_swiglu(float* hb, const float* hb2, size_t n, int device) {
    int rc = op_begin(device);
    if (rc) return rc;
    OpBuf a, b;
    if ((rc = a.upload(hb, 4 * n)) || (rc = b.upload(hb2, 4 * n))) return rc;
    hipLaunchKernelGGL(k_op_swiglu, dim3(256), dim3(256), 0, 0, a.as<float>(), b.as<float>(), n);
    if ((rc = op_end())) return rc;
    HIP_TRY(hipMemcpy(hb, a.p, 4 * n, hipMemcpyDeviceToHost));
    return Q3_OK;
}

int q3_op_expf(float* x, size_t n, int device) {
    int rc = op_begin(device);
    if (rc) return rc;
    OpBuf a;
    if ((rc = a.upload(x, 4 * n))) return rc;
    hipLaunchKernelGGL(k_op_expf, dim3(512), dim3(256), 0, 0, a.as<float>(), n);
    if ((rc = op_end())) return rc;
    HIP_TRY(hipMemcpy(x, a.p, 4 * n, hipMemcpyDeviceToHost));
    return Q3_OK;
}

int q3_op_attention(float* xb, float* q, float* key_cache_layer, const float* value_cache_layer, const float* q_norm_w,
                    const float* k_norm_w, size_t pos, size_t seq_len, size_t n_heads, size_t n_kv_heads, size_t head_dim,
                    uint32_t flags, int device) {
    int rc = op_begin(device);
    if (rc) return rc;
    if (pos >= seq_len || n_kv_heads == 0 || n_heads % n_kv_heads || head_dim % 8 || head_dim > 256 ||
        (head_dim & (head_dim - 1)))
        return fail(Q3_ERR_UNSUPPORTED, "unsupported attention shape");
    const size_t ahd = n_heads * head_dim, kvd = n_kv_heads * head_dim;
    OpBuf dq, dk, dv, dqw, dkw, dxb, drope, dkraw, datt;
    if ((rc = dq.upload(q, 4 * ahd)) || (rc = dk.upload(key_cache_layer, 4 * seq_len * kvd)) ||
        (rc = dv.upload(value_cache_layer, 4 * seq_len * kvd)) || (rc = dqw.upload(q_norm_w, 4 * head_dim)) ||
        (rc = dkw.upload(k_norm_w, 4 * head_dim)) || (rc = dxb.alloc(4 * ahd)) ||
        (rc = dkraw.upload(key_cache_layer + pos * kvd, 4 * kvd)))
        return rc;
    const size_t half = head_dim / 2;
    std::vector<float> tab(seq_len * head_dim);
    for (size_t p = 0; p < seq_len; ++p)
        for (size_t i = 0; i < half; ++i) {
            const float freq = powf(1e6f, -((float)i) / (float)half);
            const float angle = (float)p * freq;
            tab[p * head_dim + 2 * i] = cosf(angle);
            tab[p * head_dim + 2 * i + 1] = sinf(angle);
        }
    if ((rc = drope.upload(tab.data(), 4 * tab.size()))) return rc;
    const bool split = pos >= 256;                       // same rule as the engine's long-context plan
    const bool att_global = split || seq_len > 4096;
    const int att_stride = att_stride_for(seq_len);
    const int nsl = (int)head_dim / attn_slice_w((int)head_dim, (int)n_heads, 256);
    OpBuf dpriv, dqout, dcmax, dvt;
    if (att_global && (rc = datt.alloc(4 * n_heads * (size_t)att_stride))) return rc;
    if (split && ((rc = dpriv.alloc(4 * n_heads * nsl * (size_t)att_stride)) || (rc = dqout.alloc(4 * ahd)) ||
                  (rc = dcmax.alloc(4 * n_heads * (size_t)cmax_stride_for(seq_len)))))
        return rc;
    AttnArgs a{};
    a.q = dq.as<float>();
    a.key_cache = dk.as<float>();
    a.k_raw = dkraw.as<float>();
    a.value_cache = dv.as<float>();
    a.q_norm_w = dqw.as<float>();
    a.k_norm_w = dkw.as<float>();
    a.rope = drope.as<float>();
    a.xb = dxb.as<float>();
    a.att_global = att_global ? datt.as<float>() : nullptr;
    a.st = nullptr;
    a.pos_override = (int)pos;
    attn_set_heads(a, (int)n_heads, (int)n_kv_heads);
    a.hd = (int)head_dim;
    a.seq_len = (int)seq_len;
    a.strict = (flags & Q3_FLAG_FAST) ? 0 : 1;
    a.write_q = 1;
    a.stamps = nullptr;
    if (split && (seq_len % 4) == 0) {
        // the engine's long-context plan streams a transposed copy of the value rows: the operator builds it the same way
        if ((rc = dvt.alloc(4 * seq_len * kvd))) return rc;
        hipLaunchKernelGGL(k_value_transpose, dim3((unsigned)((kvd + 63) / 64), (unsigned)((seq_len + 63) / 64), 1u), dim3(kWG), 0, 0,
                           (const float*)dv.p, dvt.as<float>(), (int)seq_len, (int)kvd, 0, (int)seq_len);
        a.value_t = dvt.as<float>();
    }
    if (split) {
        a.q_out = dqout.as<float>();
        Launch A, B;
        if ((rc = make_split_attn(A, B, a, datt.as<float>(), dcmax.as<float>(), dpriv.as<float>(), 256))) return rc;
        launch(A, 0);
        launch(B, 0);
        if ((rc = op_end())) return rc;
        HIP_TRY(hipMemcpy(dq.p, dqout.p, 4 * ahd, hipMemcpyDeviceToDevice));
    } else if ((head_dim == 64 || head_dim == 128) && dev_knob("Q3_ATT_SHORT", 1)) {
        const AttnShape sh = attn_short_shape((int)head_dim, (int)n_heads, (int)seq_len);
        if ((rc = launch_now(0, sh.fn, sh.grid, sh.block, sh.smem, a))) return rc;
    } else {
        if ((rc = launch_now(0, k_attn, dim3((unsigned)n_heads), dim3(kWG), attn_smem_bytes((int)head_dim, att_global ? 0 : (int)seq_len), a))) return rc;
    }
    if ((rc = op_end())) return rc;
    HIP_TRY(hipMemcpy(xb, dxb.p, 4 * ahd, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(q, dq.p, 4 * ahd, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(key_cache_layer + pos * kvd, (float*)dk.p + pos * kvd, 4 * kvd, hipMemcpyDeviceToHost));
    return Q3_OK;
}

#ifdef Q3_DEV
/* developer micro-benchmark (not part of the drop-in surface; exported by the -DQ3_DEV build only): average device time of the stand-alone
 * W8A8 GEMV (PRO_PREQ/EPI_STORE) over `reps` launches on random weights resident in HBM.  ru/ju/wg_per_cu
 * <= 0 pick the planner's choice.  Distinct weight copies are cycled so nothing stays cache-resident. */
int q3_dev_bench_gemv(size_t n, size_t d, size_t group_size, int wg_per_cu, int ru, int ju, int reps, int device,
                      float* avg_us, int32_t* used /*[3]: RU, JU, grid*/) {
    int rc = op_begin(device);
    if (rc) return rc;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    const size_t wbytes = n * d, sbytes = 4 * (n * d / group_size);
    size_t copies = (512ull << 20) / (wbytes + sbytes) + 1;
    if (copies > 16) copies = 16;
    if (copies < 2) copies = 2;
    OpBuf dw, ds, dxq, dxs, dout;
    if ((rc = dw.alloc(wbytes * copies)) || (rc = ds.alloc(sbytes * copies)) || (rc = dxq.alloc(n)) ||
        (rc = dxs.alloc(4 * (n / group_size))) || (rc = dout.alloc(4 * d)))
        return rc;
    HIP_TRY(hipMemset(dw.p, 0x11, wbytes * copies));
    HIP_TRY(hipMemset(ds.p, 0, sbytes * copies));
    HIP_TRY(hipMemset(dxq.p, 1, n));
    HIP_TRY(hipMemset(dxs.p, 0, 4 * (n / group_size)));
    GemvShape gs = plan_gemv((int)d, (int)n, (int)group_size, false, 1, prop.multiProcessorCount, wg_per_cu > 0 ? wg_per_cu : 4);
    if (ru > 0) gs.RU = ru;
    if (ju > 0) gs.JU = ju;
    if (ru > 0 || ju > 0) {
        const long nb = ((long)d + gs.RU - 1) / gs.RU;
        long grid = (nb + kWaves - 1) / kWaves;
        const long cap = (long)prop.multiProcessorCount * (wg_per_cu > 0 ? wg_per_cu : 4);
        gs.grid = (unsigned)(grid > cap ? cap : grid);
    }
    if (ru > 0 || ju > 0) { gs.FIN = 0; gs.PF = 0; }
    GemvFn fn = pick<PRO_PREQ, EPI_STORE>((int)group_size, gs.RU, gs.JU, gs.FIN, gs.PF);
    if (!fn) return fail(Q3_ERR_UNSUPPORTED, "no kernel for tile %dx%d", gs.RU, gs.JU);
    const size_t smem = gemv_smem_bytes((int)n, (int)group_size, gs.RU, false);
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    std::vector<Launch> ls(copies);              // one record per weight copy
    for (size_t i = 0; i < copies; ++i) {
        GemvArgs a{};
        a.n = (int)n;
        a.group = (int)group_size;
        a.vr = gs.RU;
        a.seg[0] = Seg{dw.as<int8_t>() + i * wbytes, (const float*)((char*)ds.p + i * sbytes), dout.as<float>(), (int)d, 0};
        a.total_rows = (int)d;
        a.pre_q = dxq.as<int8_t>();
        a.pre_s = dxs.as<float>();
        if ((rc = make_launch(ls[i], F_NEXT, fn, dim3(gs.grid), dim3(kWG), smem, a))) return rc;
    }
    for (int i = 0; i < 3; ++i) launch(ls[(size_t)i % copies], 0);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipEventRecord(e0, 0));
    for (int i = 0; i < reps; ++i) launch(ls[(size_t)i % copies], 0);
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (avg_us) *avg_us = ms * 1e3f / reps;
    if (used) { used[0] = gs.RU; used[1] = gs.JU; used[2] = (int)gs.grid; }
    return op_end();
}

#endif  // Q3_DEV

int q3_op_sample(const float* logits, size_t n, float temperature, float topp, uint64_t* rng_state, int32_t* index, int device) {
    if (int rc = op_draw_check(logits, n, temperature, topp, rng_state, index, device)) return rc;
    return op_draw(logits, n, temperature, topp, 0, rng_state, index);
}

int q3_op_sample_top_k(const float* logits, size_t n, float temperature, float topp, int top_k, uint64_t* rng_state, int32_t* index, int device) {
    if (int rc = op_draw_check(logits, n, temperature, topp, rng_state, index, device)) return rc;
    if (n > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 logits");
    if (top_k < 1 || top_k > kTopkMax || (size_t)top_k > n)
        return fail(Q3_ERR_ARG, "top_k %d out of range (1..%d, at most n %zu)", top_k, kTopkMax, n);
    return op_draw(logits, n, temperature, topp, top_k, rng_state, index);
}

int q3_op_penalize(const float* logits, const uint32_t* counts, size_t n, float presence, float frequency, float* out, int32_t* argmax, int device) {
    g_err[0] = 0;
    int rc;
    if ((rc = penalties_check(presence, frequency))) return rc;
    if (!logits || !counts || !out || !argmax || n == 0) return fail(Q3_ERR_ARG, "null argument");
    if (n > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 logits");
    if ((rc = op_begin(device))) return rc;
    OpBuf dl, dc, dout, dkeys, dctl;
    const PenCtl h{presence, frequency};
    if ((rc = dl.upload(logits, 4 * n)) || (rc = dc.upload(counts, 4 * n)) || (rc = dout.alloc(4 * n)) || (rc = dkeys.alloc(8 * (size_t)kPenSlices)) ||
        (rc = dctl.upload(&h, sizeof(h))))
        return rc;
    // one row, emitting, the counts as given: k_pen_apply without a pass (PenArgs::cols null)
    PenArgs a{};
    a.logits = dl.as<float>();
    a.pen_logits = dout.as<float>();
    a.counts = dc.as<unsigned>();
    a.pen_slots = dkeys.as<unsigned long long>();
    a.ctl = dctl.as<PenCtl>();
    a.n = (int)n;
    a.max_streams = 1;
    if ((rc = launch_now(0, k_pen_apply, dim3(kPenSlices, 1), dim3(kPenThreads), 0, a)) || (rc = op_end())) return rc;
    unsigned long long keys[kPenSlices], best = 0ull;
    HIP_TRY(hipMemcpy(out, dout.p, 4 * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(keys, dkeys.p, sizeof keys, hipMemcpyDeviceToHost));
    for (int i = 0; i < kPenSlices; ++i) best = std::max(best, keys[i]);
    *argmax = (int32_t)(best & 0xffffffffull);
    return Q3_OK;
}

int q3_op_logit_bias(const float* logits, size_t n, const q3_bias_entry* entries, size_t n_entries, int mode, uint32_t g, const uint32_t* counts,
                     float presence, float frequency, float* out, int32_t* argmax, int device) {
    g_err[0] = 0;
    int rc;
    if (mode != kBiasAdd && mode != kBiasAllow) return fail(Q3_ERR_ARG, "mode %d is neither ADD (0) nor ALLOW (1)", mode);
    if ((rc = penalties_check(presence, frequency))) return rc;
    if (!logits || !out || !argmax || n == 0) return fail(Q3_ERR_ARG, "null argument");
    if (n > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 logits");
    BiasTable t;
    const uint8_t m = (uint8_t)mode;
    if ((rc = bias_check(entries, &n_entries, &m, 1, (long)n, t))) return rc;
    if ((rc = op_begin(device))) return rc;
    OpBuf dl, dc, dout, dkeys, dpen, dent, doff, dmode, dctl;
    const PenCtl hp{presence, frequency};
    if ((rc = dl.upload(logits, 4 * n)) || (rc = dout.alloc(4 * n)) || (rc = dkeys.alloc(8 * (size_t)kPenSlices)) || (rc = dpen.upload(&hp, sizeof(hp))) ||
        (rc = dent.upload(t.entries.data(), sizeof(BiasEntry) * t.entries.size())) || (rc = doff.upload(t.off.data(), 4 * t.off.size())) ||
        (rc = dmode.upload(t.modes.data(), 1)) || (counts && (rc = dc.upload(counts, 4 * n))))
        return rc;
    BiasCtl h{};
    h.entries = dent.as<BiasEntry>();
    h.list_off = doff.as<unsigned>();
    h.modes = dmode.as<unsigned char>();
    h.counts = counts ? dc.as<unsigned>() : nullptr;
    h.n_lists = 1;
    h.n_requests = 1;
    h.g_op = g;
    if ((rc = dctl.upload(&h, sizeof(h)))) return rc;
    // one row, emitting, request 0 at output g, the counts as given: k_bias_apply without a pass (PenArgs::cols null)
    PenArgs a{};
    a.logits = dl.as<float>();
    a.pen_logits = dout.as<float>();
    a.pen_slots = dkeys.as<unsigned long long>();
    a.ctl = dpen.as<PenCtl>();
    a.n = (int)n;
    a.max_streams = 1;
    if ((rc = launch_now(0, k_bias_apply, dim3(kPenSlices, 1), dim3(kPenThreads), 0, a, (const BiasCtl*)dctl.as<BiasCtl>())) || (rc = op_end())) return rc;
    unsigned long long keys[kPenSlices], best = 0ull;
    HIP_TRY(hipMemcpy(out, dout.p, 4 * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(keys, dkeys.p, sizeof keys, hipMemcpyDeviceToHost));
    for (int i = 0; i < kPenSlices; ++i) best = std::max(best, keys[i]);
    *argmax = (int32_t)(best & 0xffffffffull);
    return Q3_OK;
}

int q3_op_guide(const float* logits, size_t n, const int16_t* next_row, const q3_bias_entry* entries, size_t n_entries, int mode, uint32_t g,
                const uint32_t* counts, float presence, float frequency, float* out, int32_t* argmax, int device) {
    g_err[0] = 0;
    int rc;
    if (mode != kBiasAdd && mode != kBiasAllow) return fail(Q3_ERR_ARG, "mode %d is neither ADD (0) nor ALLOW (1)", mode);
    if ((rc = penalties_check(presence, frequency))) return rc;
    if (!logits || !next_row || !out || !argmax || n == 0) return fail(Q3_ERR_ARG, "null argument");
    if (n > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 logits");
    BiasTable t;
    const uint8_t m = (uint8_t)mode;
    if ((rc = bias_check(entries, &n_entries, &m, 1, (long)n, t))) return rc;
    if ((rc = op_begin(device))) return rc;
    OpBuf dl, dc, dout, dkeys, dpen, dent, doff, dmode, dctl, dnext, dstate, dgctl;
    const PenCtl hp{presence, frequency};
    const int zero = 0;
    if ((rc = dl.upload(logits, 4 * n)) || (rc = dout.alloc(4 * n)) || (rc = dkeys.alloc(8 * (size_t)kPenSlices)) || (rc = dpen.upload(&hp, sizeof(hp))) ||
        (rc = dent.upload(t.entries.data(), sizeof(BiasEntry) * t.entries.size())) || (rc = doff.upload(t.off.data(), 4 * t.off.size())) ||
        (rc = dmode.upload(t.modes.data(), 1)) || (counts && (rc = dc.upload(counts, 4 * n))) || (rc = dnext.upload(next_row, 2 * n)) ||
        (rc = dstate.upload(&zero, sizeof(zero))))
        return rc;
    BiasCtl h{};
    h.entries = dent.as<BiasEntry>();
    h.list_off = doff.as<unsigned>();
    h.modes = dmode.as<unsigned char>();
    h.counts = counts ? dc.as<unsigned>() : nullptr;
    h.n_lists = 1;
    h.n_requests = 1;
    h.g_op = g;
    // a guide of the one state given, which request 0 starts in and its slot is in: the row holds whatever g is
    GuideCtl hg{};
    hg.next = dnext.as<short>();
    hg.start = dstate.as<int>();
    hg.state = dstate.as<int>();
    hg.n_states = 1;
    hg.n_start = 1;
    if ((rc = dctl.upload(&h, sizeof(h))) || (rc = dgctl.upload(&hg, sizeof(hg)))) return rc;
    // one row, emitting, request 0 at output g, the counts as given: k_guide_apply without a pass (PenArgs::cols null)
    PenArgs a{};
    a.logits = dl.as<float>();
    a.pen_logits = dout.as<float>();
    a.pen_slots = dkeys.as<unsigned long long>();
    a.ctl = dpen.as<PenCtl>();
    a.n = (int)n;
    a.max_streams = 1;
    if ((rc = launch_now(0, k_guide_apply, dim3(kPenSlices, 1), dim3(kPenThreads), 0, a, (const BiasCtl*)dctl.as<BiasCtl>(), (const GuideCtl*)dgctl.as<GuideCtl>())) ||
        (rc = op_end()))
        return rc;
    unsigned long long keys[kPenSlices], best = 0ull;
    HIP_TRY(hipMemcpy(out, dout.p, 4 * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(keys, dkeys.p, sizeof keys, hipMemcpyDeviceToHost));
    for (int i = 0; i < kPenSlices; ++i) best = std::max(best, keys[i]);
    *argmax = (int32_t)(best & 0xffffffffull);
    return Q3_OK;
}

int q3_op_guide_sparse(const float* logits, size_t n, int32_t dflt, const q3_guide_edge* edges, size_t n_edges, const q3_bias_entry* entries,
                       size_t n_entries, int mode, uint32_t g, const uint32_t* counts, float presence, float frequency, float* out, int32_t* argmax,
                       int device) {
    g_err[0] = 0;
    int rc;
    if (mode != kBiasAdd && mode != kBiasAllow) return fail(Q3_ERR_ARG, "mode %d is neither ADD (0) nor ALLOW (1)", mode);
    if ((rc = penalties_check(presence, frequency))) return rc;
    if (!logits || !out || !argmax || n == 0) return fail(Q3_ERR_ARG, "null argument");
    if (n > (size_t)INT32_MAX) return fail(Q3_ERR_ARG, "more than 2^31 logits");
    if (!edges && n_edges) return fail(Q3_ERR_ARG, "null edges with %zu edges", n_edges);
    if (n_edges > n) return fail(Q3_ERR_ARG, "%zu edges over %zu logits", n_edges, n);
    if (dflt < -1 || dflt >= kGuideSpMaxStates) return fail(Q3_ERR_ARG, "dflt = %d: -1 (forbidden) or a state below %d", dflt, kGuideSpMaxStates);
    for (size_t k = 0; k < n_edges; ++k) {
        if (edges[k].token < 0 || (size_t)edges[k].token >= n) return fail(Q3_ERR_ARG, "edges[%zu].token = %d outside the %zu logits", k, edges[k].token, n);
        if (k && edges[k].token <= edges[k - 1].token) return fail(Q3_ERR_ARG, "edges[%zu].token = %d is not above its predecessor: tokens ascend strictly", k, edges[k].token);
        if (edges[k].next < -1 || edges[k].next >= kGuideSpMaxStates)
            return fail(Q3_ERR_ARG, "edges[%zu].next = %d: -1 (forbidden) or a state below %d", k, edges[k].next, kGuideSpMaxStates);
    }
    BiasTable t;
    const uint8_t m = (uint8_t)mode;
    if ((rc = bias_check(entries, &n_entries, &m, 1, (long)n, t))) return rc;
    if ((rc = op_begin(device))) return rc;
    OpBuf dl, dc, dout, dkeys, dpen, dent, doff, dmode, dctl, ddflt, droff, dedges, dstate, dgctl;
    const PenCtl hp{presence, frequency};
    const int zero = 0;
    const uint32_t roff[2] = {0u, (uint32_t)n_edges};
    const q3_guide_edge none{0, -1};
    if ((rc = dl.upload(logits, 4 * n)) || (rc = dout.alloc(4 * n)) || (rc = dkeys.alloc(8 * (size_t)kPenSlices)) || (rc = dpen.upload(&hp, sizeof(hp))) ||
        (rc = dent.upload(t.entries.data(), sizeof(BiasEntry) * t.entries.size())) || (rc = doff.upload(t.off.data(), 4 * t.off.size())) ||
        (rc = dmode.upload(t.modes.data(), 1)) || (counts && (rc = dc.upload(counts, 4 * n))) || (rc = ddflt.upload(&dflt, sizeof(dflt))) ||
        (rc = droff.upload(roff, sizeof(roff))) || (rc = dedges.upload(n_edges ? edges : &none, sizeof(GuideEdge) * std::max(n_edges, (size_t)1))) ||
        (rc = dstate.upload(&zero, sizeof(zero))))
        return rc;
    BiasCtl h{};
    h.entries = dent.as<BiasEntry>();
    h.list_off = doff.as<unsigned>();
    h.modes = dmode.as<unsigned char>();
    h.counts = counts ? dc.as<unsigned>() : nullptr;
    h.n_lists = 1;
    h.n_requests = 1;
    h.g_op = g;
    // a guide of the one state given, which request 0 starts in and its slot is in: the row holds whatever g is
    GuideSpCtl hg{};
    hg.dflt = ddflt.as<int>();
    hg.row_off = droff.as<unsigned>();
    hg.edges = dedges.as<GuideEdge>();
    hg.start = dstate.as<int>();
    hg.state = dstate.as<int>();
    hg.n_states = 1;
    hg.n_start = 1;
    hg.n_edges = (int)n_edges;
    if ((rc = dctl.upload(&h, sizeof(h))) || (rc = dgctl.upload(&hg, sizeof(hg)))) return rc;
    // one row, emitting, request 0 at output g, the counts as given: k_guide_sp_apply without a pass (PenArgs::cols null)
    PenArgs a{};
    a.logits = dl.as<float>();
    a.pen_logits = dout.as<float>();
    a.pen_slots = dkeys.as<unsigned long long>();
    a.ctl = dpen.as<PenCtl>();
    a.n = (int)n;
    a.max_streams = 1;
    if ((rc = launch_now(0, k_guide_sp_apply, dim3(kPenSlices, 1), dim3(kPenThreads), 0, a, (const BiasCtl*)dctl.as<BiasCtl>(),
                         (const GuideSpCtl*)dgctl.as<GuideSpCtl>())) ||
        (rc = op_end()))
        return rc;
    unsigned long long keys[kPenSlices], best = 0ull;
    HIP_TRY(hipMemcpy(out, dout.p, 4 * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(keys, dkeys.p, sizeof keys, hipMemcpyDeviceToHost));
    for (int i = 0; i < kPenSlices; ++i) best = std::max(best, keys[i]);
    *argmax = (int32_t)(best & 0xffffffffull);
    return Q3_OK;
}

int q3_op_argmax(const float* logits, size_t n, int32_t* index, int device) {
    int rc = op_begin(device);
    if (rc) return rc;
    if (!index) return fail(Q3_ERR_ARG, "null argument");
    if (n == 0) { *index = 0; return Q3_OK; }   // unwrap_or_default
    OpBuf dl, dc;
    unsigned long long zero = 0;
    if ((rc = dl.upload(logits, 4 * n)) || (rc = dc.upload(&zero, 8))) return rc;
    hipLaunchKernelGGL(k_op_argmax, dim3(256), dim3(kWG), 0, 0, dl.as<float>(), n, dc.as<unsigned long long>());
    if ((rc = op_end())) return rc;
    unsigned long long cell = 0;
    HIP_TRY(hipMemcpy(&cell, dc.p, 8, hipMemcpyDeviceToHost));
    *index = (int32_t)(cell & 0xffffffffull);
    return Q3_OK;
}

}  // extern "C"

#include "q3_batch_host.inc"
#include "q3_plan_host.inc"
#include "q3_dense_host.inc"
#include "q3_cols_host.inc"
#include "q3_stop_host.inc"
#include "q3_prefix_host.inc"
#include "q3_embed_host.inc"
#include "q3_choice_host.inc"
#include "q3_score_host.inc"
