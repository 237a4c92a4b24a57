/*
 * qwen3_hip.h -- C ABI of libqwen3_hip.so, the MI355X (gfx950) Qwen3 Q8 decode engine.
 *
 * Drop-in boundary: the reference has no FFI; its seam is the Rust trait
 *     pub trait Transformer { fn forward(&mut self, token: usize, pos: usize) -> &[f32];
 *                             fn get_config(&self) -> &ModelConfig; }
 * (qwen3-inference/src/models/mod.rs:13-18), built by TransformerBuilder::build (models/mod.rs:55-73).
 * A `Transformers::Qwen3Hip` variant inside qwen3-inference binds exactly the entry points of section 1
 * (INTEGRATION.md shows the ~80-line Rust shim).  Plain pointers and sizes only; no torch / HIP types.
 *
 * Threading: one caller at a time per engine (mirrors `&mut self`); engines are independent, one per
 * GPU, no communication (replicas only -- the path does not shard).
 * Errors: 0 on success, negative q3_status otherwise; q3_last_error() gives the calling thread's
 * message.  There is NO CPU fallback: without a usable HIP device q3_create fails.
 *
 * Environment: libqwen3_hip.so reads exactly these variables (tests/test_host_and_abi.py checks the binary):
 *     Q3_PREFILL_M=<16..4096>   positions per weight pass of q3_prefill_batched and of section 2g (default 2048; <= 32 selects
 *                               the batch-32 kernels).  The dense attention scratch grows with it: 4 * M * n_heads * context bytes.
 *     Q3_DEBUG_TIMING=1         host-side timing of q3_forward / q3_host_generate phases on stderr.
 *
 * Build options (qwen3-rs_amd/Makefile, `make abl EXTRA=-D... ABL=name` -> libq3_<name>.so; never part of libqwen3_hip.so):
 *     -DQ3_TICKET_ACQ_REL       the classifier's last-arriver ticket (csrc/q3_gemv.h, EPI_LOGITS) with acquire + release ordering
 *                               on its two device-scope read-modify-writes instead of relaxed.  The shipped library keeps
 *                               them relaxed: every workgroup's fetch_max on the argmax cell and its fetch_add on the ticket
 *                               are device-scope RMWs executed at the L2 / memory coherence point, and the ticket's operand
 *                               DATA-DEPENDS on the maximum's return value, so the add cannot issue before the max has
 *                               returned; the last arriver then reads the cell with another RMW.  That is an argument about
 *                               gfx950 (RMWs are performed at one point of coherence, in issue order per address
 *                               dependence), not about the HIP memory model, which would want release on the max and acquire
 *                               on the ticket.  Measured cost of the ordered form: +1.4 ... +4.8 us per token
 *                               (profiles/r05_ticket_order.txt: a release is a buffer_wbl2 in each of ~590 workgroups).
 *                               Build it when porting to another target or toolchain.
 * Every other Q3_* switch (a choice between kernel forms that the product runs for other shapes, workgroup overrides,
 * in-kernel timelines) exists only in the developer build, libqwen3_hip_dev.so (`make -C qwen3-rs_amd dev`, -DQ3_DEV);
 * results are identical in both builds.
 */
#ifndef QWEN3_HIP_H
#define QWEN3_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Q3_ABI_VERSION 1

typedef enum q3_status {
    Q3_OK = 0,
    Q3_ERR_IO = -1,        /* open / mmap failed                        (models/mod.rs:56-59) */
    Q3_ERR_FORMAT = -2,    /* bad magic / version / dims / truncated    (configuration.rs:116-146, utils.rs:21-56) */
    Q3_ERR_ARG = -3,       /* null pointer, token/pos out of range (the reference panics: layers.rs:73-75,335) */
    Q3_ERR_HIP = -4,       /* HIP runtime error / no device */
    Q3_ERR_UNSUPPORTED = -5, /* shape the kernels do not cover (e.g. group_size not a multiple of 16) */
    Q3_ERR_INTERNAL = -6   /* the library caught itself breaking one of its own invariants (section 2h: a scheduler that does not end) */
} q3_status;

/* ModelConfig, qwen3-inference/src/configuration.rs:18-30 (seq_len already clamped by ctx_len) */
typedef struct q3_config {
    int32_t architecture_id;
    int32_t dim;
    int32_t hidden_dim;
    int32_t n_layers;
    int32_t n_heads;
    int32_t n_kv_heads;
    int32_t head_dim;
    int32_t seq_len;
    int32_t vocab_size;
    int32_t group_size;
    int32_t shared_classifier; /* bool */
} q3_config;

typedef struct q3_engine q3_engine;

/* q3_create flags.
 * Default (flags = 0): every f32 sum is reduced in the reference's sequential order, so logits are
 * BIT-IDENTICAL to the CPU path and greedy token sequences are identical by construction. */
#define Q3_FLAG_FAST 1u /* opt-in: wavefront-tree reductions for the RMSNorm / attention sums and, for the listed shapes
                           (group 64), for the fold of a matmul row's group terms.  Not bit-exact: a 28-layer W8A8 stack
                           amplifies a 1e-7 reordering difference to its own int8 quantization-noise floor (logit deltas of
                           ~0.1), so greedy tokens can differ from the CPU path.  Of the int8
                           group-quant matmul, the integer group dots and each group term ((dot as f32) * ws) * xs
                           (tensor.rs:53-60) are exact in both modes; only the ORDER in which a row's group terms are
                           added differs (a tree instead of the ascending chain).  quantize, SwiGLU, expf and the
                           sampler are identical in both modes. */
#define Q3_FLAG_NO_GRAPH 2u /* launch kernels eagerly instead of replaying a captured hipGraph */
#define Q3_FLAG_NO_VALUE_T 4u /* do not keep the TRANSPOSED copy of the value cache.  Reference-order engines whose context
                           can reach the split attention path (seq_len > 256, a multiple of 4) keep the value cache twice:
                           row-major [L][seq_len][kv_dim] and transposed [L][kv_dim][seq_len], n_layers * kv_dim * seq_len * 4
                           bytes each (Qwen3-8B: 6.0 GB at 40,960 positions, 19.3 GB at 131,072; 0.6B: 4.7 GB at 40,960).
                           The copy lets the long-context output kernel stream 1 KB runs instead of 64-byte pieces
                           (config-3 decode 468 -> 503 tok/s when it went in).  With this flag the engine allocates the
                           row-major cache only and the long-context kernel reads it (same results bit for bit).
                           Q3_FLAG_FAST engines never allocate the copy (their output kernel does not read it). */

/* ------------------------------------------------------------------------------------------------
 * 1. The reference surface
 * ---------------------------------------------------------------------------------------------- */

/* TransformerBuilder::new(path).with_ctx_length(ctx).build()          models/mod.rs:45-73
 * ctx_len 0 = keep the checkpoint's seq_len.  device = HIP device ordinal. */
int q3_create(const char* checkpoint_path, uint32_t ctx_len, int device, uint32_t flags, q3_engine** out);

/* Transformer::get_config                                              models/mod.rs:17 */
int q3_get_config(const q3_engine* e, q3_config* out);

/* Transformer::forward(token, pos) -> &[f32; vocab_size]               models/qwen3.rs:62-79
 * Returns a host pointer to vocab_size logits, valid until the next call on this engine (same lifetime
 * as the reference's borrow from &mut self), or NULL on error (the Rust shim panics, as the reference
 * does on out-of-range indices). */
const float* q3_forward(q3_engine* e, size_t token, size_t pos);

/* Drop for the transformer */
void q3_destroy(q3_engine* e);

const char* q3_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * 2. Extensions outside the reference surface (same arithmetic, less egress)
 * ---------------------------------------------------------------------------------------------- */

/* forward + Sampler::sample_argmax (sampler.rs:57-59: last maximum under f32::total_cmp) on the device;
 * only the 4-byte token id crosses PCIe. */
int q3_forward_argmax(q3_engine* e, size_t token, size_t pos, int32_t* next_token);

/* The greedy inner loop of `generate` (generation.rs:31-46,153-162 with temperature 0) kept on the
 * device: step k runs forward(tok_k, first_pos + k) and tok_{k+1} = argmax.  tok_0 = first_token.
 * Writes tok_1..tok_n into out_tokens (n = n_tokens).  No termination check: callers cut at BOS/EOS
 * (generation.rs:35) afterwards.  Requires first_pos + n_tokens <= seq_len. */
int q3_generate_greedy(q3_engine* e, size_t first_token, size_t first_pos, size_t n_tokens, int32_t* out_tokens);

/* The reference's own decode loop on top of q3_forward, in compiled host code: forward -> `logits.to_vec()` ->
 * Sampler::sample_argmax on the HOST (generation.rs:31-46,153-162; sampler.rs:57-59) -> feed back.  The logits cross
 * PCIe every token, exactly what a Rust caller of the Transformers::Qwen3Hip shim observes.  *seconds (may be NULL) is
 * the TokenMetrics interval (generation.rs:198-233): from before the first forward to after the last sample.
 * Tokens are identical to q3_generate_greedy.  bench.py reports this as `forward_surface`. */
int q3_host_generate(q3_engine* e, size_t first_token, size_t first_pos, size_t n_tokens, int32_t* out_tokens, double* seconds);

/* The host half of generate_next_token as q3_host_generate runs it (no device involved): copy n logits to `copy`
 * (generation.rs:160 `logits.to_vec()`; may be NULL) and return Sampler::sample_argmax of them -- the index of the LAST maximum
 * under f32::total_cmp (sampler.rs:57-59, Iterator::max_by).  One vectorised pass (AVX2 when the host has it). */
size_t q3_host_sample_argmax(const float* logits, size_t n, float* copy);

/* The prompt loop of `chat` (handle_user_turn, generation.rs:116-123) kept on the device: every prompt token is
 * forwarded in order at first_pos, first_pos+1, ... (sequential prefill: identical K/V rows and logits to n calls
 * of q3_forward), the per-token sample is discarded, and the argmax after the LAST prompt token -- the first
 * generated token -- is returned.  Continue with q3_generate_greedy(e, *next_token, first_pos + n_tokens, ...). */
int q3_prefill(q3_engine* e, const int32_t* tokens, size_t n_tokens, size_t first_pos, int32_t* next_token);

/* Sampler::new(vocab_size, temperature, topp, rng_seed) + Sampler::sample on the device (sampler.rs:29-42,118-139):
 * temperature scaling, softmax, one xorshift64* coin per draw, multinomial (topp <= 0 or >= 1) or top-p.  After this
 * call with temperature > 0, every token the engine draws itself -- q3_forward_argmax / q3_forward_sample,
 * q3_generate_greedy / q3_generate_sampled, and the last position of q3_prefill / q3_prefill_batched -- comes from
 * Sampler::sample instead of the argmax, and a chat-mode prefill advances the rng by one coin per prompt position like
 * the reference's discarded samples (generation.rs:116-123).  temperature 0 restores the argmax path (no coin drawn).
 * All running sums are walked in the reference's order (bit-identical probabilities and tokens); candidates of EQUAL
 * probability in top-p are ordered by ascending token id (the reference's sort_unstable_by leaves that unspecified).
 * q3_forward() is unaffected: it returns logits and leaves sampling to the caller.  Batched decode has its own
 * per-stream samplers (q3_batch_sampler_set). */
int q3_sampler_set(q3_engine* e, float temperature, float topp, uint64_t rng_seed);
int q3_sampler_get_rng(q3_engine* e, uint64_t* rng_state);
int q3_forward_sample(q3_engine* e, size_t token, size_t pos, int32_t* next_token);
int q3_generate_sampled(q3_engine* e, size_t first_token, size_t first_pos, size_t n_tokens, int32_t* out_tokens);

/* Fresh-engine state: zero the KV cache (models/qwen3.rs:439-440) */
int q3_reset_kv(q3_engine* e);

/* Copy device state back for parity tests: kind 0 = key cache, 1 = value cache ([L][seq_len][kv_dim]),
 * 2 = x after the final RMSNorm ([dim]).  `count` floats starting at `offset`. */
int q3_read_state(q3_engine* e, int kind, size_t offset, size_t count, float* out);

/* Per-kernel timing of one forward(token,pos), launched eagerly with HIP events around every kernel
 * on the engine's stream.  Kernel family i is named by q3_profile_name(i); ms[i] / launches[i] are
 * accumulated over `reps` forwards.  Returns the number of families (<= cap). */
int q3_profile(q3_engine* e, size_t token, size_t pos, int reps, float* ms, int32_t* launches, int cap);
const char* q3_profile_name(int family);

/* Header parse + validation only (configuration.rs:77-146); does not touch the GPU. */
int q3_parse_header(const uint8_t* data, size_t len, q3_config* out);

uint32_t q3_abi_version(void);
/* First 16 hex digits of the SHA-256 over the library's sources (csrc/ + this header, in sorted file-name order), baked in by
 * the Makefile: lets a test harness detect a prebuilt libqwen3_hip.so that does not match the checked-out sources. */
const char* q3_build_id(void);

/* ------------------------------------------------------------------------------------------------
 * 2b. Batched decode: up to 32 independent streams (each its own KV cache, token and position) advance
 * one token per step while the weights are streamed ONCE per step through the int8 matrix cores.  This
 * serves N concurrent `generate` loops (generation.rs:9-48), which the reference can only run as N
 * processes.  Every stream's logits are bit-identical to the same (token, pos) sequence through
 * q3_forward on a fresh engine.  Stream i of a call always uses KV slot i.
 * ------------------------------------------------------------------------------------------------ */

/* Allocate the batched state: an MFMA-ordered copy of the weights, max_streams (1..32) zero-filled KV caches
 * of min(ctx_len, engine seq_len) rows (0 = engine seq_len) and scratch.  Needs group_size 64/128/256 and
 * every matrix height a multiple of 16 (Q3_ERR_UNSUPPORTED otherwise).  Calling it again re-allocates
 * (and clears) the state.
 * Group sizes 512 and 1024 are single-stream only: q3_forward, q3_prefill, the greedy / sampled loops and the operator entry
 * points take them (any power of two in [16, 1024]), while q3_batch_init -- and with it everything of sections 2b to 2i,
 * q3_prefill_batched and q3_verify included -- answers Q3_ERR_UNSUPPORTED ("batched decode needs group_size 64, 128 or 256 ...")
 * and leaves the engine usable.  At 128 and 256 every batched block holds at most 32 columns (no dense kernels). */
int q3_batch_init(q3_engine* e, int max_streams, uint32_t ctx_len);

/* One step: stream i runs forward(tokens[i], pos[i]).  logits_out ([n_streams][vocab_size], host) and
 * argmax_out ([n_streams], sample_argmax of each row, sampler.rs:57-59) may each be NULL. */
int q3_forward_batch(q3_engine* e, const int32_t* tokens, const int32_t* pos, int n_streams, float* logits_out,
                     int32_t* argmax_out);

/* n_steps greedy steps for every stream with no host round trip; out_tokens is [n_streams][n_steps]: row i
 * equals q3_generate_greedy(first_tokens[i], first_pos[i], n_steps) on a fresh engine. */
int q3_generate_greedy_batch(q3_engine* e, const int32_t* first_tokens, const int32_t* first_pos, int n_streams,
                             size_t n_steps, int32_t* out_tokens);

/* Per-stream Sampler::sample for the batched decode (one sampler per stream: same temperature / top-p, stream i seeded
 * with rng_seeds[i], [max_streams] values).  With temperature > 0 the tokens of q3_forward_batch (argmax_out) and
 * q3_generate_greedy_batch are drawn exactly as q3_sampler_set + q3_forward_sample would draw them for that stream alone;
 * temperature 0 restores the argmax. */
int q3_batch_sampler_set(q3_engine* e, float temperature, float topp, const uint64_t* rng_seeds);

/* Zero every stream's KV cache. */
int q3_batch_reset_kv(q3_engine* e);

/* q3_prefill with the prompt walked in blocks of up to 2,048 consecutive positions (env Q3_PREFILL_M; blocks of <= 32 use
 * the batch-32 kernels), each block ONE pass over the weights on the matrix cores; the positions read and write the engine's own KV cache (the one q3_forward uses).
 * Sequential-equivalent: cache rows and the returned first generated token are bit-identical to q3_prefill, i.e. to
 * the prompt loop of `chat` (generation.rs:116-123).  Same shape limits as q3_batch_init (Q3_ERR_UNSUPPORTED otherwise);
 * does not need q3_batch_init (allocates the MFMA-ordered weight copy on first use, no per-stream caches). */
int q3_prefill_batched(q3_engine* e, const int32_t* tokens, size_t n_tokens, size_t first_pos, int32_t* next_token);

/* Parity tap: kind 0 key cache / 1 value cache ([n_layers][ctx][kv_dim]) / 2 residual stream x of one stream. */
int q3_batch_read_state(q3_engine* e, int stream, int kind, size_t offset, size_t count, float* out);

/* ------------------------------------------------------------------------------------------------
 * 2c. Lossless draft verification and prompt-lookup speculative greedy decode: several tokens per pass over the
 * weights for ONE stream.  A block of up to 32 consecutive positions -- the current token and drafted continuations -- goes
 * through the short-block kernels of q3_prefill_batched over the engine's own KV cache and through the n-column
 * classifier of the batched decode; a draft is accepted exactly when it equals the argmax of the position in front of it,
 * so every returned token is the token q3_generate_greedy returns, bit-identical logits and cache rows included.
 * Refused with Q3_ERR_UNSUPPORTED: a Q3_FLAG_FAST engine (its block and single-stream kernels are not bit-equal to each
 * other), an engine whose sampler is set to a temperature > 0 (these two names are greedy only: section 2d holds for any
 * sampler setting), and the shapes q3_batch_init refuses.  The packed weight copy of q3_prefill_batched is allocated on first use and shared with it and
 * with q3_batch_init.  No environment variable: everything is an argument.
 * ------------------------------------------------------------------------------------------------ */
#define Q3_VERIFY_MAX 32

/* Forward tokens[0..n_tokens) at first_pos, first_pos + 1, ... in ONE weight pass.  tokens[0] is certain, tokens[1..) are drafts.
 *   next_tokens[i] = sample_argmax(forward(tokens[i], first_pos + i)) with tokens[0..i] as the sequence so far   (i < n_tokens)
 *   *n_accepted    = a = the number of leading drafts with tokens[j] == next_tokens[j - 1]   (j = 1, 2, ...)
 * next_tokens[0..a] are the a + 1 tokens q3_generate_greedy returns for (tokens[0], first_pos, a + 1), and on return the
 * engine is in the state that call leaves: cache rows first_pos .. first_pos + a written (the transposed value cache too),
 * rows first_pos + a + 1 .. first_pos + n_tokens - 1 RESTORED to their content before the call.
 * logits_out (may be NULL): [n_tokens][vocab_size]; row i is bit-identical to q3_forward on the same token prefix, rows
 * behind a rejected draft included (they are the logits of the sequence the caller proposed).
 * Q3_ERR_ARG: n_tokens 0 or > Q3_VERIFY_MAX, first_pos + n_tokens > seq_len, a token outside the vocabulary. */
int q3_verify(q3_engine* e, const int32_t* tokens, size_t n_tokens, size_t first_pos, int32_t* next_tokens, size_t* n_accepted,
              float* logits_out);

/* The prompt-lookup drafter alone (host only, never touches the GPU).  With S = seq[0..n) and g = ngram: take the LARGEST
 * i < n - g with S[i..i+g) == S[n-g..n); the draft is S[i+g .. min(i+g+draft_len, n)), copied to `draft` (room for draft_len
 * tokens).  Returns the number of tokens written; 0 (no draft) when there is no such i, when n <= g, or when draft_len < 1. */
size_t q3_lookup_draft(const int32_t* seq, size_t n, int ngram, int draft_len, int32_t* draft);

/* The incremental form of the same drafter, as q3_generate_lookup runs it (a hash of n-grams, O(1) amortised per token; host
 * only): seq[0..n_corpus) is entered first, then seq grows one token at a time.  For every length m = n_corpus .. n, the draft
 * over seq[0..m) goes to drafts[(m - n_corpus) * draft_len ..] and its length to lens[m - n_corpus] (n - n_corpus + 1 entries). */
int q3_lookup_trace(const int32_t* seq, size_t n, size_t n_corpus, int ngram, int draft_len, int32_t* drafts, int32_t* lens);

typedef struct q3_spec_stats {
    uint64_t verify_passes; /* block passes over the weights */
    uint64_t single_steps;  /* ordinary single-stream steps (no draft) */
    uint64_t drafted;       /* draft tokens put through a pass */
    uint64_t accepted;      /* ... of which accepted */
} q3_spec_stats;

/* q3_generate_greedy with prompt-lookup drafts: the same out_tokens and the same engine state, in fewer weight passes.
 * S = corpus ++ [first_token] ++ the tokens generated so far.  Each round drafts from S (the rule above, at most draft_len
 * tokens, cut so that the round yields no more tokens than are still wanted, and cut in front of a corpus token outside the
 * vocabulary); no draft -> one ordinary single-stream step through the decode graph; a draft of d tokens -> one pass of the
 * block [current token, d drafts] that yields accepted + 1 tokens.  A call uses one block width, draft_len + 1 columns:
 * shorter drafts are padded with repeats of their last column, no plan or graph is rebuilt between rounds.  `corpus` is
 * the text to look continuations up in -- in real use the prompt -- and need not be what the KV cache holds.  Only the
 * accepted count and the token ids cross PCIe.  stats may be NULL.
 * Q3_ERR_ARG: ngram < 1, draft_len outside 0 .. Q3_VERIFY_MAX - 1, first_pos + n_tokens > seq_len. */
int q3_generate_lookup(q3_engine* e, const int32_t* corpus, size_t n_corpus, size_t first_token, size_t first_pos, size_t n_tokens,
                       int ngram, int draft_len, int32_t* out_tokens, q3_spec_stats* stats);

/* ------------------------------------------------------------------------------------------------
 * 3. Operator-level entry points: the reference's public free functions (tensor.rs, layers.rs) run on
 *    the device over caller (host) buffers.  Used by the parity tests; same kernels/device functions
 *    as the fused forward.  `device` as in q3_create.  q3_op_rmsnorm, q3_op_softmax, q3_op_attention and
 *    q3_op_gemv_role take flags: 0 (reference order) or Q3_FLAG_FAST; the others (quantize, dequantize, matmul,
 *    swiglu, expf, sample, argmax) have one form, identical in both modes.
 * ---------------------------------------------------------------------------------------------- */

/* tensor::quantize(qx, x, size, group_size)                             tensor.rs:91-119 */
int q3_op_quantize(int8_t* q, float* s, const float* x, size_t size, size_t group_size, int device);
/* tensor::dequantize                                                    tensor.rs:72-80 */
int q3_op_dequantize(const int8_t* q, const float* s, float* x, size_t size, size_t group_size, int device);
/* tensor::matmul(xout, x, w, n, d, group_size)                          tensor.rs:23-62 */
int q3_op_matmul(float* xout, const int8_t* xq, const float* xs, const int8_t* wq, const float* ws, size_t n,
                 size_t d, size_t group_size, int device);
/* One fused GEMV launch of the decode plan, alone: the kernel, grid, workgroup width and LDS size the planner picks for this
 * (prologue, epilogue, n, rows, group_size, flags) -- the shape-specialised table entry when the shape is listed (group 64, n of
 * a listed model; flags selects the reference-order or the tolerance-mode table), the generic kernel otherwise.
 *   Q3_ROLE_NORM_QKV     xb = RMSNorm(in, norm_w); out = [Wq; Wk; Wv] quantize(xb)   wq: [rows + 2*rows_kv][n], out the same count
 *                        (rows = query rows, rows_kv = key rows = value rows, all multiples of head_dim)
 *   Q3_ROLE_NORM_SWIGLU  out[r] = silu(W1 xq)[r] * (W3 xq)[r]                        wq: W1 then W3, [2*rows][n]; out [rows]
 *   Q3_ROLE_QUANT_RESID  out += W quantize(in)                                        out [rows], read and written
 *   Q3_ROLE_PREQR_RESID  out += W (pre_q, pre_s)          listed n only (the planner's fallback is QUANT_RESID): else Q3_ERR_UNSUPPORTED
 *   Q3_ROLE_NORM_LOGITS  out = Wcls quantize(RMSNorm(in, norm_w)); *argmax_index = Sampler::sample_argmax(out) as the launch computes it
 * ws: [weight rows][n / group_size].  tap_out (NORM roles, may be NULL): the kernel's own copy of the normalised vector, [n] --
 * the operand it quantizes.  launch_info (may be NULL): {1 if a table entry was launched else 0, grid, threads per workgroup,
 * rows per wave batch}.  rows_kv / head_dim are read for Q3_ROLE_NORM_QKV only.  Unused inputs of a role may be NULL. */
#define Q3_ROLE_NORM_QKV 0
#define Q3_ROLE_NORM_SWIGLU 1
#define Q3_ROLE_QUANT_RESID 2
#define Q3_ROLE_PREQR_RESID 3
#define Q3_ROLE_NORM_LOGITS 4
int q3_op_gemv_role(int role, float* out, float* tap_out, int32_t* argmax_index, int32_t* launch_info, const float* in,
                    const float* norm_w, const int8_t* pre_q, const float* pre_s, const int8_t* wq, const float* ws, size_t n,
                    size_t rows, size_t rows_kv, size_t head_dim, size_t group_size, uint32_t flags, int device);
/* RMSNorm::forward                                                      layers.rs:109-119 */
int q3_op_rmsnorm(float* out, const float* in, const float* weight, size_t n, uint32_t flags, int device);
/* layers::softmax                                                       layers.rs:495-506 */
int q3_op_softmax(float* x, size_t n, uint32_t flags, int device);
/* FeedForward SwiGLU: hb = hb*sigmoid(hb)*hb2                           layers.rs:472-475 */
int q3_op_swiglu(float* hb, const float* hb2, size_t n, int device);
/* f32::exp as the device computes it (glibc expf algorithm), elementwise */
int q3_op_expf(float* x, size_t n, int device);
/* MultiHeadAttention: QK-RMSNorm + RoPE + GQA attention of ONE layer    layers.rs:346-419
 * key/value: the layer's cache [seq_len][kv_dim] (row `pos` holds the raw k/v projections on entry;
 * on return the K row is normalised+rotated in place).  q: [n_heads*head_dim] in/out.  xb: output. */
int q3_op_attention(float* xb, float* q, float* key_cache_layer, const float* value_cache_layer,
                    const float* q_norm_w, const float* k_norm_w, size_t pos, size_t seq_len, size_t n_heads,
                    size_t n_kv_heads, size_t head_dim, uint32_t flags, int device);
/* Sampler::sample with temperature > 0 on caller logits: one draw, *rng_state advanced by one coin   sampler.rs:118-139 */
int q3_op_sample(const float* logits, size_t n, float temperature, float topp, uint64_t* rng_state, int32_t* index, int device);
/* Sampler::sample_argmax                                                sampler.rs:57-59 */
int q3_op_argmax(const float* logits, size_t n, int32_t* index, int device);

/* ------------------------------------------------------------------------------------------------
 * 2d. (behind section 3 so that section 2c stays as it was.)  Draft verification under the sampler: section 2c for any
 * setting of q3_sampler_set.  Sampler::sample is a deterministic
 * function of (logits, rng state) with one xorshift64* coin per draw (sampler.rs:44-54,118-139), so the token the sequential
 * loop (generation.rs:153-162) draws at position first_pos + i depends only on the logits of the prefix and on the coin i + 1
 * steps behind the rng state at entry.  The rule: a draft is accepted exactly when it is the token the sampler draws -- the
 * draw of the column in front of it, made with that coin.  No rejection sampling, no second distribution: every returned
 * token, every cache row and the rng afterwards are bit-identical to q3_generate_sampled.  The pass is section 2c's with the
 * per-stream draws of the batched decode (one workgroup per column) in place of the argmax; the draw scratch of 32 columns
 * (~5.3 MB per column at a 151,936-entry vocabulary) is allocated by the first pass that samples.  Refused with
 * Q3_ERR_UNSUPPORTED: a Q3_FLAG_FAST engine and the shapes q3_batch_init refuses.
 * ------------------------------------------------------------------------------------------------ */

/* q3_verify under the sampler.  With the engine's temperature / top-p and R = the rng state at entry:
 *   next_tokens[i] = Sampler::sample(forward(tokens[i], first_pos + i)) drawn with the rng state i coins behind R   (sampler.rs:118-139)
 *   *n_accepted    = a = the number of leading drafts with tokens[j] == next_tokens[j - 1]
 * On return the engine is where q3_generate_sampled(tokens[0], first_pos, a + 1) leaves it: rows first_pos .. first_pos + a
 * written (the transposed value cache too), later rows restored, the single-stream state and output tokens set, and
 * q3_sampler_get_rng = R advanced a + 1 coins -- the draws behind a rejection are not consumed.  next_tokens[a + 1 ..) are
 * the draws the rejected columns made on the proposed prefix with their own coins; they change nothing.
 * logits_out: as for q3_verify, the raw logits (bit-identical to q3_forward; the sampler does not touch them).
 * With temperature 0 (or no q3_sampler_set) it is q3_verify: same results, no coin drawn.  Q3_ERR_ARG as for q3_verify. */
int q3_verify_draw(q3_engine* e, const int32_t* tokens, size_t n_tokens, size_t first_pos, int32_t* next_tokens, size_t* n_accepted,
                   float* logits_out);

/* q3_generate_lookup under the sampler: out_tokens, the engine state and the final rng equal those of
 * q3_generate_sampled(first_token, first_pos, n_tokens) (generation.rs:153-162 with Sampler::sample).  Rounds as in
 * q3_generate_lookup: no draft -> one ordinary sampled single-stream step through the decode graph; d drafts -> one pass.
 * stats as there.  A caller that stops at a token inside a call (BOS / EOS) has drawn the coins behind it: both front ends put
 * the rng back with q3_sampler_get_rng before and q3_sampler_set after such a round (cli/q3_cli.cpp). */
int q3_generate_lookup_draw(q3_engine* e, const int32_t* corpus, size_t n_corpus, size_t first_token, size_t first_pos, size_t n_tokens,
                            int ngram, int draft_len, int32_t* out_tokens, q3_spec_stats* stats);

/* ------------------------------------------------------------------------------------------------
 * 2e. (behind 2d so that the earlier sections stay as they were.)  Ragged column passes over the batched state of section 2b:
 * every column of a pass is a (slot, token, position) triple, so one pass over the packed weights can hold decode columns of
 * some streams next to several consecutive prompt positions of others.  This is what chunked prompts, slot reuse and serving
 * more requests than slots need; section 2b's "stream i uses KV slot i, one position per stream" is the special case
 * slots = 0 .. n - 1.  The layers are the short block's of q3_prefill_batched (all key and value rows of the pass enter the
 * caches before any column attends) with every column's cache base taken from a slot table; the classifier is the n-column
 * one of the batched decode.  The standard is section 2b's: logits and cache rows are bit-identical to feeding the slot's
 * token history through q3_forward on a fresh engine of the same context.  Greedy only.
 * ------------------------------------------------------------------------------------------------ */
#define Q3_COLS_MAX 32

/* One pass of n_cols (1 .. Q3_COLS_MAX) columns: column j runs forward(tokens[j], pos[j]) over the KV cache of slot slots[j].
 * The columns of one slot form a RUN: they are adjacent, their positions are consecutive and ascending, and a slot has at most
 * one run in a pass.  Column j of a run sees the rows the run's earlier columns write in the same pass; like q3_forward, a
 * column reads rows 0 .. pos[j] of its slot and nothing else, so a slot need not be cleared between two sequences.
 * next_out[j] = sample_argmax of column j; logits_out row j = its logits.  Each may be NULL.
 * A pass of n_cols columns runs a plan of the next width in {1, 2, 4, 8, 16, 32}, the columns past n_cols repeating the last
 * one (same slot, token and position: the same bits to the same rows); the plans are built on first use and kept, so passes
 * of changing width rebuild nothing, and neither do calls of section 2b in between after their first.
 * Q3_ERR_ARG: no q3_batch_init; n_cols outside 1 .. Q3_COLS_MAX; a slot outside 0 .. max_streams - 1; a slot in two runs; a run
 * whose positions are not consecutive; a token outside the vocabulary; a position >= the batch context.
 * Q3_ERR_UNSUPPORTED: a Q3_FLAG_FAST engine (its block and decode kernels are not bit-equal to each other, as in section 2c);
 * a batch sampler set to a temperature > 0 (q3_batch_sampler_set); the shapes the short prefill block refuses ("needs the
 * per-kv-head attention kernel"). */
int q3_batch_step_cols(q3_engine* e, const int32_t* slots, const int32_t* tokens, const int32_t* pos, int n_cols,
                       float* logits_out /* [n_cols][vocab] or NULL */, int32_t* next_out /* [n_cols] or NULL */);

typedef struct q3_cols_stats { uint64_t passes, live_columns, prompt_columns, decode_columns; } q3_cols_stats;

/* The pass table q3_generate_many_greedy runs, as a pure function of the lengths (host only, never touches the GPU).  Request r
 * has a prompt of prompt_len[r] >= 1 tokens and wants n_new[r] >= 1 tokens.  A slot holding a request is in its PROMPT phase
 * until the last prompt token has been through a pass and in its DECODE phase afterwards.  Pass after pass, until no request is
 * queued or held:
 *   1. Admit.  While a slot is free and requests are queued, the next request, in ascending index, takes the lowest free slot.
 *   2. Decode columns first: one column per decode-phase slot, in ascending slot order; its token is the slot's last produced
 *      token, its position prompt_len + g - 1 with g tokens produced so far.
 *   3. Prompt columns fill the rest of the Q3_COLS_MAX columns: prompt-phase slots in ascending slot order, each taking
 *      min(remaining prompt, remaining columns) consecutive positions (a slot that finds no column left waits).
 *   4. A run that reaches its prompt's last token produces y_0 in that pass; the slot decodes from the next pass.
 *   5. A request that has produced n_new tokens frees its slot for the next pass.
 * (A prompt-phase slot at the front always gets a column: it holds a slot itself, so at most 31 slots decode beside it.)
 * table (may be NULL: count only): one entry {pass, slot, position, request} per column, passes ascending, columns in pass
 * order; *n_entries = the number of columns whether or not they fit; stats as for the loop.  n_entries, stats may be NULL.
 * Q3_ERR_ARG: no request, a prompt_len or n_new of 0, max_streams outside 1 .. 32, a table smaller than the schedule; a prompt_len
 * or n_new above INT32_MAX, or lengths whose running sum is (the table is int32_t, and so are the scheduler's records: refused at
 * once, as q3_cols_schedule_stop and the loops refuse them). */
int q3_cols_schedule(const size_t* prompt_len, const size_t* n_new, size_t n_requests, int max_streams,
                     int32_t* table /* [cap][4]: pass, slot, pos, request */, size_t cap, size_t* n_entries, q3_cols_stats* stats);

/* n_requests greedy generations through the max_streams slots of the batched state, by the schedule above.  Request r yields
 * y_0 .. y_{n_new[r] - 1} at out_tokens[n_new[0] + .. + n_new[r - 1] ..]: y_0 = q3_prefill(prompt_r, 0) and the rest
 * q3_generate_greedy(y_0, prompt_len[r], n_new[r] - 1), both on a fresh engine -- bit-identical whatever else shares its passes
 * and whatever the slot held before (slots are not cleared between occupants).  No EOS check, as in q3_generate_greedy.
 * Device-resident: the pass table and the prompts are uploaded once, a small kernel between two passes resolves every column's
 * token (a prompt token or the slot's last token), writes the states and the slot table of the next pass and stores the tokens
 * the last pass produced; the passes replay one captured graph per plan width; only token ids cross PCIe and the call
 * synchronises once, at its end.  stats may be NULL.
 * Q3_ERR_ARG: an empty prompt, n_new[r] == 0, prompt_len[r] + n_new[r] - 1 > the batch context, a token outside the vocabulary;
 * otherwise as q3_batch_step_cols. */
int q3_generate_many_greedy(q3_engine* e, const int32_t* prompts /* concatenated */, const size_t* prompt_len, const size_t* n_new,
                            size_t n_requests, int32_t* out_tokens /* concatenated, n_new[r] each */, q3_cols_stats* stats);

/* ------------------------------------------------------------------------------------------------
 * 2f. (behind 2e so that the earlier sections stay as they were.)  Column passes under the sampler: section 2e for any sampler
 * setting, per slot and per request.  Sampler::sample is a deterministic function of (logits, rng state) with one xorshift64* coin
 * per draw (sampler.rs:44-54,118-139), and the prompt loop of `chat` draws and discards one sample per prompt position
 * (generation.rs:116-123), which q3_prefill reproduces.  The rule: column k of a slot's run is drawn with the slot's rng advanced
 * k coins, and after the pass the slot's rng is advanced by the run's length.  Only the draw behind a prompt's last position and
 * the draws of decode columns are made and kept; an interior prompt column consumes its coin and does no sampling work.  No
 * rejection sampling, no second distribution: tokens and cache rows are bit-identical to q3_sampler_set + q3_prefill +
 * q3_generate_sampled on a fresh single-stream engine, whatever else shares the passes, whichever slot a request lands in and
 * whatever that slot held before.  (generate-mode coin accounting -- generation.rs:25-39, no coin on interior prompt positions --
 * is not offered: this section follows q3_prefill, as q3_generate_many_greedy does.)
 * A pass is section 2e's plan with the per-column draws of section 2d behind the classifier (their scratch of 32 columns is
 * allocated by the first pass that samples) and a turn kernel that commits draws; the plans are a second set of six, built on
 * first use.  Temperature and top-p are read from device memory when a pass runs: changing them rebuilds nothing.  The names of
 * section 2e launch exactly what they launched before.
 * ------------------------------------------------------------------------------------------------ */

/* q3_batch_step_cols under the per-slot samplers of q3_batch_sampler_set (slot i = stream i: the same rng stream q3_forward_batch
 * advances).  Column j at index k of its slot's run is drawn with that slot's rng advanced k coins; afterwards the slot's rng is
 * advanced by the run's length.  keep[j] == 0: the coin is consumed, no draw is made and next_out[j] = -1 (the prompt loop's
 * discarded sample); otherwise next_out[j] is the draw, the token q3_forward_sample returns at that point of the slot's history on
 * an engine seeded like the slot.  logits_out: the raw logits, as in q3_verify_draw.  With temperature 0, or no batch sampler
 * set, it is q3_batch_step_cols: argmax, no coin, keep ignored.  Errors: those of q3_batch_step_cols, except that a sampling
 * batch is accepted. */
int q3_batch_step_cols_draw(q3_engine* e, const int32_t* slots, const int32_t* tokens, const int32_t* pos, int n_cols,
                            const uint8_t* keep /* [n_cols] or NULL = all kept */, float* logits_out, int32_t* next_out);

/* q3_generate_many_greedy under one sampler per request: the schedule of q3_cols_schedule, unchanged, and the same output layout.
 * Request r yields the tokens of a fresh single-stream engine after q3_sampler_set(temperature[r], topp[r], seeds[r]):
 * y_0 = q3_prefill(prompt_r, 0), y_1 .. = q3_generate_sampled(y_0, prompt_len[r], n_new[r] - 1).  A request's first column loads
 * its sampler into the slot it landed in.  temperature[r] == 0: the request is greedy (argmax, no coin, seed ignored); greedy and
 * sampled requests may share passes.  Device-resident like the greedy loop: the table, the prompts and the per-request sampler
 * parameters are uploaded once, the passes replay one captured graph per plan width, only token ids cross PCIe and the call
 * synchronises once.  It keeps per-slot sampler states of its own and needs no q3_batch_sampler_set; the per-stream sampler
 * states of section 2b are unspecified after the call: call q3_batch_sampler_set again before the next sampled call of section 2b
 * or q3_batch_step_cols_draw.
 * Q3_ERR_ARG: a null array, a negative or NaN temperature, a top-p outside [0, 1], and everything q3_generate_many_greedy rejects.
 * Q3_ERR_UNSUPPORTED: a Q3_FLAG_FAST engine, the shapes the short prefill block refuses. */
int q3_generate_many_sampled(q3_engine* e, const int32_t* prompts /* concatenated */, const size_t* prompt_len, const size_t* n_new,
                             size_t n_requests, const float* temperature, const float* topp, const uint64_t* seeds /* [n_requests] each */,
                             int32_t* out_tokens /* concatenated, n_new[r] each */, q3_cols_stats* stats);

/* ------------------------------------------------------------------------------------------------
 * 2g. (behind 2f so that the earlier sections stay as they were.)  Dense blocks over the slots: many prompts per weight pass.
 * A column pass holds 32 columns, so a 2,048-token prompt enters its slot in 64 passes over the weights.  q3_prefill_batched
 * moves such a prompt through the dense kernels in one block, but only into the single-stream cache.  Here the columns of a dense
 * block are RUNS of several slots of section 2b's state: a run is a slot and consecutive ascending positions of that slot, a slot
 * has at most one run in a block, every run starts at a column that is a multiple of 8, and the columns between a run's end and
 * the next run's start (or the block's end, rounded up to 8) repeat the run's last column -- same slot, token and position, the
 * same bits to the same rows: the pad rule of sections 2c and 2e.  Every column takes its cache base from a slot table as long
 * as the block.  The standard is section 2e's: cache rows and every token are bit-identical to q3_prefill on a fresh engine,
 * whichever slot a prompt lands in, whatever shares its block and whatever the slot held before.  A block forms no logits (the
 * reference computes and discards them for prompt positions): a prompt's last token goes through a column pass.
 * Blocks hold up to Q3_PREFILL_M columns (default 2,048, as for q3_prefill_batched).  Their scratch -- the per-column buffers and the
 * attention score rows, 4 * M * n_heads * (largest first_pos + length of a call, rounded up to 256) bytes -- sits beside the
 * 32-column scratch of q3_batch_init, is allocated by the first call that needs it and released with the batched state
 * (q3_batch_init starts it over); using it rebuilds none of the kept plans of sections 2b, 2e and 2f.  A block of 32 columns or
 * fewer is an ordinary column pass of its live columns (under a sampler every one with keep = 0); a shape the dense kernels do not
 * take (group size other than 64, head_dim other than 128, other than 2 or 4 query heads per kv head) packs with a cap of 32, so
 * every shape q3_batch_step_cols accepts works.
 * ------------------------------------------------------------------------------------------------ */
typedef struct q3_dense_stats { uint64_t blocks, live_columns, pad_columns; } q3_dense_stats;

/* How runs are packed into blocks, as a pure function of the lengths (host only, never touches the GPU):
 *   1. Runs are taken in index order.
 *   2. A run starts at the next multiple of 8 behind the last piece of the current block; where that is block_cap, the block is
 *      closed and the run starts the next one at column 0.
 *   3. It takes min(what is left of it, block_cap - start) columns; what did not fit continues as the first piece of the next
 *      block.  A run therefore never has two pieces in one block, and its pieces are consecutive in the table.
 * A block's width is the end of its last piece rounded up to 8; pad_columns counts, over all blocks, width - live columns.
 * table (may be NULL: count only): one entry {block, first column, run, offset in the run} per piece, in order; a piece ends where
 * the run's next piece starts or the run ends.  *n_entries = the number of pieces whether or not they fit.  n_entries, stats may
 * be NULL.  Q3_ERR_ARG: no run, a run_len of 0, block_cap below 16 or not a multiple of 16, a table smaller than the packing. */
int q3_dense_pack(const size_t* run_len, size_t n_runs, int block_cap, int32_t* table /* [cap][4]: block, first column, run, offset in the run */,
                  size_t cap, size_t* n_entries, q3_dense_stats* stats);

/* Cache rows only: run r feeds tokens[run_len[0] + .. + run_len[r - 1] ..] into slot slots[r] at positions first_pos[r] ..
 * first_pos[r] + run_len[r] - 1, the runs packed by q3_dense_pack with block_cap = Q3_PREFILL_M.  Afterwards those rows of the
 * slot's key and value caches are bit-identical to what q3_prefill writes -- to what q3_forward of the same tokens at those
 * positions writes on a fresh engine holding the same earlier rows -- and no other row of any slot has changed.  No logits, no
 * token: send the prompt's last token through q3_batch_step_cols.
 * Under a sampling batch (q3_batch_sampler_set, temperature > 0) the rng of slot slots[r] is advanced by run_len[r] coins, the
 * rule of section 2f; q3_batch_step_cols_draw of the prompt's last token then draws the token q3_prefill returns.  With
 * temperature 0, or no batch sampler, no rng is touched.  The call synchronises once.  stats may be NULL.
 * Q3_ERR_ARG: no q3_batch_init; no run; a slot outside 0 .. max_streams - 1; a slot named twice; an empty run; a position at or past
 * the batch context; a token outside the vocabulary.
 * Q3_ERR_UNSUPPORTED: a Q3_FLAG_FAST engine; the shapes q3_batch_step_cols refuses. */
int q3_batch_prefill_slots(q3_engine* e, const int32_t* slots, const int32_t* tokens /* concatenated */, const size_t* run_len,
                           const int32_t* first_pos, size_t n_runs, q3_dense_stats* stats);

/* q3_generate_many_greedy (temperature, topp and seeds all NULL) or q3_generate_many_sampled with long prompts entered through
 * dense blocks.  The output layout and every output token are theirs, for any dense_min.
 *   Request r is DENSE when dense_min > 0 and prompt_len[r] - 1 >= dense_min; dense_min == 0 runs the loops of sections 2e / 2f
 *   unchanged.  The column schedule is q3_cols_schedule with a dense request's prompt length taken as 1: its one prompt column is
 *   its last prompt token at position prompt_len[r] - 1, and its decode columns follow from there.
 *   In front of every pass, the dense requests whose prompt column the pass holds are packed by q3_dense_pack in ascending
 *   request index, each a run of prompt_len[r] - 1 tokens at position 0 of the slot the schedule gave it, and their blocks are
 *   enqueued on the stream in front of the pass (a block of 32 columns or fewer as a column pass of its own).
 *   Under the sampler a dense request's first column pass column loads its (temperature, top-p, seed) into the slot, and its
 *   prompt column is drawn with the seed state advanced prompt_len[r] - 1 coins.
 * The host knows all of this from the lengths: the loop stays device-resident and synchronises once.  stats counts the passes of
 * the column schedule as q3_cols_schedule does for the lengths above; dstats the blocks (narrow ones included).  Either may be NULL.
 * Errors as for q3_generate_many_greedy / q3_generate_many_sampled; some but not all of the three sampler arrays NULL: Q3_ERR_ARG. */
int q3_generate_many_dense(q3_engine* e, const int32_t* prompts /* concatenated */, const size_t* prompt_len, const size_t* n_new,
                           size_t n_requests, const float* temperature, const float* topp, const uint64_t* seeds /* all three NULL: greedy */,
                           size_t dense_min, int32_t* out_tokens /* concatenated, n_new[r] each */, q3_cols_stats* stats, q3_dense_stats* dstats);

/* ------------------------------------------------------------------------------------------------
 * 2h. (behind 2g so that the earlier sections stay as they were.)  Stop tokens in the loop: requests end at EOS and free their
 * slot at once.  The loops of sections 2e / 2f run a pass table that is a pure function of (prompt_len, n_new); for chat traffic
 * n_new is a cap, and a request that emits EOS at token 20 of 512 would hold its slot, and a column of every pass, for 492 more
 * passes.  Here the device decides after every pass which requests have ended, frees their slots, admits the next queued
 * requests and lays out the next pass.
 * With n_emit[r] = the index of the first stop token among request r's tokens plus one, or n_new[r] if there is none: rule 5 of
 * q3_cols_schedule frees a slot when its request has produced n_new tokens, so a request that ends at its stop token is exactly
 * a request with n_new[r] = n_emit[r].  The loop runs, pass for pass and column for column, the schedule
 * q3_cols_schedule(prompt_len, n_emit, ...), and every token it returns is bit-identical to what q3_generate_many_greedy /
 * q3_generate_many_sampled return for the same request.
 * A small kernel between two passes applies the five rules to a scheduler state in device memory and writes the next pass as a
 * table of one row; the kept plans of sections 2e / 2f and their turn kernels run it unchanged.  The host reads one 8-byte status
 * per pass (the number of live columns picks the plan width): ONE SYNCHRONISATION PER PASS, where the loops of 2e / 2f
 * synchronise once per call.  The names of the earlier sections launch exactly what they launched before.
 * Dense blocks (q3_generate_many_dense's dense_min) are not offered in this section: every prompt enters through column passes.
 * ------------------------------------------------------------------------------------------------ */
#define Q3_STOP_MAX 8

/* q3_generate_many_greedy (temperature, topp and seeds all NULL) or q3_generate_many_sampled, ending every request at its first
 * stop token.  The output layout is theirs: request r's tokens start at out_tokens[n_new[0] + .. + n_new[r - 1]]; its first
 * n_out[r] entries are its tokens, the stop token included as the last one, and the entries behind them are -1.
 * n_out[r] == n_emit[r] as defined above.  stats counts the passes actually run: those of q3_cols_schedule(prompt_len, n_emit).
 * Under the sampler the rules of section 2f hold: a request's first column loads its sampler into the slot, greedy and sampled
 * requests may share passes, and no coin is drawn behind a stop token.  n_stop == 0: the call equals the loops of 2e / 2f.
 * Q3_ERR_ARG: n_stop > Q3_STOP_MAX; a null stop_tokens with n_stop > 0; a stop token outside the vocabulary; a null n_out; some
 * but not all of the three sampler arrays NULL; everything q3_generate_many_greedy / q3_generate_many_sampled reject.
 * Q3_ERR_UNSUPPORTED: as for those two.
 * Q3_ERR_INTERNAL: the scheduler asked for more than sum(prompt_len[r] + n_new[r]) passes (every pass advances at least one
 * column, so it cannot): a bug ends as an error code, never as an endless loop. */
int q3_generate_many_stop(q3_engine* e, const int32_t* prompts /* concatenated */, const size_t* prompt_len, const size_t* n_new,
                          size_t n_requests, const float* temperature, const float* topp, const uint64_t* seeds /* all three NULL: greedy */,
                          const int32_t* stop_tokens, size_t n_stop, int32_t* out_tokens /* concatenated, n_new[r] each */,
                          size_t* n_out /* [n_requests] */, q3_cols_stats* stats);

/* The passes q3_generate_many_stop runs when request r would produce the tokens rows[n_new[0] + .. + n_new[r - 1] ..] (host only,
 * never touches the GPU): the scheduler step of the device loop, run pass by pass on the host and fed from rows.  table,
 * n_entries and stats as for q3_cols_schedule; n_out as for q3_generate_many_stop; each may be NULL.
 * Q3_ERR_ARG: what q3_cols_schedule rejects, null rows, n_stop > Q3_STOP_MAX, a null stop_tokens with n_stop > 0. */
int q3_cols_schedule_stop(const size_t* prompt_len, const size_t* n_new, size_t n_requests, int max_streams,
                          const int32_t* rows /* concatenated, n_new[r] each */, const int32_t* stop_tokens, size_t n_stop,
                          int32_t* table /* [cap][4]: pass, slot, pos, request */, size_t cap, size_t* n_entries, size_t* n_out,
                          q3_cols_stats* stats);

/* ------------------------------------------------------------------------------------------------
 * 2i. (behind 2h so that the earlier sections stay as they were.)  A shared prompt prefix: prefill once, copy its key and value
 * rows to the slots.  Chat requests begin with the same system prompt, template or few-shot block, and the loops of sections 2e to 2h
 * send those tokens through the weights again for every request.  Those sections guarantee that a slot's cache rows are bit-identical
 * whichever slot a request lands in and whatever the slot held before, so the rows of a shared prefix are the same bits in every
 * slot: sharing them is a copy, with nothing to approximate and no tolerance.
 * The batched caches are f32 [stream][layer][context][kv_dim], so rows [p, p + n) of one layer of one slot are one contiguous run in
 * the key cache and one in the value cache.  One kernel launch copies such runs of every layer of both caches from one source to up
 * to 32 destinations; every source word is read once and written once per destination, as raw 32-bit words (NaN payloads, -0.0 and
 * denormals pass through).  The prefix is COPIED into each slot and the attention kernels read it there as they read any other
 * row.  Not offered: dense entry of the suffixes (q3_generate_many_dense's dense_min), a different prefix per request, and
 * attention that reads a shared prefix in place without the copy.
 * ------------------------------------------------------------------------------------------------ */

/* Rows first_pos .. first_pos + n_rows - 1 of every layer of src_slot's key and value caches are copied into each of the n_dst slots
 * dst_slots[i].  No other row of any slot changes and no rng is touched.  This is what forking needs: several samples of one prompt,
 * or one conversation continued several ways.  Allowed on a Q3_FLAG_FAST engine (it only copies).  The call synchronises once.
 * Q3_ERR_ARG: no q3_batch_init; n_dst outside 1 .. max_streams - 1; a slot outside 0 .. max_streams - 1; src_slot among the
 * destinations; a destination named twice; n_rows == 0; first_pos + n_rows > the batch context. */
int q3_batch_copy_rows(q3_engine* e, int src_slot, const int32_t* dst_slots, int n_dst, size_t first_pos, size_t n_rows);

/* The resident prefix.  tokens[0 .. n) are prefilled at positions 0 .. n - 1 INTO SLOT 0 -- rows 0 .. n - 1 of slot 0 are overwritten
 * -- by the blocks and passes of q3_batch_prefill_slots (dense blocks where the shape takes them, column passes otherwise), in a form
 * that touches no slot rng whatever q3_batch_sampler_set says.  The rows are then copied into a prefix store of
 * 2 * n_layers * n * kv_dim floats, allocated beside the batched state and released with it (q3_batch_init drops it).  The store is
 * private to this section: no other entry point reads or writes it, q3_batch_reset_kv leaves it alone, and whatever later calls do
 * to slot 0 does not change it.  The engine keeps n and a copy of the tokens.  n == 0 releases the store; a new prefix replaces the
 * old one; a call that fails leaves no prefix resident.
 * Q3_ERR_ARG: no q3_batch_init; n >= the batch context; a token outside the vocabulary.
 * Q3_ERR_UNSUPPORTED: what q3_batch_prefill_slots refuses (a Q3_FLAG_FAST engine, the shapes q3_batch_step_cols refuses). */
int q3_batch_prefix_set(q3_engine* e, const int32_t* tokens, size_t n);

/* What is resident: *n = the number of prefix tokens (0: none, also without q3_batch_init); tokens (may be NULL) receives the
 * first min(*n, cap) of them. */
int q3_batch_prefix_get(const q3_engine* e, size_t* n, int32_t* tokens, size_t cap);

/* q3_generate_many_stop for requests that all begin with the resident prefix of P tokens.  The arguments are those of
 * q3_generate_many_stop; prompts and prompt_len are each request's SUFFIX, at least one token, behind the prefix.
 * For every request r, out_tokens and n_out[r] are exactly what q3_generate_many_stop returns for the full prompt prefix ++ suffix_r
 * with the same sampler arrays and stop set -- with n_stop == 0, what q3_generate_many_greedy / q3_generate_many_sampled return.
 * The passes are those of q3_cols_schedule(suffix lengths, n_emit) with P added to every position, and stats counts them: the
 * schedule no longer contains the prefix.
 * In front of the first pass one kernel launch copies the store into rows 0 .. P - 1 of the min(n_requests, max_streams) lowest
 * slots, the slots the schedule can use (rule 1 admits into the lowest free slot).  Requests write only rows >= P and slots are not
 * cleared between occupants, so the one copy serves every later occupant of a slot.  n_stop == 0 runs the tabled loop of sections
 * 2e / 2f: device-resident, the copy enqueued on the engine's stream, one synchronisation per call.  n_stop > 0 runs the loop of
 * section 2h.
 * Under the sampler the prompt loop draws and discards one coin per prompt position (section 2f), so a sampled request enters its
 * first column with its seed state advanced P coins; a greedy request draws no coin.
 * Dense entry of the suffixes (dense_min) is not offered in this section: every suffix enters through column passes.
 * Q3_ERR_ARG: no resident prefix; P + prompt_len[r] + n_new[r] - 1 > the batch context; everything q3_generate_many_stop rejects.
 * Q3_ERR_UNSUPPORTED, Q3_ERR_INTERNAL: as for q3_generate_many_stop. */
int q3_generate_many_prefix(q3_engine* e, const int32_t* prompts /* suffixes, concatenated */, const size_t* prompt_len, const size_t* n_new,
                            size_t n_requests, const float* temperature, const float* topp, const uint64_t* seeds /* all three NULL: greedy */,
                            const int32_t* stop_tokens, size_t n_stop, int32_t* out_tokens /* concatenated, n_new[r] each */,
                            size_t* n_out /* [n_requests] */, q3_cols_stats* stats);

/* ------------------------------------------------------------------------------------------------
 * 2j. (behind 2i so that the earlier sections stay as they were.)  Embeddings: the last-token vectors of many prompts through
 * dense blocks.  A Qwen3 checkpoint that is an embedding model (the Qwen3-Embedding family: the same architecture, the same Q8
 * export) never uses the classifier: its output is the hidden state of the last prompt token behind the final RMSNorm,
 * L2-normalised and possibly cut to a leading sub-vector.  The blocks of section 2g run every layer in full for every column and
 * launch nothing behind the layers, so when a block ends its scratch x[column][dim] holds the last layer's residual of every
 * column.  One more kernel (k_embed_rows, csrc/q3_embed.h), one workgroup per prompt that ENDS in the block, computes for that
 * column, in f32 with no FMA contraction, exactly
 *     ss  = (((-0.0 + x0*x0) + x1*x1) + ... )       over dim terms
 *     f   = 1.0f / sqrtf(ss / (float)dim + 1e-6f)
 *     y_i = w_i * (f * x_i)                          i < dim, w = the final norm's weight          (RMSNorm::forward, layers.rs:109-119)
 * and with Q3_EMBED_L2, over the FIRST out_dim components only,
 *     s2  = (((-0.0 + y0*y0) + y1*y1) + ... )       over out_dim terms
 *     nrm = sqrtf(s2);  d = nrm > 1e-12f ? nrm : 1e-12f     (torch F.normalize's eps; a NaN nrm takes the eps)
 *     out_i = y_i / d                                IEEE divide, i < out_dim
 * Without the flag out_i = y_i for i < out_dim.  No classifier runs anywhere in the call: a block of 32 columns or fewer, and
 * every block of a shape the dense kernels refuse, runs the layer launches of the kept column plan of section 2e and stops in
 * front of its classifier, its columns set up from a run table as a wide block's are.
 * ------------------------------------------------------------------------------------------------ */
#define Q3_EMBED_L2     1u   /* L2-normalise the (possibly truncated) vector */
#define Q3_EMBED_PREFIX 2u   /* prompts are SUFFIXES behind the resident prefix of section 2i */
typedef struct q3_embed_stats { uint64_t waves, blocks, live_columns, pad_columns; } q3_embed_stats;

/* out[r][0 .. out_dim) = the vector of request r, whose prompt is prompts[prompt_len[0] + .. + prompt_len[r - 1] ..] -- with
 * Q3_EMBED_PREFIX the resident prefix of P tokens followed by those tokens.  out_dim 0 means dim.
 * Standard: row r without Q3_EMBED_L2 and with out_dim = dim is bit-identical to q3_read_state kind 2 after q3_prefill(t[0 .. n - 1))
 * followed by q3_forward(t[n - 1], n - 1) on a fresh engine of the same context, t the request's n prompt tokens.  It does not
 * depend on the slot, on the neighbours in the block, on the slot's earlier contents or on the wave.  The other flag and out_dim
 * apply the arithmetic above to that row.
 * Schedule, a pure function of the lengths: requests go in index order; with S = max_streams, wave w holds requests
 * [w S, (w + 1) S); the i-th request of a wave uses slot i from position 0 (with Q3_EMBED_PREFIX from position P); each wave is
 * packed on its own by the rule of q3_dense_pack with block_cap = Q3_PREFILL_M (32 for a shape the dense kernels refuse), so a
 * slot has at most one run per block; blocks are enqueued in order, and behind each block one k_embed_rows launch covers the runs
 * that end in it (a run whose last piece lies in a later block is not named; pad columns never are).  stats (may be NULL): the
 * number of waves and the sums of the per-wave q3_dense_stats.
 * Execution: everything is enqueued on the engine's stream -- the uploads of the prompts, the run tables and the gather tables,
 * with Q3_EMBED_PREFIX one launch that copies the store into rows 0 .. P - 1 of the min(n_requests, S) lowest slots, then the
 * blocks and their gathers -- followed by ONE device-to-host copy and ONE synchronisation.  (A call that has to enlarge one of
 * its device buffers waits for the stream before it does.)  The device output rows belong to the batched state: grown on
 * demand, released with it.  The blocks run in the form q3_batch_prefix_set uses: no slot rng is touched whatever
 * q3_batch_sampler_set says.  The kept decode, column and dense plans and their graphs are not rebuilt.
 * Afterwards rows first .. first + len - 1 of the slots used hold the prompts' cache rows, as after q3_batch_prefill_slots, and
 * no other row has changed.  THE SLOTS ARE OVERWRITTEN FROM SLOT 0 UP: A CALLER WITH LIVE REQUESTS IN THE SLOTS MUST NOT CALL THIS.
 * Every failing call leaves the engine usable.
 * Q3_ERR_ARG: a null engine (checked before anything touches the GPU) or null arrays; n_requests == 0; no q3_batch_init; an empty
 * prompt; a token outside the vocabulary; P + prompt_len[r] > the batch context; out_dim > dim; unknown flag bits;
 * Q3_EMBED_PREFIX with no resident prefix.
 * Q3_ERR_UNSUPPORTED: what q3_batch_prefill_slots refuses (a Q3_FLAG_FAST engine, the shapes q3_batch_step_cols refuses). */
int q3_embed_many(q3_engine* e, const int32_t* prompts /* concatenated */, const size_t* prompt_len, size_t n_requests,
                  uint32_t flags, size_t out_dim /* 0 = dim */, float* out /* host, [n_requests][out_dim] */, q3_embed_stats* stats);

/* ------------------------------------------------------------------------------------------------
 * 2k. (behind 2j so that the earlier sections stay as they were.)  Choice logits: the classifier's scores of a few candidate tokens
 * behind the last position of many prompts.  A reranker (the Qwen3-Reranker family: the same architecture, the same Q8 export, read
 * out as softmax([logit("no"), logit("yes")])[1]), a multiple-choice evaluator or a yes/no classifier asks for k numbers of the
 * vocab_size the classifier can produce.  The prompts go through the blocks of section 2j, which run no classifier, and behind each
 * block one more kernel (k_choice_rows, csrc/q3_choice.h), one workgroup per (prompt that ENDS in the block, part of 32
 * candidates), computes for the column x of the prompt's last token and a candidate id c, in f32 with no FMA contraction, exactly
 *     ss   = (((-0.0 + x0*x0) + x1*x1) + ... )      over dim terms
 *     f    = 1.0f / sqrtf(ss / (float)dim + 1e-6f)
 *     y_i  = w_i * (f * x_i)                         w = the final norm's weight                    (RMSNorm::forward, layers.rs:109-119)
 *   per group g of G = group_size consecutive i:
 *     xs_g = max|y_i| / 127.0f;   xq_i = round-half-away(y_i / xs_g) as i8, IEEE divide, saturating, NaN -> 0;  xs_g == 0: xq_i = 0
 *                                                                                                    (tensor.rs:91-119)
 *     d_g  = sum over the group of wq[c][i] * xq_i   in int32, exact
 *     t_g  = ((float)d_g * ws[c][g]) * xs_g          two roundings                                  (tensor.rs:59)
 *   logit  = (((t_0 + t_1) + t_2) + ... )            groups ascending
 * with wq / ws the classifier matrix: the token embedding table under shared_classifier, lm_head otherwise.  This is the arithmetic
 * of the single-stream classifier launch, restated for k rows: the norm and the quantizer are that launch's own prologue code.  No
 * other row of the matrix is read, no full-vocabulary pass runs, and nothing is normalised on the device: softmax over the
 * candidates is the caller's (generation.choose does it on the host in float64).
 * ------------------------------------------------------------------------------------------------ */
#define Q3_CHOICE_PREFIX      2u   /* prompts are SUFFIXES behind the resident prefix of section 2i (the bit of Q3_EMBED_PREFIX) */
#define Q3_CHOICE_PER_REQUEST 4u   /* cand holds one list of k ids per request, [n_requests][k]; otherwise one list [k] for all */
#define Q3_CHOICE_MAX 256

/* out[r][j] = the logit of token cand_r[j] behind the last token of request r, cand_r = cand + r k with Q3_CHOICE_PER_REQUEST and
 * cand otherwise.  Prompts, prompt_len and the prefix flag are those of q3_embed_many.
 * Standard: out[r][j] is bit-identical to logits[cand_r[j]] of q3_forward(t[n - 1], n - 1) after q3_prefill(t[0 .. n - 1)) on a fresh
 * single-stream engine of the same context, t the request's n prompt tokens.  An id may appear more than once in a list and gives
 * equal values.  The value does not depend on the slot, the neighbours in the block, the other candidates or the wave.
 * Schedule, slots, execution and stats: exactly those of q3_embed_many (one walk serves both), with k_choice_rows in the place of
 * k_embed_rows and one more upload, the candidate ids; ONE device-to-host copy of [n_requests][k] floats and ONE synchronisation.
 * The uploaded ids and the device output rows belong to the batched state: grown on demand (the stream is waited for first),
 * released with it.  No slot rng is touched.  THE SLOTS ARE OVERWRITTEN FROM SLOT 0 UP, as by q3_embed_many.
 * Every failing call leaves the engine usable.
 * Q3_ERR_ARG: everything q3_embed_many refuses (out_dim aside); a null cand; k == 0 or k > Q3_CHOICE_MAX; a candidate outside
 * [0, vocab_size); unknown flag bits.
 * Q3_ERR_UNSUPPORTED: what q3_embed_many refuses; dim > 4096, more than the norm prologue holds (refused before anything is
 * enqueued). */
int q3_choice_many(q3_engine* e, const int32_t* prompts /* concatenated */, const size_t* prompt_len, size_t n_requests,
                   const int32_t* cand, size_t k, uint32_t flags, float* out /* host, [n_requests][k] */, q3_embed_stats* stats);

/* ------------------------------------------------------------------------------------------------
 * 2l. (behind 2k so that the earlier sections stay as they were.)  Scores: what the model says about every next token of many
 * given sequences -- perplexity, the log-likelihood of a continuation of several tokens, "is this continuation the greedy one",
 * filtering by loss.  For position i of a sequence t that needs log P(t[i+1] | t[0..i]): a log-softmax over the whole vocabulary
 * at every position.  The prompts go through the blocks of section 2j.  Behind each block its SCORED columns are copied, up to 32
 * at a time, into the 32-column scratch (k_score_gather, csrc/q3_score.h) and run through the classifier of a kept column plan of
 * section 2e -- the final norm, the quantizer and the int8 matrix-core launch: for all V = vocab_size rows c the logit l[c] of
 * section 2k, bit-identical to q3_forward's -- and two more kernels reduce each row l[0 .. V) on the device to a record, in f32
 * with no FMA contraction:
 *     target = l[t[i+1]]
 *     max    = fmaxf(... fmaxf(fmaxf(-inf, l[0]), l[1]) ..., l[V-1])                                    (layers.rs:496)
 *     sum    = ((-0.0f + expf(l[0] - max)) + expf(l[1] - max)) + ...          in index order, V terms   (layers.rs:497-503)
 *     argmax = the last index of the maximum in total order (-0.0 below +0.0)                          (sampler.rs:57-59)
 * sum is the denominator Sampler::sample forms at temperature 1 (k_score_exp spreads the exps over the chip; k_score_sum walks them
 * with the verified sequential sum of the device sampler).  max and argmax are read from the keys the classifier launch leaves per
 * workgroup.  Nothing else is computed on the device: there is no logf; log P = (target - max) - log(sum) is the caller's
 * (generation.logprobs_of forms it in float64).  No logit leaves the GPU, and none becomes an address.
 * ------------------------------------------------------------------------------------------------ */
typedef struct q3_score_rec { float target; float max; float sum; int32_t argmax; } q3_score_rec;
typedef struct q3_score_stats { uint64_t waves, blocks, live_columns, pad_columns, chunks, scored; } q3_score_stats;
#define Q3_SCORE_PREFIX 2u   /* prompts are SUFFIXES behind the resident prefix of section 2i (the bit of Q3_EMBED_PREFIX) */

/* Request r of n = prompt_len[r] tokens t gets n - score_from[r] records, the requests' records concatenated in out.  Record j
 * describes the logits behind token t[i], i = score_from[r] - 1 + j, with target t[i + 1].  1 <= score_from[r] <= n; score_from NULL
 * means 1 for every request (every position but the last is scored).  score_from[r] == n, and so every one-token request, gives no
 * record.  With Q3_SCORE_PREFIX the tokens are suffixes behind the resident prefix, as for q3_embed_many; the first suffix token is
 * never a target.  out may be NULL only if the call produces no record.
 * Standard: target and sum are bit-identical to the numbers above formed on the host, expf glibc's, from the logits of
 * q3_forward(t[i], i) after q3_prefill(t[0 .. i)) on a fresh single-stream engine of the same context; argmax is equal; max is equal
 * as a float value (a maximum that is a zero may carry either sign; sum does not depend on which).  A row that holds a NaN logit is
 * outside the standard; the call does not fault on it.  The values do not depend on the slot, the wave, the neighbours, the chunk a
 * column lands in or score_from.
 * Schedule: waves, blocks, runs, slots and the prefix copy are exactly those of q3_embed_many.  Behind each block, the block's scored
 * columns -- live columns whose token has a successor in its request at or behind score_from -- are cut in column order into chunks
 * of up to 32; a chunk of m columns runs k_score_gather (not for a block of 32 columns or fewer whose column j is the chunk's row
 * j: it stands in the scratch already), the two classifier launches of the column plan of the narrowest width that holds m (columns
 * m and up repeat the last one), k_score_exp and k_score_sum.  Pads and unscored columns cost no classifier work; a block with no
 * scored column launches nothing behind its layers.  stats (may be NULL): q3_embed_stats' four, chunks = the sum over the blocks of
 * ceil(scored columns / 32), scored = the number of records: pure functions of the lengths and score_from (q3_score_pack).
 * Execution: everything on the engine's stream, then ONE device-to-host copy of the records and ONE synchronisation.  The table of
 * scored columns and the records belong to the batched state: grown on demand (the stream is waited for first), released with
 * it.  The exps of a chunk (32 rows of vocab_size floats, up to a multiple of 4) are made once, by the first call or the first plan
 * with records of section 2o, whichever comes first, and never replaced.  No slot rng is touched; no kept plan or graph is rebuilt.  THE SLOTS ARE OVERWRITTEN FROM SLOT 0 UP, as
 * by q3_embed_many.  Every failing call leaves the engine usable.
 * Q3_ERR_ARG: everything q3_embed_many refuses (out_dim aside; a null engine before anything touches the GPU); a score_from entry
 * outside [1, prompt_len[r]]; a null out with records to write; unknown flag bits.
 * Q3_ERR_UNSUPPORTED: what q3_embed_many refuses (a Q3_FLAG_FAST engine). */
int q3_score_many(q3_engine* e, const int32_t* prompts /* concatenated */, const size_t* prompt_len, size_t n_requests,
                  const size_t* score_from /* [n_requests] or NULL = all 1 */, uint32_t flags,
                  q3_score_rec* out /* host, concatenated */, q3_score_stats* stats);

/* The schedule of q3_score_many without an engine or a GPU: stats as that call fills them for max_streams slots and blocks of
 * block_cap columns (q3_dense_pack's rule per wave).  Q3_ERR_ARG: what q3_score_many refuses of the lengths and score_from;
 * max_streams outside 1..32; a block_cap q3_dense_pack refuses. */
int q3_score_pack(const size_t* prompt_len, size_t n_requests, const size_t* score_from /* or NULL */, int max_streams, int block_cap,
                  q3_score_stats* stats);

/* ------------------------------------------------------------------------------------------------
 * 2m. (behind 2l so that the earlier sections stay as they were.)  Top-k log-probabilities: beside the record of section 2l, the k
 * most likely tokens of every scored position with their logits (the top_logprobs of completion APIs, distillation targets, "what
 * did the model expect here instead") and the rank of the token that came (top-k accuracy, MRR, filtering by surprise).  The rows
 * l[0 .. V) are those of section 2l, standing behind the classifier launch of every chunk; two more kernels select from them
 * (csrc/q3_score_top.h).
 * THE ORDER.  The key of entry i of a row is
 *     key(i) = ((uint64)total_order_key(l[i]) << 32) | i
 * with total_order_key the unsigned image of f32::total_cmp: the key the classifier leaves per workgroup in the argmax slots.
 *     top[0 .. k)  the entries of the k largest keys, largest first, as {l[i], i}
 *     rank         the number of entries whose key exceeds key(target): 0 means the target is the argmax
 * So ties in the logit go to the HIGHER index, as for argmax ("the last index of the maximum in total order"), -0.0 sorts below
 * +0.0, top[0].index == argmax, and rank < k exactly when the target is top[rank].  Keys are distinct integers: the result does not
 * depend on how a row is split over workgroups, and there is no tolerance anywhere.  As in 2l nothing is normalised on the device:
 * log P(top[j]) = (top[j].logit - max) - log(sum) with the record's max and sum (generation.top_logprobs_of, in float64).
 * ------------------------------------------------------------------------------------------------ */
#define Q3_SCORE_TOP_MAX 64
typedef struct q3_score_top { float logit; int32_t index; } q3_score_top;

/* q3_score_many with the k best and the rank of every record: top[j] of record i stands in top[i k + j], its rank in rank[i] (rank
 * may be NULL: no rank is copied back).  Records, schedule, stats, slots, the prefix flag and the refusals are exactly those of
 * q3_score_many, and q3_score_pack describes both calls.  1 <= k <= Q3_SCORE_TOP_MAX and k <= vocab_size.
 * Standard: out as for q3_score_many, bit for bit what that call gives on the same engine.  top[j].logit is bit-identical to
 * logits[top[j].index] of the q3_forward named there; the indices and the rank are equal to those of a host sort of that row's
 * keys.  A row that holds a NaN logit is outside the standard; the call does not fault on it: only loop indices, counters and the
 * host-checked table entries become addresses, no logit and no key read back from memory.
 * Schedule: every chunk runs, behind k_score_sum, k_score_top_part -- grid (parts, m): the k largest keys of one slice of a row,
 * sorted, by k rounds of a workgroup-wide maximum, and the slice's count of keys above the target's -- and k_score_top_merge -- one
 * workgroup per row copies the parts' lists into LDS, and one wave of it merges them and sums the counts.  parts is 64 (the
 * developer build reads Q3_SCORE_TOP_PARTS, 1 .. 64, in every call: another split, the same results).
 * Execution: as q3_score_many, with up to two more device-to-host copies in front of the ONE synchronisation: the tops and, if
 * asked for, the ranks.  The tops and the ranks belong to the batched state: grown on demand (the stream is waited for first),
 * released with it.  The parts' lists and counts of a chunk are made by the first call with k > 0 at their full size ([32][64][64]
 * keys, [32][64] counts, about 1 MiB), never replaced, and shared with the plans with records of section 2o.  No slot rng is touched; no kept plan or graph is rebuilt.  Every failing call
 * leaves the engine usable.
 * Q3_ERR_ARG: k outside 1 .. Q3_SCORE_TOP_MAX (checked first, with the null engine, before anything touches the GPU); everything
 * q3_score_many refuses; k > vocab_size; a null top with records to write.
 * Q3_ERR_UNSUPPORTED: what q3_score_many refuses. */
int q3_score_top_many(q3_engine* e, const int32_t* prompts /* concatenated */, const size_t* prompt_len, size_t n_requests,
                      const size_t* score_from /* [n_requests] or NULL = all 1 */, uint32_t flags, int k,
                      q3_score_rec* out /* host, concatenated */, q3_score_top* top /* host, [records][k] */,
                      int32_t* rank /* host, [records], or NULL */, q3_score_stats* stats);

/* ------------------------------------------------------------------------------------------------
 * 2n. (behind 2m so that the earlier sections stay as they were.)  Top-k sampling: every draw the engine makes at temperature > 0 is
 * taken among the k most likely tokens (the model cards' third sampling setting, beside temperature and top-p).
 * THE RULE.  A draw with top_k = k, 1 <= k <= Q3_TOP_K_MAX, is Sampler::sample (sampler.rs:118-139) applied to the logits with
 * every entry outside the SURVIVOR SET replaced by -inf.  The survivors are the entries of the k largest keys of section 2m,
 *     key(i) = ((uint64)total_order_key(l[i]) << 32) | i,
 * so equal logits go to the HIGHER index, as for the argmax, and k = 1 leaves the argmax.  The rest follows from the masking, bit
 * for bit: the softmax maximum is the scaled top survivor; e = expf(l / T - max) per survivor; the denominator is the sequential
 * f32 sum from -0.0 over the survivors in ascending token index (a masked entry adds an exact zero); p = e * (1 / sum); ONE
 * xorshift64* coin per draw, so the rng advances exactly as without top-k.  0 < topp < 1: the cutoff is (1 - topp) / (V - 1) with
 * the FULL vocabulary size V, the survivors with p >= cutoff are sorted by (probability descending, index ascending), and the
 * cumulative sum and the cdf walk are sequential.  Otherwise: a sequential cdf over the survivors in ascending index.
 * One deviation: a multinomial walk whose f32 cdf ends below the coin (37 equal survivors end at 0.9999998) returns the
 * highest-index SURVIVOR; the masked reference returns index V - 1, which is masked.
 * At temperature 0 top_k is ignored: argmax, no coin.  A discarded prompt-position draw consumes its coin and selects nothing; a
 * temperature-0 slot inside a sampled column pass takes the argmax: both as without top-k.  A NaN logit is outside the standard
 * and harmless: no value read back from memory becomes an address, and the drawn index is clamped to the vocabulary.
 * What runs (csrc/q3_topk.h).  k_sample_exp, k_sample and the chip-wide passes of a draw are replaced by two launches: k_topk_part
 * -- grid (64 slices, columns), the k largest keys of every slice, section 2m's selection -- and k_topk_draw -- one wave per
 * column merges the lists and draws.  On / off is a property of the plan (a second form of every sampled plan, built on first
 * use); the value of k stands in device memory and is read when a pass runs.  top_k = 0: every entry point launches exactly what
 * it launched before this section existed.
 * ------------------------------------------------------------------------------------------------ */
#define Q3_TOP_K_MAX 64   /* = Q3_SCORE_TOP_MAX */

/* The engine-wide top_k, default 0 = off.  It holds for every draw at temperature > 0 of every entry point: q3_forward_sample,
 * q3_generate_sampled, the last position of q3_prefill / q3_prefill_batched; q3_forward_batch / q3_generate_greedy_batch under
 * q3_batch_sampler_set; q3_verify_draw, q3_generate_lookup_draw, q3_batch_step_cols_draw, q3_generate_many_sampled and the
 * sampled forms of q3_generate_many_dense / _stop / _prefix.  It is independent of q3_sampler_set, q3_batch_sampler_set and
 * q3_batch_init and survives all of them and every q3_generate_many_* call.
 * Execution: waits for the stream; the first k > 0 allocates the k word and the slices' lists (32 columns x 64 x 64 keys, 1 MiB).
 * Changing k between two non-zero values rebuilds and recaptures nothing; switching between 0 and k > 0 selects the other form
 * of the plans (the one step plan of section 2b is rebuilt on its next use, the kept column plans of both forms stay).
 * Q3_ERR_ARG: null engine; top_k < 0, > Q3_TOP_K_MAX or > vocab_size. */
int q3_sampler_top_k(q3_engine* e, int top_k);
int q3_sampler_get_top_k(const q3_engine* e, int* top_k);

/* q3_op_sample among the top_k largest logits: one draw by the rule above on a host vector.  Arguments and refusals of
 * q3_op_sample, and Q3_ERR_ARG for top_k outside 1 .. Q3_TOP_K_MAX or > n (0 is an error here: that draw is q3_op_sample). */
int q3_op_sample_top_k(const float* logits, size_t n, float temperature, float topp, int top_k, uint64_t* rng_state, int32_t* index, int device);

/* ------------------------------------------------------------------------------------------------
 * 2o. (behind 2n so that the earlier sections stay as they were.)  Log-probabilities of GENERATED tokens: the records of section 2l,
 * and with top_n > 0 the tops and ranks of section 2m, for every token the five q3_generate_many_* loops produce, taken inside the
 * loop (completion-API logprobs / top_logprobs, best-of-n by sequence likelihood, confidence filtering, distillation targets from
 * sampled text).  Without it a caller sends prompt + output back through q3_score_many: a second pass over the weights.
 * THE RULE.  Token out_tokens[o] of a call was taken from a row of logits l[0 .. V): the classifier row of the column whose
 * ColEnt::out == o.  Record o is section 2l's record of that row with target = out_tokens[o]: {l[target], max, sum, argmax};
 * top[o top_n ..] and rank[o] are section 2m's values for the same row and target.  The records are taken on the RAW logits:
 * temperature 1, the full vocabulary, in front of top-k and top-p -- the numbers q3_score_many gives, not the sampler's rescaled
 * distribution.  Nothing is normalised on the device (generation.logprobs_of / top_logprobs_of form log P in float64).  Under
 * q3_generate_many_stop / _prefix the entries at or behind n_out[r] of a request are all-zero bytes.  Dense blocks and
 * prompt-interior columns form no record.
 * Standard (no tolerance anywhere): tokens, cache rows and rng states are bit-identical to the same call with the setting off.  The
 * records of request r equal what q3_score_many gives for the sequence prompt_r + tokens_r with score_from[r] = prompt_len[r] (with
 * Q3_SCORE_PREFIX: the suffixes): target and sum by bits, argmax equal, max by value; top and rank equal those of q3_score_top_many
 * on the same input.  On a greedy request and on a temperature-0 request argmax == token, rank == 0 and bits(target) == bits(max).
 * A row that holds a NaN is outside the standard and does not fault: the target index used as an address is the committed token
 * clamped to [0, V); no logit and no key read back from memory becomes an address.
 * What runs (csrc/q3_genlp.h).  A third axis on the column plans -- off, records, records + top -- built on first use; the existing
 * forms and their graphs are untouched, and at -1 every entry point launches exactly what it launched before this section existed.
 * With records, behind the draws of a sampled plan and in front of the turn kernel: k_score_exp (grid 64 x width) and k_score_sum
 * (grid width), the kernels of section 2l themselves with their row source -- there a host table -- replaced by what the device
 * knows (PassRows): row j is column j of the pass, columns past the pass's live ones or with out < 0 return at once, the target is
 * the token the turn kernel commits (one device function both call).  With top_n > 0 also k_score_top_part (grid 64 x width) and
 * k_score_top_merge (grid width), section 2m's selection.  The exps and the parts' lists are the scratch of sections 2l and 2m,
 * one allocation of fixed size per batched state that no call replaces.  The value of top_n and the destinations stand in a control block in device memory, uploaded once per call and read
 * when a pass runs: 1 and 64 share every plan and graph.
 * IT DOES NOT TOUCH q3_batch_step_cols[_draw], section 2b (q3_forward_batch, q3_generate_greedy_batch), the verify paths or
 * single-stream decode: none of them forms a record under any setting.  A single-stream caller runs q3_generate_many_* with one
 * request.
 * ------------------------------------------------------------------------------------------------ */

/* The engine-wide setting: -1 = off (default).  0: one q3_score_rec per generated token.  1 .. Q3_SCORE_TOP_MAX: also the top_n best
 * and the rank.  It holds for q3_generate_many_greedy, _sampled, _dense, _stop and _prefix, and survives q3_sampler_set,
 * q3_batch_sampler_set, q3_batch_init and every generate call.
 * Execution: waits for the stream.  The first value >= 0 allocates the control block in the batched state; with no batched state yet,
 * the first generate call under the setting does.  The exps and the parts' lists are the scratch of sections 2l and 2m, made when
 * the first plan with records is built if no score call has made them.  Switching the value rebuilds no kept plan: the plans of each of the three forms stay.
 * Q3_ERR_ARG: top_n < -1 or > Q3_SCORE_TOP_MAX (checked first, then the null engine, before anything touches the GPU); top_n >
 * vocab_size.  A failing call leaves the engine usable and the setting as it was. */
int q3_gen_logprobs(q3_engine* e, int top_n);
int q3_gen_logprobs_get(const q3_engine* e, int* top_n);

/* Records first .. first + count - 1 of the LAST q3_generate_many_* call, indexed exactly as its out_tokens; top is [count][top_n]
 * with the top_n that call ran under (NULL only if that was 0), rank [count] or NULL (with top_n 0 nothing is written to either).
 * Execution: up to three device-to-host copies and ONE synchronisation.  The generate calls keep their synchronisation counts (one
 * per call; one per pass in the stop loop): the per-call buffers (records, tops, ranks, each as long as out_tokens) belong to the
 * batched state, are grown behind the call's existing synchronisation, cleared on the stream in front of the first pass and released
 * with the state.  Results stay valid until the next q3_generate_many_* call, q3_batch_init or q3_destroy.
 * Q3_ERR_ARG: a null engine; no q3_generate_many_* call has run with the setting on since q3_batch_init, or the last one ran with
 * it off or failed; first + count past that call's total of n_new; null recs; null top while that call's top_n > 0. */
int q3_gen_logprobs_read(q3_engine* e, size_t first, size_t count, q3_score_rec* recs, q3_score_top* top /* [count][top_n] or NULL */,
                         int32_t* rank /* [count] or NULL */);

/* ------------------------------------------------------------------------------------------------
 * 2p. (behind 2o so that the earlier sections stay as they were.)  Presence and frequency penalties: a token becomes less likely
 * because its request has already produced it (presence_penalty / frequency_penalty of the completion APIs, the remedy for endless
 * repetition), inside the five q3_generate_many_* loops, where no logit reaches the host.
 * THE RULE.  Request r has produced y_0 .. y_{j-1}; its next token y_j is taken from a classifier row l[0 .. V).  c[v] is the number
 * of i < j with y_i == v: prompt tokens, a shared prefix and other requests' tokens do not count.  The PENALISED row is
 *     c[v] == 0:  l'[v] = l[v]                                          (the same bits, -0.0 and NaN payloads included)
 *     c[v] >  0:  l'[v] = l[v] - (presence + frequency * (float)c[v])
 * with every operation of the second line rounded to f32 on its own: multiply, then add, then subtract, nothing fused.  y_j is what
 * the engine takes from l without the setting, taken from l' instead: in a greedy call and for a temperature-0 request the index of
 * the largest key ((uint64)total_order_key(l'[v]) << 32) | v, so equal values go to the HIGHER index; otherwise Sampler::sample, or
 * section 2n's draw among the top_k, over l' -- the softmax maximum is the largest penalised value, and the penalties come in front of
 * temperature, top-k and top-p.  ONE coin per draw as before: the rng advances exactly as without penalties.  y_0 is taken from the raw
 * row: all counts are zero.  The stop decision, the schedule, the cache rows and the coins of discarded prompt positions are unchanged.
 * SECTION 2o's RECORDS STAY ON THE RAW ROW l: under penalties the records of a call still equal q3_score_many on prompt + output, but
 * "argmax == token, rank == 0, bits(target) == bits(max)" of a greedy or temperature-0 request NO LONGER HOLD in general -- the
 * committed token is the argmax of l', the record's argmax that of l.
 * A NaN logit is outside the standard and harmless: only loop indices, ColEnt::out, slot numbers and the committed token clamped to
 * [0, V) become addresses.
 * What runs (csrc/q3_penalty.h).  A fourth axis on the column plans, built on first use; the existing forms and their graphs are
 * untouched, and at (0, 0) every entry point launches exactly what it launched before this section existed.  Behind the classifier:
 * k_pen_apply -- grid (64 slices, width): l' of every emitting column into a buffer of its own (the classifier's output is never
 * written) and the largest key of every slice; a column that emits nothing leaves key 0 and returns.  Sampled plans fold those keys
 * (k_spec_colmax) and draw over l'; the records, if any, follow on the raw rows; k_pen_count -- one workgroup -- adds the token about
 * to be committed to its KV slot's counts; the turn kernel of a greedy plan folds the slices' keys in place of the classifier's.
 * The column that emits a request's first token (the emitting column fed from the prompt) copies its row and clears its slot's counts.
 * The values stand in device memory and are read when a pass runs: two non-zero settings share every plan and graph.
 * IT DOES NOT TOUCH q3_batch_step_cols[_draw], section 2b, the verify paths or single-stream decode; a single-stream caller runs
 * q3_generate_many_* with one request.  The setting is engine-wide: no per-request values, no penalty over the prompt.
 * ------------------------------------------------------------------------------------------------ */

/* The engine-wide setting, default (0, 0) = off.  It holds for every token q3_generate_many_greedy, _sampled, _dense, _stop and
 * _prefix produce, greedy and sampled, and survives q3_sampler_set, q3_batch_sampler_set, q3_batch_init, q3_sampler_top_k,
 * q3_gen_logprobs and every generate call.
 * Execution: waits for the stream.  The first non-zero setting allocates the penalty state in the batched state -- counts
 * [max_streams][V] u32, penalised rows [32][V] f32, slice keys [32][64] and the two values, about 39 MB at V = 151,936 and 32 slots,
 * released with the state; with no batched state yet, the first generate call under the setting does.  Changing between two non-zero
 * settings rebuilds and recaptures nothing; switching between (0, 0) and a non-zero setting selects the other form of the kept plans.
 * Q3_ERR_ARG: a value that is not finite or lies outside [-2, 2] (checked first, then the null engine, before anything touches the
 * GPU).  A refused call changes nothing. */
int q3_sampler_penalties(q3_engine* e, float presence, float frequency);
int q3_sampler_get_penalties(const q3_engine* e, float* presence, float* frequency);

/* The rule above on a host vector: k_pen_apply once over logits[0 .. n) and counts[0 .. n).  out receives l', argmax the index of the
 * largest key of l'.  Q3_ERR_ARG (before anything touches the GPU): the values as above; a null pointer; n == 0 or n >= 2^31. */
int q3_op_penalize(const float* logits, const uint32_t* counts, size_t n, float presence, float frequency, float* out /* [n] */, int32_t* argmax,
                   int device);

/* ------------------------------------------------------------------------------------------------
 * 2q. (behind 2p so that the earlier sections stay as they were.)  Logit bias, banned and allowed tokens, min_tokens: the caller
 * constrains which tokens may come (logit_bias, bad_words, allowed_token_ids or guided choice, min_tokens of the completion APIs),
 * inside the five q3_generate_many_* loops, where no logit reaches the host and a request's next column depends on the token it just
 * committed.
 * THE RULE.  Request r is about to produce its output y_g (g = 0: the token behind the prompt) from classifier row l[0 .. V).  It has
 * a list of at most Q3_BIAS_MAX entries with distinct tokens, and a mode.  An entry is ACTIVE for y_g when until == 0 || g < until.
 * The ADJUSTED row is
 *     v listed, active, bias +-0:     a[v] = l[v]            (the same bits)
 *     v listed, active, otherwise:    a[v] = l[v] + bias     (one f32 rounding; bias -inf gives -inf)
 *     v listed, not active:           a[v] = l[v]            (the same bits, under both modes)
 *     v unlisted, Q3_BIAS_ADD:        a[v] = l[v]            (the same bits, -0.0 and NaN payloads included)
 *     v unlisted, Q3_BIAS_ALLOW:      a[v] = -inf            (bits 0xFF800000)
 * Section 2p's penalties, if set, then apply to a in place of l: c[v] > 0 gives a[v] - (presence + frequency * c[v]) with the same
 * three roundings, c[v] == 0 the bits of a[v].  Everything downstream takes this row exactly as section 2p defines it for l': greedy
 * and temperature-0 requests the largest key ((uint64)total_order_key << 32) | v, so equal values go to the HIGHER index; sampled
 * requests Sampler::sample, or section 2n's draw among the top_k, over it -- one coin per draw, the softmax maximum the largest
 * adjusted value.  Unlike the penalties THE RULE APPLIES TO y_0 TOO.  The stop decision, the schedule, the cache rows and the coins of
 * discarded prompt positions are unchanged.  SECTION 2o's RECORDS STAY ON THE RAW ROW l, as under 2p: the record's target is the
 * committed token, its log-probability, argmax and rank are those of the unconstrained distribution.
 * min_tokens needs nothing of the scheduler: a stop token carried as {eos, -inf, until = min_tokens} cannot be committed for
 * g < min_tokens, so the stop rule never sees it.
 * A BANNED TOKEN has probability exactly 0 under the sampler (exp(-inf - max) == 0).  The reference sampler's fall-through -- index
 * n - 1, or the last index of the nucleus, when rounding leaves the coin above the cumulative sum -- is kept as it is: the standard
 * is bit-equality with q3_op_sample / q3_op_sample_top_k on the adjusted row, not "a banned token can never appear".
 * +inf + (-inf) is NaN.  A NaN logit is outside the standard and harmless, as in 2p: only loop indices, ColsCtl::out, slot numbers,
 * request and entry indices clamped to their arrays and the committed token clamped to [0, V) become addresses.
 * What runs (csrc/q3_bias.h).  One more form on the fourth axis of the column plans (off / penalties / adjusted), built on first use.
 * k_bias_apply stands where k_pen_apply stands, with its grid (64 slices, width), its row buffer and its slice keys, so the turn
 * kernels, k_spec_colmax, the sampler and the top-k selection run as under penalties.  A column learns its request and g from
 * ColsCtl::out[j] == o_off[r] + g by a search over the call's o_off; a slice whose part of the list is empty copies.  Whether
 * penalties apply on top is read from device memory when a pass runs; without them no counts array is allocated or read.  The lists,
 * their offsets, the modes and o_off are uploaded by every generate call under a table: two tables share every plan and graph.  With
 * no table set every entry point launches exactly what it launched before this section existed.
 * IT DOES NOT TOUCH q3_batch_step_cols[_draw], section 2b, the verify paths, single-stream decode, q3_embed_many, q3_choice_many,
 * q3_score_many or q3_score_top_many.
 * ------------------------------------------------------------------------------------------------ */
typedef struct q3_bias_entry { int32_t token; float bias; uint32_t until; } q3_bias_entry;
#define Q3_BIAS_MAX   4096
#define Q3_BIAS_ADD   0
#define Q3_BIAS_ALLOW 1

/* The engine-wide table, default none = off.  n_lists == 0 turns it off; n_lists == 1: the one list holds for every request of every
 * call; n_lists > 1: list r belongs to request r, and a q3_generate_many_* call whose n_requests != n_lists returns Q3_ERR_ARG before
 * anything runs.  entries: the lists one behind the other, list i of n_entries[i] entries in any order (the library keeps a copy,
 * sorted by token).  mode: per list, or NULL for Q3_BIAS_ADD throughout.  The table holds for every token q3_generate_many_greedy,
 * _sampled, _dense, _stop and _prefix produce, and survives q3_sampler_set, q3_batch_sampler_set, q3_batch_init, q3_sampler_top_k,
 * q3_gen_logprobs, q3_sampler_penalties and every generate call.
 * Execution: waits for the stream; the device side is made by the first generate call under a table.
 * Q3_ERR_ARG, checked before the engine or the GPU is touched: a null array with a non-zero count; a list longer than Q3_BIAS_MAX; a
 * token twice in one list; a negative token; a bias that is NaN, +inf, or finite outside [-100, 100]; a mode other than 0 or 1; an
 * ALLOW list with no finite-bias entry.  Then the null engine, then what needs the model: a token >= vocab_size; an ADD list whose
 * -inf entries number >= vocab_size.  A refused call changes nothing. */
int q3_logit_bias_set(q3_engine* e, const q3_bias_entry* entries /* concatenated */, const size_t* n_entries /* [n_lists] */,
                      const uint8_t* mode /* [n_lists] or NULL: all ADD */, size_t n_lists);
int q3_logit_bias_get(const q3_engine* e, size_t* n_lists, size_t* n_entries_total);

/* The rule above on a host vector: k_bias_apply once over logits[0 .. n) for output index g of a request with the one list given,
 * then the penalties over counts[0 .. n) where counts is not NULL.  out receives the row, argmax the index of its largest key.
 * Q3_ERR_ARG (before anything touches the GPU): the list as above with vocab_size n; the penalty values as in 2p; a null pointer;
 * n == 0 or n >= 2^31. */
int q3_op_logit_bias(const float* logits, size_t n, const q3_bias_entry* entries, size_t n_entries, int mode, uint32_t g,
                     const uint32_t* counts /* or NULL: no penalties */, float presence, float frequency, float* out /* [n] */, int32_t* argmax,
                     int device);

/* ------------------------------------------------------------------------------------------------
 * 2r. (behind 2q so that the earlier sections stay as they were.)  Guided decoding: a constraint that changes with what the request
 * has produced so far -- one of several multi-token labels, a regular expression, a fixed JSON skeleton, multi-token banned
 * sequences -- as a token automaton whose state lives on the device beside the KV slot and advances where the token is committed,
 * inside the five q3_generate_many_* loops.
 * THE RULE.  A GUIDE is a table next[n_states][V] of int16_t: next[s][v] >= 0, in state s token v may come and leads to that state;
 * -1, it may not; and a list start[].  Request r is about to produce y_g from classifier row l[0 .. V):
 *     start state   s_0 = start[r], or start[0] where there is one entry.  s_0 == -1: the request is unguided, its row is l and it
 *                   advances no state.
 *     masked row    m[v] = l[v] (the same bits) where next[s_g][v] >= 0, bits 0xFF800000 (-inf) otherwise.
 *     bias          section 2q's table, if set, applies to m in place of l; section 2p's penalties on top, exactly as there.
 *     downstream    everything downstream takes that row as 2q defines it: greedy and temperature-0 requests the largest key, equal
 *                   values to the HIGHER index; sampled requests Sampler::sample or section 2n's draw among the top_k; one coin per
 *                   draw.
 *     state step    after the commit s_{g+1} = next[s_g][y_g] where that is >= 0, else s_g.
 * THE ELSE BRANCH OF THE STATE STEP IS REACHABLE: the sampler's fall-through (2q: index n - 1 ... is kept as it is) and a row with
 * no finite entry -- a bias table that bans a state's only tokens, the caller's mistake, under greedy it commits V - 1 by the key
 * rule -- can commit a token the state forbids.  The state then stays.  Only indices clamped to their arrays become addresses.
 * As in 2q THE RULE HOLDS FOR y_0 TOO, SECTION 2o's RECORDS STAY ON THE RAW ROW l with the committed token as target, and the stop
 * decision, the schedule, the cache rows and the coins of discarded prompt positions are unchanged.  Termination stays with the
 * stop tokens: an automaton that wants to end lets EOS through in its accepting states.
 * What runs (csrc/q3_guide.h).  One more form on the fourth axis of the column plans (off / penalties / adjusted / masked), chosen
 * whenever a guide is set, whatever the table and the penalties, built on first use.  k_guide_apply stands where k_bias_apply
 * stands, with its grid, slices and outputs: it reads the state -- start[r] where g == 0, else the KV slot's -- streams the state's
 * row of the table beside the logits, then applies 2q and 2p as k_bias_apply does (with no table: one empty ADD list).
 * k_guide_step stands where k_bias_count stands: it writes the slot's next state from the token about to be committed, starting
 * from start[r] for g == 0 so that a reused slot needs no reset, then counts where penalties are set.  The table goes to the device
 * once per q3_guide_set (and again after q3_batch_init), at the first generate call under it; start[] and a control block go with
 * every call.  The plans point at the control block: two guides share every plan and graph.  With no guide set every entry point
 * launches exactly what it launched before this section existed.
 * IT DOES NOT TOUCH q3_batch_step_cols[_draw], section 2b, the verify paths, single-stream decode, q3_embed_many, q3_choice_many,
 * q3_score_many or q3_score_top_many.
 * ------------------------------------------------------------------------------------------------ */
#define Q3_GUIDE_MAX_STATES 4096

/* The engine-wide guide, default none = off.  n_states == 0 turns it off.  n_start == 1: every request of every call starts in
 * start[0]; n_start > 1: request r starts in start[r], and a q3_generate_many_* call whose n_requests != n_start returns Q3_ERR_ARG
 * before anything runs.  The library keeps a copy of both arrays.  The guide holds for every token q3_generate_many_greedy,
 * _sampled, _dense, _stop and _prefix produce, and survives q3_sampler_set, q3_batch_sampler_set, q3_batch_init, q3_sampler_top_k,
 * q3_gen_logprobs, q3_sampler_penalties, q3_logit_bias_set and every generate call.
 * Execution: waits for the stream; the device side is made by the first generate call under a guide.
 * Q3_ERR_ARG, checked before the engine or the GPU is touched: a null array with a non-zero count; n_states > Q3_GUIDE_MAX_STATES;
 * n_start == 0 with states; a start outside [-1, n_states); an entry of next outside [-1, n_states); a state whose row allows no
 * token; vocab == 0 or vocab >= 2^31.  Then the null engine, then vocab != vocab_size.  A refused call changes nothing. */
int q3_guide_set(q3_engine* e, const int16_t* next /* [n_states][vocab] */, size_t n_states, size_t vocab,
                 const int32_t* start /* [n_start] */, size_t n_start);
int q3_guide_get(const q3_engine* e, size_t* n_states, size_t* n_start);

/* The rule above on a host vector: k_guide_apply once over logits[0 .. n) for a request in the state whose row of the table is
 * next_row[0 .. n), at output index g with the one list given (n_entries == 0: none), then the penalties over counts[0 .. n) where
 * counts is not NULL.  out receives the row, argmax the index of its largest key.  Q3_ERR_ARG (before anything touches the GPU):
 * what q3_op_logit_bias refuses, and a null next_row. */
int q3_op_guide(const float* logits, size_t n, const int16_t* next_row /* [n] */, const q3_bias_entry* entries, size_t n_entries,
                int mode, uint32_t g, const uint32_t* counts /* or NULL: no penalties */, float presence, float frequency, float* out /* [n] */,
                int32_t* argmax, int device);

/* ------------------------------------------------------------------------------------------------
 * 2s. (behind 2r so that the earlier sections stay as they were.)  Sparse guides: section 2r's guide on a compressed table, for
 * automata whose dense table does not fit -- one dense state costs 2 V bytes, 304 KB at V = 151,936, and a dense state number ends
 * at 32,767 -- such as the lift of a regular expression to the tokens of a real vocabulary.
 * THE RULE IS 2r's, UNCHANGED: the masked row with 0xFF800000 (-inf) for forbidden tokens, 2q's table on m in place of l, 2p's
 * penalties on top, the state step s_{g+1} = next[s_g][y_g] where that is >= 0, else s_g, start[r] == -1 for an unguided request,
 * y_0 under the rule too, section 2o's records on the RAW ROW l, and the stop decision, the schedule, the cache rows and the coins
 * untouched.  ONLY THE STATEMENT OF next[s][v] CHANGES:
 *     dflt[n_states]          int32_t: what every unlisted token does in state s: -1 forbidden, otherwise the state it leads to.
 *     row_off[n_states + 1]   uint32_t: state s owns edges[row_off[s] .. row_off[s + 1]).
 *     edges[n_edges]          q3_guide_edge { token, next }: within a state the tokens ascend strictly; next is -1 or a state.
 *     next[s][v]              the edge's next where v is listed in state s, else dflt[s].
 * ONE GUIDE HOLDS AT A TIME: setting either form clears the other, q3_guide_set(e, NULL, 0, 0, NULL, 0) clears both, and so does
 * q3_guide_set_sparse with n_states == 0.  q3_guide_get answers for the dense form alone and reads 0, 0 under a sparse guide;
 * q3_guide_get_sparse reads 0, 0, 0 under a dense one.
 * What runs (csrc/q3_guide_sparse.h).  A fifth form on the fourth axis of the column plans, chosen whenever a sparse guide is set.
 * k_guide_sp_apply stands where k_guide_apply stands, with its grid, slices and outputs: the workgroup finds its slice's part of
 * the state's edges by two searches; where that is empty the allowed bit is dflt[s] >= 0 for the whole slice and nothing more is
 * read; otherwise a byte per token in LDS takes the default, the slice's edges stream over it, and the logits stream with the byte
 * beside them -- 8 V + 8 E_s bytes per emitting column, E_s the state's edges, against 2r's 10 V.  k_guide_sp_step stands where
 * k_guide_step stands: one search of the state's edges for the committed token, else dflt.  The arrays go to the device once per
 * q3_guide_set_sparse (and again after q3_batch_init), at the first generate call under it; start[] and a control block go with
 * every call; two sparse guides share every plan and graph.  The kernels and plans of 2r, 2q and 2p are as they were, and with no
 * sparse guide set every entry point launches exactly what it launched before this section existed.
 * IT DOES NOT TOUCH q3_batch_step_cols[_draw], section 2b, the verify paths, single-stream decode, q3_embed_many, q3_choice_many,
 * q3_score_many or q3_score_top_many.
 * ------------------------------------------------------------------------------------------------ */
#define Q3_GUIDE_SPARSE_MAX_STATES 1048576
#define Q3_GUIDE_SPARSE_MAX_EDGES 134217728
typedef struct q3_guide_edge { int32_t token; int32_t next; } q3_guide_edge;

/* The engine-wide sparse guide; start[], n_start, what it holds for and what it survives are q3_guide_set's.  The library keeps a
 * copy of the arrays.  Execution: waits for the stream; the device side is made by the first generate call under the guide.
 * Q3_ERR_ARG, checked before the engine or the GPU is touched: a null array with a non-zero count; n_states >
 * Q3_GUIDE_SPARSE_MAX_STATES; n_edges > Q3_GUIDE_SPARSE_MAX_EDGES; n_start == 0 with states; vocab == 0 or vocab >= 2^31; a start,
 * a dflt or an edge's next outside [-1, n_states); row_off[0] != 0, an offset below the one before it, row_off[n_states] !=
 * n_edges; an edge's token outside [0, vocab) or not above the token before it in its state; a state that allows no token.  Then
 * the null engine, then vocab != vocab_size.  A refused call changes nothing. */
int q3_guide_set_sparse(q3_engine* e, const int32_t* dflt /* [n_states] */, const uint32_t* row_off /* [n_states + 1] */,
                        const q3_guide_edge* edges /* [n_edges] */, size_t n_states, size_t n_edges, size_t vocab,
                        const int32_t* start /* [n_start] */, size_t n_start);
int q3_guide_get_sparse(const q3_engine* e, size_t* n_states, size_t* n_edges, size_t* n_start);

/* The rule on a host vector: k_guide_sp_apply once over logits[0 .. n) for a request in a state with default dflt and the edges
 * given, at output index g with the one list given, then the penalties where counts is not NULL: q3_op_guide with the state's row
 * in the sparse statement.  Q3_ERR_ARG (before anything touches the GPU): what q3_op_logit_bias refuses; null edges with a count;
 * more edges than logits; a token outside [0, n) or not ascending strictly; dflt or a next outside [-1,
 * Q3_GUIDE_SPARSE_MAX_STATES). */
int q3_op_guide_sparse(const float* logits, size_t n, int32_t dflt, const q3_guide_edge* edges, size_t n_edges, const q3_bias_entry* entries,
                       size_t n_entries, int mode, uint32_t g, const uint32_t* counts /* or NULL: no penalties */, float presence, float frequency,
                       float* out /* [n] */, int32_t* argmax, int device);

/* ------------------------------------------------------------------------------------------------
 * 2t. (behind 2s so that the earlier sections stay as they were.)  Stop sequences: a request ends where the tokens it has produced
 * complete one of several SEQUENCES, as the stop=[...] of a serving API asks -- "\n\n", "Question:", "</answer>" -- where section
 * 2h ends it at a single token.  A STOP AUTOMATON is stated in section 2s's arrays -- dflt[n_states], row_off[n_states + 1],
 * edges[n_edges] of q3_guide_edge, start[n_start], next[s][v] the edge's next where v is listed in state s, else dflt[s] -- and ONLY
 * THE READING OF next[s][v] == -1 CHANGES: here it means "the sequence is complete, and the request ends with this token".
 *     start      request r starts in start[r], or in start[0] where n_start == 1; start[r] == -1: no stop sequences for request r.
 *     step       only GENERATED tokens move the state, y_0 being the first token stepped; prompt tokens and a shared prefix (2i)
 *                never do.  With s_0 = start and x = next[s_g][y_g]: x == -1 ends the request with n_out[r] = g + 1, the
 *                completing token included, as with a stop token; otherwise s_{g+1} = x.
 *     n_emit[r]  the smallest of: the index of the first stop token + 1, the index of the first completing token + 1, n_new[r].
 * Everything section 2h promises holds with this n_emit: the tokens are bit-identical to the loops at the cap, the passes and stats
 * are those of q3_cols_schedule(prompt_len, n_emit), -1 stands behind the last token, no coin is drawn behind the end, and the next
 * occupant of a slot starts from its own start state whatever state the previous occupant left.
 * IT IS INDEPENDENT OF EVERY OTHER ENGINE-WIDE SETTING: logits, cache rows, coins, the records of 2o, penalties (2p), bias and
 * min_tokens (2q) and guides (2r, 2s) are untouched, and a guide and a stop automaton may both be set.  min_tokens of section 2q
 * bans stop TOKENS among a row's first tokens; it does NOT delay a sequence match.
 * HONOURED BY THE TWO LOOPS THAT HAVE A DEVICE SCHEDULER: q3_generate_many_stop, also with n_stop == 0, and
 * q3_generate_many_prefix, which under a stop automaton runs the loop of section 2h also with n_stop == 0.
 * q3_generate_many_greedy, q3_generate_many_sampled and q3_generate_many_dense return exactly n_new tokens by contract and do not
 * read it, as they do not know stop tokens.
 * What runs (csrc/q3_stop_seq.h).  One __host__ __device__ function, stop_seq_next, steps a state: one search of the state's edges for
 * the token, else dflt; the device loop, the host twin below and q3_op_stop_seq all call it.  While a stop automaton is set,
 * k_cols_sched_seq stands where k_cols_sched stands -- one workgroup, one launch per pass, between two passes: it stages the
 * scheduler state and the slots' last tokens in LDS as k_cols_sched does; then thread i < max_streams steps slot i where that slot
 * produced a token in the pass just committed, from the request's start state on its first output and from the slot's stored state
 * otherwise, and sets a per-slot "sequence complete" flag; behind a barrier thread 0 runs the scheduler step, whose rule 5 reads
 * end = g == n_new || stop token || flag.  The searches of the slots run in parallel lanes, log2(E_s) dependent loads each.  The
 * per-slot states live in device memory beside the scheduler state, in a struct of their own.  No plan key, column plan or turn
 * kernel changes and no launch or synchronisation is added per pass.  The arrays go to the device once per q3_stop_seq_set (and
 * again after q3_batch_init), at the first generate call under it; start[] and a control block go with every call.  With no stop
 * automaton set every entry point launches exactly what it launched before this section existed.
 * Only clamped values become addresses: states to [-1, n_states), edge indices to the state's range inside [0, n_edges], the token
 * to [0, vocab).
 * ------------------------------------------------------------------------------------------------ */
#define Q3_STOP_SEQ_MAX_STATES 65536
#define Q3_STOP_SEQ_MAX_EDGES 16777216

/* The engine-wide stop automaton; it survives what q3_guide_set_sparse survives, and n_states == 0 clears it.  The library keeps a
 * copy of the arrays.  Execution: waits for the stream; the device side is made by the first generate call under it.
 * Q3_ERR_ARG, checked before the engine or the GPU is touched, by the code and in the order of q3_guide_set_sparse with the caps
 * above in the place of its own: a null array with a non-zero count; edges without states; n_states > Q3_STOP_SEQ_MAX_STATES;
 * n_edges > Q3_STOP_SEQ_MAX_EDGES; vocab == 0 or vocab >= 2^31; n_start == 0 with states; a start outside [-1, n_states);
 * row_off[0] != 0, an offset below the one before it, row_off[n_states] != n_edges; a dflt outside [-1, n_states); an edge's token
 * outside [0, vocab) or not above the token before it in its state; an edge's next outside [-1, n_states).  NOT refused: a state
 * that allows no token -- dflt[s] == -1 with no edges says that every token completes a sequence there.  Then the null engine,
 * then vocab != vocab_size.  A refused call changes nothing.
 * A q3_generate_many_* call whose number of requests is neither n_start nor meets n_start == 1 is refused (Q3_ERR_ARG). */
int q3_stop_seq_set(q3_engine* e, const int32_t* dflt /* [n_states] */, const uint32_t* row_off /* [n_states + 1] */,
                    const q3_guide_edge* edges /* [n_edges] */, size_t n_states, size_t n_edges, size_t vocab,
                    const int32_t* start /* [n_start] */, size_t n_start);
int q3_stop_seq_get(const q3_engine* e, size_t* n_states, size_t* n_edges, size_t* n_start);

/* q3_cols_schedule_stop under a stop automaton (host only, never touches the GPU): the passes q3_generate_many_stop runs when
 * request r would produce rows[..] and ends at its first stop token or completed sequence.  The host steps the function the device
 * runs, pass by pass.  n_states == 0: q3_cols_schedule_stop, entry for entry.  A token of rows outside [0, vocab) is clamped into it.
 * Q3_ERR_ARG: null rows and the stop-list refusals of q3_cols_schedule_stop; then what q3_stop_seq_set refuses about the arrays; then
 * what q3_cols_schedule rejects; then n_start != 1 && n_start != n_requests. */
int q3_cols_schedule_stop_seq(const size_t* prompt_len, const size_t* n_new, size_t n_requests, int max_streams,
                              const int32_t* rows /* concatenated, n_new[r] each */, const int32_t* stop_tokens, size_t n_stop,
                              const int32_t* dflt, const uint32_t* row_off, const q3_guide_edge* edges, size_t n_states, size_t n_edges,
                              size_t vocab, const int32_t* start, size_t n_start,
                              int32_t* table /* [cap][4]: pass, slot, pos, request */, size_t cap, size_t* n_entries, size_t* n_out,
                              q3_cols_stats* stats);

/* One token stream over the tables, on the host with the step function the kernel calls: from start_state, token after token until
 * one completes a sequence.  *n_emit = the index of the completing token + 1, or n_tokens; *end_state = the state behind the last
 * token stepped, or -1 on a match.  start_state == -1 steps nothing: n_tokens and -1.  A token outside [0, vocab) is clamped into it.
 * Q3_ERR_ARG: what q3_stop_seq_set refuses about the arrays with start_state as the one start; no states; null tokens with a count;
 * a null n_emit or end_state. */
int q3_op_stop_seq(const int32_t* dflt, const uint32_t* row_off, const q3_guide_edge* edges, size_t n_states, size_t n_edges, size_t vocab,
                   int32_t start_state, const int32_t* tokens, size_t n_tokens, size_t* n_emit, int32_t* end_state);

#ifdef __cplusplus
}
#endif
#endif /* QWEN3_HIP_H */
