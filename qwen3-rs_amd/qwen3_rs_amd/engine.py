"""ctypes binding of libqwen3_hip.so (include/qwen3_hip.h) shaped like the reference's Rust API."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from typing import List, Optional, Tuple

import numpy as np

FLAG_FAST = 1
FLAG_NO_GRAPH = 2
FLAG_NO_VALUE_T = 4
# q3_op_gemv_role roles (Q3_ROLE_* of include/qwen3_hip.h)
ROLE_NORM_QKV, ROLE_NORM_SWIGLU, ROLE_QUANT_RESID, ROLE_PREQR_RESID, ROLE_NORM_LOGITS = range(5)

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_DIST_DIR = os.path.dirname(_PKG_DIR)

# every symbol include/qwen3_hip.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = [
    "q3_create", "q3_get_config", "q3_forward", "q3_destroy", "q3_last_error", "q3_forward_argmax",
    "q3_generate_greedy", "q3_host_generate", "q3_host_sample_argmax", "q3_prefill", "q3_reset_kv", "q3_read_state", "q3_batch_init", "q3_forward_batch",
    "q3_generate_greedy_batch", "q3_batch_reset_kv", "q3_batch_read_state", "q3_prefill_batched", "q3_batch_sampler_set", "q3_sampler_set", "q3_sampler_get_rng", "q3_forward_sample", "q3_generate_sampled", "q3_profile", "q3_profile_name", "q3_parse_header",
    "q3_abi_version", "q3_build_id", "q3_op_quantize", "q3_op_dequantize", "q3_op_matmul", "q3_op_rmsnorm", "q3_op_softmax",
    "q3_op_swiglu", "q3_op_expf", "q3_op_attention", "q3_op_argmax", "q3_op_sample", "q3_op_gemv_role",
    "q3_verify", "q3_lookup_draft", "q3_lookup_trace", "q3_generate_lookup",
    "q3_verify_draw", "q3_generate_lookup_draw",
    "q3_batch_step_cols", "q3_cols_schedule", "q3_generate_many_greedy",
    "q3_batch_step_cols_draw", "q3_generate_many_sampled",
    "q3_dense_pack", "q3_batch_prefill_slots", "q3_generate_many_dense",
    "q3_generate_many_stop", "q3_cols_schedule_stop",
    "q3_batch_copy_rows", "q3_batch_prefix_set", "q3_batch_prefix_get", "q3_generate_many_prefix",
    "q3_embed_many",
    "q3_choice_many",
    "q3_score_many", "q3_score_pack",
    "q3_score_top_many",
    "q3_sampler_top_k", "q3_sampler_get_top_k", "q3_op_sample_top_k",
    "q3_gen_logprobs", "q3_gen_logprobs_get", "q3_gen_logprobs_read",
    "q3_sampler_penalties", "q3_sampler_get_penalties", "q3_op_penalize",
    "q3_logit_bias_set", "q3_logit_bias_get", "q3_op_logit_bias",
    "q3_guide_set", "q3_guide_get", "q3_op_guide",
    "q3_guide_set_sparse", "q3_guide_get_sparse", "q3_op_guide_sparse",
    "q3_stop_seq_set", "q3_stop_seq_get", "q3_cols_schedule_stop_seq", "q3_op_stop_seq",
]
GUIDE_MAX_STATES = 4096  # Q3_GUIDE_MAX_STATES (section 2r)
GUIDE_SPARSE_MAX_STATES = 1 << 20   # Q3_GUIDE_SPARSE_MAX_STATES (section 2s)
GUIDE_SPARSE_MAX_EDGES = 1 << 27    # Q3_GUIDE_SPARSE_MAX_EDGES
EDGE_DTYPE = np.dtype([("token", np.int32), ("next", np.int32)])   # q3_guide_edge
STOP_SEQ_MAX_STATES = 1 << 16       # Q3_STOP_SEQ_MAX_STATES (section 2t)
STOP_SEQ_MAX_EDGES = 1 << 24        # Q3_STOP_SEQ_MAX_EDGES
PENALTY_MAX = 2.0        # |presence|, |frequency| <= 2 (section 2p)
BIAS_MAX = 4096          # Q3_BIAS_MAX: entries per list (section 2q)
BIAS_LIMIT = 100.0       # a finite bias lies in -100 .. 100; -inf bans
BIAS_ADD, BIAS_ALLOW = 0, 1
BIAS_DTYPE = np.dtype([("token", np.int32), ("bias", np.float32), ("until", np.uint32)])     # q3_bias_entry
VERIFY_MAX = 32          # Q3_VERIFY_MAX
COLS_MAX = 32            # Q3_COLS_MAX
STOP_MAX = 8             # Q3_STOP_MAX
EMBED_L2, EMBED_PREFIX = 1, 2   # Q3_EMBED_L2, Q3_EMBED_PREFIX
CHOICE_PREFIX, CHOICE_PER_REQUEST = 2, 4   # Q3_CHOICE_PREFIX, Q3_CHOICE_PER_REQUEST
CHOICE_MAX = 256         # Q3_CHOICE_MAX
SCORE_PREFIX = 2         # Q3_SCORE_PREFIX
# q3_score_rec as a numpy record: what Transformer.score_many returns per scored position
SCORE_DTYPE = np.dtype([("target", np.float32), ("max", np.float32), ("sum", np.float32), ("argmax", np.int32)])
SCORE_TOP_MAX = 64       # Q3_SCORE_TOP_MAX
# q3_score_top as a numpy record: one of the k best tokens of a scored position (Transformer.score_top_many)
TOP_DTYPE = np.dtype([("logit", np.float32), ("index", np.int32)])
TOP_K_MAX = 64           # Q3_TOP_K_MAX


class Q3Error(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[q3 status {code}] {msg}")
        self.code = code
        self.msg = msg


class _Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "architecture_id", "dim", "hidden_dim", "n_layers", "n_heads", "n_kv_heads", "head_dim", "seq_len",
        "vocab_size", "group_size", "shared_classifier")]


class _SpecStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("verify_passes", "single_steps", "drafted", "accepted")]


@dataclasses.dataclass(frozen=True)
class SpecStats:
    """q3_spec_stats: what a generate_lookup call did"""
    verify_passes: int
    single_steps: int
    drafted: int
    accepted: int


class _ColsStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("passes", "live_columns", "prompt_columns", "decode_columns")]


@dataclasses.dataclass(frozen=True)
class ColsStats:
    """q3_cols_stats: the passes of a generate_many_greedy call and what their columns held"""
    passes: int
    live_columns: int
    prompt_columns: int
    decode_columns: int


class _DenseStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("blocks", "live_columns", "pad_columns")]


@dataclasses.dataclass(frozen=True)
class DenseStats:
    """q3_dense_stats: the dense blocks of a call, their live columns and their pads"""
    blocks: int
    live_columns: int
    pad_columns: int


class _EmbedStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("waves", "blocks", "live_columns", "pad_columns")]


@dataclasses.dataclass(frozen=True)
class EmbedStats:
    """q3_embed_stats: the waves of an embed_many call and the sums of their DenseStats"""
    waves: int
    blocks: int
    live_columns: int
    pad_columns: int


class _ScoreStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("waves", "blocks", "live_columns", "pad_columns", "chunks", "scored")]


@dataclasses.dataclass(frozen=True)
class ScoreStats:
    """q3_score_stats: EmbedStats' four, the classifier chunks of up to 32 scored columns and the records of a score_many call"""
    waves: int
    blocks: int
    live_columns: int
    pad_columns: int
    chunks: int
    scored: int


@dataclasses.dataclass(frozen=True)
class ModelConfig:
    """qwen3-inference/src/configuration.rs:18-30"""
    architecture_id: int
    dim: int
    hidden_dim: int
    n_layers: int
    n_heads: int
    n_kv_heads: int
    head_dim: int
    seq_len: int
    vocab_size: int
    group_size: int
    shared_classifier: bool

    @staticmethod
    def _from_c(c: _Config) -> "ModelConfig":
        return ModelConfig(c.architecture_id, c.dim, c.hidden_dim, c.n_layers, c.n_heads, c.n_kv_heads, c.head_dim,
                           c.seq_len, c.vocab_size, c.group_size, bool(c.shared_classifier))


def lib_path() -> str:
    return os.environ.get("Q3_HIP_LIB", os.path.join(_DIST_DIR, "libqwen3_hip.so"))


_lib: Optional[C.CDLL] = None


def source_build_id() -> str:
    """The id `make` bakes into the library: sha256 over csrc/* (sorted), include/qwen3_hip.h and the Makefile (compiler flags) -- first 16 hex digits.  A library built with ad-hoc `EXTRA=-D...` switches carries a different id."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_DIST_DIR, "csrc", "*"))) + [os.path.join(os.path.dirname(_DIST_DIR), "include", "qwen3_hip.h"),
                                                                          os.path.join(_DIST_DIR, "Makefile")]
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    h.update(b"\n")          # the Makefile appends its EXTRA switches (none for the product build) and a newline
    return h.hexdigest()[:16]


def dev_lib_path() -> str:
    """The developer build (`make -C qwen3-rs_amd dev`, -DQ3_DEV): the same sources plus the A/B switches (Q3_* environment
    variables beyond the documented ones), the kernel forms that lost their A/B, ablation bits and in-kernel timelines."""
    return os.path.join(_DIST_DIR, "libqwen3_hip_dev.so")


_libs: dict = {}


def load_library() -> C.CDLL:
    """Load libqwen3_hip.so.  Fails loudly: the HIP library is the product, there is nothing to fall back to."""
    global _lib
    if _lib is not None:
        return _lib
    _lib = _bind(lib_path())
    return _lib


class use_library:
    """Context manager: engines and operators created inside use the library at `path` (tests of the developer build's kernel
    forms: `with q3.use_library(q3.dev_lib_path()): ...`).  Objects keep the library they were created with."""

    def __init__(self, path: str):
        self.path = path

    def __enter__(self):
        global _lib
        self._saved = _lib
        _lib = _bind(self.path)
        return _lib

    def __exit__(self, *exc):
        global _lib
        _lib = self._saved
        return False


def _bind(path: str) -> C.CDLL:
    path = os.path.abspath(path)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise Q3Error(-1, f"{path} not found: build it with `make -C {_DIST_DIR}` (or __graft_entry__.build())")
    L = C.CDLL(path)
    fp, i8p, u8p, sz = C.POINTER(C.c_float), C.POINTER(C.c_int8), C.POINTER(C.c_uint8), C.c_size_t
    L.q3_last_error.restype = C.c_char_p
    L.q3_abi_version.restype = C.c_uint32
    L.q3_build_id.restype = C.c_char_p
    L.q3_create.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
    L.q3_get_config.argtypes = [C.c_void_p, C.POINTER(_Config)]
    L.q3_forward.argtypes = [C.c_void_p, sz, sz]
    L.q3_forward.restype = fp
    L.q3_destroy.argtypes = [C.c_void_p]
    L.q3_destroy.restype = None
    L.q3_forward_argmax.argtypes = [C.c_void_p, sz, sz, C.POINTER(C.c_int32)]
    L.q3_generate_greedy.argtypes = [C.c_void_p, sz, sz, sz, C.POINTER(C.c_int32)]
    L.q3_host_generate.argtypes = [C.c_void_p, sz, sz, sz, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.q3_host_sample_argmax.argtypes = [fp, sz, fp]
    L.q3_host_sample_argmax.restype = sz
    L.q3_prefill.argtypes = [C.c_void_p, C.POINTER(C.c_int32), sz, sz, C.POINTER(C.c_int32)]
    L.q3_prefill_batched.argtypes = [C.c_void_p, C.POINTER(C.c_int32), sz, sz, C.POINTER(C.c_int32)]
    L.q3_sampler_set.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint64]
    L.q3_sampler_get_rng.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.q3_sampler_top_k.argtypes = [C.c_void_p, C.c_int]
    L.q3_sampler_get_top_k.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.q3_forward_sample.argtypes = [C.c_void_p, sz, sz, C.POINTER(C.c_int32)]
    L.q3_generate_sampled.argtypes = [C.c_void_p, sz, sz, sz, C.POINTER(C.c_int32)]
    L.q3_reset_kv.argtypes = [C.c_void_p]
    L.q3_read_state.argtypes = [C.c_void_p, C.c_int, sz, sz, fp]
    i32p = C.POINTER(C.c_int32)
    L.q3_batch_init.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.q3_forward_batch.argtypes = [C.c_void_p, i32p, i32p, C.c_int, fp, i32p]
    L.q3_generate_greedy_batch.argtypes = [C.c_void_p, i32p, i32p, C.c_int, sz, i32p]
    L.q3_batch_sampler_set.argtypes = [C.c_void_p, C.c_float, C.c_float, C.POINTER(C.c_uint64)]
    L.q3_batch_reset_kv.argtypes = [C.c_void_p]
    L.q3_batch_read_state.argtypes = [C.c_void_p, C.c_int, C.c_int, sz, sz, fp]
    L.q3_verify.argtypes = [C.c_void_p, i32p, sz, sz, i32p, C.POINTER(sz), fp]
    L.q3_verify_draw.argtypes = L.q3_verify.argtypes
    L.q3_lookup_draft.argtypes = [i32p, sz, C.c_int, C.c_int, i32p]
    L.q3_lookup_draft.restype = sz
    L.q3_lookup_trace.argtypes = [i32p, sz, sz, C.c_int, C.c_int, i32p, i32p]
    L.q3_generate_lookup.argtypes = [C.c_void_p, i32p, sz, sz, sz, sz, C.c_int, C.c_int, i32p, C.POINTER(_SpecStats)]
    L.q3_generate_lookup_draw.argtypes = L.q3_generate_lookup.argtypes
    szp = C.POINTER(sz)
    L.q3_batch_step_cols.argtypes = [C.c_void_p, i32p, i32p, i32p, C.c_int, fp, i32p]
    L.q3_cols_schedule.argtypes = [szp, szp, sz, C.c_int, i32p, sz, szp, C.POINTER(_ColsStats)]
    L.q3_generate_many_greedy.argtypes = [C.c_void_p, i32p, szp, szp, sz, i32p, C.POINTER(_ColsStats)]
    L.q3_batch_step_cols_draw.argtypes = [C.c_void_p, i32p, i32p, i32p, C.c_int, u8p, fp, i32p]
    L.q3_generate_many_sampled.argtypes = [C.c_void_p, i32p, szp, szp, sz, fp, fp, C.POINTER(C.c_uint64), i32p, C.POINTER(_ColsStats)]
    L.q3_dense_pack.argtypes = [szp, sz, C.c_int, i32p, sz, szp, C.POINTER(_DenseStats)]
    L.q3_batch_prefill_slots.argtypes = [C.c_void_p, i32p, i32p, szp, i32p, sz, C.POINTER(_DenseStats)]
    L.q3_generate_many_dense.argtypes = [C.c_void_p, i32p, szp, szp, sz, fp, fp, C.POINTER(C.c_uint64), sz, i32p, C.POINTER(_ColsStats),
                                         C.POINTER(_DenseStats)]
    L.q3_generate_many_stop.argtypes = [C.c_void_p, i32p, szp, szp, sz, fp, fp, C.POINTER(C.c_uint64), i32p, sz, i32p, szp, C.POINTER(_ColsStats)]
    L.q3_cols_schedule_stop.argtypes = [szp, szp, sz, C.c_int, i32p, i32p, sz, i32p, sz, szp, szp, C.POINTER(_ColsStats)]
    L.q3_batch_copy_rows.argtypes = [C.c_void_p, C.c_int, i32p, C.c_int, sz, sz]
    L.q3_batch_prefix_set.argtypes = [C.c_void_p, i32p, sz]
    L.q3_batch_prefix_get.argtypes = [C.c_void_p, szp, i32p, sz]
    L.q3_generate_many_prefix.argtypes = L.q3_generate_many_stop.argtypes
    L.q3_embed_many.argtypes = [C.c_void_p, i32p, szp, sz, C.c_uint32, sz, fp, C.POINTER(_EmbedStats)]
    L.q3_choice_many.argtypes = [C.c_void_p, i32p, szp, sz, i32p, sz, C.c_uint32, fp, C.POINTER(_EmbedStats)]
    L.q3_score_many.argtypes = [C.c_void_p, i32p, szp, sz, szp, C.c_uint32, C.c_void_p, C.POINTER(_ScoreStats)]
    L.q3_score_pack.argtypes = [szp, sz, szp, C.c_int, C.c_int, C.POINTER(_ScoreStats)]
    L.q3_score_top_many.argtypes = [C.c_void_p, i32p, szp, sz, szp, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_ScoreStats)]
    L.q3_gen_logprobs.argtypes = [C.c_void_p, C.c_int]
    L.q3_gen_logprobs_get.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.q3_gen_logprobs_read.argtypes = [C.c_void_p, sz, sz, C.c_void_p, C.c_void_p, C.c_void_p]
    L.q3_profile.argtypes = [C.c_void_p, sz, sz, C.c_int, fp, C.POINTER(C.c_int32), C.c_int]
    L.q3_profile_name.argtypes = [C.c_int]
    L.q3_profile_name.restype = C.c_char_p
    L.q3_parse_header.argtypes = [u8p, sz, C.POINTER(_Config)]
    L.q3_op_quantize.argtypes = [i8p, fp, fp, sz, sz, C.c_int]
    L.q3_op_dequantize.argtypes = [i8p, fp, fp, sz, sz, C.c_int]
    L.q3_op_matmul.argtypes = [fp, i8p, fp, i8p, fp, sz, sz, sz, C.c_int]
    L.q3_op_gemv_role.argtypes = [C.c_int, fp, fp, i32p, i32p, fp, fp, i8p, fp, i8p, fp, sz, sz, sz, sz, sz, C.c_uint32, C.c_int]
    L.q3_op_rmsnorm.argtypes = [fp, fp, fp, sz, C.c_uint32, C.c_int]
    L.q3_op_softmax.argtypes = [fp, sz, C.c_uint32, C.c_int]
    L.q3_op_swiglu.argtypes = [fp, fp, sz, C.c_int]
    L.q3_op_expf.argtypes = [fp, sz, C.c_int]
    L.q3_op_attention.argtypes = [fp, fp, fp, fp, fp, fp, sz, sz, sz, sz, sz, C.c_uint32, C.c_int]
    L.q3_op_argmax.argtypes = [fp, sz, C.POINTER(C.c_int32), C.c_int]
    L.q3_op_sample.argtypes = [fp, sz, C.c_float, C.c_float, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.c_int]
    L.q3_op_sample_top_k.argtypes = [fp, sz, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.c_int]
    L.q3_sampler_penalties.argtypes = [C.c_void_p, C.c_float, C.c_float]
    L.q3_sampler_get_penalties.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.q3_op_penalize.argtypes = [fp, C.POINTER(C.c_uint32), sz, C.c_float, C.c_float, fp, C.POINTER(C.c_int32), C.c_int]
    L.q3_logit_bias_set.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), sz]
    L.q3_logit_bias_get.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.q3_op_logit_bias.argtypes = [fp, sz, C.c_void_p, sz, C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.c_float, C.c_float, fp, C.POINTER(C.c_int32),
                                   C.c_int]
    L.q3_guide_set.argtypes = [C.c_void_p, C.c_void_p, sz, sz, C.POINTER(C.c_int32), sz]
    L.q3_guide_get.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.q3_op_guide.argtypes = [fp, sz, C.c_void_p, C.c_void_p, sz, C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.c_float, C.c_float, fp,
                              C.POINTER(C.c_int32), C.c_int]
    L.q3_guide_set_sparse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, sz, sz, sz, C.POINTER(C.c_int32), sz]
    L.q3_guide_get_sparse.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.q3_op_guide_sparse.argtypes = [fp, sz, C.c_int32, C.c_void_p, sz, C.c_void_p, sz, C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.c_float, C.c_float, fp,
                                     C.POINTER(C.c_int32), C.c_int]
    L.q3_stop_seq_set.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, sz, sz, sz, C.POINTER(C.c_int32), sz]
    L.q3_stop_seq_get.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.q3_cols_schedule_stop_seq.argtypes = [szp, szp, sz, C.c_int, i32p, i32p, sz, C.c_void_p, C.c_void_p, C.c_void_p, sz, sz, sz, C.POINTER(C.c_int32), sz,
                                            i32p, sz, szp, szp, C.POINTER(_ColsStats)]
    L.q3_op_stop_seq.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, sz, sz, sz, C.c_int32, i32p, sz, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    _libs[path] = L
    return L


def _check_bias_list(entries, mode=BIAS_ADD, who="list"):
    """One list of q3_logit_bias_set / q3_op_logit_bias as the library accepts it, checked before the call: a dict {token: bias} or a
    sequence of (token, bias) / (token, bias, until).  Returns [(token, bias, until)] sorted by token."""
    if isinstance(mode, bool) or not isinstance(mode, (int, np.integer)):
        raise TypeError(f"{who}: mode must be BIAS_ADD (0) or BIAS_ALLOW (1), got {mode!r}")
    if mode not in (BIAS_ADD, BIAS_ALLOW):
        raise ValueError(f"{who}: mode {mode} is neither BIAS_ADD (0) nor BIAS_ALLOW (1)")
    if isinstance(entries, (str, bytes)) or not hasattr(entries, "__iter__"):
        raise TypeError(f"{who}: a dict {{token: bias}} or a sequence of (token, bias[, until]), got {entries!r}")
    items = [(k, v, 0) for k, v in entries.items()] if isinstance(entries, dict) else [tuple(x) if hasattr(x, "__iter__") else x for x in entries]
    out, seen = [], set()
    for x in items:
        if not isinstance(x, tuple) or len(x) not in (2, 3):
            raise TypeError(f"{who}: an entry is (token, bias) or (token, bias, until), got {x!r}")
        token, bias, until = x if len(x) == 3 else (x[0], x[1], 0)
        if isinstance(token, bool) or not isinstance(token, (int, np.integer)):
            raise TypeError(f"{who}: token must be an integer, got {token!r}")
        if isinstance(until, bool) or not isinstance(until, (int, np.integer)):
            raise TypeError(f"{who}: until must be an integer, got {until!r}")
        if isinstance(bias, bool) or not isinstance(bias, (int, float, np.integer, np.floating)):
            raise TypeError(f"{who}: bias must be a number, got {bias!r}")
        if token < 0 or token > 0x7fffffff:
            raise ValueError(f"{who}: token {token} out of range")
        if until < 0 or until > 0xffffffff:
            raise ValueError(f"{who}: until {until} out of range")
        with np.errstate(over="ignore"):
            f = np.float32(bias)
        if not (f == -np.inf or abs(f) <= np.float32(BIAS_LIMIT)):        # false for a NaN and for +inf
            raise ValueError(f"{who}: bias {bias} of token {token} is neither -inf nor finite in -{BIAS_LIMIT}..{BIAS_LIMIT}")
        if int(token) in seen:
            raise ValueError(f"{who}: token {token} twice")
        seen.add(int(token))
        out.append((int(token), float(f), int(until)))
    if len(out) > BIAS_MAX:
        raise ValueError(f"{who}: {len(out)} entries, at most {BIAS_MAX}")
    if mode == BIAS_ALLOW and not any(np.isfinite(b) for _, b, _ in out):
        raise ValueError(f"{who}: an ALLOW list without a finite bias allows no token")
    return sorted(out)


def _check_bias_table(lists, modes):
    """(lists, modes) of Transformer.set_logit_bias, checked and normalised: per list [(token, bias, until)], per list a mode"""
    if isinstance(lists, (dict, str, bytes)) or not hasattr(lists, "__iter__"):
        raise TypeError(f"lists must be a sequence of lists (one for all requests, or one per request), got {lists!r}")
    lists = list(lists)
    if modes is None:
        modes = [BIAS_ADD] * len(lists)
    if isinstance(modes, (str, bytes)) or not hasattr(modes, "__iter__"):
        raise TypeError(f"modes must be None or one mode per list, got {modes!r}")
    modes = list(modes)
    if len(modes) != len(lists):
        raise ValueError(f"{len(lists)} lists and {len(modes)} modes")
    return [_check_bias_list(l, m, f"list {i}") for i, (l, m) in enumerate(zip(lists, modes))], [int(m) for m in modes]


def _bias_array(entries):
    a = np.zeros(len(entries), dtype=BIAS_DTYPE)
    for i, (token, bias, until) in enumerate(entries):
        a[i] = (token, bias, until)
    return a


def _check_penalties(presence, frequency):
    """the values q3_sampler_penalties and q3_op_penalize accept (finite, -2 .. 2 once rounded to f32), checked before the call"""
    for name, v in (("presence", presence), ("frequency", frequency)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError(f"{name} penalty must be a number, got {v!r}")
        with np.errstate(over="ignore"):
            f = np.float32(v)
        if not np.isfinite(f) or abs(f) > np.float32(PENALTY_MAX):
            raise ValueError(f"{name} penalty {v} out of range (finite, -{PENALTY_MAX}..{PENALTY_MAX})")


def _check(rc: int):
    if rc != 0:
        raise Q3Error(rc, load_library().q3_last_error().decode(errors="replace"))


def _check_top_k(k, lowest: int, n: int):
    """the range q3_sampler_top_k (lowest 0: off) and q3_op_sample_top_k (lowest 1) accept, checked before the call"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"top_k must be an integer, got {k!r}")
    if k < lowest or k > TOP_K_MAX or k > n:
        raise ValueError(f"top_k {k} out of range ({lowest}..{TOP_K_MAX}, at most the vocabulary's {n} entries)")


def _check_gen_logprobs(top_n, n: int):
    """the range q3_gen_logprobs accepts (-1: off), checked before the call"""
    if isinstance(top_n, bool) or not isinstance(top_n, (int, np.integer)):
        raise TypeError(f"logprobs must be an integer, got {top_n!r}")
    if top_n < -1 or top_n > SCORE_TOP_MAX or top_n > n:
        raise ValueError(f"logprobs {top_n} out of range (-1..{SCORE_TOP_MAX}, at most the vocabulary's {n} entries)")


def _i32_array(tokens):
    return (C.c_int32 * max(1, len(tokens)))(*[int(t) for t in tokens])


def lookup_draft(seq, ngram: int, draft_len: int) -> List[int]:
    """The prompt-lookup drafter (q3_lookup_draft, host only): the continuation of the latest earlier occurrence of the last
    `ngram` tokens of seq, at most draft_len tokens; [] = no draft."""
    out = (C.c_int32 * max(1, draft_len))()
    k = load_library().q3_lookup_draft(_i32_array(seq), len(seq), ngram, draft_len, out)
    return [int(out[i]) for i in range(k)]


def lookup_trace(seq, n_corpus: int, ngram: int, draft_len: int) -> List[List[int]]:
    """The incremental drafter of generate_lookup (q3_lookup_trace, host only): the drafts over seq[:m] for m = n_corpus .. len(seq)."""
    rows = len(seq) - n_corpus + 1
    drafts = (C.c_int32 * max(1, rows * draft_len))()
    lens = (C.c_int32 * max(1, rows))()
    _check(load_library().q3_lookup_trace(_i32_array(seq), len(seq), n_corpus, ngram, draft_len, drafts, lens))
    return [[int(drafts[r * draft_len + k]) for k in range(lens[r])] for r in range(rows)]


def _size_array(values):
    return (C.c_size_t * max(1, len(values)))(*[int(v) for v in values])


def cols_schedule(prompt_len, n_new, max_streams: int):
    """The pass table of generate_many_greedy (q3_cols_schedule, host only): ([(pass, slot, pos, request), ...] in column order,
    ColsStats) for requests of prompt_len[r] prompt tokens and n_new[r] new tokens through max_streams slots."""
    if len(prompt_len) != len(n_new):
        raise ValueError("one n_new per prompt")
    L = load_library()
    pl, nn, n, st = _size_array(prompt_len), _size_array(n_new), C.c_size_t(0), _ColsStats()
    _check(L.q3_cols_schedule(pl, nn, len(prompt_len), max_streams, None, 0, C.byref(n), C.byref(st)))
    table = (C.c_int32 * max(1, 4 * n.value))()
    _check(L.q3_cols_schedule(pl, nn, len(prompt_len), max_streams, table, n.value, C.byref(n), C.byref(st)))
    rows = [tuple(int(table[4 * i + k]) for k in range(4)) for i in range(n.value)]
    return rows, ColsStats(st.passes, st.live_columns, st.prompt_columns, st.decode_columns)


def cols_schedule_stop(prompt_len, n_new, max_streams: int, rows, stop_tokens):
    """The passes generate_many_stop runs when request r would produce the tokens rows[r] (n_new[r] of them) and ends at its first
    token of stop_tokens (q3_cols_schedule_stop, host only: the scheduler step of the device loop, run on the host).
    Returns ([(pass, slot, pos, request), ...] in column order, n_out per request, ColsStats)."""
    if len(prompt_len) != len(n_new) or len(rows) != len(n_new) or any(len(r) != int(k) for r, k in zip(rows, n_new)):
        raise ValueError("one n_new and one row of n_new tokens per prompt")
    L = load_library()
    nr = len(prompt_len)
    pl, nn, n, st = _size_array(prompt_len), _size_array(n_new), C.c_size_t(0), _ColsStats()
    flat, stop, n_out = _i32_array([t for r in rows for t in r]), _i32_array(stop_tokens), _size_array([0] * nr)
    _check(L.q3_cols_schedule_stop(pl, nn, nr, max_streams, flat, stop, len(stop_tokens), None, 0, C.byref(n), n_out, C.byref(st)))
    table = (C.c_int32 * max(1, 4 * n.value))()
    _check(L.q3_cols_schedule_stop(pl, nn, nr, max_streams, flat, stop, len(stop_tokens), table, n.value, C.byref(n), n_out, C.byref(st)))
    cols = [tuple(int(table[4 * i + k]) for k in range(4)) for i in range(n.value)]
    return cols, [int(n_out[r]) for r in range(nr)], ColsStats(st.passes, st.live_columns, st.prompt_columns, st.decode_columns)


def _sparse_tables(default, offsets, tokens, targets):
    """the arrays of a SparseAutomaton as the library takes them: (dflt int32, row_off uint32, edges EDGE_DTYPE), checked for type
    and range of the integer formats only -- what the tables may say is the library's to refuse"""
    arrays = []
    for name, a in (("default", default), ("offsets", offsets), ("tokens", tokens), ("targets", targets)):
        a = np.asarray(a)
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise TypeError(f"{name} must be a vector of integers")
        if a.size and (a.min() < -0x80000000 or a.max() > (0xffffffff if name == "offsets" else 0x7fffffff)):
            raise ValueError(f"an entry of {name} does not fit its 32 bits")
        arrays.append(a)
    default, offsets, tokens, targets = arrays
    if tokens.size != targets.size or (offsets.size and offsets.min() < 0):
        raise ValueError("tokens must hold as many entries as targets, and no offset may be negative")
    edges = np.empty(tokens.size, dtype=EDGE_DTYPE)
    edges["token"], edges["next"] = tokens, targets
    return np.ascontiguousarray(default, dtype=np.int32), np.ascontiguousarray(offsets, dtype=np.uint32), edges


def _void(a):
    return a.ctypes.data_as(C.c_void_p) if a.size else None


def cols_schedule_stop_seq(prompt_len, n_new, max_streams: int, rows, stop_tokens, tables, vocab_size: int, start):
    """cols_schedule_stop under a stop automaton (q3_cols_schedule_stop_seq, host only: the scheduler step and the automaton step of
    the device loop, run on the host).  tables: (default, offsets, tokens, targets) as guide.SparseAutomaton holds them, or None for
    no automaton; start: one start state, or one per request (-1: no stop sequences for that request).
    Returns ([(pass, slot, pos, request), ...] in column order, n_out per request, ColsStats)."""
    if len(prompt_len) != len(n_new) or len(rows) != len(n_new) or any(len(r) != int(k) for r, k in zip(rows, n_new)):
        raise ValueError("one n_new and one row of n_new tokens per prompt")
    L = load_library()
    nr = len(prompt_len)
    pl, nn, n, st = _size_array(prompt_len), _size_array(n_new), C.c_size_t(0), _ColsStats()
    flat, stop, n_out = _i32_array([t for r in rows for t in r]), _i32_array(stop_tokens), _size_array([0] * nr)
    if tables is None:
        auto = (None, None, None, 0, 0, 0, None, 0)
    else:
        dflt, off, edges = _sparse_tables(*tables)
        starts = [int(start)] if isinstance(start, (int, np.integer)) else [int(x) for x in start]
        auto = (_void(dflt), _void(off), _void(edges), dflt.size, edges.size, int(vocab_size), _i32_array(starts), len(starts))
    _check(L.q3_cols_schedule_stop_seq(pl, nn, nr, max_streams, flat, stop, len(stop_tokens), *auto, None, 0, C.byref(n), n_out, C.byref(st)))
    table = (C.c_int32 * max(1, 4 * n.value))()
    _check(L.q3_cols_schedule_stop_seq(pl, nn, nr, max_streams, flat, stop, len(stop_tokens), *auto, table, n.value, C.byref(n), n_out, C.byref(st)))
    cols = [tuple(int(table[4 * i + k]) for k in range(4)) for i in range(n.value)]
    return cols, [int(n_out[r]) for r in range(nr)], ColsStats(st.passes, st.live_columns, st.prompt_columns, st.decode_columns)


def dense_pack(run_len, block_cap: int):
    """How runs of run_len[r] columns are packed into dense blocks of up to block_cap columns (q3_dense_pack, host only):
    ([(block, first column, run, offset in the run), ...] in order, DenseStats)."""
    L = load_library()
    rl, n, st = _size_array(run_len), C.c_size_t(0), _DenseStats()
    _check(L.q3_dense_pack(rl, len(run_len), block_cap, None, 0, C.byref(n), C.byref(st)))
    table = (C.c_int32 * max(1, 4 * n.value))()
    _check(L.q3_dense_pack(rl, len(run_len), block_cap, table, n.value, C.byref(n), C.byref(st)))
    rows = [tuple(int(table[4 * i + k]) for k in range(4)) for i in range(n.value)]
    return rows, DenseStats(st.blocks, st.live_columns, st.pad_columns)


def score_pack(prompt_len, score_from, max_streams: int, block_cap: int) -> ScoreStats:
    """The schedule of score_many (q3_score_pack, host only): its ScoreStats for prompts of prompt_len[r] tokens scored from
    score_from[r] (None: 1 everywhere) through max_streams slots and dense blocks of up to block_cap columns."""
    if score_from is not None and len(score_from) != len(prompt_len):
        raise IndexError("one score_from per prompt")
    st = _ScoreStats()
    rc = load_library().q3_score_pack(_size_array(prompt_len), len(prompt_len), None if score_from is None else _size_array(score_from),
                                      max_streams, block_cap, C.byref(st))
    if rc == -3:
        raise IndexError(load_library().q3_last_error().decode(errors="replace"))
    _check(rc)
    return ScoreStats(st.waves, st.blocks, st.live_columns, st.pad_columns, st.chunks, st.scored)


def parse_header(data: bytes) -> ModelConfig:
    """configuration.rs:77-146 via the library's own parser (no GPU needed)."""
    L = load_library()
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data if data else b"\0")
    cfg = _Config()
    _check(L.q3_parse_header(buf, len(data), C.byref(cfg)))
    return ModelConfig._from_c(cfg)


class Transformer:
    """`trait Transformer` (models/mod.rs:13-18) implemented by the HIP engine."""

    def __init__(self, handle: int, lib: C.CDLL):
        self._h = C.c_void_p(handle)
        self._lib = lib
        cfg = _Config()
        _check(lib.q3_get_config(self._h, C.byref(cfg)))
        self._config = ModelConfig._from_c(cfg)
        self._sampler = None                     # (temperature, topp) of the last set_sampler

    # -- the reference surface ------------------------------------------------------------------
    def forward(self, token: int, pos: int) -> np.ndarray:
        """forward(token,pos) -> logits[vocab_size] (models/qwen3.rs:62-79).  The returned array is a VIEW of
        the engine's host buffer, valid until the next call -- the same borrow rule as `&[f32]` from
        `&mut self`; copy it like generation.rs:160 does."""
        if token < 0 or pos < 0:
            raise IndexError("negative index")
        p = self._lib.q3_forward(self._h, token, pos)
        if not p:
            msg = self._lib.q3_last_error().decode(errors="replace")
            if "out of range" in msg:
                raise IndexError(msg)   # the reference panics on slice indexing (layers.rs:73-75,335)
            raise Q3Error(-4, msg)
        return np.ctypeslib.as_array(p, shape=(self._config.vocab_size,))

    def get_config(self) -> ModelConfig:
        return self._config

    # -- extensions -------------------------------------------------------------------------------
    def forward_argmax(self, token: int, pos: int) -> int:
        out = C.c_int32(-1)
        rc = self._lib.q3_forward_argmax(self._h, token, pos, C.byref(out))
        if rc == -3:
            raise IndexError(self._lib.q3_last_error().decode(errors="replace"))
        _check(rc)
        return int(out.value)

    def forward_sample(self, token: int, pos: int) -> int:
        """forward + the device sampler's draw (q3_forward_sample; argmax while no sampler with temperature > 0 is set)"""
        out = C.c_int32(-1)
        rc = self._lib.q3_forward_sample(self._h, token, pos, C.byref(out))
        if rc == -3:
            raise IndexError(self._lib.q3_last_error().decode(errors="replace"))
        _check(rc)
        return int(out.value)

    def generate_greedy(self, first_token: int, first_pos: int, n_tokens: int) -> List[int]:
        buf = (C.c_int32 * max(1, n_tokens))()
        rc = self._lib.q3_generate_greedy(self._h, first_token, first_pos, n_tokens, buf)
        if rc == -3:
            raise IndexError(self._lib.q3_last_error().decode(errors="replace"))
        _check(rc)
        return [int(buf[i]) for i in range(n_tokens)]

    def host_generate(self, first_token: int, first_pos: int, n_tokens: int) -> Tuple[List[int], float]:
        """The reference's decode loop in compiled host code on top of forward(): logits egress + host argmax per
        token (generation.rs:153-162).  Returns (tokens, TokenMetrics seconds)."""
        buf = (C.c_int32 * max(1, n_tokens))()
        secs = C.c_double(0.0)
        rc = self._lib.q3_host_generate(self._h, first_token, first_pos, n_tokens, buf, C.byref(secs))
        if rc == -3:
            raise IndexError(self._lib.q3_last_error().decode(errors="replace"))
        _check(rc)
        return [int(buf[i]) for i in range(n_tokens)], float(secs.value)

    def prefill(self, tokens, first_pos: int = 0, batched: bool = False) -> int:
        """chat-mode prompt loop on the device (generation.rs:116-123); returns the first generated token.
        batched=True walks the prompt in blocks of up to 2,048 positions per weight pass (q3_prefill_batched; Q3_PREFILL_M), same results."""
        arr = (C.c_int32 * len(tokens))(*[int(t) for t in tokens])
        out = C.c_int32(-1)
        fn = self._lib.q3_prefill_batched if batched else self._lib.q3_prefill
        rc = fn(self._h, arr, len(tokens), first_pos, C.byref(out))
        if rc == -3:
            raise IndexError(self._lib.q3_last_error().decode(errors="replace"))
        _check(rc)
        return int(out.value)

    # ---- draft verification and prompt-lookup decode (include/qwen3_hip.h section 2c)
    def verify(self, tokens, first_pos: int, want_logits: bool = False):
        """One weight pass over tokens (tokens[0] certain, the rest drafts) at first_pos..: returns (next_tokens, n_accepted) or,
        with want_logits, (next_tokens, n_accepted, logits [n, vocab]).  next_tokens[:n_accepted + 1] are the greedy tokens and
        the engine is left as generate_greedy(tokens[0], first_pos, n_accepted + 1) leaves it."""
        return self._verify(self._lib.q3_verify, tokens, first_pos, want_logits)

    def verify_draw(self, tokens, first_pos: int, want_logits: bool = False):
        """verify() under the device sampler (q3_verify_draw, section 2d): next_tokens[i] is the sampler's draw on column i with
        the rng i coins past its state at entry; the engine and the rng are left as generate_sampled(tokens[0], first_pos,
        n_accepted + 1) leaves them.  With temperature 0 it is verify()."""
        return self._verify(self._lib.q3_verify_draw, tokens, first_pos, want_logits)

    def _verify(self, fn, tokens, first_pos: int, want_logits: bool):
        n = len(tokens)
        nxt = (C.c_int32 * max(1, n))()
        acc = C.c_size_t(0)
        logits = np.zeros((n, self._config.vocab_size), dtype=np.float32) if want_logits else None
        lp = logits.ctypes.data_as(C.POINTER(C.c_float)) if want_logits else None
        rc = fn(self._h, _i32_array(tokens), n, first_pos, nxt, C.byref(acc), lp)
        if rc == -3:
            raise IndexError(self._lib.q3_last_error().decode(errors="replace"))
        _check(rc)
        out = [int(nxt[i]) for i in range(n)]
        return (out, int(acc.value), logits) if want_logits else (out, int(acc.value))

    def generate_lookup(self, corpus, first_token: int, first_pos: int, n_tokens: int, ngram: int = 2, draft_len: int = 8):
        """generate_greedy with prompt-lookup drafts (q3_generate_lookup): the same tokens and engine state in fewer weight
        passes.  corpus: the tokens to look continuations up in (the prompt).  Returns (tokens, SpecStats)."""
        return self._generate_lookup(self._lib.q3_generate_lookup, corpus, first_token, first_pos, n_tokens, ngram, draft_len)

    def generate_lookup_draw(self, corpus, first_token: int, first_pos: int, n_tokens: int, ngram: int = 2, draft_len: int = 8,
                             stop_tokens=()):
        """generate_sampled with prompt-lookup drafts (q3_generate_lookup_draw, section 2d): a draft is accepted exactly when it
        is the token the sampler draws, so tokens, engine state and final rng equal generate_sampled's at any temperature.
        Returns (tokens, SpecStats).
        stop_tokens: a loop that ends at a stop token never draws behind it, a call of n_tokens does.  With stop_tokens the
        returned tokens end with the first stop token and the rng is put back to where that token's draw left it, so whatever
        is sampled next is what the token-by-token loop would sample (cache rows written behind it are rewritten before they
        are read, as after any shorter call)."""
        coins = bool(stop_tokens) and self._sampler is not None and self._sampler[0] > 0.0
        rng = self.sampler_rng_state() if coins else 0
        toks, stats = self._generate_lookup(self._lib.q3_generate_lookup_draw, corpus, first_token, first_pos, n_tokens, ngram, draft_len)
        k = next((i for i, t in enumerate(toks) if t in stop_tokens), None)
        if k is not None:
            if coins and k + 1 < len(toks):
                for _ in range(k + 1):                    # sampler.rs:44-49
                    rng ^= rng >> 12
                    rng = (rng ^ (rng << 25)) & 0xFFFFFFFFFFFFFFFF
                    rng ^= rng >> 27
                self.set_sampler(self._sampler[0], self._sampler[1], rng)
            toks = toks[:k + 1]
        return toks, stats

    def _generate_lookup(self, fn, corpus, first_token: int, first_pos: int, n_tokens: int, ngram: int, draft_len: int):
        buf = (C.c_int32 * max(1, n_tokens))()
        st = _SpecStats()
        rc = fn(self._h, _i32_array(corpus), len(corpus), first_token, first_pos, n_tokens, ngram, draft_len, buf, C.byref(st))
        if rc == -3:
            raise IndexError(self._lib.q3_last_error().decode(errors="replace"))
        _check(rc)
        return [int(buf[i]) for i in range(n_tokens)], SpecStats(st.verify_passes, st.single_steps, st.drafted, st.accepted)

    def set_sampler(self, temperature: float, topp: float, rng_seed: int):
        """Sampler::new (sampler.rs:29-42) on the device: subsequent forward_argmax / generate_greedy / prefill calls draw
        with Sampler::sample; temperature 0 restores greedy decoding."""
        _check(self._lib.q3_sampler_set(self._h, temperature, topp, rng_seed))
        self._sampler = (temperature, topp)

    def set_top_k(self, k: int):
        """Top-k sampling (q3_sampler_top_k, include/qwen3_hip.h section 2n): every draw the engine makes at temperature > 0 -- single
        stream, batched decode, verify blocks and column passes alike -- is taken among the k most likely tokens; 0 turns it off.
        The setting is the engine's: it survives set_sampler, batch_init, batch_sampler_set and every generate_many call, and
        changing it between two non-zero values rebuilds nothing."""
        _check_top_k(k, 0, self._config.vocab_size)
        _check(self._lib.q3_sampler_top_k(self._h, k))

    @property
    def top_k(self) -> int:
        """the engine's top-k setting (q3_sampler_get_top_k); 0: off"""
        out = C.c_int(0)
        _check(self._lib.q3_sampler_get_top_k(self._h, C.byref(out)))
        return int(out.value)

    def sampler_rng_state(self) -> int:
        out = C.c_uint64(0)
        _check(self._lib.q3_sampler_get_rng(self._h, C.byref(out)))
        return int(out.value)

    def reset_kv(self):
        _check(self._lib.q3_reset_kv(self._h))

    def read_state(self, kind: str, offset: int = 0, count: Optional[int] = None) -> np.ndarray:
        c = self._config
        kinds = {"key": 0, "value": 1, "x": 2}
        total = c.dim if kind == "x" else c.n_layers * c.seq_len * c.n_kv_heads * c.head_dim
        count = total - offset if count is None else count
        out = np.zeros(count, dtype=np.float32)
        _check(self._lib.q3_read_state(self._h, kinds[kind], offset, count, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    # ---- batched decode (include/qwen3_hip.h section 2b): N concurrent generate loops, weights streamed once per step
    def batch_init(self, max_streams: int, ctx_len: int = 0):
        _check(self._lib.q3_batch_init(self._h, max_streams, ctx_len))
        self._batch_ctx = min(ctx_len, self._config.seq_len) if ctx_len else self._config.seq_len

    def _batch_rc(self, rc):
        if rc == -3:
            raise IndexError(self._lib.q3_last_error().decode(errors="replace"))
        _check(rc)

    def forward_batch(self, tokens, pos, want_logits: bool = True):
        """Stream i runs forward(tokens[i], pos[i]); returns (logits [n, vocab] or None, argmax list)."""
        n = len(tokens)
        tk = (C.c_int32 * n)(*[int(t) for t in tokens])
        ps = (C.c_int32 * n)(*[int(p) for p in pos])
        am = (C.c_int32 * n)()
        logits = np.zeros((n, self._config.vocab_size), dtype=np.float32) if want_logits else None
        lp = logits.ctypes.data_as(C.POINTER(C.c_float)) if want_logits else None
        self._batch_rc(self._lib.q3_forward_batch(self._h, tk, ps, n, lp, am))
        return logits, [int(v) for v in am]

    def generate_greedy_batch(self, first_tokens, first_pos, n_steps: int) -> np.ndarray:
        """[n_streams, n_steps] greedy tokens, the whole loop on the device."""
        n = len(first_tokens)
        tk = (C.c_int32 * n)(*[int(t) for t in first_tokens])
        ps = (C.c_int32 * n)(*[int(p) for p in first_pos])
        out = np.zeros((n, n_steps), dtype=np.int32)
        self._batch_rc(self._lib.q3_generate_greedy_batch(self._h, tk, ps, n, n_steps, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    # ---- ragged column passes over the batched state (include/qwen3_hip.h section 2e)
    def batch_step_cols(self, slots, tokens, pos, want_logits: bool = False):
        """One weight pass of up to 32 columns: column j runs forward(tokens[j], pos[j]) over the KV cache of slot slots[j]; the
        columns of a slot are adjacent with consecutive positions.  Returns the argmax list or, with want_logits,
        (logits [n, vocab], argmax list)."""
        n = len(slots)
        if not (len(tokens) == n and len(pos) == n):
            raise ValueError("one token and one position per column")
        nxt = (C.c_int32 * max(1, n))()
        logits = np.zeros((n, self._config.vocab_size), dtype=np.float32) if want_logits else None
        lp = logits.ctypes.data_as(C.POINTER(C.c_float)) if want_logits else None
        self._batch_rc(self._lib.q3_batch_step_cols(self._h, _i32_array(slots), _i32_array(tokens), _i32_array(pos), n, lp, nxt))
        out = [int(nxt[i]) for i in range(n)]
        return (logits, out) if want_logits else out

    def generate_many_greedy(self, prompts, n_new):
        """Greedy generations of many requests through the slots of batch_init, the whole loop on the device
        (q3_generate_many_greedy): prompts enter in chunks next to the decode columns of other slots, finished requests hand
        their slot to the next one.  prompts: one token list per request; n_new: tokens wanted per request (the first is the
        token behind the prompt).  Returns ([n_new[r] tokens] per request, ColsStats)."""
        return self._generate_many(prompts, n_new, None, lambda rq, smp, out, st: self._batch_rc(self._lib.q3_generate_many_greedy(*rq, out, st)))[:2]

    def _generate_many(self, prompts, n_new, sampler, call):
        """What every generate_many_* does around its library function.  call(rq, smp, out, st) runs it: rq = (handle, concatenated
        prompts, prompt lengths, n_new, number of requests), smp = the three per-request sampler arrays made from sampler =
        (temperature, topp, seeds), one value per request or a scalar each (sampler None: three None), out the output buffer,
        st the q3_cols_stats.  It returns the function's n_out array, to which the rows are cut, or None: rows of n_new tokens.
        Returns (rows, ColsStats, the output buffer as the library filled it, tokens per row)."""
        n = len(prompts)
        if len(n_new) != n:
            raise ValueError("one n_new per prompt")

        def per_request(v, what, ctype, conv):
            vals = [v] * n if np.isscalar(v) else list(v)
            if len(vals) != n:
                raise ValueError(f"one {what} per request, or a scalar")
            return (ctype * max(1, n))(*[conv(x) for x in vals])
        smp = (None, None, None)
        if sampler is not None:
            temperature, topp, seeds = sampler
            smp = (per_request(temperature, "temperature", C.c_float, float), per_request(topp, "topp", C.c_float, float),
                   per_request(seeds, "seed", C.c_uint64, lambda x: int(x) & 0xFFFFFFFFFFFFFFFF))
        flat = [int(t) for p in prompts for t in p]
        total = sum(int(k) for k in n_new)
        out = (C.c_int32 * max(1, total))()
        st = _ColsStats()
        n_out = call((self._h, _i32_array(flat), _size_array([len(p) for p in prompts]), _size_array(n_new), n), smp, out, C.byref(st))
        got = [int(k) for k in n_new] if n_out is None else [int(n_out[r]) for r in range(n)]
        self._gen_last = ([int(k) for k in n_new], got, getattr(self, "_gen_lp", -1))    # what read_gen_logprobs cuts the call's records by
        buf, rows, at = out[:total], [], 0
        for k, g in zip(n_new, got):
            rows.append(buf[at:at + g])
            at += int(k)
        return rows, ColsStats(st.passes, st.live_columns, st.prompt_columns, st.decode_columns), buf, got

    # ---- column passes under the sampler (include/qwen3_hip.h section 2f)
    def batch_step_cols_draw(self, slots, tokens, pos, keep=None, want_logits: bool = False):
        """batch_step_cols under the per-slot samplers of set_batch_sampler (q3_batch_step_cols_draw): column j at index k of its
        slot's run is drawn with the slot's rng advanced k coins, and the slot's rng moves on by the run's length.  keep: one
        flag per column (None = all kept); a column with keep 0 consumes its coin, draws nothing and returns -1.  Returns the
        list of draws or, with want_logits, (raw logits [n, vocab], draws)."""
        n = len(slots)
        if not (len(tokens) == n and len(pos) == n and (keep is None or len(keep) == n)):
            raise ValueError("one token, one position and one keep flag per column")
        nxt = (C.c_int32 * max(1, n))()
        kp = None if keep is None else (C.c_uint8 * max(1, n))(*[1 if k else 0 for k in keep])
        logits = np.zeros((n, self._config.vocab_size), dtype=np.float32) if want_logits else None
        lp = logits.ctypes.data_as(C.POINTER(C.c_float)) if want_logits else None
        self._batch_rc(self._lib.q3_batch_step_cols_draw(self._h, _i32_array(slots), _i32_array(tokens), _i32_array(pos), n, kp, lp, nxt))
        out = [int(nxt[i]) for i in range(n)]
        return (logits, out) if want_logits else out

    def generate_many_sampled(self, prompts, n_new, temperature, topp, seeds):
        """generate_many_greedy with one sampler per request (q3_generate_many_sampled): request r is drawn as a fresh engine after
        set_sampler(temperature[r], topp[r], seeds[r]) draws prefill + generate_greedy; temperature 0 makes a request greedy.
        temperature / topp / seeds: one value per request, or a scalar for all.  Returns (rows, ColsStats).  The per-stream
        states of set_batch_sampler are unspecified afterwards: set them again before using them."""
        return self._generate_many(prompts, n_new, (temperature, topp, seeds),
                                   lambda rq, smp, out, st: self._batch_rc(self._lib.q3_generate_many_sampled(*rq, *smp, out, st)))[:2]

    # ---- dense blocks over the slots (include/qwen3_hip.h section 2g)
    dense_pack = staticmethod(dense_pack)

    def batch_prefill_slots(self, slots, prompts, first_pos):
        """Cache rows of many slots in dense blocks (q3_batch_prefill_slots): prompts[r] enters slot slots[r] at positions
        first_pos[r] ..; several runs share one pass over the weights.  No logits and no token: the prompt's last token goes
        through batch_step_cols.  Under a sampling batch the slot's rng moves on by the run's length.  Returns DenseStats."""
        n = len(slots)
        if not (len(prompts) == n and len(first_pos) == n):
            raise ValueError("one prompt and one first position per slot")
        flat = [int(t) for p in prompts for t in p]
        st = _DenseStats()
        self._batch_rc(self._lib.q3_batch_prefill_slots(self._h, _i32_array(slots), _i32_array(flat), _size_array([len(p) for p in prompts]),
                                                        _i32_array(first_pos), n, C.byref(st)))
        return DenseStats(st.blocks, st.live_columns, st.pad_columns)

    def generate_many_dense(self, prompts, n_new, sampler=None, dense_min: int = 64):
        """generate_many_greedy (sampler None) or generate_many_sampled (sampler = (temperature, topp, seeds), one value per
        request or a scalar) with every prompt of more than dense_min tokens entered through dense blocks
        (q3_generate_many_dense): the same rows for any dense_min; 0 runs the column loops unchanged.
        Returns (rows, ColsStats, DenseStats)."""
        ds = _DenseStats()
        rows, stats = self._generate_many(prompts, n_new, sampler, lambda rq, smp, out, st: self._batch_rc(
            self._lib.q3_generate_many_dense(*rq, *smp, int(dense_min), out, st, C.byref(ds))))[:2]
        return rows, stats, DenseStats(ds.blocks, ds.live_columns, ds.pad_columns)

    # ---- stop tokens in the device loop (include/qwen3_hip.h section 2h)
    cols_schedule_stop = staticmethod(cols_schedule_stop)

    def generate_many_stop(self, prompts, n_new, stop_tokens, sampler=None, raw: bool = False):
        """generate_many_greedy (sampler None) or generate_many_sampled (sampler = (temperature, topp, seeds), one value per
        request or a scalar) with every request ended on the device at its first token of stop_tokens (at most 8;
        q3_generate_many_stop): its slot goes to the next queued request at once, n_new[r] is a cap.  Returns (rows, ColsStats):
        row r holds the request's tokens up to and including the stop token, the stats count the passes actually run.
        raw=True: (the whole output buffer as the library filled it, n_out per request, ColsStats)."""
        return self._generate_many_stop(self._lib.q3_generate_many_stop, prompts, n_new, stop_tokens, sampler, raw)

    def _generate_many_stop(self, fn, prompts, n_new, stop_tokens, sampler, raw):
        def call(rq, smp, out, st):
            stop, n_out = [int(t) for t in stop_tokens], _size_array([0] * len(prompts))
            self._batch_rc(fn(*rq, *smp, _i32_array(stop), len(stop), out, n_out, st))
            return n_out
        rows, stats, out, got = self._generate_many(prompts, n_new, sampler, call)
        return (out, got, stats) if raw else (rows, stats)

    # ---- a shared prompt prefix (include/qwen3_hip.h section 2i)
    def batch_copy_rows(self, src_slot: int, dst_slots, first_pos: int, n_rows: int):
        """Key and value rows first_pos .. first_pos + n_rows - 1 of every layer of slot src_slot are copied into each slot of
        dst_slots by one kernel launch (q3_batch_copy_rows); nothing else changes.  What forking a prompt needs."""
        if first_pos < 0 or n_rows < 0:
            raise IndexError("negative index")
        self._batch_rc(self._lib.q3_batch_copy_rows(self._h, int(src_slot), _i32_array(dst_slots), len(dst_slots), first_pos, n_rows))

    def batch_prefix_set(self, tokens):
        """Make `tokens` the resident shared prefix (q3_batch_prefix_set): they are prefilled once at positions 0 .. into slot 0,
        whose rows 0 .. len(tokens) - 1 are overwritten, and kept in a store of their own for generate_many_prefix.  [] releases it."""
        self._batch_rc(self._lib.q3_batch_prefix_set(self._h, _i32_array(tokens), len(tokens)))

    def batch_prefix_get(self) -> List[int]:
        """The tokens of the resident shared prefix ([]: none)"""
        n = C.c_size_t(0)
        _check(self._lib.q3_batch_prefix_get(self._h, C.byref(n), None, 0))
        buf = (C.c_int32 * max(1, n.value))()
        _check(self._lib.q3_batch_prefix_get(self._h, C.byref(n), buf, n.value))
        return [int(buf[i]) for i in range(n.value)]

    def generate_many_prefix(self, suffixes, n_new, stop_tokens=(), sampler=None, raw: bool = False):
        """generate_many_stop for requests that all begin with the resident prefix (q3_generate_many_prefix): suffixes[r] is what
        follows the prefix in request r (at least one token).  The rows are those of generate_many_stop -- without stop tokens, of
        generate_many_greedy / generate_many_sampled -- on the full prompts prefix + suffixes[r]; the passes are those of the
        suffixes alone.  Arguments and return value as for generate_many_stop."""
        return self._generate_many_stop(self._lib.q3_generate_many_prefix, suffixes, n_new, stop_tokens, sampler, raw)

    # ---- stop sequences (include/qwen3_hip.h section 2t)
    cols_schedule_stop_seq = staticmethod(cols_schedule_stop_seq)

    def set_stop_sequences(self, automaton, start=None):
        """The stop automaton of every generate_many_stop / generate_many_prefix call (q3_stop_seq_set): a guide.SparseAutomaton (or
        anything with its default, offsets, tokens, targets and start) in which a target of -1 means "the sequence is complete": a
        request ends with the token that completes one, as it ends with a stop token (stops.stop_automaton and
        stops.stop_automaton_from_strings build them).  start: None for the automaton's own start state, one state for every
        request, or a sequence of one per request (-1: no stop sequences for that request); a call with another number of requests
        raises.  None turns it off (the default).  Only generated tokens move the state.  The setting is the engine's: it survives
        what set_guide_sparse survives, it is independent of guides, bias, penalties, logprobs and min_tokens, and the loops without
        a device scheduler (generate_many_greedy / _sampled / _dense) do not read it."""
        if automaton is None:
            _check(self._lib.q3_stop_seq_set(self._h, None, None, None, 0, 0, 0, None, 0))
            self._stop_seq = None
            return
        dflt, off, edges = _sparse_tables(automaton.default, automaton.offsets, automaton.tokens, automaton.targets)
        if start is None:
            start = automaton.start
        starts = [start] if isinstance(start, (int, np.integer)) and not isinstance(start, bool) else list(start)
        if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in starts):
            raise TypeError(f"start must be an integer or a sequence of integers, got {start!r}")
        if any(x < -1 or x > 0x7fffffff for x in starts):
            raise ValueError("a start state lies outside -1 .. 2^31 - 1")
        st = (C.c_int32 * max(len(starts), 1))(*starts)
        vocab = int(getattr(automaton, "vocab_size", self.get_config().vocab_size))      # another vocabulary than the engine's is refused
        _check(self._lib.q3_stop_seq_set(self._h, _void(dflt), _void(off), _void(edges), dflt.size, edges.size, vocab, st, len(starts)))
        self._stop_seq = (automaton, [int(x) for x in starts], (dflt.size, edges.size))

    def get_stop_sequences(self):
        """the engine's stop automaton as (automaton, start) in the form set_stop_sequences takes them; (None, []): none set.  The
        library holds the tables and tells their size (q3_stop_seq_get); the automaton is the object kept here."""
        n_states, n_edges, n_start = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        _check(self._lib.q3_stop_seq_get(self._h, C.byref(n_states), C.byref(n_edges), C.byref(n_start)))
        kept = getattr(self, "_stop_seq", None)
        have = (0, 0, 0) if kept is None else (kept[2][0], kept[2][1], len(kept[1]))
        if (int(n_states.value), int(n_edges.value), int(n_start.value)) != have:
            raise Q3Error(-5, "the engine's stop automaton was not set through this object")
        return (None, []) if kept is None else (kept[0], list(kept[1]))

    # ---- embeddings (include/qwen3_hip.h section 2j)
    def embed_many(self, prompts, normalize: bool = True, out_dim: Optional[int] = None, use_prefix: bool = False):
        """The last-token vectors of many prompts (q3_embed_many): row r is the final RMSNorm of prompts[r]'s last token, cut to its
        first out_dim components (None: dim) and, with normalize, L2-normalised.  The prompts go through the slots of batch_init
        in waves of dense blocks, from slot 0 up -- whatever the slots held is overwritten -- and no classifier runs.
        use_prefix: the prompts are suffixes behind the resident prefix of batch_prefix_set.
        Returns (float32 array [len(prompts), out_dim], EmbedStats)."""
        n = len(prompts)
        dim = self._config.dim
        if out_dim is not None and out_dim < 1:
            raise IndexError("out_dim must be at least 1")
        od = dim if out_dim is None else int(out_dim)
        flat = [int(t) for p in prompts for t in p]
        out = np.zeros((n, min(od, dim)), dtype=np.float32)
        st = _EmbedStats()
        flags = (EMBED_L2 if normalize else 0) | (EMBED_PREFIX if use_prefix else 0)
        self._batch_rc(self._lib.q3_embed_many(self._h, _i32_array(flat), _size_array([len(p) for p in prompts]), n, flags, od,
                                               out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
        return out, EmbedStats(st.waves, st.blocks, st.live_columns, st.pad_columns)

    # ---- choice logits (include/qwen3_hip.h section 2k)
    def choice_many(self, prompts, candidates, use_prefix: bool = False):
        """The logits of a few candidate tokens behind the last token of many prompts (q3_choice_many): out[r][j] is, bit for bit,
        forward(prompts[r][-1], len - 1)[candidates_r[j]] behind a prefill of the rest, with no classifier pass over the vocabulary.
        candidates: one list of token ids for every prompt, or one list per prompt, all of the same length k (1 .. CHOICE_MAX).
        The prompts go through the slots of batch_init as in embed_many, from slot 0 up -- whatever the slots held is overwritten.
        use_prefix: the prompts are suffixes behind the resident prefix of batch_prefix_set.
        Returns (float32 array [len(prompts), k], EmbedStats)."""
        n = len(prompts)
        cands = list(candidates)
        per_request = len(cands) > 0 and all(hasattr(c, "__len__") for c in cands)
        if per_request:
            if len(cands) != n:
                raise IndexError("one candidate list per prompt")
            k = len(cands[0])
            if any(len(c) != k for c in cands):
                raise IndexError("the candidate lists differ in length")
            ids = [int(t) for c in cands for t in c]
        else:
            k, ids = len(cands), [int(t) for t in cands]
        flat = [int(t) for p in prompts for t in p]
        out = np.zeros((n, k), dtype=np.float32)
        st = _EmbedStats()
        flags = (CHOICE_PREFIX if use_prefix else 0) | (CHOICE_PER_REQUEST if per_request else 0)
        self._batch_rc(self._lib.q3_choice_many(self._h, _i32_array(flat), _size_array([len(p) for p in prompts]), n, _i32_array(ids), k, flags,
                                                out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
        return out, EmbedStats(st.waves, st.blocks, st.live_columns, st.pad_columns)

    # ---- scores (include/qwen3_hip.h section 2l)
    def score_many(self, prompts, score_from=None, use_prefix: bool = False):
        """What the model says about every next token of many prompts (q3_score_many).  Request r of n tokens t gets
        n - score_from[r] records of SCORE_DTYPE: record j describes the logits l behind t[i], i = score_from[r] - 1 + j --
        target = l[t[i + 1]], max = the largest logit, sum = the sequential f32 sum of expf(l - max) over the vocabulary, argmax --
        target and sum bit for bit what forward() per position gives; log P(t[i + 1] | t[..i]) = (target - max) - log(sum)
        (generation.logprobs_of).  score_from: None (every position but the last is scored) or one value per prompt, 1 .. n.
        The prompts go through the slots of batch_init as in embed_many, from slot 0 up -- whatever the slots held is overwritten.
        use_prefix: the prompts are suffixes behind the resident prefix of batch_prefix_set.
        Returns (one SCORE_DTYPE array per request, ScoreStats)."""
        recs, _, _, stats = self._score(prompts, score_from, use_prefix, None)
        return recs, stats

    # ---- top-k log-probabilities (include/qwen3_hip.h section 2m)
    def score_top_many(self, prompts, k: int, score_from=None, use_prefix: bool = False):
        """score_many with the k most likely tokens of every scored position and the rank of its target (q3_score_top_many).
        Per request of n_r records: the SCORE_DTYPE records, bit for bit score_many's; an (n_r, k) array of TOP_DTYPE, column j
        the token of the j-th largest key ((total_order_key(logit) << 32) | index: ties in the logit go to the higher index, as
        for argmax) with its logit, bit for bit forward()'s; an int32 array of ranks, the number of tokens whose key exceeds the
        target's -- 0: the target is the argmax; rank < k: the target is column rank.  log P of an alternative is
        (logit - max) - log(sum) with the record's max and sum (generation.top_logprobs_of).  1 <= k <= SCORE_TOP_MAX, k <=
        vocab_size.  Everything else as score_many.
        Returns (records, tops, ranks, ScoreStats), the first three one array per request."""
        return self._score(prompts, score_from, use_prefix, int(k))

    def _score(self, prompts, score_from, use_prefix, k):
        """score_many (k None) and score_top_many: (records, tops, ranks, ScoreStats), tops and ranks None for k None"""
        n = len(prompts)
        lens = [len(p) for p in prompts]
        if score_from is not None:
            score_from = [int(v) for v in score_from]
            if len(score_from) != n:
                raise IndexError("one score_from per prompt")
        sf = [1] * n if score_from is None else score_from
        counts = [max(0, ln - f) if f >= 1 else 0 for ln, f in zip(lens, sf)]
        flat = [int(t) for p in prompts for t in p]
        out = np.zeros(sum(counts), dtype=SCORE_DTYPE)
        st = _ScoreStats()
        args = (self._h, _i32_array(flat), _size_array(lens), n, None if score_from is None else _size_array(score_from), SCORE_PREFIX if use_prefix else 0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        top = rank = None
        if k is not None:
            top = np.zeros((out.size, max(0, min(k, SCORE_TOP_MAX))), dtype=TOP_DTYPE)
            rank = np.zeros(out.size, dtype=np.int32)
            self._batch_rc(self._lib.q3_score_top_many(*args, k, ptr(out), ptr(top), ptr(rank), C.byref(st)))
        else:
            self._batch_rc(self._lib.q3_score_many(*args, ptr(out), C.byref(st)))
        ends = np.cumsum([0] + counts)
        cut = lambda a: None if a is None else [a[ends[r]:ends[r + 1]] for r in range(n)]
        return cut(out), cut(top), cut(rank), ScoreStats(st.waves, st.blocks, st.live_columns, st.pad_columns, st.chunks, st.scored)

    # ---- log-probabilities of generated tokens (include/qwen3_hip.h section 2o)
    def set_gen_logprobs(self, top_n: int):
        """Records of the tokens every generate_many_* call produces (q3_gen_logprobs): -1 turns them off (the default), 0 takes one
        SCORE_DTYPE record per generated token, 1 .. SCORE_TOP_MAX also the top_n most likely tokens and the token's rank.  The
        records are score_many's on prompt + output -- the raw logits, in front of temperature, top-k and top-p -- taken inside
        the loop; the tokens are the same with the setting on or off.  The setting is the engine's: it survives set_sampler,
        batch_init and every generate_many call, and it does not touch batch_step_cols, forward_batch, verify or single-stream decode."""
        _check_gen_logprobs(top_n, self._config.vocab_size)
        _check(self._lib.q3_gen_logprobs(self._h, int(top_n)))
        self._gen_lp = int(top_n)

    def get_gen_logprobs(self) -> int:
        """the engine's setting (q3_gen_logprobs_get); -1: off"""
        out = C.c_int(-1)
        _check(self._lib.q3_gen_logprobs_get(self._h, C.byref(out)))
        return int(out.value)

    # ---- presence and frequency penalties (include/qwen3_hip.h section 2p)
    def set_penalties(self, presence: float, frequency: float):
        """Presence and frequency penalties of every generate_many_* call (q3_sampler_penalties): a token the request has produced c > 0
        times has presence + frequency * c taken off its logit before the argmax or the draw; prompt tokens do not count.  (0, 0)
        turns them off (the default).  The setting is the engine's: it survives set_sampler, batch_init, set_top_k, set_gen_logprobs
        and every generate_many call, and it does not touch batch_step_cols, forward_batch, verify or single-stream decode."""
        _check_penalties(presence, frequency)
        _check(self._lib.q3_sampler_penalties(self._h, float(presence), float(frequency)))

    def get_penalties(self):
        """the engine's (presence, frequency) (q3_sampler_get_penalties); (0.0, 0.0): off"""
        p, f = C.c_float(0.0), C.c_float(0.0)
        _check(self._lib.q3_sampler_get_penalties(self._h, C.byref(p), C.byref(f)))
        return float(p.value), float(f.value)

    # ---- logit bias, banned and allowed tokens (include/qwen3_hip.h section 2q)
    def set_logit_bias(self, lists, modes=None):
        """The table of every generate_many_* call (q3_logit_bias_set).  lists: [] turns it off (the default); one list holds for every
        request of every call; several, list r belongs to request r and a call with another number of requests raises.  A list is a
        dict {token: bias} or a sequence of (token, bias[, until]): an entry acts on a request's output g while until == 0 or
        g < until; bias is added to the token's logit before the penalties, the argmax or the draw; -inf bans the token.  modes: per
        list BIAS_ADD (unlisted tokens keep their logits; the default) or BIAS_ALLOW (unlisted tokens become -inf).  The setting is
        the engine's: it survives set_sampler, batch_init, set_top_k, set_gen_logprobs, set_penalties and every generate_many call,
        and it does not touch batch_step_cols, forward_batch, verify, score, choose, embed or single-stream decode."""
        lists, modes = _check_bias_table(lists, modes)
        flat = _bias_array([x for l in lists for x in l])
        n = (C.c_size_t * max(len(lists), 1))(*[len(l) for l in lists])
        m = (C.c_uint8 * max(len(lists), 1))(*modes)
        _check(self._lib.q3_logit_bias_set(self._h, flat.ctypes.data_as(C.c_void_p) if flat.size else None, n, m, len(lists)))
        self._logit_bias = (lists, modes)

    def get_logit_bias(self):
        """the engine's table as (lists, modes) in the form set_logit_bias takes them, every list [(token, bias, until)] sorted by token;
        ([], []): off.  The library holds the table and tells its size (q3_logit_bias_get); the lists are the copy kept here."""
        n_lists, n_total = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib.q3_logit_bias_get(self._h, C.byref(n_lists), C.byref(n_total)))
        lists, modes = getattr(self, "_logit_bias", ([], []))
        if (int(n_lists.value), int(n_total.value)) != (len(lists), sum(len(l) for l in lists)):
            raise Q3Error(-5, "the engine's logit-bias table was not set through this object")
        return [list(l) for l in lists], list(modes)

    # ---- guided decoding (include/qwen3_hip.h section 2r)
    def set_guide(self, next, start):
        """The guide of every generate_many_* call (q3_guide_set).  next: a table [n_states][vocab_size] of integers, next[s][v] >= 0:
        in state s token v may come and leads to that state, -1: it may not (guide.Automaton builds such tables); None or an empty
        table turns the guide off (the default).  start: one state for every request of every call, or a sequence of one per request
        (-1: that request is unguided), and a call with another number of requests raises.  In state s a request's next token is
        taken from its row with the forbidden tokens at -inf, in front of set_logit_bias and set_penalties; the committed token
        moves the state.  The setting is the engine's: it survives set_sampler, batch_init, set_top_k, set_gen_logprobs,
        set_penalties, set_logit_bias and every generate_many call, and it does not touch batch_step_cols, forward_batch, verify,
        score, choose, embed or single-stream decode."""
        if next is None or np.size(next) == 0:
            _check(self._lib.q3_guide_set(self._h, None, 0, 0, None, 0))
            self._guide, self._guide_sparse = (None, []), None
            return
        table = np.asarray(next)
        if table.ndim != 2 or not np.issubdtype(table.dtype, np.integer):
            raise TypeError("next must be an integer table [n_states][vocab_size]")
        if table.min() < -1 or table.max() > 0x7fff:
            raise ValueError("an entry of next lies outside -1 .. 32767")
        table = np.ascontiguousarray(table, dtype=np.int16)
        starts = [start] if isinstance(start, (int, np.integer)) and not isinstance(start, bool) else list(start)
        if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in starts):
            raise TypeError(f"start must be an integer or a sequence of integers, got {start!r}")
        if any(x < -1 or x > 0x7fffffff for x in starts):
            raise ValueError("a start state lies outside -1 .. 2^31 - 1")
        st = (C.c_int32 * max(len(starts), 1))(*starts)
        _check(self._lib.q3_guide_set(self._h, table.ctypes.data_as(C.c_void_p), table.shape[0], table.shape[1], st, len(starts)))
        self._guide = (table, [int(x) for x in starts])
        self._guide_sparse = None

    # ---- sparse guides (include/qwen3_hip.h section 2s)
    def set_guide_sparse(self, default, offsets, tokens, targets, start):
        """The guide of every generate_many_* call in its sparse form (q3_guide_set_sparse): the rule of set_guide with next[s][v]
        stated as default[s] for every token state s does not list, and targets[k] for tokens[k], offsets[s] <= k < offsets[s + 1]
        (guide.SparseAutomaton holds such arrays).  Up to GUIDE_SPARSE_MAX_STATES states.  start, what the guide holds for and what
        it survives are set_guide's.  One guide holds at a time: this call clears a guide of set_guide and the other way round;
        default None or empty turns both off."""
        if default is None or np.size(default) == 0:
            _check(self._lib.q3_guide_set_sparse(self._h, None, None, None, 0, 0, 0, None, 0))
            self._guide, self._guide_sparse = (None, []), None
            return
        arrays = []
        for name, a in (("default", default), ("offsets", offsets), ("tokens", tokens), ("targets", targets)):
            a = np.asarray(a)
            if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
                raise TypeError(f"{name} must be a vector of integers")
            if a.size and (a.min() < -1 or a.max() > 0x7fffffff):
                raise ValueError(f"an entry of {name} lies outside -1 .. 2^31 - 1")
            arrays.append(a)
        default, offsets, tokens, targets = arrays
        if offsets.size != default.size + 1 or tokens.size != targets.size or (offsets.size and offsets.min() < 0):
            raise ValueError("offsets must hold one entry more than default, none negative, and tokens as many as targets")
        dflt = np.ascontiguousarray(default, dtype=np.int32)
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        edges = np.empty(tokens.size, dtype=EDGE_DTYPE)
        edges["token"], edges["next"] = tokens, targets
        starts = [start] if isinstance(start, (int, np.integer)) and not isinstance(start, bool) else list(start)
        if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in starts):
            raise TypeError(f"start must be an integer or a sequence of integers, got {start!r}")
        if any(x < -1 or x > 0x7fffffff for x in starts):
            raise ValueError("a start state lies outside -1 .. 2^31 - 1")
        st = (C.c_int32 * max(len(starts), 1))(*starts)
        _check(self._lib.q3_guide_set_sparse(self._h, dflt.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                                             edges.ctypes.data_as(C.c_void_p) if edges.size else None, dflt.size, edges.size,
                                             self.get_config().vocab_size, st, len(starts)))
        self._guide_sparse = (dflt, off.astype(np.int64), edges["token"].copy(), edges["next"].copy(), [int(x) for x in starts])
        self._guide = (None, [])

    def get_guide_sparse(self):
        """the engine's sparse guide as (default, offsets, tokens, targets, start) in the form set_guide_sparse takes them;
        (None, None, None, None, []): none set.  The library holds the guide and tells its size (q3_guide_get_sparse); the arrays are
        the copy kept here."""
        n_states, n_edges, n_start = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        _check(self._lib.q3_guide_get_sparse(self._h, C.byref(n_states), C.byref(n_edges), C.byref(n_start)))
        kept = getattr(self, "_guide_sparse", None)
        have = (0, 0, 0) if kept is None else (kept[0].size, kept[2].size, len(kept[4]))
        if (int(n_states.value), int(n_edges.value), int(n_start.value)) != have:
            raise Q3Error(-5, "the engine's sparse guide was not set through this object")
        return (None, None, None, None, []) if kept is None else (kept[0], kept[1], kept[2], kept[3], list(kept[4]))

    def get_guide(self):
        """the engine's guide as (next, start) in the form set_guide takes them; (None, []): off.  The library holds the guide and
        tells its size (q3_guide_get); the arrays are the copy kept here."""
        n_states, n_start = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib.q3_guide_get(self._h, C.byref(n_states), C.byref(n_start)))
        table, starts = getattr(self, "_guide", (None, []))
        if (int(n_states.value), int(n_start.value)) != (0 if table is None else table.shape[0], len(starts)):
            raise Q3Error(-5, "the engine's guide was not set through this object")
        return table, list(starts)

    def read_gen_logprobs(self, n_per_row=None):
        """The records of the last generate_many_* call (q3_gen_logprobs_read), which ran under set_gen_logprobs(top_n >= 0): per
        request (records, tops, ranks) -- SCORE_DTYPE[n], TOP_DTYPE[n, top_n], int32[n], entry j for the request's j-th token; tops
        has no columns and ranks is empty where the call ran with top_n 0.  n_per_row: entries wanted per request (None: as many
        as the call gave the request tokens; more than that reads the zero bytes behind a request that ended early)."""
        cap, got, k = getattr(self, "_gen_last", ([], [], -1))
        want = got if n_per_row is None else [int(v) for v in n_per_row]
        if len(want) != len(cap) or any(w < 0 or w > c for w, c in zip(want, cap)):
            raise IndexError("n_per_row: one count per request of the last call, at most its n_new")
        total = sum(cap)
        recs = np.zeros(total, dtype=SCORE_DTYPE)
        top = np.zeros((total, max(k, 0)), dtype=TOP_DTYPE)
        rank = np.zeros(total if k > 0 else 0, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        self._batch_rc(self._lib.q3_gen_logprobs_read(self._h, 0, total, recs.ctypes.data_as(C.c_void_p), ptr(top), ptr(rank)))
        out, at = [], 0
        for c, w in zip(cap, want):
            out.append((recs[at:at + w], top[at:at + w], rank[at:at + w] if k > 0 else rank[:0]))
            at += c
        return out

    def set_batch_sampler(self, temperature: float, topp: float, rng_seeds):
        """one Sampler per stream (sampler.rs:29-42), stream i seeded with rng_seeds[i]; temperature 0 = greedy"""
        seeds = (C.c_uint64 * 32)(*([int(s) for s in rng_seeds] + [0] * (32 - len(rng_seeds))))
        _check(self._lib.q3_batch_sampler_set(self._h, temperature, topp, seeds))

    def batch_reset_kv(self):
        _check(self._lib.q3_batch_reset_kv(self._h))

    def batch_read_state(self, stream: int, kind: str, offset: int = 0, count: Optional[int] = None) -> np.ndarray:
        c = self._config
        kinds = {"key": 0, "value": 1, "x": 2}
        total = c.dim if kind == "x" else c.n_layers * self._batch_ctx * c.n_kv_heads * c.head_dim
        count = total - offset if count is None else count
        out = np.zeros(count, dtype=np.float32)
        _check(self._lib.q3_batch_read_state(self._h, stream, kinds[kind], offset, count, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def profile(self, token: int, pos: int, reps: int = 1):
        """Per kernel-family (name, total ms, launches) over `reps` eager forwards, HIP events on the engine stream."""
        cap = 16
        ms = (C.c_float * cap)()
        n = (C.c_int32 * cap)()
        k = self._lib.q3_profile(self._h, token, pos, reps, ms, n, cap)
        if k < 0:
            _check(k)
        return [(self._lib.q3_profile_name(i).decode(), float(ms[i]), int(n[i])) for i in range(k)]

    def close(self):
        if self._h:
            self._lib.q3_destroy(self._h)
            self._h = C.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TransformerBuilder:
    """models/mod.rs:40-74: TransformerBuilder::new(path).with_ctx_length(Some(n)).build()"""

    def __init__(self, checkpoint_path: str):
        self.checkpoint_path = checkpoint_path
        self.ctx_length: Optional[int] = None
        self.device = int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("Q3_DEVICE_FROM_RANK") else 0
        # Q3_EAGER_LAUNCH=1: launch kernels eagerly instead of replaying hipGraphs (profiling runs: rocprofv3's kernel trace
        # of this ROCm build crashes on long back-to-back graph replays)
        self.flags = FLAG_NO_GRAPH if os.environ.get("Q3_EAGER_LAUNCH") else 0

    def with_ctx_length(self, ctx_length: Optional[int]) -> "TransformerBuilder":
        self.ctx_length = ctx_length
        return self

    def with_device(self, device: int) -> "TransformerBuilder":
        self.device = device
        return self

    def with_strict(self, strict: bool = True) -> "TransformerBuilder":
        """strict (default): reference summation order, bit-identical logits.  False: tree reductions."""
        self.flags = (self.flags & ~FLAG_FAST) if strict else (self.flags | FLAG_FAST)
        return self

    def with_value_transposed(self, keep: bool = True) -> "TransformerBuilder":
        """keep (default): contexts past 256 positions hold the value cache twice (row-major + transposed, include/qwen3_hip.h
        Q3_FLAG_NO_VALUE_T has the byte counts).  False: the row-major cache only; same results, slower long-context decode."""
        self.flags = (self.flags & ~FLAG_NO_VALUE_T) if keep else (self.flags | FLAG_NO_VALUE_T)
        return self

    def with_graph(self, graph: bool = True) -> "TransformerBuilder":
        self.flags = (self.flags & ~FLAG_NO_GRAPH) if graph else (self.flags | FLAG_NO_GRAPH)
        return self

    def build(self) -> Transformer:
        L = load_library()
        h = C.c_void_p()
        rc = L.q3_create(self.checkpoint_path.encode(), int(self.ctx_length or 0), self.device, self.flags, C.byref(h))
        _check(rc)
        return Transformer(h.value, L)


class _Ops:
    """The reference's public free functions (tensor.rs / layers.rs) executed by the device kernels."""

    def __init__(self, device: int = 0):
        self.device = device

    @staticmethod
    def _fp(a):
        return a.ctypes.data_as(C.POINTER(C.c_float))

    @staticmethod
    def _i8(a):
        return a.ctypes.data_as(C.POINTER(C.c_int8))

    def quantize(self, x, group_size: int) -> Tuple[np.ndarray, np.ndarray]:
        x = np.ascontiguousarray(x, dtype=np.float32)
        q = np.zeros(x.size, dtype=np.int8)
        s = np.zeros(max(1, x.size // group_size), dtype=np.float32)
        _check(load_library().q3_op_quantize(self._i8(q), self._fp(s), self._fp(x), x.size, group_size, self.device))
        return q, s[: x.size // group_size]

    def dequantize(self, q, s, group_size: int) -> np.ndarray:
        q = np.ascontiguousarray(q, dtype=np.int8)
        s = np.ascontiguousarray(s, dtype=np.float32)
        x = np.zeros(q.size, dtype=np.float32)
        _check(load_library().q3_op_dequantize(self._i8(q), self._fp(s), self._fp(x), q.size, group_size, self.device))
        return x

    def matmul(self, xq, xs, wq, ws, n: int, d: int, group_size: int) -> np.ndarray:
        xq = np.ascontiguousarray(xq, dtype=np.int8)
        xs = np.ascontiguousarray(xs, dtype=np.float32)
        wq = np.ascontiguousarray(wq, dtype=np.int8)
        ws = np.ascontiguousarray(ws, dtype=np.float32)
        out = np.zeros(d, dtype=np.float32)
        _check(load_library().q3_op_matmul(self._fp(out), self._i8(xq), self._fp(xs), self._i8(wq), self._fp(ws), n, d,
                                           group_size, self.device))
        return out

    def gemv_role(self, role: int, wq, ws, n: int, rows: int, group_size: int, x=None, norm_w=None, pre_q=None, pre_s=None,
                  out=None, rows_kv: int = 0, head_dim: int = 0, strict: bool = True) -> dict:
        """one fused GEMV launch of the decode plan (q3_op_gemv_role; role = ROLE_*).  Returns {"out", "tap" (NORM roles),
        "argmax" (LOGITS), "info": [table entry?, grid, threads per workgroup, rows per wave batch]}."""
        wq = np.ascontiguousarray(wq, dtype=np.int8)
        ws = np.ascontiguousarray(ws, dtype=np.float32)
        n_out = rows + 2 * rows_kv if role == ROLE_NORM_QKV else rows
        n_w = n_out if role != ROLE_NORM_SWIGLU else 2 * rows
        if wq.size != n_w * n or ws.size != n_w * (n // group_size):
            raise ValueError(f"weights: {n_w} rows of {n} expected")
        norm = role in (ROLE_NORM_QKV, ROLE_NORM_SWIGLU, ROLE_NORM_LOGITS)
        o = np.zeros(n_out, dtype=np.float32) if out is None else np.array(out, dtype=np.float32, copy=True)
        if o.size != n_out:
            raise ValueError("out: one float per output row")
        null_f, null_b = C.POINTER(C.c_float)(), C.POINTER(C.c_int8)()
        keep = []

        def f32(a, size):
            if a is None:
                return null_f
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.size != size:
                raise ValueError(f"{size} floats expected, got {a.size}")
            keep.append(a)
            return self._fp(a)

        def i32(a):
            return a.ctypes.data_as(C.POINTER(C.c_int32))
        pq = null_b
        if pre_q is not None:
            pre_q = np.ascontiguousarray(pre_q, dtype=np.int8)
            if pre_q.size != n:
                raise ValueError("pre_q: n int8 expected")
            pq = self._i8(pre_q)
        tap = np.zeros(n, dtype=np.float32) if norm else None
        am = np.full(1, -1, dtype=np.int32)
        info = np.zeros(4, dtype=np.int32)
        _check(load_library().q3_op_gemv_role(role, self._fp(o), self._fp(tap) if norm else null_f, i32(am), i32(info),
                                              f32(x, n), f32(norm_w, n), pq, f32(pre_s, n // group_size), self._i8(wq),
                                              self._fp(ws), n, rows, rows_kv, head_dim, group_size,
                                              0 if strict else FLAG_FAST, self.device))
        return {"out": o, "tap": tap, "argmax": int(am[0]), "info": [int(v) for v in info]}

    def rmsnorm(self, x, w, strict: bool = True) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        w = np.ascontiguousarray(w, dtype=np.float32)
        out = np.zeros_like(x)
        _check(load_library().q3_op_rmsnorm(self._fp(out), self._fp(x), self._fp(w), x.size,
                                            0 if strict else FLAG_FAST, self.device))
        return out

    def softmax(self, a, strict: bool = True) -> np.ndarray:
        a = np.array(a, dtype=np.float32, copy=True)
        _check(load_library().q3_op_softmax(self._fp(a), a.size, 0 if strict else FLAG_FAST, self.device))
        return a

    def swiglu(self, g, u) -> np.ndarray:
        g = np.array(g, dtype=np.float32, copy=True)
        u = np.ascontiguousarray(u, dtype=np.float32)
        _check(load_library().q3_op_swiglu(self._fp(g), self._fp(u), g.size, self.device))
        return g

    def expf(self, x) -> np.ndarray:
        x = np.array(x, dtype=np.float32, copy=True)
        _check(load_library().q3_op_expf(self._fp(x), x.size, self.device))
        return x

    def attention(self, q, key_layer, value_layer, q_norm_w, k_norm_w, pos, n_heads, n_kv_heads, head_dim,
                  strict: bool = True):
        q = np.array(q, dtype=np.float32, copy=True)
        k = np.array(key_layer, dtype=np.float32, copy=True)
        v = np.ascontiguousarray(value_layer, dtype=np.float32)
        seq_len = k.size // (n_kv_heads * head_dim)
        xb = np.zeros(n_heads * head_dim, dtype=np.float32)
        qw = np.ascontiguousarray(q_norm_w, dtype=np.float32)
        kw = np.ascontiguousarray(k_norm_w, dtype=np.float32)
        _check(load_library().q3_op_attention(self._fp(xb), self._fp(q), self._fp(k), self._fp(v), self._fp(qw),
                                              self._fp(kw), pos, seq_len, n_heads, n_kv_heads, head_dim,
                                              0 if strict else FLAG_FAST, self.device))
        return xb, q, k

    def argmax(self, logits) -> int:
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        out = C.c_int32(-1)
        _check(load_library().q3_op_argmax(self._fp(logits), logits.size, C.byref(out), self.device))
        return int(out.value)

    def sample(self, logits, temperature: float, topp: float, rng_state: int):
        """one Sampler::sample draw on the device; returns (token, new rng_state)"""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        out, st = C.c_int32(-1), C.c_uint64(rng_state)
        _check(load_library().q3_op_sample(self._fp(logits), logits.size, temperature, topp, C.byref(st), C.byref(out), self.device))
        return int(out.value), int(st.value)

    def sample_top_k(self, logits, temperature: float, topp: float, top_k: int, rng_state: int):
        """one Sampler::sample draw among the top_k largest logits on the device (q3_op_sample_top_k); returns (token, new rng_state)"""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        _check_top_k(top_k, 1, logits.size)
        out, st = C.c_int32(-1), C.c_uint64(rng_state)
        _check(load_library().q3_op_sample_top_k(self._fp(logits), logits.size, temperature, topp, top_k, C.byref(st), C.byref(out), self.device))
        return int(out.value), int(st.value)

    def penalize(self, logits, counts, presence: float, frequency: float):
        """The penalised row of include/qwen3_hip.h section 2p on the device (q3_op_penalize): l' = l where counts is 0, else
        l - (presence + frequency * counts), every step rounded to f32.  Returns (l' as float32[n], the index of its largest key)."""
        _check_penalties(presence, frequency)
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        if logits.ndim != 1 or logits.shape != counts.shape or logits.size == 0:
            raise ValueError("logits and counts must be non-empty vectors of one length")
        out, idx = np.empty_like(logits), C.c_int32(-1)
        _check(load_library().q3_op_penalize(self._fp(logits), counts.ctypes.data_as(C.POINTER(C.c_uint32)), logits.size, float(presence),
                                             float(frequency), self._fp(out), C.byref(idx), self.device))
        return out, int(idx.value)

    def logit_bias(self, logits, entries, mode: int = BIAS_ADD, g: int = 0, counts=None, presence: float = 0.0, frequency: float = 0.0):
        """The adjusted row of include/qwen3_hip.h section 2q on the device (q3_op_logit_bias): the list `entries` (set_logit_bias's
        form) under `mode` for a request's output index g, then with counts the penalties of section 2p on top.  Returns (the row as
        float32[n], the index of its largest key)."""
        ent = _check_bias_list(entries, mode, "entries")
        _check_penalties(presence, frequency)
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
            raise TypeError(f"g must be an integer, got {g!r}")
        if g < 0 or g > 0xffffffff:
            raise ValueError(f"g {g} out of range")
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        if logits.ndim != 1 or logits.size == 0:
            raise ValueError("logits must be a non-empty vector")
        cp = None
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.uint32)
            if counts.shape != logits.shape:
                raise ValueError("logits and counts must be vectors of one length")
            cp = counts.ctypes.data_as(C.POINTER(C.c_uint32))
        if any(t >= logits.size for t, _, _ in ent):
            raise ValueError(f"a token of the list lies outside the {logits.size} logits")
        flat = _bias_array(ent)
        out, idx = np.empty_like(logits), C.c_int32(-1)
        _check(load_library().q3_op_logit_bias(self._fp(logits), logits.size, flat.ctypes.data_as(C.c_void_p) if flat.size else None, len(ent), int(mode),
                                               int(g), cp, float(presence), float(frequency), self._fp(out), C.byref(idx), self.device))
        return out, int(idx.value)

    def guide(self, logits, next_row, entries=(), mode: int = BIAS_ADD, g: int = 0, counts=None, presence: float = 0.0, frequency: float = 0.0):
        """The masked row of include/qwen3_hip.h section 2r on the device (q3_op_guide): tokens whose entry of `next_row` (one state's
        row of a guide's table) is negative become -inf, then the list `entries` under `mode` for output index g and, with counts,
        the penalties apply as in ops.logit_bias.  Returns (the row as float32[n], the index of its largest key)."""
        ent = _check_bias_list(entries, mode, "entries")
        _check_penalties(presence, frequency)
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
            raise TypeError(f"g must be an integer, got {g!r}")
        if g < 0 or g > 0xffffffff:
            raise ValueError(f"g {g} out of range")
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        if logits.ndim != 1 or logits.size == 0:
            raise ValueError("logits must be a non-empty vector")
        next_row = np.asarray(next_row)
        if next_row.shape != logits.shape or not np.issubdtype(next_row.dtype, np.integer):
            raise ValueError("next_row must be an integer vector of the length of logits")
        if next_row.min() < -0x8000 or next_row.max() > 0x7fff:
            raise ValueError("an entry of next_row does not fit int16")
        next_row = np.ascontiguousarray(next_row, dtype=np.int16)
        cp = None
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.uint32)
            if counts.shape != logits.shape:
                raise ValueError("logits and counts must be vectors of one length")
            cp = counts.ctypes.data_as(C.POINTER(C.c_uint32))
        if any(t >= logits.size for t, _, _ in ent):
            raise ValueError(f"a token of the list lies outside the {logits.size} logits")
        flat = _bias_array(ent)
        out, idx = np.empty_like(logits), C.c_int32(-1)
        _check(load_library().q3_op_guide(self._fp(logits), logits.size, next_row.ctypes.data_as(C.c_void_p),
                                          flat.ctypes.data_as(C.c_void_p) if flat.size else None, len(ent), int(mode), int(g), cp, float(presence),
                                          float(frequency), self._fp(out), C.byref(idx), self.device))
        return out, int(idx.value)

    def guide_sparse(self, logits, default, tokens=(), targets=(), entries=(), mode: int = BIAS_ADD, g: int = 0, counts=None, presence: float = 0.0,
                     frequency: float = 0.0):
        """ops.guide with the state's row in the sparse statement of section 2s (q3_op_guide_sparse): token tokens[k] does targets[k],
        every other token does `default`; negative: forbidden.  tokens ascend strictly.  Returns (the row as float32[n], the index of
        its largest key)."""
        ent = _check_bias_list(entries, mode, "entries")
        _check_penalties(presence, frequency)
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
            raise TypeError(f"g must be an integer, got {g!r}")
        if g < 0 or g > 0xffffffff:
            raise ValueError(f"g {g} out of range")
        if isinstance(default, bool) or not isinstance(default, (int, np.integer)):
            raise TypeError(f"default must be an integer, got {default!r}")
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        if logits.ndim != 1 or logits.size == 0:
            raise ValueError("logits must be a non-empty vector")
        tokens, targets = np.asarray(tokens), np.asarray(targets)
        if tokens.ndim != 1 or tokens.shape != targets.shape or (tokens.size and not (np.issubdtype(tokens.dtype, np.integer) and np.issubdtype(targets.dtype, np.integer))):
            raise ValueError("tokens and targets must be integer vectors of one length")
        if tokens.size and (tokens.min() < 0 or tokens.max() >= logits.size or (np.diff(tokens) <= 0).any()):
            raise ValueError(f"tokens must ascend strictly inside the {logits.size} logits")
        if not -1 <= default < GUIDE_SPARSE_MAX_STATES or (targets.size and (targets.min() < -1 or targets.max() >= GUIDE_SPARSE_MAX_STATES)):
            raise ValueError(f"default or a target lies outside -1 .. {GUIDE_SPARSE_MAX_STATES - 1}")
        edges = np.empty(tokens.size, dtype=EDGE_DTYPE)
        edges["token"], edges["next"] = tokens, targets
        cp = None
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.uint32)
            if counts.shape != logits.shape:
                raise ValueError("logits and counts must be vectors of one length")
            cp = counts.ctypes.data_as(C.POINTER(C.c_uint32))
        if any(t >= logits.size for t, _, _ in ent):
            raise ValueError(f"a token of the list lies outside the {logits.size} logits")
        flat = _bias_array(ent)
        out, idx = np.empty_like(logits), C.c_int32(-1)
        _check(load_library().q3_op_guide_sparse(self._fp(logits), logits.size, int(default), edges.ctypes.data_as(C.c_void_p) if edges.size else None,
                                                 edges.size, flat.ctypes.data_as(C.c_void_p) if flat.size else None, len(ent), int(mode), int(g), cp,
                                                 float(presence), float(frequency), self._fp(out), C.byref(idx), self.device))
        return out, int(idx.value)

    def stop_seq(self, default, offsets, tokens, targets, vocab_size: int, start_state: int, stream):
        """One token stream over a stop automaton, on the host with the step function the device loop calls (q3_op_stop_seq): from
        start_state, token after token until next[state][token] is -1.  Returns (n_emit, end_state): the index of the completing
        token + 1 or len(stream), and the state behind the last token stepped or -1 on a match."""
        dflt, off, edges = _sparse_tables(default, offsets, tokens, targets)
        toks = [int(t) for t in stream]
        n_emit, end = C.c_size_t(0), C.c_int32(0)
        _check(load_library().q3_op_stop_seq(_void(dflt), _void(off), _void(edges), dflt.size, edges.size, int(vocab_size), int(start_state),
                                             _i32_array(toks) if toks else None, len(toks), C.byref(n_emit), C.byref(end)))
        return int(n_emit.value), int(end.value)


ops = _Ops()


def op_sample_top_k(logits, temperature: float, topp: float, top_k: int, rng_state: int):
    """ops.sample_top_k: the operator entry of top-k sampling, beside ops.sample"""
    return ops.sample_top_k(logits, temperature, topp, top_k, rng_state)
