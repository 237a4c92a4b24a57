"""qwen3_rs_amd -- MI355X (gfx950) Qwen3 Q8 decode engine behind qwen3-rs's `Transformer` surface.

Host-side mirror (ctypes over the C ABI in include/qwen3_hip.h) of the reference interface for the hot
path only:  TransformerBuilder / Transformer.forward / get_config  (qwen3-inference/src/models/mod.rs),
the free functions of tensor.rs / layers.rs, the `generate` / `chat` call patterns (generation.rs) and
the checkpoint format (qwen3-export/src/model_exporter.rs).  All compute runs in libqwen3_hip.so
(hand-written HIP kernels); there is no CPU fallback -- loading fails loudly if the library is missing.
"""
from .engine import (Q3Error, ModelConfig, Transformer, TransformerBuilder, lib_path, dev_lib_path, load_library, use_library, ops,
                     FLAG_FAST, FLAG_NO_GRAPH, FLAG_NO_VALUE_T, EXPORTED_SYMBOLS, source_build_id, SpecStats, VERIFY_MAX, lookup_draft,
                     lookup_trace, ColsStats, COLS_MAX, cols_schedule, DenseStats, dense_pack, STOP_MAX, cols_schedule_stop, EmbedStats,
                     EMBED_L2, EMBED_PREFIX, CHOICE_PREFIX, CHOICE_PER_REQUEST, CHOICE_MAX, ScoreStats, SCORE_PREFIX, SCORE_DTYPE, score_pack,
                     SCORE_TOP_MAX, TOP_DTYPE, TOP_K_MAX, op_sample_top_k, BIAS_MAX, BIAS_ADD, BIAS_ALLOW, BIAS_DTYPE, GUIDE_MAX_STATES,
                     GUIDE_SPARSE_MAX_STATES, GUIDE_SPARSE_MAX_EDGES, EDGE_DTYPE, STOP_SEQ_MAX_STATES, STOP_SEQ_MAX_EDGES,
                     cols_schedule_stop_seq)
from .generation import (generate, chat_turn, generate_many, embed, common_prefix_len, TokenMetrics, sample_argmax, choose, rerank,
                         normalise_logits, RERANK_TEMPLATE, RERANK_INSTRUCTION, score, loglikelihood, perplexity, logprobs_of,
                         top_logprobs, top_logprobs_of, merge_logit_bias)
from . import checkpoint
from . import guide
from .guide import Automaton, SparseAutomaton, regex_dfa
from . import stops
from .stops import stop_automaton, stop_automaton_from_strings, cut_at_stop

__all__ = ["GUIDE_MAX_STATES", "GUIDE_SPARSE_MAX_STATES", "GUIDE_SPARSE_MAX_EDGES", "EDGE_DTYPE", "guide", "Automaton", "SparseAutomaton", "regex_dfa", "BIAS_MAX", "BIAS_ADD", "BIAS_ALLOW", "BIAS_DTYPE", "merge_logit_bias", "Q3Error", "ModelConfig", "Transformer", "TransformerBuilder", "lib_path", "dev_lib_path", "load_library", "use_library", "ops",
           "FLAG_FAST", "FLAG_NO_GRAPH", "FLAG_NO_VALUE_T", "EXPORTED_SYMBOLS", "source_build_id", "generate", "chat_turn", "TokenMetrics",
           "sample_argmax", "checkpoint", "SpecStats", "VERIFY_MAX", "lookup_draft", "lookup_trace",
           "ColsStats", "COLS_MAX", "cols_schedule", "generate_many", "DenseStats", "dense_pack",
           "STOP_MAX", "cols_schedule_stop", "common_prefix_len", "embed", "EmbedStats", "EMBED_L2", "EMBED_PREFIX",
           "CHOICE_PREFIX", "CHOICE_PER_REQUEST", "CHOICE_MAX", "choose", "rerank", "normalise_logits", "RERANK_TEMPLATE", "RERANK_INSTRUCTION",
           "ScoreStats", "SCORE_PREFIX", "SCORE_DTYPE", "score_pack", "score", "loglikelihood", "perplexity", "logprobs_of",
           "SCORE_TOP_MAX", "TOP_DTYPE", "top_logprobs", "top_logprobs_of", "TOP_K_MAX", "op_sample_top_k",
           "STOP_SEQ_MAX_STATES", "STOP_SEQ_MAX_EDGES", "cols_schedule_stop_seq", "stops", "stop_automaton", "stop_automaton_from_strings",
           "cut_at_stop"]
