"""The requests of the shared-prefix tests (include/qwen3_hip.h section 2i): a prefix of P tokens in front of the suffixes of
cols_stop_cases.prompts, on the shapes and contexts of cols_stop_cases at 3 slots and CAP 10.  A suffix that would not fit the
context behind the prefix is shortened so that P + suffix + CAP - 1 <= the context (tiny-g64 only: ctx 96)."""
import numpy as np

import cols_stop_cases as sc

CKPT_SEED = 97531
SLOTS, CAP = sc.SLOTS, sc.CAP
# shape -> the prefix lengths of the full-prompt equality test
PREFIX_LENS = {"tiny-g64": (1, 7, 33, 40), "small-hd128": (33, 70), "qwen3-4b-dims-l2": (100,)}
# shape -> the prefix length of the sampler / stop / residency tests
PREFIX_ONE = {"tiny-g64": 7, "small-hd128": 33, "qwen3-4b-dims-l2": 100}
PREFIX_MAX = 100


def context(shape, name):
    return sc.SHAPES[name] or shape.max_seq_len


def prefix(vocab_size, P):
    """the first P tokens of one fixed stream: the prefixes of one shape are prefixes of each other"""
    assert P <= PREFIX_MAX
    return [int(t) for t in np.random.default_rng(5200).integers(0, vocab_size, PREFIX_MAX)[:P]]


def suffixes(vocab_size, ctx, P):
    room = ctx - P - (CAP - 1)
    assert room >= 1
    return [s[:room] for s in sc.prompts(vocab_size)]
