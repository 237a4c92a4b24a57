"""The shared prompt prefix (include/qwen3_hip.h section 2i) as far as it goes without a GPU: the header, the exports, the
Python surface and the front end's argument checks."""
import os
import re

import pytest

from conftest import ROOT

NAMES = ["q3_batch_copy_rows", "q3_batch_prefix_set", "q3_batch_prefix_get", "q3_generate_many_prefix"]


def header():
    with open(os.path.join(ROOT, "include", "qwen3_hip.h")) as fh:
        return fh.read()


def test_names_are_declared_exported_and_listed(q3):
    text = header()
    lib = q3.load_library()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, text, re.M), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in q3.EXPORTED_SYMBOLS
    for method in ("batch_copy_rows", "batch_prefix_set", "batch_prefix_get", "generate_many_prefix"):
        assert callable(getattr(q3.Transformer, method))
    # the section sits behind 2h and says what it leaves out
    assert text.index(" * 2i. ") > text.index(" * 2h. ")
    assert "Dense entry of the suffixes (dense_min) is not offered in this section" in text


def test_abi_version_is_still_1(q3):
    assert re.search(r"^#define Q3_ABI_VERSION 1$", header(), re.M)
    assert q3.load_library().q3_abi_version() == 1


def test_entry_points_reject_a_null_engine(q3):
    import ctypes as C
    lib = q3.load_library()
    n = C.c_size_t(7)
    assert lib.q3_batch_copy_rows(None, 0, (C.c_int32 * 1)(1), 1, 0, 1) == -3
    assert lib.q3_batch_prefix_set(None, (C.c_int32 * 1)(1), 1) == -3
    assert lib.q3_batch_prefix_get(None, C.byref(n), None, 0) == -3
    assert lib.q3_generate_many_prefix(None, None, None, None, 0, None, None, None, None, 0, None, None, None) == -3


@pytest.mark.parametrize("prompts, want", [
    ([[1, 2, 3], [4, 5, 6]], 0),                             # nothing shared
    ([[1, 2, 3], [1, 2, 3]], 2),                             # everything shared: one token is left
    ([[1, 2], [1, 2, 3, 4]], 1),                             # one prompt is a prefix of another
    ([[1, 2, 3, 4]], 3),                                     # a single request
    ([[1, 2, 9, 4], [1, 2, 7, 4], [1, 2, 9, 9]], 2),
    ([[5], [5, 6]], 0),
    ([], 0),
])
def test_common_prefix_len(q3, prompts, want):
    assert q3.common_prefix_len(prompts) == want
    from qwen3_rs_amd.generation import common_prefix_len
    assert common_prefix_len(prompts) == want


class Stub:
    """Records what generate_many calls; no engine behind it."""

    def __init__(self):
        self.calls, self.prefix, self._batch_ctx = [], [], 64

    def get_config(self):
        import types
        return types.SimpleNamespace(seq_len=64)

    def batch_prefix_get(self):
        return list(self.prefix)

    def batch_prefix_set(self, tokens):
        self.calls.append(("set", list(tokens)))
        self.prefix = list(tokens)

    def generate_many_prefix(self, suffixes, n_new, stop_tokens=(), sampler=None):
        self.calls.append(("prefix", [list(s) for s in suffixes], list(n_new), list(stop_tokens), sampler))
        return [[7] * k for k in n_new], "stats"

    def generate_many_greedy(self, prompts, n_new):
        self.calls.append(("greedy", [list(p) for p in prompts], list(n_new)))
        return [[7] * k for k in n_new], "stats"


def test_generate_many_argument_checks(q3):
    t = Stub()
    with pytest.raises(ValueError, match="dense_min"):
        q3.generate_many(t, [[1, 2], [1, 3]], 4, shared_prefix=[9], dense_min=8)
    with pytest.raises(ValueError, match="dense_min"):
        q3.generate_many(t, [[1, 2], [1, 3]], 4, shared_prefix=True, dense_min=8)
    with pytest.raises(ValueError):
        q3.generate_many(t, [[1, 2], []], 4, shared_prefix=[9])
    assert t.calls == []


def test_generate_many_routes_a_shared_prefix(q3):
    t = Stub()
    rows, _ = q3.generate_many(t, [[1, 2, 3], [1, 2, 4, 5]], 4, shared_prefix=True)
    assert t.calls == [("set", [1, 2]), ("prefix", [[3], [4, 5]], [4, 4], [], None)] and rows == [[7] * 4] * 2
    t.calls.clear()
    q3.generate_many(t, [[3], [4, 5]], 4, stop_tokens=[8], shared_prefix=[1, 2], stop_on_device=True)     # resident already: not set again
    assert t.calls == [("prefix", [[3], [4, 5]], [4, 4], [8], None)]
    t.calls.clear()
    q3.generate_many(t, [[3] * 60, [4]], 4, shared_prefix=[1, 2])                   # n_new counts the prefix: 64 - 2 - 60 + 1
    assert t.calls == [("prefix", [[3] * 60, [4]], [3, 4], [], None)]
    t.calls.clear()
    q3.generate_many(t, [[1, 2], [3, 4]], 4, shared_prefix=True)                    # nothing shared: today's path
    q3.generate_many(t, [[1, 2], [3, 4]], 4)
    assert t.calls == [("greedy", [[1, 2], [3, 4]], [4, 4])] * 2
