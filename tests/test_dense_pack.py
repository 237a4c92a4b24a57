"""CPU tests of section 2g of include/qwen3_hip.h: the three names are declared, listed and exported, and q3_dense_pack equals the
restatement of its rule in tests/dense_sim.py, entry for entry, with the invariants the dense kernels rely on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_sim
from conftest import ROOT

NEW = {"q3_dense_pack", "q3_batch_prefill_slots", "q3_generate_many_dense"}
CAPS = (16, 128, 2048)
FIXED = [[1], [7], [8], [9], [1, 7, 8, 9], [9, 8, 7, 1], [128], [128, 1], [120, 8, 1], [300], [5, 4200, 3], [16] * 9, [2048, 2048], [41, 97, 8]]


def test_header_symbol_list_and_binary_agree_on_the_new_names(q3):
    hdr = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    declared = set(re.findall(r"\b(q3_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(q3.EXPORTED_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", q3.lib_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert NEW <= exported
    lib = q3.load_library()
    assert len(lib.q3_generate_many_dense.argtypes) == len(lib.q3_generate_many_sampled.argtypes) + 2      # dense_min, dstats


def cases():
    rng = np.random.default_rng(20260)
    out = [(lens, cap) for lens in FIXED for cap in CAPS]
    for _ in range(300):
        cap = int(rng.choice(CAPS))
        n = int(rng.integers(1, 12))
        hi = int(rng.choice([10, cap, 3 * cap]))
        out.append(([int(v) for v in rng.integers(1, hi + 1, n)], cap))
    return out


def test_pack_equals_the_restated_rule(q3):
    n_long = n_exact = 0
    for lens, cap in cases():
        got, st = q3.dense_pack(lens, cap)
        want, wst, plen = dense_sim.pack(lens, cap)
        assert got == want, (lens, cap)
        assert (st.blocks, st.live_columns, st.pad_columns) == tuple(wst), (lens, cap)
        # the invariants: aligned starts, one piece of a run per block, consecutive pieces, every column counted
        assert all(c % 8 == 0 and 0 <= c < cap for _, c, _, _ in got)
        assert len({(b, r) for b, _, r, _ in got}) == len(got)
        assert [r for _, _, r, _ in got] == sorted(r for _, _, r, _ in got)
        assert [b for b, _, _, _ in got] == sorted(b for b, _, _, _ in got)
        for r, n in enumerate(lens):
            mine = [(i, e) for i, e in enumerate(got) if e[2] == r]
            assert [i for i, _ in mine] == list(range(mine[0][0], mine[0][0] + len(mine)))
            assert [e[3] for _, e in mine] == [sum(plen[i] for i, _ in mine[:k]) for k in range(len(mine))]
            assert sum(plen[i] for i, _ in mine) == n
            assert [e[0] for _, e in mine] == list(range(mine[0][1][0], mine[0][1][0] + len(mine)))
            n_long += len(mine) > 2
        for i, (b, c, _, _) in enumerate(got):
            assert c + plen[i] <= cap
            n_exact += c + plen[i] == cap
            if i and got[i - 1][0] == b:
                assert c == -(-(got[i - 1][1] + plen[i - 1]) // 8) * 8
        assert st.live_columns == sum(lens)
        assert st.blocks == got[-1][0] + 1
    assert n_long > 10 and n_exact > 10          # runs over more than two blocks, pieces that end a block exactly


def test_pack_arguments(q3):
    lib = q3.load_library()
    sz = C.c_size_t
    one = (sz * 1)(5)
    n = sz(0)
    assert lib.q3_dense_pack(one, 1, 16, None, 0, C.byref(n), None) == 0 and n.value == 1       # count only
    three = (sz * 3)(20, 20, 20)
    assert lib.q3_dense_pack(three, 3, 16, None, 0, C.byref(n), None) == 0 and n.value == 6
    small = (C.c_int32 * 8)()
    assert lib.q3_dense_pack(three, 3, 16, small, 2, C.byref(n), None) == -3 and n.value == 6
    assert [int(v) for v in small] == [0, 0, 0, 0, 1, 0, 0, 16]
    assert lib.q3_dense_pack(three, 0, 16, None, 0, None, None) == -3
    assert lib.q3_dense_pack(None, 3, 16, None, 0, None, None) == -3
    assert lib.q3_dense_pack((sz * 2)(4, 0), 2, 16, None, 0, None, None) == -3
    for cap in (0, 8, 24, -16):
        assert lib.q3_dense_pack(three, 3, cap, None, 0, None, None) == -3
    with pytest.raises(q3.Q3Error):
        q3.dense_pack([3, 0], 16)
