"""q3_cols_schedule_stop (include/qwen3_hip.h section 2h): the scheduler step of the stop-token loop, run pass by pass on the host.
A request that ends at its first stop token is a request with n_new = n_emit, so the passes must be those of the simulation of
section 2e's five rules for (prompt_len, n_emit), entry for entry.  Host only: no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cols_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"q3_generate_many_stop", "q3_cols_schedule_stop"}
N_RANDOM = 200


def n_emit_of(rows, stop):
    """index of the first stop token of every row plus one, or the row's length"""
    return [next((i + 1 for i, t in enumerate(r) if t in stop), len(r)) for r in rows]


def random_case(seed):
    rng = np.random.default_rng(5000 + seed)
    ms = int(rng.integers(1, 33))
    nr = int(rng.integers(1, 41))
    plen = [int(v) for v in rng.integers(1, 71, nr)]
    nnew = [int(v) for v in rng.integers(1, 13, nr)]
    rows = [[int(t) for t in rng.integers(0, 6, k)] for k in nnew]
    stop = [int(t) for t in rng.choice(6, int(rng.integers(0, 4)), replace=False)]
    return plen, nnew, ms, rows, stop


def check(q3, plen, nnew, ms, rows, stop):
    emit = n_emit_of(rows, set(stop))
    want, wstats = cols_sim.schedule(plen, emit, ms)
    got, n_out, stats = q3.cols_schedule_stop(plen, nnew, ms, rows, stop)
    assert n_out == emit
    assert got == want
    assert (stats.passes, stats.live_columns, stats.prompt_columns, stats.decode_columns) == tuple(wstats)
    return emit


def test_names_declared_listed_exported(q3):
    hdr = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    declared = set(re.findall(r"\b(q3_[a-z0-9_]+)\s*\(", hdr))
    assert NEW <= declared and NEW <= set(q3.EXPORTED_SYMBOLS)
    lib = q3.load_library()
    for s in NEW:
        assert hasattr(lib, s)
    assert "#define Q3_STOP_MAX 8" in hdr and q3.STOP_MAX == 8
    assert "#define Q3_ABI_VERSION 1" in hdr


@pytest.mark.parametrize("block", range(8))
def test_random_cases_equal_simulation(q3, block):
    for seed in range(block * 25, block * 25 + 25):
        check(q3, *random_case(seed))


def test_random_cases_cover_every_kind():
    """the random cases hold requests stopped early, stopped at y_0 and never stopped -- and each of those next to a freed slot's
    next occupant -- so the comparison above cannot pass without a stop ever mattering"""
    early = first = never = last = queued = 0
    for seed in range(N_RANDOM):
        plen, nnew, ms, rows, stop = random_case(seed)
        emit = n_emit_of(rows, set(stop))
        for r, (e, k) in enumerate(zip(emit, nnew)):
            hit = rows[r][e - 1] in stop
            first += hit and e == 1 and k > 1
            early += hit and 1 < e < k
            last += hit and e == k and k > 1
            never += not hit
        queued += len(plen) > ms and emit != nnew
    assert min(early, first, never, last) >= 50, (early, first, never, last)
    assert queued >= 20, queued


PLEN, NNEW = [1, 3, 33, 40, 7, 70, 2], [4, 1, 12, 9, 6, 5, 8]


def rows_of(fill, nnew=NNEW):
    return [[fill] * k for k in nnew]


@pytest.mark.parametrize("ms", [1, 2, 3, 32])
def test_every_request_stops_at_y0(q3, ms):
    emit = check(q3, PLEN, NNEW, ms, rows_of(5), [5])
    assert emit == [1] * len(PLEN)


@pytest.mark.parametrize("ms", [1, 3, 32])
def test_no_stop_token_occurs(q3, ms):
    emit = check(q3, PLEN, NNEW, ms, rows_of(2), [5, 4, 0])
    assert emit == NNEW
    table, _, stats = q3.cols_schedule_stop(PLEN, NNEW, ms, rows_of(2), [5, 4, 0])
    assert (table, stats) == q3.cols_schedule(PLEN, NNEW, ms)


@pytest.mark.parametrize("ms", [1, 3, 32])
def test_stop_token_at_the_last_index(q3, ms):
    rows = [[2] * (k - 1) + [5] for k in NNEW]
    emit = check(q3, PLEN, NNEW, ms, rows, [5])
    assert emit == NNEW


def test_one_slot_many_requests(q3):
    plen, nnew = [3, 1, 40, 2] * 10, [5, 7, 2, 12] * 10
    rng = np.random.default_rng(77)
    rows = [[int(t) for t in rng.integers(0, 4, k)] for k in nnew]
    emit = check(q3, plen, nnew, 1, rows, [0])
    assert any(e < k for e, k in zip(emit, nnew)) and any(e == 1 for e in emit)


@pytest.mark.parametrize("ms", [1, 2, 32])
def test_no_stop_list_equals_cols_schedule(q3, ms):
    rng = np.random.default_rng(78)
    rows = [[int(t) for t in rng.integers(0, 6, k)] for k in NNEW]
    table, n_out, stats = q3.cols_schedule_stop(PLEN, NNEW, ms, rows, [])
    assert (table, stats) == q3.cols_schedule(PLEN, NNEW, ms)
    assert n_out == NNEW


def test_stop_list_of_eight(q3):
    rows = [[int(t) for t in np.random.default_rng(79 + r).integers(0, 20, k)] for r, k in enumerate(NNEW)]
    check(q3, PLEN, NNEW, 3, rows, [19, 3, 5, 7, 11, 13, 17, 2])


def test_arguments(q3):
    L = q3.load_library()
    sz, i32 = C.c_size_t, C.c_int32
    plen, nnew, rows, stop = (sz * 1)(4), (sz * 1)(3), (i32 * 3)(1, 2, 3), (i32 * 9)(*range(10, 19))
    n, n_out = sz(0), (sz * 1)(0)

    def call(pl=plen, nn=nnew, nr=1, ms=1, rw=rows, stp=stop, ns=1, table=None, cap=0):
        return L.q3_cols_schedule_stop(pl, nn, nr, ms, rw, stp, ns, table, cap, C.byref(n), n_out, None)

    assert call() == 0 and n.value == 4 + 3 - 1 and n_out[0] == 3
    assert call(stp=(i32 * 1)(2)) == 0 and n.value == 4 + 2 - 1 and n_out[0] == 2
    assert call(stp=None, ns=0) == 0 and n.value == 6                       # no stop list at all
    assert call(ns=8) == 0
    assert call(ns=9) == -3 and "stop tokens" in L.q3_last_error().decode()
    assert call(stp=None, ns=1) == -3
    assert call(rw=None) == -3
    small = (i32 * 8)()
    assert call(table=small, cap=2) == -3 and n.value == 6                  # table too small
    zero = (sz * 1)(0)
    assert call(pl=zero) == -3 and call(nn=zero) == -3 and call(nr=0) == -3
    for ms in (0, 33):
        assert call(ms=ms) == -3
    assert L.q3_cols_schedule_stop(plen, nnew, 1, 1, rows, stop, 1, None, 0, None, None, None) == 0      # every output optional
    with pytest.raises(ValueError):
        q3.cols_schedule_stop([4], [3], 1, [[1, 2]], [1])                   # a row shorter than n_new
    with pytest.raises(q3.Q3Error):
        q3.cols_schedule_stop([4], [3], 1, [[1, 2, 3]], list(range(9)))
