"""q3_cols_schedule (include/qwen3_hip.h section 2e): the pass table of q3_generate_many_greedy is a pure function of the request
lengths.  Host only: no GPU."""
import ctypes as C

import pytest

import cols_sim

# (prompt_len, n_new, max_streams)
CASES = [
    ([5], [1], 1),                                          # one request, one pass
    ([1], [7], 1),                                          # prompt of one token
    ([31], [3], 2), ([32], [3], 2), ([33], [3], 2),         # around one pass width
    ([70], [1], 1), ([70], [5], 32),                        # three chunks
    ([1, 3, 33, 40, 7], [4, 1, 20, 9, 33], 1),              # more requests than slots
    ([1, 3, 33, 40, 7], [4, 1, 20, 9, 33], 2),
    ([1, 3, 33, 40, 7], [4, 1, 20, 9, 33], 32),
    ([31, 32, 33, 70, 1, 1, 32], [1, 2, 1, 6, 1, 9, 1], 2),
    ([3] * 40, [4] * 40, 32),                               # 32 prompts of 3 fill a pass: the last slots wait for a column
    ([2] * 33 + [70], [50] * 33 + [2], 32),                 # 32 decoding slots, then a prompt entering beside 31 of them
    ([12, 70, 5], [3, 2, 40], 2),
]


def _ids(c):
    return f"{len(c[0])}req-{c[2]}slots-{max(c[0])}p"


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_schedule_equals_simulation(q3, case):
    plen, nnew, ms = case
    want, wstats = cols_sim.schedule(plen, nnew, ms)
    got, stats = q3.cols_schedule(plen, nnew, ms)
    assert got == want
    assert (stats.passes, stats.live_columns, stats.prompt_columns, stats.decode_columns) == tuple(wstats)
    assert stats.live_columns == len(got) == stats.prompt_columns + stats.decode_columns


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_schedule_properties(q3, case):
    plen, nnew, ms = case
    table, stats = q3.cols_schedule(plen, nnew, ms)
    passes = {}
    for p, slot, pos, req in table:
        passes.setdefault(p, []).append((slot, pos, req))
    assert sorted(passes) == list(range(stats.passes))
    assert [p for p, *_ in table] == sorted(p for p, *_ in table)
    seen = {r: [] for r in range(len(plen))}
    for p in range(stats.passes):
        cols = passes[p]
        assert 1 <= len(cols) <= 32
        runs = []
        for slot, pos, req in cols:
            assert 0 <= slot < ms
            if runs and runs[-1][0] == slot:
                assert pos == runs[-1][2] + 1 and req == runs[-1][1]          # a run: adjacent, consecutive, one request
                runs[-1][2] = pos
            else:
                runs.append([slot, req, pos])
            seen[req].append(pos)
        assert len({r[0] for r in runs}) == len(runs)                         # each slot in at most one run
    for r in range(len(plen)):
        assert seen[r] == list(range(plen[r] + nnew[r] - 1))                  # every prompt and decode position once, in order


def test_schedule_arguments(q3):
    L = q3.load_library()
    sz = C.c_size_t
    one = (sz * 1)(4)
    n = sz(0)
    assert L.q3_cols_schedule(one, one, 1, 1, None, 0, C.byref(n), None) == 0 and n.value == 4 + 4 - 1
    small = (C.c_int32 * 8)()
    assert L.q3_cols_schedule(one, one, 1, 1, small, 2, C.byref(n), None) == -3 and n.value == 7      # table too small
    zero = (sz * 1)(0)
    assert L.q3_cols_schedule(zero, one, 1, 1, None, 0, None, None) == -3                               # empty prompt
    assert L.q3_cols_schedule(one, zero, 1, 1, None, 0, None, None) == -3                               # n_new 0
    assert L.q3_cols_schedule(one, one, 0, 1, None, 0, None, None) == -3
    for ms in (0, 33):
        assert L.q3_cols_schedule(one, one, 1, ms, None, 0, None, None) == -3
    assert L.q3_cols_schedule((sz * 1)(2 ** 31), one, 1, 1, None, 0, None, None) == -3                  # a length past INT32_MAX
    with pytest.raises(q3.Q3Error):
        q3.cols_schedule([3], [0], 2)
