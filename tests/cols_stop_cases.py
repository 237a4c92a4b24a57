"""The requests of the stop-token tests (include/qwen3_hip.h section 2h) and how their stop sets are chosen.  The synthetic checkpoints
never emit an EOS of their own, so a test first runs the existing loop at the cap and then picks, from the rows it got, a stop set
under which the requests end in every way that matters."""
import itertools

import numpy as np

import cols_sim

STOP_MAX = 8
CKPT_SEED = 2468
# shape -> batch context, as in test_batch_cols.py
SHAPES = {"tiny-g64": 0, "small-hd128": 0, "qwen3-4b-dims-l2": 512}
PROMPT_LEN = (1, 2, 5, 33, 40, 3, 64)
SLOTS, CAP = 3, 10
TEMPERATURE = (0.0, 0.8, 1.0, 0.0, 0.6, 1.0, 0.9)
TOPP = 0.9
SEEDS = tuple(0x9E3779B97F4A7C15 + 1000003 * r for r in range(len(PROMPT_LEN)))


def prompts(vocab_size):
    return [[int(t) for t in np.random.default_rng(4100 + r).integers(0, vocab_size, n)] for r, n in enumerate(PROMPT_LEN)]


def n_emit_of(rows, stop):
    """index of the first stop token of every row plus one, or the row's length"""
    stop = set(stop)
    return [next((i + 1 for i, t in enumerate(r) if t in stop), len(r)) for r in rows]


def kinds(rows, stop):
    """(requests stopped at y_0, stopped inside their row, never stopped)"""
    emit = n_emit_of(rows, stop)
    hit = [r[e - 1] in set(stop) for r, e in zip(rows, emit)]
    at_y0 = sum(h and e == 1 for h, e in zip(hit, emit))
    inside = sum(h and 1 < e < len(r) for h, e, r in zip(hit, emit, rows))
    return at_y0, inside, sum(not h for h in hit)


def passes_saved(rows, stop, prompt_len=PROMPT_LEN, slots=SLOTS):
    """passes of the schedule at the rows' full lengths minus passes when every request ends at its stop token"""
    return (cols_sim.schedule(prompt_len, [len(r) for r in rows], slots)[1].passes
            - cols_sim.schedule(prompt_len, n_emit_of(rows, stop), slots)[1].passes)


def pick_stops(rows, prompt_len=PROMPT_LEN, slots=SLOTS):
    """The first set of at most three tokens of the rows (at most STOP_MAX), in ascending order of size and value, under which at
    least one request stops at y_0, one inside its row, one never, and the schedule gets shorter.  None: there is none."""
    cand = sorted({t for r in rows for t in r})
    for size in (1, 2, 3):
        for stop in itertools.combinations(cand, size):
            if all(v >= 1 for v in kinds(rows, stop)) and passes_saved(rows, stop, prompt_len, slots) >= 1:
                return list(stop)
    return None
