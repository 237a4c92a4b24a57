"""Reference code of the stop-sequence tests (include/qwen3_hip.h section 2t): brute force with no automaton in it, the designed
vocabulary of the compiler tests, and the picker of the GPU tests."""
import itertools

import numpy as np

import cols_sim
from cols_stop_cases import PROMPT_LEN, SLOTS

ALPHABET = (b"a", b"b", b"\n")
# every string of 1 to 3 bytes over the alphabet, then two tokens of no bytes: 3 + 9 + 27 + 2 = 41 tokens
VOCAB = [b"".join(p) for n in (1, 2, 3) for p in itertools.product(ALPHABET, repeat=n)] + [b"", b""]
EMPTY = (len(VOCAB) - 2, len(VOCAB) - 1)


def tok(b: bytes) -> int:
    return VOCAB.index(b)


def n_emit_strings(tokens, vocab, strings):
    """the smallest i such that the bytes of tokens[:i] contain a stop string, or len(tokens)"""
    pats = [s if isinstance(s, bytes) else s.encode("utf-8") for s in strings]
    text = b""
    for i, t in enumerate(tokens):
        text += vocab[t]
        if any(p in text for p in pats):
            return i + 1
    return len(tokens)


def n_emit_seqs(tokens, seqs):
    """the smallest i such that tokens[:i] ends with one of seqs (plain sub-list search), or len(tokens)"""
    tokens = list(tokens)
    for i in range(1, len(tokens) + 1):
        if any(len(q) <= i and tokens[i - len(q):i] == list(q) for q in seqs):
            return i
    return len(tokens)


def n_emit_rows(rows, seqs, stop_tokens=(), starts=None):
    """per row the smaller of the first stop token's and the first completed sequence's index + 1, or the row's length;
    starts[r] == -1: request r has no stop sequences"""
    stop = set(stop_tokens)
    out = []
    for r, row in enumerate(rows):
        a = next((i + 1 for i, t in enumerate(row) if t in stop), len(row))
        b = len(row) if starts is not None and starts[r] < 0 else n_emit_seqs(row, seqs)
        out.append(min(a, b))
    return out


def slot_successions(prompt_len, n_emit, slots):
    """[(slot, request, the request that takes the slot next)] of the schedule cols_sim lays out"""
    table, _ = cols_sim.schedule(prompt_len, n_emit, slots)
    order = {}
    for _, slot, _, req in table:
        if not order.setdefault(slot, []) or order[slot][-1] != req:
            order[slot].append(req)
    return [(slot, a, b) for slot, reqs in order.items() for a, b in zip(reqs, reqs[1:])]


def occurs(rows, seq):
    seq = list(seq)
    return any(r[i:i + len(seq)] == seq for r in rows for i in range(len(r) - len(seq) + 1))


def pick_stop_seqs(rows, prompt_len=PROMPT_LEN, slots=SLOTS):
    """A stop list for the rows of the existing loop at the cap, as (seqs, n_emit, what): a one-token sequence that ends a request
    at y_0, a sequence of two or more tokens that ends a request inside its row (so that state is carried across passes), and a
    RESET sequence: the last token at the cap of a request that never ends followed by y_0 of the request that takes its slot
    next -- widened by the token in front where two tokens do not do -- which occurs nowhere contiguously in any row, so the next
    occupant must not end at y_0.  At least one request never ends and at least one pass is saved.  None: there is no such list."""
    cap_passes = cols_sim.schedule(prompt_len, [len(r) for r in rows], slots)[1].passes
    firsts = sorted({r[0] for r in rows})
    for y0 in firsts:
        for r2, row in enumerate(rows):
            for n, i in itertools.product((2, 3), range(1, len(row) - 1)):
                if i + 1 < n:
                    continue
                inner = row[i + 1 - n:i + 1]               # ends at index i: inside the row, not at y_0, not at the cap
                base = [[y0], inner]
                emit = n_emit_rows(rows, base)
                if emit[r2] != i + 1 or inner == [y0] * n:
                    continue
                for width in (2, 3):
                    for slot, a, b in slot_successions(prompt_len, emit, slots):
                        if emit[a] != len(rows[a]) or len(rows[a]) < width - 1:
                            continue
                        reset = rows[a][len(rows[a]) - (width - 1):] + [rows[b][0]]
                        if occurs(rows, reset) or reset in base:
                            continue
                        seqs = base + [reset]
                        got = n_emit_rows(rows, seqs)
                        if got != emit:
                            continue
                        at_y0 = sum(e == 1 and row_[0] == y0 for e, row_ in zip(got, rows))
                        never = sum(e == len(row_) and not any(row_[max(0, len(row_) - len(q)):] == q for q in seqs) for e, row_ in zip(got, rows))
                        saved = cap_passes - cols_sim.schedule(prompt_len, got, slots)[1].passes
                        if at_y0 >= 1 and never >= 1 and saved >= 1 and got[b] > 1:
                            return seqs, got, {"y0": y0, "inner": (r2, inner), "reset": (slot, a, b, reset), "saved": saved}
    return None


def check_pick(rows, seqs, emit, what, prompt_len=PROMPT_LEN, slots=SLOTS):
    """the conditions of the picker, asserted"""
    assert emit == n_emit_rows(rows, seqs)
    assert any(e == 1 and r[0] == what["y0"] for e, r in zip(emit, rows)), "no request ends at y_0 through a one-token sequence"
    r2, inner = what["inner"]
    assert len(inner) >= 2 and 1 < emit[r2] < len(rows[r2]) and rows[r2][emit[r2] - len(inner):emit[r2]] == inner, "no sequence of two tokens ends a request inside its row"
    assert any(e == len(r) and not any(r[max(0, len(r) - len(q)):] == q for q in seqs) for e, r in zip(emit, rows)), "every request ends"
    assert what["saved"] >= 1 and cols_sim.schedule(prompt_len, [len(r) for r in rows], slots)[1].passes - cols_sim.schedule(prompt_len, emit, slots)[1].passes == what["saved"]
    slot, a, b, reset = what["reset"]
    assert (slot, a, b) in slot_successions(prompt_len, emit, slots)
    assert emit[a] == len(rows[a]) and reset == rows[a][len(rows[a]) - (len(reset) - 1):] + [rows[b][0]] and not occurs(rows, reset)
    assert emit[b] > 1, "the next occupant ends at y_0"
