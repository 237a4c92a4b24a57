"""CPU tests of the prompt-lookup drafter (include/qwen3_hip.h section 2c): q3_lookup_draft is the definition, q3_lookup_trace
the incremental hashed form the speculative loop runs; both against the Python restatement in spec_sim.py."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from spec_sim import draft_ref, simulate


CRAFTED = [
    # (sequence, ngram, draft_len, expected draft)
    ([1, 2, 3, 4, 5], 2, 4, []),                                  # no earlier occurrence of (4, 5)
    ([7, 8, 1, 7, 8, 2, 7, 8, 3, 7, 8], 2, 1, [3]),               # several matches: the latest one
    ([7, 8, 1, 7, 8, 2, 7, 8, 3, 7, 8], 2, 4, [3, 7, 8]),         # ... whose continuation runs into the end of the sequence
    ([5, 5, 5, 5], 2, 3, [5]),                                    # the match overlaps the suffix: i = 1, continuation S[3:]
    ([5, 5, 5, 5], 1, 3, [5]),                                    # i = 2
    ([1, 2, 3, 1, 2, 3, 1, 2], 2, 8, [3, 1, 2]),                  # i = 3
    ([1, 2, 3, 1, 2, 3, 1, 2], 3, 2, [3, 1]),                     # suffix (3, 1, 2) at i = 2
    ([4, 9], 2, 4, []),                                           # n == ngram
    ([4], 2, 4, []),                                              # n < ngram
    ([], 1, 4, []),
    ([1, 2, 1, 2], 2, 0, []),                                     # draft_len 0
    ([1, 2, 1, 2], 2, 5, [1, 2]),
    ([3, 1, 2, 9, 1, 2], 2, 1, [9]),
]


@pytest.mark.parametrize("seq,ngram,draft_len,want", CRAFTED)
def test_lookup_draft_crafted(q3, seq, ngram, draft_len, want):
    assert draft_ref(seq, ngram, draft_len) == want               # the restatement says what the table says
    assert q3.lookup_draft(seq, ngram, draft_len) == want
    # the incremental drafter, grown from every split point
    for n_corpus in range(len(seq) + 1):
        rows = q3.lookup_trace(seq, n_corpus, ngram, max(draft_len, 1))
        assert rows[-1] == draft_ref(seq, ngram, max(draft_len, 1)), n_corpus


def test_lookup_draft_random_small_alphabet(q3):
    """1,000 random sequences over alphabets of 2..6 symbols (repeats everywhere): the definition in C, and the hashed incremental
    drafter at EVERY prefix, equal the rescanning Python definition."""
    rng = np.random.default_rng(20)
    for case in range(1000):
        n = int(rng.integers(0, 60))
        alpha = int(rng.integers(2, 7))
        seq = [int(v) for v in rng.integers(0, alpha, n)]
        ngram = int(rng.integers(1, 5))
        draft_len = int(rng.integers(1, 9))
        assert q3.lookup_draft(seq, ngram, draft_len) == draft_ref(seq, ngram, draft_len), (case, seq, ngram, draft_len)
        n_corpus = int(rng.integers(0, n + 1))
        rows = q3.lookup_trace(seq, n_corpus, ngram, draft_len)
        assert len(rows) == n - n_corpus + 1
        for r, m in enumerate(range(n_corpus, n + 1)):
            assert rows[r] == draft_ref(seq[:m], ngram, draft_len), (case, m, seq, ngram, draft_len)


def test_lookup_draft_large_token_ids_and_long_ngram(q3):
    """token ids up to 2^31 - 1 and windows longer than the sequence's period: the hash is only a filter, tokens are compared"""
    rng = np.random.default_rng(3)
    base = [int(v) for v in rng.integers(0, 2 ** 31 - 1, 70)]
    seq = base + base[:68]
    assert q3.lookup_draft(seq, 64, 5) == draft_ref(seq, 64, 5) == base[68:70] + base[:3]
    rows = q3.lookup_trace(seq, 70, 64, 5)
    for r, m in enumerate(range(70, len(seq) + 1)):
        assert rows[r] == draft_ref(seq[:m], 64, 5), m


def test_lookup_trace_rejects_bad_arguments(q3):
    with pytest.raises(q3.Q3Error) as e:
        q3.lookup_trace([1, 2, 3], 1, 0, 4)
    assert e.value.code == -3
    with pytest.raises(q3.Q3Error):
        q3.lookup_trace([1, 2, 3], 5, 2, 4)


def test_simulation_accounts_for_every_token():
    """the loop restatement the GPU tests take their expected statistics from: every reference token is produced exactly once"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        G = [int(v) for v in rng.integers(0, 4, int(rng.integers(1, 80)))]
        corpus = [int(v) for v in rng.integers(0, 4, int(rng.integers(0, 30)))]
        sim = simulate(G, corpus, 1, int(rng.integers(1, 4)), int(rng.integers(1, 32)))
        assert sim["single_steps"] + sum(a + 1 for _, a in sim["passes"]) == len(G)
        assert all(1 <= d <= 31 and 0 <= a <= d for d, a in sim["passes"])
    assert simulate([5, 6, 7, 8], [1, 5, 6, 7, 8], 1, 1, 8) == {"verify_passes": 1, "single_steps": 0, "drafted": 3, "accepted": 3, "passes": [(3, 3)]}
    assert simulate([5, 6], [], 1, 64, 8)["verify_passes"] == 0


def test_header_section_2c_symbols_are_bound_and_exported(q3):
    hdr = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    sec = hdr[hdr.index(" * 2c. "):hdr.index(" * 3. Operator-level")]
    declared = set(re.findall(r"\b(q3_[a-z0-9_]+)\s*\(", sec))
    assert declared == {"q3_verify", "q3_lookup_draft", "q3_lookup_trace", "q3_generate_lookup"}
    assert declared <= set(q3.EXPORTED_SYMBOLS)
    lib = q3.load_library()
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert "#define Q3_VERIFY_MAX 32" in hdr and q3.VERIFY_MAX == 32
    assert lib.q3_abi_version() == 1


class _GreedyFake:
    """forward() of a scripted model, and generate_lookup() as the plain greedy loop over it (what the engine guarantees)"""

    def __init__(self, vocab=7, seq_len=40):
        self.vocab, self.seq_len = vocab, seq_len

    def get_config(self):
        class C:
            seq_len = self.seq_len
        return C

    def forward(self, token, pos):
        lg = np.zeros(self.vocab, dtype=np.float32)
        lg[(token * 3 + pos // 5) % self.vocab] = 1.0
        return lg

    def generate_lookup(self, corpus, token, pos, n, ngram=2, draft_len=8):
        assert 0 < n <= draft_len + 1 and pos + n <= self.seq_len
        out = []
        for k in range(n):
            token = int(np.argmax(self.forward(token, pos + k)))
            out.append(token)
        return out, None


def test_generate_and_chat_turn_lookup_option_call_pattern(q3):
    """lookup=(ngram, draft_len) routes the greedy decode through generate_lookup in rounds of draft_len + 1 tokens: same tokens, same
    stop handling (generate outputs the stop token, chat ends the turn in front of it), same final position."""
    t = _GreedyFake()
    for stop in ((), (2,), (5,), (0,)):
        for mx in (None, 7, 30):
            assert q3.generate(t, [1, 2, 3], max_new_tokens=mx, stop_tokens=stop, lookup=(2, 4))[0] == \
                   q3.generate(t, [1, 2, 3], max_new_tokens=mx, stop_tokens=stop)[0], (stop, mx)
        for mx in (5, 100):
            assert q3.chat_turn(t, [1, 2, 3], 4, mx, stop_tokens=stop, lookup=(2, 4))[:2] == \
                   q3.chat_turn(t, [1, 2, 3], 4, mx, stop_tokens=stop)[:2], (stop, mx)
    with pytest.raises(ValueError):
        q3.generate(t, [1, 2, 3], lookup=(2, 8), on_logits=lambda *a: None)
    with pytest.raises(ValueError):
        q3.generate(t, [1, 2, 3], lookup=(2, 32))
