"""Log-probabilities of generated tokens (include/qwen3_hip.h section 2o): a generate result expanded into the q3_score_many /
q3_score_top_many call that must reproduce its records, and the comparisons of the header's standard.  Helper module of
tests/test_genlp_host.py and tests/test_genlp.py (not a conftest).

Request r with prompt p and generated tokens g: the sequence p + g scored from len(p) gives len(g) records, record j the logits
behind the token in front of g[j] with target g[j] -- the row g[j] was taken from.  Behind a resident prefix the prompts are the
suffixes and the call is the one with Q3_SCORE_PREFIX."""
import numpy as np

import score_ref
import score_top_ref as tr
from score_ref import assert_records
from score_top_ref import assert_tops


def score_call(prompts, rows):
    """(sequences, score_from) of the score call that reproduces the records of `rows`, the tokens generated behind `prompts`"""
    seqs = [[int(t) for t in p] + [int(t) for t in g] for p, g in zip(prompts, rows)]
    return seqs, [len(p) for p in prompts]


def expected(t, prompts, rows, k, use_prefix=False):
    """per request (records, tops or None, ranks or None) from the engine's own score calls; k == 0: score_many alone"""
    seqs, sf = score_call(prompts, rows)
    if k == 0:
        recs = t.score_many(seqs, sf, use_prefix=use_prefix)[0]
        return [(r, None, None) for r in recs]
    recs, tops, ranks, _ = t.score_top_many(seqs, k, sf, use_prefix=use_prefix)
    return list(zip(recs, tops, ranks))


def from_logits(logit_rows, tokens, k):
    """(records, tops, ranks) of one request restated on the host: logit_rows[j] is the row tokens[j] was taken from"""
    recs = score_ref.records(logit_rows, tokens)
    tops = np.stack([tr.top(l, k) for l in logit_rows]) if k else np.zeros((len(tokens), 0), dtype=tr.DTYPE)
    ranks = np.array([tr.rank(l, x) for l, x in zip(logit_rows, tokens)], dtype=np.int32)
    return recs, tops, ranks


def assert_same(got, want, rows, k, what):
    """got: Transformer.read_gen_logprobs() cut to the rows; want: expected() or from_logits() per request.  The header's standard:
    target and sum by bits, argmax equal, max by value; tops by bits and index; ranks equal"""
    assert len(got) == len(want) == len(rows), what
    for r, ((recs, tops, ranks), (wrecs, wtops, wranks), row) in enumerate(zip(got, want, rows)):
        w = f"{what}: request {r} of {len(row)} tokens"
        assert recs.shape == (len(row),) and tops.shape == (len(row), k), (w, recs.shape, tops.shape)
        assert_records(recs, wrecs, w)
        if k:
            assert_tops(tops, wtops[:, :k], w)
            assert ranks.dtype == np.int32 and np.array_equal(ranks, wranks), (w, ranks, wranks)
            hit = np.flatnonzero(ranks < k)                 # rank < k exactly when the token is top[rank]
            assert np.array_equal(tops["index"][hit, ranks[hit]], np.asarray(row, dtype=np.int32)[hit]), w
            assert all(int(x) not in tops["index"][i] for i, x in enumerate(row) if ranks[i] >= k), w
        else:
            assert ranks.size == 0, w


def assert_greedy_identities(recs, ranks, row, what):
    """a greedy or temperature-0 request: argmax == token, rank == 0, bits(target) == bits(max)"""
    assert np.array_equal(recs["argmax"], np.asarray(row, dtype=np.int32)), what
    assert np.array_equal(np.ascontiguousarray(recs["target"]).view(np.uint32), np.ascontiguousarray(recs["max"]).view(np.uint32)), what
    if ranks is not None and ranks.size:
        assert not ranks.any(), (what, ranks)


def assert_zero_behind(full, n_out, what):
    """full: read_gen_logprobs(n_new), every request's whole stretch of the buffers: all-zero bytes at and behind n_out[r]"""
    for r, ((recs, tops, ranks), n) in enumerate(zip(full, n_out)):
        for a in (recs[n:], tops[n:], ranks[n:]):
            assert not np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8).any(), f"{what}: request {r}: bytes behind its {n} tokens"
