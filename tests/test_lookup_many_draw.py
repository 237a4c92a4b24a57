"""Prompt-lookup drafts under the sampler (include/qwen3_hip.h section 2w).  No tolerance: q3_generate_many_lookup_draw equals the sampled
q3_generate_many_stop in rows, n_out, slot rng states and cache rows.  Synthetic logits are near flat and a sampled draft almost never
stands there, so the main cases run on a designed-logits checkpoint (logit_ckpt's construction): token t draws (t + 1) % 4 with p = 0.78
and ALT[t % 4] with p = 0.22 at temperature 1, everything else 30 below -- output that walks the cycle 0 1 2 3 with skips.  7 is drawn
only behind a 1 and lies in the prompts behind a 1: STOP ends requests on a token an ngram-1 draft proposed.  The synthetic shapes of
cols_draw_cases (head_dim 64 and 128) check the identity alone."""
import ctypes as C
import os
from unittest import mock

import numpy as np
import pytest

import cols_draw_cases as cdc
import logit_ckpt as lc
from conftest import ROOT, assert_biteq

V, ALT, SLOTS, STOP, NGRAM = lc.V_SMALL, [2, 7, 0, 1], 3, [7], 1
CYCLE = [0, 1, 2, 3, 0, 1, 7, 0, 1, 2]
PROMPTS = [CYCLE[:8], CYCLE[1:2], CYCLE[:9], CYCLE[3:8], CYCLE[4:8]]
N_NEW = [40, 30, 24, 12, 25]
SAMPLER = ([1.0, 0.0, 0.7, 1.0, 0.7], [1.0, 0.9, 0.9, 0.95, 1.0], [42, 7, 0x9E3779B97F4A7C15, 11, 5])


def _design(c, n):
    d = np.full(n, lc.PEAK - 30.0)
    d[(c + 1) % 4], d[ALT[c]] = lc.PEAK, lc.PEAK - 1.25
    return d


@pytest.fixture(scope="session")
def cycle_ckpt(tmp_ckpt_dir):
    """logit_ckpt.write over four designs of this file, which its tables hold for the length of that one call"""
    designs = {f"cycle_{c}": (lambda k, c=c: _design(c, k), 1.0, []) for c in range(4)}
    with mock.patch.dict(lc.DESIGNS, designs), mock.patch.dict(lc.FILES, {"cycle": (V, list(designs))}):
        return lc.write(os.path.join(tmp_ckpt_dir, "cycle.bin"), "cycle")


@pytest.fixture(scope="session")
def oracle_rows(oracle, cycle_ckpt):
    """the designed requests without a stop list on the C oracle: Sampler + forward, the chat rule of section 2f"""
    m, rows = oracle.OracleModel(cycle_ckpt, 0), []
    for P, n, T, p, seed in zip(PROMPTS, N_NEW, *SAMPLER):
        s = oracle.Sampler(V, T, p, seed)
        pick = s.sample if T > 0 else oracle.sample_argmax
        for pos, tok in enumerate(P):
            y = pick(m.forward(tok, pos))
        row = [y]
        while len(row) < n:
            row.append(pick(m.forward(row[-1], len(P) + len(row) - 1)))
        rows.append(row)
    m.close()
    return rows


def test_symbols_and_refusals_without_a_gpu(q3):
    hdr = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    L = q3.load_library()
    for name in ("q3_generate_many_lookup_draw", "q3_batch_slot_rng"):
        assert name + "(" in hdr and name in q3.EXPORTED_SYMBOLS and hasattr(L, name)
    one = lambda t, v: (t * 1)(v)
    for ngram, dl, fw, word in [(3, 8, 0, "null engine"), (0, 8, 0, "ngram"), (3, 0, 0, "draft_len"), (3, 32, 0, "draft_len"), (3, 8, 3, "fill_width"),
                                (3, 8, 64, "fill_width")]:
        rc = L.q3_generate_many_lookup_draw(None, one(C.c_int32, 1), one(C.c_size_t, 1), one(C.c_size_t, 1), 1, one(C.c_float, 1.0), one(C.c_float, 0.9),
                                            one(C.c_uint64, 1), None, 0, ngram, dl, fw, one(C.c_int32, 0), one(C.c_size_t, 0), None, None)
        assert rc == -3 and word in L.q3_last_error().decode()
    assert L.q3_batch_slot_rng(None, 0, C.byref(C.c_uint64(0))) == -3


def test_reference_rows_hold_standing_and_falling_drafts(q3, oracle_rows):
    """q3.lookup_draft over prompt + row so far, held against the oracle's row: drafts stand and fall in every sampled request, and a
    request cut at STOP ends on a standing draft"""
    def walk(P, row, n):
        stood = fell = k = 0
        g = 1
        while g < len(row):
            d = q3.lookup_draft(P + row[:g], NGRAM, min(8, n - g - 1)) if n - g - 1 > 0 else []
            k = 0
            while k < len(d) and g + k < len(row) and d[k] == row[g + k]:
                k += 1
            stood, fell = stood + k, fell + (1 if k < len(d) and g + k < len(row) else 0)
            g += k + 1
        return stood, fell, k > 0 and g == len(row) + 1       # ... the last walk's last standing draft is the row's last token
    ends_on_draft = False
    for P, n, T, row in zip(PROMPTS, N_NEW, SAMPLER[0], oracle_rows):
        stood, fell, _ = walk(P, row, n)
        assert stood > 0 and (fell > 0 or T == 0.0), (row, stood, fell)
        ends_on_draft |= STOP[0] in row and walk(P, row[:row.index(STOP[0]) + 1], n)[2]
    assert ends_on_draft


_PLAIN = {}


def _engine_run(q3, path, top_k, prompts, n_new, sampler, stop, lookup):
    """on a fresh engine: the requests; then the first SLOTS of them alone, a slot each, and the rng and the readable cache rows they leave"""
    def run(t, k):
        args = prompts[:k], n_new[:k]
        if lookup is None:
            return t.generate_many_stop(*args, stop, tuple(v[:k] for v in sampler), raw=True)[:2] + (None,)
        r = t.generate_many_lookup_draw(*args, tuple(v[:k] for v in sampler), stop, ngram=NGRAM, draft_len=lookup[0], fill_width=lookup[1], raw=True)
        return r[:2] + (r[3],)
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(SLOTS)
        t.set_top_k(top_k)
        many, few, c = run(t, len(prompts)), run(t, SLOTS), t.get_config()
        kv = [t.batch_read_state(i, kind).reshape(c.n_layers, t._batch_ctx, -1)[:, :len(prompts[i]) + few[1][i] - 1]
              for i in range(SLOTS) for kind in ("key", "value")]
        return many[:2], few[:2], [t.batch_slot_rng(i) for i in range(SLOTS)], kv, many[2]


def _check(q3, path, top_k, prompts, n_new, sampler, stop, lookup):
    """the lookup loop against the plain sampled loop (run once per checkpoint, top-k and stop list); returns the LookupStats"""
    key = (path, top_k, tuple(stop))
    if key not in _PLAIN:
        _PLAIN[key] = _engine_run(q3, path, top_k, prompts, n_new, sampler, stop, None)
    plain, got = _PLAIN[key], _engine_run(q3, path, top_k, prompts, n_new, sampler, stop, lookup)
    assert got[:3] == plain[:3]                               # rows with the -1 behind them and n_out of both calls, slot rng states
    for a, b in zip(got[3], plain[3]):
        assert_biteq(a, b, "cache rows")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("top_k", [0, 20])
@pytest.mark.parametrize("fill_width", [0, 32])
@pytest.mark.parametrize("draft_len", [1, 8, 31])
def test_designed_rows_equal_the_plain_sampled_loop(q3, cycle_ckpt, oracle_rows, draft_len, fill_width, top_k):
    got = _check(q3, cycle_ckpt, top_k, PROMPTS, N_NEW, SAMPLER, [], (draft_len, fill_width))
    assert got[4].accepted > 0 and got[4].drafted > got[4].accepted
    if top_k == 0:                                            # the oracle's Sampler knows no top-k
        assert got[0][0] == [tok for row in oracle_rows for tok in row]


@pytest.mark.gpu
def test_stop_list_equals_the_plain_sampled_loop(q3, cycle_ckpt):
    """Requests end at STOP as in the plain loop.  That one of them ends on a standing draft is what the CPU test shows of these rows
    (at fill_width 32 every draft has a column); here only the identity and an early end are asserted."""
    got = _check(q3, cycle_ckpt, 0, PROMPTS, N_NEW, SAMPLER, STOP, (8, 32))
    assert any(k < n for k, n in zip(got[0][1], N_NEW)) and got[4].accepted > 0


@pytest.mark.gpu
def test_generate_many_routes_lookup_with_a_sampler(q3, cycle_ckpt, oracle_rows):
    with q3.TransformerBuilder(cycle_ckpt).build() as t:
        t.batch_init(SLOTS)
        rows, _ = q3.generate_many(t, PROMPTS, max(N_NEW), sampler=SAMPLER, stop_on_device=True, lookup=8, lookup_ngram=NGRAM, lookup_fill=32)
        assert t.last_lookup_stats.accepted > 0
        with pytest.raises(ValueError, match="plain loops only"):
            q3.generate_many(t, PROMPTS, 4, sampler=SAMPLER, stop_on_device=True, lookup=8, logprobs=0)
    assert [r[:n] for r, n in zip(rows, N_NEW)] == oracle_rows


@pytest.mark.gpu
@pytest.mark.parametrize("top_k", [0, 20])
@pytest.mark.parametrize("fill_width", [0, 32])
@pytest.mark.parametrize("draft_len", [1, 8, 31])
@pytest.mark.parametrize("name", ["tiny-g64", "small-hd128"])
def test_synthetic_shapes_equal_the_plain_sampled_loop(q3, tmp_ckpt_dir, name, draft_len, fill_width, top_k):
    shape = q3.checkpoint.SHAPES[name]
    path = os.path.join(tmp_ckpt_dir, f"lookupdraw-{name}.bin")
    q3.checkpoint.ensure_synthetic_checkpoint(path, shape, seed=cdc.CKPT_SEED)
    temps, topps = zip(cdc.GREEDY, *cdc.SAMPLERS, cdc.SAMPLERS[0])      # request 0 greedy, request 1 at temperature 1
    _check(q3, path, top_k, cdc.prompts(shape.vocab_size), list(cdc.N_NEW), (list(temps), list(topps), cdc.request_seeds(0)), [],
           (draft_len, fill_width))


@pytest.mark.gpu
def test_fast_engine_and_slot_rng_arguments(q3, cycle_ckpt):
    with q3.TransformerBuilder(cycle_ckpt).with_strict(False).build() as t:
        t.batch_init(SLOTS)
        with pytest.raises(q3.Q3Error, match="Q3_FLAG_FAST"):
            t.generate_many_lookup_draw(PROMPTS, N_NEW, SAMPLER)
    with q3.TransformerBuilder(cycle_ckpt).build() as t:
        t.batch_init(SLOTS)
        with pytest.raises(q3.Q3Error, match="no sampled"):
            t.batch_slot_rng(0)
        t.generate_many_lookup_draw(PROMPTS[:1], [2], (1.0, 1.0, 3))
        with pytest.raises(q3.Q3Error, match="out of range"):
            t.batch_slot_rng(SLOTS)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["penalties", "logit_bias", "guide", "guide_sparse", "logprobs", "stop_seq", "prefix"])
def test_refusals_leave_the_engine_usable(q3, cycle_ckpt, setting):
    on, off, word = {"penalties": (lambda t: t.set_penalties(0.5, 0.0), lambda t: t.set_penalties(0.0, 0.0), "q3_sampler_penalties"),
                     "logit_bias": (lambda t: t.set_logit_bias([{5: 1.0}]), lambda t: t.set_logit_bias([]), "q3_logit_bias_set"),
                     "guide": (lambda t: t.set_guide(np.zeros((1, V), dtype=np.int32), 0), lambda t: t.set_guide(None, 0), "q3_guide_set"),
                     "guide_sparse": (lambda t: t.set_guide_sparse([0], [0, 0], [], [], 0), lambda t: t.set_guide_sparse(None, None, None, None, 0),
                                      "q3_guide_set_sparse"),
                     "logprobs": (lambda t: t.set_gen_logprobs(0), lambda t: t.set_gen_logprobs(-1), "q3_gen_logprobs"),
                     "stop_seq": (lambda t: t.set_stop_sequences(q3.stops.stop_automaton([[5, 5, 5]], V)), lambda t: t.set_stop_sequences(None),
                                  "q3_stop_seq_set"),
                     "prefix": (lambda t: t.batch_prefix_set([1, 2]), lambda t: t.batch_prefix_set([]), "q3_batch_prefix_set")}[setting]
    with q3.TransformerBuilder(cycle_ckpt).build() as t:
        t.batch_init(SLOTS)
        want = t.generate_many_stop(PROMPTS, N_NEW, STOP, SAMPLER, raw=True)[:2]
        on(t)
        with pytest.raises(q3.Q3Error) as err:
            t.generate_many_lookup_draw(PROMPTS, N_NEW, SAMPLER, STOP)
        assert err.value.code == -5 and word in err.value.msg
        off(t)
        assert t.generate_many_lookup_draw(PROMPTS, N_NEW, SAMPLER, STOP, ngram=NGRAM, raw=True)[:2] == want
