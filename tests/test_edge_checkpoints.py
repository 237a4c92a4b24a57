"""Every decode path on edge-valued checkpoints (tests/edge_ckpt.py), bit for bit against the oracle.

The batched paths -- batched decode, dense prefill, draft verification, column passes, the device-resident loops and the sampler
behind them -- have no operator entry points, so their special-case branches (exp outside its main range, SwiGLU at +-88, all-zero
quantizer groups, ties in token selection) are reached here through the checkpoint: its norm vectors and int8 rows are set so that
the reference itself walks into each case.

Two parts.  The unmarked part runs the numpy reference alone (oracle.np_oracle.NpQwen3 with its softmax / swiglu / quantize wrapped)
over every (shape, edit, schedule) the GPU part uses and asserts that the edge is really reached: these are conditions, and a GPU
case is listed only if its witness holds.  The GPU part compares every path with the C oracle directly -- never only with
q3_forward, so that forward and a batched path cannot share a mistake.

Schedules.  Every single-stream path computes the same forwards: greedy decode from TOK0 at position 0 (G = the greedy tokens), so
prefill and verify of [TOK0] + G[:k-1] and the column runs must reproduce the rows of one oracle run.  Batched decode runs
`streams()`: ragged start positions over a zeroed cache."""
import numpy as np
import pytest

import edge_ckpt
from conftest import assert_biteq, bits
from spec_sim import simulate

gpu = pytest.mark.gpu

TOK0 = 3
# shape -> engine context, single-stream positions, prompt lengths of the dense prefill (both sides of a 16-position tile / of 256)
SHAPES = {
    "tiny-g64": dict(ctx=0, n=24, prefill=(15, 17, 24)),                  # head_dim 64: generic forms, k_attn_gqa*
    "small-hd128": dict(ctx=0, n=81, prefill=(15, 17, 81)),               # head_dim 128: k_attn_short2, k_attn_pf2
    "small-longctx": dict(ctx=512, n=257, prefill=(17, 81, 257)),         # the split path, multi-chunk rows, k_value_transpose
    "qwen3-0.6b-dims-l2": dict(ctx=64, n=12, prefill=()),                 # shape-specialised k_gemv, k_bquant_split<.., 1024, ..>
    "qwen3-4b-dims-l2": dict(ctx=64, n=0, prefill=()),                    # rows with masked tail groups; batched decode only
    "tiny-g64-untied": dict(ctx=0, n=12, prefill=()),                     # its own lm_head: the other branch of tied_classifier
}
SEPARATE = ["hot_scores", "far_scores", "hot_gate", "zero_groups", "zero_keys", "tied_classifier", "flat_logits"]
SINGLE = ([("tiny-g64", e) for e in SEPARATE + ["all"]] + [("small-hd128", e) for e in SEPARATE + ["all"]] +
          [("small-longctx", "hot_scores"), ("small-longctx", "far_scores"), ("small-longctx", "all"), ("small-longctx", "tied_classifier"),
           ("qwen3-0.6b-dims-l2", "all"), ("qwen3-0.6b-dims-l2", "tied_classifier"), ("tiny-g64-untied", "tied_classifier")])
PREFILL = [(s, e) for s, e in SINGLE if SHAPES[s]["prefill"]]
BATCH = ([(s, e, n) for s in ("tiny-g64", "small-hd128") for e in SEPARATE + ["all"] for n in (3, 17)] +
         [("small-longctx", "hot_scores", 3), ("small-longctx", "far_scores", 3), ("small-longctx", "all", 17), ("qwen3-0.6b-dims-l2", "all", 17),
          ("qwen3-4b-dims-l2", "all", 17), ("tiny-g64-untied", "tied_classifier", 3)])
SPEC = [(s, e) for s in ("tiny-g64", "small-hd128") for e in ("tied_classifier", "flat_logits", "all", "far_scores")]
COLS = ([(s, e) for s in ("tiny-g64", "small-hd128") for e in ("all", "tied_classifier", "flat_logits")] +
        [(s, e) for s in ("small-longctx", "qwen3-0.6b-dims-l2") for e in ("all", "tied_classifier")])
COLS_RUN, COLS_LAST = 11, 11      # positions of the mixed pass's run / of the longest generate_many_greedy request
DRAW = [(s, e) for s in ("tiny-g64", "small-hd128") for e in ("tied_classifier", "flat_logits")]
SAMPLERS = [(1.0, 1.0), (0.7, 0.9), (1.0, 0.0)]
DRAW_SEED, N_DRAW = 42, 16
FAST = [(s, e) for s in ("tiny-g64", "small-hd128") for e in ("tied_classifier", "flat_logits")]
N_SPEC = 24                       # tokens of the prompt-lookup runs
VERIFY_N, VERIFY_WRONG = 8, (1, 4, 7)


def streams(name, n_streams):
    """(first tokens, first positions, steps) of the batched-decode schedule: ragged starts over a zeroed cache; on small-longctx one
    stream starts at 253 so that its steps cross position 256"""
    V = edge_ckpt.SHAPES[name].vocab_size
    toks = [(37 * i + TOK0) % V for i in range(n_streams)]
    pos = [(5 * i) % 7 for i in range(n_streams)]
    steps = 4
    if name == "small-longctx":
        pos[2], steps = 253, 6
    if name == "qwen3-4b-dims-l2":
        steps = 2
    return toks, pos, steps


def twins(G, every=5):
    """the prompt-lookup corpus that proposes the even twin: G with every 5th token's lowest bit flipped"""
    return [g ^ 1 if i % every == every - 1 else g for i, g in enumerate(G)]


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    d = tmp_path_factory.mktemp("edge")

    def get(name, edit):
        return edge_ckpt.write(str(d / f"{name}-{edit}.bin"), name, edit)
    return get


# ---------------------------------------------------------------------------------------------------------------------
# part 1 (no GPU): the numpy reference reaches the edge on every case of part 2
# ---------------------------------------------------------------------------------------------------------------------
def assert_witness(edit, steps, shape, what):
    """the conditions of the edit over the recorded forwards `steps` (edge_ckpt.Recorder.steps)"""
    L = shape.n_layers
    parts = {"all": ["hot_scores", "hot_gate", "zero_groups", "tied_classifier"]}.get(edit, [edit])
    for s in steps:
        assert np.isfinite(s["logits"]).all(), what
    if "hot_scores" in parts:
        for l in range(L):
            assert sum(s["cold_rows"][l] for s in steps) >= 1, f"{what}: no softmax input <= -88 below its row maximum in layer {l}"
        assert sum(s["subnormal"] for s in steps) >= 1, f"{what}: no subnormal probability"
    if "far_scores" in parts:
        for l in range(L):
            assert sum(s["far"][l] for s in steps) >= 1, f"{what}: no softmax input <= -750 below its row maximum in layer {l}"
    if "hot_gate" in parts:
        assert sum(s["gate_lo"] for s in steps) >= 1, f"{what}: no gate below -88.8"
        assert sum(s["gate_hi"] for s in steps) >= 1, f"{what}: no gate above 88"
        assert sum(s["swiglu_negzero"] for s in steps) >= 1, f"{what}: no -0.0 SwiGLU output"
    if "zero_groups" in parts:
        for s in steps:
            for site in (0, 1, 3):                             # QKV input, Wo input, W2 input
                assert all(c >= 1 for c in s["zero_groups"][site]), f"{what}: no zero group at quantizer site {site}"
        for l in range(L):
            assert sum(s["hidden_negzero"][l] for s in steps) >= 1, f"{what}: no -0.0 in a zero hidden-buffer group, layer {l}"
    if "zero_keys" in parts:
        for l in range(L):
            assert sum(s["uniform_rows"][l] for s in steps) >= 1, f"{what}: no uniform softmax row in layer {l}"
    if "tied_classifier" in parts:
        for s in steps:
            lg = s["logits"]
            at = np.nonzero(lg == lg.max())[0]
            assert at.size == 2 and at[0] % 2 == 0 and at[1] == at[0] + 1, f"{what}: maximum at {at}"
            assert np.array_equal(bits(lg[0::2]), bits(lg[1::2])), what
    if "flat_logits" in parts:
        for s in steps:
            assert not bits(s["logits"]).any(), f"{what}: a logit is not +0.0"


@pytest.fixture
def recorded(np_oracle, ckpt, monkeypatch):
    def get(name, edit):
        rec = edge_ckpt.Recorder(np_oracle, edge_ckpt.SHAPES[name])
        rec.install(monkeypatch.setattr)
        return rec, np_oracle.NpQwen3(ckpt(name, edit), SHAPES[name]["ctx"])
    return get


@pytest.mark.parametrize("name,edit", SINGLE)
def test_witness_single_stream(np_oracle, recorded, name, edit):
    """greedy decode from TOK0 for n positions; the conditions hold on every prefix a dense-prefill case uses, on the verify block
    and on the prompt-lookup run as well"""
    rec, m = recorded(name, edit)
    shape, n = edge_ckpt.SHAPES[name], SHAPES[name]["n"]
    tok, G = TOK0, []
    for pos in range(n):
        tok = np_oracle.argmax_last(rec.forward(m, tok, pos))
        G.append(tok)
    lengths = {n} | set(SHAPES[name]["prefill"])
    if (name, edit) in SPEC:
        lengths |= {VERIFY_N, N_SPEC}
    if (name, edit) in COLS:
        lengths |= {COLS_RUN, COLS_LAST}
    for k in sorted(lengths):
        assert_witness(edit, rec.steps[:k], shape, f"{name} {edit} first {k} positions")
    if edit == "flat_logits":
        assert G == [shape.vocab_size - 1] * n
    if edit in ("tied_classifier", "all"):
        assert all(g % 2 == 1 for g in G)
    if (name, edit) in SPEC:                                   # the corpus proposes right tokens and even twins
        if edit != "far_scores":
            assert all(g % 2 == 1 for g in G[:N_SPEC])
        sim = simulate(G[:N_SPEC], twins(G[:N_SPEC]), TOK0, 1, 8)
        assert sim["drafted"] > sim["accepted"] > 0, sim


@pytest.mark.parametrize("name,edit,n_streams", BATCH)
def test_witness_batched_schedule(np_oracle, recorded, name, edit, n_streams):
    rec, m = recorded(name, edit)
    toks, pos, steps = streams(name, n_streams)
    for t0, p0 in zip(toks, pos):
        m.key[:] = 0
        m.val[:] = 0
        tok = t0
        for k in range(steps):
            tok = np_oracle.argmax_last(rec.forward(m, tok, p0 + k))
    assert_witness(edit, rec.steps, edge_ckpt.SHAPES[name], f"{name} {edit} {n_streams} streams")


@pytest.mark.parametrize("T,p", SAMPLERS)
@pytest.mark.parametrize("name,edit", DRAW)
def test_witness_sampled_schedule(np_oracle, recorded, name, edit, T, p):
    rec, m = recorded(name, edit)
    shape = edge_ckpt.SHAPES[name]
    s = np_oracle.NpSampler(shape.vocab_size, T, p, DRAW_SEED)
    tok = TOK0
    for pos in range(N_DRAW):
        tok = s.sample(rec.forward(m, tok, pos))
    assert_witness(edit, rec.steps, shape, f"{name} {edit} T {T} p {p}")


# ---------------------------------------------------------------------------------------------------------------------
# part 2 (GPU): every path against the C oracle
# ---------------------------------------------------------------------------------------------------------------------
_refs = {}


def engine(q3, path, name, fast=False):
    b = q3.TransformerBuilder(path).with_ctx_length(SHAPES[name]["ctx"] or None)
    return (b.with_strict(False) if fast else b).build()


def greedy_ref(oracle, path, name, tok0=TOK0, pos0=0, n=None):
    """the C oracle's greedy loop over a zeroed cache: (tokens, logits [n, V], key cache, value cache); computed once"""
    n = SHAPES[name]["n"] if n is None else n
    key = (path, tok0, pos0, n)
    if key not in _refs:
        om = oracle.OracleModel(path, SHAPES[name]["ctx"])
        tok, G, LG = tok0, [], []
        for k in range(n):
            lg = om.forward(tok, pos0 + k)
            tok = oracle.sample_argmax(lg)
            G.append(tok)
            LG.append(lg)
        K, V = om.kv_cache()
        om.close()
        for a in (K, V):
            a.setflags(write=False)
        _refs[key] = (G, np.stack(LG), K, V)
    return _refs[key]


def sampled_ref(oracle, path, name, T, p):
    """the C oracle's sampled loop: (tokens, rng state after each draw)"""
    key = (path, T, p)
    if key not in _refs:
        om = oracle.OracleModel(path, SHAPES[name]["ctx"])
        s = oracle.Sampler(om.get_config().vocab_size, T, p, DRAW_SEED)
        tok, S, states = TOK0, [], []
        for pos in range(N_DRAW):
            tok = s.sample(om.forward(tok, pos))
            S.append(tok)
            states.append(int(s.rng_state.value))
        om.close()
        _refs[key] = (S, states)
    return _refs[key]


def first_rows(cache, n, pos0=0):
    """the oracle's cache with only rows pos0 .. pos0 + n - 1 kept: what a run of n positions over a zeroed cache leaves"""
    out = np.zeros_like(cache)
    out[:, pos0:pos0 + n] = cache[:, pos0:pos0 + n]
    return out


def check_caches(t, K, V, n, what):
    assert_biteq(t.read_state("key"), first_rows(K, n).reshape(-1), f"{what}: key rows")
    assert_biteq(t.read_state("value"), first_rows(V, n).reshape(-1), f"{what}: value rows")


def check_flat(shape, tokens, logits=None):
    assert list(tokens) == [shape.vocab_size - 1] * len(tokens)
    if logits is not None:
        assert not bits(logits).any(), "a logit is not +0.0"


@gpu
@pytest.mark.parametrize("name,edit", SINGLE)
def test_forward_greedy_loop_and_prefill(q3, oracle, ckpt, name, edit):
    """q3_forward (logits, K/V rows), q3_generate_greedy (the device loop) and q3_prefill"""
    path, n, shape = ckpt(name, edit), SHAPES[name]["n"], edge_ckpt.SHAPES[name]
    G, LG, K, V = greedy_ref(oracle, path, name)
    with engine(q3, path, name) as t:
        tok = TOK0
        for pos in range(n):
            lg = np.array(t.forward(tok, pos), copy=True)
            assert_biteq(lg, LG[pos], f"logits at position {pos}")
            tok = G[pos]
        check_caches(t, K, V, n, "forward")
        t.reset_kv()
        got = t.generate_greedy(TOK0, 0, n)
        assert got == G
        check_caches(t, K, V, n, "generate_greedy")
        t.reset_kv()
        assert t.prefill([TOK0] + G[:n - 1], 0) == G[n - 1]
        check_caches(t, K, V, n, "prefill")
    if edit == "flat_logits":
        check_flat(shape, got, LG)


@gpu
@pytest.mark.parametrize("name,edit", PREFILL)
def test_prefill_batched(q3, oracle, ckpt, name, edit):
    """q3_prefill_batched at prompt lengths on both sides of a 16-position tile and of 256: cache rows and the next token"""
    path = ckpt(name, edit)
    G, _, K, V = greedy_ref(oracle, path, name)
    with engine(q3, path, name) as t:
        for k in SHAPES[name]["prefill"]:
            t.reset_kv()
            assert t.prefill([TOK0] + G[:k - 1], 0, batched=True) == G[k - 1], f"token behind {k} positions"
            check_caches(t, K, V, k, f"{k} positions")
    if edit == "flat_logits":
        check_flat(edge_ckpt.SHAPES[name], G)


def run_batched(q3, oracle, path, name, n_streams):
    shape = edge_ckpt.SHAPES[name]
    toks0, pos0, steps = streams(name, n_streams)
    refs = [greedy_ref(oracle, path, name, toks0[i], pos0[i], steps) for i in range(n_streams)]
    with engine(q3, path, name) as t:
        t.batch_init(n_streams)
        toks = list(toks0)
        for k in range(steps):
            lg, am = t.forward_batch(toks, [p + k for p in pos0])
            for i, (G, LG, _, _) in enumerate(refs):
                assert_biteq(lg[i], LG[k], f"stream {i} step {k} logits")
                assert am[i] == G[k], f"stream {i} step {k} token"
            toks = am
        for i, (_, _, K, V) in enumerate(refs):
            assert_biteq(t.batch_read_state(i, "key"), first_rows(K, steps, pos0[i]).reshape(-1), f"stream {i} key cache")
            assert_biteq(t.batch_read_state(i, "value"), first_rows(V, steps, pos0[i]).reshape(-1), f"stream {i} value cache")
        t.batch_reset_kv()
        out = t.generate_greedy_batch(toks0, pos0, steps)
        for i, (G, _, K, V) in enumerate(refs):
            assert [int(v) for v in out[i]] == G, f"stream {i} of the device loop"
            assert_biteq(t.batch_read_state(i, "key"), first_rows(K, steps, pos0[i]).reshape(-1), f"stream {i} key cache, device loop")
            assert_biteq(t.batch_read_state(i, "value"), first_rows(V, steps, pos0[i]).reshape(-1), f"stream {i} value cache, device loop")
    return shape, refs


@gpu
@pytest.mark.parametrize("name,edit,n_streams", BATCH)
def test_batched_decode(q3, oracle, ckpt, name, edit, n_streams):
    """q3_forward_batch / q3_generate_greedy_batch: per-stream logits, tokens and caches against the oracle's per-stream runs"""
    shape, refs = run_batched(q3, oracle, ckpt(name, edit), name, n_streams)
    if edit == "flat_logits":
        for G, LG, _, _ in refs:
            check_flat(shape, G, LG)


@gpu
@pytest.mark.parametrize("form", range(1, 7))
def test_batched_decode_forms(q3, oracle, ckpt, form, dev_forms):
    """the forms of the batched step the planner takes on other shapes (test_gpu_parity._DGEMM_FORMS), on `all`"""
    from test_gpu_parity import _DGEMM_FORMS
    dev_forms(_DGEMM_FORMS[form])
    run_batched(q3, oracle, ckpt("qwen3-0.6b-dims-l2", "all"), "qwen3-0.6b-dims-l2", 17)


@gpu
@pytest.mark.parametrize("name,edit", SPEC)
def test_verify_rejects_the_even_twin(q3, oracle, ckpt, name, edit):
    """q3_verify: the all-right draft is accepted; a draft holding the even twin of the right token -- a logit equal to the maximum,
    but not the last maximum -- is rejected at that index (first, middle, last draft of the block); tokens, logits and restored rows"""
    path = ckpt(name, edit)
    G, LG, K, V = greedy_ref(oracle, path, name)
    n = VERIFY_N
    with engine(q3, path, name) as t:
        nxt, a, lg = t.verify([TOK0] + G[:n - 1], 0, want_logits=True)
        assert a == n - 1 and nxt == G[:n]
        assert_biteq(lg, LG[:n], "logits of the accepted block")
        check_caches(t, K, V, n, "accepted block")
        for j in VERIFY_WRONG:
            block = [TOK0] + G[:n - 1]
            assert block[j] % 2 == 1 or edit == "far_scores"       # (far_scores has no twins: any wrong draft)
            block[j] ^= 1
            t.reset_kv()
            nxt, a, lg = t.verify(block, 0, want_logits=True)
            assert a == j - 1, f"even twin at draft {j}: {a} accepted"
            assert nxt[:j] == G[:j]
            assert_biteq(lg[:j], LG[:j], f"logits before the twin at {j}")
            check_caches(t, K, V, j, f"even twin at draft {j}")
            if edit == "flat_logits":                          # the commit folds a maximum that ties across every classifier workgroup
                check_flat(edge_ckpt.SHAPES[name], nxt, lg)
    if edit == "flat_logits":
        check_flat(edge_ckpt.SHAPES[name], G[:n], LG[:n])


@gpu
@pytest.mark.parametrize("name,edit", SPEC)
def test_generate_lookup_with_twins_in_the_corpus(q3, oracle, ckpt, name, edit):
    """q3_generate_lookup over a corpus that proposes the even twin: the oracle's greedy tokens, the simulated statistics"""
    path = ckpt(name, edit)
    G, _, K, V = greedy_ref(oracle, path, name)
    G = G[:N_SPEC]
    sim = simulate(G, twins(G), TOK0, 1, 8)
    with engine(q3, path, name) as t:
        got, st = t.generate_lookup(twins(G), TOK0, 0, N_SPEC, ngram=1, draft_len=8)
        assert got == G
        assert (st.verify_passes, st.single_steps, st.drafted, st.accepted) == (sim["verify_passes"], sim["single_steps"], sim["drafted"], sim["accepted"])
        check_caches(t, K, V, N_SPEC, "generate_lookup")
        t.reset_kv()
        assert t.generate_greedy(TOK0, 0, N_SPEC) == G
    if edit == "flat_logits":
        check_flat(edge_ckpt.SHAPES[name], got)


@gpu
@pytest.mark.parametrize("T,p", SAMPLERS)
@pytest.mark.parametrize("name,edit", DRAW)
def test_sampled_paths(q3, oracle, ckpt, name, edit, T, p):
    """q3_generate_sampled, q3_verify_draw and q3_generate_lookup_draw where probabilities tie (pairs under tied_classifier, the whole
    vocabulary under flat_logits): tokens and rng state equal oracle.Sampler's, so the device sort keeps the reference's stable order"""
    path, V = ckpt(name, edit), edge_ckpt.SHAPES[name].vocab_size
    S, states = sampled_ref(oracle, path, name, T, p)
    n = VERIFY_N
    with engine(q3, path, name) as t:
        t.set_sampler(T, p, DRAW_SEED)
        assert t.generate_greedy(TOK0, 0, N_DRAW) == S         # q3_generate_sampled: the same loop with the sampler set
        assert t.sampler_rng_state() == states[-1]
        t.reset_kv()
        t.set_sampler(T, p, DRAW_SEED)
        nxt, a = t.verify_draw([TOK0] + S[:n - 1], 0)
        assert a == n - 1 and nxt == S[:n]
        assert t.sampler_rng_state() == states[n - 1]
        for j in VERIFY_WRONG:
            block = [TOK0] + S[:n - 1]
            block[j] = block[j] ^ 1 if edit == "tied_classifier" else (block[j] + 1) % V
            t.reset_kv()
            t.set_sampler(T, p, DRAW_SEED)
            nxt, a = t.verify_draw(block, 0)
            assert a == j - 1 and nxt[:j] == S[:j], f"wrong draft {j}"
            assert t.sampler_rng_state() == states[j - 1]
        t.reset_kv()
        t.set_sampler(T, p, DRAW_SEED)
        got, _ = t.generate_lookup_draw(twins(S), TOK0, 0, N_DRAW, ngram=1, draft_len=8)
        assert got == S
        assert t.sampler_rng_state() == states[-1]


@gpu
@pytest.mark.parametrize("name,edit", COLS)
def test_column_passes(q3, oracle, ckpt, name, edit):
    """q3_batch_step_cols: one mixed pass, a run of 11 next to two decode columns; q3_generate_many_greedy: three requests through two
    slots.  Every column is a row of the oracle's greedy run."""
    path = ckpt(name, edit)
    G, LG, K, V = greedy_ref(oracle, path, name)
    seq = [TOK0] + G
    with engine(q3, path, name) as t:
        t.batch_init(3)
        r = COLS_RUN
        t.batch_step_cols([1] * 5, seq[:5], list(range(5)))                            # slot 1: positions 0 .. 4
        lg, am = t.batch_step_cols([0] * r + [1, 2], seq[:r] + [seq[5], seq[0]], list(range(r)) + [5, 0], want_logits=True)
        assert_biteq(lg[:r], LG[:r], "run from position 0")
        assert_biteq(lg[r], LG[5], "decode column at position 5")
        assert_biteq(lg[r + 1], LG[0], "decode column at position 0")
        assert am == G[:r] + [G[5], G[0]]
        for slot, rows in ((0, r), (1, 6), (2, 1)):
            assert_biteq(t.batch_read_state(slot, "key"), first_rows(K, rows).reshape(-1), f"slot {slot} key rows")
            assert_biteq(t.batch_read_state(slot, "value"), first_rows(V, rows).reshape(-1), f"slot {slot} value rows")
    with engine(q3, path, name) as t:
        t.batch_init(2)
        lens, new = (1, 5, 9), (6, 4, 3)                       # the last request forwards positions 0 .. COLS_LAST - 1
        rows, _ = t.generate_many_greedy([seq[:k] for k in lens], list(new))
        for r, (k, m) in enumerate(zip(lens, new)):
            assert rows[r] == G[k - 1:k - 1 + m], f"request {r}"
    if edit == "flat_logits":
        check_flat(edge_ckpt.SHAPES[name], am + [x for r in rows for x in r], lg)


@gpu
@pytest.mark.parametrize("name,edit", FAST)
def test_fast_mode_keeps_what_numerics_cannot_blur(q3, ckpt, name, edit):
    """Q3_FLAG_FAST: equal classifier rows give bit-equal logits and the last maximum is the odd index; all-zero logits give
    vocab_size - 1 -- in forward, forward_batch and prefill_batched.  No tolerance is set on these checkpoints."""
    path, shape = ckpt(name, edit), edge_ckpt.SHAPES[name]

    def check(tok, lg=None):
        if edit == "flat_logits":
            assert tok == shape.vocab_size - 1
        else:
            assert tok % 2 == 1
            if lg is not None:
                assert np.array_equal(bits(lg[0::2]), bits(lg[1::2])), "twin logits differ"
                assert tok == q3.sample_argmax(lg)

    with engine(q3, path, name, fast=True) as t:
        tok, seq = TOK0, [TOK0]
        for pos in range(8):
            lg = np.array(t.forward(tok, pos), copy=True)
            tok = t.forward_argmax(tok, pos)
            check(tok, lg)
            seq.append(tok)
        for k in (15, 17):
            t.reset_kv()
            check(t.prefill((seq * 3)[:k], 0, batched=True))
        toks, pos, _ = streams(name, 3)
        t.batch_init(3)
        for k in range(3):
            lg, am = t.forward_batch(toks, [p + k for p in pos])
            for i in range(3):
                check(am[i], lg[i])
            toks = am
