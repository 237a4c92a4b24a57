"""GPU tests of section 2c of include/qwen3_hip.h: q3_verify (one weight pass over a block of drafted tokens) and
q3_generate_lookup (greedy decode with prompt-lookup drafts).  Every equality is bit for bit; the yardstick is always
q3_generate_greedy / q3_forward on a second, fresh engine, plus the C oracle on tiny-g64.  Expected statistics come from the
loop restated in Python (spec_sim.simulate), never from an acceptance rate."""
import os

import numpy as np
import pytest

from conftest import assert_biteq, golden_path
from spec_sim import simulate

pytestmark = pytest.mark.gpu

# shape -> (checkpoint seed, first token, context length for the engine; 0 = the checkpoint's)
MODELS = {
    "tiny-g64": (99, 3, 0),                 # seq_len 96
    "small-hd128": (21, 17, 0),             # seq_len 256, head_dim 128
    "small-longctx": (99, 3, 512),          # head_dim 64, context past the split attention path
    "qwen3-0.6b-dims-l2": (1235, 11, 512),
    "qwen3-4b-dims-l2": (1235, 11, 512),
    "qwen3-8b-dims-l2": (1235, 11, 512),
}
N_REF = 60


@pytest.fixture(scope="module")
def ckpt(q3, tmp_path_factory):
    made = {}

    def get(name, seed=None):
        seed = MODELS[name][0] if seed is None else seed
        if (name, seed) not in made:
            path = str(tmp_path_factory.mktemp("spec") / f"{name}-{seed}.bin")
            q3.checkpoint.write_synthetic_checkpoint(path, q3.checkpoint.SHAPES[name], seed=seed)
            made[(name, seed)] = path
        return made[(name, seed)]
    return get


def engine(q3, path, ctx, flags=0):
    b = q3.TransformerBuilder(path)
    if ctx:
        b = b.with_ctx_length(ctx)
    b.flags |= flags
    return b.build()


_refs = {}


def reference(q3, path, ctx, tok0, p0, n, extra=16):
    """G = generate_greedy(tok0, p0, n) on a fresh engine, the whole caches after it, `extra` further greedy tokens and the logits
    of one forward after those."""
    key = (path, ctx, tok0, p0, n, extra)
    if key not in _refs:
        with engine(q3, path, ctx) as t:
            G = t.generate_greedy(tok0, p0, n)
            k, v = t.read_state("key"), t.read_state("value")
            more = t.generate_greedy(G[-1], p0 + n, extra) if extra else []
            lg = np.array(t.forward(more[-1], p0 + n + extra), copy=True) if extra else None
        _refs[key] = (G, k, v, more, lg)
    return _refs[key]


def check_continues(t, G, p0, n, more, lg):
    extra = len(more)
    assert t.generate_greedy(G[-1], p0 + n, extra) == more
    assert_biteq(t.forward(more[-1], p0 + n + extra), lg, "logits of a forward after the speculative run")


# ---------------------------------------------------------------------------------------------------------------------
# q3_verify
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_verify_all_drafts_right(q3, ckpt, name):
    """Walking the greedy tokens G in blocks of n: every draft is accepted, next_tokens are G, and the WHOLE caches equal those of
    the greedy loop over the same number of tokens."""
    seed, tok0, ctx = MODELS[name]
    path = ckpt(name)
    G = reference(q3, path, ctx, tok0, 0, 64, extra=0)[0]
    with engine(q3, path, ctx) as t, engine(q3, path, ctx) as ref:
        for n in (1, 2, 5, 16, 32):
            t.reset_kv()
            ref.reset_kv()
            cur, k = tok0, 0
            while k + n <= 64:
                nxt, a = t.verify([cur] + G[k:k + n - 1], k)
                assert a == n - 1, (n, k, a)
                assert nxt == G[k:k + n], (n, k)
                cur, k = G[k + n - 1], k + n
            assert ref.generate_greedy(tok0, 0, k) == G[:k]
            assert_biteq(t.read_state("key"), ref.read_state("key"), f"key cache, blocks of {n}")
            assert_biteq(t.read_state("value"), ref.read_state("value"), f"value cache, blocks of {n}")


@pytest.mark.parametrize("name", list(MODELS))
def test_verify_first_wrong_draft_at_every_index(q3, ckpt, name):
    """Draft j replaced by (t + 1) % vocab, for every j in 1..n-1: n_accepted == j - 1, the returned prefix is right and the whole
    caches are those of an engine that ran exactly j greedy steps."""
    seed, tok0, ctx = MODELS[name]
    path = ckpt(name)
    G = reference(q3, path, ctx, tok0, 0, 64, extra=0)[0]
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    with engine(q3, path, ctx) as t, engine(q3, path, ctx) as ref:
        after = {}
        for j in range(1, 32):
            ref.reset_kv()
            assert ref.generate_greedy(tok0, 0, j) == G[:j]
            after[j] = (ref.read_state("key"), ref.read_state("value"))
        for n in (2, 5, 16, 32):
            for j in range(1, n):
                block = [tok0] + G[:n - 1]
                block[j] = (block[j] + 1) % vocab
                t.reset_kv()
                nxt, a = t.verify(block, 0)
                assert a == j - 1, (n, j, a)
                assert nxt[:j] == G[:j], (n, j)
                assert_biteq(t.read_state("key"), after[j][0], f"key cache, n {n}, first wrong draft {j}")
                assert_biteq(t.read_state("value"), after[j][1], f"value cache, n {n}, first wrong draft {j}")


@pytest.mark.parametrize("name", list(MODELS))
def test_verify_restores_rows_that_held_data(q3, ckpt, name):
    """The same on a cache that already holds non-zero rows past the block (64 decoded tokens, then a block at position 8 inside
    them): rejected rows come back as they WERE, not zeroed -- the whole cache stays that of the 64-token decode."""
    seed, tok0, ctx = MODELS[name]
    path = ckpt(name)
    G, want_k, want_v, _, _ = reference(q3, path, ctx, tok0, 0, 64, extra=0)
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    with engine(q3, path, ctx) as t:
        assert t.generate_greedy(tok0, 0, 64) == G
        for n, js in ((32, range(1, 32)), (5, range(1, 5))):
            for j in js:
                block = G[7:7 + n]                                 # G[7] is the input at position 8
                block[j] = (block[j] + 1) % vocab
                nxt, a = t.verify(block, 8)
                assert a == j - 1 and nxt[:j] == G[8:8 + j], (n, j, a)
                assert_biteq(t.read_state("key"), want_k, f"key cache, n {n}, first wrong draft {j}")
                assert_biteq(t.read_state("value"), want_v, f"value cache, n {n}, first wrong draft {j}")
        assert t.generate_greedy(G[39], 40, 24) == G[40:]


@pytest.mark.parametrize("name", list(MODELS))
def test_verify_logits_equal_forward(q3, ckpt, name):
    """logits_out row i == q3_forward(tokens[i], first_pos + i) on a fresh engine fed the same token prefix, rows behind a rejected
    draft included."""
    seed, tok0, ctx = MODELS[name]
    path = ckpt(name)
    G = reference(q3, path, ctx, tok0, 0, 64, extra=0)[0]
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    for n, wrong in ((6, 3), (32, None), (17, 1)):
        block = G[3:3 + n]                                         # G[3] is the input at position 4
        if wrong is not None:
            block[wrong] = (block[wrong] + 1) % vocab
        with engine(q3, path, ctx) as t:
            t.generate_greedy(tok0, 0, 4)                          # the block starts at position 4 behind four real rows
            nxt, a, lg = t.verify(block, 4, want_logits=True)
            assert a == (n - 1 if wrong is None else wrong - 1)
        with engine(q3, path, ctx) as ref:
            ref.generate_greedy(tok0, 0, 4)
            for i, tk in enumerate(block):
                want = np.array(ref.forward(tk, 4 + i), copy=True)
                assert_biteq(lg[i], want, f"logits row {i} of a block of {n}")
                assert nxt[i] == q3.sample_argmax(want)


# ---------------------------------------------------------------------------------------------------------------------
# q3_generate_lookup
# ---------------------------------------------------------------------------------------------------------------------
def corpus_of(kind, G, vocab):
    if kind == "empty":
        return []
    if kind == "G":
        return list(G)
    if kind == "G7":                                               # every 7th token altered
        return [(g + 1) % vocab if i % 7 == 6 else g for i, g in enumerate(G)]
    rng = np.random.default_rng(7)                                 # "random": tokens of G in random order -- 1-grams match, continuations rarely
    return [int(G[i]) for i in rng.integers(0, len(G), 80)]


# (corpus, ngram, draft_len, first_pos)
LOOKUP_CASES = [
    ("empty", 2, 4, 0), ("G", 2, 31, 0), ("G7", 2, 4, 0), ("random", 1, 4, 0), ("empty", 1, 1, 0), ("empty", 3, 31, 5),
    ("G", 3, 4, 5), ("G7", 1, 31, 0), ("random", 2, 31, 5), ("empty", 64, 4, 0), ("G7", 3, 1, 0),
]


def lookup_sims(q3, path, name):
    seed, tok0, ctx = MODELS[name]
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    out = []
    for kind, ngram, draft_len, p0 in LOOKUP_CASES:
        G = reference(q3, path, ctx, tok0, p0, N_REF)[0]
        corpus = corpus_of(kind, G, vocab)
        out.append((corpus, simulate(G, corpus, tok0, ngram, draft_len)))
    return out


@pytest.mark.parametrize("name", list(MODELS))
def test_lookup_cases_take_every_branch(q3, ckpt, name):
    """A condition on the chosen inputs, asserted on the simulation alone: over the cases of this shape there is a single-stream
    step, a fully accepted draft, a partly accepted draft and a draft rejected at its first token; ngram 64 never drafts."""
    sims = lookup_sims(q3, ckpt(name), name)
    passes = [p for _, s in sims for p in s["passes"]]
    assert any(s["single_steps"] > 0 for _, s in sims)
    assert any(a == d for d, a in passes), "no fully accepted draft"
    assert any(0 < a < d for d, a in passes), "no partly accepted draft"
    assert any(a == 0 for d, a in passes), "no draft rejected at its first token"
    for (kind, ngram, _, _), (_, s) in zip(LOOKUP_CASES, sims):
        if ngram == 64:
            assert s["verify_passes"] == 0 and s["single_steps"] == N_REF


@pytest.mark.parametrize("case", range(len(LOOKUP_CASES)), ids=[f"{c[0]}-g{c[1]}-d{c[2]}-p{c[3]}" for c in LOOKUP_CASES])
@pytest.mark.parametrize("name", list(MODELS))
def test_generate_lookup_equals_generate_greedy(q3, ckpt, name, case):
    """Tokens, whole caches, the four statistics of the simulation, then 16 plain greedy steps and one forward's logits on the
    same engine -- all equal to the plain greedy run."""
    seed, tok0, ctx = MODELS[name]
    path = ckpt(name)
    kind, ngram, draft_len, p0 = LOOKUP_CASES[case]
    G, want_k, want_v, more, lg = reference(q3, path, ctx, tok0, p0, N_REF)
    corpus, sim = lookup_sims(q3, path, name)[case]
    with engine(q3, path, ctx) as t:
        got, st = t.generate_lookup(corpus, tok0, p0, N_REF, ngram=ngram, draft_len=draft_len)
        assert got == G
        assert (st.verify_passes, st.single_steps, st.drafted, st.accepted) == \
               (sim["verify_passes"], sim["single_steps"], sim["drafted"], sim["accepted"]), (st, sim)
        assert_biteq(t.read_state("key"), want_k, "key cache after generate_lookup")
        assert_biteq(t.read_state("value"), want_v, "value cache after generate_lookup")
        check_continues(t, G, p0, N_REF, more, lg)


def test_generate_lookup_eager_launches(q3, ckpt):
    """Q3_FLAG_NO_GRAPH: the pass launched kernel by kernel instead of replayed"""
    name = "small-hd128"
    seed, tok0, ctx = MODELS[name]
    path = ckpt(name)
    G, want_k, want_v, more, lg = reference(q3, path, ctx, tok0, 0, N_REF)
    with engine(q3, path, ctx, flags=q3.FLAG_NO_GRAPH) as t:
        got, st = t.generate_lookup(G, tok0, 0, N_REF, ngram=2, draft_len=8)
        assert got == G and st.verify_passes > 0
        assert_biteq(t.read_state("key"), want_k, "key cache")
        assert_biteq(t.read_state("value"), want_v, "value cache")
        check_continues(t, G, 0, N_REF, more, lg)


@pytest.mark.parametrize("flags", [0, 4], ids=["value_t", "no_value_t"])
@pytest.mark.parametrize("kind", ["G", "G7"])
def test_lookup_across_the_split_attention_path(q3, ckpt, kind, flags):
    """small-longctx from position 200 to 400 (crosses 256, where attention switches to the split kernels that stream the TRANSPOSED
    value cache): accepted rows must have their transposed columns, or the plain greedy steps afterwards diverge."""
    name = "small-longctx"
    seed, tok0, ctx = MODELS[name]
    path = ckpt(name)
    prompt = q3.checkpoint.iter_prompt_tokens(q3.checkpoint.SHAPES[name], 5, 200)
    with engine(q3, path, ctx) as ref:
        first = ref.prefill(prompt, 0)
        G = ref.generate_greedy(first, 200, 200)
        more = ref.generate_greedy(G[-1], 400, 16)
        want_k, want_v = ref.read_state("key"), ref.read_state("value")
    corpus = corpus_of(kind, G, q3.checkpoint.SHAPES[name].vocab_size)
    sim = simulate(G, corpus, first, 2, 8)
    assert sim["verify_passes"] > 0 and sim["accepted"] > 0
    with engine(q3, path, ctx, flags=flags) as t:
        assert t.prefill(prompt, 0) == first
        got, st = t.generate_lookup(corpus, first, 200, 200, ngram=2, draft_len=8)
        assert got == G
        assert (st.verify_passes, st.single_steps, st.drafted, st.accepted) == (sim["verify_passes"], sim["single_steps"], sim["drafted"], sim["accepted"])
        assert t.generate_greedy(G[-1], 400, 16) == more
        assert_biteq(t.read_state("key"), want_k, "key cache")
        assert_biteq(t.read_state("value"), want_v, "value cache")


@pytest.mark.parametrize("flags", [0, 4], ids=["value_t", "no_value_t"])
def test_verify_block_past_position_1024_4b_dims(q3, ckpt, flags):
    """qwen3-4b-dims-l2 at its full 4,096-position context: one 32-column pass and a lookup run behind a 1,030-token prompt, then
    plain greedy decode (the long-context kernels) continues identically."""
    name = "qwen3-4b-dims-l2"
    path = ckpt(name)
    shape = q3.checkpoint.SHAPES[name]
    prompt = q3.checkpoint.iter_prompt_tokens(shape, 5, 1030)
    with engine(q3, path, 0) as ref:
        first = ref.prefill(prompt, 0, batched=True)
        G = ref.generate_greedy(first, 1030, 72)
        want_k, want_v = ref.read_state("key"), ref.read_state("value")
    with engine(q3, path, 0, flags=flags) as t:
        assert t.prefill(prompt, 0, batched=True) == first
        nxt, a = t.verify([first] + G[:31], 1030)
        assert a == 31 and nxt == G[:32]
        block = [G[31]] + G[32:40]
        block[5] = (block[5] + 1) % shape.vocab_size
        nxt, a = t.verify(block, 1062)
        assert a == 4 and nxt[:5] == G[32:37]
        got, st = t.generate_lookup(G, G[36], 1067, 19, ngram=2, draft_len=8)
        assert got == G[37:56]
        assert t.generate_greedy(G[55], 1086, 16) == G[56:]
        assert_biteq(t.read_state("key"), want_k, "key cache")
        assert_biteq(t.read_state("value"), want_v, "value cache")


def test_verify_limits_and_refusals(q3, ckpt):
    """A block ending exactly at seq_len works; one past it, 33 tokens, a FAST engine, an active sampler and a group-32 checkpoint are
    refused with the documented status -- and the engine stays usable."""
    name = "tiny-g64"
    seed, tok0, ctx = MODELS[name]
    path = ckpt(name)
    S = q3.checkpoint.SHAPES[name].max_seq_len
    with engine(q3, path, 0) as ref:
        G = ref.generate_greedy(tok0, 0, S)
        want_k, want_v = ref.read_state("key"), ref.read_state("value")
    with engine(q3, path, 0) as t:
        assert t.generate_greedy(tok0, 0, S - 5) == G[:S - 5]
        with pytest.raises(IndexError):
            t.verify([G[S - 6]] + G[S - 5:S], S - 5)               # 6 tokens from S - 5: one past the end
        with pytest.raises(IndexError):
            t.verify([1] * 33, 0)
        with pytest.raises(IndexError):
            t.verify([], 0)
        with pytest.raises(IndexError):
            t.verify([1, 10 ** 6], 0)
        with pytest.raises(IndexError):
            t.generate_lookup([], tok0, 0, 8, ngram=0, draft_len=4)
        with pytest.raises(IndexError):
            t.generate_lookup([], tok0, 0, 8, ngram=2, draft_len=32)
        with pytest.raises(IndexError):
            t.generate_lookup([], tok0, S - 4, 5, ngram=2, draft_len=4)
        nxt, a = t.verify([G[S - 6]] + G[S - 5:S - 1], S - 5)      # 5 tokens: positions S - 5 .. S - 1
        assert a == 4 and nxt == G[S - 5:]
        assert_biteq(t.read_state("key"), want_k, "key cache, block ending at seq_len")
        assert_biteq(t.read_state("value"), want_v, "value cache, block ending at seq_len")
        t.set_sampler(0.8, 0.9, 1)
        with pytest.raises(q3.Q3Error) as err:
            t.verify([tok0, G[0]], 0)
        assert err.value.code == -5 and "temperature" in err.value.msg
        with pytest.raises(q3.Q3Error) as err:
            t.generate_lookup([], tok0, 0, 8)
        assert err.value.code == -5
        t.set_sampler(0.0, 0.9, 1)
        t.reset_kv()
        got, st = t.generate_lookup(G, tok0, 0, S, ngram=2, draft_len=31)       # a run that ends exactly at seq_len
        assert got == G and st.verify_passes > 0
        assert_biteq(t.read_state("key"), want_k, "key cache, run ending at seq_len")
    with engine(q3, path, 0, flags=q3.FLAG_FAST) as t:
        with pytest.raises(q3.Q3Error) as err:
            t.verify([tok0, G[0]], 0)
        assert err.value.code == -5 and "Q3_FLAG_FAST" in err.value.msg
        with pytest.raises(q3.Q3Error) as err:
            t.generate_lookup([], tok0, 0, 8)
        assert err.value.code == -5
        assert len(t.generate_greedy(tok0, 0, 4)) == 4
    with engine(q3, golden_path("tiny-untied.bin"), 0) as t:
        want = t.generate_greedy(5, 0, 6)
        t.reset_kv()
        with pytest.raises(q3.Q3Error) as err:
            t.verify([5, want[0]], 0)
        assert err.value.code == -5
        with pytest.raises(q3.Q3Error) as err:
            t.generate_lookup([], 5, 0, 6)
        assert err.value.code == -5
        assert t.generate_greedy(5, 0, 6) == want


def test_lookup_full_size_0_6b(q3, tmp_ckpt_dir):
    path = os.path.join(tmp_ckpt_dir, "qwen3-0.6b.bin")
    q3.checkpoint.ensure_synthetic_checkpoint(path, q3.checkpoint.SHAPES["qwen3-0.6b"], seed=1234)
    with engine(q3, path, 1024) as ref:
        G = ref.generate_greedy(9, 0, 64)
        more = ref.generate_greedy(G[-1], 64, 8)
    sim = simulate(G, G, 9, 2, 8)
    with engine(q3, path, 1024) as t:
        got, st = t.generate_lookup(G, 9, 0, 64, ngram=2, draft_len=8)
        assert got == G
        assert (st.verify_passes, st.single_steps, st.drafted, st.accepted) == (sim["verify_passes"], sim["single_steps"], sim["drafted"], sim["accepted"])
        assert t.generate_greedy(G[-1], 64, 8) == more


def test_lookup_equals_the_c_oracle_greedy_loop(q3, oracle, ckpt):
    name = "tiny-g64"
    seed, tok0, ctx = MODELS[name]
    path = ckpt(name)
    om = oracle.OracleModel(path)
    want, tok = [], tok0
    for pos in range(48):
        tok = oracle.sample_argmax(om.forward(tok, pos))
        want.append(tok)
    with engine(q3, path, 0) as t:
        for corpus, ngram, draft_len in (([], 2, 4), (want, 2, 31), (want, 1, 3)):
            t.reset_kv()
            got, st = t.generate_lookup(corpus, tok0, 0, 48, ngram=ngram, draft_len=draft_len)
            assert got == want, (ngram, draft_len)
            sim = simulate(want, corpus, tok0, ngram, draft_len)
            assert (st.verify_passes, st.single_steps, st.drafted, st.accepted) == (sim["verify_passes"], sim["single_steps"], sim["drafted"], sim["accepted"])


def test_batched_decode_and_batched_prefill_share_the_context_with_verify(q3, ckpt):
    """q3_batch_init + generate_greedy_batch and prefill(batched=True) still work on an engine that has verified, and verify still
    works after them (one BatchCtx, re-planned in both directions)."""
    name = "small-hd128"
    seed, tok0, ctx = MODELS[name]
    path = ckpt(name)
    shape = q3.checkpoint.SHAPES[name]
    G = reference(q3, path, ctx, tok0, 0, 64, extra=0)[0]
    prompt = q3.checkpoint.iter_prompt_tokens(shape, 5, 40)
    with engine(q3, path, ctx) as ref:
        want_first = ref.prefill(prompt, 0)
        want_rest = ref.generate_greedy(want_first, 40, 8)
    with engine(q3, path, ctx) as t:
        nxt, a = t.verify([tok0] + G[:15], 0)
        assert a == 15 and nxt == G[:16]
        t.batch_init(2)                                            # re-allocates the shared context with 2 stream caches
        out = t.generate_greedy_batch([tok0, tok0], [0, 0], 12)
        assert out[0].tolist() == G[:12] and out[1].tolist() == G[:12]
        nxt, a = t.verify([G[15]] + G[16:47], 16)                  # 32 columns on a context created for 2 streams
        assert a == 31 and nxt == G[16:48]
        t.batch_reset_kv()
        out = t.generate_greedy_batch([tok0, tok0], [0, 0], 5)
        assert out[0].tolist() == G[:5] and out[1].tolist() == G[:5]
        assert t.prefill(prompt, 0, batched=True) == want_first
        got, st = t.generate_lookup(prompt, want_first, 40, 8, ngram=1, draft_len=4)
        assert got == want_rest
        assert t.prefill(prompt, 0, batched=True) == want_first
        assert t.generate_greedy(want_first, 40, 8) == want_rest


@pytest.mark.parametrize("front_end", ["python", "cpp"])
def test_cli_lookup_prints_the_same_bytes(q3, tmp_path, front_end):
    """Both command lines: stdout with --lookup 8 is byte-identical to stdout without it (generate and chat mode, greedy, a chat that
    wraps its window included); --lookup with a temperature > 0 is refused."""
    import subprocess
    import sys
    from conftest import ROOT
    from qwen3_rs_amd import tokenizer as tk
    from test_tokenizer_cli import cpp_cli, make_tokenizer_json
    ck = q3.checkpoint
    d = str(tmp_path)
    n_vocab = make_tokenizer_json(d)
    shape = ck.ModelShape(256, 384, 2, 4, 2, n_vocab + (16 - n_vocab % 16) % 16, 96, 64, True, 64)
    path = os.path.join(d, "model.bin")
    ck.write_synthetic_checkpoint(path, shape, seed=12)
    tk.export_tokenizer(d, path, 1, 2)
    open(path + ".template", "w").write("<|im_start|>%s<|im_end|>")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "qwen3-rs_amd"))
    cli = [sys.executable, "-m", "qwen3_rs_amd.cli", "inference", path] if front_end == "python" else [cpp_cli(), "inference", path]
    for extra, stdin in ((["-m", "generate", "-i", "hello world", "-t", "0", "-c", "90"], b""),
                         (["-m", "generate", "-i", "hello world hello", "-t", "0"], b""),
                         (["-m", "chat", "-t", "0", "-c", "64"], b"hello world\n"),
                         (["-m", "chat", "-t", "0", "-c", "24"], b"hello world\nhello again world\n")):
        outs = []
        for lookup in ([], ["--lookup", "8"], ["--lookup", "31"]):
            r = subprocess.run(cli + extra + lookup, env=env, capture_output=True, timeout=600, input=stdin)
            assert r.returncode == 0, r.stderr.decode(errors="replace")
            outs.append(r.stdout)
        assert outs[0] == outs[1] == outs[2] and len(outs[0]) > 10, (extra, outs)
    r = subprocess.run(cli + ["-m", "generate", "-i", "hello", "-t", "0.7", "--lookup", "8"], env=env, capture_output=True, timeout=600)
    assert r.returncode == 1 and b"greedy only" in r.stderr


def test_generate_and_chat_turn_lookup_option(q3, ckpt):
    """qwen3_rs_amd.generate / chat_turn with lookup=(ngram, draft_len): the tokens of the default path"""
    name = "small-hd128"
    seed, tok0, ctx = MODELS[name]
    path = ckpt(name)
    prompt = q3.checkpoint.iter_prompt_tokens(q3.checkpoint.SHAPES[name], 5, 9)
    with engine(q3, path, ctx) as t:
        want, _ = q3.generate(t, prompt, max_new_tokens=70)
        stop = [want[33]]
        want_stop, _ = q3.generate(t, prompt, stop_tokens=stop)
        want_chat, want_pos, _ = q3.chat_turn(t, prompt, 3, 50)
        want_chat_stop, want_pos_stop, _ = q3.chat_turn(t, prompt, 3, 200, stop_tokens=[want_chat[20]])
    with engine(q3, path, ctx) as t:
        got, m = q3.generate(t, prompt, max_new_tokens=70, lookup=(2, 8))
        assert got == want and m.generated_count == 70
        assert q3.generate(t, prompt, stop_tokens=stop, lookup=(1, 31))[0] == want_stop
        got, pos, _ = q3.chat_turn(t, prompt, 3, 50, lookup=(2, 8))
        assert (got, pos) == (want_chat, want_pos)
        got, pos, _ = q3.chat_turn(t, prompt, 3, 200, stop_tokens=[want_chat[20]], lookup=(2, 4))
        assert (got, pos) == (want_chat_stop, want_pos_stop)
        with pytest.raises(ValueError):
            q3.generate(t, prompt, lookup=(2, 8), sample=lambda lg: 0)
