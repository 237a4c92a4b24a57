"""GPU tests of section 2d of include/qwen3_hip.h: q3_verify_draw (one weight pass over a block of drafts, every column drawn by the
device sampler with its own coin) and q3_generate_lookup_draw (sampled decode with prompt-lookup drafts).  Every equality is bit
for bit -- tokens, whole caches, rng state; the yardstick is q3_generate_sampled / q3_forward on a second engine, plus the C
oracle's sampled loop.  Expected statistics come from spec_sim.simulate, never from an acceptance rate.

The golden fixtures tiny.bin / tiny-untied.bin have quantization groups of 16 / 32, which the block kernels do not take
(q3_batch_init refuses them, and so does section 2c): on them the documented refusal is what is tested, and the oracle
agreement runs on the group-64 shapes the oracle decodes quickly (spec_draw_cases.ORACLE_MODELS)."""
import os

import numpy as np
import pytest

from conftest import assert_biteq, golden_path
from spec_draw_cases import N_REF, ORACLE_MODELS, SAMPLERS, SEEDS, g7, lookup_cases
from spec_sim import simulate
from test_speculative import MODELS, engine

pytestmark = pytest.mark.gpu

COMBOS = [(T, p, seed) for (T, p) in SAMPLERS for seed in SEEDS]


@pytest.fixture(scope="module")
def ckpt(q3, tmp_ckpt_dir):
    def get(name):
        path = os.path.join(tmp_ckpt_dir, f"draw-{name}-{MODELS[name][0]}.bin")
        return q3.checkpoint.ensure_synthetic_checkpoint(path, q3.checkpoint.SHAPES[name], seed=MODELS[name][0])
    return get


def sampled(t, T, p, seed, tok0, p0, n):
    """q3_generate_sampled(tok0, p0, n) from a zeroed cache and a freshly seeded sampler: tokens, rng after them"""
    t.reset_kv()
    t.set_sampler(T, p, seed)
    G = t.generate_greedy(tok0, p0, n)           # q3_generate_sampled: the same loop, the sampler set
    return G, t.sampler_rng_state()


def same_engine_state(t, ref, tok, pos, what, extra=6):
    """rng, whole caches, and the next `extra` sampled tokens (which read State, the transposed value cache and the rng)"""
    assert t.sampler_rng_state() == ref.sampler_rng_state(), what
    assert_biteq(t.read_state("key"), ref.read_state("key"), f"key cache, {what}")
    assert_biteq(t.read_state("value"), ref.read_state("value"), f"value cache, {what}")
    if extra:
        assert t.generate_greedy(tok, pos, extra) == ref.generate_greedy(tok, pos, extra), what
        assert t.sampler_rng_state() == ref.sampler_rng_state(), what


# ---------------------------------------------------------------------------------------------------------------------
# q3_verify_draw
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_verify_draw_all_drafts_right(q3, ckpt, name):
    """Walking the sampled tokens G in blocks of n: every draft is accepted, next_tokens are G, the rng is the reference's after as
    many draws, the whole caches are equal and sampled decode continues identically."""
    _, tok0, ctx = MODELS[name]
    path = ckpt(name)
    with engine(q3, path, ctx) as t, engine(q3, path, ctx) as ref:
        for T, p, seed in COMBOS:
            G, _ = sampled(ref, T, p, seed, tok0, 0, 64)
            for n in (2, 8, 32):
                t.reset_kv()
                t.set_sampler(T, p, seed)
                cur, k = tok0, 0
                while k + n <= 64:
                    nxt, a = t.verify_draw([cur] + G[k:k + n - 1], k)
                    assert a == n - 1, (T, p, seed, n, k, a)
                    assert nxt == G[k:k + n], (T, p, seed, n, k)
                    cur, k = G[k + n - 1], k + n
                assert sampled(ref, T, p, seed, tok0, 0, k)[0] == G[:k]
                same_engine_state(t, ref, G[k - 1], k, f"T {T} p {p} seed {seed} blocks of {n}")


@pytest.mark.parametrize("name", list(MODELS))
def test_verify_draw_first_wrong_draft(q3, ckpt, name):
    """Draft j replaced by (t + 1) % vocab: n_accepted == j - 1, the rng has advanced j coins only, the whole caches are those of an
    engine that drew exactly j tokens, and sampled decode continues identically."""
    _, tok0, ctx = MODELS[name]
    path = ckpt(name)
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    with engine(q3, path, ctx) as t, engine(q3, path, ctx) as ref:
        for T, p, seed in COMBOS[::2] + COMBOS[1:2]:
            G, _ = sampled(ref, T, p, seed, tok0, 0, 32)
            for n, js in ((2, (1,)), (8, (1, 4, 7)), (32, (1, 13, 31))):
                for j in js:
                    block = [tok0] + G[:n - 1]
                    block[j] = (block[j] + 1) % vocab
                    t.reset_kv()
                    t.set_sampler(T, p, seed)
                    nxt, a = t.verify_draw(block, 0)
                    assert a == j - 1, (T, p, seed, n, j, a)
                    assert nxt[:j] == G[:j], (T, p, seed, n, j)
                    assert sampled(ref, T, p, seed, tok0, 0, j)[0] == G[:j]
                    same_engine_state(t, ref, G[j - 1], j, f"T {T} p {p} seed {seed} n {n} first wrong draft {j}", extra=4)


@pytest.mark.parametrize("name", list(MODELS))
def test_verify_draw_restores_rows_that_held_data_and_returns_raw_logits(q3, ckpt, name):
    """On a cache that holds 48 sampled rows, a block at position 8 inside them drawn with the rng the loop had there (the seed IS the
    state): rejected rows come back as they were, so the whole cache stays that of the 48-token run; logits_out rows are those of
    q3_forward on the proposed prefix, rows behind the rejection included -- the sampler has not touched them."""
    _, tok0, ctx = MODELS[name]
    path = ckpt(name)
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    T, p, seed = COMBOS[3]
    with engine(q3, path, ctx) as t, engine(q3, path, ctx) as ref:
        _, rng8 = sampled(ref, T, p, seed, tok0, 0, 8)
        G, _ = sampled(t, T, p, seed, tok0, 0, 48)
        want_k, want_v = t.read_state("key"), t.read_state("value")
        for n, j in ((32, 1), (32, 20), (8, 5)):
            block = G[7:7 + n]                                     # G[7] is the input at position 8
            block[j] = (block[j] + 1) % vocab
            t.set_sampler(T, p, rng8)
            nxt, a, lg = t.verify_draw(block, 8, want_logits=True)
            assert a == j - 1 and nxt[:j] == G[8:8 + j], (n, j, a)
            assert_biteq(t.read_state("key"), want_k, f"key cache, n {n}, first wrong draft {j}")
            assert_biteq(t.read_state("value"), want_v, f"value cache, n {n}, first wrong draft {j}")
        assert sampled(ref, T, p, seed, tok0, 0, 8)[0] == G[:8]
        for i, tk in enumerate(block):                             # the last block: n 8, wrong at 5
            assert_biteq(lg[i], np.array(ref.forward(tk, 8 + i), copy=True), f"logits row {i}")


def test_verify_draw_block_ending_at_seq_len_limits_and_refusals(q3, ckpt):
    name = "tiny-g64"
    _, tok0, ctx = MODELS[name]
    path = ckpt(name)
    S = q3.checkpoint.SHAPES[name].max_seq_len
    T, p, seed = COMBOS[2]
    with engine(q3, path, 0) as t, engine(q3, path, 0) as ref:
        G, _ = sampled(ref, T, p, seed, tok0, 0, S)
        assert sampled(t, T, p, seed, tok0, 0, S - 5)[0] == G[:S - 5]
        for bad in (([G[S - 6]] + G[S - 5:S], S - 5), ([1] * 33, 0), ([], 0), ([1, 10 ** 6], 0)):
            with pytest.raises(IndexError):
                t.verify_draw(*bad)
        with pytest.raises(IndexError):
            t.generate_lookup_draw([], tok0, 0, 8, ngram=0, draft_len=4)
        with pytest.raises(IndexError):
            t.generate_lookup_draw([], tok0, 0, 8, ngram=2, draft_len=32)
        with pytest.raises(IndexError):
            t.generate_lookup_draw([], tok0, S - 4, 5, ngram=2, draft_len=4)
        assert t.sampler_rng_state() == sampled(ref, T, p, seed, tok0, 0, S - 5)[1]      # a refused call draws nothing
        nxt, a = t.verify_draw([G[S - 6]] + G[S - 5:S - 1], S - 5)                       # positions S - 5 .. S - 1
        assert a == 4 and nxt == G[S - 5:]
        assert sampled(ref, T, p, seed, tok0, 0, S)[0] == G
        same_engine_state(t, ref, 0, 0, "block ending at seq_len", extra=0)
        # the old names keep their greedy-only contract
        with pytest.raises(q3.Q3Error) as err:
            t.verify([tok0, G[0]], 0)
        assert err.value.code == -5 and "temperature" in err.value.msg
        with pytest.raises(q3.Q3Error) as err:
            t.generate_lookup([], tok0, 0, 8)
        assert err.value.code == -5 and "temperature" in err.value.msg
    with engine(q3, path, 0, flags=q3.FLAG_FAST) as t:
        for temperature in (0.0, 0.8):
            t.set_sampler(temperature, 0.9, 1)
            with pytest.raises(q3.Q3Error) as err:
                t.verify_draw([tok0, G[0]], 0)
            assert err.value.code == -5 and "Q3_FLAG_FAST" in err.value.msg
            with pytest.raises(q3.Q3Error) as err:
                t.generate_lookup_draw([], tok0, 0, 8)
            assert err.value.code == -5
        assert len(t.generate_greedy(tok0, 0, 4)) == 4


@pytest.mark.parametrize("fixture", ["tiny.bin", "tiny-untied.bin"])
def test_golden_fixtures_are_refused_and_stay_usable(q3, oracle, fixture):
    """Group sizes 16 / 32: the shapes q3_batch_init refuses.  Status -5, no coin drawn, and the engine's own sampled loop still
    equals the C oracle's."""
    path = golden_path(fixture)
    T, p, seed = 0.8, 0.9, 42
    om = oracle.OracleModel(path)
    s = oracle.Sampler(om.get_config().vocab_size, T, p, seed)
    want, tok = [], 5
    for pos in range(12):
        tok = s.sample(om.forward(tok, pos))
        want.append(tok)
    with engine(q3, path, 0) as t:
        t.set_sampler(T, p, seed)
        with pytest.raises(q3.Q3Error) as err:
            t.verify_draw([5, want[0]], 0)
        assert err.value.code == -5
        with pytest.raises(q3.Q3Error) as err:
            t.generate_lookup_draw(want, 5, 0, 12)
        assert err.value.code == -5
        assert t.sampler_rng_state() == seed
        assert t.generate_greedy(5, 0, 12) == want


# ---------------------------------------------------------------------------------------------------------------------
# q3_generate_lookup_draw
# ---------------------------------------------------------------------------------------------------------------------
def stats_of(st):
    return (st.verify_passes, st.single_steps, st.drafted, st.accepted)


def sim_stats(sim):
    return (sim["verify_passes"], sim["single_steps"], sim["drafted"], sim["accepted"])


@pytest.mark.parametrize("name", list(ORACLE_MODELS))
def test_generate_lookup_draw_equals_generate_sampled_and_the_c_oracle(q3, oracle, ckpt, tmp_ckpt_dir, name):
    """Every case of spec_draw_cases.lookup_cases() of this shape: tokens, whole caches, final rng and the continuation equal the plain
    sampled run, the tokens equal the C oracle's sampled loop, the four statistics equal the simulation's and a draft was accepted."""
    from test_speculative_draw_host import oracle_sampled
    _, tok0, ctx = MODELS[name]
    path = ckpt(name)
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    with engine(q3, path, ctx) as t, engine(q3, path, ctx) as ref:
        for case in lookup_cases():
            if case[0] != name:
                continue
            _, T, p, seed, ngram, draft_len, p0 = case
            G, _ = sampled(ref, T, p, seed, tok0, p0, N_REF)
            assert G == oracle_sampled(q3, oracle, tmp_ckpt_dir, name, T, p, seed, p0), case
            corpus = g7(G, vocab)
            sim = simulate(G, corpus, tok0, ngram, draft_len)
            assert sim["accepted"] > 0 and sim["drafted"] > sim["accepted"], case
            t.reset_kv()
            t.set_sampler(T, p, seed)
            got, st = t.generate_lookup_draw(corpus, tok0, p0, N_REF, ngram=ngram, draft_len=draft_len)
            assert got == G, case
            assert stats_of(st) == sim_stats(sim), (case, st, sim)
            assert st.accepted > 0
            same_engine_state(t, ref, G[-1], p0 + N_REF, f"{case}")


def test_generate_lookup_draw_eager_launches_and_sampler_off_and_on(q3, ckpt):
    """Q3_FLAG_NO_GRAPH (the pass launched kernel by kernel), then the sampler switched off -- temperature 0 gives exactly
    generate_lookup -- and on again with other parameters on the same engine (the plan changes with on / off only)."""
    name = "small-hd128"
    _, tok0, ctx = MODELS[name]
    path = ckpt(name)
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    for flags in (q3.FLAG_NO_GRAPH, 0):
        with engine(q3, path, ctx, flags=flags) as t, engine(q3, path, ctx) as ref:
            for T, p, seed in (COMBOS[1], (0.0, 0.9, 7), COMBOS[4], (0.0, 1.0, 7), COMBOS[2]):
                G, _ = sampled(ref, T, p, seed, tok0, 0, N_REF)
                corpus = g7(G, vocab)
                sim = simulate(G, corpus, tok0, 2, 8)
                t.reset_kv()
                t.set_sampler(T, p, seed)
                got, st = t.generate_lookup_draw(corpus, tok0, 0, N_REF, ngram=2, draft_len=8)
                assert got == G and stats_of(st) == sim_stats(sim) and st.accepted > 0, (flags, T, p, seed)
                same_engine_state(t, ref, G[-1], N_REF, f"flags {flags} T {T} p {p}")
                if T == 0.0:
                    t.reset_kv()
                    got2, st2 = t.generate_lookup(corpus, tok0, 0, N_REF, ngram=2, draft_len=8)
                    assert (got2, st2) == (got, st)
                    nxt, a = t.verify_draw([G[-1]] + G[:3], N_REF)
                    assert (nxt, a) == ref.verify([G[-1]] + G[:3], N_REF)
                    assert t.sampler_rng_state() == seed               # no coin drawn


def test_lookup_draw_full_size_vocabulary(q3, ckpt):
    """qwen3-0.6b-dims-l2 (151,936-entry vocabulary: radix-sorted candidate lists, the full-size draw scratch), corpus = the output"""
    name = "qwen3-0.6b-dims-l2"
    _, tok0, ctx = MODELS[name]
    path = ckpt(name)
    T, p, seed = COMBOS[2]
    with engine(q3, path, ctx) as t, engine(q3, path, ctx) as ref:
        G, _ = sampled(ref, T, p, seed, tok0, 0, 48)
        corpus = g7(G, q3.checkpoint.SHAPES[name].vocab_size)
        sim = simulate(G, corpus, tok0, 2, 8)
        t.set_sampler(T, p, seed)
        got, st = t.generate_lookup_draw(corpus, tok0, 0, 48, ngram=2, draft_len=8)
        assert got == G and stats_of(st) == sim_stats(sim) and st.accepted > 0 and st.drafted > st.accepted
        same_engine_state(t, ref, G[-1], 48, "0.6b dims")


# ---------------------------------------------------------------------------------------------------------------------
# front ends
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("front_end", ["python", "cpp"])
def test_cli_speculate_prints_the_same_bytes(q3, tmp_path, front_end):
    """Both command lines: stdout with --speculate 8 / 31 is byte-identical to stdout without it at -t 0.8 -p 0.9 -s 42 (generate mode,
    chat mode, chats of several turns and one that wraps its window); --speculate 8 -t 0 prints what --lookup 8 prints; --lookup
    keeps its greedy-only refusal."""
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
    samp = ["-t", "0.8", "-p", "0.9", "-s", "42"]

    def run(args, stdin=b""):
        r = subprocess.run(cli + args, env=env, capture_output=True, timeout=600, input=stdin)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        return r.stdout

    for extra, stdin in ((["-m", "generate", "-i", "hello world", "-c", "90"] + samp, b""),
                         (["-m", "generate", "-i", "hello world hello"] + samp, b""),
                         (["-m", "generate", "-i", "hello world hello", "-t", "0.3", "-p", "0.9", "-s", "7"], b""),
                         (["-m", "chat", "-c", "64"] + samp, b"hello world\n"),
                         (["-m", "chat"] + samp, b"hello world\nhello again world\nworld hello\n"),
                         (["-m", "chat", "-c", "24"] + samp, b"hello world\nhello again world\n")):
        outs = [run(extra + spec, stdin) for spec in ([], ["--speculate", "8"], ["--speculate", "31"])]
        assert outs[0] == outs[1] == outs[2] and len(outs[0]) > 10, (extra, outs)
    for extra, stdin in ((["-m", "generate", "-i", "hello world hello", "-t", "0"], b""), (["-m", "chat", "-t", "0", "-c", "24"], b"hello world\nhello again world\n")):
        assert run(extra + ["--speculate", "8"], stdin) == run(extra + ["--lookup", "8"], stdin) == run(extra, stdin)
    r = subprocess.run(cli + ["-m", "generate", "-i", "hello", "-t", "0.7", "--lookup", "8"], env=env, capture_output=True, timeout=600)
    assert r.returncode == 1 and b"greedy only" in r.stderr
    r = subprocess.run(cli + ["-m", "generate", "-i", "hello", "--speculate", "32"], env=env, capture_output=True, timeout=600)
    assert r.returncode == 1 and b"--speculate" in r.stderr


def test_generate_and_chat_turn_speculate_option(q3, oracle, ckpt):
    """qwen3_rs_amd.generate / chat_turn with speculate=(ngram, draft_len) and the device sampler: the tokens of the default path
    sampling on the host with the same Sampler (the C oracle's); a round cut at a stop token gives the coins behind it back."""
    name = "small-hd128"
    _, tok0, ctx = MODELS[name]
    path = ckpt(name)
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    prompt = q3.checkpoint.iter_prompt_tokens(q3.checkpoint.SHAPES[name], 5, 9)
    for T, p, seed in (COMBOS[2], COMBOS[5]):
        host = lambda: oracle.Sampler(vocab, T, p, seed).sample
        with engine(q3, path, ctx) as t:
            want, _ = q3.generate(t, prompt, max_new_tokens=70, sample=host())
            stop = [want[33]]
            want_stop, _ = q3.generate(t, prompt, stop_tokens=stop, sample=host())
            want_chat, want_pos, _ = q3.chat_turn(t, prompt, 3, 50, sample=host())
            want_chat_stop, want_pos_stop, _ = q3.chat_turn(t, prompt, 3, 200, stop_tokens=[want_chat[20]], sample=host())
        with engine(q3, path, ctx) as t, engine(q3, path, ctx) as ref:
            t.set_sampler(T, p, seed)
            got, m = q3.generate(t, prompt, max_new_tokens=70, speculate=(2, 8))
            assert got == want and m.generated_count == 70
            t.set_sampler(T, p, seed)
            assert q3.generate(t, prompt, stop_tokens=stop, speculate=(1, 31))[0] == want_stop
            ref.set_sampler(T, p, seed)
            assert ref.generate_greedy(prompt[-1], len(prompt) - 1, len(want_stop)) == want_stop
            assert t.sampler_rng_state() == ref.sampler_rng_state()            # nothing drawn behind the stop token
            t.set_sampler(T, p, seed)
            got, pos, _ = q3.chat_turn(t, prompt, 3, 50, speculate=(2, 8))
            assert (got, pos) == (want_chat, want_pos)
            t.set_sampler(T, p, seed)
            got, pos, _ = q3.chat_turn(t, prompt, 3, 200, stop_tokens=[want_chat[20]], speculate=(2, 4))
            assert (got, pos) == (want_chat_stop, want_pos_stop)
            with pytest.raises(ValueError):
                q3.generate(t, prompt, speculate=(2, 8), sample=lambda lg: 0)
            with pytest.raises(ValueError):
                q3.generate(t, prompt, speculate=(2, 8), lookup=(2, 8))
