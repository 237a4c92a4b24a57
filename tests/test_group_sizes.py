"""Every path at the quantization group sizes the engine accepts beyond 64: 128 and 256 single-stream and batched, 512 and 1024
single-stream (shapes and what each reaches: tests/group_cases.py).  Strict mode; the GPU part compares bit for bit -- single stream
against the C oracle, batched against single-stream runs of the same engine build, which the single-stream tests tie to the oracle.

The CPU part (not marked gpu) holds the witnesses: both oracles agree on every shape, and a quantizer whose group maximum stays
inside one 64-lane wave (group_cases.quantize_per_wave) disagrees with the oracle in every group that the G = 512 / 1024 tests feed
it, and in none at G <= 256 -- so those tests cannot pass by luck.

The operator-level rows for these group sizes live in tests/test_gpu_parity.py (quantize, matmul) and tests/test_tolerance_mode.py
(the GENERIC roles)."""
import numpy as np
import pytest

import cols_sim
import group_cases as gc
from conftest import assert_biteq

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """name -> path of the shape's synthetic checkpoint (1 - 35 MB), written once"""
    from qwen3_rs_amd import checkpoint as ck
    root = tmp_path_factory.mktemp("groups")
    made = {}

    def get(name):
        if name not in made:
            made[name] = ck.ensure_synthetic_checkpoint(str(root / f"{name}.bin"), gc.SHAPES[name], seed=gc.CKPT_SEED)
        return made[name]
    return get


# ---------------------------------------------------------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.SHAPES))
def test_both_oracles_agree(oracle, np_oracle, ckpt, name):
    shape = gc.SHAPES[name]
    a, b = oracle.OracleModel(ckpt(name)), np_oracle.NpQwen3(ckpt(name))
    for pos, tok in enumerate(gc.forward_tokens(shape)[:3]):
        assert_biteq(a.forward(tok, pos), b.forward(tok, pos), f"{name} pos {pos}")


@pytest.mark.parametrize("name", list(gc.SHAPES))
def test_exporter_keeps_the_group_size(oracle, name):
    """model_exporter.rs:47-57 on the row lengths of the shape's matrices: --group-size G survives"""
    from qwen3_rs_amd import checkpoint as ck
    s = gc.SHAPES[name]
    for n in (s.dim, s.hidden_dim, s.all_heads_dim):
        assert ck.find_optimal_group_size(n, s.group_size) == s.group_size
        assert oracle.find_optimal_group_size(n, s.group_size) == s.group_size


@pytest.mark.parametrize("G", [512, 1024])
def test_per_wave_maximum_differs_on_the_operator_vectors(oracle, G):
    bad, n = gc.groups_that_differ(gc.max_sweep_vector(G), G, oracle.quantize)
    assert bad == n == G // 4
    bad, n = gc.groups_that_differ(gc.random_vector(G), G, oracle.quantize)
    assert bad == n - 1                                   # all but the zero group


@pytest.mark.parametrize("name", gc.SINGLE_ONLY)
def test_per_wave_maximum_differs_on_every_token_of_the_model_tests(oracle, ckpt, name):
    """the layer-0 quantizer input of EVERY token of the vocabulary (so of each token the model tests feed, generated ones included)"""
    shape = gc.SHAPES[name]
    x = gc.layer0_inputs(ckpt(name), shape, oracle.rmsnorm, oracle.dequantize)
    assert x.shape == (shape.vocab_size, shape.dim)
    bad, n = gc.groups_that_differ(x.reshape(-1), shape.group_size, oracle.quantize)
    assert bad == n == shape.vocab_size * shape.dim // shape.group_size


@pytest.mark.parametrize("G", [16, 64, 128, 256])
def test_per_wave_maximum_is_the_reference_rule_up_to_256(oracle, G):
    for x in (gc.max_sweep_vector(G), gc.random_vector(G)):
        assert gc.groups_that_differ(x, G, oracle.quantize)[0] == 0


def test_reduced_column_tables_keep_their_edges():
    """prompts that do not fit one 32-column pass, more requests than slots, a greedy request among sampled ones"""
    assert max(gc.COLS_PROMPT_LEN) > 32 and min(gc.COLS_PROMPT_LEN) == 1 and len(gc.COLS_PROMPT_LEN) > gc.COLS_SLOTS
    assert 0.0 in gc.COLS_TEMPERATURE and any(t > 0 for t in gc.COLS_TEMPERATURE)
    assert all(gc.PREFIX_LEN + n + gc.COLS_NEW - 1 <= s.max_seq_len for n in gc.COLS_PROMPT_LEN for s in gc.SHAPES.values())
    assert gc.PREFILL_POS + gc.PREFILL_LEN + 6 <= 96 and gc.PREFILL_LEN > 2 * 32


# ---------------------------------------------------------------------------------------------------------------------
# GPU part, single stream: all eight shapes against the C oracle
# ---------------------------------------------------------------------------------------------------------------------
class OracleRef:
    """What the C oracle makes of one shape's schedules: computed once, never changed."""

    def __init__(self, oracle, path, shape):
        self.o, self.path, self.shape = oracle, path, shape
        self._memo = {}

    def _once(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def forwards(self):
        def run():
            om = self.o.OracleModel(self.path)
            return [om.forward(tok, pos).copy() for pos, tok in enumerate(gc.forward_tokens(self.shape))]
        return self._once("fw", run)

    def loop(self, sampler):
        """`chat` on prompt(shape): one sample per prompt position, all but the last discarded (generation.rs:116-123), then the decode
        loop: (first token, the tokens behind it, rng state, key rows, value rows)"""
        def run():
            om = self.o.OracleModel(self.path)
            T, p, seed = sampler or (0.0, 0.9, 0)
            smp = self.o.Sampler(self.shape.vocab_size, T, p, seed)
            prompt = gc.prompt(self.shape)
            n_new = gc.N_DRAWS if sampler else gc.N_GREEDY
            for pos, tok in enumerate(prompt):
                nxt = smp.sample(om.forward(tok, pos))
            toks = [nxt]
            for k in range(n_new):
                toks.append(smp.sample(om.forward(toks[-1], len(prompt) + k)))
            key, val = om.kv_cache()
            n = len(prompt) + n_new
            return toks[0], toks[1:], smp.rng_state.value, key[:, :n].copy(), val[:, :n].copy()
        return self._once(("loop", sampler), run)


@pytest.fixture(scope="module")
def refs(oracle, ckpt):
    made = {}

    def get(name):
        if name not in made:
            made[name] = OracleRef(oracle, ckpt(name), gc.SHAPES[name])
        return made[name]
    return get


def kv_rows(t, n, state=None):
    c = t.get_config()
    kvd = c.n_kv_heads * c.head_dim
    k, v = state or (t.read_state("key"), t.read_state("value"))
    return k.reshape(c.n_layers, -1, kvd)[:, :n], v.reshape(c.n_layers, -1, kvd)[:, :n]


@gpu
@pytest.mark.parametrize("name", list(gc.SHAPES))
def test_forward_vs_oracle(q3, refs, ckpt, name):
    want = refs(name).forwards()
    with q3.TransformerBuilder(ckpt(name)).build() as t:
        for pos, tok in enumerate(gc.forward_tokens(gc.SHAPES[name])):
            assert_biteq(t.forward(tok, pos), want[pos], f"{name} pos {pos}")


@gpu
@pytest.mark.parametrize("name", list(gc.SHAPES))
def test_prefill_and_greedy_loop_vs_oracle(q3, refs, ckpt, name):
    first, rest, _, wk, wv = refs(name).loop(None)
    prompt = gc.prompt(gc.SHAPES[name])
    with q3.TransformerBuilder(ckpt(name)).build() as t:
        assert t.prefill(prompt, 0) == first
        assert t.generate_greedy(first, len(prompt), gc.N_GREEDY) == rest
        k, v = kv_rows(t, len(prompt) + gc.N_GREEDY)
        assert_biteq(k, wk, "key rows")
        assert_biteq(v, wv, "value rows")


@gpu
@pytest.mark.parametrize("name", list(gc.SHAPES))
def test_sampled_draws_vs_oracle(q3, refs, ckpt, name):
    first, rest, rng, wk, _ = refs(name).loop(gc.SAMPLER)
    gfirst, grest = refs(name).loop(None)[:2]
    assert [first] + rest != [gfirst] + grest[:gc.N_DRAWS], "every draw is the argmax: the case shows nothing"
    prompt = gc.prompt(gc.SHAPES[name])
    with q3.TransformerBuilder(ckpt(name)).build() as t:
        t.set_sampler(*gc.SAMPLER)
        assert t.prefill(prompt, 0) == first
        tok, got = first, []
        for k in range(gc.N_DRAWS):                          # step by step: forward + Sampler::sample on the device
            tok = t.forward_sample(tok, len(prompt) + k)
            got.append(tok)
        assert got == rest
        assert t.sampler_rng_state() == rng
        assert_biteq(kv_rows(t, len(prompt) + gc.N_DRAWS)[0], wk, "key rows")


@gpu
def test_eager_launch_mode_g512(q3, refs, ckpt):
    want = refs("g512").forwards()
    first, rest = refs("g512").loop(None)[:2]
    prompt = gc.prompt(gc.SHAPES["g512"])
    with q3.TransformerBuilder(ckpt("g512")).with_graph(False).build() as t:
        for pos, tok in enumerate(gc.forward_tokens(gc.SHAPES["g512"])):
            assert_biteq(t.forward(tok, pos), want[pos], f"pos {pos}")
        t.reset_kv()
        assert t.prefill(prompt, 0) == first and t.generate_greedy(first, len(prompt), gc.N_GREEDY) == rest


@gpu
@pytest.mark.parametrize("name", gc.SINGLE_ONLY)
def test_batch_init_is_refused_and_the_engine_stays_usable(q3, refs, ckpt, name):
    want = refs(name).forwards()
    G = gc.SHAPES[name].group_size
    with q3.TransformerBuilder(ckpt(name)).build() as t:
        with pytest.raises(q3.Q3Error) as ei:
            t.batch_init(2)
        assert ei.value.code == -5
        assert f"batched decode needs group_size 64, 128 or 256 (one quantization group = 1, 2 or 4 64-byte MFMA steps), got {G}" in ei.value.msg
        for pos, tok in enumerate(gc.forward_tokens(gc.SHAPES[name])):
            assert_biteq(t.forward(tok, pos), want[pos], f"{name} pos {pos} behind the refusal")


# ---------------------------------------------------------------------------------------------------------------------
# GPU part, batched: the six shapes with G = 128 / 256 against single-stream runs
# ---------------------------------------------------------------------------------------------------------------------
class Single:
    """The single-stream references of one shape, each from a zeroed cache of one kept engine: computed once, never changed."""

    def __init__(self, q3, path, shape):
        self.q3, self.path, self.shape = q3, path, shape
        self._t, self._memo = None, {}

    def engine(self):
        return self.q3.TransformerBuilder(self.path).build()

    def batch_engine(self, slots):
        t = self.engine()
        t.batch_init(slots)
        return t

    def fresh(self):
        if self._t is None:
            self._t = self.engine()
        self._t.reset_kv()
        self._t.set_sampler(0.0, 0.9, 0)
        return self._t

    def close(self):
        if self._t is not None:
            self._t.close()
            self._t = None

    def _once(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def stream(self, i):
        """stream i of group_cases.streams: (logits of BATCH_STEPS greedy steps, tokens, key cache, value cache)"""
        def run():
            toks, pos = gc.streams(self.shape, 32)
            t, tok, ll, tt = self.fresh(), toks[i], [], []
            for k in range(gc.BATCH_STEPS):
                ll.append(np.array(t.forward(tok, pos[i] + k), copy=True))
                tok = self.q3.sample_argmax(ll[-1])
                tt.append(tok)
            return ll, tt, t.read_state("key"), t.read_state("value")
        return self._once(("stream", i), run)

    def stream_sampled(self, i, T, p, seed, steps):
        def run():
            toks, pos = gc.streams(self.shape, 32)
            t = self.fresh()
            t.set_sampler(T, p, seed)
            return t.generate_greedy(toks[i], pos[i], steps)
        return self._once(("sampled", i, T, p, seed, steps), run)

    def prefill(self):
        """PREFILL_LEN tokens from PREFILL_POS, then 6 greedy tokens: (first, rest, key cache, value cache)"""
        def run():
            t = self.fresh()
            prompt = gc.prompt(self.shape, gc.PREFILL_LEN, 3400)
            first = t.prefill(prompt, gc.PREFILL_POS)
            rest = t.generate_greedy(first, gc.PREFILL_POS + gc.PREFILL_LEN, 6)
            return first, rest, t.read_state("key"), t.read_state("value")
        return self._once("prefill", run)

    def greedy(self, tok0, n):
        """G = generate_greedy(tok0, 0, n), the caches after it, and the logits of every step through forward()"""
        def run():
            t = self.fresh()
            G = t.generate_greedy(tok0, 0, n)
            k, v = t.read_state("key"), t.read_state("value")
            t.reset_kv()
            lg = [np.array(t.forward(tok, pos), copy=True) for pos, tok in enumerate([tok0] + G[:-1])]
            return G, k, v, lg
        return self._once(("greedy", tok0, n), run)

    def sampled(self, tok0, n, T, p, seed):
        def run():
            t = self.fresh()
            t.set_sampler(T, p, seed)
            G = t.generate_greedy(tok0, 0, n)
            return G, t.sampler_rng_state(), t.read_state("key"), t.read_state("value")
        return self._once(("smp", tok0, n, T, p, seed), run)

    def request(self, prompt, n_new, T=0.0, p=0.9, seed=0):
        """one request of the column-pass loops on an engine of its own (the rule of cols_draw_cases): (row, key rows, value rows)"""
        def run():
            t = self.fresh()
            t.set_sampler(T, p, seed)
            y0 = t.prefill(prompt, 0)
            row = [y0] + (t.generate_greedy(y0, len(prompt), n_new - 1) if n_new > 1 else [])
            k, v = kv_rows(t, len(prompt) + n_new - 1)
            return row, k.copy(), v.copy()
        return self._once(("req", tuple(prompt), n_new, T, p, seed if T > 0 else 0), run)


@pytest.fixture(scope="module")
def singles(q3, ckpt):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Single(q3, ckpt(name), gc.SHAPES[name])
        return made[name]
    yield get
    for s in made.values():
        s.close()


@gpu
@pytest.mark.parametrize("n_streams", gc.STREAM_COUNTS)
@pytest.mark.parametrize("name", gc.BATCHED)
def test_batched_decode_equals_single_stream(q3, singles, name, n_streams):
    """forward_batch / generate_greedy_batch at ragged start positions: logits, tokens and whole caches of the checked streams"""
    s = singles(name)
    toks0, pos0 = gc.streams(s.shape, n_streams)
    check = gc.checked_streams(n_streams)
    ref = {i: s.stream(i) for i in check}
    with s.batch_engine(n_streams) as t:
        toks = list(toks0)
        for k in range(gc.BATCH_STEPS):
            lg, am = t.forward_batch(toks, [p + k for p in pos0])
            for i in check:
                assert_biteq(lg[i], ref[i][0][k], f"stream {i} step {k} logits")
                assert am[i] == ref[i][1][k]
            toks = am
        for i in check:
            assert_biteq(t.batch_read_state(i, "key"), ref[i][2], f"stream {i} key cache")
            assert_biteq(t.batch_read_state(i, "value"), ref[i][3], f"stream {i} value cache")
        t.batch_reset_kv()
        out = t.generate_greedy_batch(toks0, pos0, gc.BATCH_STEPS)
        for i in check:
            assert [int(v) for v in out[i]] == ref[i][1], f"stream {i}"


@gpu
@pytest.mark.parametrize("prefill_m", [None, "256"])
@pytest.mark.parametrize("name", gc.BATCHED)
def test_batched_prefill_equals_prefill(q3, singles, name, prefill_m, monkeypatch):
    """70 tokens from position 3 in blocks of at most 32 positions -- also when Q3_PREFILL_M asks for 256: other group sizes than 64
    have no dense kernels, prefill_block_cap clamps the block"""
    s = singles(name)
    first, rest, wk, wv = s.prefill()
    if prefill_m:
        monkeypatch.setenv("Q3_PREFILL_M", prefill_m)
    with s.engine() as t:
        assert t.prefill(gc.prompt(s.shape, gc.PREFILL_LEN, 3400), gc.PREFILL_POS, batched=True) == first
        assert t.generate_greedy(first, gc.PREFILL_POS + gc.PREFILL_LEN, 6) == rest
        assert_biteq(t.read_state("key"), wk, "key cache")
        assert_biteq(t.read_state("value"), wv, "value cache")


@gpu
@pytest.mark.parametrize("name", gc.BATCHED)
def test_verify_and_lookup_equal_the_greedy_loop(q3, singles, name):
    s = singles(name)
    tok0, n = 5, 40
    G, wk, wv, wlg = s.greedy(tok0, n)
    V = s.shape.vocab_size
    with s.engine() as t:
        for nb in (5, 32):                                   # every draft right: blocks of nb walk the greedy tokens
            t.reset_kv()
            cur, k = tok0, 0
            while k + nb <= n:
                nxt, a, lg = t.verify([cur] + G[k:k + nb - 1], k, want_logits=True)
                assert a == nb - 1 and nxt == G[k:k + nb], (nb, k, a)
                assert_biteq(lg, np.stack(wlg[k:k + nb]), f"logits of the block at {k}")
                cur, k = G[k + nb - 1], k + nb
            kk, vv = kv_rows(t, k)
            assert_biteq(kk, kv_rows(t, k, (wk, wv))[0], f"key rows, blocks of {nb}")
            assert_biteq(vv, kv_rows(t, k, (wk, wv))[1], f"value rows, blocks of {nb}")
        for nb, j in ((32, 13), (5, 1)):                     # draft j wrong: the engine is left as after j greedy steps
            t.reset_kv()
            block = [tok0] + G[:nb - 1]
            block[j] = (block[j] + 1) % V
            nxt, a = t.verify(block, 0)
            assert a == j - 1 and nxt[:j] == G[:j]
            assert t.generate_greedy(G[j - 1], j, n - j) == G[j:]
            assert_biteq(t.read_state("key"), wk, "key cache behind a rejected draft")
            assert_biteq(t.read_state("value"), wv, "value cache behind a rejected draft")
        t.reset_kv()
        got, st = t.generate_lookup(G, tok0, 0, n, ngram=2, draft_len=8)       # the corpus holds the continuation: drafts are accepted
        assert got == G and st.accepted > 0 and st.verify_passes > 0
        assert_biteq(t.read_state("key"), wk, "key cache after generate_lookup")
        assert_biteq(t.read_state("value"), wv, "value cache after generate_lookup")


@gpu
@pytest.mark.parametrize("name", gc.BATCHED)
def test_verify_draw_and_lookup_draw_equal_the_sampled_loop(q3, singles, name):
    s = singles(name)
    tok0, n = 5, 40
    T, p, seed = gc.SAMPLER
    G, rng, wk, wv = s.sampled(tok0, n, T, p, seed)
    assert G != s.greedy(tok0, n)[0]
    V = s.shape.vocab_size
    with s.engine() as t:
        for nb in (8, 32):
            t.reset_kv()
            t.set_sampler(T, p, seed)
            cur, k = tok0, 0
            while k + nb <= n:
                nxt, a = t.verify_draw([cur] + G[k:k + nb - 1], k)
                assert a == nb - 1 and nxt == G[k:k + nb], (nb, k, a)
                cur, k = G[k + nb - 1], k + nb
            assert t.generate_greedy(cur, k, n - k) == G[k:] and t.sampler_rng_state() == rng
            assert_biteq(t.read_state("key"), wk, f"key cache, blocks of {nb}")
        t.reset_kv()
        t.set_sampler(T, p, seed)
        block = [tok0] + G[:31]
        block[13] = (block[13] + 1) % V
        nxt, a = t.verify_draw(block, 0)
        assert a == 12 and nxt[:13] == G[:13]
        assert t.generate_greedy(G[12], 13, n - 13) == G[13:] and t.sampler_rng_state() == rng
        assert_biteq(t.read_state("value"), wv, "value cache behind a rejected draft")
        t.reset_kv()
        t.set_sampler(T, p, seed)
        got, st = t.generate_lookup_draw(G, tok0, 0, n, ngram=2, draft_len=8)
        assert got == G and st.accepted > 0 and t.sampler_rng_state() == rng
        assert_biteq(t.read_state("key"), wk, "key cache after generate_lookup_draw")
        assert_biteq(t.read_state("value"), wv, "value cache after generate_lookup_draw")


@gpu
@pytest.mark.parametrize("name", gc.BATCHED)
def test_per_stream_samplers(q3, singles, name):
    s = singles(name)
    n, steps = 17, 8
    toks0, pos0 = gc.streams(s.shape, n)
    seeds = [11 + 7 * i for i in range(n)]
    T, p = gc.SAMPLER[:2]
    check = gc.checked_streams(n)
    with s.batch_engine(n) as t:
        t.set_batch_sampler(T, p, seeds)
        out = t.generate_greedy_batch(toks0, pos0, steps)
        for i in check:
            assert [int(v) for v in out[i]] == s.stream_sampled(i, T, p, seeds[i], steps), f"stream {i}"
        assert any([int(v) for v in out[i][:gc.BATCH_STEPS]] != s.stream(i)[1] for i in check)


@gpu
@pytest.mark.parametrize("name", gc.BATCHED)
def test_column_passes_walk_and_mix_slots(q3, singles, name):
    """q3_batch_step_cols: slot 1 walked in runs of 1, 2, 5 and 32 columns; then one pass with a run from position 0, a decode column
    behind those 40 rows and a one-column slot -- logits of every column and the slots' rows against forward()"""
    s = singles(name)
    (Ga, ka, va, la), (Gb, kb, vb, lb) = s.greedy(5, 41), s.greedy(9, 8)
    ta, tb = [5] + Ga, [9] + Gb
    with s.batch_engine(3) as t:
        p, got = 0, []
        for c in (1, 2, 5, 32):
            lg, am = t.batch_step_cols([1] * c, ta[p:p + c], list(range(p, p + c)), want_logits=True)
            assert am == Ga[p:p + c]
            got.append(lg)
            p += c
        assert_biteq(np.concatenate(got), np.stack(la[:40]), "runs of slot 1")
        lg, am = t.batch_step_cols([0] * 7 + [1] + [2], tb[:7] + [ta[40]] + [tb[0]], list(range(7)) + [40, 0], want_logits=True)
        assert_biteq(lg[:7], np.stack(lb[:7]), "run of 7 from position 0")
        assert_biteq(lg[7], la[40], "decode column at position 40")
        assert_biteq(lg[8], lb[0], "one column")
        for slot, (wk, wv), n in ((0, (kb, vb), 7), (1, (ka, va), 41), (2, (kb, vb), 1)):
            k, v = kv_rows(t, 96, (t.batch_read_state(slot, "key"), t.batch_read_state(slot, "value")))
            assert_biteq(k[:, :n], kv_rows(t, n, (wk, wv))[0], f"slot {slot} key rows")
            assert_biteq(v[:, :n], kv_rows(t, n, (wk, wv))[1], f"slot {slot} value rows")
            assert not k[:, n:].any() and not v[:, n:].any(), f"slot {slot}: rows past {n} written"


def tup(stats):
    return (stats.passes, stats.live_columns, stats.prompt_columns, stats.decode_columns)


@gpu
@pytest.mark.parametrize("name", gc.BATCHED)
def test_generate_many_loops(q3, singles, name):
    """5 requests through 3 slots, 6 new tokens each: greedy, under per-request samplers, with stop tokens on the device and behind a
    shared prefix -- every row is the request's on an engine of its own, every schedule the simulator's"""
    s = singles(name)
    prompts, N, new = gc.cols_prompts(s.shape), len(gc.COLS_PROMPT_LEN), [gc.COLS_NEW] * len(gc.COLS_PROMPT_LEN)
    smp = (list(gc.COLS_TEMPERATURE), gc.COLS_TOPP, list(gc.COLS_SEEDS))
    want_g = [s.request(p, gc.COLS_NEW)[0] for p in prompts]
    want_s = [s.request(p, gc.COLS_NEW, T, gc.COLS_TOPP, seed)[0] for p, T, seed in zip(prompts, gc.COLS_TEMPERATURE, gc.COLS_SEEDS)]
    assert want_s != want_g
    wstats = cols_sim.schedule(gc.COLS_PROMPT_LEN, new, gc.COLS_SLOTS)[1]
    with s.batch_engine(gc.COLS_SLOTS) as t:
        rows, stats = t.generate_many_greedy(prompts, new)
        assert rows == want_g and tup(stats) == tuple(wstats)
        rows, stats = t.generate_many_sampled(prompts, new, *smp)
        assert rows == want_s and tup(stats) == tuple(wstats)
        # stop tokens: the token request 3 emits second ends it inside its row, and whoever else emits it
        for want, sampler in ((want_g, None), (want_s, smp)):
            stop = [want[3][1]]
            emit = [next((i + 1 for i, tk in enumerate(r) if tk in stop), len(r)) for r in want]
            assert emit[3] <= 2
            rows, stats = t.generate_many_stop(prompts, new, stop, sampler)
            assert rows == [r[:e] for r, e in zip(want, emit)]
            assert tup(stats) == tuple(cols_sim.schedule(gc.COLS_PROMPT_LEN, emit, gc.COLS_SLOTS)[1])
        # the cache rows of the last occupant of every slot of one greedy call
        table, _ = cols_sim.schedule(gc.COLS_PROMPT_LEN, new, gc.COLS_SLOTS)
        last = {}
        for _, slot, _, req in table:
            last[slot] = req
        t.generate_many_greedy(prompts, new)
        for slot, r in last.items():
            _, wk, wv = s.request(prompts[r], gc.COLS_NEW)
            n = len(prompts[r]) + gc.COLS_NEW - 1
            k, v = kv_rows(t, n, (t.batch_read_state(slot, "key"), t.batch_read_state(slot, "value")))
            assert_biteq(k, wk, f"slot {slot} key rows")
            assert_biteq(v, wv, f"slot {slot} value rows")
    # shared prefix: the rows of the full prompts, the passes of the suffixes
    prefix = gc.cols_prefix(s.shape)
    full_g = [s.request(prefix + p, gc.COLS_NEW)[0] for p in prompts]
    full_s = [s.request(prefix + p, gc.COLS_NEW, T, gc.COLS_TOPP, seed)[0] for p, T, seed in zip(prompts, gc.COLS_TEMPERATURE, gc.COLS_SEEDS)]
    with s.batch_engine(gc.COLS_SLOTS) as t:
        t.batch_prefix_set(prefix)
        assert t.batch_prefix_get() == prefix
        for want, sampler in ((full_g, None), (full_s, smp)):
            rows, stats = t.generate_many_prefix(prompts, new, (), sampler)
            assert rows == want and tup(stats) == tuple(wstats)


@gpu
@pytest.mark.parametrize("name", gc.BATCHED)
def test_dense_requests_pack_with_a_cap_of_32(q3, singles, name):
    """include/qwen3_hip.h section 2g: a shape the dense kernels do not take packs with a cap of 32 -- the same tokens for any
    dense_min, blocks counted as q3_dense_pack counts them at 32 columns, and no dense kernel ever launched (they refuse G != 64)"""
    s = singles(name)
    prompts, new = gc.cols_prompts(s.shape), [gc.COLS_NEW] * len(gc.COLS_PROMPT_LEN)
    want = [s.request(p, gc.COLS_NEW)[0] for p in prompts]
    dense = [r for r, n in enumerate(gc.COLS_PROMPT_LEN) if n - 1 >= 8]
    assert len(dense) == 2
    with s.batch_engine(gc.COLS_SLOTS) as t:
        rows, st, ds = t.generate_many_dense(prompts, new, None, 8)
        assert rows == want
        assert st == q3.cols_schedule([1 if r in dense else n for r, n in enumerate(gc.COLS_PROMPT_LEN)], new, gc.COLS_SLOTS)[1]
        assert ds.live_columns == sum(gc.COLS_PROMPT_LEN[r] - 1 for r in dense) and ds.blocks >= 2
        st = t.batch_prefill_slots([2, 0], [prompts[4][:-1], prompts[3][:-1]], [0, 0])
        assert st.live_columns == 39 + 32 and st.blocks == q3.dense_pack([39, 32], 32)[1].blocks
        for slot, r in ((2, 4), (0, 3)):
            _, wk, wv = s.request(prompts[r], gc.COLS_NEW)
            n = len(prompts[r]) - 1
            k, v = kv_rows(t, n, (t.batch_read_state(slot, "key"), t.batch_read_state(slot, "value")))
            assert_biteq(k, wk[:, :n], f"slot {slot} key rows")
            assert_biteq(v, wv[:, :n], f"slot {slot} value rows")
