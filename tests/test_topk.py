"""Top-k sampling on the device (include/qwen3_hip.h section 2n; csrc/q3_topk.h).  Tokens and rng states are compared with `==`:
q3_op_sample_top_k and the single-stream engine against the oracle's Sampler on the masked logits (tests/topk_ref.py), every
batched draw site against the single-stream loop of the same engine under the same k and seed, which the tests before pin to
the oracle.

The batched sites run on the synthetic tiny-g64 checkpoint and on a designed one: the batched kernels refuse the group size 16 of
tests/golden/tiny.bin, which serves the single-stream k = 1 test."""
import os
import subprocess
import sys

import numpy as np
import pytest

import logit_ckpt as lc
import topk_ref as tr
from conftest import ROOT, golden_path
from test_topk_host import DESIGNED, design_logits, settings_of

pytestmark = pytest.mark.gpu

KS = [1, 2, 20, 64]
COINS = 8
T0, P0 = 0.6, 0.95


def chain(q3, oracle, l, T, p, k, seed, what, n=COINS):
    """n successive coins: the device's draw and rng against the oracle's, the rng handed on"""
    rng = seed
    for i in range(n):
        want = tr.sample_top_k(oracle, l, T, p, k, rng)
        assert q3.ops.sample_top_k(l, T, p, k, rng) == want, (what, T, p, k, seed, i)
        rng = want[1]


# ---------------------------------------------------------------------------------------------------------------------
# q3_op_sample_top_k
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random"] + DESIGNED)
def test_op_small_vocabulary(q3, oracle, name):
    """V = 2,000: 64 slices of 32 entries (the last of 16), every slice shorter than k = 64"""
    if name == "random":
        l = (np.random.Generator(np.random.PCG64(30)).standard_normal(lc.V_SMALL) * 3).astype(np.float32)
        settings = [(T0, P0), (T0, 1.0), (1.0, 0.5)]
    else:
        l, settings = design_logits(name), settings_of(name)
    for k in KS:
        for T, p in settings:
            chain(q3, oracle, l, T, p, k, lc.SEEDS[k % 8], name)


def test_op_partial_last_slice(q3, oracle):
    """V = 2,001: slices of 32, the last one a single entry -- and it holds the maximum"""
    l = (np.random.Generator(np.random.PCG64(31)).standard_normal(2001) * 3).astype(np.float32)
    l[2000] = l.max() + 1
    for k in KS:
        for T, p in [(T0, P0), (T0, 1.0)]:
            chain(q3, oracle, l, T, p, k, 99 + k, "V 2001")
    levels = design_logits("levels", 2001)
    for k in (20, 64):
        chain(q3, oracle, levels, 1.0, 0.9, k, 7, "levels at V 2001")


@pytest.mark.parametrize("name", DESIGNED)
def test_op_full_vocabulary(q3, oracle, name):
    """V = 151,936: a slice is 2,374 entries, one tile of the part kernel with a partial last row of threads"""
    l = design_logits(name, lc.V_BIG)
    T, p = lc.DESIGNS[name][2][0]
    for k in KS:
        chain(q3, oracle, l, T, p, k, lc.SEEDS[(k + 3) % 8], name, n=COINS if k == 20 else 2)
    chain(q3, oracle, l, T, 1.0, 20, 31337, name, n=2)


def test_op_three_finite_logits(q3, oracle):
    """k = 20 with 3 finite logits: 17 survivors are -inf, their exponentials exact zeros"""
    l = np.full(lc.V_SMALL, -np.inf, dtype=np.float32)
    l[[3, 700, 1999]] = [1.0, 2.5, 2.0]
    for T, p in [(T0, P0), (1.0, 1.0), (1.0, 0.3)]:
        chain(q3, oracle, l, T, p, 20, 42, "three finite")
    drawn = {q3.ops.sample_top_k(l, 1.0, 1.0, 20, s)[0] for s in range(1, 60)}
    assert drawn == {3, 700, 1999}


def test_op_fall_through(q3, oracle):
    """the multinomial walk ends below the coin: the highest-index survivor, not V - 1"""
    l = tr.fall_through_logits()
    want = tr.sample_top_k(oracle, l, 1.0, 1.0, tr.FALL_THROUGH_K, tr.FALL_THROUGH_SEED)
    assert want[0] == int(tr.survivors(l, tr.FALL_THROUGH_K)[-1]) != l.size - 1
    assert q3.ops.sample_top_k(l, 1.0, 1.0, tr.FALL_THROUGH_K, tr.FALL_THROUGH_SEED) == want


def test_op_refusals(q3):
    lib = q3.load_library()
    import ctypes as C
    l = np.zeros(16, dtype=np.float32)
    fp = l.ctypes.data_as(C.POINTER(C.c_float))
    st, out = C.c_uint64(1), C.c_int32(-1)
    for k in (0, -1, 65, 17):
        assert lib.q3_op_sample_top_k(fp, 16, 1.0, 0.9, k, C.byref(st), C.byref(out), 0) == -3 and b"top_k" in lib.q3_last_error()
    assert lib.q3_op_sample_top_k(fp, 16, 0.0, 0.9, 4, C.byref(st), C.byref(out), 0) == -3
    assert lib.q3_op_sample_top_k(fp, 16, 1.0, 1.5, 4, C.byref(st), C.byref(out), 0) == -3
    assert lib.q3_op_sample_top_k(None, 16, 1.0, 0.9, 4, C.byref(st), C.byref(out), 0) == -3
    assert st.value == 1


# ---------------------------------------------------------------------------------------------------------------------
# the single-stream engine on designed checkpoints
# ---------------------------------------------------------------------------------------------------------------------
class Ref:
    """a designed checkpoint and the oracle's logits of its four designs"""

    def __init__(self, oracle, path, file):
        self.oracle, self.file, self.path = oracle, file, lc.write(path, file)
        self.V, self.names = lc.FILES[file]
        om = oracle.OracleModel(self.path)
        self.by_group = [om.forward(g, 0) for g in range(4)]
        om.close()

    def loop(self, tok0, T, p, k, seed, n, burn=0):
        return tr.loop(self.oracle, lambda tok: self.by_group[tok % 4], tok0, T, p, k, seed, n, burn)


@pytest.fixture(scope="module")
def refs(oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("topk")
    made = {}

    def get(file):
        if file not in made:
            made[file] = Ref(oracle, str(d / f"{file}.bin"), file)
        return made[file]
    return get


@pytest.mark.parametrize("file", ["small_a", "big_a"])
def test_single_stream_against_the_oracle(q3, refs, file):
    """set_sampler + set_top_k(20) + prefill + 8 sampled tokens; then set_top_k(5) and nothing else; then set_top_k(0)"""
    ref = refs(file)
    with q3.TransformerBuilder(ref.path).build() as t:
        for g in range(4):
            seed = lc.SEEDS[g]
            prompt = [(5 * g + 1) % ref.V, (9 * g + 2) % ref.V, g]
            t.reset_kv()
            t.set_sampler(T0, P0, seed)
            t.set_top_k(20)
            assert t.top_k == 20
            want, rng = ref.loop(g, T0, P0, 20, seed, 8, burn=2)
            first = t.prefill(prompt, 0)
            assert [first] + t.generate_greedy(first, 3, 7) == want, (file, ref.names[g])
            assert t.sampler_rng_state() == rng
            t.set_top_k(5)                                  # k alone: the plan and the rng stay
            want5, rng2 = ref.loop(want[-1], T0, P0, 5, rng, 8)
            assert t.generate_greedy(want[-1], 10, 8) == want5, (file, ref.names[g], "k = 5")
            assert t.sampler_rng_state() == rng2
            want = want5
            t.set_top_k(0)
            assert t.top_k == 0
            want0, rng3 = ref.loop(want[-1], T0, P0, 0, rng2, 8)
            assert t.generate_greedy(want[-1], 18, 8) == want0, (file, ref.names[g], "k = 0")
            assert t.sampler_rng_state() == rng3
        # forward_sample and multinomial draws (top-p 1.0) under k = 64
        t.set_top_k(64)
        for g in range(4):
            t.set_sampler(1.0, 1.0, 77 + g)
            want, rng = ref.loop(g, 1.0, 1.0, 64, 77 + g, 1)
            assert (t.forward_sample(g, 0), t.sampler_rng_state()) == (want[0], rng)


def test_one_survivor_is_greedy_decoding_with_coins(q3):
    path = golden_path("tiny.bin")
    with q3.TransformerBuilder(path).build() as t:
        greedy = t.generate_greedy(7, 0, 12)
        t.reset_kv()
        t.set_sampler(1.0, 0.9, 4242)
        t.set_top_k(1)
        assert t.generate_greedy(7, 0, 12) == greedy
        rng = 4242
        for _ in range(12):
            rng = lc.first_coin(rng)[1]
        assert t.sampler_rng_state() == rng
        # temperature 0 ignores k: no coin
        t.reset_kv()
        t.set_sampler(0.0, 0.9, 4242)
        t.set_top_k(20)
        assert t.generate_greedy(7, 0, 12) == greedy and t.sampler_rng_state() == 4242


def test_engine_refusals(q3, tmp_path):
    import ctypes as C
    shape = q3.checkpoint.ModelShape(64, 128, 1, 4, 2, 32, 16, 16, True, 16)
    path = str(tmp_path / "v32.bin")
    q3.checkpoint.write_synthetic_checkpoint(path, shape, seed=5)
    with q3.TransformerBuilder(path).build() as t:
        for k in (-1, 65, 33):
            assert t._lib.q3_sampler_top_k(t._h, k) == -3 and b"top_k" in t._lib.q3_last_error()
            with pytest.raises(ValueError):
                t.set_top_k(k)
        assert t.top_k == 0
        t.set_top_k(32)
        t.set_sampler(1.0, 1.0, 3)
        out = C.c_int(-1)
        assert t._lib.q3_sampler_get_top_k(t._h, C.byref(out)) == 0 and out.value == 32
        assert 0 <= t.forward_sample(1, 0) < 32
        assert t._lib.q3_sampler_top_k(t._h, 33) == -3 and t.top_k == 32       # a refused call changes nothing


# ---------------------------------------------------------------------------------------------------------------------
# every batched draw site against the single-stream loop
# ---------------------------------------------------------------------------------------------------------------------
K = 20


class Site:
    """a checkpoint the batched kernels take, one engine for the sites and one for the single-stream references"""

    def __init__(self, q3, path):
        self.q3, self.path = q3, path
        self.t = q3.TransformerBuilder(path).build()
        self.s = q3.TransformerBuilder(path).build()
        self.V = self.t.get_config().vocab_size
        self.t.set_top_k(K)
        self.s.set_top_k(K)
        self._memo = {}

    def close(self):
        self.t.close()
        self.s.close()

    def single(self, prompt, T, p, seed, n):
        """prefill + generate_greedy under (T, p, seed) and top_k = K on the reference engine: (n tokens, rng behind them)"""
        k = (tuple(prompt), T, p, seed, n)
        if k not in self._memo:
            s = self.s
            s.reset_kv()
            s.set_sampler(T, p, seed)
            first = s.prefill(prompt, 0)
            toks = [first] + (s.generate_greedy(first, len(prompt), n - 1) if n > 1 else [])
            self._memo[k] = (toks, s.sampler_rng_state() if T > 0 else seed)
        return self._memo[k]


@pytest.fixture(scope="module", params=["tiny-g64", "small_a"])
def site(request, q3, refs, tmp_path_factory):
    if request.param == "small_a":
        path = refs("small_a").path
    else:
        path = str(tmp_path_factory.mktemp("topk_site") / "tiny-g64.bin")
        q3.checkpoint.write_synthetic_checkpoint(path, q3.checkpoint.SHAPES["tiny-g64"], seed=2468)
    s = Site(q3, path)
    yield s
    s.close()


def test_the_reference_engine_differs_from_the_plain_sampler(site):
    """the yardstick of this section is not vacuous: with top_k = 0 the same seeds draw other tokens somewhere"""
    with_k = [site.single([t0], 1.0, 1.0, 11 + t0, 6)[0] for t0 in range(8)]
    site.s.set_top_k(0)
    try:
        plain = []
        for t0 in range(8):
            site.s.reset_kv()
            site.s.set_sampler(1.0, 1.0, 11 + t0)
            first = site.s.prefill([t0], 0)
            plain.append([first] + site.s.generate_greedy(first, 1, 5))
    finally:
        site.s.set_top_k(K)
    assert plain != with_k


def test_forward_batch(site):
    t, seeds, toks = site.t, [101, 202, 303], [3, 9, 14]
    t.batch_init(3)
    t.set_batch_sampler(T0, P0, seeds)
    _, drawn = t.forward_batch(toks, [0, 0, 0], want_logits=False)
    assert drawn == [site.single([toks[i]], T0, P0, seeds[i], 1)[0][0] for i in range(3)]
    t.batch_reset_kv()
    t.set_batch_sampler(T0, P0, seeds)
    out = t.generate_greedy_batch(toks, [0, 0, 0], 5)
    for i in range(3):
        assert [int(v) for v in out[i]] == site.single([toks[i]], T0, P0, seeds[i], 5)[0], f"stream {i}"


def test_verify_draw(site):
    """a block of 5 tokens whose third draft is wrong: two drafts accepted, three tokens drawn, the rng three coins on"""
    t, tok0, seed = site.t, 6, 555
    G, _ = site.single([tok0], T0, P0, seed, 5)
    block = [tok0] + G[:4]
    t.reset_kv()
    t.set_sampler(T0, P0, seed)
    nxt, a = t.verify_draw(block, 0)
    assert (nxt, a) == (G, 4)
    block[3] = (block[3] + 1) % site.V
    t.reset_kv()
    t.set_sampler(T0, P0, seed)
    nxt, a = t.verify_draw(block, 0)
    assert (nxt[:3], a) == (G[:3], 2)
    assert t.sampler_rng_state() == site.single([tok0], T0, P0, seed, 3)[1]


def test_generate_lookup_draw(site):
    """the expected continuation as corpus: its drafts are accepted, and the tokens and the rng are the loop's"""
    t, tok0, seed = site.t, 2, 808
    G, rng = site.single([tok0], T0, P0, seed, 10)
    t.reset_kv()
    t.set_sampler(T0, P0, seed)
    toks, stats = t.generate_lookup_draw([tok0] + G, tok0, 0, 10, ngram=1, draft_len=4)
    assert toks == G and t.sampler_rng_state() == rng
    assert stats.verify_passes > 0


def test_batch_step_cols_draw(site):
    """a prompt run of three columns (two discarded coins, one kept draw) beside a single column of another slot"""
    t, seeds = site.t, [31, 32, 33]
    run, other = [4, 8, 15], [16]
    t.batch_init(3)
    t.set_batch_sampler(T0, P0, seeds)
    drawn = t.batch_step_cols_draw([0, 0, 0, 2], run + other, [0, 1, 2, 0], keep=[0, 0, 1, 1])
    assert drawn == [-1, -1, site.single(run, T0, P0, seeds[0], 1)[0][0], site.single(other, T0, P0, seeds[2], 1)[0][0]]


def requests(V):
    prompts = [[(7 * r + 3 * i + 1) % V for i in range(n)] for r, n in enumerate([1, 3, 2, 5, 4])]
    temps = [T0, 1.0, 0.0, T0, 1.0]
    topps = [P0, 1.0, 0.9, 0.5, 0.9]
    seeds = [900 + r for r in range(5)]
    return prompts, temps, topps, seeds


def test_generate_many_sampled(site):
    """5 requests on 3 slots, request 2 at temperature 0"""
    t = site.t
    prompts, temps, topps, seeds = requests(site.V)
    want = [site.single(prompts[r], temps[r], topps[r], seeds[r], 4)[0] for r in range(5)]
    t.batch_init(3)
    rows, _ = t.generate_many_sampled(prompts, [4] * 5, temps, topps, seeds)
    assert rows == want


@pytest.mark.parametrize("how", ["stop_on_device", "shared_prefix", "dense_min"])
def test_generate_many_paths(q3, site, how):
    t = site.t
    prompts, temps, topps, seeds = requests(site.V)
    full = [site.single(prompts[r], temps[r], topps[r], seeds[r], 6)[0] for r in range(5)]
    kw, stop = {}, ()
    if how == "stop_on_device":
        stop = (full[0][2], full[3][4])
        kw = {"stop_on_device": True}
    elif how == "shared_prefix":
        prefix = [5, 6, 7]
        full = [site.single(prefix + prompts[r], temps[r], topps[r], seeds[r], 6)[0] for r in range(5)]
        kw = {"shared_prefix": prefix}
    else:
        kw = {"dense_min": 2}
    want = []
    for row in full:
        k = next((i for i, tok in enumerate(row) if tok in stop), None)
        want.append(row if k is None else row[:k + 1])
    t.batch_init(3)
    rows, _ = q3.generate_many(t, prompts, 6, stop_tokens=stop, sampler=(temps, topps, seeds), **kw)
    assert rows == want, how


def test_both_clis_print_the_same_bytes(q3, tmp_path, capsysbinary):
    """-t 0.6 -p 0.95 -s 42 -k 20 -m generate: the C++ front end (one process) and the Python one (in this process) print the same
    bytes; --speculate prints them too, and -k 0 prints others"""
    from qwen3_rs_amd import cli
    from qwen3_rs_amd import tokenizer as tk
    from test_tokenizer_cli import cpp_cli, make_tokenizer_json
    ck = q3.checkpoint
    d = str(tmp_path)
    n_vocab = make_tokenizer_json(d)
    shape = ck.ModelShape(256, 384, 2, 4, 2, n_vocab + (16 - n_vocab % 16) % 16, 96, 64, True, 64)
    path = os.path.join(d, "model.bin")
    ck.write_synthetic_checkpoint(path, shape, seed=12)
    tk.export_tokenizer(d, path, 1, 2)
    common = ["inference", path, "-t", "0.6", "-p", "0.95", "-s", "42", "-m", "generate", "-i", "hello world", "-c", "40"]
    outs = []
    for extra in (["-k", "20"], ["-k", "20", "--speculate", "4"], ["--top-k", "0"]):
        capsysbinary.readouterr()
        assert cli.main(common + extra) == 0
        outs.append(capsysbinary.readouterr().out)
    cc = subprocess.run([cpp_cli()] + common + ["-k", "20"], capture_output=True, timeout=120)
    assert cc.returncode == 0, cc.stderr[-400:]
    assert len(cc.stdout) > 0 and cc.stdout == outs[0]
    assert outs[1] == outs[0]
    assert outs[2] != outs[0]
