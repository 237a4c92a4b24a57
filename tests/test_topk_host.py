"""Top-k sampling on the CPU (include/qwen3_hip.h section 2n): the two restatements of tests/topk_ref.py agree on every draw the GPU
tests compare the kernels with, the rule's corner cases are what the header says, the fall-through constant is a fall-through,
and the Python wrappers refuse what they must before anything reaches the library."""
import os

import numpy as np
import pytest

import logit_ckpt as lc
import topk_ref as tr
from conftest import ROOT

V = lc.V_SMALL
KS = [1, 2, 20, 63, 64]
DESIGNED = ["peaked", "uniform", "twins", "levels", "ramp", "ramp_up"]


def design_logits(name, vocab=V):
    fn, T0, _ = lc.DESIGNS[name]
    return (fn(vocab) * T0).astype(np.float32)


def settings_of(name):
    s = list(lc.DESIGNS[name][2])
    T = s[0][0]
    return s if (T, 1.0) in s else s + [(T, 1.0)]


def inputs():
    rng = np.random.Generator(np.random.PCG64(20))
    yield "random", (rng.standard_normal(V) * 3).astype(np.float32), [(0.6, 0.95), (1.0, 0.5), (0.6, 1.0), (1.3, 0.0)]
    for name in DESIGNED:
        yield name, design_logits(name), settings_of(name)


def test_the_two_restatements_agree(oracle, np_oracle):
    n = 0
    for name, l, settings in inputs():
        for k in KS:
            for T, p in settings:
                for seed in lc.seeds_for(name, 3):
                    a = tr.sample_top_k(oracle, l, T, p, k, seed)
                    b = tr.sample_top_k_np(np_oracle, l, T, p, k, seed)
                    assert a == b, (name, k, T, p, seed)
                    assert a[0] in tr.survivors(l, k)
                    n += 1
    assert n > 400


def test_every_entry_a_survivor_is_the_plain_draw(oracle, np_oracle):
    rng = np.random.Generator(np.random.PCG64(21))
    l = rng.standard_normal(64).astype(np.float32)
    for T, p in [(0.6, 0.95), (1.0, 1.0), (0.8, 0.3)]:
        for seed in lc.SEEDS:
            s = oracle.Sampler(64, T, p, seed)
            want = (s.sample(l), int(s.rng_state.value))
            assert tr.sample_top_k(oracle, l, T, p, 64, seed) == want
            assert tr.sample_top_k_np(np_oracle, l, T, p, 64, seed) == want


def test_one_survivor_is_the_argmax_and_one_coin(oracle, np_oracle):
    for name, l, settings in inputs():
        for T, p in settings:
            for seed in lc.SEEDS[:3]:
                want = (oracle.sample_argmax(l), lc.first_coin(seed)[1])
                assert tr.sample_top_k(oracle, l, T, p, 1, seed) == want, (name, T, p)
                assert tr.sample_top_k_np(np_oracle, l, T, p, 1, seed) == want, (name, T, p)


def test_temperature_zero_ignores_k_and_takes_no_coin(oracle, np_oracle):
    l = design_logits("levels")
    assert tr.sample_top_k(oracle, l, 0.0, 0.9, 20, 42) == (oracle.sample_argmax(l), 42)
    assert tr.sample_top_k_np(np_oracle, l, 0.0, 0.9, 20, 42) == (oracle.sample_argmax(l), 42)


def test_ties_go_to_the_higher_index(oracle):
    l = design_logits("uniform")
    assert list(tr.survivors(l, 5)) == [V - 5, V - 4, V - 3, V - 2, V - 1]
    drawn = {tr.sample_top_k(oracle, l, 1.0, 1.0, 5, seed)[0] for seed in range(1, 200)}
    assert drawn == {V - 5, V - 4, V - 3, V - 2, V - 1}
    # -0.0 sorts below +0.0, and an index decides only between equal keys
    assert list(tr.survivors(np.array([0.0, -0.0, 0.0, -1.0], dtype=np.float32), 2)) == [0, 2]


def test_the_fall_through_constant_is_one(oracle, np_oracle):
    l = tr.fall_through_logits()
    s = tr.survivors(l, tr.FALL_THROUGH_K)
    assert s.size == 37 and np.all(l[s] == 2.0) and s[-1] != l.size - 1
    p = np_oracle.softmax(tr.masked(l, tr.FALL_THROUGH_K)[0])
    cdf = np.float32(0.0)
    for v in p[s]:
        cdf = np.float32(cdf + v)
    coin, state = lc.first_coin(tr.FALL_THROUGH_SEED)
    assert float(cdf) < 1.0 and coin >= cdf, (float(cdf), float(coin))
    # the masked reference returns the masked index V - 1; the rule gives the highest-index survivor
    smp = oracle.Sampler(l.size, 1.0, 1.0, tr.FALL_THROUGH_SEED)
    assert smp.sample(tr.masked(l, tr.FALL_THROUGH_K)[0]) == l.size - 1
    assert tr.sample_top_k(oracle, l, 1.0, 1.0, tr.FALL_THROUGH_K, tr.FALL_THROUGH_SEED) == (int(s[-1]), state)
    assert tr.sample_top_k_np(np_oracle, l, 1.0, 1.0, tr.FALL_THROUGH_K, tr.FALL_THROUGH_SEED) == (int(s[-1]), state)


def test_header_and_symbols(q3):
    with open(os.path.join(ROOT, "include", "qwen3_hip.h")) as f:
        header = f.read()
    lib = q3.load_library()
    for sym in ("q3_sampler_top_k", "q3_sampler_get_top_k", "q3_op_sample_top_k"):
        assert sym in q3.EXPORTED_SYMBOLS and hasattr(lib, sym) and f"int {sym}(" in header
    assert "#define Q3_TOP_K_MAX 64" in header and q3.TOP_K_MAX == tr.TOP_K_MAX == q3.SCORE_TOP_MAX == 64
    assert header.index("int q3_sampler_top_k(") > header.index("#define Q3_TOP_K_MAX") > header.index("2n. (behind 2m") > header.index("int q3_score_top_many(")
    assert int(header.split("#define Q3_ABI_VERSION ")[1].split()[0]) == 1 and lib.q3_abi_version() == 1
    assert lib.q3_sampler_top_k(None, 5) == -3 and lib.q3_sampler_get_top_k(None, None) == -3


def test_wrappers_refuse_before_they_call(q3):
    l = np.zeros(16, dtype=np.float32)
    for k in (0, -1, 65, 17):
        with pytest.raises(ValueError):
            q3.ops.sample_top_k(l, 1.0, 0.9, k, 1)
        with pytest.raises(ValueError):
            q3.op_sample_top_k(l, 1.0, 0.9, k, 1)
    with pytest.raises(TypeError):
        q3.ops.sample_top_k(l, 1.0, 0.9, 2.0, 1)

    class NoEngine(q3.Transformer):                    # set_top_k's checks run in front of the library call
        def __init__(self, vocab):
            self._config = type("C", (), {"vocab_size": vocab})()
            self._h = None
            self._lib = None

        def __del__(self):
            pass
    t = NoEngine(32)
    for k in (-1, 65, 33):
        with pytest.raises(ValueError):
            t.set_top_k(k)
    with pytest.raises(TypeError):
        t.set_top_k(True)


def test_a_host_sample_callback_with_top_k_is_refused(q3):
    class T:
        top_k = 20

        def get_config(self):
            return type("C", (), {"seq_len": 8})()
    with pytest.raises(ValueError, match="set_top_k"):
        q3.generate(T(), [1, 2], 4, sample=lambda logits: 0)
    with pytest.raises(ValueError, match="set_top_k"):
        q3.chat_turn(T(), [1, 2], 0, 4, sample=lambda logits: 0)


def test_both_clis_take_the_flag_and_refuse_alike(q3, capsys):
    import subprocess
    from qwen3_rs_amd import cli
    assert cli.build_parser().parse_args(["inference", "x.bin", "-k", "20"]).top_k == 20
    assert cli.build_parser().parse_args(["inference", "x.bin", "--top-k", "5"]).top_k == 5
    assert cli.build_parser().parse_args(["inference", "x.bin"]).top_k == 0
    assert cli.main(["inference", "x.bin", "-k", "65"]) == 1
    py_err = capsys.readouterr().err
    exe = os.path.join(ROOT, "qwen3-rs_amd", "q3_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qwen3-rs_amd"), "cli"])
    r = subprocess.run([exe, "inference", "x.bin", "-k", "65"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr == py_err and "--top-k takes 0 (off) or a count of 1..64" in py_err
