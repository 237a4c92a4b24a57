"""CPU part of the designed-logits sampler tests (tests/logit_ckpt.py): the written checkpoints parse and give the designed logits on
both oracles, every witness condition of the design table holds on the oracle's logits of the written files, and the two
restatements of Sampler::sample (oracle.Sampler in C, np_oracle.NpSampler) agree on every draw the GPU tests compare against."""
import os

import numpy as np
import pytest

import logit_ckpt as lc
from conftest import assert_biteq

ALL_FILES = lc.BIG_FILES + lc.SMALL_FILES


@pytest.fixture(scope="module")
def files(oracle, np_oracle, tmp_path_factory):
    """file -> (path, {design: the C oracle's logits}, {(design, T, p): witness}), each computed once"""
    d = tmp_path_factory.mktemp("designed")
    made = {}

    def get(file):
        if file not in made:
            path = lc.write(str(d / f"{file}.bin"), file)
            om = oracle.OracleModel(path)
            logits = {name: om.forward(g, 0) for name, g, _, _ in lc.cases(file)}
            om.close()
            wit = {(name, T, p): lc.witness(np_oracle, logits[name], T, p) for name, _, T, p in lc.cases(file)}
            made[file] = (path, logits, wit)
        return made[file]
    return get


@pytest.mark.parametrize("file", ALL_FILES)
def test_written_file_parses_and_both_oracles_give_the_designed_logits(oracle, np_oracle, files, file):
    path, logits, _ = files(file)
    V, names = lc.FILES[file]
    shape = lc.ck.read_header(path)
    assert shape == lc.shape_of(V) and shape.file_size() == os.path.getsize(path)
    om = oracle.OracleModel(path)
    nm = np_oracle.NpQwen3(path)
    for g, name in enumerate(names):
        tok = g + 4 * (1 + g)                                        # another token of the residue class than the fixture's
        a = om.forward(tok, 0)
        assert_biteq(a, logits[name], f"{name}: tokens {g} and {tok}")
        assert_biteq(nm.forward(tok, 0), a, f"{name}: numpy oracle")
        assert_biteq(om.forward(tok, 3), a, f"{name}: position 3")
        fn, T0, _ = lc.DESIGNS[name]
        want = fn(V) * T0
        assert np.allclose(a, want, rtol=4e-7, atol=0.0), name        # design x c, c = 16 to three roundings
        # the map design -> logit keeps ties and order
        o = np.argsort(want, kind="stable")
        assert np.all(np.diff(a[o]) >= 0) and np.unique(a).size == np.unique(want.astype(np.float32)).size
    om.close()


def test_witnesses_of_the_full_vocabulary(files):
    """the table of the module docstring of logit_ckpt, condition by condition, on the oracle's logits of the written files"""
    wa, wb = files("big_a")[2], files("big_b")[2]
    margin = lc.HIST_ORDER_ERROR
    w = wa[("peaked", 0.7, 0.9)]
    assert w["candidates"] == 4 and w["nucleus"] == 2 and w["threshold_found"] and w["prefix_crossed"]
    w = wa[("uniform", 1.0, 0.9985)]
    assert w["distinct"] == 1 and w["candidates"] == w["n"] == lc.V_BIG
    assert w["threshold_found"] and w["hist_margin"] > margin and w["n0"] == w["n"]
    assert not w["prefix_crossed"] and not w["crossed_all"] and w["total_all"] < 0.9985
    w = wa[("second_try", 1.0, lc.TOPP_SECOND_TRY)]
    n_low = int(np.count_nonzero(np.arange(lc.V_BIG) % 37 == 7))
    assert w["threshold_found"] and w["hist_margin"] > margin and w["n0"] == lc.V_BIG - n_low
    assert not w["prefix_crossed"] and w["prefix_total"] < lc.TOPP_SECOND_TRY
    assert w["crossed_all"] and w["n0"] < w["nucleus"] < w["candidates"] == lc.V_BIG
    w = wa[("head_flat", 1.0, 0.9)]
    assert not w["threshold_found"] and w["hist_margin"] > margin and w["n0"] == w["candidates"] == lc.V_BIG > lc.RADIX_MIN
    assert w["below_window"] == lc.V_BIG - 1 and w["crossed_all"] and lc.RADIX_MIN < w["nucleus"] < lc.V_BIG
    for key in (("levels", 1.0, 0.9), ("levels", 0.3, 0.5)):
        w = wb[key]
        assert w["distinct"] == 5 and w["nucleus_in_ties"] and w["prefix_crossed"] and lc.RADIX_MIN < w["nucleus"] < w["n0"]
    for key in (("ramp", 1.0, 0.95), ("ramp", 0.5, 0.999), ("ramp", 1.0, 1.0)):
        w = wb[key]
        assert w["subnormal"] > 500 and w["zeros"] > 100000 and w["subnormal"] + w["zeros"] < w["n"]
    assert wb[("ramp", 1.0, 0.95)]["prefix_crossed"] and wb[("ramp", 0.5, 0.999)]["crossed_all"]
    for K in (2048, 2049):
        w = wb[(f"count_{K}", 1.0, 0.9)]
        assert w["candidates"] == w["n0"] == K and w["threshold_found"] and w["prefix_crossed"] and w["nucleus_in_ties"]
    assert 2048 <= lc.RADIX_MIN < 2049
    wc = files("big_c")[2]
    w = wc[("second_try_block", 1.0, lc.TOPP_SECOND_TRY)]
    assert w["threshold_found"] and w["hist_margin"] > margin and w["n0"] == lc.V_BIG - lc.N_LOW == lc.V_BIG - n_low
    assert not w["prefix_crossed"] and w["crossed_all"] and w["n0"] < w["nucleus"] < w["candidates"] == lc.V_BIG
    assert (lc.V_BIG - lc.N_LOW) // 64 * 64 + 64 > lc.V_BIG - lc.N_LOW          # all waves but one hold one bin
    w = wc[("head_far", 1.0, 0.9)]
    assert not w["threshold_found"] and w["hist_margin"] > margin and w["below_window"] == lc.V_BIG - 1 == w["n0"] - 1 and w["crossed_all"]
    assert wc[("twins", 1.0, 0.4)]["candidates"] == 2 and wc[("twins", 1.0, 0.4)]["nucleus"] == 1
    assert wc[("twins", 1.0, 0.9)]["nucleus"] == 2 and wc[("twins", 1.0, 0.9)]["nucleus_in_ties"] is False
    w = wc[("ramp_up", 1.0, 0.95)]
    assert w["subnormal"] > 500 and w["zeros"] > 100000 and w["prefix_crossed"]
    per = -(-lc.V_BIG // (256 * 256)) * 256                                     # k_sample_count's range per workgroup
    last = (lc.V_BIG - 1) // per                                                # every candidate in the last two ranges, the last a partial one
    assert lc.V_BIG % per != 0 and lc.V_BIG - w["candidates"] >= (last - 1) * per and w["candidates"] > lc.V_BIG - last * per
    # the peak and the ramps' top are far from logit 0 (see logit_ckpt.PEAK)
    assert files("big_a")[1]["peaked"].max() > 60 and files("big_b")[1]["ramp"].max() < -90 and files("big_c")[1]["ramp_up"].max() < -90


def test_witnesses_of_the_2000_entry_vocabulary(files):
    wa, wb = files("small_a")[2], files("small_b")[2]
    assert lc.V_SMALL <= lc.RADIX_MIN and lc.V_SMALL % 64 != 0 and lc.V_SMALL % 16 == 0 and lc.V_SMALL < 4096
    w = wa[("peaked", 0.7, 0.9)]
    assert w["candidates"] == 4 and w["nucleus"] == 2
    for key in (("levels", 1.0, 0.9), ("levels", 0.3, 0.5)):
        assert wa[key]["distinct"] == 5 and wa[key]["nucleus_in_ties"]
    for key in (("ramp_steep", 1.0, 0.95), ("ramp_steep", 0.5, 0.999), ("ramp_steep", 1.0, 1.0)):
        assert wa[key]["subnormal"] > 10 and wa[key]["zeros"] > 1000
    assert wa[("count_64", 1.0, 0.9)]["candidates"] == wa[("count_64", 1.0, 0.9)]["n0"] == 64           # one full wave
    assert wb[("count_65", 1.0, 0.9)]["candidates"] == wb[("count_65", 1.0, 0.9)]["n0"] == 65           # ... and one more


def test_coin_extreme_seeds():
    for s in lc.COIN_LOW_SEEDS:
        assert lc.first_coin(s)[0] < 2.0 ** -20
    for s in lc.COIN_HIGH_SEEDS:
        assert lc.first_coin(s)[0] > 1.0 - 2.0 ** -20


@pytest.mark.parametrize("file", ALL_FILES)
def test_both_samplers_draw_the_same(oracle, np_oracle, files, file):
    """every (design, setting, seed) of the GPU tests: oracle.Sampler and NpSampler draw the same token and leave the same rng state
    (per seed NpSampler's parts are called on the softmax the witness already holds; NpSampler.sample itself, with its 152k-entry
    expf loop, draws once per design and setting)"""
    _, logits, wit = files(file)
    V = lc.FILES[file][0]
    ends = set()
    for name, _, T, p in lc.cases(file):
        probs = wit[(name, T, p)]["p"]
        for seed in lc.seeds_for(name):
            c = oracle.Sampler(V, T, p, seed)
            want = c.sample(logits[name])
            n = np_oracle.NpSampler(V, T, p, seed)
            coin = n.random_f32()
            got = n.sample_mult(probs, coin) if (p <= 0.0 or p >= 1.0) else n.sample_topp(probs, coin)
            assert (got, n.state) == (want, c.rng_state.value), (name, T, p, seed)
            assert n.state == lc.first_coin(seed)[1]
            if seed in lc.COIN_LOW_SEEDS + lc.COIN_HIGH_SEEDS:
                ends.add((name, T, p, seed in lc.COIN_LOW_SEEDS, want))
        n, c = np_oracle.NpSampler(V, T, p, lc.SEEDS[-1]), oracle.Sampler(V, T, p, lc.SEEDS[-1])
        assert (n.sample(logits[name]), n.state) == (c.sample(logits[name]), c.rng_state.value), (name, T, p)
    # the low coins draw the head of the list, the high coins do not (unless the nucleus is that one token)
    head = {"peaked": 5, "ramp_up": V - 1, "twins": 9}
    for key in {e[:3] for e in ends}:
        low, high = {e[4] for e in ends if e[:3] == key and e[3]}, {e[4] for e in ends if e[:3] == key and not e[3]}
        if not (key[0] == "ramp_up" and key[2] >= 1.0):               # (the plain cdf walks in index order: there the ramp's foot)
            assert low == {head.get(key[0], 0)}, (key, low, high)
        assert not (low & high) or wit[key]["nucleus"] == 1, (key, low, high)


def test_second_try_depends_on_the_second_attempt(oracle, files):
    """with the second attempt skipped (last = n0 - 1 over the first attempt's candidates) second_try draws other tokens"""
    for file, name in (("big_a", "second_try"), ("big_c", "second_try_block")):
        _, logits, wit = files(file)
        w = wit[(name, 1.0, lc.TOPP_SECOND_TRY)]
        differ = 0
        for seed in lc.seeds_for(name):
            want = oracle.Sampler(lc.V_BIG, 1.0, lc.TOPP_SECOND_TRY, seed).sample(logits[name])
            differ += lc.draw_without_second_attempt(w, lc.first_coin(seed)[0]) != want
        assert differ >= len(lc.SEEDS) // 2, name
    _, logits, wit = files("big_a")
    # in `uniform` the first attempt's candidates already are all of them: the same draw either way
    w = wit[("uniform", 1.0, 0.9985)]
    for seed in lc.SEEDS[:2]:
        assert lc.draw_without_second_attempt(w, lc.first_coin(seed)[0]) == oracle.Sampler(lc.V_BIG, 1.0, 0.9985, seed).sample(logits["uniform"])
