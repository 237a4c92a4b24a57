"""Every sampler path on designed logits (tests/logit_ckpt.py) at the product's 151,936-entry vocabulary and at 2,000 entries: the
pipelined draw of the single-stream engine, its two developer forms, q3_op_sample, the batched sampler, draft verification under the
sampler and the column passes under the sampler.  Every assertion is exact equality of tokens and of the rng state with the C
oracle's Sampler on the C oracle's logits; there are no tolerances.

The logits of such a checkpoint depend on the input token alone (token t: design t % 4 of its file, at every position), which
test_forward_gives_the_oracles_logits asserts first; that is what lets the oracle compute each design's logits once and walk
its sampled loops over those vectors.  tests/test_designed_logits.py (CPU) checks that the designs meet the conditions they
were made for and that the two CPU restatements of the sampler agree on every draw used here."""
import numpy as np
import pytest

import logit_ckpt as lc
from conftest import assert_biteq

pytestmark = pytest.mark.gpu

ALL_FILES = lc.BIG_FILES + lc.SMALL_FILES
CHAIN = (0.8, 0.95)                                 # the setting of the loops that hop between designs
# a second setting per file for the multi-stream paths: second_try's and second_try_block's own (the latter's second attempt
# decides the token in the single-workgroup kernel of the batched sampler and of a verify column), and nuclei that end inside
# levels' ties
OWN = {"big_a": (1.0, lc.TOPP_SECOND_TRY), "big_b": (1.0, 0.9), "big_c": (1.0, lc.TOPP_SECOND_TRY), "small_a": (1.0, 0.9), "small_b": (0.3, 0.5)}


class Ref:
    """One file's oracle side: the C oracle's logits per design and every expected (token, rng), computed once and never changed."""

    def __init__(self, oracle, path, file):
        self.oracle, self.file, self.path = oracle, file, lc.write(path, file)
        self.V, self.names = lc.FILES[file]
        om = oracle.OracleModel(self.path)
        self.by_group = [om.forward(g, 0) for g in range(4)]
        self.at5 = [om.forward(g + 8, 5) for g in range(4)]
        om.close()
        self._memo = {}

    def logits(self, token):
        return self.by_group[token % 4]

    def draw(self, name, T, p, seed):
        return self.loop(self.names.index(name), T, p, seed, 1)

    def loop(self, tok0, T, p, seed, n, burn=0):
        """the oracle's sampled loop from tok0: `burn` discarded coins (prompt positions), then n draws, each the next input.
        Returns (tokens, rng state behind them)"""
        k = (tok0 % 4, T, p, seed, n, burn)
        if k not in self._memo:
            s = self.oracle.Sampler(self.V, T, p, seed)
            for _ in range(burn):
                s.random_u32()
            tok, out = tok0, []
            for _ in range(n):
                tok = s.sample(self.logits(tok))
                out.append(tok)
            self._memo[k] = (out, s.rng_state.value)
        return self._memo[k]


@pytest.fixture(scope="module")
def refs(oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("designed")
    made = {}

    def get(file):
        if file not in made:
            made[file] = Ref(oracle, str(d / f"{file}.bin"), file)
        return made[file]
    return get


def engine(q3, ref):
    return q3.TransformerBuilder(ref.path).build()


def per_design_draws(t, ref, n_seeds):
    """every design of the file under each of its settings: one draw per seed from a freshly seeded sampler, positions 0 .. 7 in turn"""
    k = 0
    for name, g, T, p in lc.cases(ref.file):
        for seed in lc.seeds_for(name, n_seeds):
            t.set_sampler(T, p, seed)
            got = t.forward_sample(g + 4 * (k % 5), k % 8)
            want, rng = ref.draw(name, T, p, seed)
            assert (got, t.sampler_rng_state()) == (want[0], rng), (ref.file, name, T, p, seed)
            k += 1


@pytest.mark.parametrize("file", ALL_FILES)
def test_forward_gives_the_oracles_logits(q3, refs, file):
    """one token per design at positions 0 and 5: bit-equal to the oracle, and the same vector at both"""
    ref = refs(file)
    with engine(q3, ref) as t:
        for g, name in enumerate(ref.names):
            assert_biteq(np.array(t.forward(g, 0), copy=True), ref.by_group[g], f"{name} at position 0")
            assert_biteq(np.array(t.forward(g + 8, 5), copy=True), ref.at5[g], f"{name} at position 5")
            assert_biteq(ref.at5[g], ref.by_group[g], f"{name}: the oracle at positions 0 and 5")


@pytest.mark.parametrize("file", ALL_FILES)
def test_single_stream_pipelined_draw(q3, refs, file):
    """the product library (k_sample_exp, k_sample phase 1, k_sample_norm_hist, k_sample_count, k_sample_scatter, k_sample phase 2):
    8 seeds and the coin extremes per design and setting, then a device-resident loop of 24 tokens from each design under CHAIN"""
    ref = refs(file)
    with engine(q3, ref) as t:
        per_design_draws(t, ref, 8)
        hops = set()
        for g in range(4):
            seed = lc.SEEDS[g]
            want, rng = ref.loop(g, *CHAIN, seed, 24)
            t.reset_kv()
            t.set_sampler(*CHAIN, seed)
            assert t.generate_greedy(g, 0, 24) == want, (file, ref.names[g])
            assert t.sampler_rng_state() == rng
            hops |= {w % 4 for w in want}
        assert len(hops) > 1, "the loops never leave one design"


@pytest.mark.parametrize("form", [{"Q3_SAMPLER_PIPELINE": "0"}, {"Q3_SAMPLER_PRE_EXP": "0"}], ids=["pipeline0", "pre_exp0"])
@pytest.mark.parametrize("file", ALL_FILES)
def test_single_stream_developer_forms(q3, refs, dev_forms, file, form):
    """the single-workgroup kernel behind k_sample_exp, and the one that takes the maximum and the exponentials itself"""
    ref = refs(file)
    dev_forms(form)
    with engine(q3, ref) as t:
        per_design_draws(t, ref, 3)


@pytest.mark.parametrize("file", ALL_FILES)
def test_op_sample(q3, refs, file):
    """q3_op_sample on the oracle's logits of every design: the single-workgroup kernel without pre_exp"""
    ref = refs(file)
    for name, g, T, p in lc.cases(file):
        for seed in lc.seeds_for(name, 2):
            want, rng = ref.draw(name, T, p, seed)
            assert q3.ops.sample(ref.by_group[g], T, p, seed) == (want[0], rng), (file, name, T, p, seed)


@pytest.mark.parametrize("file", ALL_FILES)
def test_batched_sampler(q3, refs, file):
    """8 streams with a sampler each, two starting on every design of the file, 6 steps on the device: each stream is its own
    oracle loop"""
    ref = refs(file)
    first = [g + 4 * (g + k) for k in (1, 2) for g in range(4)]
    pos = [0, 3, 1, 0, 2, 0, 5, 1]
    with engine(q3, ref) as t:
        t.batch_init(8)
        for T, p in (CHAIN, OWN[file]):
            seeds = [s + 17 for s in lc.SEEDS]
            t.batch_reset_kv()
            t.set_batch_sampler(T, p, seeds)
            out = t.generate_greedy_batch(first, pos, 6)
            for i in range(8):
                assert [int(v) for v in out[i]] == ref.loop(first[i], T, p, seeds[i], 6)[0], (file, T, p, f"stream {i}")


@pytest.mark.parametrize("file", lc.BIG_FILES)
def test_verify_draw(q3, refs, file):
    """blocks of 8 columns, the smallest multi-column verify block: the oracle's sampled sequence as drafts is accepted whole; with
    draft 4 wrong, 3 drafts are accepted, the next tokens are the oracle's and the rng is 4 coins on"""
    ref = refs(file)
    with engine(q3, ref) as t:
        for (T, p), tok0 in [(CHAIN, 3), (CHAIN, 1), (OWN[file], 2), (OWN[file], 0)]:
            seed = lc.SEEDS[4] + tok0
            G, rng8 = ref.loop(tok0, T, p, seed, 8)
            t.reset_kv()
            t.set_sampler(T, p, seed)
            nxt, a = t.verify_draw([tok0] + G[:7], 0)
            assert (nxt, a) == (G, 7), (file, T, p, tok0)
            assert t.sampler_rng_state() == rng8
            block = [tok0] + G[:7]
            block[4] = (block[4] + 1) % ref.V
            t.reset_kv()
            t.set_sampler(T, p, seed)
            nxt, a = t.verify_draw(block, 0)
            assert (nxt[:4], a) == (G[:4], 3), (file, T, p, tok0)
            assert t.sampler_rng_state() == ref.loop(tok0, T, p, seed, 4)[1]


@pytest.mark.parametrize("file", lc.BIG_FILES)
def test_column_passes_under_the_sampler(q3, refs, file):
    """generate_many_sampled: 6 requests on 4 slots, prompts of 1 to 5 tokens, 4 new tokens each, every request with a setting of
    the table and a prompt that ends on that setting's design: the oracle's chat-pattern loop, one discarded coin per prompt
    position in front of the last"""
    ref = refs(file)
    table = lc.cases(file)
    lens = [1, 2, 3, 4, 5, 3]
    reqs = []
    for r, n in enumerate(lens):
        name, g, T, p = table[r % len(table)]
        prompt = [(7 * r + 3 * i + 11) % ref.V for i in range(n - 1)] + [g + 4 * r]
        reqs.append((prompt, T, p, lc.SEEDS[r] + 5))
    want = [ref.loop(P[-1], T, p, seed, 4, burn=len(P) - 1)[0] for P, T, p, seed in reqs]
    with engine(q3, ref) as t:
        t.batch_init(4)
        rows, _ = t.generate_many_sampled([P for P, _, _, _ in reqs], [4] * len(reqs), [T for _, T, _, _ in reqs],
                                          [p for _, _, p, _ in reqs], [s for _, _, _, s in reqs])
        assert rows == want
