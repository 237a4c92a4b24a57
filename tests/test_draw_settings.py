"""The order in which the sampler settings arrive on one engine (include/qwen3_hip.h sections 2b, 2d, 2n): set_top_k before or
after set_sampler, set_batch_sampler twice, the column site made by the first sampled pass and made again behind a second
batch_init, top_k switched under column plans that already exist.  Plans and graphs carry the addresses of the draw sites'
buffers (csrc/q3_draw_host.inc), so a buffer that is replaced or a plan that is not rebuilt shows as a wrong draw here.

One long-lived engine goes through the steps; after each, its draws -- tokens and sampler_rng_state, compared with `==` -- are
those of a fresh engine that received only the settings then in force, in the plain order (set_sampler, set_top_k, batch_init,
set_batch_sampler).  What the draws compute is pinned elsewhere (test_topk.py, test_sampler_designed.py, test_batch_cols_draw.py).

The seeds below are ones for which the fresh engines show that the comparison is not vacuous: the batch seeds SEEDS_A and
SEEDS_B draw different tokens, and the requests of REQ_SEEDS draw different rows under top_k = 5 and top_k = 0.  Both are
asserted on the fresh engines' results only."""
import pytest

pytestmark = pytest.mark.gpu

T, P = 1.0, 0.95
SEED_1, SEED_2, SEED_V = 1234, 98765, 555
SEEDS_A, SEEDS_B = [101, 202, 303, 404], [505, 606, 707, 808]
REQ_SEEDS = [900, 901, 902, 903]
STREAMS = 4
PROMPTS = [[3], [9, 14, 2], [7, 1], [20, 21, 22, 23]]
REQ_T, REQ_P = [T, 0.6, T, T], [P, 1.0, 1.0, 0.9]
BLOCK = [6, 17, 40, 3, 250]


@pytest.fixture(scope="module")
def path(q3, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("draw_settings") / "tiny-g64.bin")
    q3.checkpoint.write_synthetic_checkpoint(p, q3.checkpoint.SHAPES["tiny-g64"], seed=2468)
    return p


def single(t):
    """forward_sample over four positions, then generate_greedy under the sampler: (tokens, tokens, rng)"""
    t.reset_kv()
    tok, stepped = 5, []
    for pos in range(4):
        tok = t.forward_sample(tok, pos)
        stepped.append(tok)
    return stepped, t.generate_greedy(tok, 4, 8), t.sampler_rng_state()


def batch(t):
    """three forward_batch steps of all streams, every stream fed its own draw"""
    t.batch_reset_kv()
    toks, drawn = [3, 9, 14, 27], []
    for pos in range(3):
        _, toks = t.forward_batch(toks, [pos] * STREAMS, want_logits=False)
        drawn.append(toks)
    return drawn


def verify(t):
    t.reset_kv()
    nxt, accepted = t.verify_draw(BLOCK, 0)
    return nxt, accepted, t.sampler_rng_state()


def many(t):
    rows, _ = t.generate_many_sampled(PROMPTS, [6] * len(PROMPTS), REQ_T, REQ_P, REQ_SEEDS)
    return rows


def fresh(q3, path, draws, sampler, top_k=0, batch_init=False, batch_sampler=None):
    """what `draws` (a list of the functions above) give on a new engine under these settings alone"""
    with q3.TransformerBuilder(path).build() as f:
        f.set_sampler(*sampler)
        f.set_top_k(top_k)
        if batch_init:
            f.batch_init(STREAMS)
        if batch_sampler:
            f.set_batch_sampler(*batch_sampler)
        return [d(f) for d in draws]


def test_settings_in_any_order(q3, path):
    with q3.TransformerBuilder(path).build() as t:
        def in_force(temperature=T):
            """the single-stream sampler as it stands now: the rng is wherever the draws so far have left it"""
            return (temperature, P, t.sampler_rng_state())

        # 1. top_k before any set_sampler: the top-k lists exist first, the engine's site and both forms of its plan come second
        t.set_top_k(20)
        t.set_sampler(T, P, SEED_1)
        assert [single(t)] == fresh(q3, path, [single], (T, P, SEED_1), top_k=20)

        # 2. top_k off: the plain form of the plan, built when the lists already stood; then temperature 0 and back
        t.set_top_k(0)
        now = in_force()
        plain = fresh(q3, path, [single], now)
        assert [single(t)] == plain
        assert plain != fresh(q3, path, [single], now, top_k=20)
        t.set_sampler(0.0, P, SEED_2)
        assert [single(t)] == fresh(q3, path, [single], (0.0, P, SEED_2))
        assert t.sampler_rng_state() == SEED_2
        t.set_sampler(T, P, SEED_2)
        assert [single(t)] == fresh(q3, path, [single], (T, P, SEED_2))

        # 3. the batch sampler twice: the second call keeps the decode site's buffers and drops the step plan
        t.batch_init(STREAMS)
        t.set_batch_sampler(T, P, SEEDS_A)
        want_a = fresh(q3, path, [batch], in_force(), batch_init=True, batch_sampler=(T, P, SEEDS_A))
        assert [batch(t)] == want_a
        t.set_batch_sampler(T, P, SEEDS_B)
        want_b = fresh(q3, path, [batch], in_force(), batch_init=True, batch_sampler=(T, P, SEEDS_B))
        assert [batch(t)] == want_b
        assert want_a != want_b

        # 4. the column site appears with the first sampled pass; a second batch_init rebuilds the context and the site with it
        t.set_sampler(T, P, SEED_V)
        assert [verify(t)] == fresh(q3, path, [verify], (T, P, SEED_V), batch_init=True, batch_sampler=(T, P, SEEDS_B))
        t.batch_init(STREAMS)
        now = in_force()
        want = fresh(q3, path, [verify, many], now, batch_init=True)
        got = [verify(t), many(t)]
        assert got == want
        rows_0 = got[1]

        # 5. top_k under the sampled column plans of step 4: the top-k plans are new, the plain ones are kept
        t.set_top_k(5)
        want_5 = fresh(q3, path, [many], in_force(), top_k=5, batch_init=True)
        assert [many(t)] == want_5
        assert want_5 != [want[1]]
        t.set_top_k(0)
        assert many(t) == rows_0
