"""Top-k log-probabilities of many prompts (include/qwen3_hip.h section 2m, q3_score_top_many).  The yardstick is forward() per
position on a single-stream engine of the same context, its logits sorted on the host by tests/score_top_ref.py: the tops are
compared by bits and indices, the ranks are equal, and the records are bit for bit score_many's on the same engine.  There is no
tolerance anywhere."""
import numpy as np
import pytest

import edge_ckpt
import group_cases
import logit_ckpt as lc
import score_ref
import score_top_ref as tr
from conftest import assert_biteq
from score_ref import assert_records
from score_top_ref import assert_tops
from test_dense_slots import check_rows
from test_embed import NAME
from test_score import ScoreModel, want_stats

pytestmark = pytest.mark.gpu

KMAX = tr.TOP_MAX


class TopModel(ScoreModel):
    """test_score.ScoreModel whose references carry, for every position but the last, the min(64, V) largest keys of the row as
    {logit, index} and the rank of the next token as well"""

    def refs(self, prompts):
        todo = [tuple(p) for p in prompts if tuple(p) not in self._refs]
        if todo:
            with self.engine() as t:
                cfg = t.get_config()
                kvd = cfg.n_kv_heads * cfg.head_dim
                kk = min(KMAX, cfg.vocab_size)
                for p in todo:
                    n = len(p)
                    t.reset_kv()
                    recs, top, rank = np.zeros(n - 1, dtype=score_ref.DTYPE), np.zeros((n - 1, kk), dtype=tr.DTYPE), np.zeros(n - 1, dtype=np.int32)
                    for i in range(n):
                        l = t.forward(p[i], i)
                        if i + 1 < n:
                            recs[i], top[i], rank[i] = score_ref.record(l, p[i + 1]), tr.top(l, kk), tr.rank(l, p[i + 1])
                    self._refs[p] = dict(prompt=list(p), records=recs, top=top, rank=rank, x=t.read_state("x").copy(),
                                         key=t.read_state("key").reshape(cfg.n_layers, self.ctx, kvd)[:, :n].copy(),
                                         value=t.read_state("value").reshape(cfg.n_layers, self.ctx, kvd)[:, :n].copy())
        return [self._refs[tuple(p)] for p in prompts]


@pytest.fixture(scope="module")
def models(q3, tmp_path_factory):
    made = {}

    def get(name=NAME, edit=None, seed=2468):
        if (name, edit) not in made:
            path = str(tmp_path_factory.mktemp("score_top") / f"{name}-{edit}.bin")
            if edit:
                edge_ckpt.write(path, name, edit)
                made[(name, edit)] = TopModel(q3, name, path)
            elif name in group_cases.SHAPES:
                q3.checkpoint.write_synthetic_checkpoint(path, group_cases.SHAPES[name], seed=group_cases.CKPT_SEED)
                made[(name, edit)] = TopModel(q3, name, path, shape=group_cases.SHAPES[name])
            else:
                q3.checkpoint.write_synthetic_checkpoint(path, q3.checkpoint.SHAPES[name], seed=seed)
                made[(name, edit)] = TopModel(q3, name, path)
        return made[(name, edit)]
    return get


def invariants(recs, tops, ranks, targets, k, what):
    """what holds of every answer, whatever the reference says: the first is the record's argmax and maximum, the keys fall
    strictly, and the rank says where the target stands -- or that it is absent"""
    n = recs.size
    assert tops.shape == (n, k) and tops.dtype == tr.DTYPE and ranks.shape == (n,) and ranks.dtype == np.int32, what
    if n == 0:
        return
    targets = np.asarray(targets, dtype=np.int32)
    assert np.array_equal(tops["index"][:, 0], recs["argmax"]), what
    assert (tops["logit"][:, 0] == recs["max"]).all(), what
    keys = tr.keys_of(tops)
    assert (keys[:, 1:] < keys[:, :-1]).all(), f"{what}: keys not strictly descending"
    tbits = np.ascontiguousarray(recs["target"]).view(np.uint32)
    for i in range(n):
        if ranks[i] < k:
            at = tops[i, ranks[i]]
            assert (at["logit"].view(np.uint32), at["index"]) == (tbits[i], targets[i]), f"{what}: record {i}: rank {ranks[i]} is not the target's place"
        else:
            assert targets[i] not in tops["index"][i], f"{what}: record {i}: rank {ranks[i]} >= {k}, yet the target is listed"


def check(got, refs, k, what, score_from=None):
    recs, tops, ranks = got[:3]
    assert len(recs) == len(tops) == len(ranks) == len(refs)
    for i, r in enumerate(refs):
        f = 1 if score_from is None else score_from[i]
        w = f"{what}: k {k}: request {i} of {len(r['prompt'])} tokens from {f}"
        assert_records(recs[i], r["records"][f - 1:], w)
        assert_tops(tops[i], r["top"][f - 1:, :k], w)
        assert np.array_equal(ranks[i], r["rank"][f - 1:]), (w, ranks[i], r["rank"][f - 1:])
        invariants(recs[i], tops[i], ranks[i], r["prompt"][f:], k, w)


def same_records(t, prompts, got, score_from=None, **kw):
    """the records of a score_top_many call are bit for bit score_many's on the same engine, and so are the stats"""
    plain, st = t.score_many(prompts, score_from, **kw)
    assert st == got[3]
    for a, b in zip(plain, got[0]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def top_raw(q3, m, refs, streams, k, what, cap=2048, score_from=None):
    """through `streams` slots on a fresh engine"""
    prompts = [r["prompt"] for r in refs]
    with m.engine() as t:
        t.batch_init(streams)
        got = t.score_top_many(prompts, k, score_from)
        check(got, refs, k, what, score_from)
        assert got[3] == want_stats(q3, [len(p) for p in prompts], score_from, streams, cap)
        same_records(t, prompts, got, score_from)
    return got


@pytest.mark.parametrize("k", [1, 2, 20, 63, 64])
def test_one_wide_block_many_slots(q3, models, k):
    m = models()
    lens = (1, 2, 9, 41, 97, 33, 8, 70)
    refs = m.by_len(100, lens)
    prompts = [r["prompt"] for r in refs]
    with m.engine() as t:
        t.batch_init(8)
        got = t.score_top_many(prompts, k)
        check(got, refs, k, "one block")
        st = got[3]
        assert st == want_stats(q3, lens, None, 8) and (st.blocks, st.scored, st.chunks) == (1, 253, 8)
        assert got[1][0].shape == (0, k) and got[2][0].size == 0
        for i, r in enumerate(refs):
            check_rows(t, i, r, lens[i], f"slot {i}")           # the prompt's rows, and nothing behind them
        same_records(t, prompts, got)


def test_chunk_edges_inside_one_block(q3, models):
    """31, 32, 33 and 65 scored columns in one block; with 33 and 65 the second request's columns straddle two chunks"""
    m = models()
    k = 20
    with m.engine() as t:
        t.batch_init(4)
        for lens, scored, chunks in (((20, 13), 31, 1), ((20, 14), 32, 1), ((20, 15), 33, 2), ((20, 15, 33), 65, 3)):
            refs = m.by_len(1100, lens)
            prompts = [r["prompt"] for r in refs]
            got = t.score_top_many(prompts, k)
            check(got, refs, k, f"{scored} scored columns")
            assert (got[3].blocks, got[3].scored, got[3].chunks) == (1, scored, chunks)
        alone = t.score_top_many(prompts[1:2], k)
        assert alone[3].chunks == 1
        for a, b in zip(alone[:3], got[:3]):
            assert a[0].tobytes() == b[1].tobytes()             # the request that straddled two chunks, scored alone


# The slices of a row: part p of `parts` = 64 is [p per, (p + 1) per), per = ceil(V / parts), walked in tiles of 2560 entries.
@pytest.mark.parametrize("name,lens,cap,per", [("tiny-g64", (50, 9), 32, 8), ("small-hd128", (40, 3), 2048, 32), (NAME, (35, 8), 2048, 64)])
def test_part_edges_small_vocabularies(q3, oracle, models, name, lens, cap, per):
    """V = 512 and 2,048: every slice (8 and 32 entries) is shorter than k = 64 and contributes what it has; V = 4,096: a slice is
    exactly k entries.  None of the three is a multiple of parts * 256 = 16,384: no slice fills a workgroup's 256 threads.
    tiny-g64 (walked through the column plans) and small-hd128 are held to the C oracle's logits as well."""
    m = models(name, seed=92) if name != NAME else models()
    V = m.shape.vocab_size
    assert -(-V // 64) == per and per <= KMAX and V % (64 * 256) and (per < KMAX or name == NAME)
    refs = m.by_len(420, lens)
    for k in (64, 7):
        got = top_raw(q3, m, refs, 2, k, name, cap=cap)
    if name == NAME:
        return
    om = oracle.OracleModel(m.path, m.ctx)
    for i, r in enumerate(refs):
        om.reset()
        p = r["prompt"]
        rows = [np.array(om.forward(p[pos], pos), copy=True) for pos in range(len(p) - 1)]
        assert_tops(got[1][i], np.stack([tr.top(l, 7) for l in rows]), f"{name}: request {i} against the oracle")
        assert got[2][i].tolist() == [tr.rank(l, t) for l, t in zip(rows, p[1:])]


@pytest.mark.parametrize("name,dim", [("qwen3-4b-dims-l2", 2560), ("qwen3-8b-dims-l2", 4096)])
def test_one_segment_vocabulary(q3, models, name, dim):
    """V = 16,384: a slice is exactly 256 entries, one per thread; dim 2560 and 4096, the latter with its own lm_head"""
    m = models(name)
    assert m.shape.dim == dim and m.shape.vocab_size == 16384 == 64 * 256
    top_raw(q3, m, m.by_len(500, (35, 8, 64)), 3, 64, name)


@pytest.mark.parametrize("parts", [1, 7, 33])
def test_the_split_of_a_row_changes_nothing(q3, models, dev_forms, parts):
    """Q3_SCORE_TOP_PARTS of the developer build: one slice of 4,096 entries is two tiles (2,560 and 1,536), the second merged with
    the best of the first; 7 slices of 586 end in one of 580; 33 slices of 125 end in one of 96 and every slice is a partial wave
    or two.  The references are the product library's."""
    m = models()
    assert m.shape.vocab_size == 4096
    refs = m.by_len(1100, (20, 15, 33))
    dev_forms({"Q3_SCORE_TOP_PARTS": str(parts)})
    for k in (64, 3):
        top_raw(q3, m, refs, 4, k, f"{parts} parts")


def test_a_vocabulary_that_is_no_multiple_of_the_parts(q3, tmp_path_factory):
    """V = 2,000 (logit_ckpt's small files): slices of 32, part 62 holds 16 entries and part 63 none"""
    V, names = lc.FILES["small_a"]
    assert V == 2000 and -(-V // 64) * 62 + 16 == V
    path = lc.write(str(tmp_path_factory.mktemp("score_top_small") / "small_a.bin"), "small_a")
    rng = np.random.default_rng(77)
    prompts = [[int(v) for v in rng.integers(0, V, n)] for n in (9, 5)]
    prompts[0][3], prompts[0][5], prompts[1][2] = V - 1, 0, 1984
    with q3.TransformerBuilder(path).build() as t:
        rows = []
        for p in prompts:
            t.reset_kv()
            rows.append([np.array(t.forward(p[i], i), copy=True) for i in range(len(p) - 1)])
        t.batch_init(2)
        for k in (64, 5):
            got = t.score_top_many(prompts, k)
            for r, p in enumerate(prompts):
                assert_tops(got[1][r], np.stack([tr.top(l, k) for l in rows[r]]), f"small_a: request {r}, k {k}")
                assert got[2][r].tolist() == [tr.rank(l, x) for l, x in zip(rows[r], p[1:])]
                invariants(got[0][r], got[1][r], got[2][r], p[1:], k, f"small_a: request {r}")
            same_records(t, prompts, got)


DESIGNED = {"big_a": ("peaked", "uniform"), "big_b": ("levels", "ramp"), "big_c": ("twins", "ramp_up")}


@pytest.mark.parametrize("file", sorted(DESIGNED))
def test_the_full_vocabulary_on_designed_logits(q3, tmp_path_factory, file):
    """151,936 logits that depend on the input token alone (token t: design t % 4 of the file), k = 64: 64 slices of 2,374, nine
    full rounds of 256 threads and one of 70.  A flat row (every key decided by the index), a tie at both ends, five levels and a
    ramp whose neighbours differ by a few ulps across every slice edge.  One target is the row's argmax, one index 0, one V - 1."""
    V, names = lc.FILES[file]
    assert V == 64 * 2374 and 2374 == 9 * 256 + 70
    path = lc.write(str(tmp_path_factory.mktemp("score_top_designed") / f"{file}.bin"), file)
    groups = [names.index(d) for d in DESIGNED[file]]
    rng = np.random.default_rng(31)
    prompts = [[int(4 * rng.integers(0, V // 4) + groups[i % len(groups)]) for i in range(n)] for n in (5, 8, 6)]
    best = {"peaked": 5, "uniform": V - 1, "levels": V - 1, "ramp": 0, "twins": V - 9, "ramp_up": V - 1}
    prompts[0][2] = best[names[prompts[0][1] % 4]]              # a target that is its row's argmax
    prompts[1][3], prompts[2][2] = 0, V - 1
    prompts[1][6] = V - 9
    k = KMAX
    memo = {}
    with q3.TransformerBuilder(path).build() as t:
        want_top, want_rank, rows = [], [], []
        for p in prompts:
            t.reset_kv()
            ls = [np.array(t.forward(p[i], i), copy=True) for i in range(len(p) - 1)]
            for l in ls:
                memo.setdefault(l.tobytes(), tr.keys(l))
            ks = [memo[l.tobytes()] for l in ls]
            want_top.append(np.stack([tr.pairs(l, np.sort(kv)[::-1][:k]) for l, kv in zip(ls, ks)]))
            want_rank.append([int(np.count_nonzero(kv > kv[x])) for kv, x in zip(ks, p[1:])])
            rows.append(ls)
        t.batch_init(3)
        got = t.score_top_many(prompts, k)
        assert got[3].scored == sum(len(p) - 1 for p in prompts) and got[3] == want_stats(q3, [len(p) for p in prompts], None, 3, 32)
        same_records(t, prompts, got)
    assert got[2][0][1] == 0 and want_rank[0][1] == 0
    seen = set()
    for r, p in enumerate(prompts):
        assert_tops(got[1][r], want_top[r], f"{file}: request {r}")
        assert got[2][r].tolist() == want_rank[r], (file, r)
        invariants(got[0][r], got[1][r], got[2][r], p[1:], k, f"{file}: request {r}")
        for i in range(len(p) - 1):
            design, idx, x = names[p[i] % 4], got[1][r]["index"][i].tolist(), p[i + 1]
            seen.add(design)
            if design == "uniform":
                assert idx == list(range(V - 1, V - 1 - k, -1)) and got[2][r][i] == V - 1 - x
            elif design == "twins":
                assert idx[:2] == [V - 9, 9] and idx[2:10] == [V - 1, V - 2, V - 3, V - 4, V - 5, V - 6, V - 7, V - 8] and idx[10] == V - 10
            elif design == "levels":
                assert idx == list(range(V - 1, V - 1 - 5 * k, -5)) and (V - 1) % 5 == 0
            elif design == "ramp":
                assert idx == list(range(k)) and got[2][r][i] == x
            elif design == "ramp_up":
                assert idx == list(range(V - 1, V - 1 - k, -1)) and got[2][r][i] == V - 1 - x
            elif design == "peaked":
                assert idx[:4] == [5, 77, 4000, V - 1] and all(v % 997 == 0 for v in idx[4:])
    assert set(DESIGNED[file]) <= seen


def test_score_from(q3, models):
    """1, n, n - 1 and values in between, a one-token request between two others, 11 requests through 4 slots in 3 waves: the
    answers are the slices of the all-positions call's"""
    m = models()
    k = 5
    lens = (120, 5, 33, 64, 7, 90, 1, 12, 40, 3, 17)
    sf = [1, 5, 32, 30, 4, 90, 1, 11, 17, 1, 9]
    refs = m.by_len(200, lens)
    prompts = [r["prompt"] for r in refs]
    with m.engine() as t:
        t.batch_init(4)
        full = t.score_top_many(prompts, k)
        assert full[3].waves == 3 and full[3] == want_stats(q3, lens, None, 4)
        check(full, refs, k, "all positions")
        part = t.score_top_many(prompts, k, sf)
        assert part[3] == want_stats(q3, lens, sf, 4) and part[3].scored == sum(n - f for n, f in zip(lens, sf))
        check(part, refs, k, "score_from", sf)
        for i, f in enumerate(sf):
            for a, b in zip(part[:3], full[:3]):
                assert a[i].tobytes() == b[i][f - 1:].tobytes(), i
        assert part[1][1].shape == (0, k) and part[2][5].size == 0 and part[1][2].shape == (1, k)
        same_records(t, prompts, part, sf)


def test_a_run_split_over_blocks(q3, models, monkeypatch):
    monkeypatch.setenv("Q3_PREFILL_M", "128")
    m = models()
    top_raw(q3, m, m.by_len(300, (300, 40, 129)), 3, 20, "blocks of 128", cap=128)


def test_a_narrow_block(q3, models):
    m = models()
    refs = m.by_len(400, (3, 5))
    top_raw(q3, m, refs, 2, 64, "one block of 16 columns")
    top_raw(q3, m, refs[:1], 1, 2, "the scored columns stand in place")


@pytest.mark.parametrize("edit", ["all", "flat_logits"])
def test_edge_valued_checkpoints(q3, models, edit):
    """all: a tied classifier: rows 2i and 2i + 1 are equal, so the tops come in pairs and the odd one stands first;
    flat_logits: every logit the sum of zero terms: as the designed `uniform`"""
    m = models(NAME, edit)
    V = m.shape.vocab_size
    refs = m.by_len(530, (41, 9))
    k = 64
    got = top_raw(q3, m, refs, 2, k, edit)
    for r, (recs, tops, ranks) in enumerate(zip(*got[:3])):
        if edit == "all":
            first, second = tops[:, 0::2], tops[:, 1::2]
            assert (first["index"] % 2 == 1).all() and (second["index"] == first["index"] - 1).all()
            assert_biteq(np.ascontiguousarray(first["logit"]), np.ascontiguousarray(second["logit"]), "the pairs tie")
        else:
            assert (tops["index"] == np.arange(V - 1, V - 1 - k, -1)).all() and not tops["logit"].any()
            assert ranks.tolist() == [V - 1 - x for x in refs[r]["prompt"][1:]]


def test_behind_the_resident_prefix(q3, models):
    m = models()
    k = 9
    prefix = m.prompt(700, 37)
    suffixes = [m.prompt(701 + i, n) for i, n in enumerate((1, 20, 60))]
    full = [prefix + s for s in suffixes]
    refs = m.refs(full)
    with m.engine() as t:
        t.batch_init(4)
        t.batch_prefix_set(prefix)
        got = t.score_top_many(suffixes, k, use_prefix=True)
        check(got, refs, k, "suffixes behind the prefix", [38] * 3)
        assert got[3] == want_stats(q3, [1, 20, 60], None, 4) and (got[3].live_columns, got[3].scored) == (81, 78)
        assert t.batch_prefix_get() == prefix
        for i, r in enumerate(refs):
            check_rows(t, i, r, len(full[i]), f"slot {i}: prefix and suffix rows")
        same_records(t, suffixes, got, use_prefix=True)
        plain = t.score_top_many(full, k, [38] * 3)
        for a, b in zip(plain[:3], got[:3]):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        want = [(q3.logprobs_of(r), np.array(tp["index"]), q3.top_logprobs_of(r, tp), rk) for r, tp, rk in zip(*got[:3])]
        for res in (q3.top_logprobs(t, full, k, [38] * 3, shared_prefix=True), q3.top_logprobs(t, suffixes, k, shared_prefix=prefix),
                    q3.top_logprobs(t, full, k, [38] * 3)):
            assert t.batch_prefix_get() == prefix
            for g, w in zip(res, want):
                assert [x.dtype for x in g] == [np.float64, np.int32, np.float64, np.int32] and all(np.array_equal(x, y) for x, y in zip(g, w))
                hit = np.flatnonzero(g[3] < k)                  # where the target is listed, its log-prob is the listed one
                assert np.array_equal(g[2][hit, g[3][hit]], g[0][hit])


def test_nothing_else_moved(q3, models):
    """score_many, embed_many and choice_many give the same bytes before and after score_top_many; generate_many, greedy and
    sampled, gives the same rows behind it; a draw under set_batch_sampler is the same draw: no slot rng was advanced"""
    m = models()
    prompts = [m.prompt(800 + i, n) for i, n in enumerate((12, 40, 3, 70, 9))]
    seeds = [21, 22, 23, 24, 25]
    T, P = 0.7, 0.9
    cands = [int(c) for c in np.random.default_rng(810).integers(0, m.shape.vocab_size, 5)]

    def rest(t):
        greedy = q3.generate_many(t, prompts, 4)[0]
        sampled = q3.generate_many(t, prompts, 4, sampler=(T, P, seeds))[0]
        t.set_batch_sampler(T, P, seeds[:3])
        return greedy, sampled

    def draw(t):
        return t.batch_step_cols_draw([0, 1, 2], [p[0] for p in prompts[:3]], [0, 0, 0])

    with m.engine() as t:
        t.batch_init(3)
        greedy, sampled = rest(t)
        draws = draw(t)
    refs = m.refs(prompts)
    with m.engine() as t:
        t.batch_init(3)
        emb, cho = t.embed_many(prompts)[0], t.choice_many(prompts, cands)[0]
        sco = [r.tobytes() for r in t.score_many(prompts)[0]]
        check(t.score_top_many(prompts, 20), refs, 20, "before")
        t.score_top_many(prompts[:2], 64, [5, 1])
        assert [r.tobytes() for r in t.score_many(prompts)[0]] == sco
        assert_biteq(t.embed_many(prompts)[0], emb, "embed_many behind score_top_many")
        assert_biteq(t.choice_many(prompts, cands)[0], cho, "choice_many behind score_top_many")
        assert rest(t) == (greedy, sampled)
        check(t.score_top_many(prompts, 3), refs, 3, "under a sampling batch")          # and no coin drawn
        assert draw(t) == draws


def test_errors_leave_the_engine_usable(q3, models):
    import ctypes as C
    m = models()
    refs = m.by_len(900, (41, 6))
    p = refs[0]["prompt"]
    V = m.shape.vocab_size
    with m.engine() as t:
        with pytest.raises(IndexError):
            t.score_top_many([p], 3)                                             # no batch_init
        t.batch_init(2)
        for prompts, sf, kw in (([], None, {}), ([p, []], None, {}), ([p[:5] + [V]], None, {}), ([p[:5] + [-1]], None, {}), ([p], [0], {}),
                                ([p], [len(p) + 1], {}), ([p, p], [1], {}), ([p], [1, 1], {}), ([p], None, dict(use_prefix=True)),
                                ([p * 20], None, {})):
            with pytest.raises(IndexError):
                t.score_top_many(prompts, 3, sf, **kw)
        for k in (0, -1, 65):
            with pytest.raises(IndexError):
                t.score_top_many([p], k)
        lens, toks, one = (C.c_size_t * 1)(len(p)), (C.c_int32 * len(p))(*p), (C.c_size_t * 1)(1)
        out = np.zeros(len(p), dtype=q3.SCORE_DTYPE).ctypes.data_as(C.c_void_p)
        top = np.zeros((len(p), 64), dtype=q3.TOP_DTYPE).ctypes.data_as(C.c_void_p)
        rank = np.zeros(len(p), dtype=np.int32).ctypes.data_as(C.c_void_p)
        for args in ((toks, lens, 1, one, 8, 3, out, top, rank), (toks, lens, 1, one, 0x80000002, 3, out, top, rank), (None, lens, 1, one, 0, 3, out, top, rank),
                     (toks, None, 1, one, 0, 3, out, top, rank), (toks, lens, 1, one, 0, 3, None, top, rank), (toks, lens, 0, one, 0, 3, out, top, rank),
                     (toks, lens, 1, one, 0, 3, out, None, rank), (toks, lens, 1, one, 0, 3, out, None, None), (toks, lens, 1, one, 0, 65, out, top, rank),
                     (toks, lens, 1, one, 0, 0, out, top, rank)):
            assert t._lib.q3_score_top_many(t._h, *args, None) == -3, args[2:6]
        assert t._lib.q3_score_top_many(t._h, toks, lens, 1, one, 0, 3, out, None, rank, None) == -3 and b"null top" in t._lib.q3_last_error()
        last = (C.c_size_t * 1)(len(p))
        assert t._lib.q3_score_top_many(t._h, toks, lens, 1, last, 0, 3, None, None, None, None) == 0       # no record: null outputs are legal
        assert t._lib.q3_score_top_many(t._h, toks, lens, 1, one, 0, 3, out, top, None, None) == 0          # no rank asked for
        check(t.score_top_many([r["prompt"] for r in refs], 64), refs, 64, "behind the refused calls")
    with m.engine(fast=True) as t:
        t.batch_init(2)
        with pytest.raises(q3.Q3Error) as ei:
            t.score_top_many([p], 3)
        assert ei.value.code == -5 and "Q3_FLAG_FAST" in ei.value.msg


def test_k_above_the_vocabulary_is_refused_and_k_equal_to_it_is_the_whole_row(q3, tmp_path):
    """V = 48, three 16-row tiles of the classifier and fewer entries than Q3_SCORE_TOP_MAX: k = 49 .. 64 is refused, k = 48 sorts
    the whole row -- 48 slices of one entry and 16 empty ones"""
    ck = q3.checkpoint
    shape = ck.ModelShape(256, 384, 2, 4, 2, 48, 96, 64, True, 64)
    path = str(tmp_path / "v48.bin")
    ck.write_synthetic_checkpoint(path, shape, seed=5)
    p = [1, 47, 0, 30, 30, 2]
    with q3.TransformerBuilder(path).build() as t:
        rows = [np.array(t.forward(p[i], i), copy=True) for i in range(len(p) - 1)]
        t.batch_init(2)
        for k in (49, 64):
            with pytest.raises(IndexError) as ei:
                t.score_top_many([p], k)
            assert "exceeds vocab_size 48" in str(ei.value)
        for k in (48, 1):
            got = t.score_top_many([p], k)
            assert_tops(got[1][0], np.stack([tr.top(l, k) for l in rows]), f"V = 48, k = {k}")
            assert got[2][0].tolist() == [tr.rank(l, x) for l, x in zip(rows, p[1:])]
            invariants(got[0][0], got[1][0], got[2][0], p[1:], k, "V = 48")
            same_records(t, [p], got)
        assert sorted(got[1][0]["index"][:, 0].tolist()) == sorted(int(np.argmax(tr.keys(l))) for l in rows)


def test_the_command_line(q3, tmp_path, capsys):
    import os
    from qwen3_rs_amd import cli
    from qwen3_rs_amd import tokenizer as tk
    from test_tokenizer_cli import make_tokenizer_json
    ck = q3.checkpoint
    d = str(tmp_path)
    n_vocab = make_tokenizer_json(d)
    shape = ck.ModelShape(256, 384, 2, 4, 2, n_vocab + (16 - n_vocab % 16) % 16, 512, 64, True, 64)
    path = os.path.join(d, "model.bin")
    ck.write_synthetic_checkpoint(path, shape, seed=12)
    tk.export_tokenizer(d, path, 1, 2)
    tok = tk.Tokenizer(path, shape.vocab_size)
    texts, out, out_top = ["hello world hello", "world hello hello lo"], os.path.join(d, "out.npy"), os.path.join(d, "top.npz")
    common = ["score", path, "-i", texts[0], "-i", texts[1], "--context", "hello?", "--streams", "2"]
    assert cli.main(common + ["-o", out]) == 0
    plain = [ln.split() for ln in capsys.readouterr().out.strip().splitlines()]
    assert cli.main(common + ["-o", out_top, "--top", "3"]) == 0
    lines = [ln.split() for ln in capsys.readouterr().out.strip().splitlines()]
    ctx = tok.encode("hello?")
    enc = [tok.encode(x) for x in texts]
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(2)
        want_plain = q3.score(t, [ctx + e for e in enc], [len(ctx)] * 2)
        want = q3.top_logprobs(t, [ctx + e for e in enc], 3, [len(ctx)] * 2)
    # without --top: the four columns and the vector of today
    assert plain == [[str(r), str(lp.size), f"{lp.sum():.6f}", f"{q3.perplexity([lp]):.6f}"] for r, lp in enumerate(want_plain)]
    got = np.load(out)
    assert got.dtype == np.float64 and np.array_equal(got, np.concatenate(want_plain))
    # with it: the same four and the count of targets among the three most likely
    assert [ln[:4] for ln in lines] == plain and [int(ln[4]) for ln in lines] == [int((w[3] < 3).sum()) for w in want] and all(len(ln) == 5 for ln in lines)
    z = np.load(out_top)
    assert sorted(z.files) == ["lengths", "logprobs", "rank", "top_ids", "top_logprobs"]
    for j, name in enumerate(("logprobs", "top_ids", "top_logprobs", "rank")):
        assert np.array_equal(z[name], np.concatenate([w[j] for w in want])), name
    assert z["lengths"].tolist() == [len(e) for e in enc] and z["top_ids"].shape == (sum(len(e) for e in enc), 3)
    assert np.array_equal(z["logprobs"], got)
