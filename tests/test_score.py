"""Scores: per-position records of many prompts (include/qwen3_hip.h section 2l, q3_score_many).  The yardstick is forward() per
position on a single-stream engine of the same context, its logits reduced on the host by tests/score_ref.py (glibc's expf, the
sequential f32 sum from -0.0).  Every record is compared as the header's standard says: target and sum by bits, argmax equal, max
by value."""
import numpy as np
import pytest

import edge_ckpt
import group_cases
import logit_ckpt as lc
import score_ref
from conftest import assert_biteq
from score_ref import assert_records
from test_choice import ChoiceModel
from test_dense_slots import check_rows
from test_embed import NAME

pytestmark = pytest.mark.gpu


class Reducer:
    """score_ref.record with the vocabulary-wide part remembered per distinct logit row (the designed checkpoints repeat theirs)"""

    def __init__(self):
        self._memo = {}

    def __call__(self, l, target):
        key = hash(l.tobytes())
        if key not in self._memo:
            self._memo[key] = score_ref.record(l, 0)
        r = self._memo[key].copy()
        r["target"] = l[target]
        return r


class ScoreModel(ChoiceModel):
    """test_embed.Model whose references carry the record of every position but the last: forward() per position, cache zeroed in
    front of every prompt; x, key and value behind the last token are what check_rows reads"""

    def refs(self, prompts):
        todo = [tuple(p) for p in prompts if tuple(p) not in self._refs]
        if todo:
            with self.engine() as t:
                cfg = t.get_config()
                kvd = cfg.n_kv_heads * cfg.head_dim
                for p in todo:
                    n = len(p)
                    t.reset_kv()
                    recs = np.zeros(n - 1, dtype=score_ref.DTYPE)
                    for i in range(n):
                        l = t.forward(p[i], i)
                        if i + 1 < n:
                            recs[i] = score_ref.record(l, p[i + 1])
                    self._refs[p] = dict(prompt=list(p), records=recs, x=t.read_state("x").copy(),
                                         key=t.read_state("key").reshape(cfg.n_layers, self.ctx, kvd)[:, :n].copy(),
                                         value=t.read_state("value").reshape(cfg.n_layers, self.ctx, kvd)[:, :n].copy())
        return [self._refs[tuple(p)] for p in prompts]


@pytest.fixture(scope="module")
def models(q3, tmp_path_factory):
    made = {}

    def get(name=NAME, edit=None, seed=2468):
        if (name, edit) not in made:
            path = str(tmp_path_factory.mktemp("score") / f"{name}-{edit}.bin")
            if edit:
                edge_ckpt.write(path, name, edit)
                made[(name, edit)] = ScoreModel(q3, name, path)
            elif name in group_cases.SHAPES:
                q3.checkpoint.write_synthetic_checkpoint(path, group_cases.SHAPES[name], seed=group_cases.CKPT_SEED)
                made[(name, edit)] = ScoreModel(q3, name, path, shape=group_cases.SHAPES[name])
            else:
                q3.checkpoint.write_synthetic_checkpoint(path, q3.checkpoint.SHAPES[name], seed=seed)
                made[(name, edit)] = ScoreModel(q3, name, path)
        return made[(name, edit)]
    return get


def want_stats(q3, lens, score_from, streams, cap=2048):
    """the schedule counted in Python, which the host-only q3_score_pack has to give as well"""
    want = q3.ScoreStats(*score_ref.schedule(list(lens), score_from, streams, cap))
    assert q3.score_pack(list(lens), score_from, streams, cap) == want
    return want


def check(recs, refs, what, score_from=None):
    assert len(recs) == len(refs)
    for i, r in enumerate(refs):
        f = 1 if score_from is None else score_from[i]
        assert_records(recs[i], r["records"][f - 1:], f"{what}: request {i} of {len(r['prompt'])} tokens from {f}")


def score_raw(q3, m, refs, streams, what, cap=2048, score_from=None):
    """through `streams` slots on a fresh engine: every record is its reference's, the stats are the schedule's"""
    with m.engine() as t:
        t.batch_init(streams)
        recs, st = t.score_many([r["prompt"] for r in refs], score_from)
        check(recs, refs, what, score_from)
        assert st == want_stats(q3, [len(r["prompt"]) for r in refs], score_from, streams, cap)
    return recs


def test_one_wide_block_many_slots(q3, models):
    m = models()
    lens = (1, 2, 9, 41, 97, 33, 8, 70)
    refs = m.by_len(100, lens)
    with m.engine() as t:
        t.batch_init(8)
        recs, st = t.score_many([r["prompt"] for r in refs])
        check(recs, refs, "one block")
        assert st == want_stats(q3, lens, None, 8) and (st.blocks, st.scored, st.chunks) == (1, 253, 8)
        assert sum(r.size for r in recs) == 253 and recs[0].size == 0
        for i, r in enumerate(refs):
            check_rows(t, i, r, lens[i], f"slot {i}")           # the prompt's rows, and nothing behind them


def test_chunk_edges_inside_one_block(q3, models):
    """31, 32, 33 and 65 scored columns in one block; with 33 and 65 the second request's columns straddle two chunks"""
    m = models()
    with m.engine() as t:
        t.batch_init(4)
        for lens, scored, chunks in (((20, 13), 31, 1), ((20, 14), 32, 1), ((20, 15), 33, 2), ((20, 15, 33), 65, 3)):
            refs = m.by_len(1100, lens)
            prompts = [r["prompt"] for r in refs]
            recs, st = t.score_many(prompts)
            check(recs, refs, f"{scored} scored columns")
            assert (st.blocks, st.scored, st.chunks) == (1, scored, chunks) and st == want_stats(q3, lens, None, 4)
        alone, st = t.score_many(prompts[1:2])
        assert st.chunks == 1
        assert_records(alone[0], recs[1], "the request that straddled two chunks, scored alone")


def test_score_from(q3, models):
    """1, n, n - 1 and values in between, a one-token request between two others, 11 requests through 4 slots in 3 waves: the
    records are the slices of the all-positions call's"""
    m = models()
    lens = (120, 5, 33, 64, 7, 90, 1, 12, 40, 3, 17)
    sf = [1, 5, 32, 30, 4, 90, 1, 11, 17, 1, 9]
    assert sf[1] == lens[1] and sf[2] == lens[2] - 1 and sf[5] == lens[5] and lens[6] == 1
    refs = m.by_len(200, lens)
    prompts = [r["prompt"] for r in refs]
    with m.engine() as t:
        t.batch_init(4)
        full, st = t.score_many(prompts)
        assert st.waves == 3 and st == want_stats(q3, lens, None, 4)
        check(full, refs, "all positions")
        part, st = t.score_many(prompts, sf)
        assert st == want_stats(q3, lens, sf, 4) and st.scored == sum(n - f for n, f in zip(lens, sf))
        check(part, refs, "score_from", sf)
        for i, f in enumerate(sf):
            assert part[i].tobytes() == full[i][f - 1:].tobytes(), i
        assert part[1].size == 0 and part[5].size == 0 and part[6].size == 0 and part[2].size == 1


def test_a_run_split_over_blocks(q3, models, monkeypatch):
    monkeypatch.setenv("Q3_PREFILL_M", "128")
    m = models()
    score_raw(q3, m, m.by_len(300, (300, 40, 129)), 3, "blocks of 128", cap=128)


def test_a_narrow_block(q3, models):
    m = models()
    refs = m.by_len(400, (3, 5))
    score_raw(q3, m, refs, 2, "one block of 16 columns")
    score_raw(q3, m, refs[:1], 1, "the scored columns stand in place")           # columns 0 and 1 are rows 0 and 1: no gather


@pytest.mark.parametrize("name,lens,cap", [("small-hd128", (40, 3), 2048), ("tiny-g64", (50, 9), 32)])
def test_small_shapes_against_the_cpu_oracle(q3, oracle, models, name, lens, cap):
    """tiny-g64 (head_dim 64) is a shape the dense kernels refuse: walked 32 columns at a time through the column plans.  Both are
    held to the single-stream engine and to the C oracle's logits"""
    m = models(name, seed=92)
    refs = m.by_len(420, lens)
    recs = score_raw(q3, m, refs, 2, name, cap=cap)
    om = oracle.OracleModel(m.path, m.ctx)
    for i, r in enumerate(refs):
        om.reset()
        p = r["prompt"]
        want = score_ref.records([np.array(om.forward(p[pos], pos), copy=True) for pos in range(len(p) - 1)], p[1:])
        assert_records(recs[i], want, f"{name}: request {i} against the oracle")


@pytest.mark.parametrize("name,dim", [("qwen3-4b-dims-l2", 2560), ("qwen3-8b-dims-l2", 4096)])
def test_one_segment_vocabulary(q3, models, name, dim):
    """V = 16,384: exactly one segment of the sequential sum; dim 2560 and 4096, the latter with its own lm_head"""
    m = models(name)
    assert m.shape.dim == dim and m.shape.vocab_size == 16384
    score_raw(q3, m, m.by_len(500, (35, 8, 64)), 3, name)


DESIGNED = {"big_a": ("peaked", "uniform"), "big_b": ("ramp",), "big_c": ("twins", "ramp_up")}


@pytest.mark.parametrize("file", sorted(DESIGNED))
def test_the_full_vocabulary_on_designed_logits(q3, tmp_path_factory, file):
    """151,936 logits that depend on the input token alone (token t: design t % 4 of the file): ten segments of the sequential
    sum, a flat row, a tie at both ends, a ramp whose exps run through the subnormals into zeros"""
    V, names = lc.FILES[file]
    path = lc.write(str(tmp_path_factory.mktemp("score_designed") / f"{file}.bin"), file)
    groups = [names.index(d) for d in DESIGNED[file]]
    rng = np.random.default_rng(31)
    prompts = []
    for n in (5, 8, 6):
        p = [int(4 * rng.integers(0, V // 4) + groups[i % len(groups)]) for i in range(n)]
        prompts.append(p)
    prompts[0][1], prompts[1][2], prompts[2][3] = groups[0], V - 4 + groups[-1], 9 if file == "big_c" else 4 + groups[0]
    prompts[1][5] = V - 9
    reduce = Reducer()
    with q3.TransformerBuilder(path).build() as t:
        want, rows = [], []
        for p in prompts:
            t.reset_kv()
            ls = [np.array(t.forward(p[i], i), copy=True) for i in range(len(p) - 1)]
            want.append(np.array([reduce(l, p[i + 1]) for i, l in enumerate(ls)], dtype=score_ref.DTYPE))
            rows.append(ls)
        t.batch_init(3)
        recs, st = t.score_many(prompts)
        assert st.scored == sum(len(p) - 1 for p in prompts) and st == want_stats(q3, [len(p) for p in prompts], None, 3, 32)
    for r, (p, got) in enumerate(zip(prompts, recs)):
        assert_records(got, want[r], f"{file}: request {r}")
        for i in range(len(p) - 1):
            design = names[p[i] % 4]
            if design == "uniform":
                assert got["sum"][i] == np.float32(151936.0) and got["argmax"][i] == V - 1
            elif design == "twins":
                assert got["argmax"][i] == V - 9 and rows[r][i][9] == rows[r][i][V - 9] == got["max"][i]
            elif design == "ramp":
                e = score_ref.exps(rows[r][i])
                assert np.isfinite(got["sum"][i]) and got["sum"][i] == score_ref.seq_sum(e)
                assert (e == 0).any() and ((e > 0) & (e < lc.TINY)).any()                # zeros and subnormals in the tail


@pytest.mark.parametrize("name", ["dims06-g128", "g256-hd128"])
def test_group_sizes_128_and_256(q3, models, name):
    m = models(name)
    assert m.shape.group_size in (128, 256)
    refs = m.by_len(520, (40, 9))
    with m.engine() as t:
        t.batch_init(2)
        recs, _ = t.score_many([r["prompt"] for r in refs])
        check(recs, refs, name)


@pytest.mark.parametrize("edit", ["all", "flat_logits"])
def test_edge_valued_checkpoints(q3, models, edit):
    """all: zero groups in the activations and a tied classifier: rows 2i and 2i + 1 are equal, the argmax is the odd one;
    flat_logits: a zero norm weight, every logit the sum of zero terms"""
    m = models(NAME, edit)
    V = m.shape.vocab_size
    recs = score_raw(q3, m, m.by_len(530, (41, 9)), 2, edit)
    if edit == "all":
        assert all((r["argmax"] % 2 == 1).all() for r in recs)
    else:
        for r in recs:
            assert not r["target"].any() and (r["max"] == 0.0).all() and (r["sum"] == np.float32(V)).all() and (r["argmax"] == V - 1).all()


def test_behind_the_resident_prefix(q3, models):
    m = models()
    prefix = m.prompt(700, 37)
    suffixes = [m.prompt(701 + i, n) for i, n in enumerate((1, 20, 60))]
    full = [prefix + s for s in suffixes]
    refs = m.refs(full)
    with m.engine() as t:
        t.batch_init(4)
        t.batch_prefix_set(prefix)
        recs, st = t.score_many(suffixes, use_prefix=True)
        check(recs, refs, "suffixes behind the prefix", [38] * 3)
        assert st == want_stats(q3, [1, 20, 60], None, 4) and (st.live_columns, st.scored) == (81, 78)
        assert t.batch_prefix_get() == prefix
        for i, r in enumerate(refs):
            check_rows(t, i, r, len(full[i]), f"slot {i}: prefix and suffix rows")
        plain, _ = t.score_many(full, [38] * 3)
        for a, b in zip(plain, recs):
            assert a.tobytes() == b.tobytes()
        want = [q3.logprobs_of(r) for r in recs]
        for got in (q3.score(t, full, [38] * 3, shared_prefix=True), q3.score(t, suffixes, shared_prefix=prefix), q3.score(t, full, [38] * 3)):
            assert t.batch_prefix_get() == prefix
            assert [g.dtype for g in got] == [np.float64] * 3 and all(np.array_equal(g, w) for g, w in zip(got, want))
        assert np.array_equal(q3.score(t, suffixes[1:2], [7], shared_prefix=prefix)[0], want[1][6:])
        ll = q3.loglikelihood(t, [s[:1] for s in suffixes], [s[1:] for s in suffixes], shared_prefix=prefix)
        for i, ((total, greedy), r, w) in enumerate(zip(ll, recs, want)):
            assert total == float(w.sum()) and greedy == bool(np.array_equal(r["argmax"], np.asarray(full[i][38:], dtype=np.int32)))
        assert ll[0] == (0.0, True)
        assert ll == q3.loglikelihood(t, [prefix + s[:1] for s in suffixes], [s[1:] for s in suffixes])
        assert q3.perplexity(want) == float(np.exp(-np.concatenate(want).mean()))


def test_nothing_else_moved(q3, models):
    """embed_many and choice_many give the same rows before and after score_many; generate_many, greedy and sampled, gives the same
    rows behind it; a draw under set_batch_sampler is the same draw: no slot rng was advanced"""
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
        recs, _ = t.score_many(prompts)
        check(recs, refs, "before")
        t.score_many(prompts[:2], [5, 1])
        assert_biteq(t.embed_many(prompts)[0], emb, "embed_many behind score_many")
        assert_biteq(t.choice_many(prompts, cands)[0], cho, "choice_many behind score_many")
        assert_biteq(t.embed_many(prompts, normalize=False)[0], np.stack([r["x"] for r in refs]), "embed_many against its references")
        assert rest(t) == (greedy, sampled)
        recs, _ = t.score_many(prompts)                         # under a sampling batch: the references' records, and no coin drawn
        check(recs, refs, "under a sampling batch")
        assert draw(t) == draws


def test_errors_leave_the_engine_usable(q3, models):
    import ctypes as C
    m = models()
    refs = m.by_len(900, (41, 6))
    p = refs[0]["prompt"]
    V = m.shape.vocab_size
    with m.engine() as t:
        with pytest.raises(IndexError):
            t.score_many([p])                                                    # no batch_init
        t.batch_init(2)
        for prompts, sf, kw in (([], None, {}), ([p, []], None, {}), ([p[:5] + [V]], None, {}), ([p[:5] + [-1]], None, {}), ([p], [0], {}),
                                ([p], [len(p) + 1], {}), ([p, p], [1], {}), ([p], [1, 1], {}), ([p], None, dict(use_prefix=True)),
                                ([p * 20], None, {})):
            with pytest.raises(IndexError):
                t.score_many(prompts, sf, **kw)
        lens, toks, one = (C.c_size_t * 1)(len(p)), (C.c_int32 * len(p))(*p), (C.c_size_t * 1)(1)
        out = np.zeros(len(p), dtype=q3.SCORE_DTYPE).ctypes.data_as(C.c_void_p)
        for args in ((toks, lens, 1, one, 8, out), (toks, lens, 1, one, 1, out), (toks, lens, 1, one, 0x80000002, out), (None, lens, 1, one, 0, out),
                     (toks, None, 1, one, 0, out), (toks, lens, 1, one, 0, None), (toks, lens, 1, None, 0, None), (toks, lens, 0, one, 0, out)):
            assert t._lib.q3_score_many(t._h, *args, None) == -3, args[2:5]
        last = (C.c_size_t * 1)(len(p))
        assert t._lib.q3_score_many(t._h, toks, lens, 1, last, 0, None, None) == 0           # no record: a null out is legal
        recs, _ = t.score_many([r["prompt"] for r in refs])
        check(recs, refs, "behind the refused calls")
    with m.engine(fast=True) as t:
        t.batch_init(2)
        with pytest.raises(q3.Q3Error) as ei:
            t.score_many([p])
        assert ei.value.code == -5 and "Q3_FLAG_FAST" in ei.value.msg


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
    texts, out = ["hello world hello", "world hello hello lo"], os.path.join(d, "out.npy")

    def lines_of(lps):
        return [[str(r), str(lp.size), f"{lp.sum():.6f}", f"{q3.perplexity([lp]):.6f}"] for r, lp in enumerate(lps)]

    assert cli.main(["score", path, "-i", texts[0], "-i", texts[1], "--streams", "2"]) == 0
    plain = [ln.split() for ln in capsys.readouterr().out.strip().splitlines()]
    assert cli.main(["score", path, "-i", texts[0], "-i", texts[1], "--context", "hello?", "-o", out, "--streams", "2"]) == 0
    behind = [ln.split() for ln in capsys.readouterr().out.strip().splitlines()]
    got = np.load(out)
    ctx = tok.encode("hello?")
    enc = [tok.encode(x) for x in texts]
    assert len(ctx) > 1 and all(len(e) > 1 for e in enc)
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(2)
        want_plain = q3.score(t, enc)
        want_behind = q3.score(t, [ctx + e for e in enc], [len(ctx)] * 2)
    assert plain == lines_of(want_plain) and [w.size for w in want_plain] == [len(e) - 1 for e in enc]
    assert behind == lines_of(want_behind) and [w.size for w in want_behind] == [len(e) for e in enc]
    assert got.dtype == np.float64 and np.array_equal(got, np.concatenate(want_behind))
