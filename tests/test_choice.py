"""Choice logits: the classifier's scores of a few candidate tokens behind many prompts (include/qwen3_hip.h section 2k,
q3_choice_many).  The yardstick is the sequential path on a single-stream engine of the same context -- prefill of all but the last
prompt token, forward of the last, its logits at the candidate ids -- and every comparison is bit for bit."""
import numpy as np
import pytest

import edge_ckpt
import group_cases
from conftest import assert_biteq
from test_dense_slots import check_rows
from test_embed import CTX, NAME, Model, pack_sum

pytestmark = pytest.mark.gpu


class ChoiceModel(Model):
    """test_embed.Model whose references carry the logits of the last token's forward as well"""

    def __init__(self, q3, name, path, ctx=CTX, shape=None):
        if shape is not None:                     # a shape of tests/group_cases.py, which edge_ckpt.SHAPES does not list
            self.q3, self.name, self.path, self.shape = q3, name, path, shape
            self.ctx = min(ctx, shape.max_seq_len)
            self._refs = {}
        else:
            super().__init__(q3, name, path, ctx)

    def refs(self, prompts):
        todo = [tuple(p) for p in prompts if tuple(p) not in self._refs]
        if todo:
            with self.engine() as t:
                cfg = t.get_config()
                kvd = cfg.n_kv_heads * cfg.head_dim
                for p in todo:
                    n = len(p)
                    t.reset_kv()
                    if n > 1:
                        t.prefill(list(p[:-1]), 0)
                    logits = t.forward(p[-1], n - 1).copy()
                    self._refs[p] = dict(prompt=list(p), logits=logits, x=t.read_state("x").copy(),
                                         key=t.read_state("key").reshape(cfg.n_layers, self.ctx, kvd)[:, :n].copy(),
                                         value=t.read_state("value").reshape(cfg.n_layers, self.ctx, kvd)[:, :n].copy())
        return [self._refs[tuple(p)] for p in prompts]

    def ids(self, seed, k):
        return [int(c) for c in np.random.default_rng(seed).integers(0, self.shape.vocab_size, k)]


@pytest.fixture(scope="module")
def models(q3, tmp_path_factory):
    made = {}

    def get(name=NAME, edit=None, seed=2468):
        if (name, edit) not in made:
            path = str(tmp_path_factory.mktemp("choice") / f"{name}-{edit}.bin")
            if edit:
                edge_ckpt.write(path, name, edit)
                made[(name, edit)] = ChoiceModel(q3, name, path)
            elif name in group_cases.SHAPES:
                q3.checkpoint.write_synthetic_checkpoint(path, group_cases.SHAPES[name], seed=group_cases.CKPT_SEED)
                made[(name, edit)] = ChoiceModel(q3, name, path, shape=group_cases.SHAPES[name])
            else:
                q3.checkpoint.write_synthetic_checkpoint(path, q3.checkpoint.SHAPES[name], seed=seed)
                made[(name, edit)] = ChoiceModel(q3, name, path)
        return made[(name, edit)]
    return get


def check(rows, refs, cands, what, per_request=False):
    """rows[r][j] is reference r's logit at its j-th candidate"""
    assert rows.dtype == np.float32 and rows.shape == (len(refs), len(cands[0]) if per_request else len(cands))
    for i, r in enumerate(refs):
        ids = cands[i] if per_request else cands
        assert_biteq(rows[i], r["logits"][ids], f"{what}: request {i} of {len(r['prompt'])} tokens")


def choice_raw(q3, m, refs, streams, cands, what, cap=2048):
    """one shared list through `streams` slots on a fresh engine: every row is its reference's, the stats are the schedule's"""
    with m.engine() as t:
        t.batch_init(streams)
        rows, st = t.choice_many([r["prompt"] for r in refs], cands)
        check(rows, refs, cands, what)
        assert st == pack_sum(q3, [len(r["prompt"]) for r in refs], streams, cap)
    return rows


def test_one_block_many_slots(q3, models):
    m = models()
    V = m.shape.vocab_size
    lens = (1, 2, 9, 41, 97, 33, 8, 70)
    cands = [0, V - 1, 17, 17]                   # the first and the last row of the matrix, and a duplicate
    refs = m.by_len(100, lens)
    with m.engine() as t:
        t.batch_init(8)
        rows, st = t.choice_many([r["prompt"] for r in refs], cands)
        check(rows, refs, cands, "one block")
        assert_biteq(rows[:, 2], rows[:, 3], "a duplicate id gives equal values")
        want = q3.dense_pack(list(lens), 2048)[1]
        assert want.blocks == 1 and st == q3.EmbedStats(1, want.blocks, want.live_columns, want.pad_columns)
        for i, r in enumerate(refs):
            check_rows(t, i, r, lens[i], f"slot {i}")


def test_candidate_counts(q3, models):
    """fewer candidates than waves, a count that is no multiple of the waves, a part of 32 and one past it, the cap and one below"""
    m = models()
    refs = m.by_len(150, (41, 9, 3))
    prompts = [r["prompt"] for r in refs]
    with m.engine() as t:
        t.batch_init(4)
        for k in (1, 3, 4, 5, 32, 33, 255, 256):
            cands = m.ids(160 + k, k)
            rows, _ = t.choice_many(prompts, cands)
            check(rows, refs, cands, f"k = {k}")


def test_per_request_lists_and_more_requests_than_slots(q3, models):
    m = models()
    lens = (120, 5, 33, 64, 7, 90, 1, 12, 40, 3, 17)
    refs = m.by_len(200, lens)
    cands = [m.ids(210 + i, 5) for i in range(len(lens))]
    assert len({tuple(c) for c in cands}) == len(cands)
    with m.engine() as t:
        t.batch_init(4)
        rows, st = t.choice_many([r["prompt"] for r in refs], cands)
        assert st.waves == 3 and st == pack_sum(q3, list(lens), 4)
        check(rows, refs, cands, "per-request lists", per_request=True)
        one, _ = t.choice_many([r["prompt"] for r in refs], cands[0])      # the shared form behind the per-request one, same buffers
        check(one, refs, cands[0], "the shared list")


def test_a_run_split_over_blocks(q3, models, monkeypatch):
    monkeypatch.setenv("Q3_PREFILL_M", "128")
    m = models()
    choice_raw(q3, m, m.by_len(300, (300, 40, 129)), 3, m.ids(310, 6), "blocks of 128", cap=128)


def test_a_narrow_block(q3, models):
    m = models()
    choice_raw(q3, m, m.by_len(400, (3, 5)), 2, m.ids(401, 7), "one block of 16 columns")


@pytest.mark.parametrize("name,lens,cap", [("small-hd128", (40, 3), 2048), ("tiny-g64", (50, 9), 32)])
def test_small_shapes_against_the_cpu_oracle(q3, oracle, models, name, lens, cap):
    """tiny-g64 (head_dim 64) is a shape the dense kernels refuse: walked 32 columns at a time through the column plans.  Both are
    held to the single-stream engine and to the C oracle"""
    m = models(name, seed=92)
    V = m.shape.vocab_size
    refs = m.by_len(420, lens)
    cands = [0, V - 1] + m.ids(421, 9)
    rows = choice_raw(q3, m, refs, 2, cands, name, cap=cap)
    om = oracle.OracleModel(m.path, m.ctx)
    for i, r in enumerate(refs):
        om.reset()
        for pos, tok in enumerate(r["prompt"]):
            want = np.array(om.forward(tok, pos), copy=True)
        assert_biteq(rows[i], want[cands], f"{name}: request {i} against the oracle")


@pytest.mark.parametrize("name,dim", [("qwen3-4b-dims-l2", 2560), ("qwen3-8b-dims-l2", 4096)])
def test_other_widths(q3, models, name, dim):
    """dim 2560: three 1 KiB chunks per row, the last half used; dim 4096 with its own lm_head: the largest PRO_NORM vector"""
    m = models(name)
    assert m.shape.dim == dim
    V = m.shape.vocab_size
    choice_raw(q3, m, m.by_len(500, (35, 8, 64)), 3, [0, V - 1] + m.ids(501, 35), name)


@pytest.mark.parametrize("name", ["dims06-g128", "g256-hd128"])
def test_group_sizes_128_and_256(q3, models, name):
    """8 and 16 lanes of a wave share a group; g256-hd128 has its own lm_head"""
    m = models(name)
    assert m.shape.group_size in (128, 256)
    V = m.shape.vocab_size
    refs = m.by_len(520, (40, 9))
    cands = [0, V - 1] + m.ids(521, 9)
    with m.engine() as t:
        t.batch_init(2)
        rows, _ = t.choice_many([r["prompt"] for r in refs], cands)
        check(rows, refs, cands, name)


@pytest.mark.parametrize("edit", ["all", "flat_logits"])
def test_edge_valued_checkpoints(q3, models, edit):
    """all: zero groups in the activations, so zero scales and zero codes, and a tied classifier: rows 2i and 2i + 1 are equal;
    flat_logits: a zero norm weight, every logit the sum of zero terms"""
    m = models(NAME, edit)
    V = m.shape.vocab_size
    cands = [0, 1, V - 2, V - 1, 500, 501] + m.ids(531, 6)
    rows = choice_raw(q3, m, m.by_len(530, (41, 9)), 2, cands, edit)
    if edit == "all":
        assert_biteq(rows[:, 0], rows[:, 1], "tied rows 0 and 1")
        assert_biteq(rows[:, 4], rows[:, 5], "tied rows 500 and 501")
    else:
        assert not rows.any()


def test_behind_the_resident_prefix(q3, models):
    m = models()
    prefix = m.prompt(700, 37)
    suffixes = [m.prompt(701 + i, n) for i, n in enumerate((1, 20, 60))]
    full = [prefix + s for s in suffixes]
    refs = m.refs(full)
    cands = m.ids(710, 6)
    with m.engine() as t:
        t.batch_init(4)
        t.batch_prefix_set(prefix)
        rows, st = t.choice_many(suffixes, cands, use_prefix=True)
        check(rows, refs, cands, "suffixes behind the prefix")
        assert st == pack_sum(q3, [1, 20, 60], 4) and st.live_columns == 81
        assert t.batch_prefix_get() == prefix
        for i, r in enumerate(refs):
            check_rows(t, i, r, len(full[i]), f"slot {i}: prefix and suffix rows")
        plain, _ = t.choice_many(full, cands)
        assert_biteq(plain, rows, "the full prompts without a prefix")
        assert_biteq(q3.choose(t, full, cands, shared_prefix=True), rows, "generation.choose, shared_prefix=True")
        assert t.batch_prefix_get() == prefix
        assert_biteq(q3.choose(t, suffixes, cands, shared_prefix=prefix), rows, "generation.choose, a token list")
        assert_biteq(q3.choose(t, full, cands), rows, "generation.choose, no prefix")
        assert t.batch_prefix_get() == prefix
        p = q3.choose(t, full, cands, shared_prefix=True, output="softmax")
        assert p.dtype == np.float64 and np.all(np.abs(p.sum(axis=1) - 1.0) <= len(cands) * 2.0 ** -52)


def test_nothing_else_moved(q3, models):
    """generate_many, greedy and sampled, gives the same rows behind a choice_many call; a draw under set_batch_sampler is the same
    draw: no slot rng was advanced.  embed_many, which shares the walk and its buffers, gives the same rows before and after."""
    m = models()
    prompts = [m.prompt(800 + i, n) for i, n in enumerate((12, 40, 3, 70, 9))]
    seeds = [21, 22, 23, 24, 25]
    T, P = 0.7, 0.9
    cands = m.ids(810, 5)

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
        before, _ = t.embed_many(prompts)
        t.choice_many(prompts, cands)
        t.choice_many(prompts[:2], [cands[:2], cands[2:4]])
        after, _ = t.embed_many(prompts)
        assert_biteq(after, before, "embed_many behind choice_many")
        assert_biteq(t.embed_many(prompts, normalize=False)[0], np.stack([r["x"] for r in refs]), "embed_many against its references")
        assert rest(t) == (greedy, sampled)
        rows, _ = t.choice_many(prompts, cands)                  # under a sampling batch: the references' rows, and no coin drawn
        check(rows, refs, cands, "under a sampling batch")
        assert draw(t) == draws


def test_errors_leave_the_engine_usable(q3, models):
    import ctypes as C
    m = models()
    refs = m.by_len(900, (41, 6))
    p = refs[0]["prompt"]
    V = m.shape.vocab_size
    cands = [3, V - 1]
    with m.engine() as t:
        with pytest.raises(IndexError):
            t.choice_many([p], cands)                                            # no batch_init
        t.batch_init(2)
        for prompts, cd, kw in (([], cands, {}), ([p, []], cands, {}), ([p[:5] + [V]], cands, {}), ([p], [3, -1], {}), ([p], [V, 3], {}),
                                ([p], [], {}), ([p], list(range(257)), {}), ([p, p], [[1, 2], [3]], {}), ([p, p], [[1, 2]], {}),
                                ([p, p], [[1, 2], [3, V]], {}), ([p], cands, dict(use_prefix=True))):
            with pytest.raises(IndexError):
                t.choice_many(prompts, cd, **kw)
        lens, toks, cd, out = (C.c_size_t * 1)(len(p)), (C.c_int32 * len(p))(*p), (C.c_int32 * 2)(*cands), (C.c_float * 2)()
        for args in ((toks, lens, 1, cd, 2, 8, out), (toks, lens, 1, cd, 2, 1, out), (toks, lens, 1, cd, 2, 0x80000002, out),
                     (toks, lens, 1, None, 2, 0, out), (None, lens, 1, cd, 2, 0, out), (toks, None, 1, cd, 2, 0, out),
                     (toks, lens, 1, cd, 2, 0, None), (toks, lens, 0, cd, 2, 0, out), (toks, lens, 1, cd, 0, 0, out), (toks, lens, 1, cd, 257, 0, out)):
            assert t._lib.q3_choice_many(t._h, *args, None) == -3, args[2:6]
        rows, _ = t.choice_many([r["prompt"] for r in refs], cands)
        check(rows, refs, cands, "behind the refused calls")
    with m.engine(fast=True) as t:
        t.batch_init(2)
        with pytest.raises(q3.Q3Error) as ei:
            t.choice_many([p], cands)
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
    docs, out = ["hello world", "world hello hello", "lo"], os.path.join(d, "out.npy")
    assert cli.main(["rerank", path, "-q", "hello?", "-d", docs[0], "-d", docs[1], "-d", docs[2], "--instruct", "hell", "--yes", "hello", "--no", "or",
                     "-o", out, "--streams", "2"]) == 0
    got = np.load(out)
    lines = capsys.readouterr().out.strip().splitlines()
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(2)
        want = q3.rerank(t, tok, "hello?", docs, instruction="hell", yes="hello", no="or")
        prompts = [tok.encode(q3.RERANK_TEMPLATE.format(instruction="hell", query="hello?", document=x)) for x in docs]
        ids = tok.encode("or") + tok.encode("hello")
        two = q3.choose(t, prompts, ids)
    assert got.dtype == np.float64 and got.shape == (3,) and np.array_equal(got, want)
    assert np.array_equal(want, q3.normalise_logits(two, "softmax")[:, 1])
    assert [ln.split()[0] for ln in lines] == ["0", "1", "2"] and [float(ln.split()[1]) for ln in lines] == [float(f"{v:.6f}") for v in want]
    assert cli.main(["rerank", path, "-q", "hello?", "-d", docs[0]]) == 1          # "yes" is three tokens in this tokenizer
