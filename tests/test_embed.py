"""Embeddings: the last-token vectors of many prompts through dense blocks (include/qwen3_hip.h section 2j, q3_embed_many).
The yardstick is the sequential path on a single-stream engine of the same context -- prefill of all but the last prompt token,
forward of the last, read_state("x") -- and every comparison is bit for bit.  The L2 part is held to its numpy restatement
(tests/embed_ref.py)."""
import os

import numpy as np
import pytest

import edge_ckpt
import embed_ref
from conftest import assert_biteq
from test_dense_slots import check_rows

pytestmark = pytest.mark.gpu

NAME, CTX = "qwen3-0.6b-dims-l2", 512


class Model:
    """One checkpoint and its single-stream references, computed once and never changed."""

    def __init__(self, q3, name, path, ctx=CTX):
        self.q3, self.name, self.path = q3, name, path
        self.shape = edge_ckpt.SHAPES[name]
        self.ctx = min(ctx, self.shape.max_seq_len)
        self._refs = {}

    def engine(self, fast=False):
        b = self.q3.TransformerBuilder(self.path).with_ctx_length(self.ctx)
        return (b.with_strict(False) if fast else b).build()

    def prompt(self, seed, n):
        rng = np.random.default_rng(seed)
        return [int(t) for t in rng.integers(0, self.shape.vocab_size, n)]

    def refs(self, prompts):
        """per prompt dict(prompt, x = read_state("x") behind forward of its last token, key / value [L, ctx, kvd] rows of the prompt);
        the missing ones on one engine, its cache zeroed in front of every prompt"""
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
                    t.forward(p[-1], n - 1)
                    self._refs[p] = dict(prompt=list(p), x=t.read_state("x").copy(),
                                         key=t.read_state("key").reshape(cfg.n_layers, self.ctx, kvd)[:, :n].copy(),
                                         value=t.read_state("value").reshape(cfg.n_layers, self.ctx, kvd)[:, :n].copy())
        return [self._refs[tuple(p)] for p in prompts]

    def by_len(self, seed, lens):
        return self.refs([self.prompt(seed + i, n) for i, n in enumerate(lens)])


@pytest.fixture(scope="module")
def models(q3, tmp_path_factory):
    made = {}

    def get(name=NAME, edit=None):
        if (name, edit) not in made:
            path = str(tmp_path_factory.mktemp("embed") / f"{name}-{edit}.bin")
            if edit:
                edge_ckpt.write(path, name, edit)
            else:
                q3.checkpoint.write_synthetic_checkpoint(path, q3.checkpoint.SHAPES[name], seed=2468)
            made[(name, edit)] = Model(q3, name, path)
        return made[(name, edit)]
    return get


def pack_sum(q3, lens, streams, cap=2048):
    """EmbedStats of the schedule: waves of `streams` requests, each packed on its own"""
    waves = [lens[i:i + streams] for i in range(0, len(lens), streams)]
    st = [q3.dense_pack(list(w), cap)[1] for w in waves]
    return q3.EmbedStats(len(waves), sum(s.blocks for s in st), sum(s.live_columns for s in st), sum(s.pad_columns for s in st))


def embed_raw(q3, m, refs, streams, what, cap=2048):
    """flags 0 through `streams` slots on a fresh engine: every row is its reference's, the stats are the schedule's"""
    with m.engine() as t:
        t.batch_init(streams)
        rows, st = t.embed_many([r["prompt"] for r in refs], normalize=False)
        assert rows.shape == (len(refs), m.shape.dim) and rows.dtype == np.float32
        for i, r in enumerate(refs):
            assert_biteq(rows[i], r["x"], f"{what}: request {i} of {len(r['prompt'])} tokens")
        assert st == pack_sum(q3, [len(r["prompt"]) for r in refs], streams, cap)
    return rows


def test_one_block_many_slots(q3, models):
    m = models()
    lens = (1, 2, 9, 41, 97, 33, 8, 70)
    refs = m.by_len(100, lens)
    with m.engine() as t:
        t.batch_init(8)
        rows, st = t.embed_many([r["prompt"] for r in refs], normalize=False)
        for i, r in enumerate(refs):
            assert_biteq(rows[i], r["x"], f"request {i} of {lens[i]} tokens")
        want = q3.dense_pack(list(lens), 2048)[1]
        assert want.blocks == 1 and st == q3.EmbedStats(1, want.blocks, want.live_columns, want.pad_columns)
        for i, r in enumerate(refs):
            check_rows(t, i, r, lens[i], f"slot {i}")           # the prompt's rows, and nothing behind them


def test_more_requests_than_slots(q3, models):
    """slot 0: 120 tokens in wave 0, 7 in wave 1 (stale rows lie behind the shorter prompt), 40 in wave 2"""
    m = models()
    lens = (120, 5, 33, 64, 7, 90, 1, 12, 40, 3, 17)
    refs = m.by_len(200, lens)
    with m.engine() as t:
        t.batch_init(4)
        rows, st = t.embed_many([r["prompt"] for r in refs], normalize=False)
        assert st.waves == 3 and st == pack_sum(q3, list(lens), 4)
        for i, r in enumerate(refs):
            assert_biteq(rows[i], r["x"], f"request {i} of {lens[i]} tokens")


def test_a_run_split_over_blocks(q3, models, monkeypatch):
    """Q3_PREFILL_M=128: the 300-token run takes three blocks and its row comes from the third, which it shares with the 40-token
    run and the first piece of the 129-token run; that run's row comes from the fourth block"""
    monkeypatch.setenv("Q3_PREFILL_M", "128")
    m = models()
    lens = (300, 40, 129)
    assert [e[:3] for e in q3.dense_pack(list(lens), 128)[0]] == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 48, 1), (2, 88, 2), (3, 0, 2)]
    embed_raw(q3, m, m.by_len(300, lens), 3, "blocks of 128", cap=128)


def test_a_narrow_block(q3, models):
    m = models()
    embed_raw(q3, m, m.by_len(400, (3, 5)), 2, "one block of 16 columns")


def narrow_model(q3, tmp_path_factory, name, seed):
    path = str(tmp_path_factory.mktemp("embed_" + name) / "m.bin")
    q3.checkpoint.write_synthetic_checkpoint(path, q3.checkpoint.SHAPES[name], seed=seed)
    return Model(q3, name, path)


def test_a_shape_the_dense_kernels_refuse(q3, tmp_path_factory):
    """tiny-g64: head_dim 64, walked 32 columns at a time, layers only"""
    m = narrow_model(q3, tmp_path_factory, "tiny-g64", 91)
    embed_raw(q3, m, m.by_len(410, (50, 9)), 2, "tiny-g64", cap=32)


@pytest.mark.parametrize("name,lens", [("small-hd128", (40, 3)), ("tiny-g64", (50, 9))])
def test_against_the_cpu_oracle(q3, oracle, tmp_path_factory, name, lens):
    m = narrow_model(q3, tmp_path_factory, name, 92)
    prompts = [m.prompt(420 + i, n) for i, n in enumerate(lens)]
    om = oracle.OracleModel(m.path, m.ctx)
    want = []
    for p in prompts:
        om.reset()
        for pos, tok in enumerate(p):
            om.forward(tok, pos)
        want.append(om.tap_x())
    with m.engine() as t:
        t.batch_init(2)
        rows, _ = t.embed_many(prompts, normalize=False)
        for i in range(len(prompts)):
            assert_biteq(rows[i], want[i], f"{name}: request {i} against the oracle")
        unit, _ = t.embed_many(prompts)
        assert_biteq(unit, embed_ref.l2(np.stack(want)), f"{name}: normalised rows against the oracle")


def test_the_4b_width(q3, models):
    """dim 2560 (40-term blocks of the exact sum), four query heads per kv head"""
    m = models("qwen3-4b-dims-l2")
    rows = embed_raw(q3, m, m.by_len(500, (35, 8, 64)), 3, "4b dims")
    assert rows.shape[1] == 2560


def test_an_edge_valued_checkpoint(q3, models):
    m = models(NAME, "all")
    embed_raw(q3, m, m.by_len(510, (41, 9)), 2, "edge values")


def test_l2_and_truncation(q3, models):
    m = models()
    refs = m.by_len(600, (41, 9, 3))
    prompts = [r["prompt"] for r in refs]
    with m.engine() as t:
        t.batch_init(4)
        raw, _ = t.embed_many(prompts, normalize=False)
        assert_biteq(raw, np.stack([r["x"] for r in refs]), "flags 0")
        for od in (1, 30, 64, 1000, 1024):
            got, _ = t.embed_many(prompts, normalize=True, out_dim=od)
            assert got.shape == (3, od)
            assert_biteq(got, embed_ref.l2(raw, od), f"L2 over the first {od}")
            cut, _ = t.embed_many(prompts, normalize=False, out_dim=od)
            assert_biteq(cut, raw[:, :od], f"the first {od}, not normalised")
        full, _ = t.embed_many(prompts)
        assert full.shape == (3, 1024)
        assert_biteq(full, embed_ref.l2(raw), "out_dim None is dim")


def test_behind_the_resident_prefix(q3, models):
    m = models()
    prefix = m.prompt(700, 37)
    suffixes = [m.prompt(701 + i, n) for i, n in enumerate((1, 20, 60))]
    full = [prefix + s for s in suffixes]
    refs = m.refs(full)
    with m.engine() as t:
        t.batch_init(4)
        t.batch_prefix_set(prefix)
        rows, st = t.embed_many(suffixes, normalize=False, use_prefix=True)
        for i, r in enumerate(refs):
            assert_biteq(rows[i], r["x"], f"suffix {i} behind the prefix")
        assert st == pack_sum(q3, [1, 20, 60], 4) and st.live_columns == 81
        assert t.batch_prefix_get() == prefix
        for i, r in enumerate(refs):
            check_rows(t, i, r, len(full[i]), f"slot {i}: prefix and suffix rows")
        plain, _ = t.embed_many(full, normalize=False)
        assert_biteq(plain, rows, "the full prompts without a prefix")
        assert_biteq(q3.embed(t, full, normalize=False, shared_prefix=True), rows, "generation.embed, shared_prefix=True")
        assert t.batch_prefix_get() == prefix
        assert_biteq(q3.embed(t, suffixes, shared_prefix=prefix, out_dim=64), embed_ref.l2(rows, 64), "generation.embed, a token list")
        assert_biteq(q3.embed(t, full, normalize=False), rows, "generation.embed, no prefix")


def test_nothing_else_moved(q3, models):
    """generate_many, greedy and sampled, gives the same rows behind an embed_many call; a draw under set_batch_sampler is the same
    draw: no slot rng was advanced"""
    m = models()
    prompts = [m.prompt(800 + i, n) for i, n in enumerate((12, 40, 3, 70, 9))]
    seeds = [21, 22, 23, 24, 25]
    T, P = 0.7, 0.9

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
    with m.engine() as t:
        t.batch_init(3)
        t.embed_many(prompts)
        t.embed_many(prompts[:2], normalize=False, out_dim=8)
        assert rest(t) == (greedy, sampled)
        rows, _ = t.embed_many(prompts, normalize=False)          # under a sampling batch: the references' rows, and no coin drawn
        for i, r in enumerate(m.refs(prompts)):
            assert_biteq(rows[i], r["x"], f"request {i} under a sampling batch")
        assert draw(t) == draws


def test_errors_leave_the_engine_usable(q3, models, tmp_path_factory):
    import ctypes as C
    m = models()
    refs = m.by_len(900, (41, 6))
    p = refs[0]["prompt"]
    V, dim = m.shape.vocab_size, m.shape.dim
    with m.engine() as t:
        with pytest.raises(IndexError):
            t.embed_many([p])                                                    # no batch_init
        t.batch_init(2)
        for prompts, kw in (([], {}), ([p, []], {}), ([p[:5] + [V]], {}), ([[-1] + p], {}), ([m.prompt(901, CTX + 1)], {}),
                            ([p], dict(out_dim=dim + 1)), ([p], dict(use_prefix=True))):
            with pytest.raises(IndexError):
                t.embed_many(prompts, **kw)
        lens, toks, out = (C.c_size_t * 1)(len(p)), (C.c_int32 * len(p))(*p), (C.c_float * dim)()
        for args in ((toks, lens, 1, 4, 0, out), (toks, lens, 1, 0x80000001, 0, out), (None, lens, 1, 0, 0, out), (toks, None, 1, 0, 0, out),
                     (toks, lens, 1, 0, 0, None), (toks, lens, 0, 0, 0, out)):
            assert t._lib.q3_embed_many(t._h, *args, None) == -3, args[2:5]
        t.batch_prefix_set(p[:37])
        with pytest.raises(IndexError):
            t.embed_many([m.prompt(902, CTX - 37 + 1)], use_prefix=True)         # P + prompt_len > the batch context
        t.batch_prefix_set([])
        rows, _ = t.embed_many([r["prompt"] for r in refs], normalize=False)
        for i, r in enumerate(refs):
            assert_biteq(rows[i], r["x"], f"request {i} behind the refused calls")
    with m.engine(fast=True) as t:
        t.batch_init(2)
        with pytest.raises(q3.Q3Error) as ei:
            t.embed_many([p])
        assert ei.value.code == -5 and "Q3_FLAG_FAST" in ei.value.msg
    # 8 query heads per kv head: the shape q3_batch_step_cols refuses
    ck = q3.checkpoint
    path = str(tmp_path_factory.mktemp("embed_kvmul8") / "kvmul8.bin")
    ck.write_synthetic_checkpoint(path, ck.ModelShape(256, 384, 2, 8, 1, 512, 96, 64, True, 64), seed=5)
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(2)
        with pytest.raises(q3.Q3Error) as ei:
            t.embed_many([[1, 2, 3]])
        assert ei.value.code == -5 and "per-kv-head attention kernel" in ei.value.msg
        assert t.forward_argmax(1, 0) >= 0                                       # the engine goes on


def test_the_command_line(q3, tmp_path, capsys):
    from qwen3_rs_amd import cli
    from qwen3_rs_amd import tokenizer as tk
    from test_tokenizer_cli import make_tokenizer_json
    ck = q3.checkpoint
    d = str(tmp_path)
    n_vocab = make_tokenizer_json(d)
    shape = ck.ModelShape(256, 384, 2, 4, 2, n_vocab + (16 - n_vocab % 16) % 16, 96, 64, True, 64)
    path = os.path.join(d, "model.bin")
    ck.write_synthetic_checkpoint(path, shape, seed=12)
    tk.export_tokenizer(d, path, 1, 2)
    tok = tk.Tokenizer(path, shape.vocab_size)
    texts, instruct, out = ["hello world", "world hello hello"], "hell: ", os.path.join(d, "out.npy")
    assert cli.main(["embed", path, "-i", texts[0], "-i", texts[1], "--instruct", instruct, "--dim", "32", "--append-token", "2", "-o", out,
                     "--streams", "2"]) == 0
    got = np.load(out)
    lines = capsys.readouterr().out.strip().splitlines()
    with q3.TransformerBuilder(path).build() as t:
        t.batch_init(2)
        want = q3.embed(t, [tok.encode(x) + [2] for x in texts], out_dim=32, shared_prefix=tok.encode(instruct))
    assert_biteq(got, want, "the saved matrix")
    assert got.shape == (2, 32) and len(lines) == 2
    for r, line in enumerate(lines):
        f = line.split()
        assert (int(f[0]), int(f[1]), len(f)) == (r, 32, 10) and [float(v) for v in f[2:]] == [float(f"{v:.6f}") for v in want[r, :8]]
