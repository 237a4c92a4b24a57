"""Call sequences over the batched state (helper module of tests/test_call_sequences_host.py and tests/test_call_sequences.py, not a
conftest).  One BatchCtx serves every entry point of include/qwen3_hip.h sections 2b to 2l, and its plans, graphs and grow-only buffers
are shared or cached between them; this module generates seeded sequences of calls, knows from the C oracle alone what every call
must return, and checks an engine op by op.

    make_sequence(seed, n_ops)  a deterministic list of ops (plain dicts, printable as a literal)
    Reference                   the oracle side: cache rows, logits and final-norm taps of any token sequence, memoised in a trie,
                                and the request rule of the header ("row r is what a fresh engine gives after prefill + generate_greedy")
    FakeEngine                  the Transformer surface answered from Reference with explicit Python state; a switch injects a leak
    run(engine, ops, reference) executes the ops, checks outputs, untouched caches and filled rows after every op
    make_settings_sequence(seed) the settings dimension: SETTING_KINDS -- the engine-wide settings of sections 2m to 2q (top_k,
                                gen_logprobs, penalties, the logit-bias table), q3_gen_logprobs_read and q3_score_top_many -- among the
                                kinds of the pair matrix; Tables derives every table from Reference alone; run() reads the records
                                behind every loop op and the four getters behind every op
    make_guide_sequence(seed)   the guide dimension: GUIDE_KINDS -- the dense guide of section 2r, the sparse guide of 2s, the stop
                                automaton of 2t, their refusals -- among the kinds above; Tables derives every automaton from Reference
                                alone; run() holds tokens, n_out, the -1 fill, stats and records to the reference under them and reads
                                the three getters behind every op

Shape: small-hd128 (dim 512, 8 heads over 4 kv heads, head_dim 128, group 64, vocabulary 2,048) with 576 positions declared instead
of 256: the score rows of the dense blocks (att_pf) are sized to the context end rounded up to 256, so on 256 positions they are
allocated once and can never grow.  record_exps of q3_score_many is sized by the vocabulary alone (32 rows of it), so within an engine
it is allocated once and can never grow: it is not among BUFFERS."""
import dataclasses
import functools
import random

import numpy as np

VOCAB, SEQ, DIM = 2048, 576, 512
NAME = "small-hd128"
DENSE_CAP = 2048                      # Q3_PREFILL_M as the tests leave it
COLS_MAX = 32
WIDTHS = (1, 2, 4, 8, 16, 32)
SETTING_BUFFERS = ("genlp_recs", "genlp_top", "genlp_rank", "bias_entries", "bias_off", "bias_ooff", "score_top", "score_rank")
BUFFERS = ("cols_table", "cols_ncols", "cols_prompts", "cols_out", "cols_aux", "cols_temp", "cols_topp", "cols_seeds", "cols_req",
           "dense_runs", "embed_rows", "embed_out", "att_pf", "score_rows", "score_out", "choice_cand", "choice_out")
SCORE_COLS = 32                       # kScoreCols: the scored columns of a block go through the classifier that many at a time
CHOICE_PART = 32                      # kChoicePart: the candidates of one workgroup


def shape(q3):
    return dataclasses.replace(q3.checkpoint.SHAPES[NAME], max_seq_len=SEQ)


def _q3():
    import qwen3_rs_amd          # host-only functions: cols_schedule, cols_schedule_stop, dense_pack
    return qwen3_rs_amd


# ---------------------------------------------------------------------------------------------------------------------------------
# tokens: every prompt is a slice of one of a few fixed base sequences, so that the oracle's rows are shared by all ops and seeds.
# The bases repeat themselves with a short period: the prompt-lookup drafter finds drafts in them.
# ---------------------------------------------------------------------------------------------------------------------------------
N_BASES, BASE_LEN = 6, 560


def _make_bases():
    rng = np.random.default_rng(20240)
    out = []
    for k in range(N_BASES):
        t = [int(v) for v in rng.integers(0, VOCAB, BASE_LEN)]
        for i in range(5 + k, BASE_LEN):
            if rng.random() < 0.6:
                t[i] = t[i - 5 - k]
        out.append(tuple(t))
    return out


BASES = _make_bases()


def toks(spec):
    """(base, end) or (base, start, end) -> the tokens"""
    k, a, b = (spec[0], 0, spec[1]) if len(spec) == 2 else spec
    return list(BASES[k][a:b])


# request templates: (base, prompt length, n_new, temperature, top-p, seed).  0 .. 11 small (2-10 tokens), 12 .. 17 medium (past 32
# columns and past every dense_min in use), 18 .. 87 the large lists (3 .. 120 tokens, most of them dense)
def _make_catalogue():
    rng = random.Random(77)
    temps, topps = (0.0, 0.7, 0.9, 1.1), (0.9, 0.95, 1.0, 0.0)
    cat = []
    for i in range(88):
        if i < 12:
            n = 2 + i % 9
        elif i < 18:
            n = 34 + 5 * (i - 12)
        else:
            n = rng.choice((3, 9, 20, 33, 35, 41, 48, 57, 64, 65, 70, 83, 97, 110, 120))
        cat.append((i % N_BASES, n, 1 + rng.randrange(4), temps[(i // 2) % 4], topps[i % 4], 1000 + i))
    for i in range(88, 91):                     # 88 .. 90: one token, for the calls that generate nothing (a score request without a record)
        cat.append((i % N_BASES, 1, 1, 0.0, 1.0, 1000 + i))
    return cat


def _extend_catalogue(cat):
    """91 .. 114, behind the 91 entries of the pair matrix so that their indices keep their meaning: the requests of the settings
    sequences, 6 to 12 new tokens behind prompts of 2 to 40 -- long enough for a produced token to come again (a count of 2 under the
    penalties) and for an allowed list of three tokens to force one"""
    rng = random.Random(78)
    temps, topps = (0.0, 0.7, 0.9, 1.1), (0.9, 0.95, 1.0, 0.0)
    for i in range(91, 115):
        n = (2, 40, 7, 33)[i - 91] if i < 95 else rng.randint(2, 40)
        cat.append((i % N_BASES, n, rng.randint(6, 12), temps[(i // 2) % 4], topps[i % 4], 1000 + i))
    return cat


CAT = _extend_catalogue(_make_catalogue())
SMALL, MEDIUM, LARGE, ONE, LONG = range(0, 12), range(12, 18), range(18, 88), range(88, 91), range(91, 115)
PREFIXES = ((5, 7), (4, 37), (3, 44))          # resident prefixes: base, length (one narrow, two wide)
DEEP = {1: (2, 300), 2: (2, 530)}              # the runs that end past 256 and past 512 positions


def xorshift(state, coins=1):
    """sampler.rs:44-49: the rng state `coins` coins on"""
    for _ in range(coins):
        state ^= state >> 12
        state = (state ^ (state << 25)) & 0xFFFFFFFFFFFFFFFF
        state ^= state >> 27
    return state


# ---------------------------------------------------------------------------------------------------------------------------------
# op kinds
# ---------------------------------------------------------------------------------------------------------------------------------
KINDS = (
    "forward_batch", "forward_batch_s", "generate_greedy_batch", "generate_greedy_batch_s", "prefill_batched",
    "verify", "generate_lookup", "verify_draw", "generate_lookup_draw",
    "batch_step_cols", "generate_many_greedy", "batch_step_cols_draw", "generate_many_sampled",
    "batch_prefill_slots", "generate_many_dense", "generate_many_stop",
    "batch_copy_rows", "batch_prefix_set", "generate_many_prefix", "embed_many", "embed_many_prefix",
    "choice_many", "choice_many_prefix", "score_many", "score_many_prefix",
    "set_batch_sampler_on", "set_batch_sampler_off", "set_sampler", "batch_reset_kv", "reset_kv", "batch_init",
    "forward", "generate_greedy",
    "refused_batch", "refused_prefill_batched", "refused_verify", "refused_cols", "refused_dense", "refused_stop", "refused_prefix",
    "refused_embed", "refused_choice", "refused_score", "refused_forward", "refused_greedy_only",
)
GREEDY_ONLY = ("forward_batch", "generate_greedy_batch", "batch_step_cols", "generate_many_greedy")     # refused under a sampling batch
NEED_DRAWS = ("forward_batch_s", "generate_greedy_batch_s")                                              # need known per-stream rng states
SAMPLING_ONLY = NEED_DRAWS + ("refused_greedy_only",)
MANY = ("generate_many_greedy", "generate_many_sampled", "generate_many_dense", "generate_many_stop", "generate_many_prefix")
CHOICE, SCORE = ("choice_many", "choice_many_prefix"), ("score_many", "score_many_prefix")
# the calls that run q3_embed_many's walk and generate nothing: legal under a sampling batch, and they draw no coin, so the per-stream
# rng states stay what they were (a NEED_DRAWS op right behind them draws the coins the seeds give)
WALKS = ("embed_many", "embed_many_prefix") + CHOICE + SCORE
NEED_PREFIX = ("generate_many_prefix", "embed_many_prefix", "choice_many_prefix", "score_many_prefix")

# ordered pairs the API makes illegal, one line of reason each
ILLEGAL = {}
for _a in GREEDY_ONLY:
    for _b in SAMPLING_ONLY:
        ILLEGAL[(_a, _b)] = "the first needs the batch sampler off, the second on, and neither changes it"
        ILLEGAL[(_b, _a)] = "the first needs the batch sampler on, the second off, and neither changes it"
    ILLEGAL[("set_batch_sampler_on", _a)] = "greedy only: refused (-5) right behind a batch sampler with temperature > 0"
for _b in SAMPLING_ONLY:
    ILLEGAL[("set_batch_sampler_off", _b)] = "needs a sampling batch, which the call in front has just switched off"
    ILLEGAL[("batch_init", _b)] = "q3_batch_init starts the batched state over: no batch sampler is set"
for _a in ("generate_many_sampled", "generate_many_dense", "generate_many_stop", "generate_many_prefix"):
    for _b in NEED_DRAWS:
        ILLEGAL[(_a, _b)] = ("the per-stream sampler states are unspecified behind a sampled loop (and behind a greedy one the batch "
                             "sampler is off): q3_batch_sampler_set has to come first")
for _b in NEED_PREFIX:
    ILLEGAL[("batch_init", _b)] = "q3_batch_init drops the resident prefix"
for _a in ("batch_init", "batch_reset_kv"):
    ILLEGAL[(_a, "batch_copy_rows")] = "legal in the API, but the sequences copy only rows whose tokens they know: every slot has just been cleared"
ALL_PAIRS = [(a, b) for a in KINDS for b in KINDS]


def pairs_of(ops):
    return {(a["op"], b["op"]) for a, b in zip(ops, ops[1:])}


# ---------------------------------------------------------------------------------------------------------------------------------
# schedules of the loops, from the library's host-only functions
# ---------------------------------------------------------------------------------------------------------------------------------
def dense_block(lens):
    """one pack of runs (always a single block here) -> (width, wide)"""
    _, st = _q3().dense_pack(list(lens), DENSE_CAP)
    assert st.blocks == 1, lens
    w = st.live_columns + st.pad_columns
    return w, w > COLS_MAX


def width_index(n):
    return next(i for i, w in enumerate(WIDTHS) if w >= n)


def _pass_sizes(table):
    sizes = {}
    for p, _, _, _ in table:
        sizes[p] = sizes.get(p, 0) + 1
    return [sizes[p] for p in sorted(sizes)]


def many_plan(lens, n_new, streams, dense_min=0, rows=None, stop=(), emit=None):
    """What a generate_many call does with requests of lens[r] prompt tokens: dict(table, stats, n_out, occupants = per slot the
    requests it held in order, passes = live columns per column pass, blocks = [(width, wide, run lengths)] of the dense requests
    in order).  emit: the n_emit of the stop loop under a stop automaton (section 2t) -- its passes and stats are those of
    q3_cols_schedule(prompt_len, n_emit)."""
    q3 = _q3()
    dense = [bool(dense_min) and n - 1 >= dense_min for n in lens]
    seen = [1 if d else n for n, d in zip(lens, dense)]
    if emit is not None:
        table, stats = q3.cols_schedule(seen, list(emit), streams)
        n_out = list(emit)
    elif stop:
        table, n_out, stats = q3.cols_schedule_stop(seen, list(n_new), streams, rows, list(stop))
    else:
        table, stats = q3.cols_schedule(seen, list(n_new), streams)
        n_out = list(n_new)
    occupants = {}
    first_pass = {}
    for p, s, _, r in table:
        if r not in first_pass:
            first_pass[r] = p
            occupants.setdefault(s, []).append(r)
    blocks = []
    for p in sorted(set(first_pass.values())):
        entering = sorted(r for r, fp in first_pass.items() if fp == p and dense[r])
        if entering:
            run_lens = [lens[r] - 1 for r in entering]
            blocks.append(dense_block(run_lens) + (run_lens,))
    return dict(table=table, stats=stats, n_out=n_out, occupants=occupants, passes=_pass_sizes(table), blocks=blocks)


def op_requests(op):
    """(prompt lengths, n_new) of a generate_many / embed op"""
    return [CAT[i][1] for i in op["reqs"]], [CAT[i][2] for i in op["reqs"]]


def candidates(op):
    """The candidate ids of a choice op, from its "cand" = (k, per request, seed): one list of k ids, or one per request.  Seeded draws
    from the vocabulary that hold 0, VOCAB - 1 and a duplicate as far as k has room for them (k = 1: one of the two edges or a draw;
    k = 2: the two edges)."""
    k, per_request, seed = op["cand"]
    r = random.Random(seed)

    def one():
        if k == 1:
            return [r.choice((0, VOCAB - 1, r.randrange(VOCAB)))]
        ids = [r.randrange(VOCAB) for _ in range(max(0, k - 3))]
        ids += [0, VOCAB - 1] + ([r.choice(ids)] if ids else [])
        r.shuffle(ids)
        return ids[:k]
    return [one() for _ in op["reqs"]] if per_request else one()


def flat_candidates(op):
    c = candidates(op)
    return [t for row in c for t in row] if op["cand"][1] else c


def score_blocks(op, streams):
    """The blocks of a score op, one per wave (dense_block asserts it): [(width, wide, scored columns in column order)].  The runs of a
    narrow block stand side by side from column 0, those of a wide one at multiples of 8."""
    lens, _ = op_requests(op)
    sf = op["score_from"] or [1] * len(lens)
    out = []
    for w0 in range(0, len(lens), streams):
        wave, first = lens[w0:w0 + streams], sf[w0:w0 + streams]
        w, wide = dense_block(wave)
        cols, at = [], 0
        for n, f in zip(wave, first):
            cols += [at + i for i in range(n) if i + 1 < n and i + 1 >= f]
            at += (n + 7) & ~7 if wide else n
        out.append((w, wide, cols))
    return out


def score_chunks(op, streams):
    """[(scored columns of the chunk, the classifier runs on them where they stand: no gather)] of a score op"""
    out = []
    for _, wide, cols in score_blocks(op, streams):
        for c0 in range(0, len(cols), SCORE_COLS):
            part = cols[c0:c0 + SCORE_COLS]
            out.append((len(part), not wide and part == list(range(len(part)))))
    return out


def form_of(draw, st):
    """(draw, topk, genlp, pen) of the column plans a loop op runs under the settings st: the plan key's four axes.  topk is on a
    sampled plan alone (plan_get clears it on a greedy one); genlp 0 off, 1 records, 2 records + top; pen 0 off, 1 penalties, 2 the
    adjusted form, which a table selects with or without penalties, 3 the masked form of a dense guide and 4 that of a sparse one,
    which a guide selects whatever the table and the penalties (st["gform"], where the walk tracks it)"""
    pen = {"dense": 3, "sparse": 4}.get(st.get("gform"), 2 if st["table"] is not None else 1 if any(st["pen"]) else 0)
    return (bool(draw), bool(draw and st["top_k"]), 0 if st["genlp"] < 0 else 1 if st["genlp"] == 0 else 2, pen)


def needs(op, streams, sampling, prefix_len, rows=None, stop=(), st=None, table=None):
    """What an op asks of the grow-only buffers, by the sizes at the call sites of cols_job_run, cols_generate_stop, cols_sampler_upload,
    q3_embed_many, q3_choice_many and q3_score_many, and which kept plans it runs: dict(buffer -> elements), cols = {(draw, width
    index)}, dense = {block width}; for a score op also chunk_cols, the column plans that only its classifier chunks run (not its walk).
    st: the settings in force (settings_walk) and table: the set_logit_bias op whose table holds -- then also the per-call buffers of
    genlp_call_begin and bias_call_begin, the tops and ranks of q3_score_top_many, and forms = {(draw, topk, genlp, pen, width index)},
    the column plans of a loop op by their whole key."""
    kind = op["op"]
    top_k = op["k"] if kind.startswith("score_top_many") else 0
    if top_k:
        kind = "score_many" + kind[len("score_top_many"):]
    need, cols, dense = {}, set(), set()

    def job(n_passes, n_prompt, n_out, n_runs, draw, per_request, max_end):
        need.update(cols_table=n_passes * COLS_MAX, cols_ncols=n_passes, cols_prompts=n_prompt, cols_out=n_out, dense_runs=n_runs)
        if draw and n_passes:
            need["cols_aux"] = n_passes * COLS_MAX
            if per_request:
                need.update(cols_temp=per_request, cols_topp=per_request, cols_seeds=per_request)
        if max_end:
            need["att_pf"] = (max_end + 255) & ~255

    if kind in MANY:
        lens, n_new = op_requests(op)
        draw = kind == "generate_many_sampled" or bool(op.get("sampled"))
        if kind == "generate_many_stop" or (kind == "generate_many_prefix" and stop):
            plan = many_plan(lens, n_new, streams, 0, rows, stop)
            need.update(cols_req=5 * len(lens), cols_prompts=sum(lens), cols_out=sum(n_new))
            if draw:
                need.update(cols_temp=len(lens), cols_topp=len(lens), cols_seeds=len(lens))
        else:
            plan = many_plan(lens, n_new, streams, op.get("dense_min", 0))
            narrow = [b for b in plan["blocks"] if not b[1]]
            wide = [b for b in plan["blocks"] if b[1]]
            job(len(plan["passes"]) + len(narrow), sum(lens), sum(n_new), sum(len(b[2]) for b in wide), draw, len(lens),
                max([max(b[2]) for b in wide], default=0))
            cols |= {(draw, width_index(sum(b[2]))) for b in narrow}
            dense |= {b[0] for b in wide}
        cols |= {(draw, width_index(n)) for n in plan["passes"]}
        if st is not None:
            if st["genlp"] >= 0:
                need["genlp_recs"] = sum(n_new)
                if st["genlp"] > 0:
                    need.update(genlp_top=sum(n_new) * st["genlp"], genlp_rank=sum(n_new))
            if table is not None:
                n_ent = table_lens(table)[0]
                need.update(bias_entries=sum(n_ent), bias_off=len(n_ent) + 1, bias_ooff=len(lens) + 1)
            return dict(need=need, cols=cols, dense=dense, forms={form_of(d, st) + (w,) for d, w in cols})
    elif kind in ("batch_prefill_slots", "batch_prefix_set"):
        runs = [(0, len(toks(op["prompt"])))] if kind == "batch_prefix_set" else [(f, len(toks(p))) for p, f in zip(op["prompts"], op["first"])]
        draw = sampling and kind == "batch_prefill_slots"
        w, wide = dense_block([n for _, n in runs])
        n_tok = sum(n for _, n in runs)
        if wide:
            job(0, n_tok, 0, len(runs), draw, 0, max(f + n for f, n in runs))
            dense.add(w)
        else:
            job(1, n_tok, 0, 0, draw, 0, 0)
            cols.add((draw, width_index(n_tok)))
    elif kind in WALKS:
        lens, _ = op_requests(op)
        P = prefix_len if kind.endswith("_prefix") else 0
        max_end = 0
        for w0 in range(0, len(lens), streams):
            wave = lens[w0:w0 + streams]
            w, wide = dense_block(wave)
            if wide:
                dense.add(w)
                max_end = max(max_end, P + max(wave))
            else:
                cols.add((False, width_index(sum(wave))))
        need.update(cols_prompts=sum(lens), dense_runs=len(lens), embed_rows=len(lens))
        if kind in CHOICE:
            k, per_request, _ = op["cand"]
            need.update(choice_cand=k * len(lens) if per_request else k, choice_out=k * len(lens))
        elif kind in SCORE:
            # every chunk runs the classifier part of the kept non-draw column plan of its width, behind wide blocks as well
            chunks = {(False, width_index(m)) for m, _ in score_chunks(op, streams)}
            first_use = chunks - cols
            cols |= chunks
            n_rec = sum(n - f for n, f in zip(lens, op["score_from"] or [1] * len(lens)))
            need.update(score_rows=n_rec, score_out=n_rec)
            if top_k:
                need.update(score_top=n_rec * top_k, score_rank=n_rec)
        else:
            need["embed_out"] = len(lens) * (op.get("out_dim") or DIM)
        if max_end:
            need["att_pf"] = (max_end + 255) & ~255
        if kind in SCORE:
            return dict(need=need, cols=cols, dense=dense, chunk_cols=first_use)
    elif kind in ("batch_step_cols", "batch_step_cols_draw"):
        cols.add((sampling and kind == "batch_step_cols_draw", width_index(len(op["slots"]))))
    return dict(need=need, cols=cols, dense=dense)


# ---------------------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------------------
SEEDS = (11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22)
N_OPS = 220
EDGE_SEED = SEEDS[3]                  # the seed that also runs on the edge-valued checkpoint: it holds the four choice and score kinds


class _Gen:
    """State the generator tracks: for the single cache and every slot the base prefix its rows are known to hold, the two samplers,
    the resident prefix, the batch shape."""

    def __init__(self, seed, avoid):
        self.rng = random.Random(seed)
        self.avoid = avoid                   # pairs other sequences cover already
        self.ops = []
        self.single = None                   # (base, n): rows 0 .. n - 1 hold that prefix
        self.slots = []
        self.streams = self.ctx = 0
        self.bs_on = self.bs_known = False
        self.ss_on = False
        self.prefix = None
        self.size = "S"
        self.large_calls = 0
        self.grown = set()                   # the choice kinds of a large phase that have made their growing call
        self.turned_off = set()              # the ops that switch off a batch sampler that was on
        self.growth = False                 # inside the epoch whose buffers have to grow: no q3_batch_init

    # -- legality
    def legal(self, kind):
        if kind in GREEDY_ONLY and self.bs_on:
            return False
        if kind in NEED_DRAWS and not (self.bs_on and self.bs_known):
            return False
        if kind == "refused_greedy_only" and not self.bs_on:
            return False
        if kind == "batch_step_cols_draw" and self.bs_on and not self.bs_known:
            return False
        if kind in NEED_PREFIX and self.prefix is None:
            return False
        if kind == "batch_copy_rows" and not (self.streams >= 2 and any(s for s in self.slots)):
            return False
        if kind in ("verify", "generate_lookup") and self.ss_on:
            return False
        if kind == "batch_init" and self.growth:
            return False
        return True

    # -- helpers
    def _place(self, held, room, m=1):
        """continue a cache that holds (base, n) by m tokens, or start a base over: (base, first position)"""
        if held and held[1] + m + 8 <= room and self.rng.random() < 0.6:
            return held[0], held[1]
        return self.rng.randrange(N_BASES), 0

    def _reqs(self, dense=False, one=False):
        r = self.rng
        if self.size == "S":
            out = r.sample(SMALL, r.randint(1, 3))
            if dense or r.random() < 0.3:
                out[r.randrange(len(out))] = r.choice(MEDIUM)
            if one and len(out) > 1 and r.random() < 0.3:      # a one-token request: no record, nothing in front of its last token
                out[r.randrange(len(out))] = r.choice(ONE)
            return out
        self.large_calls += 1                                  # every large list is longer than the one before it
        n = min(38, 18 + 2 * self.large_calls) if self.size == "L1" else min(70, 50 + 2 * self.large_calls)
        return list(LARGE[:n])

    def _score_from(self, reqs):
        r = self.rng
        lens = [CAT[i][1] for i in reqs]
        if self.size == "S":
            mode = r.randrange(4)
            if mode == 0:
                return None
            if mode == 1:                                      # the first request alone: its scored columns are the block's first (no gather)
                sf = [1] + lens[1:]
            else:
                sf = [r.choice((1, n, max(1, n - 1), r.randint(1, n))) for n in lens]
            if self.growth and sf == lens:                     # where the buffers have to grow, the small calls have a record too
                sf[max(range(len(lens)), key=lens.__getitem__)] = 1
            return sf
        # a large list: the first wide blocks that can hold them score 31, 32 and 33 columns, the others all they have (more than 64)
        sf, targets = [1] * len(lens), [31, 32, 33]
        for w0 in range(0, len(lens), self.streams):
            wave = lens[w0:w0 + self.streams]
            if targets and dense_block(wave)[1] and sum(n - 1 for n in wave) >= targets[0]:
                left = targets.pop(0)
                order = list(range(len(wave)))
                r.shuffle(order)
                for j in order:
                    take = min(wave[j] - 1, left)
                    left -= take
                    sf[w0 + j] = wave[j] - take
        return sf

    # -- one emitter per kind
    def emit(self, kind, **force):
        r = self.rng
        op = {"op": kind}
        S, ctx = self.streams, self.ctx
        if kind in ("forward_batch", "forward_batch_s", "generate_greedy_batch", "generate_greedy_batch_s", "refused_batch"):
            n = r.randint(1, S)
            steps = r.randint(1, 4) if "generate" in kind else 1
            tk, ps = [], []
            for i in range(n):
                k, p = self._place(self.slots[i], ctx, steps)
                tk.append(BASES[k][p])
                ps.append(p)
                if kind != "refused_batch":
                    self.slots[i] = (k, p + 1)
            if kind == "refused_batch":
                tk[r.randrange(n)] = VOCAB
            if "generate" in kind:
                op.update(first=tk, pos=ps, steps=steps)
            else:
                op.update(tokens=tk, pos=ps)
        elif kind in ("prefill_batched", "refused_prefill_batched"):
            m = r.choice((2, 5, 9, 33, 40, 47)) if self.size == "S" else r.choice((70, 100, 120))
            k, p = self._place(self.single, SEQ, m)
            if kind == "refused_prefill_batched":
                op.update(prompt=(k, 0, m), pos=SEQ - m + 1)
            else:
                op.update(prompt=(k, p, p + m), pos=p)
                self.single = (k, p + m)
        elif kind in ("verify", "verify_draw", "refused_verify"):
            n = r.randint(1, 9)
            k, p = self._place(self.single, SEQ, n)
            t = list(BASES[k][p:p + n])
            if n > 2 and r.random() < 0.5:
                t[r.randrange(1, n)] = r.randrange(VOCAB)      # a draft the model need not even see: rejected unless drawn
            if kind == "refused_verify":
                t[-1] = VOCAB
                op.update(tokens=t, pos=p, draw=self.ss_on)
            else:
                op.update(tokens=t, pos=p)
                self.single = (k, p + 1)
        elif kind in ("generate_lookup", "generate_lookup_draw", "generate_greedy"):
            n = r.randint(1, 6)
            k, p = self._place(self.single, SEQ, n)
            op.update(first=BASES[k][p], pos=p, n=n)
            if kind != "generate_greedy":
                op.update(corpus=(k, 0, max(p, 12)), ngram=r.choice((1, 2)), draft_len=r.choice((0, 3, 7)))
            self.single = (k, p + 1)
        elif kind in ("forward", "refused_forward"):
            k, p = self._place(self.single, SEQ)
            if kind == "refused_forward":
                op.update(token=BASES[k][p], pos=SEQ)
            else:
                op.update(token=BASES[k][p], pos=p)
                self.single = (k, p + 1)
        elif kind in ("batch_step_cols", "batch_step_cols_draw", "refused_cols", "refused_greedy_only"):
            slots = r.sample(range(S), 1 if force.get("one") else r.randint(1, min(S, 3)))
            left = COLS_MAX
            sl, tk, ps = [], [], []
            for j, s in enumerate(slots):
                m = r.randint(1, min(left - (len(slots) - 1 - j), 1 if force.get("one") else r.choice((1, 3, 12))))
                left -= m
                k, p = self._place(self.slots[s], ctx, m)
                sl += [s] * m
                tk += list(BASES[k][p:p + m])
                ps += list(range(p, p + m))
                if not kind.startswith("refused"):
                    self.slots[s] = (k, p + m)
            if kind == "refused_cols":
                sl[-1] = S
                op["draw"] = self.bs_on
            op.update(slots=sl, tokens=tk, pos=ps)
            if kind == "batch_step_cols_draw" and r.random() < 0.4:
                op["keep"] = [int(j + 1 == len(sl) or sl[j + 1] != sl[j] or r.random() < 0.5) for j in range(len(sl))]
        elif kind in MANY or kind == "refused_stop":
            op["reqs"] = self._reqs(dense=kind == "generate_many_dense")
            if kind == "generate_many_dense":
                op.update(sampled=self.bs_on or r.random() < 0.5, dense_min=r.choice((8, 32, 64)))
            elif kind in ("generate_many_stop", "generate_many_prefix", "refused_stop"):
                op["sampled"] = self.bs_on or r.random() < 0.5
                cand = [(i, j) for i in op["reqs"] for j in range(CAT[i][2])]
                k = 0 if kind == "generate_many_prefix" and r.random() < 0.5 else min(len(cand), r.randint(1, 4))
                op["stop_at"] = r.sample(cand, k)              # (request, index): that token of the request's own row is a stop token
            if kind == "refused_stop":
                op["bad"] = r.randrange(len(op["reqs"]))       # that request's prompt ends with a token outside the vocabulary
            else:
                used = min(len(op["reqs"]), S)
                self.slots[:used] = [None] * used
                if kind == "generate_many_sampled" or op.get("sampled"):
                    self.bs_known = False
        elif kind in ("batch_prefill_slots", "refused_dense"):
            if force.get("wide"):                              # one run of 41 tokens: a block of 48 columns
                op.update(slots=[0], prompts=[(1, 0, 41)], first=[0])
                self.slots[0] = (1, 41)
            elif self.size != "S" and kind == "batch_prefill_slots":
                s = r.randrange(S)
                op.update(slots=[s], prompts=[DEEP[int(self.size[1])]], first=[0])
                self.slots[s] = DEEP[int(self.size[1])]
            else:
                slots = r.sample(range(S), r.randint(1, min(S, 3)))
                prompts, first = [], []
                for s in slots:
                    m = r.choice((3, 8, 20, 34, 41, 60))
                    k, p = self._place(self.slots[s], ctx, m)
                    prompts.append((k, p, p + m))
                    first.append(p)
                    if kind == "batch_prefill_slots":
                        self.slots[s] = (k, p + m)
                if kind == "refused_dense":
                    slots[-1] = S
                op.update(slots=slots, prompts=prompts, first=first)
        elif kind in ("batch_copy_rows", "refused_prefix"):
            held = [s for s in range(S) if self.slots[s]] if kind == "batch_copy_rows" else list(range(S))
            src = r.choice(held)
            k, n = self.slots[src] or (0, 8)
            dst = r.sample([s for s in range(S) if s != src], r.randint(1, max(1, min(S - 1, 3)))) if S > 1 else [0]
            ext = [s for s in dst if self.slots[s] and self.slots[s][0] == k and self.slots[s][1] < n]
            if kind == "batch_copy_rows" and ext and r.random() < 0.5:
                dst = ext[:1]
                first = self.slots[dst[0]][1]
                rows = r.randint(1, n - first)
            else:
                first, rows = 0, r.randint(1, n)
            if kind == "refused_prefix":
                dst[-1] = S
            else:
                for s in dst:
                    self.slots[s] = (k, first + rows)
            op.update(src=src, dst=dst, first=first, n=rows)
        elif kind == "batch_prefix_set":
            self.prefix = r.choice(PREFIXES)
            op["prompt"] = self.prefix
            self.slots[0] = self.prefix
        elif kind in ("embed_many", "embed_many_prefix", "refused_embed"):
            op.update(reqs=self._reqs(), normalize=r.random() < 0.5, out_dim=r.choice((None, None, 64, 30)) if self.size == "S" else None)
            if kind == "refused_embed":
                op["bad"] = r.randrange(len(op["reqs"]))
            else:
                used = min(len(op["reqs"]), S)
                self.slots[:used] = [None] * used
        elif kind in CHOICE or kind == "refused_choice":
            op["reqs"] = self._reqs(one=True)
            if self.size != "S" and kind not in self.grown:    # the call of a large phase that has to grow both buffers
                self.grown.add(kind)
                op["cand"] = (33, True, r.getrandbits(24))
            else:                                              # 33 and 70: a second and a third grid part of kChoicePart candidates
                op["cand"] = (r.choice((1, 2, 5, 33, 70) if self.size == "S" else (1, 2, 5, 33)), r.random() < 0.5, r.getrandbits(24))
            if kind == "refused_choice":                       # a candidate equal to VOCAB, no candidate at all, a token out of range
                op.update(bad=r.choice(("cand", "k0", "token")), at=r.randrange(len(op["reqs"])))
            else:
                used = min(len(op["reqs"]), S)
                self.slots[:used] = [None] * used
        elif kind in SCORE or kind == "refused_score":
            if force.get("steer"):                             # 33 scored columns of a wide block: a chunk of 32 and a chunk of 1
                op.update(reqs=[MEDIUM[0]], score_from=None)
            else:
                op["reqs"] = self._reqs(one=True)
                op["score_from"] = self._score_from(op["reqs"])
            if kind == "refused_score":                        # score_from 0 or n + 1, a token out of range, an empty prompt
                op.update(bad=r.choice(("from0", "from_past", "token", "empty")), at=r.randrange(len(op["reqs"])))
            else:
                used = min(len(op["reqs"]), S)
                self.slots[:used] = [None] * used
        elif kind in ("set_batch_sampler_on", "set_batch_sampler_off"):
            on = kind.endswith("_on")
            op.update(T=r.choice((0.7, 0.9, 1.2)) if on else 0.0, P=r.choice((0.9, 0.95, 1.0)), seeds=[r.getrandbits(48) + 1 for _ in range(S)])
            if self.bs_on and not on:
                self.turned_off.add(len(self.ops))
            self.bs_on, self.bs_known = on, True
        elif kind == "set_sampler":
            op.update(T=0.0 if self.ss_on else r.choice((0.8, 1.1)), P=r.choice((0.9, 1.0)), seed=r.getrandbits(48) + 1)
            self.ss_on = op["T"] > 0
        elif kind == "batch_reset_kv":
            self.slots = [None] * S
        elif kind == "reset_kv":
            self.single = None
        elif kind == "batch_init":
            streams = force.get("streams") or r.choice([s for s in (2, 3, 5, 8) if s != S])
            ctx = force.get("ctx", r.choice((192, 256, 0) if streams <= 3 else (192, 256)))
            op.update(streams=streams, ctx=ctx)
            self.streams, self.ctx = streams, min(ctx, SEQ) if ctx else SEQ
            self.slots = [None] * streams
            self.bs_on = self.bs_known = False
            self.prefix = None
        self.ops.append(op)
        return op

    # -- the walk
    def pick(self, must):
        prev = self.ops[-1]["op"]
        legal = [k for k in KINDS if self.legal(k) and (prev, k) not in ILLEGAL]
        seen = pairs_of(self.ops) | self.avoid

        def score(k):
            new = (prev, k) not in seen
            onward = sum(1 for b in KINDS if (k, b) not in seen and (k, b) not in ILLEGAL)
            return 1000 * new + 400 * (k in must) + onward + self.rng.random()
        return max(legal, key=score)

    def enable(self, kind):
        """the state changers that make `kind` legal, if any are needed"""
        if kind in SAMPLING_ONLY and not (self.bs_on and self.bs_known):
            self.emit("set_batch_sampler_on")
        if kind in GREEDY_ONLY and self.bs_on:
            self.emit("set_batch_sampler_off")
        if kind == "batch_step_cols_draw" and self.bs_on and not self.bs_known:
            self.emit("set_batch_sampler_on")
        if kind in ("verify", "generate_lookup") and self.ss_on:
            self.emit("set_sampler")
        if kind in NEED_PREFIX and self.prefix is None:
            self.emit("batch_prefix_set")
        if kind == "batch_copy_rows" and not any(self.slots):
            self.emit("batch_prefill_slots")

    def target(self, must):
        """a pair of kinds that no sequence has adjacent yet: the state both need, then the two ops (one, where the first is the last op)"""
        seen = pairs_of(self.ops) | self.avoid
        prev = self.ops[-1]["op"]
        off = ("batch_init",) if self.growth else ()
        todo = [p for p in ALL_PAIRS if p not in seen and p not in ILLEGAL and p[0] not in off and p[1] not in off]
        if not todo:
            return self.emit(self.pick(must))
        ready = [p for p in todo if self.legal(p[0]) and self.legal(p[1]) and (prev, p[0]) not in ILLEGAL]
        owed = [p for p in todo if p[0] in must or p[1] in must]
        open_pairs = set(todo)
        for pool in ([p for p in todo if p[0] == prev and self.legal(p[1])], [p for p in ready if (prev, p[0]) in open_pairs], ready, todo):
            if pool:
                a, b = self.rng.choice([p for p in pool if p in owed] or pool)
                break
        if a != prev:
            self.enable(b)
            self.enable(a)
            if not self.legal(a) or (self.ops[-1]["op"], a) in ILLEGAL:
                return self.emit(self.pick(must))
            self.emit(a)
        if self.legal(b):
            self.emit(b)

    def phase(self, size, n_ops, must):
        """about n_ops ops of one size class, every kind of `must` among them"""
        self.size = size
        must = list(must)
        start = len(self.ops)
        self.large_calls = 0
        self.grown = set()
        if size != "S":                                        # the kinds that have to grow the buffers come first
            for k in must:
                self.enable(k)
                self.emit(k)
            must = []
        while len(self.ops) < start + n_ops:
            at = len(self.ops)
            if len(must) + 4 >= start + n_ops - at:                # no room left: the kinds the phase owes, in a legal order
                k = next((m for m in must if self.legal(m) and (self.ops[-1]["op"], m) not in ILLEGAL), None)
                if k == "set_batch_sampler_off" and not self.bs_on:
                    k = "set_batch_sampler_on"
                if k is None and must:
                    k = "set_batch_sampler_off" if self.bs_on else "set_batch_sampler_on"
                self.emit(k or self.pick(()))
            else:
                self.target(must)
            for i, o in enumerate(self.ops[at:], at):              # (switching the batch sampler off counts where it was on)
                if o["op"] in must and (o["op"] != "set_batch_sampler_off" or i in self.turned_off):
                    must.remove(o["op"])
        assert not must, (size, must)


GROW = ("generate_many_greedy", "generate_many_sampled", "generate_many_dense", "generate_many_stop", "embed_many", "batch_prefill_slots",
        "choice_many", "score_many")


def _sequence(seed, n_ops, avoid):
    g = _Gen(seed, avoid)
    r = g.rng
    a, c = r.sample((2, 3, 5, 8), 2)
    b = r.choice([s for s in (2, 3, 4) if s != a])
    unit = n_ops // 10
    # epoch 0, 256 positions: everything small; the first dense call fixes dense_cap
    g.emit("batch_init", streams=a, ctx=256)
    g.phase("S", 2 * unit, ("generate_many_dense", "set_batch_sampler_on", "set_batch_sampler_off", "batch_prefix_set"))
    # epoch 1, the whole context, few slots: small - large - small - larger - small, no q3_batch_init in between, so that every
    # grow-only buffer is re-allocated twice behind plans that were cached while it was small
    g.emit("batch_init", streams=b if b != g.streams else 4, ctx=0)
    g.growth = True
    # the first use of two column-plan widths (32 and 1, non-draw) is a score chunk's, through plan_get in the walk's grow callback;
    # the column pass of one column behind it runs the plan the chunk has made
    g.emit("score_many", steer=True)
    g.emit("batch_step_cols", one=True)
    warm = ("generate_many_greedy", "generate_many_greedy", "generate_many_sampled", "generate_many_sampled", "generate_many_dense",
            "generate_many_dense", "batch_prefill_slots", "batch_prefill_slots", "embed_many", "embed_many", "generate_many_stop",
            "choice_many", "choice_many", "score_many", "score_many", "set_batch_sampler_on", "set_batch_sampler_off")
    g.phase("S", 2 * unit, warm)
    for _ in range(2):                                         # the second one runs the kept plan of that width
        g.emit("batch_prefill_slots", wide=True)
    for size in ("L1", "L2"):
        g.phase(size, unit, GROW)
        g.phase("S", unit - 1, GROW)
        g.emit("batch_prefill_slots", wide=True)               # small again: score rows of 256 positions would do
    g.growth = False
    # epoch 2: another number of slots, 256 positions again
    g.emit("batch_init", streams=c if c != g.streams else 6, ctx=256)
    g.phase("S", max(unit, n_ops - len(g.ops)), ("generate_many_dense", "set_batch_sampler_on", "set_batch_sampler_off"))
    return g.ops


@functools.lru_cache(maxsize=None)
def _cached_sequence(seed, n_ops):
    avoid = set()
    if seed in SEEDS:                                           # a seed of the suite steers away from the pairs of the seeds in front of it
        for s in SEEDS[:SEEDS.index(seed)]:
            avoid |= pairs_of(_cached_sequence(s, n_ops))
    return _sequence(seed, n_ops, frozenset(avoid))


def make_sequence(seed, n_ops=N_OPS):
    """The ops of a seed: deterministic, legal in the state the ops before them leave, sizes small - large - small - larger - small"""
    import copy
    return copy.deepcopy(_cached_sequence(seed, n_ops))


# ---------------------------------------------------------------------------------------------------------------------------------
# the settings dimension: the engine-wide settings of sections 2m to 2q among the calls above.  These kinds are no part of KINDS or
# ALL_PAIRS: the pair matrix and its twelve seeds stay what they were (tests/test_call_sequences_host.py holds their digests)
# ---------------------------------------------------------------------------------------------------------------------------------
SETTING_KINDS = ("set_top_k", "set_gen_logprobs", "set_penalties", "set_logit_bias", "read_gen_logprobs", "score_top_many", "score_top_many_prefix",
                 "refused_set_top_k", "refused_set_gen_logprobs", "refused_set_penalties", "refused_set_logit_bias", "refused_bias_lists",
                 "refused_score_top")
SETTERS = ("set_top_k", "set_gen_logprobs", "set_penalties", "set_logit_bias")
TOP_KS = (0, 1, 5, 20, 64)
GEN_LPS = (-1, 0, 3, 64)
PENALTIES = ((0.0, 0.0), (0.5, 0.25), (-0.5, 0.75), (1.0, -0.25), (1.5, 2.0))      # a negative presence, a negative frequency, both positive
BIAS_FORMS = ("off", "one", "per", "big")
# a loop kind in its greedy and in its sampled form
VARIANTS = (("generate_many_greedy", False), ("generate_many_sampled", True), ("generate_many_dense", False), ("generate_many_dense", True),
            ("generate_many_stop", False), ("generate_many_stop", True), ("generate_many_prefix", False), ("generate_many_prefix", True))
SETTING_SEEDS = (31, 32, 33, 34, 35, 36)
SETTING_EDGE_SEED = SETTING_SEEDS[1]
OFF = dict(top_k=0, genlp=-1, pen=0, bias="off")


def setting_states():
    """The states every loop variant has to run under: every value class of every setting alone, every pair of settings on, all
    four on.  dict(top_k, genlp, pen = index into PENALTIES, bias = form)"""
    rng = random.Random(5)
    alone = ([dict(OFF, top_k=v) for v in TOP_KS[1:]] + [dict(OFF, genlp=v) for v in GEN_LPS[1:]] + [dict(OFF, pen=i) for i in range(1, len(PENALTIES))]
             + [dict(OFF, bias=f) for f in BIAS_FORMS[1:]])
    pick = dict(top_k=TOP_KS[1:], genlp=GEN_LPS[1:], pen=range(1, len(PENALTIES)), bias=BIAS_FORMS[1:])
    names = list(pick)
    pairs = [dict(OFF, **{a: rng.choice(pick[a]), b: rng.choice(pick[b])}) for i, a in enumerate(names) for b in names[i + 1:]]
    return alone + pairs + [{a: rng.choice(pick[a]) for a in names}]


def form_states():
    """one state per column-plan form that exists: (needs a sampled loop, state) -- top_k on or off, the three genlp forms, the three
    forms of the penalty axis"""
    return [(draw, dict(top_k=5 if topk else 0, genlp=lp, pen=2 if pen == 1 else 0, bias="per" if pen == 2 else "off"))
            for draw, topk in ((False, False), (True, False), (True, True)) for lp in (-1, 0, 3) for pen in range(3)]


def is_big(state):
    """what the small phases of the growth epoch leave out: 64 tops per record and the long lists"""
    return state["genlp"] == 64 or state["bias"] in ("one", "big")


class _SGen(_Gen):
    """_Gen with the four settings tracked and the emitters of SETTING_KINDS"""

    def __init__(self, seed, avoid=frozenset()):
        super().__init__(seed, avoid)
        self.state = dict(OFF)
        self.n_lists = 0                     # of a per-request table in force
        self.users = 0                       # loop ops under the table in force
        self.force = None
        self.built = set()                   # (form, width index) of the column plans of the epoch

    def _reqs(self, dense=False, one=False):
        if self.force is not None:
            return list(self.force)
        return super()._reqs(dense, one)

    def st(self):
        s = self.state
        return dict(top_k=s["top_k"], genlp=s["genlp"], pen=PENALTIES[s["pen"]], table=None if s["bias"] == "off" else 0)

    def emit(self, kind, **force):
        if kind not in SETTING_KINDS:
            op = super().emit(kind, **force)
            if kind == "batch_init":
                self.built = set()
            return op
        r, S = self.rng, self.streams
        op = {"op": kind}
        if kind == "set_top_k":
            op["k"] = self.state["top_k"] = force["k"]
        elif kind == "set_gen_logprobs":
            op["n"] = self.state["genlp"] = force["n"]
        elif kind == "set_penalties":
            self.state["pen"] = force["i"]
            op["p"], op["f"] = PENALTIES[force["i"]]
        elif kind == "set_logit_bias":
            self.state["bias"] = force["form"]
            self.n_lists = force.get("n", 0) if force["form"] == "per" else 0
            self.users = 0
            op.update(form=force["form"], n=self.n_lists, par=force.get("par", r.randrange(2)), seed=r.getrandbits(24))
        elif kind in ("score_top_many", "score_top_many_prefix", "refused_score_top"):
            op["reqs"] = force.get("reqs") or r.sample(SMALL, r.randint(1, 2))
            op["k"] = force.get("k") or (r.choice((0, 65)) if kind == "refused_score_top" else r.choice((1, 5)))
            op["score_from"] = None if "reqs" in force else self._score_from(op["reqs"])
            if kind != "refused_score_top":
                used = min(len(op["reqs"]), S)
                self.slots[:used] = [None] * used
        elif kind == "refused_set_top_k":
            op["k"] = r.choice((65, -1))
        elif kind == "refused_set_gen_logprobs":
            op["n"] = r.choice((-2, 65))
        elif kind == "refused_set_penalties":
            op["bad"] = r.choice(("2.5", "nan"))
        elif kind == "refused_set_logit_bias":
            op.update(bad=r.choice(("twice", "vocab", "inf", "allow")), at=r.randrange(100))
        elif kind == "refused_bias_lists":
            op.update(kind="generate_many_stop", reqs=r.sample(LONG, self.n_lists + 1), sampled=self.bs_on, stop_at=[])
        self.ops.append(op)
        return op

    def legal(self, kind):
        if kind == "score_top_many_prefix":
            return self.prefix is not None
        if kind == "refused_bias_lists":
            return self.n_lists > 1
        return super().legal(kind)

    # -- the settings
    def goto(self, state, n=None):
        """the setting ops that lead to `state` (n: the lists of a per-request table), in a seeded order"""
        todo = [k for k in state if state[k] != self.state[k] or (k == "bias" and state[k] == "per" and n != self.n_lists)]
        self.rng.shuffle(todo)
        for k in todo:
            self.set(k, state[k], n)

    def owed(self, pair):
        """a kind of SETTING_KINDS, legal here, that no sequence has in that place yet: pair(kind) is the ordered pair it would make"""
        seen = pairs_of(self.ops) | self.avoid
        kinds = [k for k in SETTING_KINDS if pair(k) not in seen and self.legal(k)]
        return self.rng.choice(kinds) if kinds else None

    def one(self, kind):
        """one op of a setting kind that leaves the settings as they are: a setter sets the value in force once more"""
        if kind in SETTERS:
            k = ("top_k", "genlp", "pen", "bias")[SETTERS.index(kind)]
            return self.set(k, self.state[k], self.n_lists)
        return self.emit(kind)

    def set(self, k, v, n=None, **force):
        if k == "bias":
            return self.emit("set_logit_bias", form=v, n=n, **force)
        if k == "top_k":
            self.emit("set_top_k", k=v)
        elif k == "genlp":
            self.emit("set_gen_logprobs", n=v)
        elif k == "pen":
            self.emit("set_penalties", i=v)

    # -- one loop op
    def loop(self, variant, reqs):
        kind, sampled = variant
        if self.state["bias"] == "per":
            assert len(reqs) == self.n_lists, (len(reqs), self.n_lists)
        if kind == "generate_many_greedy" and self.bs_on:
            self.emit("set_batch_sampler_off")
        if kind == "generate_many_prefix" and self.prefix is None:
            self.emit("batch_prefix_set")
        if kind in ("generate_many_dense", "generate_many_stop", "generate_many_prefix") and not sampled and self.bs_on:
            self.emit("set_batch_sampler_off")
        self.force = list(reqs)
        op = super().emit(kind)
        self.force = None
        if kind not in ("generate_many_greedy", "generate_many_sampled"):
            op["sampled"] = sampled
            if sampled:
                self.bs_known = False
        if kind == "generate_many_dense":
            op["dense_min"] = self.rng.choice((8, 32))
        self.users += 1
        if kind in ("generate_many_greedy", "generate_many_sampled", "generate_many_dense"):
            self.built |= needs(op, self.streams, self.bs_on, 0, st=self.st())["forms"]
        return op

    def reqs(self, n=None, lo=1, hi=3):
        if self.state["bias"] == "per":
            n = self.n_lists
        return self.rng.sample(LONG, n or self.rng.randint(lo, hi))

    def reqs_for(self, variant, new):
        """a request list whose column plans all exist in the epoch (new False) or of which one does not (new True)"""
        draw = variant[1]
        best = None
        for _ in range(60):
            reqs = self.reqs(lo=1, hi=min(4, 2 * self.streams))
            lens, n_new = [CAT[i][1] for i in reqs], [CAT[i][2] for i in reqs]
            forms = {form_of(draw, self.st()) + (width_index(n),) for n in many_plan(lens, n_new, self.streams)["passes"]}
            if bool(forms - self.built) == new:
                return reqs
            best = best or reqs
        return best

    def filler(self, pool):
        """one op of another kind between two loop ops"""
        kind = self.rng.choice(pool)
        if not self.legal(kind) or (self.ops[-1]["op"], kind) in ILLEGAL or kind in NEED_DRAWS or kind in GREEDY_ONLY:
            kind = "read_gen_logprobs"
        self.one(kind)


# the kinds of the pair matrix that are no loop and start nothing over: what stands between the loop ops of a settings sequence, and
# what has to leave the settings alone
QUIET = tuple(k for k in KINDS if k not in MANY and k != "batch_init")
BETWEEN = ("read_gen_logprobs", "score_top_many", "batch_step_cols_draw", "batch_prefill_slots", "embed_many", "choice_many", "score_many",
           "verify_draw", "forward", "generate_lookup_draw", "set_sampler", "batch_reset_kv", "batch_copy_rows", "prefill_batched",
           "generate_greedy", "refused_stop")


def _settings_sequence(seed, avoid=frozenset()):
    """190 to 260 ops in three epochs (what the coverage tests/test_call_sequences_host.py asserts takes: some 65 loop ops, the
    setting ops that lead from one state to the next, and every setting kind in front of and behind every loop kind).  Epoch 0 is the one whose per-call buffers grow behind cached plans (small - medium - small -
    large - small, the whole context, few slots); epochs 1 and 2 start the batched state over with other slot counts, the last one
    with more, under the settings in force.  The loop variants run through the states of setting_states() that fall to this seed,
    a variant at a time, other kinds between them; a toggle stretch switches one setting on, to another value and off under kept
    plans; a stretch under all four settings goes through the quiet kinds that fall to this seed."""
    g = _SGen(seed, avoid)
    r = g.rng
    at = SETTING_SEEDS.index(seed) if seed in SETTING_SEEDS else seed % 6
    states = setting_states()
    cells = [(v, s) for si, s in enumerate(states) for vi, v in enumerate(VARIANTS) if (si + vi) % len(SETTING_SEEDS) == at]
    for fi, (draw, state) in enumerate(form_states()):          # every form, on two loop kinds: the second finds the first one's plans
        if fi % len(SETTING_SEEDS) == at:
            cells += [(v, state) for v in VARIANTS if v[1] == draw and v[0] != "generate_many_prefix"][:2]
    small = [c for c in cells if not is_big(c[1])]
    big = [c for c in cells if is_big(c[1])]
    r.shuffle(small)
    key = lambda c: sorted((k, str(v)) for k, v in c[1].items())
    small.sort(key=key)
    big.sort(key=key)
    b = r.choice((2, 3, 4))
    a = r.choice([v for v in (2, 3, 5) if v != b])
    c = r.choice((6, 8))

    def cut(cells, k):
        """k, moved on to where the state changes: the cells of one state stay in one epoch"""
        while 0 < k < len(cells) and cells[k - 1][1] == cells[k][1]:
            k += 1
        return k

    def run(cells, fill=0.3):
        reqs = state_before = None
        for variant, state in cells:
            n = r.randint(2, 3) if state["bias"] == "per" else None
            if state == state_before:                           # the same requests: the widths of the loop op in front
                n = len(reqs)
            if state["bias"] != "off" and (g.state["bias"] != "off" and (g.users >= 3 or state["bias"] != g.state["bias"])):
                g.emit("set_logit_bias", form="off")        # a table is made for the loop ops behind it: a few, so that its bans fit the list
            g.goto(state, n)
            x = g.owed(lambda k: (k, variant[0]))
            if x:
                g.one(x)
            reqs = reqs if state == state_before and (state["bias"] != "per" or len(reqs) == g.n_lists) else g.reqs()
            state_before = state
            g.loop(variant, reqs)
            x = g.owed(lambda k: (variant[0], k))
            if x:
                g.one(x)
            elif r.random() < fill:
                g.filler(BETWEEN)

    def grow(size, reqs, variant_a, variant_b):
        """the medium and the large phase: 64 tops per record, the long list, then one list per request, a score call with tops"""
        g.goto(dict(genlp=64, pen=r.randrange(1, len(PENALTIES))))
        g.emit("set_logit_bias", form=size)
        g.loop(variant_a, reqs)
        g.emit("read_gen_logprobs")
        g.emit("set_logit_bias", form="per", n=len(reqs))
        g.loop(variant_b, reqs)
        g.emit("refused_bias_lists")
        g.emit("read_gen_logprobs")                             # refused: the failed call has left nothing to read
        g.emit("score_top_many", reqs=reqs, k=64)
        g.emit("set_logit_bias", form="off")

    def small_again(variant_a, variant_b):
        """the same kinds, small: 3 tops, one short list per request"""
        g.goto(dict(genlp=3))
        g.emit("set_logit_bias", form="per", n=2)
        g.loop(variant_a, g.reqs())
        g.loop(variant_b, g.reqs())
        g.emit("score_top_many", k=r.choice((1, 5)))
        g.emit("set_logit_bias", form="off")

    va, vb = r.choice(VARIANTS[:2]), r.choice(VARIANTS[4:6])
    # epoch 0: the growth epoch
    g.emit("batch_init", streams=b, ctx=0)
    g.growth = True
    for _ in range(2):
        g.emit("batch_prefill_slots", wide=True)               # a dense plan, and its second use
    small_again(va, vb)
    third, two = cut(small, len(small) // 3), cut(small, 2 * len(small) // 3)
    half = cut(big, len(big) // 2)
    run(small[:third])
    small_again(va, vb)
    grow("one", list(LONG[:7]), va, vb)
    small_again(va, vb)
    run(small[third:two])
    grow("big", list(LONG[:12]), va, vb)
    small_again(va, vb)
    g.growth = False
    # the toggle stretch: one setting on, to another value, off and on again, under the kept plans of both forms; behind every
    # switch a loop op on kept widths and one that builds a width
    name = ("top_k", "genlp", "pen", "bias", "top_k", "pen")[at]
    vals = dict(top_k=(5, 20), genlp=(0, 3), pen=(1, 2), bias=("per", "per"))[name]
    tv = VARIANTS[1] if name == "top_k" else r.choice(VARIANTS[:2])
    g.goto(dict(OFF))
    g.loop(tv, g.reqs())
    for v in (vals[0], OFF[name], vals[0], vals[1], OFF[name]):
        if name == "bias" and g.state["bias"] != "off" and v != "off":
            g.emit("set_logit_bias", form="off")
        g.set(name, v, 2)
        g.loop(tv, g.reqs_for(tv, False))
        g.loop(tv, g.reqs_for(tv, True))
    # all four on across q3_batch_init to another slot count
    all_on = dict(states[-1], bias="per")
    g.goto(all_on, 2)
    g.emit("batch_init", streams=a, ctx=256)
    g.loop(r.choice(VARIANTS), g.reqs())
    # epoch 1: the rest of the small states and the first of the big ones
    run(small[two:] + big[:half])
    # all four on, across the state changers and the quiet kinds that fall to this seed, a loop op behind them
    g.emit("set_logit_bias", form="off")
    g.goto(dict(all_on, bias="off"))
    g.emit("set_logit_bias", form="per", n=3, par=1)           # its first list allows three tokens
    quiet = [k for i, k in enumerate(QUIET) if i % len(SETTING_SEEDS) == at] + ["set_sampler", "set_batch_sampler_on", "batch_step_cols_draw",
                                                                                 "set_batch_sampler_off", "batch_step_cols_draw", "batch_reset_kv"]
    for k in quiet:
        g.enable(k)
        if g.legal(k) and (g.ops[-1]["op"], k) not in ILLEGAL:
            g.emit(k)
    g.loop(r.choice(VARIANTS), g.reqs())
    g.emit("read_gen_logprobs")
    # epoch 2: more slots, under all four
    g.emit("batch_init", streams=c, ctx=r.choice((192, 256)))
    g.emit("read_gen_logprobs")
    g.loop(r.choice(VARIANTS), g.reqs())
    run(big[half:])
    g.goto(dict(OFF))
    g.loop(r.choice(VARIANTS), g.reqs())
    return g.ops


@functools.lru_cache(maxsize=None)
def _cached_settings_sequence(seed):
    avoid = set()
    if seed in SETTING_SEEDS:                                   # as for SEEDS: away from the pairs the seeds in front have
        for s in SETTING_SEEDS[:SETTING_SEEDS.index(seed)]:
            avoid |= pairs_of(_cached_settings_sequence(s))
    return _settings_sequence(seed, frozenset(avoid))


def make_settings_sequence(seed):
    """The ops of a settings seed: deterministic, legal in the state the ops before them leave"""
    import copy
    return copy.deepcopy(_cached_settings_sequence(seed))


# ---------------------------------------------------------------------------------------------------------------------------------
# the guide dimension: the dense guide of section 2r, the sparse guide of 2s and the stop automaton of 2t among the calls above.
# These kinds are no part of KINDS or SETTING_KINDS: the twelve sequences of the pair matrix and the six settings sequences stay
# what they were (tests/test_call_sequences_host.py holds the digests of all eighteen)
# ---------------------------------------------------------------------------------------------------------------------------------
GUIDE_KINDS = ("set_guide", "set_guide_sparse", "set_stop_seq", "refused_set_guide", "refused_set_guide_sparse", "refused_set_stop_seq",
               "refused_guide_starts")
GUIDE_SETTERS = GUIDE_KINDS[:3]
GUIDE_FORMS = ("off", "all", "trie", "cycle", "per", "big")
SPARSE_FORMS = ("off", "all", "trie", "cycle", "per", "dflt", "half", "big")
STOP_FORMS = ("off", "hit1", "hit2", "hit3", "overlap", "never", "per", "any", "big")
# one refused form per reason group of the header: a state that allows no token, a start outside [-1, n_states), another vocabulary
# (for q3_guide_set_sparse, whose vocabulary the binding states itself: a token outside it), an entry, a dflt or an edge outside the
# states, a token that does not ascend, row_off[n_states] != n_edges
GUIDE_REFUSALS = {"refused_set_guide": ("dead", "start", "vocab", "entry"), "refused_set_guide_sparse": ("dead", "ascend", "row_off", "start", "vocab"),
                  "refused_set_stop_seq": ("ascend", "row_off", "start", "vocab", "dflt")}
GUIDE_BUFFERS = ("guide_next", "guide_start", "guide_sp_dflt", "guide_sp_off", "guide_sp_edges", "guide_sp_start", "stop_seq_dflt", "stop_seq_off",
                 "stop_seq_edges", "stop_seq_start")
GUIDE_SEEDS = (41, 42, 43, 44, 45, 46)
GUIDE_EDGE_SEED = GUIDE_SEEDS[1]
G_OFF = dict(OFF, guide=("off", "off"), stop="off")         # guide: (which of the two forms, the automaton's form)
STOP_VARIANTS = VARIANTS[4:]                                # the two loops with a device scheduler: they honour the stop automaton


def guide_states():
    """The states every loop variant has to run under: every guide form and every stop form alone (the forms "big" run where the
    buffers grow), a guide with a stop automaton, a guide with each of the four earlier settings at one value"""
    alone = ([dict(G_OFF, guide=("dense", f)) for f in GUIDE_FORMS[1:-1]] + [dict(G_OFF, guide=("sparse", f)) for f in SPARSE_FORMS[1:-1]]
             + [dict(G_OFF, stop=f) for f in STOP_FORMS[1:-1]])
    both = [dict(G_OFF, guide=("dense", "cycle"), stop="hit2"), dict(G_OFF, guide=("sparse", "trie"), stop="hit1")]
    other = [dict(G_OFF, guide=("dense", "cycle"), top_k=5), dict(G_OFF, guide=("sparse", "cycle"), genlp=3), dict(G_OFF, guide=("dense", "trie"), pen=1),
             dict(G_OFF, guide=("sparse", "half"), bias="per")]
    return alone + both + other


def guide_form_states():
    """one state per column-plan form under a guide: (needs a sampled loop, state) -- top_k on or off, the three genlp forms, the two
    guide forms of the penalty axis: 18"""
    return [(draw, dict(G_OFF, top_k=5 if topk else 0, genlp=lp, guide=(kind, "cycle")))
            for draw, topk in ((False, False), (True, False), (True, True)) for lp in (-1, 0, 3) for kind in ("dense", "sparse")]


class _GGen(_SGen):
    """_SGen with the guide and the stop automaton tracked as two more settings, and the emitters of GUIDE_KINDS"""

    def __init__(self, seed, avoid=frozenset()):
        super().__init__(seed, avoid)
        self.state = dict(G_OFF)
        self.n_of = dict(guide=0, stop=0)    # the start states of a per-request form in force

    def st(self):
        s = super().st()
        s["gform"] = None if self.state["guide"][0] == "off" else self.state["guide"][0]
        return s

    def need(self):
        """the number of requests a loop op must have: the lists of a per-request table, the start states of a per-request automaton"""
        n = {v for v in (self.n_lists, self.n_of["guide"], self.n_of["stop"]) if v > 1}
        assert len(n) <= 1, n
        return n.pop() if n else 0

    def reqs(self, n=None, lo=2, hi=4):
        return self.rng.sample(LONG, self.need() or n or self.rng.randint(lo, hi))

    def reqs_for(self, variant, new):
        """one request whose column plans all exist in the epoch (new False) or of which one does not (new True): its prompt alone
        decides the widths, so that a form keeps widths to build through several visits"""
        order = list(LONG)
        self.rng.shuffle(order)
        for i in ([] if self.need() else order):
            forms = {form_of(variant[1], self.st()) + (width_index(n),) for n in many_plan([CAT[i][1]], [CAT[i][2]], self.streams)["passes"]}
            if bool(forms - self.built) == new:
                return [i]
        return super().reqs_for(variant, new)

    def loop(self, variant, reqs):
        op = super().loop(variant, reqs)
        if op["op"] in ("generate_many_stop", "generate_many_prefix"):          # by the request list, as the host tests count them
            rows, stop = ([[0] * CAT[i][2] for i in op["reqs"]], (1,)) if op["stop_at"] else (None, ())
            self.built |= needs(op, self.streams, self.bs_on, 0, rows, stop, st=self.st())["forms"]
        return op

    def legal(self, kind):
        if kind == "refused_guide_starts":
            return max(self.n_of.values()) > 1
        return super().legal(kind)

    def emit(self, kind, **force):
        if kind not in GUIDE_KINDS:
            return super().emit(kind, **force)
        r = self.rng
        op = {"op": kind}
        if kind in GUIDE_SETTERS:
            form = force["form"]
            op.update(form=form, seed=r.getrandbits(24))
            per = form in ("per", "big")
            if per:
                op["n"] = force["n"]
            for k in ("size", "early", "ns"):
                if force.get(k):
                    op[k] = force[k]
            if kind == "set_stop_seq":
                self.state["stop"], self.n_of["stop"] = form, force["n"] if per else 0
            else:
                self.state["guide"] = ("off", "off") if form == "off" else ("dense" if kind == "set_guide" else "sparse", form)
                self.n_of["guide"] = force["n"] if per else 0
        elif kind == "refused_guide_starts":
            which = "guide" if self.n_of["guide"] > 1 else "stop"
            op.update(kind="generate_many_stop", reqs=r.sample(LONG, self.n_of[which] + 1), sampled=self.bs_on, stop_at=[],
                      of=self.state["guide"][0] if which == "guide" else "stop")
        else:
            op.update(bad=force.get("bad") or r.choice(GUIDE_REFUSALS[kind]), at=r.randrange(100))
        self.ops.append(op)
        return op

    def set(self, k, v, n=None, **force):
        if k == "guide":
            if v[0] == "off":
                return self.emit("set_guide" if self.state["guide"][0] != "sparse" else "set_guide_sparse", form="off")
            return self.emit("set_guide" if v[0] == "dense" else "set_guide_sparse", form=v[1], n=n, **force)
        if k == "stop":
            return self.emit("set_stop_seq", form=v, n=n, **force)
        return super().set(k, v, n, **force)

    def goto(self, state, n=None):
        per = dict(bias=lambda v: v == "per", guide=lambda v: v[1] in ("per", "big"), stop=lambda v: v in ("per", "big"))
        have = dict(bias=self.n_lists, guide=self.n_of["guide"], stop=self.n_of["stop"])
        todo = [k for k in state if state[k] != self.state[k] or (k in per and per[k](state[k]) and n != have[k])]
        self.rng.shuffle(todo)
        for k in todo:
            self.set(k, state[k], n)

    def owed(self, pair):
        seen = pairs_of(self.ops) | self.avoid
        kinds = [k for k in GUIDE_KINDS if pair(k) not in seen and self.legal(k)]
        return self.rng.choice(kinds) if kinds else None

    def one(self, kind):
        """one op of a guide kind that leaves the forms in force: a setter sets the form in force once more, with another automaton"""
        if kind == "set_stop_seq":
            return self.emit(kind, form=self.state["stop"], n=self.n_of["stop"])
        if kind in GUIDE_SETTERS:
            kinds = dict(dense="set_guide", sparse="set_guide_sparse")
            if kinds.get(self.state["guide"][0], kind) != kind:                  # the other form is in force: it stays in force
                return self.emit("refused_" + kind)
            return self.emit(kind, form=self.state["guide"][1], n=self.n_of["guide"])
        if kind in GUIDE_KINDS:
            return self.emit(kind)
        return super().one(kind)


def _guide_sequence(seed, avoid=frozenset()):
    """Three epochs in the shape of a settings sequence.  Epoch 0 is the one whose arrays grow behind cached plans (small - medium -
    small - large - small: the dense table, the sparse arrays, the stop automaton and their start states), then a toggle stretch:
    guide off -> dense -> dense (another table, the same states) -> sparse -> dense -> off and stop automaton off -> on -> another ->
    off under kept plans, two loop ops behind every switch.  Epochs 1 and 2 start the batched state over with other slot counts, the
    last one with more, under a guide and a stop automaton.  The loop variants run through the states of guide_states() and
    guide_form_states() that fall to this seed; a stretch under a guide and a stop automaton goes through the quiet kinds that fall
    to this seed; one op runs under a table that bans a state's only tokens (the else branch of the state step), one under
    min_tokens with a sequence that completes in front of it."""
    g = _GGen(seed, avoid)
    r = g.rng
    at = GUIDE_SEEDS.index(seed) if seed in GUIDE_SEEDS else seed % 6
    n_seeds = len(GUIDE_SEEDS)
    cells = [(v, s) for si, s in enumerate(guide_states()) for vi, v in enumerate(VARIANTS) if (si + vi) % n_seeds == at]
    for fi, (draw, state) in enumerate(guide_form_states()):    # every form, on two loop kinds: the second finds the first one's plans
        if fi % n_seeds == at:
            cells += [(v, state) for v in VARIANTS if v[1] == draw and v[0] != "generate_many_prefix"][:2]
    r.shuffle(cells)
    cells.sort(key=lambda c: sorted((k, str(v)) for k, v in c[1].items()))
    b = r.choice((2, 3))
    a = r.choice([v for v in (2, 3, 4) if v != b])
    c = r.choice((6, 8))
    kind_of = lambda k: "dense" if k % 2 == at % 2 else "sparse"
    both = lambda k: dict(G_OFF, guide=(kind_of(k), "cycle"), stop="hit2")

    def cut(k):
        while 0 < k < len(cells) and cells[k - 1][1] == cells[k][1]:
            k += 1
        return k

    def run(cells, fill=0.25):
        reqs = before = None
        for variant, state in cells:
            per = state["bias"] == "per" or state["guide"][1] == "per" or state["stop"] == "per"
            n = (len(reqs) if state == before else r.randint(3, 4)) if per else None
            if state["bias"] != "off" and g.state["bias"] != "off" and (g.users >= 3 or state["bias"] != g.state["bias"]):
                g.emit("set_logit_bias", form="off")
            g.goto(state, n)
            x = g.owed(lambda k: (k, variant[0]))
            if x:
                g.one(x)
            reqs = reqs if state == before and (not g.need() or len(reqs) == g.need()) else g.reqs()
            before = state
            g.loop(variant, reqs)
            x = g.owed(lambda k: (variant[0], k))
            if x:
                g.one(x)
            elif r.random() < fill:
                g.filler(BETWEEN)

    def grow(k, reqs):
        """the medium and the large phase: the dense table "big" with one start per request, then the sparse arrays and the stop
        automaton "big"; a call with one request more is refused under each of the three"""
        n = len(reqs)
        va, vb, vc = VARIANTS[(2 * at + k) % 8], VARIANTS[(2 * at + k + 3) % 8], STOP_VARIANTS[(2 * at + k) % 4]
        g.goto(dict(G_OFF))
        g.emit("set_guide", form="big", size=k + 1, n=n)
        g.loop(va, reqs)
        if k == 0:
            g.emit("refused_guide_starts")
        if vb not in STOP_VARIANTS:                             # a loop that does not read it runs beside the large stop automaton
            g.emit("set_stop_seq", form="big", size=k + 1, n=n)
        g.emit("set_guide_sparse", form="big", size=k + 1, n=n)
        g.loop(vb, reqs)
        if k == 1:
            g.emit("refused_guide_starts")
        g.emit("set_guide_sparse", form="off")
        if vb in STOP_VARIANTS:
            g.emit("set_stop_seq", form="big", size=k + 1, n=n)
        g.emit("refused_guide_starts")
        g.loop(vc, reqs)                                        # the stop automaton alone, on a loop that honours it: its arrays grow here
        g.emit("set_stop_seq", form="off")
        return va, vb, vc

    def small_again(va, vb, vc):
        """the same kinds, small"""
        g.goto(dict(G_OFF))
        g.emit("set_guide", form="cycle")
        g.loop(va, g.reqs())
        g.emit("set_guide_sparse", form="dflt")
        g.loop(vb, g.reqs())
        g.emit("set_stop_seq", form="hit1")
        g.loop(vc, g.reqs())
        g.emit("set_guide_sparse", form="off")
        g.emit("set_stop_seq", form="off")

    # epoch 0: the growth epoch
    g.emit("batch_init", streams=b, ctx=0)
    g.growth = True
    for _ in range(2):
        g.emit("batch_prefill_slots", wide=True)               # a dense plan, and its second use
    third, two = cut(len(cells) // 3), cut(2 * len(cells) // 3)
    firsts = [(VARIANTS[(2 * at + k) % 8], VARIANTS[(2 * at + k + 3) % 8], STOP_VARIANTS[(2 * at + k) % 4]) for k in (0, 1)]
    small_again(*firsts[0])
    small_again(*firsts[1])
    run(cells[:third])
    grow(0, list(LONG[:7]))
    small_again(*firsts[0])
    grow(1, list(LONG[:12]))
    small_again(*firsts[1])
    small_again(*firsts[0])
    g.growth = False
    for kind, vals in GUIDE_REFUSALS.items():                   # every refusal value falls to a seed
        g.emit(kind, bad=vals[at % len(vals)])
    # the toggle stretch of the guide, under the kept plans of all three forms: behind every switch a loop op on kept widths and one
    # that builds a width
    tv = r.choice(VARIANTS[:2])
    g.goto(dict(G_OFF, genlp=0))                                # (with records: forms of which the epoch has built few widths)
    g.loop(tv, [LONG[0]])
    for kind in ("set_guide", "set_guide_sparse"):
        g.emit(kind, form="cycle", ns=4)
        g.loop(tv, [LONG[0]])
    g.emit("set_guide_sparse", form="off")
    for kind, form in (("set_guide", "cycle"), ("set_guide", "cycle"), ("set_guide_sparse", "cycle"), ("set_guide", "cycle"), ("set_guide", "off")):
        g.emit(kind, form=form, ns=4 if form == "cycle" else None)
        g.loop(tv, g.reqs_for(tv, False))
        g.loop(tv, g.reqs_for(tv, True))
    # ... and of the stop automaton, on a loop that honours it
    sv = r.choice(STOP_VARIANTS)
    g.loop(sv, [LONG[0]])
    for form in ("hit2", "overlap", "off"):                     # (overlap: every seed ends a request over a fall-back edge)
        g.emit("set_stop_seq", form=form)
        g.loop(sv, g.reqs_for(sv, False))
        g.loop(sv, g.reqs_for(sv, True))
    # a guide and a stop automaton across q3_batch_init to another slot count
    g.goto(both(0))
    g.emit("batch_init", streams=a, ctx=256)
    g.loop(r.choice(STOP_VARIANTS), g.reqs())
    # epoch 1: the second third of the cells
    run(cells[third:two])
    # the else branch of the state step: a table that bans the three tokens the cycle's small state allows, under greedy
    g.goto(dict(G_OFF, guide=(kind_of(1), "cycle")))
    g.emit("set_logit_bias", form="kill")
    g.loop(r.choice((VARIANTS[0], VARIANTS[4])), g.reqs())
    g.emit("set_logit_bias", form="off")
    # min_tokens does not delay a sequence match: a sequence that completes with the first token, under a list with until = 4
    g.goto(dict(G_OFF))
    g.emit("set_stop_seq", form="hit1", early=True)
    g.emit("set_logit_bias", form="min")
    g.loop(r.choice(STOP_VARIANTS), g.reqs())
    g.emit("set_logit_bias", form="off")
    # a guide and a stop automaton, across the state changers and the quiet kinds that fall to this seed, a loop op behind them
    g.goto(both(1))
    quiet = [k for i, k in enumerate(QUIET) if i % n_seeds == at] + ["set_sampler", "set_batch_sampler_on", "batch_step_cols_draw",
                                                                      "set_batch_sampler_off", "batch_step_cols_draw", "batch_reset_kv"]
    for k in quiet:
        g.enable(k)
        if g.legal(k) and (g.ops[-1]["op"], k) not in ILLEGAL:
            g.emit(k)
    g.loop(r.choice(STOP_VARIANTS), g.reqs())
    # epoch 2: more slots, under both
    g.emit("batch_init", streams=c, ctx=r.choice((192, 256)))
    g.loop(r.choice(STOP_VARIANTS), g.reqs())
    run(cells[two:])
    g.goto(dict(G_OFF))
    g.loop(r.choice(VARIANTS), g.reqs())
    return g.ops


@functools.lru_cache(maxsize=None)
def _cached_guide_sequence(seed):
    avoid = set()
    if seed in GUIDE_SEEDS:                                     # as for SEEDS: away from the pairs the seeds in front have
        for s in GUIDE_SEEDS[:GUIDE_SEEDS.index(seed)]:
            avoid |= pairs_of(_cached_guide_sequence(s))
    return _guide_sequence(seed, frozenset(avoid))


def make_guide_sequence(seed):
    """The ops of a guide seed: deterministic, legal in the state the ops before them leave"""
    import copy
    return copy.deepcopy(_cached_guide_sequence(seed))


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference: the C oracle, memoised
# ---------------------------------------------------------------------------------------------------------------------------------
class _Node:
    __slots__ = ("parent", "tok", "pos", "k", "v", "logits", "x", "kids", "wide")

    def __init__(self, parent, tok):
        self.parent, self.tok, self.pos, self.kids, self.wide = parent, tok, (parent.pos + 1 if parent else -1), {}, None


class Reference:
    """Everything the tests expect comes from here, and everything here comes from oracle.OracleModel.forward, oracle.Sampler and
    oracle.sample_argmax.  A trie over token sequences holds, per sequence, the key and value rows its last token writes, its logits
    and its final-norm tap; the oracle's cache is loaded with a node's path before the node's children are computed (its rows depend on
    the tokens in front of them and on nothing else)."""

    def __init__(self, oracle, path):
        self.oracle = oracle
        self.om = oracle.OracleModel(path, SEQ)
        c = self.om.config
        assert (c.seq_len, c.vocab_size, c.dim) == (SEQ, VOCAB, DIM)
        self.L, self.kvd = c.n_layers, c.n_kv_heads * c.head_dim
        lib = oracle.lib()
        shp = (c.n_layers, c.seq_len, self.kvd)
        self._K = np.ctypeslib.as_array(lib.q3o_key_cache(self.om._h), shape=shp)        # the oracle's own caches, not copies
        self._V = np.ctypeslib.as_array(lib.q3o_value_cache(self.om._h), shape=shp)
        self.root = _Node(None, -1)
        self._at = self.root
        self._memo = {}
        self.forwards = 0

    @staticmethod
    def _path(node):
        out = []
        while node.parent is not None:
            out.append(node)
            node = node.parent
        return out[::-1]

    def _load(self, node):
        if self._at is node:
            return
        want, have = self._path(node), self._path(self._at)
        c = 0
        while c < len(want) and c < len(have) and want[c] is have[c]:
            c += 1
        for n in want[c:]:
            self._K[:, n.pos] = n.k
            self._V[:, n.pos] = n.v
        self._at = node

    def child(self, node, tok):
        n = node.kids.get(tok)
        if n is None:
            self._load(node)
            n = _Node(node, tok)
            n.logits = self.om.forward(tok, n.pos)
            n.k, n.v, n.x = self._K[:, n.pos].copy(), self._V[:, n.pos].copy(), self.om.tap_x()
            node.kids[tok] = n
            self._at = n
            self.forwards += 1
        return n

    def node(self, seq):
        n = self.root
        for t in seq:
            n = self.child(n, t)
        return n

    @staticmethod
    def record(node, target):
        """score_ref.record(node.logits, target).  Its vocabulary-wide part (max, sum, argmax) is kept on the node: score_ref.exps goes
        through ctypes element by element, once per node and not once per op"""
        import score_ref
        if node.wide is None:
            r = score_ref.record(node.logits, 0)
            node.wide = (r["max"], r["sum"], r["argmax"])
        out = np.zeros((), dtype=score_ref.DTYPE)
        out["target"], (out["max"], out["sum"], out["argmax"]) = node.logits[target], node.wide
        return out

    def draw(self, logits, T, P, state, top_k=0):
        """(token, rng state afterwards): Sampler::sample with that state, the argmax and no coin at temperature 0; under top_k > 0
        section 2n's draw among the survivors (topk_ref.sample_top_k over the same oracle sampler)"""
        if not T > 0:
            return self.oracle.sample_argmax(logits), state
        if top_k:
            import topk_ref
            return topk_ref.sample_top_k(self.oracle, logits, T, P, top_k, state)
        s = self.oracle.Sampler(VOCAB, T, P, state)
        tok = s.sample(logits)
        return tok, int(s.rng_state.value)

    def generate(self, prompt, n_new, sampler=None, top_k=0, presence=0.0, frequency=0.0, entries=(), mode=0, dev=(), guide=None, start=-1):
        """The header's rule for request rows: what a fresh engine returns for prefill(prompt) and generate_greedy behind it, after
        set_sampler(temperature, topp, seed) when sampler = (temperature, topp, seed) -- one discarded sample per prompt position
        in front of the last.  Under the engine-wide settings of sections 2n, 2p and 2q output g is taken from
        bias_ref.rule(row, entries, mode, g, counts, presence, frequency) -- the table first, the penalties over the request's own
        outputs on top -- by the largest key (pen_ref.argmax_key) or by the draw among the top_k.  dev: deviations from the rule,
        the injected leaks of FakeEngine alone -- ("counts0", ((token, count), ..)) counts the request does not start from zero with,
        ("per_g", ((entries, mode, g), ..)) the list and the output index each output is adjusted by, ("adjusted",) the records
        are taken on the adjusted row.
        guide (a Guide) and start >= 0: sections 2r and 2s -- the row of output g is masked by the guide's row of state s_g first
        (guide_ref.mask), bias_ref.rule runs on the masked row, and behind the commit s_{g+1} = next[s_g][y_g] where that is >= 0,
        else s_g; the records stay on the raw row.  Deviations: ("g0state", s) the request starts in s and not in start, ("y0_raw",)
        output 0 is not masked, ("masked_records",) the records are taken on the masked row.
        Returns (the n_new tokens, the rng state afterwards, per token the node whose logits it was taken from, per token the row a
        record is taken on: None for the node's own logits)."""
        if guide is None or start < 0:
            guide, start = None, -1
        key = (tuple(prompt), n_new, sampler, top_k, presence, frequency, tuple(entries), mode, dev, guide.key if guide else None, start)
        if key not in self._memo:
            T, P, state = sampler if sampler else (0.0, 1.0, 0)
            plain = not (top_k or presence or frequency or entries or mode or dev or guide)
            dev_of = dict((d[0], d[1:]) for d in dev)
            n, tok, out, nodes, rows = self.root, None, [], [], []
            for t in prompt:
                n = self.child(n, t)
                if T > 0 and plain:
                    tok, state = self.draw(n.logits, T, P, state)
            if plain:
                if not T > 0:
                    tok = self.oracle.sample_argmax(n.logits)
                out.append(tok)
                nodes.append(n)
                while len(out) < n_new:
                    n = self.child(n, tok)
                    tok, state = self.draw(n.logits, T, P, state)
                    out.append(tok)
                    nodes.append(n)
                rows = [None] * n_new
            else:
                import bias_ref
                import pen_ref
                if T > 0:
                    state = xorshift(state, len(prompt) - 1)           # a discarded prompt-position draw burns its coin and selects nothing
                counts = np.zeros(VOCAB, dtype=np.uint32)
                for t, c in (dev_of["counts0"][0] if "counts0" in dev_of else ()):
                    counts[t] = c
                pen = bool(presence or frequency)
                s = dev_of["g0state"][0] if "g0state" in dev_of else start
                for g in range(n_new):
                    if g:
                        n = self.child(n, tok)
                    en, mo, ge = dev_of["per_g"][0][g] if "per_g" in dev_of else (entries, mode, g)
                    raw = n.logits
                    if guide is not None and s >= 0 and not (g == 0 and "y0_raw" in dev_of):
                        import guide_ref
                        raw = guide_ref.mask(n.logits, guide.row(s))
                    row = bias_ref.rule(raw, en, mo, ge, counts if pen else None, presence, frequency)
                    if T > 0:
                        tok, state = self.draw(row, T, P, state, top_k)
                    else:
                        tok = pen_ref.argmax_key(row)
                    counts[tok] += 1
                    if guide is not None and s >= 0:
                        s = guide.step(s, int(tok))
                    out.append(int(tok))
                    nodes.append(n)
                    rows.append(row if "adjusted" in dev_of else raw if "masked_records" in dev_of and raw is not n.logits else None)
            self._memo[key] = (out, state, nodes, rows)
        return self._memo[key]


def cut_at_stop(row, stop):
    for i, t in enumerate(row):
        if t in stop:
            return row[:i + 1]
    return row


class Guide:
    """A guide as the reference reads it, in either statement: kind "dense" with next[n_states][V], or "sparse" with the four arrays
    (default, offsets, tokens, targets); starts as the setter takes them.  row(s) is next[s][0 .. V) in both."""

    def __init__(self, kind, arrays, starts):
        import hashlib
        self.kind, self.starts = kind, [int(s) for s in starts]
        h = hashlib.blake2b(digest_size=16)
        if kind == "dense":
            self.next = np.ascontiguousarray(arrays, dtype=np.int16)
            self.n_states = self.next.shape[0]
            h.update(self.next.tobytes())
        else:
            d, o, t, x = arrays
            self.default, self.offsets = np.ascontiguousarray(d, dtype=np.int32), np.ascontiguousarray(o, dtype=np.int64)
            self.tokens, self.targets = np.ascontiguousarray(t, dtype=np.int32), np.ascontiguousarray(x, dtype=np.int32)
            self.n_states = self.default.size
            for a in (self.default, self.offsets, self.tokens, self.targets):
                h.update(a.tobytes())
                h.update(b"|")
        self.key = (kind, h.hexdigest())
        self._rows = {}

    def row(self, s):
        if self.kind == "dense":
            return self.next[s]
        if s not in self._rows:
            a, b = int(self.offsets[s]), int(self.offsets[s + 1])
            row = np.full(VOCAB, self.default[s], dtype=np.int32)
            row[self.tokens[a:b]] = self.targets[a:b]
            self._rows[s] = row
        return self._rows[s]

    def step(self, s, tok):
        """the state step with its else branch"""
        if s < 0:
            return s
        to = int(self.row(s)[tok])
        return to if to >= 0 else s

    def state_of(self, s, tokens):
        for t in tokens:
            s = self.step(s, t)
        return s

    def start_of(self, r):
        return self.starts[0] if len(self.starts) == 1 else self.starts[r]

    def sizes(self):
        """what the grow-only arrays of the form hold (guide_call_begin, guide_sp_call_begin)"""
        if self.kind == "dense":
            return dict(guide_next=self.next.size, guide_start=len(self.starts))
        return dict(guide_sp_dflt=self.n_states, guide_sp_off=self.n_states + 1, guide_sp_edges=max(self.tokens.size, 1), guide_sp_start=len(self.starts))


def stop_next(a, s, tok):
    """next[s][tok] of a stop automaton in section 2s's arrays"""
    lo, hi = int(a.offsets[s]), int(a.offsets[s + 1])
    k = lo + int(np.searchsorted(a.tokens[lo:hi], tok))
    return int(a.targets[k]) if k < hi and a.tokens[k] == tok else int(a.default[s])


def stop_emit(a, start, row, from_index=0):
    """(n_emit, the state left) of one row under the stop automaton a stepped from `start`, by the automaton itself: what the leaks of
    FakeEngine need, which start somewhere else than the rule says.  Matches in front of from_index do not end the row."""
    s = start
    if s < 0:
        return len(row), -1
    for i, t in enumerate(row):
        x = stop_next(a, s, t)
        if x < 0:
            if i >= from_index:
                return i + 1, -1
            x = a.start
        s = x
    return len(row), s


def check_sparse_arrays(default, offsets, tokens, targets, starts, vocab, dead_ok):
    """what q3_guide_set_sparse and q3_stop_seq_set refuse about their arrays (IndexError: the binding's Q3_ERR_ARG)"""
    d, o, t, x = (np.asarray(v, dtype=np.int64) for v in (default, offsets, tokens, targets))
    S, E = d.size, t.size
    bad = (S == 0 or not starts or o.size != S + 1 or x.size != E or vocab != VOCAB or any(not -1 <= s < S for s in starts)
           or o[0] != 0 or (np.diff(o) < 0).any() or o[-1] != E or d.min() < -1 or d.max() >= S
           or (E and (t.min() < 0 or t.max() >= vocab or x.min() < -1 or x.max() >= S)))
    if not bad:
        own = np.repeat(np.arange(S), np.diff(o))
        bad = E > 1 and bool(((np.diff(t) <= 0) & (own[1:] == own[:-1])).any())
        allowed = np.bincount(own[x >= 0], minlength=S) if E else np.zeros(S, dtype=np.int64)
        bad = bad or (not dead_ok and bool(((allowed == 0) & ((d < 0) | (np.diff(o) == vocab))).any()))
    if bad:
        raise IndexError("the arrays of a sparse automaton are refused")


# ---------------------------------------------------------------------------------------------------------------------------------
# the fake engine: explicit state, answers from the reference
# ---------------------------------------------------------------------------------------------------------------------------------
class Refused(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"[status {code}] {msg}")
        self.code = code


class _Cache:
    def __init__(self, ref, ctx):
        self.K = np.zeros((ref.L, ctx, ref.kvd), dtype=np.float32)
        self.V = np.zeros_like(self.K)
        self.hist, self.node, self.ctx = [], ref.root, ctx


LEAKS = ("sampler", "prefix", "length", "slot_rng", "stale_cand")
SETTING_LEAKS = ("pen_counts", "pen_prompt", "bias_stale", "bias_ooff", "genlp_stale", "genlp_penalised", "topk_init", "settings_touch_cols",
                 "score_top_shared")
GUIDE_LEAKS = ("guide_slot_state", "guide_y0_raw", "guide_init_dropped", "guide_both_forms", "guide_table_stale", "guide_start_shared",
               "guide_touch_cols", "guide_records_masked", "stop_prompt_steps", "stop_slot_state", "stop_in_plain_loops", "stop_min_tokens",
               "stop_init_dropped")


class FakeEngine:
    """The calls of Transformer that touch the batched state, and the single-stream ones that share the engine, over explicit state:
    per cache its rows and the tokens they were computed from, the two samplers with their rng states, the resident prefix, the batch
    shape.  Every number comes from Reference.  leak: one of LEAKS --
        "sampler": a slot's sampler state is carried from one generate_many_sampled call into the next instead of being loaded
        "prefix":  the resident prefix survives q3_batch_init
        "length":  batch_reset_kv leaves the rows of every slot's occupant in place
        "slot_rng": a choice or score call advances the sampler state of every slot it fills by one coin per prompt token, as a dense
                   generate loop does and these calls must not
        "stale_cand": choice_many answers with the previous call's candidate ids at every index that call had: a candidate buffer
                   that is uploaded only where it has grown
    and of SETTING_LEAKS, over the state of sections 2m to 2q --
        "pen_counts": a slot's produced-token counts are not cleared for its next occupant, within a call and across calls
        "pen_prompt": the prompt's tokens enter the counts
        "bias_stale": a call under a shorter table sees the previous table's entries at the indices it did not overwrite: they
                   stand behind its last list
        "bias_ooff": a column finds its request and its output index g from the previous call's o_off
        "genlp_stale": the entries of the record buffers that a call does not write keep the previous call's bytes (no clear)
        "genlp_penalised": the records are taken on the adjusted row
        "topk_init": batch_init resets top_k to 0
        "settings_touch_cols": batch_step_cols_draw adjusts its rows by the table's first list and the slot's counts
        "score_top_shared": score_top_many behind a loop with tops answers the first chunk's tops and ranks from the part lists
                   the loop's last pass left
    and of GUIDE_LEAKS, over the state of sections 2r to 2t --
        "guide_slot_state": a reused slot's first output is taken in the state its predecessor left, not in start[r]
        "guide_y0_raw": output 0 is not masked
        "guide_init_dropped": batch_init clears the guide
        "guide_both_forms": setting the sparse form leaves the dense one in force
        "guide_table_stale": a set_guide with the state count of the table before keeps that table (a serial number that is not bumped)
        "guide_start_shared": every request starts in start[0]
        "guide_touch_cols": batch_step_cols_draw masks its rows by the guide's start state
        "guide_records_masked": the records are taken on the masked row
        "stop_prompt_steps": the tokens in front of the first output -- the resident prefix and the prompt -- move the stop state
        "stop_slot_state": the next occupant of a slot continues from the stop state its predecessor left
        "stop_in_plain_loops": generate_many_greedy, _sampled and _dense cut their rows
        "stop_min_tokens": a sequence match in front of the largest `until` of the request's list does not end the request
        "stop_init_dropped": batch_init clears the stop automaton"""

    def __init__(self, ref, leak=None):
        assert leak is None or leak in LEAKS + SETTING_LEAKS + GUIDE_LEAKS
        self.guide = self.guide_held = None  # the Guide in force (either form), and the one a leak keeps on the device
        self.stopa = None                    # (automaton, starts): the stop automaton in force
        self.ref, self.leak = ref, leak
        self.single = _Cache(ref, SEQ)
        self.slots, self.streams, self.ctx = [], 0, 0
        self.sT, self.sP, self.srng = 0.0, 1.0, None
        self.bT, self.bP, self.brng = 0.0, 1.0, []
        self.prefix = []
        self.loop_rng = {}
        self.last_cand = []
        self.touched = {}
        # the engine-wide settings: they outlive batch_init, both samplers and every call
        self.k_top, self.genlp, self.pen, self.bias = 0, -1, (0.0, 0.0), ([], [])
        self.gen = None                      # the records of the last loop call: dict(k, cap, got, recs, tops, ranks), None: nothing to read
        self.dev = {}                        # what the leaks need of the device: counts per slot, the buffers a call found in place

    # -- the settings (sections 2m to 2q)
    def set_top_k(self, k):
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= 64:
            raise ValueError("top_k out of range")
        self.k_top = k

    top_k = property(lambda self: self.k_top)

    def set_gen_logprobs(self, top_n):
        if not -1 <= top_n <= 64:
            raise ValueError("logprobs out of range")
        self.genlp = top_n

    def get_gen_logprobs(self):
        return self.genlp

    def set_penalties(self, presence, frequency):
        with np.errstate(over="ignore"):
            v = [np.float32(presence), np.float32(frequency)]
        if not all(np.isfinite(x) and abs(x) <= 2 for x in v):
            raise ValueError("penalty out of range")
        self.pen = (float(v[0]), float(v[1]))

    def get_penalties(self):
        return self.pen

    def set_logit_bias(self, lists, modes=None):
        lists = [list(l.items()) if isinstance(l, dict) else list(l) for l in lists]
        modes = [0] * len(lists) if modes is None else [int(m) for m in modes]
        if len(modes) != len(lists):
            raise ValueError("one mode per list")
        norm = []
        for l, m in zip(lists, modes):
            ent = sorted((int(e[0]), float(np.float32(e[1])), int(e[2]) if len(e) > 2 else 0) for e in l)
            if (len({e[0] for e in ent}) != len(ent) or any(not 0 <= e[0] < VOCAB for e in ent)
                    or any(not (e[1] == -np.inf or abs(e[1]) <= 100) for e in ent) or m not in (0, 1)
                    or (m == 1 and not any(np.isfinite(e[1]) for e in ent))):
                raise ValueError("a token twice or out of range, a bias that is neither -inf nor within 100, or an ALLOW list that allows nothing")
            norm.append(ent)
        self.bias = (norm, modes)

    def get_logit_bias(self):
        return [list(l) for l in self.bias[0]], list(self.bias[1])

    # -- guides and the stop automaton (sections 2r to 2t)
    @staticmethod
    def _starts(start):
        starts = [start] if isinstance(start, (int, np.integer)) else list(start)
        if any(s < -1 for s in starts):
            raise IndexError("a start state below -1")
        return [int(s) for s in starts]

    def set_guide(self, next, start):
        self.left_dense = None
        if next is None or np.size(next) == 0:
            self.guide = self.guide_held = None
            return
        t, starts = np.asarray(next), self._starts(start)
        S = t.shape[0]
        if (t.ndim != 2 or t.shape[1] != VOCAB or S > 4096 or not starts or t.min() < -1 or t.max() >= S or any(s >= S for s in starts)
                or not (t >= 0).any(axis=1).all()):
            raise IndexError("a table with another vocabulary, an entry or a start outside its states, or a state that allows no token")
        held = self.guide_held
        self.guide = self.guide_held = Guide("dense", t, starts)
        if self.leak == "guide_table_stale" and held is not None and held.kind == "dense" and held.n_states == S:
            self.guide_held = Guide("dense", held.next, starts)

    def set_guide_sparse(self, default, offsets, tokens, targets, start):
        if default is None or np.size(default) == 0:
            self.guide = self.guide_held = self.left_dense = None
            return
        starts = self._starts(start)
        check_sparse_arrays(default, offsets, tokens, targets, starts, VOCAB, False)
        self.left_dense = self.guide if self.leak == "guide_both_forms" and self.guide is not None and self.guide.kind == "dense" else None
        self.guide = self.guide_held = Guide("sparse", (default, offsets, tokens, targets), starts)

    left_dense = None

    def get_guide(self):
        g = self.left_dense or self.guide
        return (g.next, list(g.starts)) if g is not None and g.kind == "dense" else (None, [])

    def get_guide_sparse(self):
        g = self.guide
        return (g.default, g.offsets, g.tokens, g.targets, list(g.starts)) if g is not None and g.kind == "sparse" else (None, None, None, None, [])

    def set_stop_sequences(self, automaton, start=None):
        if automaton is None:
            self.stopa = None
            return
        starts = self._starts(automaton.start if start is None else start)
        check_sparse_arrays(automaton.default, automaton.offsets, automaton.tokens, automaton.targets, starts, int(getattr(automaton, "vocab_size", VOCAB)), True)
        self.stopa = (automaton, starts)

    def get_stop_sequences(self):
        return (None, []) if self.stopa is None else (self.stopa[0], list(self.stopa[1]))

    def _guide_now(self):
        """the guide the loops run under"""
        return self.left_dense or self.guide_held

    def read_gen_logprobs(self, n_per_row=None):
        import score_top_ref
        g = self.gen
        if g is None:
            raise IndexError("the last generate_many call left no records")
        want = g["got"] if n_per_row is None else [int(v) for v in n_per_row]
        if len(want) != len(g["cap"]) or any(w < 0 or w > c for w, c in zip(want, g["cap"])):
            raise IndexError("n_per_row")
        k, out, at = g["k"], [], 0
        tops = g["tops"].reshape(-1, k) if k else np.zeros((sum(g["cap"]), 0), dtype=score_top_ref.DTYPE)
        for c, w in zip(g["cap"], want):
            out.append((g["recs"][at:at + w].copy(), tops[at:at + w].copy(), g["ranks"][at:at + w].copy() if k > 0 else g["ranks"][:0].copy()))
            at += c
        return out

    # -- state
    def _cache(self, cid):
        return self.single if cid == "single" else self.slots[cid]

    def _touch(self, cid, lo, hi):
        if self.touched.get(cid) != "all":
            a, b = self.touched.get(cid, (lo, hi))
            self.touched[cid] = (min(a, lo), max(b, hi))

    def _feed(self, cid, tok, pos):
        """forward(tok, pos) over that cache: the node of its history with tok behind it; the row is written"""
        c = self._cache(cid)
        assert len(c.hist) >= pos, f"the model does not know rows {len(c.hist)} .. {pos - 1} of cache {cid}"
        if len(c.hist) > pos:
            c.hist = c.hist[:pos]
            c.node = self.ref.node(c.hist)
        c.node = self.ref.child(c.node, tok)
        c.hist.append(tok)
        c.K[:, pos], c.V[:, pos] = c.node.k, c.node.v
        self._touch(cid, pos, pos + 1)
        return c.node

    def _check_tokens(self, tokens):
        if any(t < 0 or t >= VOCAB for t in tokens):
            raise IndexError("token outside the vocabulary")

    def _sdraw(self, logits):
        tok, self.srng = self.ref.draw(logits, self.sT, self.sP, self.srng, self.k_top)
        return tok

    # -- the single stream
    def forward(self, token, pos):
        self._check_tokens([token])
        if pos >= SEQ:
            raise IndexError("position out of range")
        return self._feed("single", token, pos).logits.copy()

    def generate_greedy(self, first, pos, n):
        out, tok = [], first
        for i in range(n):
            tok = self._sdraw(self._feed("single", tok, pos + i).logits)
            out.append(tok)
        return out

    def prefill(self, tokens, pos=0, batched=False):
        self._check_tokens(tokens)
        if pos + len(tokens) > SEQ:
            raise IndexError("the prompt ends past the context")
        for i, t in enumerate(tokens):
            tok = self._sdraw(self._feed("single", t, pos + i).logits)        # one (discarded) sample per prompt position
        return tok

    def _verify(self, tokens, pos):
        self._check_tokens(tokens)
        if not 1 <= len(tokens) <= COLS_MAX or pos + len(tokens) > SEQ:
            raise IndexError("block out of range")
        c, n = self.single, len(tokens)
        keep = (c.K[:, pos:pos + n].copy(), c.V[:, pos:pos + n].copy())
        logits, nxt = [], []
        for i, t in enumerate(tokens):
            lg = self._feed("single", t, pos + i).logits
            logits.append(lg)
            nxt.append(self.ref.draw(lg, self.sT, self.sP, xorshift(self.srng, i) if self.sT > 0 else 0, self.k_top)[0])
        a = 0
        while a + 1 < n and tokens[a + 1] == nxt[a]:
            a += 1
        c.K[:, pos + a + 1:pos + n], c.V[:, pos + a + 1:pos + n] = keep[0][:, a + 1:], keep[1][:, a + 1:]
        c.hist = c.hist[:pos + a + 1]
        c.node = self.ref.node(c.hist)
        self.touched["single"] = (pos, pos + a + 1)
        if self.sT > 0:
            self.srng = xorshift(self.srng, a + 1)
        return nxt, a, np.stack(logits)

    def verify(self, tokens, pos, want_logits=True):
        if self.sT > 0:
            raise Refused(-5, "greedy only")
        return self._verify(tokens, pos)

    def verify_draw(self, tokens, pos, want_logits=True):
        return self._verify(tokens, pos)

    def generate_lookup(self, corpus, first, pos, n, ngram=2, draft_len=8):
        if self.sT > 0:
            raise Refused(-5, "greedy only")
        return self.generate_greedy(first, pos, n), None

    def generate_lookup_draw(self, corpus, first, pos, n, ngram=2, draft_len=8):
        return self.generate_greedy(first, pos, n), None

    def set_sampler(self, T, P, seed):
        self.sT, self.sP, self.srng = T, P, seed

    def sampler_rng_state(self):
        return self.srng

    def reset_kv(self):
        self.single = _Cache(self.ref, SEQ)
        self.touched["single"] = "all"

    def read_state(self, kind):
        return (self.single.K if kind == "key" else self.single.V).reshape(-1)

    # -- the batched state
    def batch_init(self, streams, ctx=0):
        self.streams, self.ctx = streams, min(ctx, SEQ) if ctx else SEQ
        self.slots = [_Cache(self.ref, self.ctx) for _ in range(streams)]
        self.bT, self.brng, self.loop_rng, self.last_cand = 0.0, [], {}, []
        self.gen, self.dev = None, {}            # the records and every buffer of the settings belong to the batched state
        if self.leak == "topk_init":
            self.k_top = 0
        if self.leak == "guide_init_dropped":
            self.guide = self.guide_held = self.left_dense = None
        if self.leak == "stop_init_dropped":
            self.stopa = None
        if self.leak != "prefix":
            self.prefix = []
        self.touched.update({s: "all" for s in range(streams)})

    def batch_read_state(self, slot, kind):
        return (self.slots[slot].K if kind == "key" else self.slots[slot].V).reshape(-1)

    def set_batch_sampler(self, T, P, seeds):
        self.bT, self.bP, self.brng = T, P, [int(s) for s in seeds][:self.streams]

    def batch_reset_kv(self):
        for s in range(self.streams):
            old = self.slots[s]
            self.slots[s] = _Cache(self.ref, self.ctx)
            if self.leak == "length":
                n = len(old.hist)
                self.slots[s].K[:, :n], self.slots[s].V[:, :n] = old.K[:, :n], old.V[:, :n]
            self.touched[s] = "all"

    def _bdraw(self, slot, logits):
        if not self.bT > 0:
            return self.ref.draw(logits, 0.0, 1.0, 0)[0]
        tok, self.brng[slot] = self.ref.draw(logits, self.bT, self.bP, self.brng[slot], self.k_top)
        return tok

    def _batch_args(self, tokens, pos):
        if not 1 <= len(tokens) <= self.streams or any(p < 0 or p >= self.ctx for p in pos):
            raise IndexError("stream or position out of range")
        self._check_tokens(tokens)

    def forward_batch(self, tokens, pos, want_logits=True):
        self._batch_args(tokens, pos)
        logits = [self._feed(i, t, p).logits for i, (t, p) in enumerate(zip(tokens, pos))]
        return np.stack(logits), [self._bdraw(i, lg) for i, lg in enumerate(logits)]

    def generate_greedy_batch(self, first, pos, steps):
        self._batch_args(first, pos)
        out = np.zeros((len(first), steps), dtype=np.int32)
        for i, (tok, p) in enumerate(zip(first, pos)):
            for k in range(steps):
                tok = self._bdraw(i, self._feed(i, tok, p + k).logits)
                out[i, k] = tok
        return out

    def _cols(self, slots, tokens, pos, keep, draw, want_draw=False):
        if not 1 <= len(slots) <= COLS_MAX or any(s < 0 or s >= self.streams for s in slots) or any(p >= self.ctx for p in pos):
            raise IndexError("column out of range")
        self._check_tokens(tokens)
        logits, out, k = [], [], 0
        for j, (s, t, p) in enumerate(zip(slots, tokens, pos)):
            k = k + 1 if j and slots[j - 1] == s else 0
            lg = self._feed(s, t, p).logits
            logits.append(lg)
            if self.leak == "settings_touch_cols" and want_draw:
                import bias_ref
                en, mo = bias_ref.list_of(self.bias, 0)
                lg = bias_ref.rule(lg, en, mo, 0, self.dev.get("counts", {}).get(s) if any(self.pen) else None, *self.pen)
            if self.leak == "guide_touch_cols" and want_draw and self._guide_now() is not None and self._guide_now().starts[0] >= 0:
                import guide_ref
                lg = guide_ref.mask(lg, self._guide_now().row(self._guide_now().starts[0]))
            if draw and keep is not None and not keep[j]:
                out.append(-1)
            elif not draw and lg is not logits[-1]:
                import pen_ref
                out.append(pen_ref.argmax_key(lg))
            else:
                out.append(self.ref.draw(lg, self.bT if draw else 0.0, self.bP, xorshift(self.brng[s], k) if draw else 0, self.k_top)[0])
            if draw and (j + 1 == len(slots) or slots[j + 1] != s):
                self.brng[s] = xorshift(self.brng[s], k + 1)
        return np.stack(logits), out

    def batch_step_cols(self, slots, tokens, pos, want_logits=True):
        if self.bT > 0:
            raise Refused(-5, "greedy only")
        return self._cols(slots, tokens, pos, None, False)

    def batch_step_cols_draw(self, slots, tokens, pos, keep=None, want_logits=True):
        return self._cols(slots, tokens, pos, keep, self.bT > 0, True)

    def batch_prefill_slots(self, slots, prompts, first):
        if any(s < 0 or s >= self.streams for s in slots):
            raise IndexError("slot out of range")
        for p in prompts:
            self._check_tokens(p)
        for s, p, f in zip(slots, prompts, first):
            for i, t in enumerate(p):
                self._feed(s, t, f + i)
            if self.bT > 0:
                self.brng[s] = xorshift(self.brng[s], len(p))
        return _q3().dense_pack([len(p) for p in prompts], DENSE_CAP)[1]

    def _many(self, prompts, n_new, sampler, dense_min=0, stop=(), prefix=(), carry=False, sched=False):
        """sched: one of the two loops with a device scheduler, which honour the stop automaton"""
        self.gen = None                          # every loop call starts here: the records of the call before are gone
        for p in prompts:
            self._check_tokens(p)
        if sampler is None and self.bT > 0:
            raise Refused(-5, "greedy only")
        n = len(prompts)
        lists, modes = self.bias
        if len(lists) > 1 and len(lists) != n:
            raise IndexError("one list per request")
        gd, sa = self._guide_now(), self.stopa
        if any(len(s) > 1 and len(s) != n for s in ([gd.starts] if gd else []) + ([sa[1]] if sa else [])):
            raise IndexError("one start state per request")
        per = [None] * n
        if sampler is not None:
            T, P, seeds = [v if isinstance(v, (list, tuple)) else [v] * n for v in sampler]
            per = [(T[r], P[r], seeds[r]) if T[r] > 0 else None for r in range(n)]
        full = [list(prefix) + list(p) for p in prompts]
        lens = [len(p) for p in prompts]
        plan = None
        if carry and self.leak == "sampler":
            plan = many_plan(lens, n_new, self.streams)
            for s, occ in plan["occupants"].items():
                for r in occ:
                    if per[r]:
                        if s in self.loop_rng:
                            per[r] = (per[r][0], per[r][1], self.loop_rng[s])
                        self.loop_rng[s] = self.ref.generate(full[r], n_new[r], per[r])[1]
        res = self._rows(full, lens, n_new, per)
        rows = [x[0] for x in res]
        out = [cut_at_stop(r, stop) for r in rows]
        emit = None
        if sa is not None and (sched or self.leak == "stop_in_plain_loops"):
            emit = self._stop_emits(sa, [list(prefix) + list(p) for p in prompts], rows, stop, lens, n_new)
            out = [r[:k] for r, k in zip(rows, emit)]
        plan = plan or many_plan(lens, n_new, self.streams, dense_min, rows, stop, emit if sched else None)
        assert [len(r) for r in out] == list(plan["n_out"]) or self.leak == "stop_in_plain_loops"
        for s, occ in sorted(plan["occupants"].items()):
            for r in occ:
                for i, t in enumerate(full[r] + out[r][:-1]):
                    self._feed(s, t, i)
        if self.genlp >= 0:
            self._records(n_new, out, res)
        return out, plan

    def _stop_emits(self, sa, prompts, rows, stop, lens, n_new):
        """n_emit per request under the stop automaton: the smallest of the first stop token's index + 1, the first completed
        sequence's index + 1 and n_new, by stop_seq_ref's plain sub-list search over the sequences the automaton was compiled from
        (automaton.seqs; None: the automaton whose one state completes with every token)"""
        import bias_ref
        import stop_seq_ref
        a, starts = sa
        per = [starts[0] if len(starts) == 1 else starts[r] for r in range(len(rows))]
        cuts = [len(cut_at_stop(r, stop)) for r in rows]
        if self.leak == "stop_prompt_steps":
            emit = []
            for r, row in enumerate(rows):
                s = per[r]
                for t in (prompts[r] if s >= 0 else ()):
                    x = stop_next(a, s, t)
                    s = x if x >= 0 else a.start
                emit.append(min(cuts[r], stop_emit(a, s, row)[0]))
            return emit
        if self.leak == "stop_min_tokens":
            floors = [max([e[2] for e in bias_ref.list_of(self.bias, r)[0]] + [1]) for r in range(len(rows))]
            return [min(cuts[r], stop_emit(a, per[r], row, floors[r] - 1)[0]) for r, row in enumerate(rows)]
        if a.seqs is None:
            emit = [1 if per[r] >= 0 else cuts[r] for r in range(len(rows))]
        else:
            emit = stop_seq_ref.n_emit_rows(rows, a.seqs, stop, per)
        if self.leak == "stop_slot_state":
            left = self.dev.setdefault("stop_state", {})
            for s, occ in sorted(many_plan(lens, n_new, self.streams, emit=emit)["occupants"].items()):
                for r in occ:
                    use = min(left[s], a.default.size - 1) if left.get(s, -1) >= 0 and per[r] >= 0 else per[r]
                    emit[r] = min(cuts[r], stop_emit(a, use, rows[r])[0])
                    left[s] = stop_emit(a, use, rows[r][:emit[r]])[1]
        return emit

    def _rows(self, full, lens, n_new, per):
        """Reference.generate per request under the settings: (tokens, rng state, nodes, record rows) each"""
        import bias_ref
        lists, modes = self.bias
        pen = any(self.pen)
        n = len(full)
        gd = self._guide_now()
        self._gctx = None
        if gd is not None:
            starts = [gd.starts[0] if self.leak == "guide_start_shared" else gd.start_of(r) for r in range(n)]
            self._gctx = dict(guide=gd, start=starts, g0=[None] * n)
            if self.leak == "guide_slot_state":
                left = self.dev.setdefault("guide_state", {})
                for s, occ in sorted(many_plan(lens, n_new, self.streams)["occupants"].items()):
                    for r in occ:
                        if left.get(s, -1) >= 0 and starts[r] >= 0:
                            self._gctx["g0"][r] = min(left[s], gd.n_states - 1)
                        got = self._one(full[r], n_new[r], per[r], bias_ref.list_of(self.bias, r), None, None, r)[0]
                        left[s] = gd.state_of(starts[r] if self._gctx["g0"][r] is None else self._gctx["g0"][r], got)
        tables = [bias_ref.list_of(self.bias, r) for r in range(n)]
        if self.leak == "bias_stale" and lists:
            # the flat entries of this table over what the buffer held: the tail of the longer table before stands behind the last list
            flat = [e for l in lists for e in l]
            old = self.dev.get("bias_flat", [])
            self.dev["bias_flat"] = flat + old[len(flat):]
            have = {e[0] for e in lists[-1]}
            tail = []
            for e in old[len(flat):]:
                if e[0] not in have:
                    have.add(e[0])
                    tail.append(e)
            if tail:
                last = len(lists) - 1
                tables = [(sorted(list(en) + tail), mo) if (len(lists) == 1 or r == last) else (en, mo) for r, (en, mo) in enumerate(tables)]
        per_g = [None] * n
        o_off = [sum(n_new[:r]) for r in range(n)]
        if self.leak == "bias_ooff" and lists:
            prev = self.dev.get("o_off")
            if prev:
                for r in range(n):
                    found = []
                    for g in range(n_new[r]):
                        o = o_off[r] + g
                        q = max(i for i, v in enumerate(prev) if v <= o)
                        en, mo = bias_ref.list_of(self.bias, min(q, len(lists) - 1))
                        found.append((tuple(en), mo, o - prev[q]))
                    per_g[r] = tuple(found)
            self.dev["o_off"] = o_off
        counts0 = [None] * n
        if pen and self.leak in ("pen_counts", "pen_prompt"):
            left = self.dev.setdefault("counts", {})
            for s, occ in sorted(many_plan(lens, n_new, self.streams)["occupants"].items()):
                for r in occ:
                    if self.leak == "pen_prompt":
                        c = {}
                        for t in full[r][len(full[r]) - lens[r]:]:
                            c[t] = c.get(t, 0) + 1
                    else:
                        c = dict(left.get(s, {}))
                    counts0[r] = tuple(sorted(c.items()))
                    got = self._one(full[r], n_new[r], per[r], tables[r], per_g[r], counts0[r], r)[0]
                    for t in got:
                        c[t] = c.get(t, 0) + 1
                    left[s] = c
        res = [self._one(full[r], n_new[r], per[r], tables[r], per_g[r], counts0[r], r) for r in range(n)]
        if pen and self.leak == "settings_touch_cols":          # the counts that leak keeps per slot: the last occupant's
            cs = self.dev.setdefault("counts", {})
            for s, occ in many_plan(lens, n_new, self.streams)["occupants"].items():
                c = np.zeros(VOCAB, dtype=np.uint32)
                for t in res[occ[-1]][0]:
                    c[t] += 1
                cs[s] = c
        return res

    def _one(self, prompt, n_new, sampler, table, per_g, counts0, r=None):
        dev = ()
        if per_g:
            dev += (("per_g", per_g),)
        if counts0:
            dev += (("counts0", counts0),)
        if self.leak == "genlp_penalised" and self.genlp >= 0:
            dev += (("adjusted",),)
        guide, start = None, -1
        if self._gctx is not None and self._gctx["start"][r] >= 0:
            guide, start = self._gctx["guide"], self._gctx["start"][r]
            if self._gctx["g0"][r] is not None:
                dev += (("g0state", self._gctx["g0"][r]),)
            if self.leak == "guide_y0_raw":
                dev += (("y0_raw",),)
            if self.leak == "guide_records_masked" and self.genlp >= 0:
                dev += (("masked_records",),)
        return self.ref.generate(prompt, n_new, sampler, self.k_top if sampler else 0, self.pen[0], self.pen[1], tuple(tuple(e) for e in table[0]), table[1], dev,
                                 guide, start)

    _gctx = None

    def _records(self, n_new, out, res):
        """the record buffers of the call as read_gen_logprobs finds them: indexed as the output tokens, cleared in front of the call"""
        import score_ref
        import score_top_ref as tr
        k, total = self.genlp, sum(n_new)
        old = self.dev.get("genlp") if self.leak == "genlp_stale" else None
        recs, tops, ranks = np.zeros(total, dtype=score_ref.DTYPE), np.zeros(total * k, dtype=tr.DTYPE), np.zeros(total, dtype=np.int32)
        if old:
            for new, was in zip((recs, tops, ranks), old):
                m = min(new.size, was.size)
                new[:m] = was[:m]
        at = 0
        last = []
        for r, row in enumerate(out):
            _, _, nodes, adj = res[r]
            for j, tok in enumerate(row):
                l = nodes[j].logits if adj[j] is None else adj[j]
                recs[at + j] = self.ref.record(nodes[j], tok) if adj[j] is None else score_ref.record(l, tok)
                if k:
                    tops[(at + j) * k:(at + j + 1) * k] = tr.top(l, k)
                    ranks[at + j] = tr.rank(l, tok)
            last.append(nodes[len(row) - 1])
            at += n_new[r]
        self.gen = dict(k=k, cap=[int(v) for v in n_new], got=[len(r) for r in out], recs=recs, tops=tops, ranks=ranks)
        self.dev["genlp"] = (recs, tops, ranks)
        self.dev["loop_last"] = last if k else None          # the rows of the loop's last columns, whose part lists a leak hands on

    def generate_many_greedy(self, prompts, n_new):
        out, plan = self._many(prompts, n_new, None)
        return out, plan["stats"]

    def generate_many_sampled(self, prompts, n_new, T, P, seeds):
        out, plan = self._many(prompts, n_new, (T, P, seeds), carry=True)
        return out, plan["stats"]

    def generate_many_dense(self, prompts, n_new, sampler=None, dense_min=64):
        out, plan = self._many(prompts, n_new, sampler, dense_min)
        live = sum(sum(b[2]) for b in plan["blocks"])
        return out, plan["stats"], _q3().DenseStats(len(plan["blocks"]), live, sum(b[0] for b in plan["blocks"]) - live)

    @staticmethod
    def _raw(out, n_new, stats, raw):
        """raw: (the output buffer as the library fills it -- -1 behind every request's last token --, n_out, stats)"""
        if not raw:
            return out, stats
        buf = [t for row, k in zip(out, n_new) for t in list(row) + [-1] * (k - len(row))]
        return buf, [len(r) for r in out], stats

    def generate_many_stop(self, prompts, n_new, stop_tokens, sampler=None, raw=False):
        out, plan = self._many(prompts, n_new, sampler, 0, tuple(stop_tokens), sched=True)
        return self._raw(out, n_new, plan["stats"], raw)

    def generate_many_prefix(self, suffixes, n_new, stop_tokens=(), sampler=None, raw=False):
        if not self.prefix:
            raise IndexError("no resident prefix")
        out, plan = self._many(suffixes, n_new, sampler, 0, tuple(stop_tokens), self.prefix, sched=True)
        return self._raw(out, n_new, plan["stats"], raw)

    def batch_copy_rows(self, src, dst, first, n):
        if not 1 <= len(dst) <= self.streams - 1 or any(s < 0 or s >= self.streams or s == src for s in dst) or first + n > self.ctx:
            raise IndexError("slot or rows out of range")
        a = self.slots[src]
        assert len(a.hist) >= first + n, "the model does not know the rows it copies"
        for s in dst:
            c = self.slots[s]
            assert c.hist[:first] == a.hist[:first], "the model does not know what the copied rows stand behind"
            c.K[:, first:first + n], c.V[:, first:first + n] = a.K[:, first:first + n], a.V[:, first:first + n]
            c.hist = a.hist[:first + n]
            c.node = self.ref.node(c.hist)
            self._touch(s, first, first + n)

    def batch_prefix_set(self, tokens):
        self._check_tokens(tokens)
        for i, t in enumerate(tokens):
            self._feed(0, t, i)
        self.prefix = list(tokens)

    def batch_prefix_get(self):
        return list(self.prefix)

    def embed_many(self, prompts, normalize=True, out_dim=None, use_prefix=False):
        import embed_ref
        for p in prompts:
            self._check_tokens(p)
        if use_prefix and not self.prefix:
            raise IndexError("no resident prefix")
        nodes, st = self._walk(prompts, use_prefix)
        rows = np.stack([n[-1].x for n in nodes])
        out = embed_ref.l2(rows, out_dim) if normalize else rows[:, :out_dim or DIM].copy()
        return out, st

    def _walk(self, prompts, use_prefix, coins=False):
        """q3_embed_many's walk: request r goes through slot r % streams from position 0 (behind the prefix).  Returns, per request, the
        nodes of its own tokens, and the EmbedStats of the schedule"""
        P = len(self.prefix) if use_prefix else 0
        nodes = []
        for r, p in enumerate(prompts):
            s = r % self.streams
            got = [self._feed(s, t, i) for i, t in enumerate((self.prefix if use_prefix else []) + list(p))]
            nodes.append(got[P:])
            if coins and self.leak == "slot_rng" and self.brng:
                self.brng[s] = xorshift(self.brng[s], len(p))
        waves = [[len(p) for p in prompts[i:i + self.streams]] for i in range(0, len(prompts), self.streams)]
        st = [_q3().dense_pack(w, DENSE_CAP)[1] for w in waves]
        return nodes, _q3().EmbedStats(len(waves), sum(s.blocks for s in st), sum(s.live_columns for s in st), sum(s.pad_columns for s in st))

    def choice_many(self, prompts, candidates, use_prefix=False):
        cands = [list(c) if hasattr(c, "__len__") else c for c in candidates]
        per_request = len(cands) > 0 and all(isinstance(c, list) for c in cands)
        k = len(cands[0]) if per_request else len(cands)
        flat = [t for c in cands for t in c] if per_request else cands
        if not 1 <= k <= 256 or (per_request and (len(cands) != len(prompts) or any(len(c) != k for c in cands))):
            raise IndexError("k out of range, or not one list of k candidates per prompt")
        self._check_tokens(flat)
        for p in prompts:
            self._check_tokens(p)
        if not prompts or any(len(p) == 0 for p in prompts) or (use_prefix and not self.prefix):
            raise IndexError("an empty prompt, or no resident prefix")
        if self.leak == "stale_cand":       # the ids already in the device buffer are not uploaded again
            flat = self.last_cand[:len(flat)] + flat[len(self.last_cand):]
        self.last_cand = list(flat)
        nodes, st = self._walk(prompts, use_prefix, coins=True)
        out = np.stack([n[-1].logits[flat[r * k:(r + 1) * k] if per_request else flat] for r, n in enumerate(nodes)])
        return out.astype(np.float32, copy=False), st

    def score_many(self, prompts, score_from=None, use_prefix=False):
        import score_ref
        lens = [len(p) for p in prompts]
        sf = [1] * len(lens) if score_from is None else list(score_from)
        if not prompts or len(sf) != len(lens) or any(n == 0 or f < 1 or f > n for n, f in zip(lens, sf)) or (use_prefix and not self.prefix):
            raise IndexError("an empty prompt, score_from out of range, or no resident prefix")
        for p in prompts:
            self._check_tokens(p)
        nodes, st = self._walk(prompts, use_prefix, coins=True)
        out = [np.array([self.ref.record(n[i], p[i + 1]) for i in range(f - 1, len(p) - 1)], dtype=score_ref.DTYPE).reshape(len(p) - f)
               for p, n, f in zip(prompts, nodes, sf)]
        sched = score_ref.schedule(lens, sf, self.streams, DENSE_CAP)
        assert sched[:4] == (st.waves, st.blocks, st.live_columns, st.pad_columns), (sched, st)
        return out, _q3().ScoreStats(*sched)


    def score_top_many(self, prompts, k, score_from=None, use_prefix=False):
        import score_top_ref as tr
        if not 1 <= k <= 64:
            raise IndexError("k out of range")
        recs, st = self.score_many(prompts, score_from, use_prefix)
        sf = [1] * len(prompts) if score_from is None else list(score_from)
        P = len(self.prefix) if use_prefix else 0
        tops, ranks, seen = [], [], 0
        shared = self.dev.pop("loop_last", None) if self.leak == "score_top_shared" else None
        for r, (p, f) in enumerate(zip(prompts, sf)):
            nodes = self.ref._path(self.ref.node((self.prefix if use_prefix else []) + list(p)))[P:]
            rows = [nodes[i].logits for i in range(f - 1, len(p) - 1)]
            if shared:
                rows = [shared[(seen + i) % len(shared)].logits if seen + i < SCORE_COLS else l for i, l in enumerate(rows)]
            seen += len(rows)
            tops.append(np.stack([tr.top(l, k) for l in rows]) if rows else np.zeros((0, k), dtype=tr.DTYPE))
            ranks.append(np.array([tr.rank(l, p[f + i]) for i, l in enumerate(rows)], dtype=np.int32))
        return recs, tops, ranks, st


# ---------------------------------------------------------------------------------------------------------------------------------
# running a sequence
# ---------------------------------------------------------------------------------------------------------------------------------
def _requests(op, ref, prefix, top_k=0, pen=(0.0, 0.0)):
    """prompts, n_new, the sampler triple or None, and the stop tokens of a loop op.  A stop token is a token of a request's own row
    as the settings in force give it with no table set (a table is derived from those rows and from these stop tokens: Tables)"""
    reqs = [CAT[i] for i in op["reqs"]]
    prompts = [toks((k, n)) for k, n, *_ in reqs]
    n_new = [c[2] for c in reqs]
    sampled = op["op"] == "generate_many_sampled" or op.get("sampled")
    sampler = ([c[3] for c in reqs], [c[4] for c in reqs], [c[5] for c in reqs]) if sampled else None
    stop = []
    for i, j in op.get("stop_at", ()):
        k, n, nn, T, P, seed = CAT[i]
        smp = (T, P, seed) if sampled and T > 0 else None
        row = ref.generate(tuple(list(prefix) + toks((k, n))), nn, smp, top_k if smp else 0, pen[0], pen[1])[0]
        if row[j] not in stop:
            stop.append(row[j])
    return prompts, n_new, sampler, stop


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine-wide settings along a sequence, and the tables of its set_logit_bias ops
# ---------------------------------------------------------------------------------------------------------------------------------
def settings_walk(ops):
    """per op what is in force in front of it: dict(top_k, genlp, pen, table = the index of the set_logit_bias op whose table holds or
    None, prefix = the resident prefix as a PREFIXES entry or None, streams).  A refused call changes nothing."""
    st = dict(top_k=0, genlp=-1, pen=(0.0, 0.0), table=None, prefix=None, streams=0, guide=None, gform=None, stop=None)
    out = []
    for i, op in enumerate(ops):
        out.append(dict(st))
        k = op["op"]
        if k in ("set_guide", "set_guide_sparse"):           # guide, stop: the index of the setter op whose automaton holds, or None;
            on = op["form"] != "off"                         # gform: which of the two guide forms; setting either clears the other
            st["guide"], st["gform"] = (i, "dense" if k == "set_guide" else "sparse") if on else (None, None)
        elif k == "set_stop_seq":
            st["stop"] = i if op["form"] != "off" else None
        if k == "set_top_k":
            st["top_k"] = op["k"]
        elif k == "set_gen_logprobs":
            st["genlp"] = op["n"]
        elif k == "set_penalties":
            st["pen"] = (float(np.float32(op["p"])), float(np.float32(op["f"])))
        elif k == "set_logit_bias":
            st["table"] = None if op["form"] == "off" else i
        elif k == "batch_prefix_set":
            st["prefix"] = op["prompt"]
        elif k == "batch_init":
            st["prefix"], st["streams"] = None, op["streams"]
    return out


BIAS_SIZES = {"one": 40, "big": 320, "add": 5, "allow": 3, "kill": 3, "min": 4}     # entries per list: static, so that needs() knows them without an oracle
NEG_INF = float("-inf")


def table_lens(op):
    """the list lengths and modes of a set_logit_bias op: per request ALLOW (three tokens) and ADD lists in turn"""
    if op["form"] == "off":
        return [], []
    if op["form"] in ("one", "big", "kill", "min"):          # (kill, min: the two lists of the guide sequences, see Tables.get)
        return [BIAS_SIZES[op["form"]]], [0]
    modes = [(r + op["par"]) % 2 for r in range(op["n"])]
    return [BIAS_SIZES["allow"] if m else BIAS_SIZES["add"] for m in modes], modes


GUIDE_BIG = {1: 1024, 2: 1536}                   # the states of the dense form "big" by op["size"]: guide_next grows twice
SPARSE_BIG = {1: (64, 128), 2: (128, 256)}       # (states, edges per state) of the sparse form "big"
STOP_BIG = {1: 150, 2: 300}                      # the sequences of the stop form "big" that never complete


def cycle_small(seed):
    """the three tokens the small state of a cycle allows, from the seed alone: a "kill" table bans exactly these"""
    return sorted(random.Random(seed ^ 0x5A5A).sample(range(1, VOCAB - 1), 3))


def guide_arrays(dense, form, seed, forbid, size=1, ns=None):
    """(n_states, the arrays of a guide form): next[n_states][V] for a dense guide, (default, offsets, tokens, targets) for a sparse
    one -- through SparseAutomaton.from_dense for the forms both have.  forbid: tokens no state allows (but a cycle's small state,
    whose three tokens come from the seed alone); ns: the states of a cycle, where the op fixes them."""
    from qwen3_rs_amd.guide import Automaton, SparseAutomaton
    V = VOCAB
    rng, r = np.random.default_rng(seed), random.Random(seed)
    forbid = np.array(sorted(forbid), dtype=np.int64)
    ok = np.ones(V, dtype=bool)
    ok[forbid] = False
    if not dense and form in ("dflt", "half", "big"):
        if form == "dflt":                       # s0: all but `forbid`; s1: no edges, everything allowed; s2: three tokens, the rest forbidden by default
            rows = [(1, forbid, np.full(forbid.size, -1)), (2, forbid[:0], forbid[:0]), (-1, np.array(cycle_small(seed)), np.zeros(3, dtype=np.int64))]
        elif form == "half":                     # s0: allowed by default, about V/2 forbidding edges with 0 and V - 1 among them; s1: no edges
            ban = np.zeros(V, dtype=bool)
            ban[rng.choice(V, V // 2, replace=False)] = True
            ban[[0, V - 1]] = True
            ban[forbid] = True
            t = np.flatnonzero(ban)
            rows = [(1, t, np.full(t.size, -1)), (0, forbid[:0], forbid[:0])]
        else:                                    # a chain of states, each with its own few allowed tokens
            S, K = SPARSE_BIG[size]
            pool = np.flatnonzero(ok)
            rows = [(-1, np.sort(rng.choice(pool, K, replace=False)), np.full(K, (s + 1) % S)) for s in range(S)]
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum([t.size for _, t, _ in rows], out=off[1:])
        return len(rows), (np.array([d for d, _, _ in rows], dtype=np.int32), off, np.concatenate([t for _, t, _ in rows]).astype(np.int32),
                           np.concatenate([x for _, _, x in rows]).astype(np.int32))
    if form == "all":                            # two states, everything allowed: the masked form on the raw row
        nxt = np.zeros((2, V), dtype=np.int16)
        nxt[0] = 1
    elif form == "trie":                         # three labels of 2, 3 and 4 tokens, then eos, then a free state
        firsts = r.sample([t for t in range(V - 1) if ok[t]], 3)
        labels = [[f] + [r.randrange(V - 1) for _ in range(n - 1)] for f, n in zip(firsts, (2, 3, 4))]
        nxt = Automaton.from_sequences(labels, V, V - 1).next.copy()
        nxt[-1] = nxt.shape[0] - 1
    elif form in ("cycle", "per"):               # 3 to 5 states of about V/2, V/16, 3, V/2 .. allowed tokens, each leading to the next
        n = ns or r.choice((3, 4, 5))
        nxt = np.full((n, V), -1, dtype=np.int16)
        for s in range(n):
            allow = np.zeros(V, dtype=bool)
            if s == 2:
                allow[cycle_small(seed)] = True
            else:
                allow[rng.choice(V, V // 16 if s == 1 else V // 2, replace=False)] = True
                allow[0], allow[V - 1] = s == 1, s == 0         # 0 only in state 1, V - 1 only in state 0
                allow &= ok
            nxt[s, allow] = (s + 1) % n
    elif form == "big":
        S = GUIDE_BIG[size]
        allow = (rng.random((S, V)) < 0.5) & ok
        nxt = np.where(allow, ((np.arange(S) + 1) % S)[:, None], -1).astype(np.int16)
    else:
        raise ValueError(form)
    if dense:
        return nxt.shape[0], nxt
    a = SparseAutomaton.from_dense(Automaton(nxt))
    return a.n_states, (a.default, a.offsets, a.tokens, a.targets)


class Tables:
    """The tables of the set_logit_bias ops of a sequence, from Reference alone, so that they bind on any logits: every loop op that
    runs under a table finds, for every one of its requests, a token banned that the request produces without the table (under the
    other settings in force, in front of its first stop token) -- for good ({tok, -inf, 0}) or up to that output (the min_tokens form
    {tok, -inf, g + 1}) -- or an allowed list of three tokens that holds none of its first tokens.  The lists are filled up to the
    static lengths of table_lens with seeded tokens of bias +0, -0, a small finite one or -inf, some with until > 0."""

    def __init__(self, ops, ref):
        self.ops, self.ref, self.st, self.memo = ops, ref, settings_walk(ops), {}
        self.gmemo, self.smemo = {}, {}

    def users(self, i, what="table"):
        return [j for j in range(i + 1, len(self.ops)) if self.ops[j]["op"] in MANY and self.st[j][what] == i]

    def plain_rows(self, j):
        """the requests of loop op j with no table and no guide set: per request the row cut at its first stop token"""
        return self.rows(j, table=False, guide=False)

    def rows(self, j, table=True, guide=True, cut=True, **other):
        """The rows of loop op j by Reference alone, each cut at its first stop token (cut False: whole), under the settings in
        force in front of it; table False: with no table set; guide False: with no guide set; other: top_k or pen replaced.  The
        stop tokens are the op's own in every case.  The stop automaton is not applied: emits() is."""
        op, st = self.ops[j], self.st[j]
        prefix = toks(st["prefix"]) if op["op"] == "generate_many_prefix" else []
        prompts, n_new, sampler, stop = _requests(op, self.ref, prefix, st["top_k"], st["pen"])
        st = dict(st, **other)
        lists = self.get(st["table"]) if table and st["table"] is not None else ([], [])
        gd = self.guide(st["guide"]) if guide and st["guide"] is not None else None
        import bias_ref
        rows = []
        for r, p in enumerate(prompts):
            smp = (sampler[0][r], sampler[1][r], sampler[2][r]) if sampler and sampler[0][r] > 0 else None
            en, mo = bias_ref.list_of(lists, r)
            row = self.ref.generate(tuple(prefix + p), n_new[r], smp, st["top_k"] if smp else 0, st["pen"][0], st["pen"][1], tuple(tuple(e) for e in en), mo, (),
                                    gd, gd.start_of(r) if gd else -1)[0]
            rows.append(cut_at_stop(row, stop) if cut else row)
        return rows

    def stop_tokens(self, j):
        op, st = self.ops[j], self.st[j]
        return _requests(op, self.ref, toks(st["prefix"]) if op["op"] == "generate_many_prefix" else [], st["top_k"], st["pen"])[3]

    def emits(self, j):
        """n_emit per request of loop op j: under a stop automaton, in the two loops that honour it, the smallest of the first stop
        token's index + 1, the first completed sequence's index + 1 (stop_seq_ref) and n_new; else the cut at the stop tokens"""
        import stop_seq_ref
        op, st = self.ops[j], self.st[j]
        whole = self.rows(j, cut=False)
        stop = self.stop_tokens(j) if op["op"] in ("generate_many_stop", "generate_many_prefix") else []
        if st["stop"] is None or op["op"] not in ("generate_many_stop", "generate_many_prefix"):
            return [len(cut_at_stop(r, stop)) for r in whole]
        a, starts = self.stop(st["stop"])
        per = [starts[0] if len(starts) == 1 else starts[r] for r in range(len(whole))]
        if a.seqs is None:
            return [1 if s >= 0 else len(cut_at_stop(r, stop)) for r, s in zip(whole, per)]
        return stop_seq_ref.n_emit_rows(whole, a.seqs, stop, per)

    def seq_emits(self, j):
        """per request of loop op j the index + 1 of the first token that completes a sequence of the stop automaton in force, by
        stop_seq_ref alone; n_new where none does, the request has no stop sequences or the loop does not honour the automaton"""
        import stop_seq_ref
        op, st = self.ops[j], self.st[j]
        whole = self.rows(j, cut=False)
        if st["stop"] is None or op["op"] not in ("generate_many_stop", "generate_many_prefix"):
            return [len(r) for r in whole]
        a, starts = self.stop(st["stop"])
        per = [starts[0] if len(starts) == 1 else starts[r] for r in range(len(whole))]
        return [len(row) if s < 0 else 1 if a.seqs is None else stop_seq_ref.n_emit_seqs(row, a.seqs) for row, s in zip(whole, per)]

    # -- the guides (sections 2r and 2s): from the op's seed, and from the first tokens its users' requests produce with no guide set
    # (under the table and the other settings in force), which no state allows: every guided request's row differs from its unguided one
    def guide(self, i):
        if i not in self.gmemo:
            op = self.ops[i]
            dense = op["op"] == "set_guide"
            forbid = sorted({row[0] for j in self.users(i, "guide") for row in self.rows(j, guide=False, cut=False)})
            n_states, arrays = guide_arrays(dense, op["form"], op["seed"], forbid, op.get("size", 1), op.get("ns"))
            r = random.Random(op["seed"] + 1)
            if op["form"] == "per":              # one request unguided, the others in the cycle's states 0 and 1 in turn
                free = r.randrange(op["n"])          # (n >= 3: both states remain among the others)
                starts = [k % 2 for k in range(op["n"] - 1)]
                starts.insert(free, -1)
            elif op["form"] == "big":            # one start per request: guide_start grows with the request list
                starts = [k % min(n_states, 7) for k in range(op["n"])]
            else:
                starts = [0]
            self.gmemo[i] = Guide("dense" if dense else "sparse", arrays, starts)
        return self.gmemo[i]

    # -- the stop automata (section 2t): sequences taken from the rows the reference gives the requests of the op's users
    def stop(self, i):
        if i not in self.smemo:
            self.smemo[i] = self._stop(i)
        return self.smemo[i]

    def _stop(self, i):
        import stop_seq_ref
        from qwen3_rs_amd.guide import SparseAutomaton
        from qwen3_rs_amd.stops import stop_automaton
        op = self.ops[i]
        form, n = op["form"], op.get("n", 1)
        rng = random.Random(op["seed"])
        users = self.users(i, "stop")
        used = [(self.rows(j, cut=False), self.rows(j)) for j in users]          # whole rows, and the rows cut at the stop tokens
        prompts = [_requests(self.ops[j], self.ref, [], self.st[j]["top_k"], self.st[j]["pen"])[0] for j in users]
        every = [row for whole, _ in used for row in whole]
        produced = {t for row in every for t in row}

        def unseen(k):
            """k tokens no request produces"""
            out = []
            while len(out) < k:
                t = rng.randrange(VOCAB)
                if t not in produced:
                    out.append(t)
            return out

        def hit(whole, cut, r, K, early=False):
            """K tokens of request r that complete strictly inside its cap: in front of its first stop token where there is room"""
            row = whole[r]
            cand = [g for g in range(K - 1, len(row) - 1)]
            front = [g for g in cand if g + 1 < len(cut[r])]
            cand = front or cand
            if not cand:
                return None
            g = min(cand) if early else rng.choice(cand)
            return tuple(row[g - K + 1:g + 1])

        starts = [0]
        if form == "any":                        # one state, dflt -1, no edges: every token completes a sequence
            a = SparseAutomaton([-1], [0, 0], [], [], 0, VOCAB, dead_ok=True)
            a.seqs = None
            return a, starts
        seqs = []
        if form in ("hit1", "hit2", "hit3"):
            K = int(form[3])
            seqs = [hit(whole, cut, rng.randrange(len(whole)), K, op.get("early", False)) for whole, cut in used]
        elif form == "overlap":
            # A = [a, b, x] never completes (x is produced nowhere); B = [b, c] completes behind a, b, where the automaton stands two
            # tokens deep in A and takes the fall-back edge to B's first state
            for whole, cut in used:
                cand = [(r, g) for r, row in enumerate(whole) for g in range(2, len(row) - 1)
                        if len({row[g - 2], row[g - 1], row[g]}) == 3 and stop_seq_ref.n_emit_seqs(row, [row[g - 1:g + 1]]) == g + 1]
                cand = [(r, g) for r, g in cand if g + 1 <= len(cut[r])] or cand
                if cand:
                    r, g = rng.choice(cand)
                    a_, b_, c_ = whole[r][g - 2:g + 1]
                    seqs += [(a_, b_, unseen(1)[0]), (b_, c_)]
        elif form == "per":                      # one start per request, one of them -1: that request has no stop sequences
            starts = [0] * n
            starts[rng.randrange(n)] = -1
            seqs = [hit(whole, cut, r, rng.choice((1, 2))) for whole, cut in used for r in range(len(whole))]
        elif form == "big":                      # many sequences no request produces, and one that hits per user
            starts = [0] * n
            seqs = [tuple(unseen(3)) for _ in range(STOP_BIG[op.get("size", 1)])] + [hit(whole, cut, rng.randrange(len(whole)), 2) for whole, cut in used]
        seqs = sorted({q for q in seqs if q})
        if form in ("hit2", "hit3", "overlap", "per", "big"):
            # baits, which no request produces and a correct engine never completes: (the last token of a request's prompt, its first
            # output) ends the request at y_0 where prompt tokens move the state; (the last token of request a, the first output of
            # request b) ends b at y_0 where b takes a's slot and finds the state a left
            baits = set()
            for (whole, cuts), ps in zip(used, prompts):
                baits |= {(p[-1], row[0]) for p, row in zip(ps, whole)}
                baits |= {(x[-1], y[0]) for rows in (whole, cuts) for i, x in enumerate(rows) for k, y in enumerate(rows) if i != k}
            seqs = sorted(set(seqs) | {q for q in baits if not stop_seq_ref.occurs(every, q) and not any(q[-len(s_):] == s_ for s_ in seqs if len(s_) < 2)})
        if form == "never" or not seqs:          # a sequence no request produces
            while True:
                q = (rng.randrange(VOCAB), rng.randrange(VOCAB))
                if not stop_seq_ref.occurs(every, q):
                    seqs.append(q)
                    break
        a = stop_automaton(seqs, VOCAB)
        a.seqs = [list(q) for q in seqs]
        return a, starts

    def get(self, i):
        if i not in self.memo and self.ops[i]["form"] in ("kill", "min"):
            op = self.ops[i]
            users = self.users(i)
            if op["form"] == "kill":             # the three tokens the small state of the cycle in force allows, banned for good
                g = self.ops[self.st[users[0]]["guide"]]
                ent = [(t, NEG_INF, 0) for t in cycle_small(g["seed"])]
            else:                                # min_tokens 4 for tokens no request produces: the rows stay, until > 0 stands in the list
                produced = {t for j in users for row in self.plain_rows(j) for t in row}
                rng = random.Random(op["seed"])
                ent = sorted((t, NEG_INF, 4) for t in rng.sample([t for t in range(VOCAB) if t not in produced], 4))
            self.memo[i] = ([ent], [0])
        if i not in self.memo:
            op = self.ops[i]
            lens, modes = table_lens(op)
            rng = random.Random(op["seed"])
            used = [self.plain_rows(j) for j in self.users(i)]
            lists = []
            for li, (n, mode) in enumerate(zip(lens, modes)):
                mine = [rows if len(lens) == 1 else [rows[li]] for rows in used]       # the rows this list has to bind on
                ent = {}
                if mode:                                                                  # ALLOW: none of the first tokens
                    first = {row[0] for rows in mine for row in rows}
                    while len(ent) < n:
                        t = rng.randrange(VOCAB)
                        if t not in first and t not in ent:
                            ent[t] = ((0.0, 0), (-0.0, 0), (NEG_INF, 2))[len(ent)]      # the third: allowed from output 2 on
                else:
                    for rows in mine:
                        for row in rows:
                            g = rng.randrange(len(row))
                            until = rng.choice((0, g + 1))
                            if row[g] in ent:
                                until = 0 if 0 in (until, ent[row[g]][1]) else max(until, ent[row[g]][1])
                            ent[row[g]] = (NEG_INF, until)
                    assert len(ent) <= n, f"op {i}: {len(ent)} banned tokens for a list of {n}"
                    produced = {t for rows in mine for row in rows for t in row}
                    while len(ent) < n:
                        t = rng.randrange(VOCAB)
                        if t not in ent and t not in produced:
                            ent[t] = (rng.choice((0.0, -0.0, 0.25, -0.5, NEG_INF)), rng.choice((0, 0, 3)))
                lists.append(sorted((t, b, u) for t, (b, u) in ent.items()))
            self.memo[i] = (lists, modes)
        return self.memo[i]


def _setting(fn, *args):
    """a setting call: the binding checks the values itself and raises ValueError where the library answers Q3_ERR_ARG"""
    try:
        return fn(*args)
    except ValueError as err:
        raise IndexError(str(err)) from None


def _fields(arrays, names):
    return [tuple(np.ascontiguousarray(a[f]) for f in names) for a in arrays]


def call(e, op, ref, prefix=(), env=None):
    """One op on an engine (a Transformer or a FakeEngine): what it returned, in a form that compares with ==/bitwise.  env: what the
    model knows in front of the op and the op does not say -- dict(top_k, pen: the settings in force, which the stop tokens of a loop
    op are derived under; table: the (lists, modes) of a set_logit_bias op; cap: the n_new of the last loop call with records)"""
    k = op["op"]
    env = env or {}
    if k == "refused_bias_lists":                   # a loop op with one request more than the table has lists
        return call(e, dict(op, op=op["kind"]), ref, prefix, env)
    if k in ("set_top_k", "refused_set_top_k"):
        return _setting(e.set_top_k, op["k"])
    if k in ("set_gen_logprobs", "refused_set_gen_logprobs"):
        return _setting(e.set_gen_logprobs, op["n"])
    if k == "set_penalties":
        return _setting(e.set_penalties, op["p"], op["f"])
    if k == "refused_set_penalties":
        return _setting(e.set_penalties, *{"2.5": (2.5, 0.0), "nan": (0.5, float("nan"))}[op["bad"]])
    if k == "set_logit_bias":
        return _setting(e.set_logit_bias, *env["table"])
    if k == "refused_set_logit_bias":
        t = 7 + op["at"]
        lists, modes = {"twice": ([[(t, 1.0), (t + 1, 0.5), (t, -1.0)]], None), "vocab": ([[(t, 1.0)], [(VOCAB, 1.0)]], None),
                        "inf": ([[(t, float("inf"))]], None), "allow": ([[(t, NEG_INF), (t + 1, NEG_INF, 4)]], [1])}[op["bad"]]
        return _setting(e.set_logit_bias, lists, modes)
    if k in ("set_guide", "set_guide_sparse"):
        g = env["auto"]
        if g is None:
            return _setting(e.set_guide, None, 0) if k == "set_guide" else _setting(e.set_guide_sparse, None, None, None, None, 0)
        if k == "set_guide":
            return _setting(e.set_guide, g.next, g.starts)
        return _setting(e.set_guide_sparse, g.default, g.offsets, g.tokens, g.targets, g.starts)
    if k == "set_stop_seq":
        return _setting(e.set_stop_sequences, *(env["auto"] or (None, None)))
    if k == "refused_set_guide":
        nxt = np.zeros((3, VOCAB + (op["bad"] == "vocab")), dtype=np.int16)
        if op["bad"] == "dead":                  # a state that allows no token
            nxt[1] = -1
        elif op["bad"] == "entry":               # an entry outside [-1, n_states)
            nxt[2, op["at"]] = 3
        return _setting(e.set_guide, nxt, [0, 3] if op["bad"] == "start" else [0])
    if k in ("refused_set_guide_sparse", "refused_set_stop_seq"):
        import types
        t = 5 + op["at"]
        dflt, off, tok, tgt, start, vocab = [0, 0], [0, 2, 3], [t, t + 1, t], [1, -1, 1], [0], VOCAB
        if op["bad"] == "dead":                  # (a guide only: a stop automaton may hold such a state)
            dflt, tgt = [0, -1], [1, -1, -1]
        elif op["bad"] == "ascend":
            tok = [t + 1, t, t]
        elif op["bad"] == "row_off":             # row_off[n_states] != n_edges
            off = [0, 2, 2]
        elif op["bad"] == "start":
            start = [0, 2]
        elif op["bad"] == "dflt":
            dflt = [0, 2]
        elif k == "refused_set_guide_sparse":    # "vocab": the binding states the engine's vocabulary itself; a token outside it
            tok = [t, VOCAB, t]
        else:
            vocab = VOCAB + 1
        if k == "refused_set_guide_sparse":
            return _setting(e.set_guide_sparse, dflt, off, tok, tgt, start)
        return _setting(e.set_stop_sequences, types.SimpleNamespace(default=dflt, offsets=off, tokens=tok, targets=tgt, start=0, vocab_size=vocab), start)
    if k == "refused_guide_starts":              # a loop op with one request more than the automaton has start states
        return call(e, dict(op, op=op["kind"]), ref, prefix, env)
    if k == "read_gen_logprobs":
        got = e.read_gen_logprobs(env.get("cap"))
        return [tuple(np.ascontiguousarray(a).tobytes() for a in g) for g in got]
    if k in ("score_top_many", "score_top_many_prefix", "refused_score_top"):
        prompts = [toks(CAT[i][:2]) for i in op["reqs"]]
        recs, tops, ranks, st = e.score_top_many(prompts, op["k"], op["score_from"], use_prefix=k == "score_top_many_prefix")
        return _fields(recs, ("target", "max", "sum", "argmax")), _fields(tops, ("logit", "index")), [np.asarray(r) for r in ranks], st
    if k in ("forward_batch", "forward_batch_s", "refused_batch"):
        lg, am = e.forward_batch(op["tokens"], op["pos"])
        return lg, am
    if k in ("generate_greedy_batch", "generate_greedy_batch_s"):
        return np.array(e.generate_greedy_batch(op["first"], op["pos"], op["steps"]))
    if k in ("prefill_batched", "refused_prefill_batched"):
        return e.prefill(toks(op["prompt"]), op["pos"], batched=True)
    if k in ("verify", "verify_draw", "refused_verify"):
        fn = e.verify_draw if k == "verify_draw" or op.get("draw") else e.verify
        nxt, a, lg = fn(op["tokens"], op["pos"], want_logits=True)
        return [int(t) for t in nxt], a, lg
    if k in ("generate_lookup", "generate_lookup_draw"):
        fn = e.generate_lookup if k == "generate_lookup" else e.generate_lookup_draw
        out, st = fn(toks(op["corpus"]), op["first"], op["pos"], op["n"], op["ngram"], op["draft_len"])
        if st is not None:
            assert st.single_steps + st.verify_passes + st.accepted == op["n"] and st.accepted <= st.drafted, st
        return [int(t) for t in out]
    if k == "generate_greedy":
        return [int(t) for t in e.generate_greedy(op["first"], op["pos"], op["n"])]
    if k in ("forward", "refused_forward"):
        return np.array(e.forward(op["token"], op["pos"]), copy=True)
    if k in ("batch_step_cols", "refused_greedy_only") or (k == "refused_cols" and not op["draw"]):
        return e.batch_step_cols(op["slots"], op["tokens"], op["pos"], want_logits=True)
    if k in ("batch_step_cols_draw", "refused_cols"):
        return e.batch_step_cols_draw(op["slots"], op["tokens"], op["pos"], keep=op.get("keep"), want_logits=True)
    if k in MANY or k == "refused_stop":
        prompts, n_new, sampler, stop = _requests(op, ref, prefix if k == "generate_many_prefix" else (), env.get("top_k", 0), env.get("pen", (0.0, 0.0)))
        if k == "generate_many_greedy":
            return e.generate_many_greedy(prompts, n_new)
        if k == "generate_many_sampled":
            return e.generate_many_sampled(prompts, n_new, *sampler)
        if k == "generate_many_dense":
            return e.generate_many_dense(prompts, n_new, sampler, op["dense_min"])
        if k == "refused_stop":
            prompts[op["bad"]][-1] = VOCAB
        # the two loops with a device scheduler: the rows, the stats, and the whole output buffer with n_out -- -1 stands behind
        # every request's last token
        fn = e.generate_many_prefix if k == "generate_many_prefix" else e.generate_many_stop
        buf, got, st = fn(prompts, n_new, stop, sampler, raw=True)
        buf = [int(t) for t in buf]
        offs = [sum(n_new[:r]) for r in range(len(n_new))]
        return [buf[o:o + g] for o, g in zip(offs, got)], st, buf, [int(g) for g in got]
    if k in ("batch_prefill_slots", "refused_dense"):
        return e.batch_prefill_slots(op["slots"], [toks(p) for p in op["prompts"]], op["first"])
    if k in ("batch_copy_rows", "refused_prefix"):
        return e.batch_copy_rows(op["src"], op["dst"], op["first"], op["n"])
    if k == "batch_prefix_set":
        return e.batch_prefix_set(toks(op["prompt"]))
    if k in ("embed_many", "embed_many_prefix", "refused_embed"):
        prompts = [toks(CAT[i][:2]) for i in op["reqs"]]
        if k == "refused_embed":
            prompts[op["bad"]][0] = VOCAB
        return e.embed_many(prompts, normalize=op["normalize"], out_dim=op["out_dim"], use_prefix=k == "embed_many_prefix")
    if k in CHOICE or k == "refused_choice":
        prompts = [toks(CAT[i][:2]) for i in op["reqs"]]
        cand = candidates(op)
        if k == "refused_choice":
            if op["bad"] == "token":
                prompts[op["at"]][-1] = VOCAB
            elif op["bad"] == "k0":
                cand = []
            else:
                (cand[op["at"]] if op["cand"][1] else cand)[-1] = VOCAB
        return e.choice_many(prompts, cand, use_prefix=k == "choice_many_prefix")
    if k in SCORE or k == "refused_score":
        prompts = [toks(CAT[i][:2]) for i in op["reqs"]]
        sf = op["score_from"]
        if k == "refused_score":
            at = op["at"]
            if op["bad"] == "token":
                prompts[at][-1] = -1
            elif op["bad"] == "empty":
                prompts[at] = []
                sf = sf and sf[:at] + [1] + sf[at + 1:]
            else:
                sf = list(sf or [1] * len(prompts))
                sf[at] = 0 if op["bad"] == "from0" else len(prompts[at]) + 1
        recs, st = e.score_many(prompts, sf, use_prefix=k == "score_many_prefix")
        # field by field, so that same() compares the three floats of every record by their bits
        return [tuple(np.ascontiguousarray(r[f]) for f in ("target", "max", "sum", "argmax")) for r in recs], st
    if k in ("set_batch_sampler_on", "set_batch_sampler_off"):
        return e.set_batch_sampler(op["T"], op["P"], op["seeds"])
    if k == "set_sampler":
        return e.set_sampler(op["T"], op["P"], op["seed"])
    if k == "batch_reset_kv":
        return e.batch_reset_kv()
    if k == "reset_kv":
        return e.reset_kv()
    if k == "batch_init":
        return e.batch_init(op["streams"], op["ctx"])
    raise ValueError(k)


def outcome(e, op, ref, prefix, env=None):
    """call(), with a refusal turned into ("refused", code): IndexError is how the binding reports Q3_ERR_ARG"""
    try:
        return call(e, op, ref, prefix, env)
    except IndexError:
        return ("refused", -3)
    except RuntimeError as err:
        if getattr(err, "code", None) is None:
            raise
        return ("refused", err.code)


def _bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    """equal: arrays bit for bit, everything else by =="""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(_bits(a), _bits(b)))
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def _read(e, cid, L, ctx, kvd):
    if cid == "single":
        return e.read_state("key").reshape(L, SEQ, kvd), e.read_state("value").reshape(L, SEQ, kvd)
    return e.batch_read_state(cid, "key").reshape(L, ctx, kvd), e.batch_read_state(cid, "value").reshape(L, ctx, kvd)


class _Lane:
    """one engine under test, the clean model beside it and the last verified copy of every cache"""

    def __init__(self, engine, ref, tables=None):
        self.e, self.ref, self.m, self.tables = engine, ref, FakeEngine(ref), tables
        self.last_read = None                # the bytes read behind the last loop op with records
        self.snap = {"single": tuple(np.array(a, copy=True) for a in _read(engine, "single", ref.L, SEQ, ref.kvd))}

    def step(self, op, i=None):
        m, ref = self.m, self.ref
        refusal = op["op"].startswith("refused")
        m.touched = {}
        prefix = list(m.prefix)
        env = dict(top_k=m.k_top, pen=m.pen, cap=m.gen and m.gen["cap"], table=self.tables.get(i) if op["op"] == "set_logit_bias" and op["form"] != "off" else ([], None))
        if op["op"] in GUIDE_SETTERS:                # the automaton of the op, from the reference alone (None: off)
            env["auto"] = None if op["form"] == "off" else self.tables.stop(i) if op["op"] == "set_stop_seq" else self.tables.guide(i)
        want = outcome(m, op, ref, prefix, env)
        got = outcome(self.e, op, ref, prefix, env)
        if refusal:
            assert isinstance(want, tuple) and want[0] == "refused", f"the model accepts this call: {want!r}"
            assert not m.touched
        if op["op"] == "read_gen_logprobs" and not (isinstance(want, tuple) and want[0] == "refused"):
            # the records of the last loop call, whatever ran in between: the bytes the read behind that call returned
            assert not (isinstance(got, tuple) and got and got[0] == "refused"), f"the read is refused ({got!r}), the reference holds records"
            assert got == self.last_read, "read_gen_logprobs returns other bytes than the read behind the loop call"
        else:
            assert same(got, want), f"the call returned {_short(got)}, the reference gives {_short(want)}"
        self.settings(op, want)
        if op["op"] == "batch_init":
            self.snap = {"single": self.snap["single"]}
        for cid in ["single"] + list(range(m.streams)):
            c = m._cache(cid)
            cur = _read(self.e, cid, ref.L, c.ctx, ref.kvd)
            t = m.touched.get(cid)
            for what, now, model in (("key", cur[0], c.K), ("value", cur[1], c.V)):
                if t == "all":
                    assert same(now, model), f"{what} rows of cache {cid}: not what a cleared cache holds"
                    continue
                old = self.snap[cid][what == "value"]
                if t is None:                        # not named by the op: one pass over the whole cache
                    assert np.array_equal(now.reshape(-1).view(np.uint64), old.reshape(-1).view(np.uint64)), \
                        f"{what} rows of cache {cid}, which the op does not name, changed" + _where(now, old, 0, 0)
                    continue
                lo, hi = t
                assert same(now[:, :lo], old[:, :lo]) and same(now[:, hi:], old[:, hi:]), \
                    f"{what} rows of cache {cid} outside {lo} .. {hi - 1} changed" + _where(now, old, lo, hi)
                n = len(c.hist)
                assert same(now[:, :n], model[:, :n]), f"{what} rows 0 .. {n - 1} of cache {cid} differ from the oracle's" + _where(now[:, :n], model[:, :n], 0, 0)
            if t or cid not in self.snap:
                self.snap[cid] = tuple(np.array(a, copy=True) for a in cur)
        assert self.e.batch_prefix_get() == m.prefix, f"resident prefix of {len(self.e.batch_prefix_get())} tokens, the reference holds {len(m.prefix)}"
        if m.srng is not None:
            assert self.e.sampler_rng_state() == m.srng, "single-stream rng state"


    def settings(self, op, want):
        """after every op: the four getters give the model's settings; behind a successful loop op under gen_logprobs >= 0 the records
        are read -- every request's whole stretch of the buffers -- and held to the reference by section 2o's standard
        (genlp_ref.assert_same): target and sum by bits, argmax equal, max by value, tops by bits and index, ranks equal; the entries at
        and behind a request's n_out are all-zero bytes"""
        import genlp_ref
        e, m = self.e, self.m
        got = (e.top_k, e.get_gen_logprobs(), tuple(e.get_penalties()), e.get_logit_bias())
        assert got == (m.k_top, m.genlp, m.pen, m.get_logit_bias()), f"the settings read back as {_short(got)}, the reference holds {_short((m.k_top, m.genlp, m.pen, m.get_logit_bias()))}"
        # the getters of sections 2r to 2t.  The library reports the counts it holds (states, edges, start states; 0 for the form
        # that is not set) and the binding answers with the copy its setter kept where they agree with it: what is compared here is
        # those counts and that copy, not the device tables.  Where the counts disagree the binding raises, which fails here too
        for name in ("get_guide", "get_guide_sparse", "get_stop_sequences"):
            hold = getattr(m, name)()
            try:
                have = getattr(e, name)()
            except RuntimeError as err:
                raise AssertionError(f"{name} raises ({err}): the library holds other counts than the setter left; the reference holds {_short(hold)}") from None
            assert same(have, hold), f"{name} reads back {_short(have)}, the reference holds {_short(hold)}"
        if op["op"] in MANY:
            self.last_read = None
            if m.gen is not None:
                cap, n_out, k = m.gen["cap"], m.gen["got"], m.gen["k"]
                full = e.read_gen_logprobs(cap)
                rows = want[0]
                genlp_ref.assert_same([tuple(a[:n] for a in f) for f, n in zip(full, n_out)], m.read_gen_logprobs(), rows, k, f"records under gen_logprobs {k}")
                genlp_ref.assert_zero_behind(full, n_out, "records")
                self.last_read = [tuple(np.ascontiguousarray(a).tobytes() for a in f) for f in full]


def _where(a, b, lo, hi):
    bad = np.argwhere(_bits(np.ascontiguousarray(a)) != _bits(np.ascontiguousarray(b)))
    bad = [x for x in bad if not lo <= x[1] < hi]
    return f" (first at layer {bad[0][0]}, row {bad[0][1]}; {len({int(x[1]) for x in bad})} rows)" if bad else ""


def _short(v):
    s = repr(v)
    return s if len(s) < 400 else s[:400] + " ..."


def run(engines, ops, ref, seed=None):
    """The ops on one engine, or on several engines interleaved op by op.  After every op: its outputs equal the reference's (logits
    and embeddings bit for bit); every cache the op does not name, and every row of a named cache outside what the op writes, is
    bit-unchanged against the copy taken before it; the rows a cache is known to hold equal the oracle's; the resident prefix and the
    single-stream rng state are the reference's."""
    tables = Tables(ops, ref)
    lanes = [_Lane(e, ref, tables) for e in (engines if isinstance(engines, (list, tuple)) else [engines])]
    for i, op in enumerate(ops):
        for j, lane in enumerate(lanes):
            try:
                lane.step(op, i)
            except AssertionError as err:
                raise AssertionError(f"seed {seed}, engine {j}, op {i} ({op['op']}): {err}\nops = {ops[:i + 1]!r}") from None
    return lanes
