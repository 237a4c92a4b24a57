#!/usr/bin/env python3
"""What ragged column passes (include/qwen3_hip.h section 2e) cost and gain on the full-size synthetic checkpoints.

    python tools/bench_serve.py [--models qwen3-0.6b,qwen3-8b] [--ctx 1024] [--out profiles] [--limit 420]

Every model is measured in a child process of its own under a time limit (one faulting run never starts the next).  Per model:
  (a) pass cost: wall time of a 32-column pass of 32 single-position slots (q3_batch_step_cols, no logits) against a
      q3_forward_batch step (no logits) at the same positions, both with one host round trip per step;
  (b) requests through q3_generate_many_greedy against the only way section 2b offers -- every prompt token stepped through
      q3_forward_batch, one token per stream and weight pass, a slot refilled when its request ends, one host round trip per
      step: 8 requests of 256 prompt tokens + 64 new through 8 slots, and 64 requests of mixed lengths through 32 slots.  Passes
      and tok/s (prompt + generated tokens per second, and generated tokens per second) for both; the tokens must be equal.
Writes <out>/serve_cols.json and serve_cols.md (a batch-32 A/B section and a sampler section already in the .md are kept).

    python tools/bench_serve.py --temperature 0.6 --topp 0.95 [--models qwen3-0.6b]

The same workloads under the sampler (section 2f).  Per model: (c) the wall time of a q3_batch_step_cols_draw pass of 1, 8 and 32
single-position columns with one column and with all columns drawing, against the greedy q3_batch_step_cols pass of the same
width (temperature 0 set on the same engine); (d) the two request workloads through q3_generate_many_sampled against
q3_generate_many_greedy.  Appends a section to <out>/serve_cols.md (an earlier section of the same name is replaced, the rest of
the file is kept) and writes <out>/serve_cols_sampled.json.

    python tools/bench_serve.py --dense-min 64 [--models qwen3-0.6b,qwen3-8b]

Long prompts through dense blocks (section 2g).  Per model, context 2,304 per slot: (e) 8 requests of 256 + 64 tokens on 8 slots
and 32 requests of 2,048 + 64 on 32 slots through q3_generate_many_dense with that dense_min against q3_generate_many_greedy on the
same engine (best of 2 calls each, the rows must be equal); prompt tok/s is measured by the same mixes with one new token per
request; (f) one block: q3_batch_prefill_slots of 8 runs of 256 tokens against q3_prefill_batched of one 2,048-token prompt.
Appends a section to <out>/serve_cols.md and writes <out>/serve_cols_dense.json.

    python tools/bench_serve.py --stop [--models qwen3-0.6b,qwen3-8b]

Stop tokens in the device loop (section 2h).  Per model: 64 requests through 32 slots with a cap of 256 new tokens -- 8 prompts of
mixed lengths, each sent 8 times, interleaved.  The synthetic checkpoints emit no EOS, so the existing loop runs once at the cap
and a stop set of at most 8 tokens is picked from its rows (the token that shortens the rows most, again and again) until
sum(n_emit) <= sum(n_new) / 2.  (The greedy rows of 64 different prompts over a 151,936-token vocabulary share too few tokens for
8 of them to halve the output; requests that repeat a prompt produce the same row and end at the same token.)  Then, best of 3
calls each behind a warm-up call: (g) q3_generate_many_greedy at the cap plus the host cut; (h) q3_generate_many_stop; (i)
q3_generate_many_greedy with n_new = n_emit -- the same passes with one synchronisation, the floor for (h).  (h) and (i) must run
the same number of passes and all three must give equal rows up to the cut.  Appends a section to <out>/serve_cols.md and writes
<out>/serve_cols_stop.json.

    python tools/bench_serve.py --prefix 512 [--models qwen3-0.6b,qwen3-8b]

A shared prompt prefix (section 2i).  Per model: 64 requests through 32 slots that all begin with the same N-token prefix, suffixes of
1 to 64 tokens, 32 new tokens each.  Best of 3 calls each behind a warm-up call: (j) q3_generate_many_greedy on the full prompts;
(k) q3_generate_many_dense(dense_min 64) on the full prompts, the stronger baseline; (l) q3_generate_many_prefix on the suffixes
with the prefix resident; the rows must be equal.  Also: q3_batch_prefix_set on its own; the copy of the N prefix rows from slot 0 to
the 31 other slots through q3_batch_copy_rows (one launch of k_kv_rows_bcast, the loop's broadcast but for one destination) with
its achieved bytes per second (read once + written 31 times), next to a loop of 2 * layers * 31 hipMemcpyAsync calls that move the
same bytes between buffers of the same layout.  Appends a section to <out>/serve_cols.md and writes <out>/serve_cols_prefix.json.

    python tools/bench_serve.py --stop-seq [--ab PARENT_TREE] [--models qwen3-0.6b,qwen3-8b]

Stop sequences in the device loop (section 2t), on the requests and the stop set of --stop.  Three comparisons, the calls taken by
turns, best of 3 rounds behind a warm-up round: (a) q3_generate_many_stop with no automaton -- the path of the commit before; with
--ab PARENT_TREE (a checkout of that commit with its library built) the same call also runs in child processes of that tree, ours
and theirs by turns, twice each, which gives the run-to-run spread; (b) the same call under an automaton of four strings lifted
over the full vocabulary that never matches: (b) - (a) over the passes is what k_cols_sched_seq costs over k_cols_sched; (c) an
automaton of token sequences that ends the requests where the stop set ends them, with n_stop == 0, against the loop at the cap plus
the host cut.  Also: the automaton's states, edges and bytes, and the host time of stop_automaton_from_strings.  Writes
<out>/stop_seq.json and <out>/stop_seq.md.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (--tree, the worker of --stop-seq --ab: the package and the library of another checkout run the call)
_TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv[:-1] else ROOT
sys.path.insert(0, os.path.join(os.path.abspath(_TREE), "qwen3-rs_amd"))

AB_MARK = "## Batch-32 decode A/B"
DENSE_MARK = "## Dense blocks over the slots"
SAMPLED_MARK = "## Under the sampler"
STOP_MARK = "## Stop tokens in the device loop"
PREFIX_MARK = "## Shared prompt prefix"


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def stepped(t, prompts, n_new, max_streams):
    """section 2b only: one token per slot and pass; returns (rows, passes)"""
    queue = list(range(len(prompts)))
    slots = [None] * max_streams
    rows = [[] for _ in prompts]
    passes = 0
    while queue or any(s is not None for s in slots):
        for i in range(max_streams):
            if slots[i] is None and queue:
                slots[i] = [queue.pop(0), 0]                           # request, position
        n = max(i for i in range(max_streams) if slots[i] is not None) + 1
        toks, pos = [], []
        for i in range(n):
            if slots[i] is None:                                       # no compaction: a hole below a live slot is stepped too
                toks.append(0)
                pos.append(0)
                continue
            r, p = slots[i]
            toks.append(prompts[r][p] if p < len(prompts[r]) else rows[r][p - len(prompts[r])])
            pos.append(p)
        _, am = t.forward_batch(toks, pos, want_logits=False)
        passes += 1
        for i in range(n):
            if slots[i] is None:
                continue
            r, p = slots[i]
            if p >= len(prompts[r]) - 1:
                rows[r].append(am[i])
            slots[i][1] = p + 1
            if len(rows[r]) == n_new[r]:
                slots[i] = None
    return rows, passes


def worker(name, ctx, ckpt_dir, seed):
    import numpy as np
    import qwen3_rs_amd as q3
    ck = q3.checkpoint
    shape = ck.SHAPES[name]
    path = os.path.join(ckpt_dir, f"{name}-seed{seed}.q3bin")
    ck.ensure_synthetic_checkpoint(path, shape, seed=seed)
    res = {"model": name, "ctx": ctx}
    rng = np.random.default_rng(7)
    with q3.TransformerBuilder(path).with_ctx_length(ctx).build() as t:
        # ---- (a) one pass
        t.batch_init(32, ctx)
        toks = [int(v) for v in rng.integers(0, shape.vocab_size, 32)]
        for p0 in (8, 256):
            pos = [p0] * 32
            t.forward_batch(toks, pos, want_logits=False)
            t.batch_step_cols(list(range(32)), toks, pos)
            fb, sc = [], []
            for _ in range(15):                                        # alternating
                t0 = time.perf_counter()
                t.forward_batch(toks, pos, want_logits=False)
                fb.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                t.batch_step_cols(list(range(32)), toks, pos)
                sc.append(time.perf_counter() - t0)
            res[f"pass_ms_pos{p0}"] = {"forward_batch": 1e3 * median(fb), "step_cols": 1e3 * median(sc)}
        # ---- (b) requests
        cases = {
            "8x(256+64), 8 slots": ([256] * 8, [64] * 8, 8),
            "64 mixed, 32 slots": ([int(v) for v in rng.integers(1, 200, 64)], [int(v) for v in rng.integers(1, 96, 64)], 32),
        }
        res["requests"] = {}
        for label, (plen, nnew, ms) in cases.items():
            prompts = [ck.iter_prompt_tokens(shape, seed + 50 + r, n) for r, n in enumerate(plen)]
            t.batch_init(ms, ctx)
            n_tok, n_gen = sum(plen) + sum(nnew) - len(plen), sum(nnew)
            t.generate_many_greedy(prompts[:2], [2, 2])                # plans
            t0 = time.perf_counter()
            rows, st = t.generate_many_greedy(prompts, nnew)
            dt_many = time.perf_counter() - t0
            t0 = time.perf_counter()
            rows2, st2 = t.generate_many_greedy(prompts, nnew)         # every plan width of this schedule now exists
            dt_many = min(dt_many, time.perf_counter() - t0)
            stepped(t, prompts[:2], [2, 2], ms)
            t0 = time.perf_counter()
            ref, ref_passes = stepped(t, prompts, nnew, ms)
            dt_step = time.perf_counter() - t0
            res["requests"][label] = {
                "tokens_equal": rows == ref and rows2 == ref, "model_tokens": n_tok, "generated": n_gen,
                "many": {"passes": st.passes, "live_columns": st.live_columns, "seconds": dt_many, "tok_s": n_tok / dt_many,
                         "gen_tok_s": n_gen / dt_many},
                "stepped": {"passes": ref_passes, "seconds": dt_step, "tok_s": n_tok / dt_step, "gen_tok_s": n_gen / dt_step},
            }
    print("RESULT " + json.dumps(res))


def worker_sampled(name, ctx, ckpt_dir, seed, temperature, topp):
    import numpy as np
    import qwen3_rs_amd as q3
    ck = q3.checkpoint
    shape = ck.SHAPES[name]
    path = os.path.join(ckpt_dir, f"{name}-seed{seed}.q3bin")
    ck.ensure_synthetic_checkpoint(path, shape, seed=seed)
    res = {"model": name, "ctx": ctx, "temperature": temperature, "topp": topp, "pass_ms": {}, "requests": {}}
    rng = np.random.default_rng(7)
    seeds = list(range(1, 33))

    def timed(call):
        call()
        xs = []
        for _ in range(15):
            t0 = time.perf_counter()
            call()
            xs.append(time.perf_counter() - t0)
        return 1e3 * median(xs)
    with q3.TransformerBuilder(path).with_ctx_length(ctx).build() as t:
        t.batch_init(32, ctx)
        toks = [int(v) for v in rng.integers(0, shape.vocab_size, 32)]
        for w in (1, 8, 32):
            slots, tk, pos = list(range(w)), toks[:w], [8] * w
            t.set_batch_sampler(0.0, topp, seeds)
            greedy = timed(lambda: t.batch_step_cols(slots, tk, pos))
            t.set_batch_sampler(temperature, topp, seeds)
            one = timed(lambda: t.batch_step_cols_draw(slots, tk, pos, keep=[1] + [0] * (w - 1)))
            every = timed(lambda: t.batch_step_cols_draw(slots, tk, pos))
            res["pass_ms"][str(w)] = {"greedy": greedy, "one_draw": one, "all_draw": every}
        t.set_batch_sampler(0.0, topp, seeds)
        cases = {
            "8x(256+64), 8 slots": ([256] * 8, [64] * 8, 8),
            "64 mixed, 32 slots": ([int(v) for v in rng.integers(1, 200, 64)], [int(v) for v in rng.integers(1, 96, 64)], 32),
        }
        for label, (plen, nnew, ms) in cases.items():
            prompts = [ck.iter_prompt_tokens(shape, seed + 50 + r, n) for r, n in enumerate(plen)]
            rs = list(range(1, len(plen) + 1))
            t.batch_init(ms, ctx)
            n_tok, n_gen = sum(plen) + sum(nnew) - len(plen), sum(nnew)
            out = {}
            for k, call in (("greedy", lambda: t.generate_many_greedy(prompts, nnew)),
                            ("sampled", lambda: t.generate_many_sampled(prompts, nnew, temperature, topp, rs))):
                call()                                                 # plans
                dts = []
                for _ in range(2):
                    t0 = time.perf_counter()
                    _, st = call()
                    dts.append(time.perf_counter() - t0)
                out[k] = {"passes": st.passes, "seconds": min(dts), "tok_s": n_tok / min(dts), "gen_tok_s": n_gen / min(dts)}
            res["requests"][label] = out
    print("RESULT " + json.dumps(res))


def worker_dense(name, ctx, ckpt_dir, seed, dense_min):
    import qwen3_rs_amd as q3
    ck = q3.checkpoint
    shape = ck.SHAPES[name]
    path = os.path.join(ckpt_dir, f"{name}-seed{seed}.q3bin")
    ck.ensure_synthetic_checkpoint(path, shape, seed=seed)
    res = {"model": name, "ctx": ctx, "dense_min": dense_min, "requests": {}}

    def best(call, n=2):
        call()                                                         # plans, scratch
        dts = []
        for _ in range(n):
            t0 = time.perf_counter()
            out = call()
            dts.append(time.perf_counter() - t0)
        return min(dts), out
    with q3.TransformerBuilder(path).with_ctx_length(ctx).build() as t:
        for label, n_req, plen, nnew in (("8x(256+64), 8 slots", 8, 256, 64), ("32x(2048+64), 32 slots", 32, 2048, 64)):
            prompts = [ck.iter_prompt_tokens(shape, seed + 50 + r, plen) for r in range(n_req)]
            t.batch_init(n_req, ctx)
            out = {}
            for k, call in (("columns", lambda nn: t.generate_many_greedy(prompts, nn)),
                            ("dense", lambda nn: t.generate_many_dense(prompts, nn, None, dense_min))):
                dt, got = best(lambda: call([nnew] * n_req))
                dt1, _ = best(lambda: call([1] * n_req))                # the prompts alone: one token behind each
                out[k] = {"passes": got[1].passes, "seconds": dt, "req_s": n_req / dt, "tok_s": n_req * (plen + nnew - 1) / dt,
                          "prompt_seconds": dt1, "prompt_tok_s": n_req * plen / dt1, "rows": got[0]}
                if k == "dense":
                    out[k]["blocks"] = got[2].blocks
            out["tokens_equal"] = out["columns"].pop("rows") == out["dense"].pop("rows")
            res["requests"][label] = out
        # ---- one block of 8 x 256 columns against one 2,048-token prompt through the single-cache path
        t.batch_init(8, ctx)
        prompts = [ck.iter_prompt_tokens(shape, seed + 50 + r, 256) for r in range(8)]
        dt_slots, _ = best(lambda: t.batch_prefill_slots(list(range(8)), prompts, [0] * 8), 5)
        res["block_ms"] = {"prefill_slots_8x256": 1e3 * dt_slots}
    with q3.TransformerBuilder(path).with_ctx_length(ctx).build() as t:
        one = ck.iter_prompt_tokens(shape, seed + 50, 2048)
        dt_one, _ = best(lambda: t.prefill(one, 0, batched=True), 5)
        res["block_ms"]["prefill_batched_1x2048"] = 1e3 * dt_one
    print("RESULT " + json.dumps(res))


def n_emit_of(rows, stop):
    return [next((i + 1 for i, t in enumerate(r) if t in stop), len(r)) for r in rows]


def pick_stop_set(rows, limit=8):
    """at most `limit` tokens, each the one that shortens the rows most given the ones before it, until the rows are half as long"""
    total, stop = sum(len(r) for r in rows), []
    while len(stop) < limit and sum(n_emit_of(rows, set(stop))) > total // 2:
        emit = n_emit_of(rows, set(stop))
        cand = sorted({t for r, e in zip(rows, emit) for t in r[:e]} - set(stop))
        stop.append(min(cand, key=lambda t: (sum(n_emit_of(rows, set(stop) | {t})), t)))
    return stop


def worker_stop(name, ctx, ckpt_dir, seed):
    import numpy as np
    import qwen3_rs_amd as q3
    ck = q3.checkpoint
    shape = ck.SHAPES[name]
    path = os.path.join(ckpt_dir, f"{name}-seed{seed}.q3bin")
    ck.ensure_synthetic_checkpoint(path, shape, seed=seed)
    rng = np.random.default_rng(7)
    n_req, ms, cap = 64, 32, 256
    plen = [int(v) for v in rng.integers(1, 200, 8)]
    distinct = [ck.iter_prompt_tokens(shape, seed + 50 + r, n) for r, n in enumerate(plen)]
    prompts = [distinct[r % 8] for r in range(n_req)]
    nnew = [cap] * n_req

    def best(call, n=3):
        call()                                                         # plans of every width the schedule uses
        dts = []
        for _ in range(n):
            t0 = time.perf_counter()
            out = call()
            dts.append(time.perf_counter() - t0)
        return min(dts), out
    with q3.TransformerBuilder(path).with_ctx_length(ctx).build() as t:
        t.batch_init(ms, ctx)
        rows, _ = t.generate_many_greedy(prompts, nnew)
        stop = pick_stop_set(rows)
        emit = n_emit_of(rows, set(stop))
        print(f"[bench_serve] {name}: stop set {stop}: {sum(emit)} of {sum(nnew)} tokens", file=sys.stderr)
        want = [r[:e] for r, e in zip(rows, emit)]

        def at_cap():
            got, st = t.generate_many_greedy(prompts, nnew)
            return [r[:e] for r, e in zip(got, n_emit_of(got, set(stop)))], st         # the host cut is part of what is timed
        dt_a, (rows_a, st_a) = best(at_cap)
        dt_b, (rows_b, st_b) = best(lambda: t.generate_many_stop(prompts, nnew, stop))
        dt_c, (rows_c, st_c) = best(lambda: t.generate_many_greedy(prompts, emit))
    res = {"model": name, "ctx": ctx, "requests": n_req, "slots": ms, "cap": cap, "stop_set": stop, "sum_n_new": sum(nnew), "sum_n_emit": sum(emit),
           "half_reached": 2 * sum(emit) <= sum(nnew), "rows_equal": rows_a == want and rows_b == want and rows_c == want,
           "passes_equal": st_b.passes == st_c.passes,
           "at_cap": {"passes": st_a.passes, "seconds": dt_a}, "stop": {"passes": st_b.passes, "seconds": dt_b},
           "n_emit": {"passes": st_c.passes, "seconds": dt_c}, "per_pass_us": 1e6 * (dt_b - dt_c) / max(1, st_b.passes)}
    print("RESULT " + json.dumps(res))


def synthetic_token_bytes(vocab_size):
    """a stand-in vocabulary for the lift: token v spells its number and a comma"""
    return [b"%d," % v for v in range(vocab_size)]


NEVER = ["12,34,x", "7,7,7,x", "99,100,x", "5,x"]       # they share bytes with thousands of tokens and end in a byte no token has


def worker_stop_seq(name, ctx, ckpt_dir, seed, parent_only):
    import numpy as np
    import qwen3_rs_amd as q3
    ck = q3.checkpoint
    shape = ck.SHAPES[name]
    path = os.path.join(ckpt_dir, f"{name}-seed{seed}.q3bin")
    ck.ensure_synthetic_checkpoint(path, shape, seed=seed)
    rng = np.random.default_rng(7)
    n_req, ms, cap = 64, 32, 256
    plen = [int(v) for v in rng.integers(1, 200, 8)]
    distinct = [ck.iter_prompt_tokens(shape, seed + 50 + r, n) for r, n in enumerate(plen)]
    prompts = [distinct[r % 8] for r in range(n_req)]
    nnew = [cap] * n_req
    res = {"model": name, "ctx": ctx, "requests": n_req, "slots": ms, "cap": cap}
    with q3.TransformerBuilder(path).with_ctx_length(ctx).build() as t:
        t.batch_init(ms, ctx)
        rows, _ = t.generate_many_greedy(prompts, nnew)
        stop = pick_stop_set(rows)
        emit = n_emit_of(rows, set(stop))
        want = [r[:e] for r, e in zip(rows, emit)]
        calls = {"a": lambda: t.generate_many_stop(prompts, nnew, stop)}
        if not parent_only:
            from qwen3_rs_amd.stops import first_match
            t0 = time.perf_counter()
            never = q3.stop_automaton_from_strings(NEVER, synthetic_token_bytes(shape.vocab_size))
            res["lift_seconds"] = time.perf_counter() - t0
            res["never"] = {"strings": NEVER, "vocab": shape.vocab_size, "states": never.n_states, "edges": never.n_edges, "bytes": 4 * never.n_states + 4 * (never.n_states + 1) + 8 * never.n_edges}
            # the sequences that end the requests where the stop set ends them: the two tokens up to each row's stop token
            seqs = sorted({tuple(r[e - 2:e]) for r, e in zip(rows, emit) if 2 <= e < len(r)})
            ends = q3.stop_automaton(seqs, shape.vocab_size)
            semit = [len(r) if (m := first_match(ends, ends.start, r)) is None else m + 1 for r in rows]
            swant = [r[:e] for r, e in zip(rows, semit)]
            res["ends"] = {"sequences": len(seqs), "states": ends.n_states, "edges": ends.n_edges, "sum_n_emit": sum(semit)}

            def under(automaton, stop_tokens):
                t.set_stop_sequences(automaton)
                try:
                    return t.generate_many_stop(prompts, nnew, stop_tokens)
                finally:
                    t.set_stop_sequences(None)

            def host_cut():
                got, st = t.generate_many_greedy(prompts, nnew)
                return [r if (m := first_match(ends, ends.start, r)) is None else r[:m + 1] for r in got], st   # the cut is part of what is timed
            calls.update({"b": lambda: under(never, stop), "c_device": lambda: under(ends, []), "c_host": host_cut})
        best, out = {}, {}
        for rnd in range(4):                                               # round 0 warms up: plans of every width the schedules use
            for k, call in calls.items():
                t0 = time.perf_counter()
                out[k] = call()
                dt = time.perf_counter() - t0
                if rnd:
                    best[k] = min(best.get(k, dt), dt)
    res.update({"stop_set": stop, "sum_n_new": sum(nnew), "sum_n_emit": sum(emit),
                "runs": {k: {"seconds": best[k], "passes": out[k][1].passes} for k in calls},
                "rows_equal": all(out[k][0] == (swant if k.startswith("c_") else want) for k in calls)})
    if not parent_only:
        res["per_pass_us"] = 1e6 * (best["b"] - best["a"]) / max(1, out["a"][1].passes)
        res["passes_equal"] = out["a"][1].passes == out["b"][1].passes
    print("RESULT " + json.dumps(res))


def main_stop_seq(a):
    results, failed = [], False
    for name in a.models.split(","):
        def child(tree, parent_only):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", name, "--ctx", str(a.ctx), "--ckpt-dir", a.ckpt_dir, "--seed", str(a.seed), "--stop-seq"]
            if parent_only:
                cmd += ["--tree", tree]
            p = subprocess.run(cmd, capture_output=True, text=True)
            sys.stderr.write(p.stderr[-2000:])
            if p.returncode != 0:
                print(f"[bench_serve] {name}: exit status {p.returncode}; stopping here", file=sys.stderr)
                return None
            return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        r = child(ROOT, False)
        if r is None:
            failed = True
            break
        if a.ab:                                                           # theirs, ours, theirs: a fault in one child starts no other
            r["ab"] = {"ours": [r["runs"]["a"]["seconds"]], "parent": []}
            for tree, key in ((a.ab, "parent"), (ROOT, "ours"), (a.ab, "parent")):
                x = child(tree, True)
                if x is None:
                    failed = True
                    break
                r["ab"][key].append(x["runs"]["a"]["seconds"])
                r["rows_equal"] = r["rows_equal"] and x["rows_equal"] and x["runs"]["a"]["passes"] == r["runs"]["a"]["passes"]
            if failed:
                break
        results.append(r)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "stop_seq.json"), "w") as f:
        json.dump(results, f, indent=1)
    lines = ["# Stop sequences in the device loop", "",
             "Written by `tools/bench_serve.py --stop-seq` (synthetic full-size checkpoints, one MI355X, context %d per slot): the requests and" % a.ctx,
             "the stop set of `--stop` -- 64 requests through 32 slots, a cap of 256 new tokens.  Wall time per call, the calls taken by turns,",
             "best of 3 rounds behind a warm-up round.", "",
             "(a) `q3_generate_many_stop` with no automaton: the path of the commit before.  (b) the same call under an automaton of four strings",
             "lifted over the full vocabulary that never matches; us per pass = ((b) - (a)) / passes: what `k_cols_sched_seq` costs over `k_cols_sched`.",
             "(c) an automaton of token sequences that ends the requests, n_stop == 0, on the device against the loop at the cap plus the host cut.",
             "Every timed call of (b) and (c) sets the automaton in front and clears it behind, so it also uploads the table anew: us per pass is an",
             "upper bound.  `profiles/serve_cols.md` gives 33 us per pass for the scheduler launch and the synchronisation of one pass.", "",
             "| model | run | passes | seconds | us per pass over (a) | rows equal |", "|---|---|---|---|---|---|"]
    label = {"a": "(a) no automaton", "b": "(b) never matches", "c_device": "(c) ends requests, device", "c_host": "(c) at the cap + host cut"}
    for r in results:
        for k in ("a", "b", "c_device", "c_host"):
            lines.append(f"| {r['model']} | {label[k]} | {r['runs'][k]['passes']} | {r['runs'][k]['seconds']:.4f} | "
                         f"{r['per_pass_us']:.1f} | {r['rows_equal']} |" if k == "b" else
                         f"| {r['model']} | {label[k]} | {r['runs'][k]['passes']} | {r['runs'][k]['seconds']:.4f} | | |")
    lines += ["", "The automaton of (b) and its lift on the host (`stop_automaton_from_strings` over a vocabulary whose token v spells `v,`):", "",
              "| model | vocabulary | strings | states | edges | table bytes | lift seconds |", "|---|---|---|---|---|---|---|"]
    for r in results:
        n = r["never"]
        lines.append(f"| {r['model']} | {n.get('vocab', '')} | {' '.join(repr(s) for s in n['strings'])} | {n['states']} | {n['edges']} | {n['bytes']} | {r['lift_seconds']:.2f} |")
    if a.ab:
        lines += ["", "(a) in processes of their own, this tree and a checkout of the commit before by turns (seconds, best of 3 each):", "",
                  "| model | this tree | the commit before |", "|---|---|---|"]
        for r in results:
            lines.append(f"| {r['model']} | {' '.join(f'{x:.4f}' for x in r['ab']['ours'])} | {' '.join(f'{x:.4f}' for x in r['ab']['parent'])} |")
    if not results:
        lines.append("not taken")
    with open(os.path.join(a.out, "stop_seq.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if not failed and results and all(r["rows_equal"] and r["passes_equal"] for r in results) else 1


def main_stop(a):
    results = []
    for name in a.models.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", name, "--ctx", str(a.ctx),
               "--ckpt-dir", a.ckpt_dir, "--seed", str(a.seed), "--stop"]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            print(f"[bench_serve] {name}: exit status {p.returncode}; stopping here", file=sys.stderr)
            break
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "serve_cols_stop.json"), "w") as f:
        json.dump(results, f, indent=1)
    lines = [STOP_MARK, "",
             "Written by `tools/bench_serve.py --stop` (context %d per slot): 64 requests through 32 slots (8 prompts of 1 to 199 tokens," % a.ctx,
             "each sent 8 times, interleaved), a cap of 256 new tokens, and a stop set of at most 8 tokens picked from the rows of the",
             "existing loop -- the token that shortens them most, again and again -- until the requests emit at most half the cap in total.",
             "Wall time per call, best of 3 behind a warm-up call.  at the cap = `q3_generate_many_greedy` with n_new = 256 plus the host cut; stop = `q3_generate_many_stop`; n_emit = `q3_generate_many_greedy` with n_new = n_emit,",
             "the same passes with one synchronisation.  us per pass = (stop - n_emit) / passes: the scheduler launches and the",
             "synchronisation of one pass.", "",
             "| model | stop set | tokens emitted / cap | loop | passes | seconds | us per pass | rows equal | passes equal |", "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        for k, label in (("at_cap", "at the cap"), ("stop", "stop"), ("n_emit", "n_emit")):
            lines.append(f"| {r['model']} | {' '.join(str(t) for t in r['stop_set'])} | {r['sum_n_emit']} / {r['sum_n_new']} | {label} | {r[k]['passes']} | "
                         f"{r[k]['seconds']:.3f} | {r['per_pass_us']:.1f} | {r['rows_equal']} | {r['passes_equal']} |" if k == "stop" else
                         f"| {r['model']} | | | {label} | {r[k]['passes']} | {r[k]['seconds']:.3f} | | | |")
    if not results:
        lines.append("not taken")
    md_path = os.path.join(a.out, "serve_cols.md")
    old = open(md_path).read() if os.path.exists(md_path) else ""
    if STOP_MARK in old:                                               # replace the earlier section, up to the next heading of its level
        at = old.index(STOP_MARK)
        nxt = old.find("\n## ", at + 1)
        old = old[:at].rstrip("\n") + "\n" + (old[nxt:] if nxt >= 0 else "")
    with open(md_path, "w") as f:
        f.write(old.rstrip("\n") + "\n\n" + "\n".join(lines) + "\n")
    ok = len(results) == len(a.models.split(",")) and all(r["rows_equal"] and r["passes_equal"] and r["half_reached"] for r in results)
    return 0 if ok else 1


def memcpy_loop_seconds(n_layers, row_floats, n_rows, ctx, n_dst, reps=3):
    """the yardstick of the broadcast: 2 * n_layers * n_dst hipMemcpyAsync calls, device to device, that move the rows of every layer of
    both caches from one block to n_dst blocks laid out like slots of `ctx` rows; best of `reps` behind a warm-up round"""
    import ctypes as C
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    layer = 4 * ctx * row_floats                                       # bytes between two layers of a slot's cache
    slot = n_layers * layer
    run = 4 * n_rows * row_floats
    bufs = []
    for _ in range(2):                                                 # key and value: n_dst + 1 slots each
        ptr = C.c_void_p()
        if hip.hipMalloc(C.byref(ptr), (n_dst + 1) * slot) != 0:
            raise RuntimeError("hipMalloc failed")
        hip.hipMemset(ptr, 1, (n_dst + 1) * slot)
        bufs.append(ptr.value)
    best = None
    for rep in range(reps + 1):
        hip.hipDeviceSynchronize()
        t0 = time.perf_counter()
        for base in bufs:
            for l in range(n_layers):
                for d in range(1, n_dst + 1):
                    if hip.hipMemcpyAsync(base + d * slot + l * layer, base + l * layer, run, 3, None) != 0:      # hipMemcpyDeviceToDevice
                        raise RuntimeError("hipMemcpyAsync failed")
        if hip.hipDeviceSynchronize() != 0:
            raise RuntimeError("hipDeviceSynchronize failed")
        dt = time.perf_counter() - t0
        if rep > 0:
            best = dt if best is None else min(best, dt)
    for b in bufs:
        hip.hipFree(b)
    return best


def worker_prefix(name, ctx, ckpt_dir, seed, n_prefix):
    import numpy as np
    import qwen3_rs_amd as q3
    ck = q3.checkpoint
    shape = ck.SHAPES[name]
    path = os.path.join(ckpt_dir, f"{name}-seed{seed}.q3bin")
    ck.ensure_synthetic_checkpoint(path, shape, seed=seed)
    rng = np.random.default_rng(7)
    n_req, ms, n_gen = 64, 32, 32
    pre = ck.iter_prompt_tokens(shape, seed + 40, n_prefix)
    suf = [ck.iter_prompt_tokens(shape, seed + 50 + r, int(n)) for r, n in enumerate(rng.integers(1, 65, n_req))]
    full = [pre + s for s in suf]
    nnew = [n_gen] * n_req

    def best(call, n=3):
        call()                                                         # plans, scratch
        dts = []
        for _ in range(n):
            t0 = time.perf_counter()
            out = call()
            dts.append(time.perf_counter() - t0)
        return min(dts), out
    with q3.TransformerBuilder(path).with_ctx_length(ctx).build() as t:
        t.batch_init(ms, ctx)
        dt_cols, (rows_cols, st_cols) = best(lambda: t.generate_many_greedy(full, nnew))
        dt_dense, (rows_dense, st_dense, ds_dense) = best(lambda: t.generate_many_dense(full, nnew, None, 64))
        dt_set, _ = best(lambda: t.batch_prefix_set(pre))
        dt_pre, (rows_pre, st_pre) = best(lambda: t.generate_many_prefix(suf, nnew))
        n_dst = ms - 1
        dt_bcast, _ = best(lambda: t.batch_copy_rows(0, list(range(1, ms)), 0, n_prefix), 5)
    moved = 2 * shape.n_layers * n_prefix * shape.kv_dim * 4 * (1 + n_dst)                 # read once, written n_dst times
    dt_memcpy = memcpy_loop_seconds(shape.n_layers, shape.kv_dim, n_prefix, ctx, n_dst)
    res = {"model": name, "ctx": ctx, "prefix": n_prefix, "requests": n_req, "slots": ms, "n_new": n_gen,
           "rows_equal": rows_cols == rows_dense == rows_pre,
           "columns": {"passes": st_cols.passes, "blocks": 0, "seconds": dt_cols},
           "dense": {"passes": st_dense.passes, "blocks": ds_dense.blocks, "seconds": dt_dense},
           "prefix_loop": {"passes": st_pre.passes, "blocks": 0, "seconds": dt_pre},
           "prefix_set_seconds": dt_set,
           "bcast": {"n_dst": n_dst, "bytes": moved, "seconds": dt_bcast, "bytes_per_s": moved / dt_bcast},
           "memcpy_loop": {"calls": 2 * shape.n_layers * n_dst, "bytes": 2 * moved * n_dst // (1 + n_dst), "seconds": dt_memcpy,
                           "bytes_per_s": (2 * moved * n_dst // (1 + n_dst)) / dt_memcpy}}
    print("RESULT " + json.dumps(res))


def main_prefix(a):
    results = []
    for name in a.models.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", name, "--ctx", str(a.ctx),
               "--ckpt-dir", a.ckpt_dir, "--seed", str(a.seed), "--prefix", str(a.prefix)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            print(f"[bench_serve] {name}: exit status {p.returncode}; stopping here", file=sys.stderr)
            break
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "serve_cols_prefix.json"), "w") as f:
        json.dump(results, f, indent=1)
    lines = [PREFIX_MARK + f" (prefix of {a.prefix} tokens)", "",
             "Written by `tools/bench_serve.py --prefix` (context %d per slot): 64 requests through 32 slots that all begin with the same" % a.ctx,
             "prefix, suffixes of 1 to 64 tokens, 32 new tokens each.  Wall time per call, best of 3 behind a warm-up call.  columns =",
             "`q3_generate_many_greedy` on the full prompts; dense = `q3_generate_many_dense` (dense_min 64) on the full prompts; prefix =",
             "`q3_generate_many_prefix` on the suffixes with the prefix resident (its broadcast into the 32 slots included); prefix_set =",
             "`q3_batch_prefix_set` on its own, paid once per prefix.", "",
             "| model | loop | passes | blocks | seconds | against dense | rows equal |", "|---|---|---|---|---|---|---|"]
    for r in results:
        for k, label in (("columns", "columns"), ("dense", "dense"), ("prefix_loop", "prefix")):
            lines.append(f"| {r['model']} | {label} | {r[k]['passes']} | {r[k]['blocks']} | {r[k]['seconds']:.3f} | "
                         f"{r['dense']['seconds'] / r[k]['seconds']:.2f}x | {r['rows_equal']} |")
        lines.append(f"| {r['model']} | prefix_set | | | {r['prefix_set_seconds']:.3f} | | |")
    lines += ["", "The copy of the prefix rows from slot 0 to the 31 other slots: one launch of `k_kv_rows_bcast` through `q3_batch_copy_rows` (wall time",
              "of the call, its synchronisation included, best of 5; bytes = read once + written 31 times) next to a loop of",
              "2 x layers x 31 `hipMemcpyAsync` calls between buffers of the same layout (bytes = read 31 times + written 31 times; best of 3):", "",
              "| model | path | calls | MB moved | ms | GB/s |", "|---|---|---|---|---|---|"]
    for r in results:
        b, m = r["bcast"], r["memcpy_loop"]
        lines.append(f"| {r['model']} | k_kv_rows_bcast | 1 | {b['bytes'] / 1e6:.0f} | {1e3 * b['seconds']:.3f} | {b['bytes_per_s'] / 1e9:.0f} |")
        lines.append(f"| {r['model']} | hipMemcpyAsync loop | {m['calls']} | {m['bytes'] / 1e6:.0f} | {1e3 * m['seconds']:.3f} | {m['bytes_per_s'] / 1e9:.0f} |")
    if not results:
        lines.append("not taken")
    md_path = os.path.join(a.out, "serve_cols.md")
    old = open(md_path).read() if os.path.exists(md_path) else ""
    if PREFIX_MARK in old:                                             # replace the earlier section, up to the next heading of its level
        at = old.index(PREFIX_MARK)
        nxt = old.find("\n## ", at + 1)
        old = old[:at].rstrip("\n") + "\n" + (old[nxt:] if nxt >= 0 else "")
    with open(md_path, "w") as f:
        f.write(old.rstrip("\n") + "\n\n" + "\n".join(lines) + "\n")
    return 0 if len(results) == len(a.models.split(",")) and all(r["rows_equal"] for r in results) else 1


def main_dense(a):
    results = []
    for name in a.models.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", name, "--ctx", str(a.ctx),
               "--ckpt-dir", a.ckpt_dir, "--seed", str(a.seed), "--dense-min", str(a.dense_min)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            print(f"[bench_serve] {name}: exit status {p.returncode}; stopping here", file=sys.stderr)
            break
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "serve_cols_dense.json"), "w") as f:
        json.dump(results, f, indent=1)
    lines = [DENSE_MARK + f" (dense_min {a.dense_min})", "",
             "Written by `tools/bench_serve.py --dense-min` (context %d per slot).  `q3_generate_many_dense` against" % a.ctx,
             "`q3_generate_many_greedy` on the same engine, best of 2 calls each behind a warm-up call; tok/s counts prompt + generated",
             "tokens; prompt tok/s is the same mix with one new token per request.", "",
             "| model | requests | loop | passes | blocks | seconds | requests/s | tok/s | prompt tok/s | tokens equal |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        for label, d in r["requests"].items():
            for k in ("columns", "dense"):
                lines.append(f"| {r['model']} | {label} | {k} | {d[k]['passes']} | {d[k].get('blocks', '')} | {d[k]['seconds']:.3f} | {d[k]['req_s']:.2f} | "
                             f"{d[k]['tok_s']:.0f} | {d[k]['prompt_tok_s']:.0f} | {d['tokens_equal']} |")
    lines += ["", "One block (wall time per call, best of 5): `q3_batch_prefill_slots` of 8 runs of 256 tokens into 8 slots against",
              "`q3_prefill_batched` of one 2,048-token prompt (which also runs the classifier once and returns a token):", "",
              "| model | prefill_slots 8 x 256 ms | prefill_batched 1 x 2,048 ms |", "|---|---|---|"]
    for r in results:
        lines.append(f"| {r['model']} | {r['block_ms']['prefill_slots_8x256']:.2f} | {r['block_ms']['prefill_batched_1x2048']:.2f} |")
    md_path = os.path.join(a.out, "serve_cols.md")
    old = open(md_path).read() if os.path.exists(md_path) else ""
    if DENSE_MARK in old:                                              # replace the earlier section, up to the next heading of its level
        at = old.index(DENSE_MARK)
        nxt = old.find("\n## ", at + 1)
        old = old[:at].rstrip("\n") + "\n" + (old[nxt:] if nxt >= 0 else "")
    with open(md_path, "w") as f:
        f.write(old.rstrip("\n") + "\n\n" + "\n".join(lines) + "\n")
    return 0 if len(results) == len(a.models.split(",")) else 1


def main_sampled(a):
    results = []
    for name in a.models.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", name, "--ctx", str(a.ctx),
               "--ckpt-dir", a.ckpt_dir, "--seed", str(a.seed), "--temperature", str(a.temperature), "--topp", str(a.topp)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            print(f"[bench_serve] {name}: exit status {p.returncode}; stopping here", file=sys.stderr)
            break
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "serve_cols_sampled.json"), "w") as f:
        json.dump(results, f, indent=1)
    lines = [SAMPLED_MARK + f" (temperature {a.temperature}, top-p {a.topp})", "",
             "Written by `tools/bench_serve.py --temperature --topp` (context %d per slot).  Wall time per call of one pass of" % a.ctx,
             "single-position columns at position 8, no logits read back, median of 15 calls per form, the forms measured one after",
             "the other on one engine: greedy = `q3_batch_step_cols` with the batch sampler at temperature 0.", "",
             "| model | columns | greedy ms | 1 column draws ms | all columns draw ms |", "|---|---|---|---|---|"]
    for r in results:
        for w, d in r["pass_ms"].items():
            lines.append(f"| {r['model']} | {w} | {d['greedy']:.3f} | {d['one_draw']:.3f} | {d['all_draw']:.3f} |")
    lines += ["", "Requests through `q3_generate_many_sampled` against `q3_generate_many_greedy` (best of 2 calls each; tok/s counts",
              "prompt + generated tokens):", "", "| model | requests | loop | passes | seconds | tok/s | gen tok/s |", "|---|---|---|---|---|---|---|"]
    for r in results:
        for label, d in r["requests"].items():
            for k in ("greedy", "sampled"):
                lines.append(f"| {r['model']} | {label} | {k} | {d[k]['passes']} | {d[k]['seconds']:.3f} | {d[k]['tok_s']:.0f} | {d[k]['gen_tok_s']:.0f} |")
    md_path = os.path.join(a.out, "serve_cols.md")
    old = open(md_path).read() if os.path.exists(md_path) else ""
    if SAMPLED_MARK in old:                                            # replace the earlier section, up to the next heading of its level
        at = old.index(SAMPLED_MARK)
        nxt = old.find("\n## ", at + 1)
        old = old[:at].rstrip("\n") + "\n" + (old[nxt:] if nxt >= 0 else "")
    with open(md_path, "w") as f:
        f.write(old.rstrip("\n") + "\n\n" + "\n".join(lines) + "\n")
    return 0 if len(results) == len(a.models.split(",")) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="qwen3-0.6b,qwen3-8b")
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--limit", type=int, default=420, help="seconds per model")
    ap.add_argument("--seed", type=int, default=1236)
    ap.add_argument("--ckpt-dir", default=os.environ.get("Q3_CKPT_DIR", "/tmp"))
    ap.add_argument("--worker")
    ap.add_argument("--temperature", type=float, help="with --topp: the workloads under the sampler (appends to serve_cols.md)")
    ap.add_argument("--topp", type=float, default=0.95)
    ap.add_argument("--dense-min", type=int, help="long prompts through dense blocks against the column loop (appends to serve_cols.md; context 2,304)")
    ap.add_argument("--stop", action="store_true", help="stop tokens in the device loop against the loop at the cap (appends to serve_cols.md)")
    ap.add_argument("--stop-seq", action="store_true", help="stop sequences in the device loop: no automaton, one that never matches, one that ends requests (writes stop_seq.md)")
    ap.add_argument("--ab", help="with --stop-seq: a checkout of the commit before, its library built; (a) also runs there")
    ap.add_argument("--tree", help=argparse.SUPPRESS)                  # worker of --ab: the tree whose package and library run (a)
    ap.add_argument("--prefix", type=int, help="requests that share a prefix of this many tokens against the loops on the full prompts (appends to serve_cols.md)")
    a = ap.parse_args()
    if a.prefix is not None:
        a.ctx = max(a.ctx, (a.prefix + 64 + 32 + 255) // 256 * 256)
        if a.worker:
            worker_prefix(a.worker, a.ctx, a.ckpt_dir, a.seed, a.prefix)
            return 0
        return main_prefix(a)
    if a.stop_seq:
        if a.worker:
            worker_stop_seq(a.worker, a.ctx, a.ckpt_dir, a.seed, a.tree is not None)
            return 0
        return main_stop_seq(a)
    if a.stop:
        if a.worker:
            worker_stop(a.worker, a.ctx, a.ckpt_dir, a.seed)
            return 0
        return main_stop(a)
    if a.dense_min is not None:
        a.ctx = max(a.ctx, 2304)
        if a.worker:
            worker_dense(a.worker, a.ctx, a.ckpt_dir, a.seed, a.dense_min)
            return 0
        return main_dense(a)
    if a.temperature is not None:
        if a.worker:
            worker_sampled(a.worker, a.ctx, a.ckpt_dir, a.seed, a.temperature, a.topp)
            return 0
        return main_sampled(a)
    if a.worker:
        worker(a.worker, a.ctx, a.ckpt_dir, a.seed)
        return 0
    results = []
    for name in a.models.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", name, "--ctx", str(a.ctx),
               "--ckpt-dir", a.ckpt_dir, "--seed", str(a.seed)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            print(f"[bench_serve] {name}: exit status {p.returncode}; stopping here", file=sys.stderr)
            break
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "serve_cols.json"), "w") as f:
        json.dump(results, f, indent=1)
    md_path = os.path.join(a.out, "serve_cols.md")
    keep = ""
    if os.path.exists(md_path):
        old = open(md_path).read()
        marks = [old.index(m) for m in (AB_MARK, SAMPLED_MARK, DENSE_MARK, STOP_MARK, PREFIX_MARK) if m in old]      # sections other runs wrote
        if marks:
            keep = old[min(marks):]
    lines = ["# Ragged column passes: pass cost and request throughput", "",
             "Written by `tools/bench_serve.py` (synthetic full-size checkpoints, one MI355X, context %d per slot)." % a.ctx, "",
             "## (a) One 32-column pass of 32 single-position slots against a `q3_forward_batch` step", "",
             "Wall time per call, no logits read back, median of 15 alternating calls.", "",
             "| model | position | forward_batch ms | step_cols ms | ratio |", "|---|---|---|---|---|"]
    for r in results:
        for p0 in (8, 256):
            d = r[f"pass_ms_pos{p0}"]
            lines.append(f"| {r['model']} | {p0} | {d['forward_batch']:.3f} | {d['step_cols']:.3f} | {d['step_cols'] / d['forward_batch']:.3f} |")
    lines += ["", "## (b) Requests: `q3_generate_many_greedy` against prompts stepped through `q3_forward_batch`", "",
              "tok/s counts every token that goes through the model (prompt + generated); gen tok/s the generated ones only.", "",
              "| model | requests | path | passes | seconds | tok/s | gen tok/s | tokens equal |", "|---|---|---|---|---|---|---|---|"]
    for r in results:
        for label, d in r["requests"].items():
            for k in ("many", "stepped"):
                lines.append(f"| {r['model']} | {label} | {k} | {d[k]['passes']} | {d[k]['seconds']:.3f} | {d[k]['tok_s']:.0f} | "
                             f"{d[k]['gen_tok_s']:.0f} | {d['tokens_equal']} |")
    with open(md_path, "w") as f:
        f.write("\n".join(lines) + "\n" + ("\n" + keep if keep else ""))
    return 0 if len(results) == len(a.models.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
