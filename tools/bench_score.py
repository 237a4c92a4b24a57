#!/usr/bin/env python3
"""What per-position scores through dense blocks (include/qwen3_hip.h section 2l) cost on the full-size synthetic checkpoints.

    python tools/bench_score.py [--models qwen3-0.6b,qwen3-8b] [--ctx 1024] [--out profiles] [--limit 500] [--reps 5]

Every model is measured in a child process of its own under a time limit (one faulting run never starts the next).  Per model,
32 slots, and for 64 prompts of 64 tokens and 64 prompts of 512 tokens (two waves of 32 prompts each):
  (a) q3_score_many over all positions, one call;
  (b) the same call with score_from = len - 8: eight records per prompt;
  (c) q3_embed_many with flags 0 on the same prompts: the cost of the blocks alone;
  (d) the per-token way that needs no q3_score_many: q3_forward for every position, the logits read back, a log-sum-exp on the
      host (numpy, float64).  It is measured on 4 of the prompts and the time is scaled by requests / 4.
The paths are repeated in turn behind one warm-up round, in one process: the three batched calls, which start one place further
on in every repetition, then (d) (tools/bench_choice.py says why); the table holds the median wall time of a call.
One more call of (a) runs with Q3_DEBUG_TIMING set: the library then records event pairs around the launch groups of every chunk
and prints their means, which the tool reads back from stderr.
The log-probs of (a) must lie within 2 V 2^-24 of (d)'s on the 4 prompts (tests/test_score.py holds them to the bits).
Writes <out>/score.json and <out>/score.md.

    python tools/bench_score.py --top 1,20,64 [--models qwen3-0.6b] [--ab PARENT_TREE] ...

measures the k best instead (section 2m) and writes <out>/score_top.json and <out>/score_top.md; the default run and its two files
are untouched.  Per model and K, on 64 prompts of 512 tokens, alternating in one process behind a warm-up round:
  (a) q3_score_top_many over all positions, one call;
  (b) q3_score_many on the same prompts;
  (c) the per-token way: q3_forward for every position, the logits read back, np.argpartition and a sort of the K best on the
      host, on 4 of the prompts, scaled by requests / 4.
The added cost per chunk is ((a) - (b)) / chunks; one more call of (a) under Q3_DEBUG_TIMING gives the library's own figure for
the selection's two launches.  On the 4 prompts the answers of (a) are held to q3_forward's rows: the logit listed is the row's
at the listed id, bit for bit, and the K logits are the row's K largest, in order (ids may differ from (c)'s only where logits
tie: (c) knows nothing of the order among equals; tests/test_score_top.py holds the ids to a host sort of the keys).
--ab PARENT_TREE: q3_score_many alone (64 x 512, all positions), a child process per measurement that imports the package and
loads the library of PARENT_TREE or of this tree by turns, three times each: the A/B of tools/ab_libs.sh for this call.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (--ab: a child measures the package and the library of another checkout)
sys.path.insert(0, os.path.join(os.environ.get("Q3_BENCH_TREE", ROOT), "qwen3-rs_amd"))

SLOTS = 32
PER_TOKEN_PROMPTS = 4
TAIL = 8
# the classifier launch of a 32-column pass, microseconds: what a chunk's tail contains
CLASSIFIER_US = {"qwen3-0.6b": 29.9, "qwen3-8b": 110.0}


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def timed_groups(call):
    """run call() with Q3_DEBUG_TIMING set and stderr going to a file; the library's per-chunk means, or None"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        os.environ["Q3_DEBUG_TIMING"] = "1"
        try:
            call()
        finally:
            del os.environ["Q3_DEBUG_TIMING"]
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode(errors="replace")
    m = re.search(r"(\d+) chunks, us per chunk: gather ([\d.]+) classifier ([\d.]+) exp ([\d.]+) sum ([\d.]+)(?: top ([\d.]+))?", text)
    if not m:
        return None
    g = {"chunks": int(m.group(1)), "gather": float(m.group(2)), "classifier": float(m.group(3)), "exp": float(m.group(4)), "sum": float(m.group(5))}
    if m.group(6) is not None:
        g["top"] = float(m.group(6))
    return g


def worker(name, ctx, ckpt_dir, seed, reps):
    import numpy as np
    import qwen3_rs_amd as q3
    ck = q3.checkpoint
    shape = ck.SHAPES[name]
    V = shape.vocab_size
    path = os.path.join(ckpt_dir, f"{name}-seed{seed}.q3bin")
    ck.ensure_synthetic_checkpoint(path, shape, seed=seed)
    res = {"model": name, "ctx": ctx, "slots": SLOTS, "reps": reps, "cases": {}}
    print(f"[bench_score] {name}: checkpoint ready", file=sys.stderr, flush=True)
    with q3.TransformerBuilder(path).with_ctx_length(ctx).build() as t:
        t.batch_init(SLOTS, ctx)
        for n_req, plen in ((64, 64), (64, 512)):
            print(f"[bench_score] {name}: {n_req} prompts of {plen} tokens", file=sys.stderr, flush=True)
            prompts = [ck.iter_prompt_tokens(shape, seed + 50 + r, plen) for r in range(n_req)]
            tail_from = [plen - TAIL] * n_req

            def score_all():
                return t.score_many(prompts)

            def score_tail():
                return t.score_many(prompts, tail_from)

            def embed():
                return t.embed_many(prompts, normalize=False)

            def per_token():
                out = []
                for p in prompts[:PER_TOKEN_PROMPTS]:
                    lp = np.zeros(plen - 1)
                    for i in range(plen - 1):
                        z = t.forward(p[i], i).astype(np.float64)
                        mx = z.max()
                        lp[i] = z[p[i + 1]] - mx - np.log(np.exp(z - mx).sum())
                    out.append(lp)
                return out
            paths = (("score_all", score_all), ("score_tail8", score_tail), ("embed_many", embed), ("per_token", per_token))
            recs, st = score_all()
            _, st8 = score_tail()
            ref = per_token()
            embed()                                                     # (with the three calls above: the warm-up round)
            worst = max(float(np.max(np.abs(q3.logprobs_of(recs[r]) - ref[r]))) for r in range(PER_TOKEN_PROMPTS))
            dts = {k: [] for k, _ in paths}
            for i in range(reps):                                       # alternating; the batched calls rotate, per_token stays last
                for k, call in paths[i % 3:3] + paths[:i % 3] + paths[3:]:
                    t0 = time.perf_counter()
                    call()
                    dts[k].append(time.perf_counter() - t0)
            med = {k: median(v) for k, v in dts.items()}
            scale = n_req / PER_TOKEN_PROMPTS
            tail_us = 1e6 * (med["score_all"] - med["embed_many"]) / st.chunks
            res["cases"][f"{n_req} x {plen}"] = {
                "requests": n_req, "prompt_len": plen, "waves": st.waves, "blocks": st.blocks, "chunks": st.chunks, "scored": st.scored,
                "chunks_tail8": st8.chunks, "scored_tail8": st8.scored,
                "logprob_max_abs_diff": worst, "logprobs_close": bool(worst <= 2 * V * 2.0 ** -24),
                "seconds": med, "all_seconds": dts, "per_token_scaled_seconds": med["per_token"] * scale,
                "speedup_over_per_token": med["per_token"] * scale / med["score_all"],
                "tail_us_per_chunk": tail_us,
                "tail8_minus_embed_plus_tails_ms": 1e3 * (med["score_tail8"] - (med["embed_many"] + st8.chunks * tail_us * 1e-6)),
                "groups_us_per_chunk": timed_groups(score_all),
            }
    print("RESULT " + json.dumps(res))


def worker_top(name, ctx, ckpt_dir, seed, reps, ks):
    import numpy as np
    import qwen3_rs_amd as q3
    ck = q3.checkpoint
    shape = ck.SHAPES[name]
    path = os.path.join(ckpt_dir, f"{name}-seed{seed}.q3bin")
    ck.ensure_synthetic_checkpoint(path, shape, seed=seed)
    n_req, plen = 64, 512
    res = {"model": name, "ctx": ctx, "slots": SLOTS, "reps": reps, "requests": n_req, "prompt_len": plen, "k": {}}
    with q3.TransformerBuilder(path).with_ctx_length(ctx).build() as t:
        t.batch_init(SLOTS, ctx)
        prompts = [ck.iter_prompt_tokens(shape, seed + 50 + r, plen) for r in range(n_req)]
        for k in ks:
            print(f"[bench_score] {name}: top {k}", file=sys.stderr, flush=True)

            def score_top():
                return t.score_top_many(prompts, k)

            def score_all():
                return t.score_many(prompts)

            def per_token():
                out = []
                for p in prompts[:PER_TOKEN_PROMPTS]:
                    ids = np.zeros((plen - 1, k), dtype=np.int64)
                    for i in range(plen - 1):
                        z = t.forward(p[i], i)
                        best = np.argpartition(z, z.size - k)[z.size - k:]
                        ids[i] = best[np.argsort(z[best])[::-1]]
                    out.append(ids)
                return out

            def agrees(got):
                for r, p in enumerate(prompts[:PER_TOKEN_PROMPTS]):
                    for i in range(plen - 1):
                        z = t.forward(p[i], i)
                        top = got[1][r][i]
                        if z[top["index"]].tobytes() != top["logit"].tobytes() or not np.array_equal(top["logit"], np.sort(z)[::-1][:k]):
                            return False
                return True
            paths = (("score_top", score_top), ("score_all", score_all), ("per_token", per_token))
            got = score_top()
            score_all()
            per_token()                                                 # (with the two calls above: the warm-up round)
            same = agrees(got)
            dts = {n: [] for n, _ in paths}
            for i in range(reps):                                       # alternating; the two batched calls swap places, per_token stays last
                for n, call in paths[i % 2:2] + paths[:i % 2] + paths[2:]:
                    t0 = time.perf_counter()
                    call()
                    dts[n].append(time.perf_counter() - t0)
            med = {n: median(v) for n, v in dts.items()}
            st = got[3]
            scaled = med["per_token"] * n_req / PER_TOKEN_PROMPTS
            res["k"][str(k)] = {"chunks": st.chunks, "scored": st.scored, "agrees_with_forward": bool(same), "seconds": med, "all_seconds": dts,
                                "added_us_per_chunk": 1e6 * (med["score_top"] - med["score_all"]) / st.chunks,
                                "per_token_scaled_seconds": scaled, "speedup_over_per_token": scaled / med["score_top"],
                                "groups_us_per_chunk": timed_groups(score_top)}
    print("RESULT " + json.dumps(res))


def worker_ab(name, ctx, ckpt_dir, seed, reps):
    """q3_score_many over 64 prompts of 512 tokens with whatever package and library Q3_BENCH_TREE names"""
    import qwen3_rs_amd as q3
    ck = q3.checkpoint
    shape = ck.SHAPES[name]
    path = os.path.join(ckpt_dir, f"{name}-seed{seed}.q3bin")
    ck.ensure_synthetic_checkpoint(path, shape, seed=seed)
    with q3.TransformerBuilder(path).with_ctx_length(ctx).build() as t:
        t.batch_init(SLOTS, ctx)
        prompts = [ck.iter_prompt_tokens(shape, seed + 50 + r, 512) for r in range(64)]
        t.score_many(prompts)
        dts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            t.score_many(prompts)
            dts.append(time.perf_counter() - t0)
    print("RESULT " + json.dumps({"build_id": q3.load_library().q3_build_id().decode(), "seconds": dts, "median": median(dts)}))


def write_top_md(results, ab, a):
    lines = ["# The k best tokens and the target's rank: `q3_score_top_many`", "",
             "Written by `tools/bench_score.py --top` (synthetic full-size checkpoints, one MI355X, %d slots, context %d per slot): 64" % (SLOTS, a.ctx),
             "prompts of 512 tokens, every position scored.  Wall time per call, median of %d repetitions that alternate the paths in one" % a.reps,
             "process behind a warm-up round.  top K = `q3_score_top_many`; score = `q3_score_many` on the same prompts; per token =",
             "`q3_forward` for every position, the logits read back, `np.argpartition` and a sort of the K best, measured on %d of the" % PER_TOKEN_PROMPTS,
             "prompts and scaled by requests / %d.  added us / chunk = (top K - score) / chunks; `top` group = the mean of the event pairs the" % PER_TOKEN_PROMPTS,
             "library records around k_score_top_part + k_score_top_merge of every chunk under `Q3_DEBUG_TIMING` (one call), beside the",
             "groups of section 2l from the same call.  Numbers of one box.", "",
             "| model | K | chunks | top K s | score s | added us / chunk | `top` group us | classifier | exp | sum | per token s (scaled) | times faster | the K largest logits of q3_forward's rows, at their ids |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        for k, c in r["k"].items():
            g = c["groups_us_per_chunk"] or {}
            lines.append(f"| {r['model']} | {k} | {c['chunks']} | {c['seconds']['score_top']:.4f} | {c['seconds']['score_all']:.4f} | {c['added_us_per_chunk']:.1f} | "
                         + " | ".join(f"{g[n]:.1f}" if n in g else "not taken" for n in ("top", "classifier", "exp", "sum"))
                         + f" | {c['per_token_scaled_seconds']:.2f} | {c['speedup_over_per_token']:.1f} | {c['agrees_with_forward']} |")
    lines += ["", "spread of the repetitions, ms (smallest - largest):", ""]
    for r in results:
        for k, c in r["k"].items():
            sp = {n: f"{1e3 * min(v):.2f} - {1e3 * max(v):.2f}" for n, v in c["all_seconds"].items()}
            lines.append(f"- {r['model']}, K = {k}: top K {sp['score_top']}; score {sp['score_all']}")
    lines += ["", "## `q3_score_many` against the parent commit", ""]
    if ab:
        lines += ["A child process per measurement, the parent's package and library and this tree's by turns (the A/B of `tools/ab_libs.sh` for this",
                  "call): median seconds of %d calls over the same 64 x 512 prompts, in the order taken." % a.reps, "",
                  "| model | round | parent (build id) | parent s | this tree (build id) | this tree s |", "|---|---|---|---|---|---|"]
        for name, rounds in ab.items():
            for i, (old, new) in enumerate(rounds):
                lines.append(f"| {name} | {i + 1} | {old['build_id']} | {old['median']:.4f} | {new['build_id']} | {new['median']:.4f} |")
            olds, news = [o["median"] for o, _ in rounds], [n["median"] for _, n in rounds]
            lines += ["", f"- {name}: parent {min(olds):.4f} - {max(olds):.4f} s, this tree {min(news):.4f} - {max(news):.4f} s over the rounds; medians "
                          f"{median(olds):.4f} and {median(news):.4f} s, {100 * (median(news) / median(olds) - 1):+.2f} %; the same build's rounds differ by "
                          f"{100 * (max(olds) / min(olds) - 1):.2f} % (parent) and {100 * (max(news) / min(news) - 1):.2f} % (this tree)."]
    else:
        lines.append("not taken")
    with open(os.path.join(a.out, "score_top.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


def run_child(cmd, name, env=None):
    """one measurement in a child of its own under the time limit; its RESULT line, or None"""
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)      # the worker's progress lines go straight to stderr
    if p.returncode != 0:
        print(f"[bench_score] {name}: exit status {p.returncode}; stopping here", file=sys.stderr)
        return None
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main_top(a):
    ks = [int(v) for v in a.top.split(",")]
    base = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--ctx", str(a.ctx), "--ckpt-dir", a.ckpt_dir,
            "--seed", str(a.seed), "--reps", str(a.reps)]
    results, ab, ok = [], {}, True
    for name in a.models.split(","):
        print(f"[bench_score] {name} --top {a.top} ...", file=sys.stderr, flush=True)
        r = run_child(base + ["--worker", name, "--top", a.top], name)
        if r is None:
            ok = False
            break
        results.append(r)
        if a.ab:
            rounds = []
            for _ in range(3):
                pair = []
                for tree in (os.path.abspath(a.ab), ROOT):
                    got = run_child(base + ["--worker-ab", name], name, dict(os.environ, Q3_BENCH_TREE=tree))
                    if got is None:
                        break
                    pair.append(got)
                if len(pair) < 2:
                    ok = False
                    break
                rounds.append(pair)
            if rounds:
                ab[name] = rounds
            if not ok:
                break
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "score_top.json"), "w") as f:
        json.dump({"results": results, "ab": ab}, f, indent=1)
    write_top_md(results, ab, a)
    return 0 if ok and all(c["agrees_with_forward"] for r in results for c in r["k"].values()) else 1


def write_md(results, a):
    lines = ["# Per-position scores through dense blocks: `q3_score_many`", "",
             "Written by `tools/bench_score.py` (synthetic full-size checkpoints, one MI355X, %d slots, context %d per slot).  Wall time" % (SLOTS, a.ctx),
             "per call, median of %d repetitions that alternate the paths in one process behind a warm-up round.  score, all =" % a.reps,
             "`q3_score_many` over every position, one call; score, last 8 = the same call with `score_from = len - 8`; embed_many =",
             "`q3_embed_many` with flags 0 on the same prompts, the cost of the blocks alone; per token = `q3_forward` for every position,",
             "the logits read back and a float64 log-sum-exp in numpy, measured on %d of the prompts and scaled by requests / %d." % (PER_TOKEN_PROMPTS, PER_TOKEN_PROMPTS),
             "Numbers of one box; the pool's boxes differ by 3-6 % (README).", "",
             "| model | prompts | path | blocks | chunks | records | seconds | records/s | log-probs within 2 V 2^-24 of per token |", "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        for label, c in r["cases"].items():
            s = c["seconds"]
            rows = (("score, all", s["score_all"], c["chunks"], c["scored"], str(c["logprobs_close"])),
                    ("score, last 8", s["score_tail8"], c["chunks_tail8"], c["scored_tail8"], ""),
                    ("embed_many", s["embed_many"], "", "", ""),
                    ("per token (scaled)", c["per_token_scaled_seconds"], "", c["scored"], ""))
            for what, sec, chunks, n, ok in rows:
                rate = f"{n / sec:.0f}" if n != "" else ""
                lines.append(f"| {r['model']} | {label} | {what} | {c['blocks'] if chunks != '' or what == 'embed_many' else ''} | {chunks} | {n} | {sec:.4f} | {rate} | {ok} |")
    lines += ["", "## Against the per-token way", ""]
    for r in results:
        for label, c in r["cases"].items():
            f = c["speedup_over_per_token"]
            lines.append(f"- {r['model']}, {label}: all positions in {c['seconds']['score_all']:.3f} s against {c['per_token_scaled_seconds']:.2f} s per token "
                         f"({c['seconds']['per_token']:.3f} s for {PER_TOKEN_PROMPTS} prompts, scaled): {f:.1f} times faster: {'a win' if f > 1 else 'NOT A WIN'}.")
    lines += ["", "## The tail per chunk", "",
              "(score, all - embed_many) / chunks, beside the classifier launch of a 32-column pass it contains (DESIGN section 5), and the",
              "means of the event pairs the library records around a chunk's launch groups under `Q3_DEBUG_TIMING` (one call; the events",
              "serialise nothing, the stream is in order anyway).  spread = the smallest and the largest repetition of a path.", "",
              "| model | prompts | chunks | tail us / chunk | classifier us (section 5) | gather | classifier | exp | sum | score, all ms, spread | embed_many ms, spread |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        bar = CLASSIFIER_US.get(r["model"])
        for label, c in r["cases"].items():
            sp = {k: f"{1e3 * min(v):.2f} - {1e3 * max(v):.2f}" for k, v in c["all_seconds"].items()}
            g = c["groups_us_per_chunk"] or {}
            lines.append(f"| {r['model']} | {label} | {c['chunks']} | {c['tail_us_per_chunk']:.1f} | {bar if bar is not None else ''} | "
                         + " | ".join(f"{g[k]:.1f}" if k in g else "not taken" for k in ("gather", "classifier", "exp", "sum"))
                         + f" | {sp['score_all']} | {sp['embed_many']} |")
    lines.append("")
    for r in results:
        bar = CLASSIFIER_US.get(r["model"])
        for label, c in r["cases"].items():
            g = c["groups_us_per_chunk"]
            if bar is None:
                continue
            if c["tail_us_per_chunk"] <= 2 * bar:
                lines.append(f"- {r['model']}, {label}: the tail, {c['tail_us_per_chunk']:.1f} us, is within twice the classifier figure ({bar:.1f} us).")
            elif g:
                top = max(("gather", "exp", "sum", "classifier"), key=lambda k: g[k])
                lines.append(f"- {r['model']}, {label}: the tail, {c['tail_us_per_chunk']:.1f} us, is more than twice the classifier figure ({bar:.1f} us); "
                             f"the largest launch group is `{top}` at {g[top]:.1f} us per chunk.")
            else:
                lines.append(f"- {r['model']}, {label}: the tail, {c['tail_us_per_chunk']:.1f} us, is more than twice the classifier figure ({bar:.1f} us); the groups were not taken.")
    lines += ["", "## score_from = len - 8", "",
              "The row should cost what `q3_embed_many` costs plus its chunks' tails.  Observed difference, score last 8 - (embed_many + chunks x",
              "tail per chunk), beside the spread of the repetitions:", ""]
    for r in results:
        for label, c in r["cases"].items():
            lo, hi = min(c["all_seconds"]["score_tail8"]), max(c["all_seconds"]["score_tail8"])
            lines.append(f"- {r['model']}, {label}: {c['chunks_tail8']} chunks; difference {c['tail8_minus_embed_plus_tails_ms']:+.2f} ms; "
                         f"score last 8 between {1e3 * lo:.2f} and {1e3 * hi:.2f} ms, median {1e3 * c['seconds']['score_tail8']:.2f} ms.")
    if not results:
        lines.append("not taken")
    with open(os.path.join(a.out, "score.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="qwen3-0.6b,qwen3-8b")
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--limit", type=int, default=500, help="seconds per model")
    ap.add_argument("--seed", type=int, default=1236)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ckpt-dir", default=os.environ.get("Q3_CKPT_DIR", "/tmp"))
    ap.add_argument("--worker")
    ap.add_argument("--render", metavar="JSON", help="write <out>/score.md again from a score.json taken earlier; measures nothing")
    ap.add_argument("--top", default=None, metavar="K[,K...]", help="measure q3_score_top_many instead: <out>/score_top.json and .md")
    ap.add_argument("--ab", default=None, metavar="PARENT_TREE", help="with --top: q3_score_many of that checkout's build against this tree's")
    ap.add_argument("--worker-ab")
    a = ap.parse_args()
    if a.render:
        write_md(json.load(open(a.render)), a)
        return 0
    if a.worker_ab:
        worker_ab(a.worker_ab, a.ctx, a.ckpt_dir, a.seed, a.reps)
        return 0
    if a.worker and a.top:
        worker_top(a.worker, a.ctx, a.ckpt_dir, a.seed, a.reps, [int(v) for v in a.top.split(",")])
        return 0
    if a.worker:
        worker(a.worker, a.ctx, a.ckpt_dir, a.seed, a.reps)
        return 0
    if a.top:
        return main_top(a)
    results = []
    for name in a.models.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", name, "--ctx", str(a.ctx),
               "--ckpt-dir", a.ckpt_dir, "--seed", str(a.seed), "--reps", str(a.reps)]
        print(f"[bench_score] {name} ...", file=sys.stderr, flush=True)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)       # the worker's progress lines go straight to stderr
        if p.returncode != 0:
            print(f"[bench_score] {name}: exit status {p.returncode}; stopping here", file=sys.stderr)
            break
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "score.json"), "w") as f:
        json.dump(results, f, indent=1)
    write_md(results, a)
    ok = len(results) == len(a.models.split(",")) and all(c["logprobs_close"] and c["speedup_over_per_token"] > 1 for r in results for c in r["cases"].values())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
