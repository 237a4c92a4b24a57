#!/usr/bin/env python3
"""What top-k sampling (include/qwen3_hip.h section 2n) costs and saves, on the full-size synthetic checkpoints.

    python tools/bench_topk.py [--models qwen3-0.6b,qwen3-8b] [--ab PARENT_TREE] [--ctx 1024] [--out profiles]

Every model is measured in a child process of its own under a time limit (one faulting run never starts the next).  All forms of a
table are measured in ONE process, by turns: round r runs every form once, the table holds the median over the rounds and the
spread (min .. max) beside it.  Times are host clocks around calls that end in a device synchronisation; the first round of every
form is a warm-up and is not counted.  Per model:
  * single stream, 128 tokens from position 0, temperature 0.6 / top-p 0.95: us per token of q3_generate_greedy with the sampler
    off, and of q3_generate_sampled with top_k 0, 1, 20 and 64;
  * column passes: one q3_verify_draw pass of 2 / 8 / 32 sampled columns with every draft right (the method of
    tools/bench_spec.py), top_k 0 against 20;
  * q3_generate_many_sampled, 64 requests of 16-token prompts and 32 new tokens on 32 slots, top_k 0 against 20;
  * the slice count of the selection pass (developer build, Q3_TOPK_PARTS 8 / 16 / 32 / 64): the sampled step at top_k 20 (one
    column) and the 32-column pass.
--ab PARENT_TREE: the greedy step and the sampled step at top_k 0 of this tree against the build of another checkout, a child
process per measurement, the two trees by turns, three times each: the paths this feature must not have moved.
Writes <out>/top_k.md and top_k.json."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("Q3_BENCH_TREE", ROOT)         # (--ab: a child measures the package and the library of another checkout)
sys.path.insert(0, os.path.join(TREE, "qwen3-rs_amd"))

T, TOPP, SEED, N = 0.6, 0.95, 42, 128
TOK0 = 9


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def stat(xs, scale=1.0):
    return {"median": scale * median(xs), "min": scale * min(xs), "max": scale * max(xs)}


def by_turns(forms, rounds):
    """forms: name -> callable returning seconds; every round runs each once, the first round is the warm-up"""
    times = {k: [] for k in forms}
    for r in range(rounds + 1):
        for k, f in forms.items():
            s = f()
            if r:
                times[k].append(s)
    return times


def timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def checkpoint(q3, name, ckpt_dir, seed):
    path = os.path.join(ckpt_dir, f"{name}-seed{seed}.q3bin")
    q3.checkpoint.ensure_synthetic_checkpoint(path, q3.checkpoint.SHAPES[name], seed=seed)
    return path


def single_forms(t):
    """greedy and the sampled step under each k, on one engine"""
    def greedy():
        t.set_sampler(0.0, TOPP, SEED)
        t.reset_kv()
        return timed(lambda: t.generate_greedy(TOK0, 0, N))

    def sampled(k):
        def f():
            t.set_sampler(T, TOPP, SEED)
            t.set_top_k(k)
            t.reset_kv()
            return timed(lambda: t.generate_greedy(TOK0, 0, N))
        return f
    forms = {"greedy": greedy}
    for k in (0, 1, 20, 64):
        forms[f"top_k {k}"] = sampled(k)
    return forms


def verify_forms(engines, n):
    """one q3_verify_draw pass of n columns at position 64 with every draft right; engines: top_k -> an engine of its own, whose
    cache keeps the 64 rows of that form's sequence"""
    p, seqs, rngs = 64, {}, {}
    for k, t in engines.items():
        t.set_sampler(T, TOPP, SEED)
        t.set_top_k(k)
        t.reset_kv()
        G = t.generate_greedy(TOK0, 0, p + 40)
        t.set_sampler(T, TOPP, SEED)
        t.reset_kv()
        t.generate_greedy(TOK0, 0, p)
        rngs[k] = t.sampler_rng_state()
        seqs[k] = [G[p - 1]] + G[p:p + 40]

    def form(k):
        t = engines[k]

        def f():
            t.set_sampler(T, TOPP, rngs[k])                 # the seed IS the state: every repeat draws the same coins
            out = []
            s = timed(lambda: out.append(t.verify_draw(seqs[k][:n], p)))
            assert out[0][1] == n - 1, (k, n, out[0][1])
            return s
        return f
    return {f"top_k {k}": form(k) for k in engines}


def many_forms(t, vocab):
    prompts = [[(31 * r + 7 * i + 3) % vocab for i in range(16)] for r in range(64)]
    seeds = [1000 + r for r in range(64)]

    def form(k):
        def f():
            t.set_top_k(k)
            return timed(lambda: t.generate_many_sampled(prompts, [32] * 64, T, TOPP, seeds))
        return f
    return {"top_k 0": form(0), "top_k 20": form(20)}


def worker(name, ctx, ckpt_dir, seed, rounds):
    import qwen3_rs_amd as q3
    path = checkpoint(q3, name, ckpt_dir, seed)
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    res = {"model": name, "ctx": ctx, "rounds": rounds}

    def build():
        return q3.TransformerBuilder(path).with_ctx_length(ctx).build()

    with build() as t, build() as u:
        res["single_us_per_token"] = {k: stat(v, 1e6 / N) for k, v in by_turns(single_forms(t), rounds).items()}
        res["verify_draw_ms"] = {str(n): {k: stat(v, 1e3) for k, v in by_turns(verify_forms({0: t, 20: u}, n), 3 * rounds).items()} for n in (2, 8, 32)}
        t.batch_init(32, 256)
        res["many_sampled_ms"] = {k: stat(v, 1e3) for k, v in by_turns(many_forms(t, vocab), rounds).items()}
    # the slice count, through the developer build's switch
    if os.path.exists(q3.dev_lib_path()):
        parts = {}
        with q3.use_library(q3.dev_lib_path()):
            for p in (8, 16, 32, 64):
                os.environ["Q3_TOPK_PARTS"] = str(p)
                with build() as t:
                    got = by_turns({"32 columns: ms per pass": verify_forms({20: t}, 32)["top_k 20"]}, 3 * rounds)
                    got.update(by_turns({"one column: us per sampled token": single_forms(t)["top_k 20"]}, rounds))
                    parts[str(p)] = {"one column: us per sampled token": stat(got["one column: us per sampled token"], 1e6 / N),
                                     "32 columns: ms per pass": stat(got["32 columns: ms per pass"], 1e3)}
            os.environ.pop("Q3_TOPK_PARTS", None)
        res["parts"] = parts
    print("BENCH_TOPK " + json.dumps(res), flush=True)


def worker_ab(name, ctx, ckpt_dir, seed, rounds):
    """this process imported the package of Q3_BENCH_TREE: its greedy step and its sampled step (no top-k call: the parent has none)"""
    import qwen3_rs_amd as q3
    path = checkpoint(q3, name, ckpt_dir, seed)
    with q3.TransformerBuilder(path).with_ctx_length(ctx).build() as t:
        def greedy():
            t.set_sampler(0.0, TOPP, SEED)
            t.reset_kv()
            return timed(lambda: t.generate_greedy(TOK0, 0, N))

        def sampled():
            t.set_sampler(T, TOPP, SEED)
            t.reset_kv()
            return timed(lambda: t.generate_greedy(TOK0, 0, N))
        got = by_turns({"greedy": greedy, "sampled": sampled}, rounds)
    print("BENCH_TOPK " + json.dumps({k: stat(v, 1e6 / N) for k, v in got.items()}), flush=True)


def run_child(cmd, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("BENCH_TOPK ")]
    if r.returncode != 0 or not line:
        print(f"exit status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}", file=sys.stderr)
        return None
    return json.loads(line[0][len("BENCH_TOPK "):])


def fmt(s):
    return f"{s['median']:.1f} ({s['min']:.1f} .. {s['max']:.1f})"


def spread(s):
    return s["max"] - s["min"]


def write_md(results, ab, out):
    md = ["# Top-k sampling: what the two launches cost (`tools/bench_topk.py`)", "",
          f"Temperature {T}, top-p {TOPP}; synthetic checkpoints.  Every table was measured in one process, its forms by turns; a cell is",
          "the median over the rounds with (min .. max) beside it.  A difference counts when it exceeds the run-to-run spread (max - min)",
          "of the `top_k 0` form of the same table.", ""]
    for r in results:
        s = r["single_us_per_token"]
        md += [f"## {r['model']} (context {r['ctx']}, {r['rounds']} rounds)", "",
               f"Single stream, {N} tokens from position 0, us per token:", "", "| form | us / token |", "|---|---|"]
        md += [f"| {k} | {fmt(v)} |" for k, v in s.items()]
        base, k20 = s["top_k 0"], s["top_k 20"]
        md += ["", f"Spread of `top_k 0`: {spread(base):.1f} us.  `top_k 20` - `top_k 0`: {k20['median'] - base['median']:+.1f} us per token; "
               f"`top_k 20` - greedy: {k20['median'] - s['greedy']['median']:+.1f} us per token; `top_k 0` - greedy: {base['median'] - s['greedy']['median']:+.1f} us.", "",
               "One `q3_verify_draw` pass with every draft right, ms:", "", "| columns | top_k 0 | top_k 20 | difference | spread of top_k 0 |", "|---|---|---|---|---|"]
        for n, v in r["verify_draw_ms"].items():
            md.append(f"| {n} | {v['top_k 0']['median']:.3f} ({v['top_k 0']['min']:.3f} .. {v['top_k 0']['max']:.3f}) | {v['top_k 20']['median']:.3f} "
                      f"({v['top_k 20']['min']:.3f} .. {v['top_k 20']['max']:.3f}) | {v['top_k 20']['median'] - v['top_k 0']['median']:+.3f} | {spread(v['top_k 0']):.3f} |")
        m = r["many_sampled_ms"]
        md += ["", f"`q3_generate_many_sampled`, 64 requests (16-token prompts, 32 new tokens) on 32 slots, ms per call: top_k 0 {fmt(m['top_k 0'])}, "
               f"top_k 20 {fmt(m['top_k 20'])}: {m['top_k 20']['median'] - m['top_k 0']['median']:+.1f} ms, spread of top_k 0 {spread(m['top_k 0']):.1f} ms.", ""]
        if "parts" in r:
            md += ["Slices per column of the selection pass (developer build, `Q3_TOPK_PARTS`), top_k 20:", "",
                   "| slices | one column: us per sampled token | 32 columns: ms per pass |", "|---|---|---|"]
            for p, v in r["parts"].items():
                a, b = v["one column: us per sampled token"], v["32 columns: ms per pass"]
                md.append(f"| {p} | {fmt(a)} | {b['median']:.3f} ({b['min']:.3f} .. {b['max']:.3f}) |")
            md.append("")
    for name, rounds in ab.items():
        md += [f"## The untouched paths against the parent: {name}", "",
               "A child process per measurement, the parent's package and library and this tree's by turns; us per token, median (min .. max):", "",
               "| round | tree | greedy | sampled, top_k 0 |", "|---|---|---|---|"]
        for i, (tree, got) in enumerate(rounds):
            md.append(f"| {i // 2 + 1} | {tree} | {fmt(got['greedy'])} | {fmt(got['sampled'])} |")
        md.append("")
    with open(os.path.join(out, "top_k.md"), "w") as f:
        f.write("\n".join(md))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="qwen3-0.6b,qwen3-8b")
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ckpt-dir", default=os.environ.get("Q3_CKPT_DIR", "/tmp"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--limit", type=int, default=420, help="seconds per child process")
    ap.add_argument("--ab", default=None, metavar="PARENT_TREE", help="the greedy and the sampled step of that checkout's build against this tree's")
    ap.add_argument("--worker")
    ap.add_argument("--worker-ab")
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.ctx, a.ckpt_dir, a.seed, a.rounds)
        return 0
    if a.worker_ab:
        worker_ab(a.worker_ab, a.ctx, a.ckpt_dir, a.seed, a.rounds)
        return 0
    base = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--ctx", str(a.ctx), "--ckpt-dir", a.ckpt_dir,
            "--seed", str(a.seed), "--rounds", str(a.rounds)]
    results, ab = [], {}
    for name in a.models.split(","):
        got = run_child(base + ["--worker", name])
        if got is None:
            break
        results.append(got)
        if a.ab:
            rounds = []
            for _ in range(3):
                for label, tree in (("parent", os.path.abspath(a.ab)), ("this tree", ROOT)):
                    got = run_child(base + ["--worker-ab", name], dict(os.environ, Q3_BENCH_TREE=tree))
                    if got is None:
                        return 1
                    rounds.append((label, got))
            ab[name] = rounds
    if not results:
        return 1
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "top_k.json"), "w") as f:
        json.dump({"results": results, "ab": ab}, f, indent=1)
    write_md(results, ab, a.out)
    print(json.dumps({"models": [r["model"] for r in results], "out": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
