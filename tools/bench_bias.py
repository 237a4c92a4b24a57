#!/usr/bin/env python3
"""What logit bias, banned and allowed tokens (include/qwen3_hip.h section 2q) cost inside generate_many, on the full-size synthetic
checkpoints.

    python tools/bench_bias.py [--models qwen3-0.6b,qwen3-8b] [--ab PARENT_TREE] [--out profiles]

Workload (tools/bench_pen.py's): 64 requests of 16-token prompts and 32 new tokens on 32 slots; greedy and sampled (temperature
0.6, top-p 0.95), each with top_k 0 and 20: four configurations.  Every model is measured in a child process of its own under a time
limit (one faulting run never starts the next).  All forms of a configuration are measured in ONE process, by turns: round r runs
every form once, the table holds the median over the rounds and the spread (min .. max) beside it; the first round of every form is a
warm-up and is not counted.  Times are host clocks around calls that end in a device synchronisation.  The forms: the generate call
with no table; with one banned token for all requests; with a 300-entry bias list per request; with a 12-token allow-list per
request; and the last of these under penalties (1.5, 0.5).
The per-pass cost of the two kernels (k_bias_apply, k_bias_count; a sampled plan also folds the slices' keys where it folded the
classifier's) is (on - off) / passes, passes as the call's q3_cols_stats count them; the byte model beside it is 8 V bytes per
emitting column (the row read, the adjusted row written), 12 V under penalties (the counts read), at 5.5 TB/s.
--ab PARENT_TREE: the call with no table of this tree against the build of another checkout (which need not know the setting), a
child process per measurement, the two trees by turns, three times each: the path this feature must not have moved.
Writes <out>/logit_bias.md and logit_bias.json."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("Q3_BENCH_TREE", ROOT)         # (--ab: a child measures the package and the library of another checkout)
sys.path.insert(0, os.path.join(TREE, "qwen3-rs_amd"))

T, TOPP = 0.6, 0.95
N_REQ, N_PROMPT, N_NEW, SLOTS, CTX = 64, 16, 32, 32, 256
CONFIGS = [("greedy", 0), ("greedy", 20), ("sampled", 0), ("sampled", 20)]
FORMS = ["off", "one ban", "300 per request", "allow 12", "allow 12 + penalties"]
PEN = (1.5, 0.5)
STREAM_TBS = 5.5                                     # what k_kv_rows_bcast streams at (profiles/serve_cols.md)
TAG = "BENCH_BIAS "


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def stat(xs, scale=1e3):
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


def requests(vocab):
    return [[(31 * r + 7 * i + 3) % vocab for i in range(N_PROMPT)] for r in range(N_REQ)], [N_NEW] * N_REQ, [1000 + r for r in range(N_REQ)]


def tables(vocab):
    """form -> (lists, modes, penalties); the tokens spread over the vocabulary, so most slices of a 300-entry list hold a few entries"""
    spread = lambda r, n, step: sorted({(7919 * r + step * i + 11) % vocab for i in range(n)})
    bias = [[(v, ((v % 9) - 4) * 0.75, 0) for v in spread(r, 300, vocab // 300 - 1)] for r in range(N_REQ)]
    allow = [[(v, 0.0, 0) for v in spread(r, 12, vocab // 12 - 5)] for r in range(N_REQ)]
    assert all(len(l) == 300 for l in bias) and all(len(l) == 12 for l in allow)
    return {"off": ([], [], (0.0, 0.0)), "one ban": ([[(vocab // 2, float("-inf"), 0)]], [0], (0.0, 0.0)),
            "300 per request": (bias, [0] * N_REQ, (0.0, 0.0)), "allow 12": (allow, [1] * N_REQ, (0.0, 0.0)),
            "allow 12 + penalties": (allow, [1] * N_REQ, PEN)}


def generate(t, mode, prompts, n_new, seeds):
    if mode == "greedy":
        return t.generate_many_greedy(prompts, n_new)
    return t.generate_many_sampled(prompts, n_new, T, TOPP, seeds)


def worker(name, ckpt_dir, seed, rounds):
    import qwen3_rs_amd as q3
    path = checkpoint(q3, name, ckpt_dir, seed)
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    prompts, n_new, seeds = requests(vocab)
    res = {"model": name, "rounds": rounds, "vocab": vocab, "configs": {}}
    with q3.TransformerBuilder(path).with_ctx_length(1024).build() as t:
        t.batch_init(SLOTS, CTX)
        for mode, top_k in CONFIGS:
            info = {}

            def form(lists, modes, pen):
                def f():
                    t.set_top_k(top_k)
                    t.set_penalties(*pen)
                    t.set_logit_bias(lists, modes)
                    out = []
                    s = timed(lambda: out.append(generate(t, mode, prompts, n_new, seeds)))
                    info["passes"], info["emitting"] = out[0][1].passes, sum(len(r) for r in out[0][0])
                    t.set_penalties(0.0, 0.0)
                    t.set_logit_bias([])
                    return s
                return f
            tb = tables(vocab)
            got = by_turns({k: form(*tb[k]) for k in FORMS}, rounds)
            res["configs"][f"{mode}, top_k {top_k}"] = dict(info, ms={k: stat(v) for k, v in got.items()})
    print(TAG + json.dumps(res), flush=True)


def worker_ab(name, ckpt_dir, seed, rounds):
    """this process imported the package of Q3_BENCH_TREE: the call with no table alone, through nothing the parent lacks"""
    import qwen3_rs_amd as q3
    path = checkpoint(q3, name, ckpt_dir, seed)
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    prompts, n_new, seeds = requests(vocab)
    with q3.TransformerBuilder(path).with_ctx_length(1024).build() as t:
        t.batch_init(SLOTS, CTX)

        def form(mode, top_k):
            def f():
                t.set_top_k(top_k)
                return timed(lambda: generate(t, mode, prompts, n_new, seeds))
            return f
        got = by_turns({f"{m}, top_k {k}": form(m, k) for m, k in CONFIGS}, rounds)
    print(TAG + json.dumps({k: [1e3 * x for x in v] for k, v in got.items()}), flush=True)


def run_child(cmd, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith(TAG)]
    if r.returncode != 0 or not line:
        print(f"exit status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}", file=sys.stderr)
        return None
    return json.loads(line[0][len(TAG):])


def fmt(s):
    return f"{s['median']:.1f} ({s['min']:.1f} .. {s['max']:.1f})"


def pooled(rounds, label, cfg):
    xs = [x for tree, got in rounds if tree == label for x in got[cfg]]
    return {"median": median(xs), "min": min(xs), "max": max(xs)}


def write_md(results, ab, out):
    md = ["# Logit bias, banned and allowed tokens inside generate_many (`tools/bench_bias.py`)", "",
          f"{N_REQ} requests of {N_PROMPT}-token prompts and {N_NEW} new tokens on {SLOTS} slots, synthetic checkpoints; sampled: temperature {T}, top-p {TOPP}.",
          "Every table was measured in one process, its forms by turns; a cell is the median over the rounds in ms per call with (min .. max)",
          "beside it.  off: no table, the plans without the two kernels; one ban: one banned token for all requests; 300 per request: a",
          f"300-entry bias list per request; allow 12: a 12-token allow-list per request; + penalties: the same under penalties {PEN}.", ""]
    for r in results:
        md += [f"## {r['model']} ({r['rounds']} rounds)", "", "| configuration | passes | " + " | ".join(FORMS) + " |", "|---|---|" + "---|" * len(FORMS)]
        for cfg, c in r["configs"].items():
            md.append(f"| {cfg} | {c['passes']} | " + " | ".join(fmt(c["ms"][k]) for k in FORMS) + " |")
        md += ["", "Per-pass cost of a table, us: (on - off) / passes, medians; the byte model: 8 V bytes (the row read, the adjusted row written) per",
               f"emitting column of an average pass at {STREAM_TBS} TB/s, 12 V under penalties (the counts read); measured / model beside every cost.", "",
               "| configuration | " + " | ".join(FORMS[1:]) + " | spread of off per pass | emitting columns per pass | byte model 8 V / 12 V |",
               "|---|" + "---|" * (len(FORMS) + 2)]
        for cfg, c in r["configs"].items():
            m, p = c["ms"], max(1, c["passes"])
            cols = c["emitting"] / p
            model = lambda k: (12.0 if "penalties" in k else 8.0) * r["vocab"] * cols / (STREAM_TBS * 1e12) * 1e6
            cost = {k: 1e3 * (m[k]["median"] - m["off"]["median"]) / p for k in FORMS[1:]}
            md.append(f"| {cfg} | " + " | ".join(f"{cost[k]:+.1f} ({cost[k] / model(k):.1f} x)" for k in FORMS[1:]) +
                      f" | {1e3 * (m['off']['max'] - m['off']['min']) / p:.1f} | {cols:.1f} | {model('off'):.1f} / {model('penalties'):.1f} |")
        md.append("")
    cond = []
    for name, rounds in ab.items():
        md += [f"## The call with no table against the parent: {name}", "",
               "A child process per measurement, the parent's package and library and this tree's by turns, three each; ms per call, median (min .. max)",
               "over all rounds of a tree's children.", "", "| configuration | parent | this tree | this tree's median inside the parent's min .. max |", "|---|---|---|---|"]
        for cfg in rounds[0][1]:
            p, h = pooled(rounds, "parent", cfg), pooled(rounds, "this tree", cfg)
            ok = p["min"] <= h["median"] <= p["max"]
            cond.append((name, cfg, ok, h["median"] < p["min"]))
            md.append(f"| {cfg} | {fmt(p)} | {fmt(h)} | {'yes' if ok else ('NO: below' if h['median'] < p['min'] else 'NO: above')} |")
        md.append("")
    md += ["## The off path", ""]
    if cond:
        bad = [f"{n}: {c} ({'below' if below else 'above'})" for n, c, ok, below in cond if not ok]
        md.append("The call with no table on this tree lies inside the min .. max of the parent's own rounds, per configuration: " +
                  ("met." if not bad else "NOT met for " + "; ".join(bad) + "."))
    else:
        md.append("Not measured: no parent tree was given (`--ab`).")
    md.append("")
    with open(os.path.join(out, "logit_bias.md"), "w") as f:
        f.write("\n".join(md))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="qwen3-0.6b,qwen3-8b")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ckpt-dir", default=os.environ.get("Q3_CKPT_DIR", "/tmp"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--limit", type=int, default=420, help="seconds per child process")
    ap.add_argument("--ab", default=None, metavar="PARENT_TREE", help="the call with no table of that checkout's build against this tree's")
    ap.add_argument("--worker")
    ap.add_argument("--worker-ab")
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.ckpt_dir, a.seed, a.rounds)
        return 0
    if a.worker_ab:
        worker_ab(a.worker_ab, a.ckpt_dir, a.seed, a.rounds)
        return 0
    base = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--ckpt-dir", a.ckpt_dir, "--seed", str(a.seed),
            "--rounds", str(a.rounds)]
    results, ab, rc = [], {}, 0

    def save():                 # what is measured so far stands on disk before the next child starts
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "logit_bias.json"), "w") as f:
            json.dump({"results": results, "ab": ab}, f, indent=1)
        write_md(results, ab, a.out)
    for name in a.models.split(","):
        got = run_child(base + ["--worker", name])
        if got is None:
            rc = 1
            break
        results.append(got)
        save()
        if a.ab:
            rounds = []
            for _ in range(3):
                for label, tree in (("parent", os.path.abspath(a.ab)), ("this tree", ROOT)):
                    got = run_child(base + ["--worker-ab", name], dict(os.environ, Q3_BENCH_TREE=tree))
                    if got is None:
                        rc = 1
                        break
                    rounds.append((label, got))
                if rc:
                    break
            if rc:
                break
            ab[name] = rounds
        save()
    if not results:
        return 1
    print(json.dumps({"models": [r["model"] for r in results], "out": a.out}))
    return rc


if __name__ == "__main__":
    sys.exit(main())
