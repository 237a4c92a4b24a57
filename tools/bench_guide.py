#!/usr/bin/env python3
"""What guided decoding (include/qwen3_hip.h section 2r) costs inside generate_many, on the full-size synthetic checkpoints.

    python tools/bench_guide.py [--models qwen3-0.6b,qwen3-8b] [--ab PARENT_TREE [--ab-models qwen3-0.6b]] [--out profiles]

The workload, the configurations, the by-turns measurement and the child processes are tools/bench_bias.py's: 64 requests of
16-token prompts and 32 new tokens on 32 slots; greedy and sampled, each with top_k 0 and 20; all forms of a configuration in ONE
process by turns, medians of the rounds behind a warm-up round, min .. max beside them.  The forms: the generate call with no guide;
under a two-state guide that allows every token (the mechanism alone: the state read, the table row streamed, the state step);
under a trie of 64 four-token labels, a start state per request; the trie under penalties (1.5, 0.5); and, as the yardstick, a
12-token allow-list per request run by k_bias_apply with no guide.
The per-pass cost of the two kernels (k_guide_apply, k_guide_step) is (on - off) / passes; the byte model beside it is 10 V bytes
per emitting column (the row read, the masked row written, 2 V of table), 14 V under penalties (the counts read), 8 V for the
allow-list form, at 5.5 TB/s.
--ab PARENT_TREE: the call with no guide of this tree against the build of another checkout (bench_bias.py's children: the two
trees by turns, three times each): the path this feature must not have moved.
Writes <out>/guide.md and guide.json."""
import argparse
import json
import os
import sys

import bench_bias as bb
from bench_bias import CONFIGS, N_NEW, N_PROMPT, N_REQ, PEN, ROOT, SLOTS, STREAM_TBS, CTX, T, TOPP, TAG

FORMS = ["off", "all allowed", "trie 64 x 4", "trie 64 x 4 + penalties", "allow 12 (k_bias_apply)"]
BYTES = {"all allowed": 10.0, "trie 64 x 4": 10.0, "trie 64 x 4 + penalties": 14.0, "allow 12 (k_bias_apply)": 8.0}


def forms(q3, vocab):
    """form -> (guide (next, start) or None, table (lists, modes), penalties)"""
    import numpy as np
    free = np.zeros((2, vocab), dtype=np.int16)
    free[0] = 1
    labels = [[(104729 * r + 7919 * i + 13) % (vocab - 1) + 1 for i in range(4)] for r in range(N_REQ)]     # eos is token 0
    trie = q3.guide.Automaton.from_sequences(labels, vocab, eos=0)
    spread = lambda r, n, step: sorted({(7919 * r + step * i + 11) % vocab for i in range(n)})
    allow = [[(v, 0.0, 0) for v in spread(r, 12, vocab // 12 - 5)] for r in range(N_REQ)]
    none, off = (None, []), ([], [])
    return {"off": (none, off, (0.0, 0.0)), "all allowed": ((free, [0]), off, (0.0, 0.0)), "trie 64 x 4": ((trie.next, [0] * N_REQ), off, (0.0, 0.0)),
            "trie 64 x 4 + penalties": ((trie.next, [0] * N_REQ), off, PEN), "allow 12 (k_bias_apply)": (none, (allow, [1] * N_REQ), (0.0, 0.0))}


def worker(name, ckpt_dir, seed, rounds):
    import qwen3_rs_amd as q3
    path = bb.checkpoint(q3, name, ckpt_dir, seed)
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    prompts, n_new, seeds = bb.requests(vocab)
    res = {"model": name, "rounds": rounds, "vocab": vocab, "configs": {}}
    fm = forms(q3, vocab)
    with q3.TransformerBuilder(path).with_ctx_length(1024).build() as t:
        t.batch_init(SLOTS, CTX)
        for mode, top_k in CONFIGS:
            info = {}

            def form(guide, table, pen):
                def f():
                    t.set_top_k(top_k)
                    t.set_penalties(*pen)
                    t.set_logit_bias(*table)
                    t.set_guide(*guide)
                    bb.generate(t, mode, prompts, [1] * N_REQ, seeds)      # untimed: a new guide's table goes to the device here
                    out = []
                    s = bb.timed(lambda: out.append(bb.generate(t, mode, prompts, n_new, seeds)))
                    info["passes"], info["emitting"] = out[0][1].passes, sum(len(r) for r in out[0][0])
                    t.set_penalties(0.0, 0.0)
                    t.set_logit_bias([])
                    t.set_guide(None, [])
                    return s
                return f
            got = bb.by_turns({k: form(*fm[k]) for k in FORMS}, rounds)
            res["configs"][f"{mode}, top_k {top_k}"] = dict(info, ms={k: bb.stat(v) for k, v in got.items()})
    print(TAG + json.dumps(res), flush=True)


def write_md(results, ab, out):
    fmt = bb.fmt
    md = ["# Guided decoding inside generate_many (`tools/bench_guide.py`)", "",
          f"{N_REQ} requests of {N_PROMPT}-token prompts and {N_NEW} new tokens on {SLOTS} slots, synthetic checkpoints; sampled: temperature {T}, top-p {TOPP}.",
          "Every table was measured in one process, its forms by turns; a cell is the median over the rounds in ms per call with (min .. max)",
          "beside it.  off: no guide, the plans without the two kernels; all allowed: a two-state guide that allows every token; trie 64 x 4: a",
          f"trie of 64 four-token labels, a start state per request; + penalties: the same under penalties {PEN}; allow 12: no guide, a 12-token",
          "allow-list per request run by k_bias_apply -- the yardstick.  Every form is set in front of its call and a call of one new token runs before the",
          "timed one, so q3_guide_set's copy and the table's upload (once per set) are not in the figures.", ""]
    for r in results:
        md += [f"## {r['model']} ({r['rounds']} rounds)", "", "| configuration | passes | " + " | ".join(FORMS) + " |", "|---|---|" + "---|" * len(FORMS)]
        for cfg, c in r["configs"].items():
            md.append(f"| {cfg} | {c['passes']} | " + " | ".join(fmt(c["ms"][k]) for k in FORMS) + " |")
        md += ["", "Per-pass cost, us: (on - off) / passes, medians; the byte model: per emitting column of an average pass 10 V bytes (the row read,",
               f"the masked row written, 2 V of table), 14 V under penalties, 8 V for the allow-list form, at {STREAM_TBS} TB/s; measured / model beside every",
               "cost.  A guide form is held against the allow-list form of the same run plus the 2 V bytes it reads on top plus the spread of off.", "",
               "| configuration | " + " | ".join(FORMS[1:]) + " | spread of off per pass | emitting columns per pass | 2 V bytes per pass | trie within allow 12 + 2 V + spread |",
               "|---|" + "---|" * (len(FORMS) + 3)]
        for cfg, c in r["configs"].items():
            m, p = c["ms"], max(1, c["passes"])
            cols = c["emitting"] / p
            model = lambda nb: nb * r["vocab"] * cols / (STREAM_TBS * 1e12) * 1e6
            cost = {k: 1e3 * (m[k]["median"] - m["off"]["median"]) / p for k in FORMS[1:]}
            spread = 1e3 * (m["off"]["max"] - m["off"]["min"]) / p
            bound = cost["allow 12 (k_bias_apply)"] + model(2.0) + spread
            md.append(f"| {cfg} | " + " | ".join(f"{cost[k]:+.1f} ({cost[k] / model(BYTES[k]):.1f} x)" for k in FORMS[1:]) +
                      f" | {spread:.1f} | {cols:.1f} | {model(2.0):.1f} | {'yes' if cost['trie 64 x 4'] <= bound else 'NO'} ({cost['trie 64 x 4']:+.1f} vs {bound:+.1f}) |")
        md.append("")
    cond = []
    for name, rounds in ab.items():
        md += [f"## The call with no guide against the parent: {name}", "",
               "A child process per measurement, the parent's package and library and this tree's by turns, three each; ms per call, median (min .. max)",
               "over all rounds of a tree's children.", "", "| configuration | parent | this tree | this tree's median inside the parent's min .. max |", "|---|---|---|---|"]
        for cfg in rounds[0][1]:
            p, h = bb.pooled(rounds, "parent", cfg), bb.pooled(rounds, "this tree", cfg)
            ok = p["min"] <= h["median"] <= p["max"]
            cond.append((name, cfg, ok, h["median"] < p["min"]))
            md.append(f"| {cfg} | {fmt(p)} | {fmt(h)} | {'yes' if ok else ('NO: below' if h['median'] < p['min'] else 'NO: above')} |")
        md.append("")
    md += ["## The off path", ""]
    if cond:
        bad = [f"{n}: {c} ({'below' if below else 'above'})" for n, c, ok, below in cond if not ok]
        md.append("The call with no guide on this tree lies inside the min .. max of the parent's own rounds, per configuration: " +
                  ("met." if not bad else "NOT met for " + "; ".join(bad) + "."))
    else:
        md.append("Not measured: no parent tree was given (`--ab`).")
    md.append("")
    with open(os.path.join(out, "guide.md"), "w") as f:
        f.write("\n".join(md))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="qwen3-0.6b,qwen3-8b")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ckpt-dir", default=os.environ.get("Q3_CKPT_DIR", "/tmp"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--limit", type=int, default=420, help="seconds per child process")
    ap.add_argument("--ab", default=None, metavar="PARENT_TREE", help="the call with no guide of that checkout's build against this tree's")
    ap.add_argument("--ab-models", default=None, help="the models --ab measures (default: all of --models)")
    ap.add_argument("--worker")
    ap.add_argument("--worker-ab")
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.ckpt_dir, a.seed, a.rounds)
        return 0
    if a.worker_ab:
        bb.worker_ab(a.worker_ab, a.ckpt_dir, a.seed, a.rounds)      # the call with no table is the call with no guide
        return 0
    base = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--ckpt-dir", a.ckpt_dir, "--seed", str(a.seed),
            "--rounds", str(a.rounds)]
    results, ab, rc = [], {}, 0

    def save():                 # what is measured so far stands on disk before the next child starts
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "guide.json"), "w") as f:
            json.dump({"results": results, "ab": ab}, f, indent=1)
        write_md(results, ab, a.out)
    for name in a.models.split(","):
        got = bb.run_child(base + ["--worker", name])
        if got is None:
            rc = 1
            break
        results.append(got)
        save()
        if a.ab and (a.ab_models is None or name in a.ab_models.split(",")):
            rounds = []
            for _ in range(3):
                for label, tree in (("parent", os.path.abspath(a.ab)), ("this tree", ROOT)):
                    got = bb.run_child(base + ["--worker-ab", name], dict(os.environ, Q3_BENCH_TREE=tree))
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
