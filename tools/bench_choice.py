#!/usr/bin/env python3
"""What choice logits through dense blocks (include/qwen3_hip.h section 2k) cost on the full-size synthetic checkpoints.

    python tools/bench_choice.py [--models qwen3-0.6b,qwen3-8b] [--ctx 1024] [--out profiles] [--limit 420] [--reps 5]

Every model is measured in a child process of its own under a time limit (one faulting run never starts the next).  Per model,
32 slots, and for 64 prompts of 64 tokens and 64 prompts of 512 tokens (two waves of 32 prompts each):
  (a) q3_choice_many with k = 2 candidates, one call; and the same call with k = 32 and k = 256;
  (b) q3_embed_many with flags 0 on the same prompts: the same set of blocks with another tail (k_embed_rows, rows of the full
      dimension copied back) -- the floor;
  (c) the per-prompt way that needs no q3_choice_many: q3_prefill_batched of all but the last token, q3_forward of the last (which
      streams the classifier and copies vocab floats back), two logits taken, prompt after prompt on the single-stream cache.
The paths are repeated in turn behind one warm-up round, in one process: the four batched calls, then (c); the table holds the median
wall time of a call.  The batched call that follows (c) costs about a millisecond more than the same call elsewhere in the round,
whichever path it is (profiles/choice.md, "What was tried"), so the four batched calls start one place further on in every
repetition: each stands behind (c) in at most two of five repetitions, and the median leaves those out for all four alike.
The rows of (a) must equal the logits of (c) at the candidate ids bit for bit.
Writes <out>/choice.json and <out>/choice.md.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-rs_amd"))

SLOTS = 32
KS = (2, 32, 256)
# the classifier launch a prompt's q3_forward pays, microseconds: what the tail of a block stands in for
CLASSIFIER_US = {"qwen3-0.6b": 29.9, "qwen3-8b": 110.0}


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def worker(name, ctx, ckpt_dir, seed, reps):
    import numpy as np
    import qwen3_rs_amd as q3
    ck = q3.checkpoint
    shape = ck.SHAPES[name]
    path = os.path.join(ckpt_dir, f"{name}-seed{seed}.q3bin")
    ck.ensure_synthetic_checkpoint(path, shape, seed=seed)
    res = {"model": name, "ctx": ctx, "slots": SLOTS, "reps": reps, "cases": {}}
    print(f"[bench_choice] {name}: checkpoint ready", file=sys.stderr, flush=True)
    rng = np.random.default_rng(seed)
    cands = {k: [int(c) for c in rng.integers(0, shape.vocab_size, k)] for k in KS}
    with q3.TransformerBuilder(path).with_ctx_length(ctx).build() as t:
        t.batch_init(SLOTS, ctx)
        for n_req, plen in ((64, 64), (64, 512)):
            print(f"[bench_choice] {name}: {n_req} prompts of {plen} tokens", file=sys.stderr, flush=True)
            prompts = [ck.iter_prompt_tokens(shape, seed + 50 + r, plen) for r in range(n_req)]

            def choice(k):
                return lambda: t.choice_many(prompts, cands[k])

            def embed():
                return t.embed_many(prompts, normalize=False)

            def single():
                rows = []
                for p in prompts:
                    t.prefill(p[:-1], 0, batched=True)
                    rows.append(t.forward(p[-1], plen - 1)[cands[2]].copy())
                return np.stack(rows)
            paths = (("choice_k2", choice(2)), ("embed_many", embed), ("choice_k32", choice(32)), ("choice_k256", choice(256)), ("per_prompt", single))
            got, st = t.choice_many(prompts, cands[2])
            ref = single()
            for _, call in paths[:4]:                                   # (with the two calls above: the warm-up round)
                call()
            dts = {k: [] for k, _ in paths}
            for i in range(reps):                                       # alternating; the batched calls rotate, per_prompt stays last
                for k, call in paths[i % 4:4] + paths[:i % 4] + paths[4:]:
                    t0 = time.perf_counter()
                    call()
                    dts[k].append(time.perf_counter() - t0)
            med = {k: median(v) for k, v in dts.items()}
            res["cases"][f"{n_req} x {plen}"] = {
                "requests": n_req, "prompt_len": plen, "waves": st.waves, "blocks": st.blocks,
                "rows_equal": bool(np.array_equal(got.view(np.int32), ref.view(np.int32))),
                "seconds": med, "all_seconds": dts,
                "prompts_per_s": {k: n_req / v for k, v in med.items()},
                "tail_us_per_block": {k: 1e6 * (med[k] - med["embed_many"]) / st.blocks for k in ("choice_k2", "choice_k32", "choice_k256")},
            }
    print("RESULT " + json.dumps(res))


def write_md(results, a):
    lines = ["# Choice logits through dense blocks: `q3_choice_many`", "",
             "Written by `tools/bench_choice.py` (synthetic full-size checkpoints, one MI355X, %d slots, context %d per slot).  Wall time" % (SLOTS, a.ctx),
             "per call, median of %d repetitions that alternate the paths in one process behind a warm-up round.  choice k = `q3_choice_many`" % a.reps,
             "with one shared list of k candidates, one call; embed_many = `q3_embed_many` with flags 0 on the same prompts, the same blocks",
             "with another tail and rows of the full dimension copied back: the floor; per prompt = `q3_prefill_batched` + `q3_forward`, two",
             "logits taken, for every prompt in turn (it streams the classifier and copies `vocab` floats once per prompt).  Numbers of one",
             "box; the pool's boxes differ by 3-6 % (README).", "",
             "| model | prompts | path | blocks | seconds | prompts/s | rows equal |", "|---|---|---|---|---|---|---|"]
    names = (("choice_k2", "choice k = 2"), ("embed_many", "embed_many"), ("choice_k32", "choice k = 32"), ("choice_k256", "choice k = 256"),
             ("per_prompt", "per prompt"))
    for r in results:
        for label, c in r["cases"].items():
            for k, what in names:
                lines.append(f"| {r['model']} | {label} | {what} | {c['blocks'] if k != 'per_prompt' else ''} | {c['seconds'][k]:.4f} | "
                             f"{c['prompts_per_s'][k]:.0f} | {c['rows_equal'] if k == 'choice_k2' else ''} |")
    lines += ["", "The tail's cost per block, (choice - embed_many) / blocks: one `k_choice_rows` launch in the place of one `k_embed_rows` launch,",
              "the upload of the ids, and k floats per prompt copied back in the place of dim.  spread = the smallest and the largest",
              "repetition of a path, against which the differences are to be read:", "",
              "| model | prompts | blocks | k = 2 us | k = 32 us | k = 256 us | choice k = 2 ms, spread | embed_many ms, spread |", "|---|---|---|---|---|---|---|---|"]
    for r in results:
        for label, c in r["cases"].items():
            sp = {k: f"{1e3 * min(v):.2f} - {1e3 * max(v):.2f}" for k, v in c["all_seconds"].items()}
            tl = c["tail_us_per_block"]
            lines.append(f"| {r['model']} | {label} | {c['blocks']} | {tl['choice_k2']:.1f} | {tl['choice_k32']:.1f} | {tl['choice_k256']:.1f} | "
                         f"{sp['choice_k2']} | {sp['embed_many']} |")
    if not results:
        lines.append("not taken")
    lines += ["", "## The two bars", ""]
    for r in results:
        bar = CLASSIFIER_US.get(r["model"])
        for label, c in r["cases"].items():
            tl = c["tail_us_per_block"]
            worst = max(tl["choice_k2"], tl["choice_k32"])
            if bar is not None:
                lines.append(f"1. {r['model']}, {label}: for k <= 32 the tail costs {worst:.1f} us per block at most against the {bar:.1f} us classifier launch "
                             f"it replaces: {'met' if worst < bar else 'MISSED'}.")
            hi = max(c["all_seconds"]["embed_many"])
            lines.append(f"2. {r['model']}, {label}: choice k = 2, median {1e3 * c['seconds']['choice_k2']:.2f} ms, against the slowest repetition of embed_many, "
                         f"{1e3 * hi:.2f} ms: {'met' if c['seconds']['choice_k2'] <= hi else 'MISSED'}.")
    lines += ["", "## What was tried", "",
              "The order of the round.  A first run repeated the paths in one fixed order, choice k = 2 always the call behind the per-prompt",
              "path.  It read k = 2 at 0.7, 1.4, 1.3 and 0.7 ms per call above embed_many (0.6B 64 x 64 and 64 x 512, 8B likewise) while k = 32",
              "and k = 256, the same kernel with more work, read within 0.2 ms of embed_many on either side: a cost of the place in the",
              "round, not of the path, and not one that grows with the blocks (2 and 16).  What the first batched call behind 64 single-stream",
              "prefills pays was not looked into.  The tool now moves the start of the batched calls on by one in every repetition; the",
              "tables above are from that form.",
              "",
              "`kChoicePart` (csrc/q3_choice.h), the candidates per workgroup, is 32, the figure the kernel began with; no other value was",
              "measured.  At 32 a workgroup's four waves hold two batches of four rows each, every part repeats the norm and the quantizer",
              "(the exact sum of squares is most of a part's time at k <= 32), and k = 256 runs 8 parts per prompt.  The rows of a wave's first",
              "batch are requested in front of the prologue; a form that requests them behind it was not measured either.  The kernel's build",
              "listing: 226 VGPRs, no scratch, 16 bytes of static LDS (the quantizer's wave maxima)."]
    with open(os.path.join(a.out, "choice.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="qwen3-0.6b,qwen3-8b")
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--limit", type=int, default=420, help="seconds per model")
    ap.add_argument("--seed", type=int, default=1236)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ckpt-dir", default=os.environ.get("Q3_CKPT_DIR", "/tmp"))
    ap.add_argument("--worker")
    ap.add_argument("--render", metavar="JSON", help="write <out>/choice.md again from a choice.json taken earlier; measures nothing")
    a = ap.parse_args()
    if a.render:
        write_md(json.load(open(a.render)), a)
        return 0
    if a.worker:
        worker(a.worker, a.ctx, a.ckpt_dir, a.seed, a.reps)
        return 0
    results = []
    for name in a.models.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", name, "--ctx", str(a.ctx),
               "--ckpt-dir", a.ckpt_dir, "--seed", str(a.seed), "--reps", str(a.reps)]
        print(f"[bench_choice] {name} ...", file=sys.stderr, flush=True)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)       # the worker's progress lines go straight to stderr
        if p.returncode != 0:
            print(f"[bench_choice] {name}: exit status {p.returncode}; stopping here", file=sys.stderr)
            break
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "choice.json"), "w") as f:
        json.dump(results, f, indent=1)
    write_md(results, a)
    ok = len(results) == len(a.models.split(",")) and all(c["rows_equal"] for r in results for c in r["cases"].values())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
