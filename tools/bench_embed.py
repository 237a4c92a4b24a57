#!/usr/bin/env python3
"""What embeddings through dense blocks (include/qwen3_hip.h section 2j) cost on the full-size synthetic checkpoints.

    python tools/bench_embed.py [--models qwen3-0.6b,qwen3-8b] [--ctx 1024] [--out profiles] [--limit 420] [--reps 5]

Every model is measured in a child process of its own under a time limit (one faulting run never starts the next).  Per model,
32 slots, and for 64 prompts of 64 tokens and 64 prompts of 512 tokens (two waves of 32 prompts each):
  (a) q3_embed_many: L2-normalised rows of the full dimension, one call;
  (b) the same prompts through q3_batch_prefill_slots, one call per wave: the cache rows alone, by code this feature does not
      touch -- the cost of the blocks;
  (c) the per-prompt way that needs no q3_embed_many: q3_prefill_batched of all but the last token, q3_forward of the last (which
      streams the classifier), q3_read_state("x"), prompt after prompt on the single-stream cache.
The three are repeated in turn, (a) (b) (c) (a) (b) (c) ..., behind one warm-up round, in one process; the table holds the median wall
time of a call.  The rows of (a), without the L2 part, must equal the rows of (c) bit for bit.
  (d) 4 prompts of 6 tokens -- one block of 32 columns or fewer, which runs the layers of the 32-column plan and no classifier --
      against one q3_batch_step_cols pass of 32 columns (4 slots x 8 positions, no logits read back), alternating, median of 15.
Writes <out>/embed.json and <out>/embed.md.
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
    print(f"[bench_embed] {name}: checkpoint ready", file=sys.stderr, flush=True)
    with q3.TransformerBuilder(path).with_ctx_length(ctx).build() as t:
        t.batch_init(SLOTS, ctx)
        for n_req, plen in ((64, 64), (64, 512)):
            print(f"[bench_embed] {name}: {n_req} prompts of {plen} tokens", file=sys.stderr, flush=True)
            prompts = [ck.iter_prompt_tokens(shape, seed + 50 + r, plen) for r in range(n_req)]
            waves = [prompts[i:i + SLOTS] for i in range(0, n_req, SLOTS)]

            def embed():
                return t.embed_many(prompts)

            def slots():
                st = [t.batch_prefill_slots(list(range(len(w))), w, [0] * len(w)) for w in waves]
                return sum(s.blocks for s in st)

            def single():
                rows = []
                for p in prompts:
                    t.prefill(p[:-1], 0, batched=True)
                    t.forward(p[-1], plen - 1)
                    rows.append(t.read_state("x"))
                return np.stack(rows)
            raw, st = t.embed_many(prompts, normalize=False)
            blocks = slots()
            ref = single()                                             # (the three calls above are the warm-up round)
            embed()
            dts = {"embed_many": [], "prefill_slots": [], "per_prompt": []}
            for _ in range(reps):                                      # alternating
                for k, call in (("embed_many", embed), ("prefill_slots", slots), ("per_prompt", single)):
                    t0 = time.perf_counter()
                    call()
                    dts[k].append(time.perf_counter() - t0)
            med = {k: median(v) for k, v in dts.items()}
            res["cases"][f"{n_req} x {plen}"] = {
                "requests": n_req, "prompt_len": plen, "waves": st.waves, "blocks": st.blocks, "blocks_prefill_slots": blocks,
                "rows_equal": bool(np.array_equal(raw.view(np.int32), ref.view(np.int32))),
                "seconds": med, "all_seconds": dts,
                "prompts_per_s": {k: n_req / v for k, v in med.items()}, "tokens_per_s": {k: n_req * plen / v for k, v in med.items()},
                "embed_minus_slots_us_per_block": 1e6 * (med["embed_many"] - med["prefill_slots"]) / st.blocks,
            }
        # ---- (d) one narrow block against one column pass of 32 columns
        small = [ck.iter_prompt_tokens(shape, seed + 150 + r, 6) for r in range(4)]
        cols = [ck.iter_prompt_tokens(shape, seed + 160 + r, 8) for r in range(4)]
        c_slots = [r for r in range(4) for _ in range(8)]
        c_toks = [tok for p in cols for tok in p]
        c_pos = [k for _ in range(4) for k in range(8)]
        _, st = t.embed_many(small)
        t.batch_step_cols(c_slots, c_toks, c_pos)
        em, sc = [], []
        for _ in range(15):                                            # alternating
            t0 = time.perf_counter()
            t.embed_many(small)
            em.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            t.batch_step_cols(c_slots, c_toks, c_pos)
            sc.append(time.perf_counter() - t0)
        res["narrow_ms"] = {"embed_4x6": 1e3 * median(em), "step_cols_32": 1e3 * median(sc), "blocks": st.blocks,
                            "columns": st.live_columns + st.pad_columns}
    print("RESULT " + json.dumps(res))


def write_md(results, a):
    lines = ["# Embeddings through dense blocks: `q3_embed_many`", "",
             "Written by `tools/bench_embed.py` (synthetic full-size checkpoints, one MI355X, %d slots, context %d per slot).  Wall time" % (SLOTS, a.ctx),
             "per call, median of %d repetitions that alternate the three paths in one process behind a warm-up round.  embed_many =" % a.reps,
             "`q3_embed_many`, L2-normalised rows of the full dimension, one call; prefill_slots = the same prompts through",
             "`q3_batch_prefill_slots`, one call per wave of 32: the blocks alone, by code this feature does not touch; per prompt =",
             "`q3_prefill_batched` + `q3_forward` + `q3_read_state(\"x\")` for every prompt in turn, the way that needs no `q3_embed_many`",
             "(it streams the classifier once per prompt).  Numbers of one box; the pool's boxes differ by 3-6 % (README).", "",
             "| model | prompts | path | blocks | seconds | prompts/s | tokens/s | rows equal |", "|---|---|---|---|---|---|---|---|"]
    for r in results:
        for label, c in r["cases"].items():
            for k, what in (("embed_many", "embed_many"), ("prefill_slots", "prefill_slots"), ("per_prompt", "per prompt")):
                lines.append(f"| {r['model']} | {label} | {what} | {c['blocks'] if k != 'per_prompt' else ''} | {c['seconds'][k]:.4f} | "
                             f"{c['prompts_per_s'][k]:.0f} | {c['tokens_per_s'][k]:.0f} | {c['rows_equal'] if k == 'embed_many' else ''} |")
    lines += ["", "embed_many minus prefill_slots, per block: what the call adds to its blocks -- one `k_embed_rows` launch per block and the copy of",
              "the rows back -- less the second synchronisation that prefill_slots pays for its second wave.  spread = the smallest and the",
              "largest repetition of either path, against which the difference is to be read:", "",
              "| model | prompts | blocks | us per block | embed_many ms, spread | prefill_slots ms, spread |", "|---|---|---|---|---|---|"]
    for r in results:
        for label, c in r["cases"].items():
            sp = {k: f"{1e3 * min(v):.2f} - {1e3 * max(v):.2f}" for k, v in c["all_seconds"].items()}
            lines.append(f"| {r['model']} | {label} | {c['blocks']} | {c['embed_minus_slots_us_per_block']:.1f} | {sp['embed_many']} | {sp['prefill_slots']} |")
    lines += ["", "One narrow block -- 4 prompts of 6 tokens, which run the layer launches of the 32-column plan and no classifier -- against one",
              "`q3_batch_step_cols` pass of 32 columns (4 slots x 8 positions, no logits read back); median of 15 alternating calls:", "",
              "| model | embed_many 4 x 6 ms | step_cols 32 columns ms | ratio |", "|---|---|---|---|"]
    for r in results:
        d = r["narrow_ms"]
        lines.append(f"| {r['model']} | {d['embed_4x6']:.3f} | {d['step_cols_32']:.3f} | {d['embed_4x6'] / d['step_cols_32']:.3f} |")
    if not results:
        lines.append("not taken")
    # the two signs the feature was expected to show
    narrow_ok = all(r["narrow_ms"]["embed_4x6"] < r["narrow_ms"]["step_cols_32"] for r in results)
    diffs = [(c["embed_minus_slots_us_per_block"], r["model"], label) for r in results for label, c in r["cases"].items()]
    worst = max(diffs, default=(0.0, "", ""))
    lines += ["", "## The two expected signs", "",
              f"1. The narrow embed costs less than the column pass: {'holds' if narrow_ok else 'DOES NOT HOLD'} on every model measured.  Both run the layer launches of the same",
              "   32-column plan.  The column pass adds the final norm, the classifier (`lm_head`, read once for the 32 columns), `k_cols_turn` and",
              "   the copies of its control block; the embed adds `k_dense_states`, one `k_embed_rows` launch and the copy of 4 rows.  The embed",
              "   enqueues its layer launches one by one where the column pass replays a captured graph; how much of the gain that takes back",
              "   was not measured.",
              "2. `embed_many` costs no more than `batch_prefill_slots` plus the gathers and the one output copy: the blocks are the launches",
              f"   `batch_prefill_slots` enqueues, and the largest difference measured is {worst[0]:.0f} us per block ({worst[1]}, {worst[2]}).  Per call that",
              "   difference is one `k_embed_rows` launch per block and the copy of 64 rows of the full dimension into pageable memory, less one",
              "   synchronisation; read it against the spread column above."]
    with open(os.path.join(a.out, "embed.md"), "w") as f:
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
    ap.add_argument("--render", metavar="JSON", help="write <out>/embed.md again from an embed.json taken earlier; measures nothing")
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
        print(f"[bench_embed] {name} ...", file=sys.stderr, flush=True)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)       # the worker's progress lines go straight to stderr
        if p.returncode != 0:
            print(f"[bench_embed] {name}: exit status {p.returncode}; stopping here", file=sys.stderr)
            break
        results.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "embed.json"), "w") as f:
        json.dump(results, f, indent=1)
    write_md(results, a)
    ok = len(results) == len(a.models.split(",")) and all(c["rows_equal"] for r in results for c in r["cases"].values())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
