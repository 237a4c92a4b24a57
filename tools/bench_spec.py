#!/usr/bin/env python3
"""Cost of draft verification and prompt-lookup decode (include/qwen3_hip.h section 2c) on the full-size synthetic checkpoints.

    python tools/bench_spec.py [--models qwen3-0.6b,qwen3-4b,qwen3-8b] [--ctx 4096] [--out profiles]

Every model is measured in a child process of its own under a time limit (one faulting run never starts the next).  Per model:
  * q3_generate_greedy tok/s (the untouched single-stream path: the yardstick);
  * the time of one q3_verify pass for n in {2, 4, 8, 16, 32} at position ~64 (4B also ~2,300), through the captured graph
    and with eager launches (Q3_FLAG_NO_GRAPH), and from it the BREAK-EVEN accepted drafts per pass = pass time / greedy
    step time - 1;
  * tok/s with every draft right (q3_verify fed the greedy tokens in blocks of 32), of q3_generate_lookup with ngram 64 (never a
    draft: the price of one host read-back per token against the device-resident loop) and of self-lookup at ngram 2 / 3 with
    the simulated acceptance beside it;
  * under the sampler (section 2d; temperature 1.0, top-p 0.9, the reference's defaults): q3_generate_sampled tok/s (untouched by
    section 2d: the yardstick of these rows) and the time of one q3_verify_draw pass for n in {2, 8, 32} at position ~64 with every
    draft right, and its break-even accepted drafts = pass time / sampled step time - 1.
Synthetic checkpoints fall into cycles under greedy decoding, which flatters self-lookup and says nothing about trained weights:
read the pass costs and break-even counts, not the self-lookup speed-up.  Writes <out>/spec_decode.json and spec_decode.md.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def worker(name, ctx, ckpt_dir, seed):
    import qwen3_rs_amd as q3
    from spec_sim import simulate
    ck = q3.checkpoint
    path = os.path.join(ckpt_dir, f"{name}-seed{seed}.q3bin")
    ck.ensure_synthetic_checkpoint(path, ck.SHAPES[name], seed=seed)
    tok0, N = 9, 256
    res = {"model": name, "ctx": ctx, "verify_ms": {}, "lookup": {}}

    def build(flags=0):
        b = q3.TransformerBuilder(path).with_ctx_length(ctx)
        b.flags |= flags
        return b.build()

    with build() as t:
        G = t.generate_greedy(tok0, 0, N)                               # warm-up + the reference tokens
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            assert t.generate_greedy(tok0, 0, N) == G
            times.append(time.perf_counter() - t0)
        step_ms = 1e3 * median(times) / N
        res["greedy_tok_s"] = N / median(times)
        res["greedy_step_ms"] = step_ms
        positions = [64] + ([2300] if name == "qwen3-4b" and ctx > 2400 else [])
        long_tokens = None
        for p in positions:
            if p > N:                                                   # a context of real rows in front of the block
                prompt = ck.iter_prompt_tokens(ck.SHAPES[name], 5, p)
                first = t.prefill(prompt, 0, batched=True)
                long_tokens = [first] + t.generate_greedy(first, p, 40)
        for mode, flags in (("graph", 0), ("eager", q3.FLAG_NO_GRAPH)):
            with build(flags) as v:
                for p in positions:
                    if p <= N:
                        v.generate_greedy(tok0, 0, p)
                        seq = [G[p - 1]] + G[p:p + 40]
                    else:
                        v.prefill(prompt, 0, batched=True)
                        seq = long_tokens
                    for n in (2, 4, 8, 16, 32):
                        v.verify(seq[:n], p)                            # plan + warm-up
                        ts = []
                        for _ in range(20):
                            t0 = time.perf_counter()
                            _, a = v.verify(seq[:n], p)
                            ts.append(time.perf_counter() - t0)
                        assert a == n - 1
                        ms = 1e3 * median(ts)
                        res["verify_ms"][f"{mode}/pos{p}/n{n}"] = {"ms": ms, "break_even_accepted": ms / step_ms - 1.0}
        # every draft right: blocks of 32 over G
        t.reset_kv()
        t.verify([tok0] + G[:31], 0)
        t.reset_kv()
        t0 = time.perf_counter()
        cur, k = tok0, 0
        while k + 32 <= N:
            nxt, a = t.verify([cur] + G[k:k + 31], k)
            cur, k = nxt[31], k + 32
        res["all_drafts_right_tok_s"] = k / (time.perf_counter() - t0)
        for label, corpus, ngram, dl in (("ngram64_no_draft", [], 64, 8), ("self_ngram2_d8", [], 2, 8), ("self_ngram3_d8", [], 3, 8),
                                         ("self_ngram2_d31", [], 2, 31)):
            n_run = 60 if ngram == 64 else N
            t.reset_kv()
            t.generate_lookup(corpus, tok0, 0, n_run, ngram=ngram, draft_len=dl)
            ts = []
            for _ in range(3):
                t.reset_kv()
                t0 = time.perf_counter()
                got, st = t.generate_lookup(corpus, tok0, 0, n_run, ngram=ngram, draft_len=dl)
                ts.append(time.perf_counter() - t0)
            assert got == G[:n_run]
            sim = simulate(G[:n_run], corpus, tok0, ngram, dl)
            assert (st.verify_passes, st.single_steps, st.drafted, st.accepted) == (sim["verify_passes"], sim["single_steps"], sim["drafted"], sim["accepted"])
            res["lookup"][label] = {"tok_s": n_run / median(ts), "verify_passes": st.verify_passes, "single_steps": st.single_steps,
                                    "drafted": st.drafted, "accepted": st.accepted, "distinct_tokens": len(set(G[:n_run])), "tokens": n_run}
    # section 2d: the same pass with every column drawn by the device sampler, against the sampled single-stream step
    T, topp, seed, p = 1.0, 0.9, 42, 64
    with build() as t:
        t.set_sampler(T, topp, seed)
        GS = t.generate_greedy(tok0, 0, N)                              # q3_generate_sampled: warm-up + the reference tokens
        times = []
        for _ in range(3):
            t.set_sampler(T, topp, seed)
            t0 = time.perf_counter()
            assert t.generate_greedy(tok0, 0, N) == GS
            times.append(time.perf_counter() - t0)
        sstep_ms = 1e3 * median(times) / N
        res["draw"] = {"temperature": T, "topp": topp, "sampled_tok_s": N / median(times), "sampled_step_ms": sstep_ms, "verify_ms": {}}
        t.set_sampler(T, topp, seed)
        t.generate_greedy(tok0, 0, p)
        rng_p = t.sampler_rng_state()                                   # the seed IS the state: every repeat draws the same coins
        seq = [GS[p - 1]] + GS[p:p + 40]
        for n in (2, 8, 32):
            t.verify_draw(seq[:n], p)                                   # scratch, plan + warm-up
            ts = []
            for _ in range(20):
                t.set_sampler(T, topp, rng_p)
                t0 = time.perf_counter()
                _, a = t.verify_draw(seq[:n], p)
                ts.append(time.perf_counter() - t0)
            assert a == n - 1
            ms = 1e3 * median(ts)
            res["draw"]["verify_ms"][f"graph/pos{p}/n{n}"] = {"ms": ms, "break_even_accepted": ms / sstep_ms - 1.0}
    print("BENCH_SPEC " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="qwen3-0.6b,qwen3-4b,qwen3-8b")
    ap.add_argument("--ctx", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--ckpt-dir", default=os.environ.get("Q3_CKPT_DIR", "/tmp"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds per model")
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.ctx, a.ckpt_dir, a.seed)
        return 0
    results = []
    for name in a.models.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", name, "--ctx", str(a.ctx), "--seed", str(a.seed),
                                "--ckpt-dir", a.ckpt_dir], capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"{name}: time limit of {a.timeout} s reached; nothing more is started", file=sys.stderr)
            break
        line = [l for l in r.stdout.splitlines() if l.startswith("BENCH_SPEC ")]
        if r.returncode != 0 or not line:
            print(f"{name}: exit status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}", file=sys.stderr)
            break
        results.append(json.loads(line[0][len("BENCH_SPEC "):]))
    if not results:
        return 1
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "spec_decode.json"), "w") as f:
        json.dump({"results": results}, f, indent=1)
    md = ["# Draft verification and prompt-lookup decode: pass costs (tools/bench_spec.py)", "",
          "Synthetic checkpoints cycle under greedy decoding: the self-lookup rows say how the loop behaves when drafts are mostly right,",
          "not what prompt lookup accepts on real text.  What carries over is the pass cost and the break-even count.",
          "The ngram-64 row (never a draft) covers 60 tokens at short positions: hold it against a greedy run of the same span, not",
          "against the 256-token greedy figure.", ""]
    for r in results:
        md += [f"## {r['model']} (context {r['ctx']})", "",
               f"greedy: {r['greedy_tok_s']:.1f} tok/s ({r['greedy_step_ms']:.3f} ms per step); every draft right, blocks of 32: "
               f"{r['all_drafts_right_tok_s']:.0f} tok/s", "",
               "| pass | ms | break-even accepted drafts |", "|---|---|---|"]
        md += [f"| {k} | {v['ms']:.3f} | {v['break_even_accepted']:.2f} |" for k, v in r["verify_ms"].items()]
        md += ["", "| lookup run | tok/s | passes | single steps | drafted | accepted | distinct tokens / tokens |", "|---|---|---|---|---|---|---|"]
        md += [f"| {k} | {v['tok_s']:.1f} | {v['verify_passes']} | {v['single_steps']} | {v['drafted']} | {v['accepted']} | {v['distinct_tokens']} / {v['tokens']} |"
               for k, v in r["lookup"].items()]
        md.append("")
        if "draw" in r:
            d = r["draw"]
            md += [f"under the sampler (temperature {d['temperature']}, top-p {d['topp']}): {d['sampled_tok_s']:.1f} tok/s "
                   f"({d['sampled_step_ms']:.3f} ms per sampled step)", "",
                   "| sampled pass (every draft right) | ms | break-even accepted drafts |", "|---|---|---|"]
            md += [f"| {k} | {v['ms']:.3f} | {v['break_even_accepted']:.2f} |" for k, v in d["verify_ms"].items()]
            md.append("")
    with open(os.path.join(a.out, "spec_decode.md"), "w") as f:
        f.write("\n".join(md))
    print(json.dumps({"models": [r["model"] for r in results], "out": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
