#!/usr/bin/env python3
"""Q4 checkpoints against their expanded Q8 twins, single-stream decode (profiles/w4.md):
   python3 tools/bench_w4.py [--shapes qwen3-0.6b,qwen3-4b,qwen3-8b] [--runs 5] [--tokens 128] [--out w4.json] [--wide]
Per shape: a synthetic Q4 file and checkpoint.expand_q4_checkpoint of it (the same values as int8, the same scales).
  rate    one process on the product library, the two engines taking turns: `runs` device loops of `tokens` tokens each,
          best / median / worst tokens per second.
  stamps  tools/kstamps.py's method (developer library, Q3_KSTAMPS=1, hipGraph replay): the average duration of the QKV, Wo,
          W1|W3 and W2 launches, one process per file; --wide adds the Q4 file under Q3_W4_WIDE=1 (the wider tiles of the sweep).
  model   bytes / 6.4 TB/s + 2.5 us beside each launch (weights + scales) -- a projection, not a measurement.
--batch (profiles/w4_batch.md): the batched state instead -- a context of 32 slots, Q4 against its expanded twin.
  rate    one process on the product library, the two engines taking turns: the step time of generate_greedy_batch at 32 and at
          8 streams and the time of a column pass of 8 columns (batch_step_cols), best / median / worst of `runs`.
  trace   rocprofv3 --kernel-trace over one process per file running `tokens` decode steps at 32 (and at 8) streams: the
          average duration of the QKV, Wo, W1|W3 and W2 launches (k_bgemm by its epilogue, k_dgemm alternating Wo, W2) and
          their spread.  (k_dgemm carries no in-kernel stamps: the trace is the one clock that covers the four families.)
  model   bytes / 6.4 TB/s + 2.5 us for both widths: weights + scales + the packed activations of the step.
Every measurement runs in a child process; the parent never touches the GPU."""
import argparse
import dataclasses
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-rs_amd"))
FIRST_TOK, FIRST_POS, CTX = 5, 7, 1024


def launch_bytes(s, bits):
    """weight + scale bytes of the four GEMV launches of a layer"""
    ahd, kvd, g = s.all_heads_dim, s.kv_dim, s.group_size
    elems = {"qkv": (ahd + 2 * kvd) * s.dim, "wo": s.dim * ahd, "w13": 2 * s.hidden_dim * s.dim, "w2": s.dim * s.hidden_dim}
    return {k: v * bits // 8 + 4 * (v // g) for k, v in elems.items()}


def child_rate(p4, p8, runs, tokens):
    import qwen3_rs_amd as q3
    eng = {4: q3.TransformerBuilder(p4).with_ctx_length(CTX).build(), 8: q3.TransformerBuilder(p8).with_ctx_length(CTX).build()}
    assert eng[4].weight_bits == 4 and eng[8].weight_bits == 8
    toks, rates = {}, {4: [], 8: []}
    for b, t in eng.items():                                  # warm-up, and the identity at the size that is timed
        toks[b] = t.generate_greedy(FIRST_TOK, FIRST_POS, tokens)
    for _ in range(runs):
        for b, t in eng.items():
            t.reset_kv()
            t0 = time.perf_counter()
            t.generate_greedy(FIRST_TOK, FIRST_POS, tokens)
            rates[b].append(tokens / (time.perf_counter() - t0))
    print(json.dumps({"tokens_equal": toks[4] == toks[8],
                      **{f"q{b}_tok_s": {"best": max(r), "median": statistics.median(r), "worst": min(r)} for b, r in rates.items()}}))


def child_stamps(path, tokens):
    import qwen3_rs_amd as q3
    t = q3.TransformerBuilder(path).with_ctx_length(CTX).build()
    t.generate_greedy(FIRST_TOK, FIRST_POS, 8)
    t.reset_kv()
    t.generate_greedy(FIRST_TOK, FIRST_POS, tokens)
    t.close()


def child_batch_rate(p4, p8, runs, steps):
    import qwen3_rs_amd as q3
    eng = {4: q3.TransformerBuilder(p4).with_ctx_length(CTX).build(), 8: q3.TransformerBuilder(p8).with_ctx_length(CTX).build()}
    for t in eng.values():
        t.batch_init(32, CTX)
    assert eng[4].batch_weight_bits == 4 and eng[8].batch_weight_bits == 8

    def decode(t, n):
        t.batch_reset_kv()
        t0 = time.perf_counter()
        out = t.generate_greedy_batch(list(range(5, 5 + n)), [FIRST_POS] * n, steps)
        return (time.perf_counter() - t0) / steps * 1e6, out.tolist()

    def cols(t):
        t.batch_reset_kv()
        t.batch_step_cols(list(range(8)), [5] * 8, [0] * 8)               # the plan, once
        t0 = time.perf_counter()
        for k in range(steps):
            out = t.batch_step_cols(list(range(8)), [5 + k] * 8, [k + 1] * 8)
        return (time.perf_counter() - t0) / steps * 1e6, out
    legs = {"decode32_us": lambda t: decode(t, 32), "decode8_us": lambda t: decode(t, 8), "cols8_us": cols}
    res = {"equal": {}}
    for leg, fn in legs.items():
        outs = {b: fn(t)[1] for b, t in eng.items()}                       # warm-up, and the identity at the size that is timed
        res["equal"][leg] = outs[4] == outs[8]
        us = {4: [], 8: []}
        for _ in range(runs):
            for b, t in eng.items():
                us[b].append(fn(t)[0])
        res[leg] = {f"q{b}": {"best": min(v), "median": statistics.median(v), "worst": max(v)} for b, v in us.items()}
    print(json.dumps(res))


def child_batch_trace(path, n, steps):
    import qwen3_rs_amd as q3
    t = q3.TransformerBuilder(path).with_ctx_length(CTX).build()
    t.batch_init(32, CTX)
    t.generate_greedy_batch(list(range(5, 5 + n)), [FIRST_POS] * n, steps)
    t.close()


def batch_trace(path, n, steps, outdir):
    """average / min / max duration (us) of the four matmul families of a decode step of n streams, from a kernel trace"""
    import csv
    import glob
    import shutil
    shutil.rmtree(outdir, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", outdir, "--", sys.executable, os.path.abspath(__file__),
           "--child-batch-trace", path, str(n), str(steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"rocprofv3 failed ({r.returncode}): {r.stderr[-400:]}")
    rows = []
    for f in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda d: int(d["Start_Timestamp"]))
    fam, resid = {"qkv": [], "wo": [], "w13": [], "w2": []}, 0
    for d in rows:
        name, us = d["Kernel_Name"].replace(" ", ""), (int(d["End_Timestamp"]) - int(d["Start_Timestamp"])) / 1e3
        if "k_dgemm<" in name or "k_bgemm<1," in name:                    # EPI_RESID = 1: the residual launches of a layer, Wo then W2
            fam["wo" if resid % 2 == 0 else "w2"].append(us)
            resid += 1
        elif "k_bgemm<4," in name:                                        # EPI_QKV
            fam["qkv"].append(us)
        elif "k_bgemm<2," in name:                                        # EPI_SWIGLU
            fam["w13"].append(us)
    shutil.rmtree(outdir, ignore_errors=True)
    return {k: {"avg": round(statistics.mean(v[len(v) // 4:]), 3), "p10": round(sorted(v[len(v) // 4:])[len(v[len(v) // 4:]) // 10], 3),
                "p90": round(sorted(v[len(v) // 4:])[9 * len(v[len(v) // 4:]) // 10], 3), "n": len(v)} for k, v in fam.items() if v}


def batch_bytes(s, bits, cols):
    """weight + scale + packed activation bytes of the four matmul launches of a layer at `cols` columns"""
    w = launch_bytes(s, bits)
    nt = 16 * ((cols + 15) // 16)
    act = {"qkv": s.dim, "wo": s.all_heads_dim, "w13": s.dim, "w2": s.hidden_dim}
    return {k: w[k] + nt * (act[k] + 4 * (act[k] // s.group_size)) for k in w}


def run_child(args, env=None, timeout=900):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(f"child {args[0]} failed ({r.returncode}): {r.stderr[-400:]}")
    return r


def stamps(path, tokens, wide=False):
    dev = os.path.join(ROOT, "qwen3-rs_amd", "libqwen3_hip_dev.so")
    env = dict(os.environ, Q3_KSTAMPS="1", Q3_HIP_LIB=dev)
    if wide:
        env["Q3_W4_WIDE"] = "1"
    r = run_child(["--child-stamps", path, tokens], env)
    k = json.loads([ln for ln in r.stderr.splitlines() if ln.startswith("[q3 kstamps]")][-1][len("[q3 kstamps] "):])
    return {f: round(v["avg_duration_us"], 3) for f, v in k["families"].items() if f in ("qkv", "wo", "w13", "w2")}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child-rate":
        return child_rate(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    if len(sys.argv) > 1 and sys.argv[1] == "--child-stamps":
        return child_stamps(sys.argv[2], int(sys.argv[3]))
    if len(sys.argv) > 1 and sys.argv[1] == "--child-batch-rate":
        return child_batch_rate(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    if len(sys.argv) > 1 and sys.argv[1] == "--child-batch-trace":
        return child_batch_trace(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="qwen3-0.6b,qwen3-4b,qwen3-8b")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--out")
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--trace-dir", default="/tmp/q3_w4_trace")
    ap.add_argument("--dir", default=os.environ.get("Q3_CKPT_DIR", "/tmp"))
    a = ap.parse_args()
    from qwen3_rs_amd import checkpoint as ck
    res = {}
    for name in a.shapes.split(","):
        s8 = ck.SHAPES[name]
        if a.layers:                                          # the shape's layers, fewer of them: the launches are the same, the files smaller
            s8, name = dataclasses.replace(s8, n_layers=a.layers), f"{name}-l{a.layers}"
        s4 = dataclasses.replace(s8, weight_bits=4)
        p4, p8 = os.path.join(a.dir, f"q3_{name}.q4.bin"), os.path.join(a.dir, f"q3_{name}.q4x.bin")
        ck.ensure_synthetic_checkpoint(p4, s4, seed=1234)
        if not (os.path.exists(p8) and os.path.getsize(p8) == s8.file_size()):
            ck.expand_q4_checkpoint(p4, p8)
        env = {k: v for k, v in os.environ.items() if k not in ("Q3_KSTAMPS", "Q3_HIP_LIB", "Q3_W4_WIDE")}
        if a.batch:
            out = json.loads(run_child(["--child-batch-rate", p4, p8, a.runs, a.tokens], env).stdout.strip().splitlines()[-1])
            out["launch_us"] = {f"{n}_streams": {"q4": batch_trace(p4, n, a.tokens, a.trace_dir), "q8": batch_trace(p8, n, a.tokens, a.trace_dir)}
                                for n in (32, 8)}
            out["byte_model_us"] = {f"{n}_streams": {f"q{b}": {k: round(v / 6.4e6 + 2.5, 2) for k, v in batch_bytes(s8, b, n).items()}
                                                     for b in (4, 8)} for n in (32, 8)}
            res[name] = out
            print(name, json.dumps(out), flush=True)
            continue
        out = json.loads(run_child(["--child-rate", p4, p8, a.runs, a.tokens], env).stdout.strip().splitlines()[-1])
        out["launch_us"] = {"q4": stamps(p4, a.tokens), "q8": stamps(p8, a.tokens)}
        if a.wide:
            out["launch_us"]["q4_wide"] = stamps(p4, a.tokens, wide=True)
        out["byte_model_us"] = {f"q{b}": {k: round(v / 6.4e6 + 2.5, 2) for k, v in launch_bytes(s8, b).items()} for b in (4, 8)}
        out["launch_bytes"] = {f"q{b}": launch_bytes(s8, b) for b in (4, 8)}
        res[name] = out
        print(name, json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
