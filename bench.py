#!/usr/bin/env python3
"""bench.py -- decode tokens/s of the MI355X Qwen3 Q8 engine on BASELINE.json's headline config.

Contract (driver):  python bench.py --gpus N --steps K --warmup W   -> ONE JSON line on stdout.
  step      = one decoded token: forward(token,pos) + greedy argmax, all on the device (weights, KV cache and
              the token feedback loop are resident in HBM when the timed region starts).
  workload  = BASELINE.json configs[1]: Qwen3-0.6B Q8 group=64 single-stream greedy decode on 1xMI355X --
              synthetic checkpoint (seed 1234) in the reference's format, 8-token prompt, the reference's
              `generate` call pattern (first forward at pos 7 over a zero KV prefix, generation.rs:26-29), ctx 1024
              (raised to the next multiple of 1024 that holds 7 + max(K, W) positions when the steps need more).
  N > 1     = N independent replicas, one process + one engine per GPU, no collective on the data path
              (the path does not shard: every listed model fits one GPU).  value = sum of tokens / max time.
  --dump-outputs DIR = after the timed steps, rank 0 writes what the timed loop handed back (tokens.npy: the K greedy
              tokens, float64) and the logits of its last step, recomputed after the timing (last_logits.npy, float32).

A plain run sets up, warms up, times the K steps and prints the line (value, ms_per_step, the end-to-end share of the
HBM roofline from the byte count).  Everything below needs runs of its own and comes only with --full:
  roofline  = the weight-streaming GEMV kernel (all instantiations of k_gemv): algorithmic weight bytes per
              launch / average launch period measured with HIP events on the engine's stream.
  forward_surface = the reference's own tok/s definition (TokenMetrics, generation.rs:198-233) on the reference's
              own surface: q3_forward + 4*vocab-byte logits copy + host argmax per token (generation.rs:153-162),
              driven from compiled host code (q3_host_generate).  PCIe-inclusive; never `value`.
  cpu_baseline = the CPU oracle (C restatement of the Rust path; no rustc in this image) timed on the host
              cores for the same run (all-core sweep winner AND one thread); also the checker of the GPU tokens:
              a token mismatch makes the line carry "parity": false and the process exit non-zero.
  other_configs = BASELINE configs 3 / 4 / 5 (one replica) measured by child processes in the same run.

Process model: the parent NEVER touches the GPU.  It writes the checkpoint (numpy), spawns one worker process per
GPU (`--worker`, RANK/LOCAL_RANK/WORLD_SIZE in the environment, gloo for the barrier and the max/sum of the timing
when N > 1), runs the CPU leg itself and relays ONE line.  Under torchrun (WORLD_SIZE already set) every rank is a
worker and rank 0 prints the line.
"""
import argparse
import json
import os
import signal
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "qwen3-rs_amd"))
sys.path.insert(0, ROOT)

HBM_PEAK_BYTES_PER_S = 8.0e12   # MI355X spec (MI355X_MICROARCH.md: 8 TB/s; ~6.29 TB/s measured copy ceiling)
SEED = 1234


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# --------------------------------------------------------------------------------------------------------------
# shared helpers
# --------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--shape", default="qwen3-0.6b")
    ap.add_argument("--ctx", type=int, default=None, help="context length (default 1024, or more when the steps need it)")
    ap.add_argument("--fast", action="store_true", help="opt-in tree-reduction mode (not bit-exact)")
    ap.add_argument("--full", action="store_true",
                    help="also roofline, forward_surface, tolerance_mode, cpu_baseline + parity, graph-replay stamps and other_configs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's outputs as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the configs 3/4/5 sub-results")
    ap.add_argument("--no-graph-stamps", action="store_true", help="roofline from eager HIP events only (skip the graph-replay stamp run)")
    ap.add_argument("--no-tolerance-mode", action="store_true", help="skip the Q3_FLAG_FAST comparison block")
    ap.add_argument("--other-budget-s", type=float, default=420.0, help="wall budget for the other_configs children")
    ap.add_argument("--ckpt-dir", default=os.environ.get("Q3_CKPT_DIR", "/tmp"))
    ap.add_argument("--worker", action="store_true", help="internal: one replica (spawned by the parent or by torchrun)")
    ap.add_argument("--stub-engine", action="store_true",
                    help="launcher self-test: workers use a host stub instead of the HIP engine (no GPU, CPU tests only)")
    return ap.parse_args(argv)


def ckpt_path(args):
    return os.path.join(args.ckpt_dir, f"q3_{args.shape}.bin")


def run_setup(args):
    from qwen3_rs_amd import checkpoint as ck
    shape = ck.SHAPES[args.shape]
    prompt = ck.iter_prompt_tokens(shape, SEED, 8)
    first_tok, first_pos = prompt[-1], len(prompt) - 1
    need = first_pos + max(args.steps, args.warmup)
    if args.ctx is None:
        # whole multiples of 1024 positions: the engine takes the context as seq_len, and its product attention forms need
        # seq_len % 8 == 0 (k_attn_short2) and % 4 == 0 (the transposed value cache of k_attn_out); other lengths fall back
        args.ctx = min(-(-need // 1024) * 1024, shape.max_seq_len)
    if need > min(args.ctx, shape.max_seq_len):
        raise SystemExit(f"steps exceed ctx ({need} positions, ctx {args.ctx}, model {shape.max_seq_len})")
    return shape, first_tok, first_pos


def gemv_bytes_per_launch(shape):
    """Algorithmic bytes one launch of each GEMV family streams: int8 weights + f32 group scales, read once
    (SURVEY.md section 8d)."""
    g = shape.group_size
    f = 1.0 + 4.0 / g
    d, h, ahd, kvd, v = shape.dim, shape.hidden_dim, shape.all_heads_dim, shape.kv_dim, shape.vocab_size
    return {"qkv": (ahd + 2 * kvd) * d * f, "wo": d * ahd * f, "w13": 2 * h * d * f, "w2": d * h * f, "lm_head": v * d * f}


def pmc_traffic(shape_name):
    """HBM read bytes per launch of the dominant streaming kernel from the committed PMC pass (rocprofv3 --pmc
    FETCH_SIZE, corrected x2 for gfx950 as MI355X_MICROARCH.md prescribes).  Counters cannot be read from inside
    this process, so the value comes from profiles/ (null when no profile of this shape is committed)."""
    suffix = {"qwen3-0.6b": "", "qwen3-4b": "_4b", "qwen3-8b": "_8b", "deepseek-r1-0528-qwen3-8b": "_8b"}.get(shape_name)
    if suffix is None:
        return None
    for rnd in ("r06", "r05", "r04", "r03", "r02", "r01"):
        f = os.path.join(ROOT, "profiles", f"{rnd}_pmc_fetch_size{suffix}.json")
        if not os.path.exists(f):
            continue
        try:
            k = json.load(open(f))["kernels"]
            tot = sum(v["avg_hbm_read_bytes_corrected"] * v["dispatches"] for n, v in k.items() if "k_gemv" in n)
            cnt = sum(v["dispatches"] for n, v in k.items() if "k_gemv" in n)
            return int(tot / cnt) if cnt else None
        except Exception:
            continue
    return None


# --------------------------------------------------------------------------------------------------------------
# worker: one replica on one GPU
# --------------------------------------------------------------------------------------------------------------
class _StubEngine:
    """Launcher self-test only (--stub-engine): no GPU, no oracle; deterministic fake tokens so the CPU test of
    `--gpus 2` can check process spawning, rank plumbing and aggregation."""

    def __init__(self, rank):
        self.rank = rank

    def generate_greedy(self, tok, pos, n):
        time.sleep(0.001 * n)
        return [(tok + pos + k) % 1000 for k in range(n)]

    def reset_kv(self):
        pass

    def close(self):
        pass


def dist_setup():
    """Replicas only: gloo carries the barrier and the max/sum of the timing -- never the data path."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if not dist.is_initialized():
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    return rank, world, local_rank


def barrier():
    # one replica never imports torch (its import alone takes seconds); dist_setup imported it when there are more
    dist = sys.modules.get("torch.distributed")
    if dist is not None and dist.is_available() and dist.is_initialized():
        dist.barrier()


def aggregate_over_ranks(local_tokens, local_seconds):
    """(sum of tokens over ranks, max of seconds over ranks).  Single process: identity."""
    if "torch.distributed" not in sys.modules:
        return int(local_tokens), float(local_seconds)
    try:
        import torch
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            t = torch.tensor([float(local_tokens)], dtype=torch.float64)
            s = torch.tensor([float(local_seconds)], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            dist.all_reduce(s, op=dist.ReduceOp.MAX)
            return int(round(t.item())), float(s.item())
    except ImportError:
        pass
    return int(local_tokens), float(local_seconds)


def dump_outputs(out_dir, eng, tokens, first_tok, first_pos):
    """What the timed loop computed in its last step: the K tokens it handed back (float64 holds them exactly) and the
    logits of its last step.  q3_generate_greedy keeps those logits on the device, so the last step's forward is run once
    more (q3_forward) on the same KV prefix, after the timing; their argmax must be the loop's last token."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "tokens.npy"), np.asarray(tokens, dtype=np.float64))
    if hasattr(eng, "forward"):
        feed = [first_tok] + [int(t) for t in tokens]
        logits = np.array(eng.forward(feed[-2], first_pos + len(tokens) - 1), dtype=np.float32)
        last_max = logits.size - 1 - int(np.argmax(logits[::-1]))         # sample_argmax: the last maximum
        if last_max != int(tokens[-1]):
            raise RuntimeError(f"recomputed last-step logits pick token {last_max}, the timed loop gave {tokens[-1]}")
        np.save(os.path.join(out_dir, "last_logits.npy"), logits)


def worker_main(args):
    """Returns the result dict on rank 0 (None elsewhere)."""
    rank, world, local_rank = dist_setup()
    shape, first_tok, first_pos = run_setup(args)
    K, W = args.steps, args.warmup
    path = ckpt_path(args)
    if not args.worker and not args.stub_engine:
        # launched by torchrun (no parent of ours wrote the checkpoint): rank 0 writes it, everyone waits
        if rank == 0:
            from qwen3_rs_amd import checkpoint as ck
            ck.ensure_synthetic_checkpoint(path, shape, seed=SEED)
        barrier()
    if args.stub_engine:
        eng = _StubEngine(rank)
    else:
        import qwen3_rs_amd as q3
        eng = q3.TransformerBuilder(path).with_ctx_length(args.ctx).with_device(local_rank).with_strict(not args.fast).build()
    if W > 0:
        eng.generate_greedy(first_tok, first_pos, W)      # untimed warmup steps
    eng.reset_kv()                                         # ends in a stream synchronise, like generate_greedy

    barrier()
    t0 = time.perf_counter()
    tokens = eng.generate_greedy(first_tok, first_pos, K)   # exactly K steps; returns after the stream drained
    dt = time.perf_counter() - t0
    barrier()
    total_tokens, max_dt = aggregate_over_ranks(K, dt)
    if rank != 0:
        eng.close()
        return None
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, eng, tokens, first_tok, first_pos)

    value = total_tokens / max_dt
    wq, ws = shape.weight_bytes_per_token()
    bytes_per_token = wq + ws
    out = {"metric": "decode tokens/sec Qwen3-0.6B Q8 g=64 @1 GPU; % of int8 HBM roofline" if args.shape == "qwen3-0.6b"
           else f"decode tokens/sec {args.shape} Q8 g=64",
           "value": round(value, 2), "unit": "tokens/s", "n_gpus": world, "steps": K, "warmup": W,
           "ms_per_step": round(max_dt / K * 1e3, 5), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "i8 (int8 x int8 -> i32 group dots, f32 scales/accumulate)", "data": "synthetic",
           "config": {"workload": f"{args.shape} Q8 group={shape.group_size} single-stream greedy decode, 8-token prompt, "
                                  f"reference generate-mode call pattern (first forward at pos 7, zero KV prefix), "
                                  f"ctx {args.ctx}, {K} tokens",
                      "mode": "tree-reduction (opt-in, not bit-exact)" if args.fast else "reference summation order (bit-identical logits)",
                      "replicas": world, "checkpoint_seed": SEED,
                      "algorithmic_bytes_per_token": bytes_per_token},
           "pct_of_hbm_roofline_end_to_end": round(100.0 * (value / world) * bytes_per_token / HBM_PEAK_BYTES_PER_S, 2),
           "_tokens": [int(t) for t in tokens]}
    if args.stub_engine:
        out["roofline"] = None
        eng.close()
        return out
    # which binary produced the numbers: the id baked into the loaded library next to the hash of the sources here
    out["build_id"] = {"library": q3.load_library().q3_build_id().decode(), "sources": q3.source_build_id()}
    if not args.full:
        eng.close()
        return out

    # ---- roofline of the dominant kernel: HIP events on the engine stream, one forward per rep (eager launches)
    reps = 20
    prof = eng.profile(first_tok, first_pos + K // 2, reps)
    bpl = gemv_bytes_per_launch(shape)
    per_kernel, gemv_ms, gemv_launches, gemv_bytes = [], 0.0, 0, 0.0
    for name, ms, n in prof:
        if n == 0:
            continue
        avg_us = ms / n * 1e3
        row = {"kernel": name, "launches_per_token": n // reps, "avg_us": round(avg_us, 3)}
        if name in bpl:
            row["bytes_per_launch"] = int(bpl[name])
            row["achieved_GBps"] = round(bpl[name] / (avg_us * 1e-6) / 1e9, 1)
            gemv_ms += ms
            gemv_launches += n
            gemv_bytes += bpl[name] * n
        per_kernel.append(row)
    achieved = gemv_bytes / (gemv_ms * 1e-3)                 # B/s over all GEMV launches
    out["roofline"] = {"bound": "hbm", "kernel": "k_gemv (W8A8 group-quant GEMV, all instantiations)",
                       "achieved": round(achieved / 1e9, 1), "peak": HBM_PEAK_BYTES_PER_S / 1e9, "unit": "GB/s",
                       "frac": round(achieved / HBM_PEAK_BYTES_PER_S, 4), "traffic": pmc_traffic(args.shape),
                       "bytes_per_launch": int(gemv_bytes / gemv_launches),
                       "avg_launch_us": round(gemv_ms / gemv_launches * 1e3, 3),
                       "launches_per_token": gemv_launches // reps, "per_kernel": per_kernel,
                       "note": "avg launch period = HIP events bracketing each kernel family's launches of one forward on the "
                               "engine stream (kernel + boundary, the quantity rocprofv3 per-dispatch durations sum to); traffic = avg "
                               "HBM read bytes per k_gemv launch from the committed PMC pass (profiles/)"}

    # ---- the reference's own surface and tok/s definition (TokenMetrics): forward + logits copy + host argmax
    try:
        eng.reset_kv()
        eng.host_generate(first_tok, first_pos, min(4, K))          # untimed: first-touch of the pinned logits buffer
        # two timed runs, the faster one reported (both listed): this leg is half host work -- a synchronous graph launch, a 607 KB
        # copy + argmax pass -- and the shared hosts' load moves it by 5-10 % between runs of the same binary
        fs_runs = []
        for _ in range(2):
            eng.reset_kv()
            fs_tokens, fs_s1 = eng.host_generate(first_tok, first_pos, K)
            fs_runs.append(fs_s1)
        fs_s = min(fs_runs)
        out["forward_surface"] = {
            "value": round(K / fs_s, 2), "unit": "tokens/s", "ms_per_step": round(fs_s / K * 1e3, 5),
            "runs_tok_s": [round(K / t, 2) for t in fs_runs],
            "tokens_match_device_loop": [int(t) for t in fs_tokens] == [int(t) for t in tokens],
            "definition": "TokenMetrics (generation.rs:198-233) around generate_next_token (generation.rs:153-162): q3_forward "
                          "(host-synchronous, 4*vocab bytes of logits over PCIe) + logits copy + host sample_argmax, K tokens, "
                          "compiled host loop (q3_host_generate) standing in for the Rust shim"}
        # BASELINE configs 1 / 2 are 128-token runs: both surfaces on 128 tokens whatever --steps is, so the
        # config-true figures are in the driver's record too; and the ratio of the two surfaces with ONE policy for both legs
        # (best of two runs each)
        n128 = min(128, args.ctx - first_pos)
        dev_runs, fs128_runs, tok128, fs128_tok = [], [], None, None
        for _ in range(2):
            eng.reset_kv()
            t1 = time.perf_counter()
            tok128 = eng.generate_greedy(first_tok, first_pos, n128)
            dev_runs.append(time.perf_counter() - t1)
        for _ in range(2):
            eng.reset_kv()
            fs128_tok, s1 = eng.host_generate(first_tok, first_pos, n128)
            fs128_runs.append(s1)
        out["value_128"] = {"value": round(n128 / min(dev_runs), 2), "unit": "tokens/s", "tokens": n128,
                            "runs_tok_s": [round(n128 / t, 2) for t in dev_runs],
                            "what": "the device-resident greedy loop of `value` on the 128-token run of BASELINE configs 1 / 2, best of two"}
        out["forward_surface_128"] = {"value": round(n128 / min(fs128_runs), 2), "unit": "tokens/s", "tokens": n128,
                                      "runs_tok_s": [round(n128 / t, 2) for t in fs128_runs],
                                      "ratio_to_device_loop": round(min(dev_runs) / min(fs128_runs), 4),
                                      "tokens_match_device_loop": [int(t) for t in fs128_tok] == [int(t) for t in tok128]}
        if not out["forward_surface_128"]["tokens_match_device_loop"]:
            out["forward_surface"]["tokens_match_device_loop"] = False
    except Exception as e:
        log(f"[bench] forward_surface failed: {e!r}")
        out["forward_surface"] = None
    if not args.fast and not args.no_tolerance_mode:
        try:
            out["tolerance_mode"] = tolerance_mode_block(q3, eng, path, args, local_rank, first_tok, first_pos)
        except Exception as e:
            log(f"[bench] tolerance_mode failed: {e!r}")
            out["tolerance_mode"] = {"error": repr(e)[:300]}
    eng.close()
    return out


def tolerance_mode_block(q3, eng, path, args, device, first_tok, first_pos, n_logit_tokens=6):
    """What the reference summation order costs (never `value`): the same workload on a Q3_FLAG_FAST engine -- wavefront-tree
    reductions for the RMSNorm / attention sums and the GEMV group fold; the int8 group dots stay exact -- next to the strict engine
    `eng` of this process.  tok/s over min(128, ctx) tokens (best of two, like value_128), max |delta logit| on the first
    n_logit_tokens forwards (both engines fed the STRICT tokens, so the same inputs are compared; the strict logits are the CPU
    oracle's bit for bit -- tests/test_gpu_parity.py, and `parity` of this line for the tokens), and how many leading greedy tokens
    of the free-running fast loop equal the strict ones."""
    import numpy as np
    n = min(128, args.ctx - first_pos)
    runs, strict_tok = [], None
    for _ in range(2):
        eng.reset_kv()
        t1 = time.perf_counter()
        strict_tok = eng.generate_greedy(first_tok, first_pos, n)
        runs.append(time.perf_counter() - t1)
    strict_s = min(runs)
    eng.reset_kv()
    feed = [first_tok] + [int(t) for t in strict_tok]
    strict_logits = [np.array(eng.forward(feed[k], first_pos + k), copy=True) for k in range(n_logit_tokens)]
    top2 = [np.sort(l)[-2:] for l in strict_logits]
    fast = q3.TransformerBuilder(path).with_ctx_length(args.ctx).with_device(device).with_strict(False).build()
    try:
        fast.generate_greedy(first_tok, first_pos, min(8, n))
        runs, fast_tok = [], None
        for _ in range(2):
            fast.reset_kv()
            t1 = time.perf_counter()
            fast_tok = fast.generate_greedy(first_tok, first_pos, n)
            runs.append(time.perf_counter() - t1)
        fast_s = min(runs)
        fast.reset_kv()
        dl = []
        for k in range(n_logit_tokens):
            fl = np.array(fast.forward(feed[k], first_pos + k), copy=True)
            dl.append(float(np.max(np.abs(fl - strict_logits[k]))))
    finally:
        fast.close()
    lead = 0
    for a, b in zip(fast_tok, strict_tok):
        if int(a) != int(b):
            break
        lead += 1
    return {"flags": "Q3_FLAG_FAST", "tokens": n, "value": round(n / fast_s, 2), "unit": "tokens/s",
            "strict_value_same_run": round(n / strict_s, 2), "ratio_to_strict": round(strict_s / fast_s, 4),
            "max_abs_delta_logit_first_tokens": [round(d, 6) for d in dl],
            "strict_top1_minus_top2_first_tokens": [round(float(t[1] - t[0]), 6) for t in top2],
            "strict_logit_std_first_tokens": [round(float(np.std(l)), 4) for l in strict_logits],
            "leading_tokens_identical_to_strict": lead,
            "what": "tree reductions (RMSNorm sum of squares, QK-norm, attention scores / softmax sum / value sums, GEMV group fold) "
                    "instead of the reference's sequential f32 sums; int8 group dots exact in both modes.  Never `value`: on the "
                    "synthetic checkpoint's near-flat logits a 1e-7 reordering difference is amplified by the re-quantisation "
                    "steps and flips greedy tokens (DESIGN.md section 3)"}


# --------------------------------------------------------------------------------------------------------------
# parent: CPU leg, other configs, launcher
# --------------------------------------------------------------------------------------------------------------
def cpu_baseline(path, ctx, first_tok, first_pos, gpu_tokens, max_tokens=128, budget_s=25.0, one_thread_budget_s=10.0):
    """Oracle leg (test infrastructure used as the reported CPU baseline, kind "port").  Sample = the first
    max_tokens (128) generated tokens of the same workload whatever --steps is, bounded by budget_s.
    Thread count: a sweep timed on 8 tokens per candidate, median of 3 repetitions each (a token is ~200 OpenMP
    fork-joins, so "all cores" loses to fewer threads on big hosts and a 2-token sweep was noise: VERDICT r2); the whole
    sweep table goes into the JSON so a run-to-run spread is visible.  The OpenMP runtime is pinned
    (OMP_PROC_BIND=close, OMP_PLACES=cores) and keeps its workers spinning between the parallel regions
    (OMP_WAIT_POLICY=active) -- set by parent_main before libgomp is loaded.  `cores` is the count actually used; a
    one-thread figure over a shorter bounded sample is reported too."""
    from oracle import q3_oracle as co
    co.build()
    m = co.OracleModel(path, ctx)
    m.forward(first_tok, first_pos)           # untimed: page-in of the mmap'd checkpoint
    ncpu = os.cpu_count() or 1
    want = min(max_tokens, ctx - first_pos)
    # more threads than ~64 never won on the 128-core / 256-thread GPU hosts, and with spinning workers
    # (OMP_WAIT_POLICY=active) an oversubscribed team takes minutes per token: the sweep stops at 64
    cands = sorted({c for c in (4, 8, 16, 32, 64) if c <= ncpu})

    def run(threads, limit, budget, pos0=None):
        co.set_num_threads(threads)
        m.reset()
        tok, pos, toks = first_tok, (first_pos if pos0 is None else pos0), []
        t0 = time.perf_counter()
        while len(toks) < limit and (time.perf_counter() - t0 < budget or len(toks) < 2):
            tok = co.sample_argmax(m.forward(tok, pos))
            toks.append(tok)
            pos += 1
        return toks, time.perf_counter() - t0

    sweep_tokens = min(8, want)
    # the sweep's 8 tokens sit in the MIDDLE of the timed run's positions (zero KV prefix: only the timing is read): the oracle's
    # strict-order attention grows with the position -- ~10 % of a token at position 130 -- and a sweep at positions 7..14 read
    # 10 % faster than the 128-token run it is compared with (r04: value_over_sweep_row 0.89-0.93 on an otherwise quiet host)
    sweep_pos0 = first_pos + max(0, (want - sweep_tokens) // 2)
    sweep, t_sweep0 = [], time.perf_counter()
    for c in cands:
        rates = []
        for _ in range(3):
            if time.perf_counter() - t_sweep0 > 20.0 and rates:
                break
            tk, dt = run(c, sweep_tokens, 5.0, sweep_pos0)
            rates.append(len(tk) / dt)
        rates_s = sorted(rates)
        sweep.append({"threads": c, "tok_s_median": round(rates_s[len(rates_s) // 2], 2), "tok_s_all": [round(r, 2) for r in rates]})
    best_c = max(sweep, key=lambda r: r["tok_s_median"])["threads"]     # the median: a count that is fast once and slow twice loses

    # The reported figure: SURVEY 8d's 128 generated tokens whatever --steps was (the CPU generates its own greedy
    # continuation; the first min(steps, 128) tokens are the ones compared with the GPU), median of 3 timed runs at
    # the chosen thread count, after one untimed token that lets the OpenMP team of that size form and settle
    # (20 tokens timed right behind a 64-thread spinning team disagreed with the sweep by 1.6x).
    full = min(max_tokens, ctx - first_pos)
    run(best_c, 1, 5.0)
    runs = []
    t_leg0 = time.perf_counter()
    for _ in range(3):
        if runs and time.perf_counter() - t_leg0 > budget_s:
            break
        tk, dt = run(best_c, full, budget_s)
        runs.append((len(tk) / dt, tk, dt))
    runs_sorted = sorted(runs, key=lambda r: r[0])
    rate, toks, dt = runs_sorted[len(runs_sorted) // 2]
    # the winner's sweep row once more, AFTER the timed runs: on these shared 256-thread hosts the rate of one thread count drifts
    # by 10-40 % within a minute, and `value` has to be read against a sweep row taken under the same load
    after = []
    for _ in range(3):
        tk, dta = run(best_c, sweep_tokens, 5.0, sweep_pos0)
        after.append(len(tk) / dta)
    for row in sweep:
        if row["threads"] == best_c:
            row["tok_s_median_after_timed_runs"] = round(sorted(after)[1], 2)
    run(1, 1, 5.0)
    toks1, dt1 = run(1, full, one_thread_budget_s)
    m.close()
    gpu = [int(t) for t in gpu_tokens]
    ncmp, ncmp1 = min(len(toks), len(gpu)), min(len(toks1), len(gpu))

    def agrees(tk):            # every timed run is compared over ITS OWN length: a run the budget cut short is not a mismatch
        k = min(len(tk), len(gpu))
        return k > 0 and tk[:k] == gpu[:k]

    match = ncmp > 0 and all(agrees(r[1]) for r in runs) and toks1[:ncmp1] == gpu[:ncmp1]
    ncmp_min = min(min(len(r[1]), len(gpu)) for r in runs)
    sweep_best = max(r["tok_s_median"] for r in sweep)
    return {"value": rate, "unit": "tokens/s", "cores": best_c, "kind": "port",
            "sample": f"{len(toks)} generated tokens of the same workload ({dt:.1f} s; median of {len(runs)} runs: "
                      f"{[round(r[0], 1) for r in runs]}) on {best_c} of {ncpu} host threads "
                      f"(winner of the sweep below: {sweep_tokens} tokens per candidate at positions {sweep_pos0}.., median of 3); C restatement of the Rust CPU "
                      f"path (no rustc in the image), OpenMP over rows/heads like rayon, threads pinned "
                      f"(OMP_PROC_BIND={os.environ.get('OMP_PROC_BIND')}, OMP_PLACES={os.environ.get('OMP_PLACES')}, "
                      f"OMP_WAIT_POLICY={os.environ.get('OMP_WAIT_POLICY')})",
            "thread_sweep": sweep, "value_over_sweep_row": round(rate / sweep_best, 3),
            "value_over_sweep_row_after": round(rate / sorted(after)[1], 3),
            "one_thread": {"value": len(toks1) / dt1, "unit": "tokens/s", "cores": 1,
                           "sample": f"first {len(toks1)} generated tokens ({dt1:.1f} s) on 1 host thread"},
            "tokens_compared": ncmp, "tokens_compared_shortest_run": ncmp_min, "tokens_match_gpu": bool(match)}, match


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _kill_group(p):
    """End a child AND everything it started (a bench.py child owns a --worker grandchild that holds the GPU)."""
    try:
        os.killpg(p.pid, signal.SIGTERM)
    except (ProcessLookupError, PermissionError):
        return
    try:
        p.wait(timeout=10)
    except subprocess.TimeoutExpired:
        pass
    try:
        os.killpg(p.pid, signal.SIGKILL)          # whatever of the group is still alive (no-op once it is gone)
    except (ProcessLookupError, PermissionError):
        pass


def spawn_workers(args, n, timeout_s=1500.0):
    """N worker processes, spawned BEFORE anything in this process touches HIP (it never does).  Each worker leads its
    own process group; all ranks are polled, and as soon as one exits non-zero (or the overall timeout passes) the
    rest are ended -- nobody is left waiting in a gloo barrier for a rank that died."""
    port = free_port()
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--gpus", str(n), "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--shape", args.shape, "--ctx", str(args.ctx), "--ckpt-dir", args.ckpt_dir]
    if args.fast:
        cmd.append("--fast")
    if args.full:
        cmd.append("--full")
    if args.dump_outputs:
        cmd += ["--dump-outputs", os.path.abspath(args.dump_outputs)]
    if args.stub_engine:
        cmd.append("--stub-engine")
    procs = []
    import tempfile
    out0 = tempfile.TemporaryFile(mode="w+")
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen(cmd, env=env, stdout=out0 if r == 0 else subprocess.DEVNULL, text=True,
                                      start_new_session=True))
    t0, failed = time.time(), None
    while True:
        rcs = [p.poll() for p in procs]
        if all(rc is not None for rc in rcs):
            break
        bad = [i for i, rc in enumerate(rcs) if rc not in (None, 0)]
        if bad:
            failed = f"rank {bad[0]} exited with code {rcs[bad[0]]}"
            break
        if time.time() - t0 > timeout_s:
            failed = f"timeout after {timeout_s:.0f} s"
            break
        time.sleep(0.05)
    if failed:
        for p in procs:
            if p.poll() is None:
                _kill_group(p)
        raise SystemExit(f"[bench] workers failed: {failed}; exit codes {[p.poll() for p in procs]}")
    out0.seek(0)
    line = [ln for ln in out0.read().splitlines() if ln.startswith("{")]
    if not line:
        raise SystemExit("[bench] rank 0 printed no result line")
    return json.loads(line[-1])


def run_child_json(cmd, timeout):
    """One other_configs child in its own process group; on timeout the whole group goes (the config-5 child is itself a
    bench.py parent whose --worker grandchild owns the GPU)."""
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        so, se = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        _kill_group(p)
        try:
            p.communicate(timeout=5)
        except Exception:
            pass
        return {"error": f"timeout after {timeout:.0f} s"}
    except BaseException:
        _kill_group(p)
        raise
    lines = [ln for ln in so.splitlines() if ln.startswith("{")]
    if not lines:
        return {"error": f"rc {p.returncode}", "stderr_tail": se[-400:]}
    d = json.loads(lines[-1])
    d["rc"] = p.returncode
    return d


def other_configs(args):
    """BASELINE configs 3 / 4 / 5 measured in this run by child processes (each owns the GPU in turn; the parent holds
    no GPU state).  Checkpoints are cached in --ckpt-dir.  Bounded by --other-budget-s: what does not fit is reported as
    skipped, never silently dropped."""
    py, tools = sys.executable, os.path.join(ROOT, "tools")
    plan = [
        ("config3 Qwen3-4B 2048-token prefill + 512-token decode",
         [py, os.path.join(tools, "bench_chat.py"), "--ckpt-dir", args.ckpt_dir]),
        ("config4 Qwen3-8B batch=32 concurrent decode streams",
         [py, os.path.join(tools, "bench_batch.py"), "--ckpt-dir", args.ckpt_dir, "--steps", "256"] +
         ([] if args.no_tolerance_mode else ["--tolerance", "64"])),
        ("config5 DeepSeek-R1-0528-Qwen3-8B, one replica of the data-parallel set",
         [py, os.path.abspath(__file__), "--shape", "deepseek-r1-0528-qwen3-8b", "--steps", "32", "--warmup", "4", "--full",
          "--no-cpu-baseline", "--no-other-configs", "--ckpt-dir", args.ckpt_dir]),
    ]
    t0, res = time.time(), {}
    for name, cmd in plan:
        left = args.other_budget_s - (time.time() - t0)
        if left < 60:
            res[name] = {"skipped": "other-configs wall budget exhausted"}
            continue
        log(f"[bench] other_configs: {name} ...")
        d = run_child_json(cmd, left)
        for k in ("_tokens",):
            d.pop(k, None)
        if isinstance(d.get("roofline"), dict):
            d["roofline"].pop("note", None)
        res[name] = d
        log(f"[bench] other_configs: {name} done ({time.time() - t0:.0f} s elapsed)")
    return res


def roofline_from_graph_stamps(out, args, shape, first_tok, first_pos, path):
    """`roofline.achieved` from kernel DURATIONS under hipGraph replay -- the launch mode `value` is measured in -- instead of eager
    HIP-event periods: tools/kstamps.py runs the same device loop once on the product library and once on the developer library with
    in-kernel begin / end stamps (lane 0 of every wave, s_memrealtime); both in child processes (this process never touches the GPU).
    achieved = algorithmic bytes of all k_gemv launches of a token / the sum of their stamped durations (gaps between launches are
    NOT kernel time and are reported separately).  The stamped durations include the instrumentation (`stamp_overhead_us_per_launch`,
    measured: (stamped - product) wall time per token / launches per token, fold launches included) -- they are used as measured, so
    the fraction is an under-estimate by that much.  The eager HIP-event figure of the worker stays as `eager_check`."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kstamps
    gk = kstamps.graph_kernel_durations(n=max(args.steps, 16), shape_name=args.shape, ctx=args.ctx, first_tok=first_tok,
                                        first_pos=first_pos, ckpt=path)
    rf = out["roofline"]
    lib_id = (out.get("build_id") or {}).get("library")
    if gk["build_id"] != lib_id or gk["stamped_build_id"] != lib_id:
        raise RuntimeError(f"stamped run is another build ({gk['build_id']} / {gk['stamped_build_id']} vs {lib_id})")
    bpl = gemv_bytes_per_launch(shape)
    tot_b, tot_us, nl, per = 0.0, 0.0, 0, []
    for fam, v in gk["families"].items():
        row = {"kernel": fam, "launches_per_token": v["launches_per_token"], "avg_duration_us": v["avg_duration_us"],
               "avg_gap_to_predecessor_us": v["avg_gap_to_predecessor_us"]}
        if fam in bpl:
            row["bytes_per_launch"] = int(bpl[fam])
            row["achieved_GBps"] = round(bpl[fam] / (v["avg_duration_us"] * 1e-6) / 1e9, 1)
            tot_b += bpl[fam] * v["launches_per_token"]
            tot_us += v["avg_duration_us"] * v["launches_per_token"]
            nl += v["launches_per_token"]
        per.append(row)
    achieved = tot_b / (tot_us * 1e-6)
    eager = {k: rf[k] for k in ("achieved", "frac", "avg_launch_us", "per_kernel", "note") if k in rf}
    rf.update({"achieved": round(achieved / 1e9, 1), "frac": round(achieved / HBM_PEAK_BYTES_PER_S, 4),
               "avg_launch_us": round(tot_us / nl, 3), "launches_per_token": nl, "per_kernel": per,
               "source": "graph-replay kernel durations (in-kernel stamps, developer build of the same sources, this run)",
               "graph_mode": {k: gk[k] for k in ("product_library_us_per_token", "stamped_developer_library_us_per_token",
                                                 "sum_duration_plus_gap_us_per_token", "wall_us_per_token_this_call",
                                                 "stamp_overhead_us_per_launch", "tokens_folded", "build_id")},
               "eager_check": eager,
               "note": "achieved = algorithmic bytes of a token's k_gemv launches / sum of their durations (first wave in .. last wave "
                       "out) under hipGraph replay, stamp overhead included as measured; eager_check = the HIP-event launch PERIODS "
                       "(kernel + boundary) of one eager forward; traffic = avg HBM read bytes per k_gemv launch from the committed "
                       "PMC pass (profiles/)"})


def parent_main(args):
    # the CPU leg's OpenMP runtime: pinned threads that spin between parallel regions (must be set before libgomp loads)
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")
    os.environ.setdefault("OMP_WAIT_POLICY", "active")
    from qwen3_rs_amd import checkpoint as ck
    shape, first_tok, first_pos = run_setup(args)
    path = ckpt_path(args)
    if not args.stub_engine:
        t0 = time.time()
        ck.ensure_synthetic_checkpoint(path, shape, seed=SEED)
        log(f"[bench] checkpoint {path} ready ({shape.file_size() / 1e6:.0f} MB, {time.time() - t0:.1f} s)")
    n = max(1, args.gpus)
    out = spawn_workers(args, n)
    tokens = out.pop("_tokens")
    parity = None                      # None: not checked (no CPU leg); True/False: tokens compared
    unchecked = False
    if args.full and n == 1 and not args.no_cpu_baseline and not args.stub_engine:
        try:
            cb, match = cpu_baseline(path, args.ctx, first_tok, first_pos, tokens)
            out["cpu_baseline"] = cb
            parity = bool(match)
        except Exception as e:
            # the checker could not run (no gcc/make on the box, oracle build failure, OOM): an infrastructure failure,
            # NOT a token mismatch -- the line says "parity": null + the error, and the exit code is 2 (1 = mismatch):
            # a requested check that did not happen must not look like a pass
            log(f"[bench] PARITY UNCHECKED: cpu_baseline could not run: {e!r}")
            out["cpu_baseline"] = None
            out["cpu_baseline_error"] = repr(e)[:300]
            parity = None
            unchecked = True
        out["parity"] = parity
        if parity is False:
            log("[bench] FATAL: GPU tokens differ from the CPU oracle")
    if args.full and n == 1 and not args.stub_engine and not args.no_graph_stamps and isinstance(out.get("roofline"), dict):
        try:
            roofline_from_graph_stamps(out, args, shape, first_tok, first_pos, path)
        except Exception as e:
            log(f"[bench] graph-mode stamps unavailable, roofline stays on eager HIP events: {e!r}")
            out["roofline"]["graph_mode_error"] = repr(e)[:300]
    fs = out.get("forward_surface")
    if isinstance(fs, dict) and not fs.get("tokens_match_device_loop", True):
        parity = False
        out["parity"] = False
        log("[bench] FATAL: q3_forward host loop and the device-resident loop disagree")
    if args.full and n == 1 and args.shape == "qwen3-0.6b" and not args.no_other_configs and not args.stub_engine:
        out["other_configs"] = other_configs(args)
    print(json.dumps(out), flush=True)
    return 1 if parity is False else (2 if unchecked else 0)


def main():
    args = parse_args()
    if args.worker or "WORLD_SIZE" in os.environ:
        out = worker_main(args)
        if out is not None:
            if not args.worker:          # launched by torchrun: this IS the result line
                out.pop("_tokens", None)
            print(json.dumps(out), flush=True)
        # a gloo group still alive at interpreter exit can abort the process ("terminate called without an active exception")
        dist = sys.modules.get("torch.distributed")
        if dist is not None and dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()
        return 0
    return parent_main(args)


if __name__ == "__main__":
    sys.exit(main())
