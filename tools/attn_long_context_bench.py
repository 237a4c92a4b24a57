"""The figures of profiles/attn_long_context.md: batched decode at context 8,192 on k_attn_streams (Q3_BATCH_ATT_GQA2G=0, developer
library) against k_attn_gqa2g, two engines of one process by turns, and column passes of 1, 8 and 32 columns on the product library."""
import dataclasses
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-rs_amd"))
import numpy as np
import qwen3_rs_amd as q3

CTX, POS, STREAMS, STEPS, RUNS = 8192, 8000, 32, 64, 5


def bmw(xs):
    return f"{min(xs) * 1e3:.3f} / {statistics.median(xs) * 1e3:.3f} / {max(xs) * 1e3:.3f} ms"


def timed(fn):
    t0 = time.perf_counter()
    fn()                                   # every call below ends in a device synchronise
    return time.perf_counter() - t0


def main():
    tmp = tempfile.mkdtemp()
    for name in ("qwen3-8b-dims-l2", "qwen3-32b-dims-l2"):
        shape = dataclasses.replace(q3.checkpoint.SHAPES[name], max_seq_len=CTX)
        path = os.path.join(tmp, name + ".bin")
        q3.checkpoint.write_synthetic_checkpoint(path, shape, seed=77)
        print(f"== {name} at context {CTX}: {shape.n_heads} / {shape.n_kv_heads} heads", flush=True)
        toks, pos = [(7 * i + 3) % shape.vocab_size for i in range(STREAMS)], [POS] * STREAMS
        with q3.use_library(q3.dev_lib_path()):
            eng = {}
            for knob in ("0", "1"):
                os.environ["Q3_BATCH_ATT_GQA2G"] = knob
                t = q3.TransformerBuilder(path).with_ctx_length(CTX).build()
                t.batch_init(STREAMS)
                eng[knob] = (t, t.generate_greedy_batch(toks, pos, STEPS))      # warm-up: the plan is built under this setting
                if knob == "0":
                    try:
                        t.batch_step_cols([0], [1], [POS])
                        print("knob 0: a column pass was NOT refused")
                    except q3.Q3Error as ex:
                        print("knob 0: column pass refused:", str(ex)[:90])
            del os.environ["Q3_BATCH_ATT_GQA2G"]
            print("same tokens:", bool(np.array_equal(eng["0"][1], eng["1"][1])))
            times = {"0": [], "1": []}
            for _ in range(RUNS):
                for knob in ("0", "1"):
                    times[knob].append(timed(lambda: eng[knob][0].generate_greedy_batch(toks, pos, STEPS)))
            for knob, label in (("0", "k_attn_streams"), ("1", "k_attn_gqa2g")):
                print(f"decode {STREAMS} streams x {STEPS} steps from {POS}, {label}: {bmw(times[knob])}; per step (best) {min(times[knob]) / STEPS * 1e3:.3f} ms")
            print(f"ratio of the best: {min(times['0']) / min(times['1']):.2f}", flush=True)
            for t, _ in eng.values():
                t.close()
        with q3.TransformerBuilder(path).with_ctx_length(CTX).build() as t:     # product library
            t.batch_init(STREAMS)
            for n in (1, 8, 32):
                slots, tk, ps = list(range(n)), toks[:n], [POS] * n
                t.batch_step_cols(slots, tk, ps)
                xs = [timed(lambda: [t.batch_step_cols(slots, tk, ps) for _ in range(20)]) / 20 for _ in range(RUNS)]
                print(f"column pass, {n} columns at {POS}: {bmw(xs)} per pass", flush=True)


if __name__ == "__main__":
    main()
