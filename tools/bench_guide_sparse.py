#!/usr/bin/env python3
"""What a sparse guide (include/qwen3_hip.h section 2s) costs inside generate_many against the dense form of the same automaton, and
what the regular-expression compiler costs on the host.

    python tools/bench_guide_sparse.py [--models qwen3-0.6b,qwen3-8b] [--ab PARENT_TREE [--ab-models qwen3-0.6b]] [--out profiles]
    python tools/bench_guide_sparse.py --host-only          (no GPU: the host part alone, kept beside what the file already holds)

The workload and the method are tools/bench_guide.py's: 64 requests of 16-token prompts and 32 new tokens on 32 slots; greedy and
sampled, each with top_k 0 and 20; all forms of a configuration in ONE process by turns, medians of the rounds behind a warm-up
round, min .. max beside them, and a call of one new token in front of every timed call so that a new guide's upload is not in the
figure.  The forms: no guide; the trie of 64 four-token labels dense and sparse; the two-state guide that allows every token dense
and sparse; and one sparse state whose default is allowed with V / 2 forbidding edges, the largest edge list a state can need.
The per-pass cost is (on - off) / passes; the byte model beside it, per emitting column at 5.5 TB/s: 10 V for a dense form, 8 V +
8 E_s for a sparse one (E_s: the edges of the state: at most 4 in the trie, 0 where all is allowed, V / 2 in the last form).
The yardstick of a sparse form is the dense form of the same automaton in the same process, the margin the spread of off.
Beside it: the table bytes of both forms of the trie and what setting and uploading each costs (a set and a one-token call, less a
one-token call under a guide the device holds).
The host part: SparseAutomaton.from_regex for three patterns over a synthetic vocabulary of 151,936 tokens (256 single bytes, then
pseudo-random ASCII and UTF-8 strings of 2 to 12 bytes: no tokenizer file is needed) against Automaton.from_byte_dfa on the same DFA.
--ab PARENT_TREE: the call with no guide of this tree against the build of another checkout, as in bench_guide.py.
Writes <out>/guide_sparse.md and guide_sparse.json."""
import argparse
import json
import os
import sys
import time

import bench_bias as bb
from bench_bias import CONFIGS, N_NEW, N_PROMPT, N_REQ, ROOT, SLOTS, STREAM_TBS, CTX, T, TOPP, TAG

FORMS = ["off", "trie dense", "trie sparse", "all allowed dense", "all allowed sparse", "half forbidden sparse"]
PAIRS = [("trie sparse", "trie dense"), ("all allowed sparse", "all allowed dense")]
HOST_VOCAB = 151936
PATTERNS = [r"\d{4}-\d{2}-\d{2}", r"[A-Za-z_]\w{0,15}", r"-?\d+(\.\d+)? ?(mm|cm|m|km)"]


def forms(q3, vocab):
    """form -> ("dense", next, start) | ("sparse", default, offsets, tokens, targets, start) | None, and form -> bytes per emitting column"""
    import numpy as np
    SA = q3.guide.SparseAutomaton
    free = np.zeros((2, vocab), dtype=np.int16)
    free[0] = 1
    labels = [[(104729 * r + 7919 * i + 13) % (vocab - 1) + 1 for i in range(4)] for r in range(N_REQ)]     # eos is token 0
    trie = q3.guide.Automaton.from_sequences(labels, vocab, eos=0)
    strie = SA.from_sequences(labels, vocab, eos=0)
    sfree = SA.from_dense(q3.guide.Automaton(free, 0))
    odd = np.arange(1, vocab, 2, dtype=np.int32)
    half = SA([0], [0, odd.size], odd, np.full(odd.size, -1, dtype=np.int32), 0, vocab)
    sp = lambda a, start: ("sparse", a.default, a.offsets, a.tokens, a.targets, start)
    got = {"off": None, "trie dense": ("dense", trie.next, [0] * N_REQ), "trie sparse": sp(strie, [0] * N_REQ),
           "all allowed dense": ("dense", free, [0]), "all allowed sparse": sp(sfree, [0]), "half forbidden sparse": sp(half, [0])}
    model = {"trie dense": 10.0 * vocab, "trie sparse": 8.0 * vocab + 8.0 * 4, "all allowed dense": 10.0 * vocab, "all allowed sparse": 8.0 * vocab,
             "half forbidden sparse": 8.0 * vocab + 8.0 * odd.size}
    sizes = {"trie dense": int(trie.next.nbytes), "trie sparse": int(4 * strie.n_states + 4 * (strie.n_states + 1) + 8 * strie.n_edges),
             "states": int(trie.n_states), "edges": int(strie.n_edges)}
    return got, model, sizes


def set_form(t, form):
    if form is None:
        t.set_guide(None, [])
    elif form[0] == "dense":
        t.set_guide(*form[1:])
    else:
        t.set_guide_sparse(*form[1:])


def worker(name, ckpt_dir, seed, rounds):
    import qwen3_rs_amd as q3
    path = bb.checkpoint(q3, name, ckpt_dir, seed)
    vocab = q3.checkpoint.SHAPES[name].vocab_size
    prompts, n_new, seeds = bb.requests(vocab)
    fm, model, sizes = forms(q3, vocab)
    res = {"model": name, "rounds": rounds, "vocab": vocab, "configs": {}, "bytes": model, "table": sizes}
    with q3.TransformerBuilder(path).with_ctx_length(1024).build() as t:
        t.batch_init(SLOTS, CTX)
        for mode, top_k in CONFIGS:
            info = {}

            def form(guide):
                def f():
                    t.set_top_k(top_k)
                    set_form(t, guide)
                    bb.generate(t, mode, prompts, [1] * N_REQ, seeds)      # untimed: a new guide goes to the device here
                    out = []
                    s = bb.timed(lambda: out.append(bb.generate(t, mode, prompts, n_new, seeds)))
                    info["passes"], info["emitting"] = out[0][1].passes, sum(len(r) for r in out[0][0])
                    t.set_guide(None, [])
                    return s
                return f
            got = bb.by_turns({k: form(fm[k]) for k in FORMS}, rounds)
            res["configs"][f"{mode}, top_k {top_k}"] = dict(info, ms={k: bb.stat(v) for k, v in got.items()})
        # setting and uploading the trie: a set and a one-token call, less a one-token call under a guide the device holds
        t.set_top_k(0)
        one = lambda: bb.generate(t, "greedy", prompts, [1] * N_REQ, seeds)
        up = {}
        for k in ("trie dense", "trie sparse"):
            def fresh():
                t.set_guide(None, [])
                one()
                return bb.timed(lambda: (set_form(t, fm[k]), one()))
            held = lambda: bb.timed(one)
            got = bb.by_turns({"set + upload + call": fresh, "call": held}, rounds)
            up[k] = {n: bb.stat(v) for n, v in got.items()}
        t.set_guide(None, [])
        res["upload_ms"] = up
    print(TAG + json.dumps(res), flush=True)


def synthetic_vocab(n=HOST_VOCAB, seed=5):
    import numpy as np
    rng = np.random.default_rng(seed)
    vocab = [bytes([b]) for b in range(256)]
    ascii_pool = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 _-.,:;/(){}[]\"'\n", dtype=np.uint8)
    wide = ["é", "ü", "ß", "日", "本", "語", "—", "😀", "λ", "ж"]
    while len(vocab) < n - 1:
        k = int(rng.integers(2, 13))
        if rng.random() < 0.9:
            vocab.append(bytes(ascii_pool[rng.integers(0, ascii_pool.size, k)]))
        else:
            vocab.append("".join(wide[int(i)] for i in rng.integers(0, len(wide), max(1, k // 3))).encode())
    vocab.append(b"<eos>")
    return vocab


def host(dense_limit):
    """from_regex against Automaton.from_byte_dfa on the same DFA, seconds; the dense builder only where its table fits dense_limit states"""
    sys.path.insert(0, os.path.join(ROOT, "qwen3-rs_amd"))
    import numpy as np
    from qwen3_rs_amd import guide
    vocab = synthetic_vocab()
    eos = len(vocab) - 1
    rows = []
    for p in PATTERNS:
        t0 = time.perf_counter()
        dfa = guide.regex_dfa(p)
        t1 = time.perf_counter()
        sp = guide.SparseAutomaton.from_byte_dfa(*dfa, vocab, eos)
        t2 = time.perf_counter()
        row = {"pattern": p, "byte_states": int(dfa[0].shape[0]), "token_states": sp.n_states, "edges": sp.n_edges, "regex_dfa_s": t1 - t0, "sparse_lift_s": t2 - t1,
               "sparse_bytes": int(4 * sp.n_states + 4 * (sp.n_states + 1) + 8 * sp.n_edges), "dense_bytes": 2 * sp.n_states * len(vocab)}
        if sp.n_states <= dense_limit:
            t3 = time.perf_counter()
            dn = guide.Automaton.from_byte_dfa(*dfa, vocab, eos)
            row["dense_lift_s"] = time.perf_counter() - t3
            row["same_table"] = bool(all(np.array_equal(sp.row(s), dn.next[s]) for s in range(sp.n_states)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return {"vocab": len(vocab), "patterns": rows}


def write_md(data, out):
    fmt = bb.fmt
    results, ab, hostd = data.get("results", []), data.get("ab", {}), data.get("host")
    md = ["# Sparse guides against dense ones inside generate_many (`tools/bench_guide_sparse.py`)", "",
          f"{N_REQ} requests of {N_PROMPT}-token prompts and {N_NEW} new tokens on {SLOTS} slots, synthetic checkpoints; sampled: temperature {T}, top-p {TOPP}.",
          "Every table was measured in one process, its forms by turns; a cell is the median over the rounds in ms per call with (min .. max)",
          "beside it.  off: no guide; trie: 64 four-token labels, a start state per request; all allowed: a two-state guide that allows every",
          "token; half forbidden: one sparse state, default allowed, every odd token a forbidding edge (E_s = V / 2).  Every form is set in front",
          "of its call and a call of one new token runs before the timed one, so the copy and the upload are not in these figures.", ""]
    for r in results:
        md += [f"## {r['model']} ({r['rounds']} rounds)", "", "| configuration | passes | " + " | ".join(FORMS) + " |", "|---|---|" + "---|" * len(FORMS)]
        for cfg, c in r["configs"].items():
            md.append(f"| {cfg} | {c['passes']} | " + " | ".join(fmt(c["ms"][k]) for k in FORMS) + " |")
        md += ["", f"Per-pass cost, us: (on - off) / passes, medians, with measured / model beside it; the model per emitting column at {STREAM_TBS} TB/s is 10 V bytes",
               "for a dense form and 8 V + 8 E_s for a sparse one.  A sparse form is held against the dense form of the same automaton plus the spread",
               "of off in the same run.", "",
               "| configuration | " + " | ".join(FORMS[1:]) + " | spread of off per pass | emitting columns per pass | " +
               " | ".join(f"{s} within {d} + spread" for s, d in PAIRS) + " |", "|---|" + "---|" * (len(FORMS) + 1 + len(PAIRS))]
        for cfg, c in r["configs"].items():
            m, p = c["ms"], max(1, c["passes"])
            cols = c["emitting"] / p
            model = lambda k: r["bytes"][k] * cols / (STREAM_TBS * 1e12) * 1e6
            cost = {k: 1e3 * (m[k]["median"] - m["off"]["median"]) / p for k in FORMS[1:]}
            spread = 1e3 * (m["off"]["max"] - m["off"]["min"]) / p
            held = [f"{'yes' if cost[s] <= cost[d] + spread else 'NO'} ({cost[s]:+.1f} vs {cost[d] + spread:+.1f})" for s, d in PAIRS]
            md.append(f"| {cfg} | " + " | ".join(f"{cost[k]:+.1f} ({cost[k] / model(k):.1f} x of {model(k):.1f})" for k in FORMS[1:]) +
                      f" | {spread:.1f} | {cols:.1f} | " + " | ".join(held) + " |")
        tb, up = r["table"], r["upload_ms"]
        md += ["", f"The trie: {tb['states']} states, {tb['edges']} edges; {tb['trie dense'] / 1e6:.1f} MB dense, {tb['trie sparse'] / 1e3:.1f} KB sparse.  Setting it and the",
               "first call under it (the host copy, the checks, the upload, a call of one new token) against that call under a guide the device holds, ms:", "",
               "| form | set + upload + call | call | difference of the medians |", "|---|---|---|---|"]
        for k in ("trie dense", "trie sparse"):
            a, b = up[k]["set + upload + call"], up[k]["call"]
            md.append(f"| {k} | {fmt(a)} | {fmt(b)} | {a['median'] - b['median']:+.1f} |")
        md.append("")
    for name, rounds in ab.items():
        md += [f"## The call with no guide against the parent: {name}", "",
               "A child process per measurement, the parent's package and library and this tree's by turns, three each; ms per call, median (min .. max)",
               "over all rounds of a tree's children.", "", "| configuration | parent | this tree | this tree's median inside the parent's min .. max |", "|---|---|---|---|"]
        for cfg in rounds[0][1]:
            p, h = bb.pooled(rounds, "parent", cfg), bb.pooled(rounds, "this tree", cfg)
            ok = p["min"] <= h["median"] <= p["max"]
            md.append(f"| {cfg} | {fmt(p)} | {fmt(h)} | {'yes' if ok else ('NO: below' if h['median'] < p['min'] else 'NO: above')} |")
        md.append("")
    if not ab:
        md += ["## The off path", "", "Not measured against a parent tree by this tool (`--ab` was not given).", ""]
    if hostd:
        md += ["## The compiler on the host", "",
               f"`SparseAutomaton.from_regex` = `regex_dfa` + the vectorised lift, against `Automaton.from_byte_dfa` (a Python loop over the tokens per state) on the",
               f"same DFA, over a synthetic vocabulary of {hostd['vocab']} tokens (256 single bytes, then pseudo-random ASCII and UTF-8 strings of 2 to 12 bytes; no",
               "tokenizer file was on disk), one run each, seconds, on the CPU of the machine that wrote this file.", "",
               "| pattern | byte states | token states | edges | regex_dfa | sparse lift | dense lift | the same table | sparse bytes | dense bytes |", "|---|---|---|---|---|---|---|---|---|---|"]
        for h in hostd["patterns"]:
            dense = f"{h['dense_lift_s']:.1f}" if "dense_lift_s" in h else "not run"
            md.append(f"| `{h['pattern']}` | {h['byte_states']} | {h['token_states']} | {h['edges']} | {h['regex_dfa_s']:.3f} | {h['sparse_lift_s']:.2f} | {dense} | "
                      f"{h.get('same_table', '-')} | {h['sparse_bytes'] / 1e3:.0f} KB | {h['dense_bytes'] / 1e6:.1f} MB |")
        md.append("")
    with open(os.path.join(out, "guide_sparse.md"), "w") as f:
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
    ap.add_argument("--host-only", action="store_true", help="the host part alone; needs no GPU")
    ap.add_argument("--no-host", action="store_true", help="leave the host part of the file as it is")
    ap.add_argument("--dense-limit", type=int, default=64, help="run the dense builder only up to this many token states")
    ap.add_argument("--worker")
    ap.add_argument("--worker-ab")
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.ckpt_dir, a.seed, a.rounds)
        return 0
    if a.worker_ab:
        bb.worker_ab(a.worker_ab, a.ckpt_dir, a.seed, a.rounds)      # the call with no table is the call with no guide
        return 0
    os.makedirs(a.out, exist_ok=True)
    file = os.path.join(a.out, "guide_sparse.json")
    data = json.load(open(file)) if os.path.exists(file) else {}

    def save():                 # what is measured so far stands on disk before the next child starts
        with open(file, "w") as f:
            json.dump(data, f, indent=1)
        write_md(data, a.out)
    if not a.no_host:
        data["host"] = host(a.dense_limit)
        save()
    if a.host_only:
        return 0
    base = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--ckpt-dir", a.ckpt_dir, "--seed", str(a.seed),
            "--rounds", str(a.rounds)]
    data["results"], data["ab"], rc = [], {}, 0
    for name in a.models.split(","):
        got = bb.run_child(base + ["--worker", name])
        if got is None:
            rc = 1
            break
        data["results"].append(got)
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
            data["ab"][name] = rounds
        save()
    if not data["results"]:
        return 1
    print(json.dumps({"models": [r["model"] for r in data["results"]], "out": a.out}))
    return rc


if __name__ == "__main__":
    sys.exit(main())
