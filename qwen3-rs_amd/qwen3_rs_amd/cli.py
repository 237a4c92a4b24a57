"""`qwen3` command line on the MI355X engine: the flags of qwen3-cli/src/main.rs:18-93.

    python -m qwen3_rs_amd.cli export <MODEL_PATH> <OUTPUT_PATH> [--group-size 64]
    python -m qwen3_rs_amd.cli inference <checkpoint> [-t 1.0] [-p 0.9] [-s SEED] [-c CTX] [-m generate|chat]
                                         [-i INPUT] [-y SYSTEM] [-r 0|1] [--lookup DRAFT_LEN] [--speculate DRAFT_LEN]
                                         [-k TOP_K]
    python -m qwen3_rs_amd.cli embed <checkpoint> -i TEXT [-i TEXT ...] [--instruct TEXT] [--dim N] [--no-normalize]
                                     [--append-token ID] [-o out.npy] [--streams N] [--context N]
    python -m qwen3_rs_amd.cli rerank <checkpoint> -q QUERY -d DOC [-d DOC ...] [--instruct TEXT] [--yes TEXT] [--no TEXT]
                                      [--streams N] [-c N] [-o out.npy]
    python -m qwen3_rs_amd.cli score <checkpoint> -i TEXT [-i TEXT ...] [--context TEXT] [--streams N] [--ctx N] [-o out.npy]
                                     [--top K]

`inference` follows generation.rs: `generate` echoes the prompt and decodes from its last token over a zero KV prefix
(:9-48); `chat` renders the template, forwards every prompt token (one rng coin each) and decodes until BOS/EOS
(:50-151).  Forward, sampling (temperature / top-p / xorshift64*) and the prompt loop all run on the device
(q3_prefill, q3_forward_sample); the host only tokenizes, prints and checks for the termination tokens.
`--lookup N` (greedy only, -t 0) decodes through q3_generate_lookup: up to N tokens drafted from the text so far (the latest
earlier occurrence of the last two tokens) are checked in one pass over the weights; the output is the same, byte for byte.
`--speculate N` does the same at any temperature through q3_generate_lookup_draw: a draft is accepted exactly when it is the
token the sampler draws, so the output is again the same, byte for byte.
`-k N` / `--top-k N` (q3_sampler_top_k; 1..64, 0 = off): every draw at -t > 0 is taken among the N most likely tokens; it is a setting
of the engine, so it holds under `--speculate` too.
`embed` reads a checkpoint out as an embedding model (q3_embed_many): every -i text is tokenized, `--append-token ID` adds one
token id to each (Qwen3-Embedding's tokenizer appends its end-of-text token; which id that is in a given .tokenizer is the
user's to state), `--instruct` is tokenized once and becomes the prefix all inputs share.  One line per input: index, dimension,
first 8 components; `-o` saves the matrix.
`rerank` reads a checkpoint out as a reranker (q3_choice_many): one prompt per -d document from the Qwen3-Reranker template
(generation.RERANK_TEMPLATE), the logits of the `--no` and `--yes` tokens behind it, softmax over the two.  One line per document:
index and P(yes); `-o` saves the scores.
`score` says how likely the checkpoint finds every -i text (q3_score_many): log P of each of its tokens given the tokens before it,
the vocabulary-wide sums formed on the device.  With `--context TEXT` every text is a continuation scored behind that context: the
tokens are encode(context) + encode(text), only the text's tokens are scored, and with more than one text the context is computed
once and kept resident as a shared prefix.  One line per text: index, scored tokens, sum of log-probs, perplexity; `-o` saves the
log-probs of all texts, concatenated in order, as one float64 vector.  `--top K` (q3_score_top_many) adds a fifth column, the scored
tokens that are among the model's K most likely ones (rank < K), and `-o` then saves an .npz: `logprobs`, `top_ids` [tokens, K],
`top_logprobs` [tokens, K] and `rank`, concatenated over the texts, and `lengths`, the scored tokens of every text.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

from . import export as export_mod
from .engine import TOP_K_MAX, TransformerBuilder
from .tokenizer import Tokenizer, export_templates, export_tokenizer


def _emit(tok: Tokenizer, token: int):
    sys.stdout.buffer.write(tok.decode_bytes(token))
    sys.stdout.flush()


def _out(raw: bytes):
    """(everything on stdout goes through the byte layer: decoded tokens are raw bytes, and mixing them with the text layer's
    own buffer reorders the output when stdout is a pipe)"""
    sys.stdout.buffer.write(raw)
    sys.stdout.flush()


LOOKUP_NGRAM = 2


def _lookup_round(t, history, pos: int, seq_len: int, lookup: int, stop=None):
    """one round of up to lookup + 1 greedy tokens: history[-1] is forwarded at pos, everything before it is the corpus.
    stop (--speculate): the round is drawn by the device sampler and ends with the first of these tokens, no coin drawn behind it"""
    if stop is not None:
        toks, _ = t.generate_lookup_draw(history[:-1], history[-1], pos, min(lookup + 1, seq_len - pos), ngram=LOOKUP_NGRAM,
                                         draft_len=lookup, stop_tokens=stop)
        return toks
    toks, _ = t.generate_lookup(history[:-1], history[-1], pos, min(lookup + 1, seq_len - pos), ngram=LOOKUP_NGRAM, draft_len=lookup)
    return toks


def run_generate(t, tok: Tokenizer, prompt: str, lookup: int = 0, speculate: bool = False) -> int:
    """generation.rs:9-48"""
    prompt_tokens = tok.encode(prompt or "")
    if not prompt_tokens:
        raise SystemExit("Please provide a prompt")
    seq_len = t.get_config().seq_len
    stop = (tok.bos_token_id, tok.eos_token_id) if speculate else None
    for p in prompt_tokens[:-1][:seq_len]:                 # echoed, never forwarded (zero KV prefix)
        _emit(tok, p)
    token, pos, n_gen, t0 = prompt_tokens[-1], len(prompt_tokens) - 1, 0, None
    history, pending = list(prompt_tokens), []
    while pos < seq_len:
        if t0 is None:
            t0 = time.perf_counter()
        if lookup:                                         # a round of tokens per call, handed out one by one
            if not pending:
                pending = _lookup_round(t, history, pos, seq_len, lookup, stop)
            nxt = pending.pop(0)
            history.append(nxt)
        else:
            nxt = t.forward_argmax(token, pos)             # Sampler::sample on the device when temperature > 0
        n_gen += 1
        if nxt in (tok.bos_token_id, tok.eos_token_id):
            break
        _emit(tok, token)
        token, pos = nxt, pos + 1
    _report(n_gen, t0)
    print()
    return 0


def _report(n_gen: int, t0):
    if t0 is not None and n_gen:
        dt = time.perf_counter() - t0
        print(f"\n[{n_gen / dt:.2f} tk/s, {n_gen} tokens in {dt:.2f}s]", file=sys.stderr)


def _prefill(t, ids, pos) -> int:
    """32 positions per weight pass when the checkpoint's shape allows it, else the sequential device loop; same result."""
    from .engine import Q3Error
    if os.environ.get("Q3_CLI_BATCHED_PREFILL", "1") != "0":
        try:
            return t.prefill(ids, pos, batched=True)
        except Q3Error as err:
            if err.code != -5:
                raise
    return t.prefill(ids, pos)


def run_chat(t, tok: Tokenizer, cli_prompt, system_prompt, lookup: int = 0, speculate: bool = False) -> int:
    """generation.rs:50-151, loop for loop: when the window is exhausted the position goes back to 0 and a user turn begins
    (generation.rs:65-69) -- the KV cache is NOT cleared, rows are simply rewritten from the front, and with a `-i` prompt
    the prompt is fed again exactly as the reference does (get_user_input, generation.rs:174-188)."""
    seq_len = t.get_config().seq_len
    stop = (tok.bos_token_id, tok.eos_token_id) if speculate else None
    pos, user_turn, nxt = 0, True, 0
    n_gen, t0 = 0, None
    history, pending = [], []                              # --lookup: the window's tokens so far, tokens of the current round
    while True:
        if pos >= seq_len:                                 # "Reset context if window exceeded"
            pos, user_turn = 0, True
            history, pending = [], []
            _out(b"\n")
        if user_turn:
            _report(n_gen, t0)
            n_gen, t0 = 0, None
            if pos == 0 and cli_prompt is not None:
                user = cli_prompt
            elif cli_prompt is not None:
                user = ""
            else:
                _out(b"> ")
                user = sys.stdin.readline().strip()
            if not user and not (pos == 0 and cli_prompt is not None):
                break
            ids = tok.encode(tok.render_prompt(pos, system_prompt, user))[: max(seq_len - pos, 0)]
            if ids:
                nxt = _prefill(t, ids, pos)
                pos += len(ids)
                history, pending = history + ids + [nxt], []
            user_turn = False
        else:
            if nxt in (tok.bos_token_id, tok.eos_token_id):
                _report(n_gen, t0)
                n_gen, t0 = 0, None
                _out(b"\n")
                user_turn = True
                continue
            if t0 is None:
                t0 = time.perf_counter()
            _emit(tok, nxt)
            if lookup and history:
                if not pending:                            # (rows a round writes past a turn's end are rewritten before they are read)
                    pending = _lookup_round(t, history, pos, seq_len, lookup, stop)
                nxt = pending.pop(0)
                history.append(nxt)
            else:
                nxt = t.forward_argmax(nxt, pos)
            n_gen += 1
            pos += 1
    return 0


def run_embed(a) -> int:
    import numpy as np
    from .generation import embed
    b = TransformerBuilder(a.checkpoint)
    if a.context:
        b = b.with_ctx_length(a.context)
    with b.build() as t:
        tok = Tokenizer(a.checkpoint, t.get_config().vocab_size, False)
        tail = [] if a.append_token is None else [a.append_token]
        prompts = [tok.encode(text) + tail for text in a.input]
        if any(not p for p in prompts):
            print("Error: an input has no token", file=sys.stderr)
            return 1
        prefix = tok.encode(a.instruct) if a.instruct else []
        t.batch_init(max(1, min(a.streams, 32, len(prompts))))
        rows = embed(t, prompts, normalize=not a.no_normalize, out_dim=a.dim, shared_prefix=prefix or None)
    for r, row in enumerate(rows):
        print(r, row.size, " ".join(f"{v:.6f}" for v in row[:8]))
    if a.output:
        np.save(a.output, rows)
    return 0


def run_rerank(a) -> int:
    import numpy as np
    from .generation import rerank
    b = TransformerBuilder(a.checkpoint)
    if a.context:
        b = b.with_ctx_length(a.context)
    with b.build() as t:
        tok = Tokenizer(a.checkpoint, t.get_config().vocab_size, False)
        t.batch_init(max(1, min(a.streams, 32, len(a.document))))
        scores = rerank(t, tok, a.query, a.document, instruction=a.instruct, yes=a.yes, no=a.no)
    for r, v in enumerate(scores):
        print(r, f"{v:.6f}")
    if a.output:
        np.save(a.output, scores)
    return 0


def score_requests(ctx, texts):
    """What `score` hands to generation.score for the context's tokens and the texts' tokens: (prompts, score_from, shared_prefix).
    Behind a context every token of a text is a target, the first one predicted from the context's last token: that token leads
    every prompt when the rest of the context is resident as the prefix (the first token behind a prefix is never a target)."""
    if not ctx:
        return [list(x) for x in texts], None, None
    if len(texts) > 1 and len(ctx) > 1:
        return [[ctx[-1]] + list(x) for x in texts], [1] * len(texts), list(ctx[:-1])
    return [list(ctx) + list(x) for x in texts], [len(ctx)] * len(texts), None


def run_score(a) -> int:
    import numpy as np
    from .generation import perplexity, score, top_logprobs
    if a.top is not None and not 1 <= a.top <= 64:
        print("Error: --top takes 1..64", file=sys.stderr)
        return 1
    b = TransformerBuilder(a.checkpoint)
    if a.ctx:
        b = b.with_ctx_length(a.ctx)
    with b.build() as t:
        tok = Tokenizer(a.checkpoint, t.get_config().vocab_size, False)
        texts = [tok.encode(text) for text in a.input]
        if any(not x for x in texts):
            print("Error: an input has no token", file=sys.stderr)
            return 1
        prompts, score_from, prefix = score_requests(tok.encode(a.context) if a.context else [], texts)
        t.batch_init(max(1, min(a.streams, 32, len(prompts))))
        if a.top is None:
            lps = score(t, prompts, score_from, shared_prefix=prefix)
        else:
            res = top_logprobs(t, prompts, a.top, score_from, shared_prefix=prefix)
            lps = [x[0] for x in res]
    for r, lp in enumerate(lps):
        print(r, lp.size, f"{lp.sum():.6f}", f"{perplexity([lp]):.6f}", *([] if a.top is None else [int((res[r][3] < a.top).sum())]))
    if a.output and a.top is None:
        np.save(a.output, np.concatenate(lps) if lps else np.zeros(0))
    elif a.output:
        with open(a.output, "wb") as f:         # the name as given: np.savez would append .npz to a path
            np.savez(f, logprobs=np.concatenate(lps), top_ids=np.concatenate([x[1] for x in res]), top_logprobs=np.concatenate([x[2] for x in res]),
                     rank=np.concatenate([x[3] for x in res]), lengths=np.array([lp.size for lp in lps], dtype=np.int64))
    return 0


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="qwen3", description="Qwen3 CLI on the MI355X engine: export and inference")
    sub = ap.add_subparsers(dest="cmd")
    ex = sub.add_parser("export", help="Export a HuggingFace Qwen3 directory to the Q8 checkpoint (+ .tokenizer)")
    ex.add_argument("MODEL_PATH")
    ex.add_argument("OUTPUT_PATH")
    ex.add_argument("--group-size", "-g", type=int, default=64)
    inf = sub.add_parser("inference", help="Qwen3 inference")
    inf.add_argument("checkpoint")
    inf.add_argument("-t", "--temperature", type=float, default=1.0)
    inf.add_argument("-p", "--topp", type=float, default=0.9)
    inf.add_argument("-k", "--top-k", type=int, default=0, metavar="TOP_K",
                     help="draw among the TOP_K most likely tokens only (1..64; 0 = off, the default)")
    inf.add_argument("-s", "--seed", type=int, default=None)
    inf.add_argument("-c", "--context", type=int, default=None)
    inf.add_argument("-m", "--mode", default="chat")
    inf.add_argument("-i", "--input", default=None)
    inf.add_argument("-y", "--system", default=None)
    inf.add_argument("-r", "--reasoning", type=int, default=0)
    inf.add_argument("--lookup", type=int, default=0, metavar="DRAFT_LEN",
                     help="greedy only (-t 0): draft up to DRAFT_LEN (1..31) tokens per weight pass by prompt lookup; 0 = off")
    inf.add_argument("--speculate", type=int, default=0, metavar="DRAFT_LEN",
                     help="any -t: the same drafts, each accepted exactly when it is the token the sampler draws; same output; 0 = off")
    em = sub.add_parser("embed", help="Last-token embeddings of texts (a Qwen3-Embedding checkpoint)")
    em.add_argument("checkpoint")
    em.add_argument("-i", "--input", action="append", required=True, metavar="TEXT", help="a text to embed; repeat for more")
    em.add_argument("--instruct", default=None, metavar="TEXT", help="tokenized once: the prefix every input shares")
    em.add_argument("--dim", type=int, default=None, metavar="N", help="keep the first N components (default: all)")
    em.add_argument("--no-normalize", action="store_true", help="no L2 normalisation")
    em.add_argument("--append-token", type=int, default=None, metavar="ID", help="a token id added behind every input")
    em.add_argument("-o", "--output", default=None, metavar="out.npy", help="save the matrix [inputs, dim]")
    em.add_argument("--streams", type=int, default=8, metavar="N", help="slots of the batched state (1..32)")
    em.add_argument("-c", "--context", type=int, default=None)
    rr = sub.add_parser("rerank", help="P(yes) of documents for a query (a Qwen3-Reranker checkpoint)")
    rr.add_argument("checkpoint")
    rr.add_argument("-q", "--query", required=True, metavar="QUERY")
    rr.add_argument("-d", "--document", action="append", required=True, metavar="DOC", help="a document to score; repeat for more")
    rr.add_argument("--instruct", default=None, metavar="TEXT", help="the task instruction (default: the model card's web-search one)")
    rr.add_argument("--yes", default="yes", metavar="TEXT", help="the answer word that counts as relevant: one token")
    rr.add_argument("--no", default="no", metavar="TEXT", help="the other answer word: one token")
    rr.add_argument("--streams", type=int, default=8, metavar="N", help="slots of the batched state (1..32)")
    rr.add_argument("-c", "--context", type=int, default=None)
    rr.add_argument("-o", "--output", default=None, metavar="out.npy", help="save the scores [documents]")
    sc = sub.add_parser("score", help="log-probabilities and perplexity of texts")
    sc.add_argument("checkpoint")
    sc.add_argument("-i", "--input", action="append", required=True, metavar="TEXT", help="a text to score; repeat for more")
    sc.add_argument("--context", default=None, metavar="TEXT", help="every text is a continuation scored behind this context")
    sc.add_argument("--streams", type=int, default=8, metavar="N", help="slots of the batched state (1..32)")
    sc.add_argument("--ctx", type=int, default=None, metavar="N", help="context length of the engine")
    sc.add_argument("-o", "--output", default=None, metavar="out.npy", help="save the log-probs of all texts, concatenated (with --top: an .npz)")
    sc.add_argument("--top", type=int, default=None, metavar="K", help="also the K most likely tokens of every position and the targets' ranks (1..64)")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.cmd == "export":
        if not os.path.isdir(a.MODEL_PATH):
            print(f"Error: Model directory does not exist: {a.MODEL_PATH}", file=sys.stderr)
            return 1
        try:
            info = export_mod.load_model_info(a.MODEL_PATH)
            shape = export_mod.export_model(a.MODEL_PATH, a.OUTPUT_PATH, a.group_size, log=lambda m: print(m, file=sys.stderr))
            if os.path.exists(os.path.join(a.MODEL_PATH, "tokenizer.json")):
                print("wrote", export_tokenizer(a.MODEL_PATH, a.OUTPUT_PATH, info.bos_token_id, info.eos_token_id), file=sys.stderr)
            else:
                print("tokenizer.json not found: no .tokenizer written", file=sys.stderr)
            try:
                for path in export_templates(a.MODEL_PATH, a.OUTPUT_PATH):
                    print("wrote", path, file=sys.stderr)
            except ValueError as err:
                print(f"no prompt templates written: {err}", file=sys.stderr)
        except (export_mod.ExportError, ValueError, OSError) as err:
            print(f"Error: {err}", file=sys.stderr)
            return 1
        print(f"wrote {a.OUTPUT_PATH}: {shape}")
        return 0
    if a.cmd == "inference":
        if a.mode not in ("generate", "chat"):
            print(f"Error: Unknown mode: {a.mode}", file=sys.stderr)
            return 1
        if a.lookup and (a.temperature > 0.0 or not 0 < a.lookup < 32):
            print("Error: --lookup takes a draft length of 1..31 and needs -t 0: speculative decoding is greedy only "
                  "(speculative sampling is not implemented)", file=sys.stderr)
            return 1
        if a.speculate and (a.lookup or not 0 < a.speculate < 32):
            print("Error: --speculate takes a draft length of 1..31 and cannot be combined with --lookup", file=sys.stderr)
            return 1
        top_k_refusal = "Error: --top-k takes 0 (off) or a count of 1..64, at most the vocabulary size"
        if not 0 <= a.top_k <= TOP_K_MAX:
            print(top_k_refusal, file=sys.stderr)
            return 1
        b = TransformerBuilder(a.checkpoint)
        if a.context:
            b = b.with_ctx_length(a.context)
        with b.build() as t:
            tok = Tokenizer(a.checkpoint, t.get_config().vocab_size, a.reasoning != 0)
            seed = a.seed if a.seed is not None else int(time.time())      # lib.rs: SystemTime seconds when no seed is given
            t.set_sampler(max(a.temperature, 0.0), min(max(a.topp, 0.0), 1.0), seed)
            if a.top_k > t.get_config().vocab_size:
                print(top_k_refusal, file=sys.stderr)
                return 1
            t.set_top_k(a.top_k)                # the engine's: --speculate's rounds draw under it too
            if a.mode == "generate":
                return run_generate(t, tok, a.input, a.lookup or a.speculate, bool(a.speculate))
            return run_chat(t, tok, a.input, a.system, a.lookup or a.speculate, bool(a.speculate))
    if a.cmd == "embed":
        from .engine import Q3Error
        try:
            return run_embed(a)
        except (Q3Error, IndexError, ValueError) as err:
            print(f"Error: {err}", file=sys.stderr)
            return 1
    if a.cmd == "rerank":
        from .engine import Q3Error
        try:
            return run_rerank(a)
        except (Q3Error, IndexError, ValueError) as err:
            print(f"Error: {err}", file=sys.stderr)
            return 1
    if a.cmd == "score":
        from .engine import Q3Error
        try:
            return run_score(a)
        except (Q3Error, IndexError, ValueError) as err:
            print(f"Error: {err}", file=sys.stderr)
            return 1
    ap.print_help()
    return 1


if __name__ == "__main__":
    sys.exit(main())
