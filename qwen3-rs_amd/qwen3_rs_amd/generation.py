"""The call patterns that reach `forward` (qwen3-inference/src/generation.rs) and the tok/s definition.

Token ids in, token ids out: tokenizer encode/decode (tokenizer.rs) is outside the hot path.  Works with
any object exposing forward(token,pos)->logits and get_config() -- the HIP Transformer or the test oracle.
"""
from __future__ import annotations

import time
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .engine import SCORE_DTYPE, TOP_DTYPE, BIAS_ADD, BIAS_ALLOW
from .guide import Automaton, SparseAutomaton, merge_guides
from .stops import compile_stop, first_match


def sample_argmax(logits: np.ndarray) -> int:
    """Sampler::sample_argmax (sampler.rs:57-59): Iterator::max_by(total_cmp) keeps the LAST maximum."""
    bits = np.ascontiguousarray(logits, dtype=np.float32).view(np.int32).astype(np.int64)
    key = np.where(bits < 0, bits ^ 0x7FFFFFFF, bits)
    if key.size == 0:
        return 0
    return int(np.nonzero(key == key.max())[0][-1])


class TokenMetrics:
    """generation.rs:198-233: clock starts before the first generated token's forward, count++ per sample."""

    def __init__(self):
        self.start_time: Optional[float] = None
        self.generated_count = 0
        self.elapsed = 0.0

    def start_generation(self):
        if self.start_time is None:
            self.start_time = time.perf_counter()

    def increment_token(self):
        self.generated_count += 1

    def report(self) -> Tuple[int, float, float]:
        if self.start_time is not None:
            self.elapsed = time.perf_counter() - self.start_time
        tps = self.generated_count / self.elapsed if self.elapsed > 0 else 0.0
        return self.generated_count, self.elapsed, tps


def _lookup_decode(transformer, history: List[int], pos: int, budget: int, stop, lookup, metrics, out: List[int], stop_first: bool,
                   draw: bool = False):
    """The greedy decode of both call patterns through Transformer.generate_lookup (q3_generate_lookup) with everything seen so
    far as the corpus: rounds of draft_len + 1 tokens, so a caller sees tokens pass by pass.  history[-1] is the token to forward
    at pos.  stop_first: chat's order (a stop token ends the turn before it is output); else generate's (it is output, then ends).
    draw: the device sampler's decode at any temperature through Transformer.generate_lookup_draw (speculate=).
    Returns the next position."""
    ngram, draft_len = lookup
    while budget > 0:
        if stop_first and history[-1] in stop:
            break
        n = min(budget, draft_len + 1)
        metrics.start_generation()
        if draw:
            toks, _ = transformer.generate_lookup_draw(history[:-1], history[-1], pos, n, ngram=ngram, draft_len=draft_len, stop_tokens=stop)
        else:
            toks, _ = transformer.generate_lookup(history[:-1], history[-1], pos, n, ngram=ngram, draft_len=draft_len)
        for i, nxt in enumerate(toks):
            if stop_first:
                out.append(history[-1])
            else:
                out.append(nxt)
            metrics.increment_token()
            history.append(nxt)
            pos += 1
            budget -= 1
            if nxt in stop:                          # rows the round wrote past this point are rewritten before they are read
                return pos
    return pos


def _check_lookup(lookup, sample, on_logits):
    if sample is not sample_argmax or on_logits is not None:
        raise ValueError("lookup= is greedy decoding on the device: no sample= / on_logits= (speculative sampling is not implemented)")
    ngram, draft_len = lookup
    if ngram < 1 or not 0 < draft_len < 32:
        raise ValueError("lookup=(ngram >= 1, 0 < draft_len < 32)")


def _check_speculate(speculate, lookup, sample, on_logits):
    if lookup is not None or sample is not sample_argmax or on_logits is not None:
        raise ValueError("speculate= decodes with the device sampler (Transformer.set_sampler): no lookup= / sample= / on_logits=")
    ngram, draft_len = speculate
    if ngram < 1 or not 0 < draft_len < 32:
        raise ValueError("speculate=(ngram >= 1, 0 < draft_len < 32)")


def _check_top_k(transformer, sample):
    """Top-k is a setting of the engine's sampler (Transformer.set_top_k): a host sample= callback draws from the whole
    vocabulary and would ignore it without a word."""
    if sample is not sample_argmax and getattr(transformer, "top_k", 0):
        raise ValueError("Transformer.set_top_k holds for the draws of the device sampler: no sample= callback with it "
                         "(draw on the device, speculate=, or set_top_k(0))")


def generate(transformer, prompt_tokens: Sequence[int], max_new_tokens: Optional[int] = None,
             stop_tokens: Iterable[int] = (), sample: Callable[[np.ndarray], int] = sample_argmax,
             on_logits: Optional[Callable[[int, int, np.ndarray], None]] = None, lookup: Optional[Tuple[int, int]] = None,
             speculate: Optional[Tuple[int, int]] = None):
    """`generate` (generation.rs:9-48).  Prompt tokens 0..n-2 never reach forward(): the first call is
    forward(prompt[n-1], n-1) over a zero KV prefix.  Returns (generated tokens incl. a terminating one,
    TokenMetrics).  max_new_tokens bounds the loop (the reference only stops at seq_len / BOS / EOS).
    speculate=(ngram, draft_len): every token is drawn on the device by the sampler of Transformer.set_sampler (any temperature;
    argmax when none is set), several per weight pass where prompt-lookup drafts are accepted -- a draft is accepted exactly when
    it is the token the sampler draws, so the tokens are those of this loop with `sample` = the same Sampler.
    Top-k needs no argument here: it is the engine's (Transformer.set_top_k) and every device draw honours it; together with a host
    `sample` callback it is a ValueError."""
    if len(prompt_tokens) == 0:
        raise ValueError("Please provide a prompt")
    _check_top_k(transformer, sample)
    stop = set(stop_tokens)
    seq_len = transformer.get_config().seq_len
    metrics = TokenMetrics()
    out: List[int] = []
    if lookup is not None or speculate is not None:
        # lookup=(ngram, draft_len): the same tokens through prompt-lookup speculative decoding, the prompt as corpus
        if speculate is not None:
            _check_speculate(speculate, lookup, sample, on_logits)
        else:
            _check_lookup(lookup, sample, on_logits)
        pos = len(prompt_tokens) - 1
        budget = max(seq_len - pos, 0) if max_new_tokens is None else min(max(seq_len - pos, 0), max_new_tokens)
        _lookup_decode(transformer, [int(t) for t in prompt_tokens], pos, budget, stop, speculate or lookup, metrics, out, False,
                       draw=speculate is not None)
        metrics.report()
        return out, metrics
    pos, token = 0, prompt_tokens[0]
    while pos < seq_len:
        if pos < len(prompt_tokens) - 1:
            nxt = prompt_tokens[pos + 1]
        else:
            if max_new_tokens is not None and len(out) >= max_new_tokens:
                break
            metrics.start_generation()
            logits = np.array(transformer.forward(token, pos), copy=True)   # generation.rs:159-160
            if on_logits is not None:
                on_logits(token, pos, logits)
            nxt = sample(logits)
            metrics.increment_token()
            out.append(nxt)
            if nxt in stop:
                break
        token = nxt
        pos += 1
    metrics.report()
    return out, metrics


def common_prefix_len(prompts: Sequence[Sequence[int]]) -> int:
    """The length of the longest prefix all prompts share that leaves every prompt at least one token behind it."""
    if not prompts:
        return 0
    n = min(len(p) for p in prompts) - 1
    first = prompts[0]
    k = 0
    while k < n and all(p[k] == first[k] for p in prompts):
        k += 1
    return k


def generate_many(transformer, prompts: Sequence[Sequence[int]], max_new_tokens: int, stop_tokens: Iterable[int] = (), sampler=None,
                  dense_min: int = 0, stop_on_device: bool = False, shared_prefix=None, logprobs: Optional[int] = None,
                  presence_penalty: float = 0.0, frequency_penalty: float = 0.0, logit_bias=None, banned_tokens=None, allowed_tokens=None,
                  min_tokens=0, guide=None, regex: Optional[str] = None, tokenizer=None, stop=None):
    """Many greedy generations served through the slots of Transformer.batch_init in ragged column passes
    (Transformer.generate_many_greedy).  Row r holds what Transformer.prefill(prompts[r], 0) followed by generate_greedy returns on
    an engine of its own: every prompt token goes through the model (chat's prompt loop, generation.rs:116-123), then up to
    max_new_tokens tokens are decoded (fewer where the batch context ends first).  Each row ends with its first stop token, the way
    generate ends at BOS / EOS (generation.rs:35).  By default the device loop checks no stop token: every request runs to
    max_new_tokens and its row is cut afterwards.
    stop_on_device=True (with stop_tokens, at most 8): the device loop ends a request at its stop token and hands its slot to the
    next queued request at once (Transformer.generate_many_stop): the same rows in fewer passes, at one synchronisation per
    pass; the stats are those of the passes actually run.  Not offered together with dense_min > 0 (ValueError).
    sampler=(temperature, topp, seeds), each one value per prompt or a scalar for all: the same through
    Transformer.generate_many_sampled -- row r is what an engine of its own draws after set_sampler(temperature, topp, seed of r).
    dense_min > 0: prompts of more than dense_min tokens enter their slots through dense blocks, many prompts per weight pass
    (Transformer.generate_many_dense); the rows are the same for any value, 0 keeps the column loops.
    shared_prefix: a token list that every request begins with; `prompts` are then the SUFFIXES behind it.  The prefix is prefilled
    once (Transformer.batch_prefix_set, unless it is already resident; rows 0 .. of slot 0 are overwritten), its cache rows are
    copied into the slots, and only the suffixes go through the weights (Transformer.generate_many_prefix): the rows are those of the
    full prompts prefix + suffix, the stats those of the suffixes.  shared_prefix=True takes the longest common prefix of `prompts`
    that leaves every prompt a token (common_prefix_len); where the prompts share nothing it is shared_prefix=None.  None (the
    default) keeps the behaviour above.  Not offered together with dense_min > 0 (ValueError).
    Top-k needs no argument here: it is the engine's (Transformer.set_top_k), and every sampled request of every path above draws
    among the k most likely tokens while it is set; temperature-0 requests ignore it.
    logprobs: None, or 0 .. 64: the log-probability of every generated token, taken inside the loop (Transformer.set_gen_logprobs,
    which is set for this call and put back afterwards), and with logprobs > 0 that many most likely tokens at every step.  They
    are those of score() / top_logprobs() on prompt + row: the model's raw distribution at temperature 1 over the full vocabulary,
    whatever sampler drew the tokens.  Works with every option above; the rows are the same with or without it.
    Returns (rows, ColsStats); with logprobs set (rows, ColsStats, per row a tuple (logprobs[n], top_ids[n, k], top_logprobs[n, k],
    rank[n]) in the shape top_logprobs() uses, n the row's length, k = logprobs; with logprobs=0 the two middle entries are empty
    and so is rank).
    presence_penalty, frequency_penalty: -2 .. 2 (Transformer.set_penalties, set for this call and put back afterwards, also when the
    call raises): a token the row has produced c > 0 times has presence_penalty + frequency_penalty * c taken off its logit before the
    argmax or the draw, in front of temperature, top-k and top-p; prompt tokens do not count.  Works with every option above; the
    logprobs stay those of the raw distribution.
    logit_bias, banned_tokens, allowed_tokens, min_tokens: the caller constrains which tokens may come (Transformer.set_logit_bias,
    set for this call and put back afterwards, also when the call raises).  Each is one value for all requests or a sequence of one
    per request.  logit_bias: {token: bias}, bias (-100 .. 100, or -inf) added to the token's logit.  banned_tokens: tokens that
    never come.  allowed_tokens: the only tokens that may come ("answer with one of these labels").  min_tokens, with stop_tokens:
    no stop token among a row's first min_tokens tokens (a stop token that also carries a logit_bias is a ValueError).  They act on
    every generated token, the first included, in front of the penalties, temperature, top-k and top-p; the logprobs stay those of
    the raw distribution.  Works with every option above.  With none of the four given the call touches no table: one set with
    Transformer.set_logit_bias simply holds.
    guide: a constraint that changes with what the row has produced so far (guide.Automaton; Transformer.set_guide, set for this call
    and put back afterwards, also when the call raises): one Automaton for all requests, or a sequence of one per request in which
    None leaves a request unguided.  In state s only the tokens the automaton allows there may come, the first token included, in
    front of logit_bias and the penalties; the committed token moves the state.  A row ends at its stop token as ever: an automaton
    that wants to end allows a stop token in its accepting states.  Works with every option above; the logprobs stay those of the
    raw distribution.  With guide=None the call touches no guide: one set with Transformer.set_guide simply holds.  guide.SparseAutomaton
    is taken wherever Automaton is (Transformer.set_guide_sparse); in a sequence that mixes the two the dense ones are converted, and
    the engine's previous guide, of either form, is put back.
    regex: shorthand for guide=SparseAutomaton.from_regex(regex, tokenizer.vocab, eos) with eos the one stop token of stop_tokens:
    every row spells a prefix of a full match of the pattern (guide.regex_dfa states the syntax), and ends with eos only behind a
    full match.  `tokenizer` is a Tokenizer or anything with a list `vocab` of the tokens' bytes.  Compiled automata are kept per
    (pattern, tokenizer, eos).  Not together with guide=.
    stop: stop SEQUENCES, the stop=[...] of a serving API: a list of strings (needs tokenizer=; a string may end inside a token or span
    several tokens), a list of token lists, a SparseAutomaton of stops.stop_automaton / stops.stop_automaton_from_strings, or a
    sequence of one such value per request in which None gives a request no stop sequences.  A row ends with the token that
    completes a sequence, as it ends with a stop token, whichever comes first; stops.cut_at_stop(text, strings) then gives the text
    in front of the stop string.  Only generated tokens count.  min_tokens does not delay a sequence.  By default the rows are cut
    on the host (SparseAutomaton.walk); with stop_on_device=True the automaton goes to the engine for this call
    (Transformer.set_stop_sequences, put back afterwards, also when the call raises) and the device loop ends the requests
    (Transformer.generate_many_stop, also without stop_tokens, or generate_many_prefix): the same rows in fewer passes.  Works
    with every option above except dense_min > 0 under stop_on_device (ValueError)."""
    if any(len(p) == 0 for p in prompts):
        raise ValueError("Please provide a prompt")
    if regex is not None:
        if guide is not None:
            raise ValueError("regex= and guide= exclude each other")
        stop_tokens = [int(t) for t in stop_tokens]
        if tokenizer is None or len(stop_tokens) != 1:
            raise ValueError("regex= needs tokenizer= and exactly one stop token, the end of a full match")
        guide = _regex_guide(regex, tokenizer, stop_tokens[0])
    stop_seq = None if stop is None else compile_stop(stop, len(prompts), transformer.get_config().vocab_size, tokenizer)
    args = (transformer, prompts, max_new_tokens, stop_tokens, sampler, dense_min, stop_on_device, shared_prefix, logprobs, presence_penalty,
            frequency_penalty, logit_bias, banned_tokens, allowed_tokens, min_tokens, stop_seq)
    if guide is None:
        return _generate_many_bias(*args)
    table, start = merge_guides(guide, len(prompts))
    if len(start) > 1:
        # the engine sees the requests the context leaves room for, and one start state for each of them
        start = [start[r] for r in _live_requests(transformer, prompts, max_new_tokens, shared_prefix)]
    guide_before = transformer.get_guide()
    sparse_before = transformer.get_guide_sparse() if hasattr(transformer, "get_guide_sparse") else None
    if isinstance(table, SparseAutomaton):
        transformer.set_guide_sparse(table.default, table.offsets, table.tokens, table.targets, start)
    else:
        transformer.set_guide(table, start)
    try:
        return _generate_many_bias(*args)
    finally:
        # one guide holds at a time: putting back the form that held clears the other
        if sparse_before is not None and sparse_before[0] is not None:
            transformer.set_guide_sparse(*sparse_before)
        else:
            transformer.set_guide(*guide_before)


_REGEX_GUIDES: dict = {}


def _regex_guide(pattern: str, tokenizer, eos: int) -> SparseAutomaton:
    """SparseAutomaton.from_regex, compiled once per (pattern, tokenizer, eos); the tokenizer is kept beside it so that its id stays its own"""
    key = (pattern, id(tokenizer), int(eos))
    if key not in _REGEX_GUIDES:
        _REGEX_GUIDES[key] = (SparseAutomaton.from_regex(pattern, tokenizer.vocab, int(eos)), tokenizer)
    return _REGEX_GUIDES[key][0]


def _generate_many_bias(transformer, prompts, max_new_tokens, stop_tokens, sampler, dense_min, stop_on_device, shared_prefix, logprobs, presence_penalty,
                        frequency_penalty, logit_bias, banned_tokens, allowed_tokens, min_tokens, stop_seq=None):
    """generate_many behind its guide handling"""
    args = (transformer, prompts, max_new_tokens, stop_tokens, sampler, dense_min, stop_on_device, shared_prefix, logprobs, presence_penalty,
            frequency_penalty, stop_seq)
    if logit_bias is None and banned_tokens is None and allowed_tokens is None and np.isscalar(min_tokens) and min_tokens == 0:
        return _generate_many_pen(*args)
    lists, modes = merge_logit_bias(len(prompts), logit_bias, banned_tokens, allowed_tokens, min_tokens, stop_tokens)
    if len(lists) > 1:
        # the engine sees the requests the context leaves room for, and one list for each of them
        live = _live_requests(transformer, prompts, max_new_tokens, shared_prefix)
        lists, modes = [lists[r] for r in live], [modes[r] for r in live]
    bias_before = transformer.get_logit_bias()
    transformer.set_logit_bias(lists, modes)
    try:
        return _generate_many_pen(*args)
    finally:
        transformer.set_logit_bias(*bias_before)


def _live_requests(transformer, prompts, max_new_tokens, shared_prefix):
    """the requests _generate_many hands to the engine: those the batch context leaves room for at least one new token"""
    ahead = 0 if shared_prefix is None or shared_prefix is False or shared_prefix is True else len(list(shared_prefix))
    ctx = getattr(transformer, "_batch_ctx", transformer.get_config().seq_len)
    return [r for r, p in enumerate(prompts) if min(max_new_tokens, ctx - ahead - len(p) + 1) > 0]


def merge_logit_bias(n_requests, logit_bias=None, banned_tokens=None, allowed_tokens=None, min_tokens=0, stop_tokens=()):
    """generate_many's four arguments as the (lists, modes) of Transformer.set_logit_bias: one list where every argument is a single
    value, else one per request.  Per list: logit_bias {token: bias} gives (token, bias, 0); a banned token (token, -inf, 0); with
    allowed_tokens the mode is BIAS_ALLOW and an allowed token without an entry gets (token, 0.0, 0); min_tokens = m > 0 gives
    (stop, -inf, m) per stop token -- skipped where the token is banned already or unlisted under BIAS_ALLOW, in place of the 0.0 of a
    token that is merely allowed, and a ValueError where logit_bias names the token."""
    def per_request(v, single):
        return v is not None and not single(v)

    def is_tokens(v):
        v = list(v)
        return all(isinstance(t, (int, np.integer)) for t in v)
    per = {"logit_bias": per_request(logit_bias, lambda v: isinstance(v, dict)), "banned_tokens": per_request(banned_tokens, is_tokens),
           "allowed_tokens": per_request(allowed_tokens, is_tokens), "min_tokens": not np.isscalar(min_tokens)}
    given = {"logit_bias": logit_bias, "banned_tokens": banned_tokens, "allowed_tokens": allowed_tokens, "min_tokens": min_tokens}
    for name, p in per.items():
        if p:
            given[name] = list(given[name])
            if len(given[name]) != n_requests:
                raise ValueError(f"{name}: {len(given[name])} values for {n_requests} requests")
    stop = sorted(set(int(t) for t in stop_tokens))
    lists, modes = [], []
    for r in range(n_requests if any(per.values()) else 1):
        at = lambda name: given[name][r] if per[name] else given[name]
        bias, banned, allowed, m = at("logit_bias"), at("banned_tokens"), at("allowed_tokens"), at("min_tokens")
        if bias is not None and not isinstance(bias, dict):
            raise TypeError(f"logit_bias must be a dict {{token: bias}}, got {bias!r}")
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)):
            raise TypeError(f"min_tokens must be an integer, got {m!r}")
        if m < 0:
            raise ValueError(f"min_tokens {m} is negative")
        named = dict(bias or {})
        ent = {t: (b, 0) for t, b in named.items()}
        for t in (banned if banned is not None else ()):
            ent[t] = (float("-inf"), 0)
        if allowed is not None:
            allowed = list(allowed)
            for t in allowed:
                ent.setdefault(t, (0.0, 0))
        for t in (stop if m > 0 else ()):
            if t in named:
                raise ValueError(f"min_tokens: stop token {t} also carries a logit_bias")
            if ent.get(t) == (float("-inf"), 0) or (allowed is not None and t not in ent):
                continue
            ent[t] = (float("-inf"), int(m))
        lists.append([(t, b, u) for t, (b, u) in sorted(ent.items())])
        modes.append(BIAS_ALLOW if allowed is not None else BIAS_ADD)
    return lists, modes


def _generate_many_pen(transformer, prompts, max_new_tokens, stop_tokens, sampler, dense_min, stop_on_device, shared_prefix, logprobs, presence_penalty,
                       frequency_penalty, stop_seq=None):
    """generate_many behind its logit-bias handling"""
    # (an engine stand-in without the setting serves a call without penalties as it did)
    if hasattr(transformer, "get_penalties") or presence_penalty != 0.0 or frequency_penalty != 0.0:
        pen_before = transformer.get_penalties()
        transformer.set_penalties(presence_penalty, frequency_penalty)
        try:
            return _generate_many_lp(transformer, prompts, max_new_tokens, stop_tokens, sampler, dense_min, stop_on_device, shared_prefix, logprobs,
                                     stop_seq)
        finally:
            transformer.set_penalties(*pen_before)
    return _generate_many_lp(transformer, prompts, max_new_tokens, stop_tokens, sampler, dense_min, stop_on_device, shared_prefix, logprobs, stop_seq)


def _generate_many_lp(transformer, prompts, max_new_tokens, stop_tokens, sampler, dense_min, stop_on_device, shared_prefix, logprobs, stop_seq=None):
    """generate_many behind its penalties handling"""
    if logprobs is not None:
        if isinstance(logprobs, bool) or not isinstance(logprobs, (int, np.integer)) or logprobs < 0 or logprobs > 64:
            raise ValueError(f"logprobs {logprobs!r} out of range (None, or 0..64)")
        before = transformer.get_gen_logprobs()
        transformer.set_gen_logprobs(int(logprobs))
        try:
            rows, stats, recs = _generate_many(transformer, prompts, max_new_tokens, stop_tokens, sampler, dense_min, stop_on_device, shared_prefix, True,
                                               stop_seq)
        finally:
            transformer.set_gen_logprobs(before)
        k = int(logprobs)
        out = []
        for row, rec in zip(rows, recs):
            if rec is None:                                  # a request the context left no room for
                rec = (np.zeros(0, dtype=SCORE_DTYPE), np.zeros((0, k), dtype=TOP_DTYPE), np.zeros(0, dtype=np.int32))
            r, t, q = (a[:len(row)] for a in rec)
            out.append((logprobs_of(r), np.array(t["index"], dtype=np.int32).reshape(len(r), k), top_logprobs_of(r, t).reshape(len(r), k),
                        np.asarray(q, dtype=np.int32)))
        return rows, stats, out
    return _generate_many(transformer, prompts, max_new_tokens, stop_tokens, sampler, dense_min, stop_on_device, shared_prefix, False, stop_seq)[:2]


def _generate_many(transformer, prompts, max_new_tokens, stop_tokens, sampler, dense_min, stop_on_device, shared_prefix, read_logprobs, stop_seq=None):
    """generate_many behind its logprobs handling: (rows, ColsStats, per row the engine's (records, tops, ranks) or None).
    stop_seq: None, or stops.compile_stop's (automaton, start) with one start state or one per prompt"""
    stop = set(stop_tokens)
    if stop_on_device and dense_min > 0:
        raise ValueError("stop_on_device=True runs column passes only: no dense_min > 0")
    if shared_prefix is not None and shared_prefix is not False and dense_min > 0:
        raise ValueError("shared_prefix runs column passes only: no dense_min > 0")
    prefix: List[int] = []
    if shared_prefix is True:
        k = common_prefix_len(prompts)
        prefix, prompts = [int(t) for t in prompts[0][:k]], [p[k:] for p in prompts]
    elif shared_prefix is not None and shared_prefix is not False:
        prefix = [int(t) for t in shared_prefix]
    ctx = getattr(transformer, "_batch_ctx", transformer.get_config().seq_len)
    n_new = [max(min(max_new_tokens, ctx - len(prefix) - len(p) + 1), 0) for p in prompts]
    live = [r for r, k in enumerate(n_new) if k > 0]
    rows: List[List[int]] = [[] for _ in prompts]
    recs = [None] * len(prompts)
    stats = None
    if live:
        live_prompts, live_new = [prompts[r] for r in live], [n_new[r] for r in live]
        per_live = None
        if sampler is not None:
            temperature, topp, seeds = ([v] * len(prompts) if np.isscalar(v) else list(v) for v in sampler)
            per_live = tuple([v[r] for r in live] for v in (temperature, topp, seeds))
        seq_start = None
        if stop_seq is not None:
            # the engine sees the requests the context leaves room for, and one start state for each of them
            seq_start = list(stop_seq[1]) if len(stop_seq[1]) == 1 else [stop_seq[1][r] for r in live]
        seq_on_device = stop_seq is not None and stop_on_device
        if seq_on_device:
            seq_before = transformer.get_stop_sequences()
            transformer.set_stop_sequences(stop_seq[0], seq_start)
        try:
            if prefix:
                if transformer.batch_prefix_get() != prefix:
                    transformer.batch_prefix_set(prefix)
                got, stats = transformer.generate_many_prefix(live_prompts, live_new, sorted(stop) if stop_on_device else (), per_live)
            elif stop_on_device and (stop or seq_on_device):
                got, stats = transformer.generate_many_stop(live_prompts, live_new, sorted(stop), per_live)
            elif dense_min > 0:
                got, stats, _ = transformer.generate_many_dense(live_prompts, live_new, per_live, dense_min)
            elif sampler is None:
                got, stats = transformer.generate_many_greedy(live_prompts, live_new)
            else:
                got, stats = transformer.generate_many_sampled(live_prompts, live_new, *per_live)
        finally:
            if seq_on_device:
                transformer.set_stop_sequences(*seq_before)
        for i, (r, toks) in enumerate(zip(live, got)):
            k = next((j for j, t in enumerate(toks) if t in stop), None)
            if stop_seq is not None:
                m = first_match(stop_seq[0], seq_start[0 if len(seq_start) == 1 else i], toks)
                k = m if k is None else (k if m is None else min(k, m))
            rows[r] = toks if k is None else toks[:k + 1]
        if read_logprobs:
            for r, rec in zip(live, transformer.read_gen_logprobs()):
                recs[r] = rec
    return rows, stats, recs


def embed(transformer, prompts: Sequence[Sequence[int]], normalize: bool = True, out_dim: Optional[int] = None, shared_prefix=None):
    """The embeddings of many prompts: the hidden state of each prompt's last token behind the final RMSNorm, cut to its first
    out_dim components (None: all) and, with normalize, L2-normalised -- what a Qwen3-Embedding checkpoint is read out by.
    The prompts go through the slots of Transformer.batch_init in dense blocks (Transformer.embed_many); the slots' contents
    are overwritten.  shared_prefix as in generate_many: a token list every prompt begins with (`prompts` are then the suffixes
    behind it; it is made resident with Transformer.batch_prefix_set unless it already is), True for the longest common prefix
    of `prompts` (common_prefix_len), None for no prefix.  Returns a float32 array [len(prompts), out_dim]."""
    if any(len(p) == 0 for p in prompts):
        raise ValueError("Please provide a prompt")
    prompts, use_prefix = _split_prefix(transformer, prompts, shared_prefix)
    return transformer.embed_many(prompts, normalize=normalize, out_dim=out_dim, use_prefix=use_prefix)[0]


def _split_prefix(transformer, prompts, shared_prefix):
    """shared_prefix of embed / choose: (the prompts behind the prefix, whether one is in use); the prefix is made resident"""
    prefix: List[int] = []
    if shared_prefix is True:
        k = common_prefix_len(prompts)
        prefix, prompts = [int(t) for t in prompts[0][:k]], [p[k:] for p in prompts]
    elif shared_prefix is not None and shared_prefix is not False:
        prefix = [int(t) for t in shared_prefix]
    if prefix and transformer.batch_prefix_get() != prefix:
        transformer.batch_prefix_set(prefix)
    return prompts, bool(prefix)


def normalise_logits(logits: np.ndarray, output: str) -> np.ndarray:
    """softmax / log_softmax over the last axis of float32 logits, in float64: the row maximum is subtracted, then exp, the sum and
    log.  Nothing is special-cased: a NaN makes its whole row NaN, and a row whose maximum is not finite (all -inf, or a +inf)
    gives NaN as numpy's -inf - -inf and inf - inf do; -inf beside finite logits gives probability 0 and log-probability -inf."""
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = z - z.max(axis=-1, keepdims=True)
        ez = np.exp(z)
        tot = ez.sum(axis=-1, keepdims=True)
        return ez / tot if output == "softmax" else z - np.log(tot)


def choose(transformer, prompts: Sequence[Sequence[int]], candidates, shared_prefix=None, output: str = "logits"):
    """The scores of a few candidate tokens behind each prompt's last token: what a reranker, a multiple-choice evaluator or a yes/no
    classifier reads.  candidates: one list of token ids for all prompts, or one list per prompt, all of one length k.  The logits
    are bit for bit those of forward() (Transformer.choice_many: the prompts go through the slots of Transformer.batch_init in
    dense blocks, no classifier pass over the vocabulary runs, the slots' contents are overwritten).  shared_prefix as in embed.
    output: "logits" returns the float32 array [len(prompts), k]; "softmax" and "log_softmax" normalise over the k candidates
    only, on the host, and return float64 (normalise_logits, which also says what NaN and infinite logits give)."""
    if output not in ("logits", "softmax", "log_softmax"):
        raise ValueError(f"unknown output {output!r}")
    if any(len(p) == 0 for p in prompts):
        raise ValueError("Please provide a prompt")
    prompts, use_prefix = _split_prefix(transformer, prompts, shared_prefix)
    logits = transformer.choice_many(prompts, candidates, use_prefix=use_prefix)[0]
    return logits if output == "logits" else normalise_logits(logits, output)


def logprobs_of(records) -> np.ndarray:
    """log P(target) of Transformer.score_many's records: (target - max) - log(sum), in float64 from the three float32 fields.
    Nothing is special-cased: sum == 0 gives what numpy's log(0) gives (+inf here), an infinite field or a NaN propagates."""
    t, m, s = (np.asarray(records[k], dtype=np.float32).astype(np.float64) for k in ("target", "max", "sum"))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (t - m) - np.log(s)


def top_logprobs_of(records, tops) -> np.ndarray:
    """log P of the alternatives of Transformer.score_top_many: (logit - max) - log(sum) per column of the (n, k) TOP_DTYPE array
    `tops`, max and sum those of the n records; float64, the expression of logprobs_of."""
    m, s = (np.asarray(records[f], dtype=np.float32).astype(np.float64)[:, None] for f in ("max", "sum"))
    l = np.asarray(tops["logit"], dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (l - m) - np.log(s)


def _score_requests(transformer, prompts, score_from, shared_prefix):
    """What score and top_logprobs hand to the engine: (prompts, score_from, use_prefix) behind the shared_prefix handling"""
    if any(len(p) == 0 for p in prompts):
        raise ValueError("Please provide a prompt")
    sf = None if score_from is None else [int(v) for v in score_from]
    if shared_prefix is True:
        # the first suffix token is never a target: the prefix ends in front of the earliest scored position's input
        k = min(common_prefix_len(prompts), min(sf if sf is not None else [1]) - 1)
        shared_prefix = None
        if k > 0:
            shared_prefix, prompts = [int(t) for t in prompts[0][:k]], [p[k:] for p in prompts]
            sf = [v - k for v in sf]
    prompts, use_prefix = _split_prefix(transformer, prompts, shared_prefix)
    return prompts, sf, use_prefix


def score(transformer, prompts: Sequence[Sequence[int]], score_from=None, shared_prefix=None, records: bool = False):
    """log P(t[i + 1] | t[0 .. i]) for the positions of many prompts: one float64 array per prompt, entry j for the target
    t[score_from[r] + j] (score_from None: every token but the first is a target; score_from[r] == len gives an empty array).
    The prompts go through the slots of Transformer.batch_init in dense blocks and the classifier runs for the scored positions
    only, 32 at a time; the vocabulary-wide sums stay on the device (Transformer.score_many), the slots' contents are overwritten.
    shared_prefix as in embed: a token list (`prompts` and score_from are then those of the suffixes behind it), True for the
    longest common prefix of `prompts` that holds no scored position's input, None for no prefix.
    records: return (log-prob arrays, the SCORE_DTYPE record arrays) instead."""
    prompts, sf, use_prefix = _score_requests(transformer, prompts, score_from, shared_prefix)
    recs = transformer.score_many(prompts, sf, use_prefix=use_prefix)[0]
    lps = [logprobs_of(r) for r in recs]
    return (lps, recs) if records else lps


def top_logprobs(transformer, prompts: Sequence[Sequence[int]], k: int, score_from=None, shared_prefix=None):
    """score() with the k most likely tokens of every scored position (Transformer.score_top_many): per prompt a tuple
    (logprobs[n], ids[n, k], top_logprobs[n, k], rank[n]) -- log P of the targets as score() gives them; the ids of the k most
    likely tokens, most likely first (ties in the logit: the higher id first); their log P; the number of tokens the model ranks
    above the target (0: the target is the most likely one; rank[j] < k: the target is ids[j, rank[j]]).  score_from and shared_prefix
    as for score()."""
    prompts, sf, use_prefix = _score_requests(transformer, prompts, score_from, shared_prefix)
    recs, tops, ranks, _ = transformer.score_top_many(prompts, k, sf, use_prefix=use_prefix)
    return [(logprobs_of(r), np.array(t["index"], dtype=np.int32), top_logprobs_of(r, t), np.asarray(q, dtype=np.int32))
            for r, t, q in zip(recs, tops, ranks)]


def loglikelihood(transformer, contexts: Sequence[Sequence[int]], continuations: Sequence[Sequence[int]], shared_prefix=None):
    """(log P(continuation | context), whether the continuation is the greedy one) for every pair, lm-eval's `loglikelihood`: one
    score call over context + continuation with score_from = len(context).  The context must hold at least one token (behind a
    shared_prefix token list: the part of it behind the prefix).  is_greedy: argmax == target at every continuation position."""
    if len(contexts) != len(continuations):
        raise ValueError("one continuation per context")
    if any(len(c) == 0 for c in contexts):
        raise ValueError("Please provide a context")
    prompts = [[int(t) for t in c] + [int(t) for t in k] for c, k in zip(contexts, continuations)]
    lps, recs = score(transformer, prompts, [len(c) for c in contexts], shared_prefix=shared_prefix, records=True)
    out = []
    for p, c, lp, rec in zip(prompts, contexts, lps, recs):
        targets = np.asarray(p[len(c):], dtype=np.int32)
        out.append((float(lp.sum()), bool(np.array_equal(rec["argmax"], targets))))
    return out


def perplexity(logprob_arrays) -> float:
    """exp(-mean log-prob) over all scored tokens of score()'s arrays, in float64 (NaN when nothing was scored)"""
    arrays = [np.asarray(a, dtype=np.float64).ravel() for a in logprob_arrays]
    lp = np.concatenate(arrays) if arrays else np.zeros(0)
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.exp(-lp.mean())) if lp.size else float("nan")


# The prompt of the Qwen3-Reranker family, as its model card gives it.  Written from memory: no such checkpoint or card was at hand
# when this was written, so the wording is unverified.
RERANK_INSTRUCTION = "Given a web search query, retrieve relevant passages that answer the query"
RERANK_TEMPLATE = ("<|im_start|>system\nJudge whether the Document meets the requirements based on the Query and the Instruct provided. "
                   "Note that the answer can only be \"yes\" or \"no\".<|im_end|>\n"
                   "<|im_start|>user\n<Instruct>: {instruction}\n<Query>: {query}\n<Document>: {document}<|im_end|>\n"
                   "<|im_start|>assistant\n<think>\n\n</think>\n\n")


def rerank(transformer, tokenizer, query: str, documents: Sequence[str], instruction: Optional[str] = None, yes: str = "yes", no: str = "no"):
    """P(yes) of every document for the query, the way a Qwen3-Reranker checkpoint is read out: one prompt per document from
    RERANK_TEMPLATE, each tokenized as a whole string; the logits of the tokens `no` and `yes` behind it (choose, the prompts'
    longest common token prefix resident and computed once); softmax over the two.  `yes` and `no` must each be exactly one token
    of the tokenizer.  Returns a float64 array [len(documents)]."""
    ids = []
    for word in (no, yes):
        enc = tokenizer.encode(word)
        if len(enc) != 1:
            raise ValueError(f"{word!r} is {len(enc)} tokens in this tokenizer: the answer words must be one token each")
        ids.append(int(enc[0]))
    instruction = RERANK_INSTRUCTION if instruction is None else instruction
    prompts = [tokenizer.encode(RERANK_TEMPLATE.format(instruction=instruction, query=query, document=d)) for d in documents]
    return choose(transformer, prompts, ids, shared_prefix=True, output="softmax")[:, 1]


def chat_turn(transformer, prompt_tokens: Sequence[int], pos: int, max_new_tokens: int,
              stop_tokens: Iterable[int] = (), sample: Callable[[np.ndarray], int] = sample_argmax,
              on_logits: Optional[Callable[[int, int, np.ndarray], None]] = None, lookup: Optional[Tuple[int, int]] = None,
              speculate: Optional[Tuple[int, int]] = None):
    """One user turn + assistant turn of `chat` (generation.rs:94-151): every prompt token goes through
    forward() one at a time (sequential prefill, a sample drawn and discarded for each), then decode until
    a stop token.  Returns (generated tokens, next pos, TokenMetrics).
    speculate=(ngram, draft_len): the turn on the device under the sampler of Transformer.set_sampler -- the prompt through
    Transformer.prefill (which draws and discards the per-prompt coins itself), the assistant turn as in generate(speculate=).
    Top-k needs no argument here: it is the engine's (Transformer.set_top_k) and every device draw honours it; together with a host
    `sample` callback it is a ValueError."""
    _check_top_k(transformer, sample)
    stop = set(stop_tokens)
    seq_len = transformer.get_config().seq_len
    next_token = 0
    if speculate is not None:
        _check_speculate(speculate, lookup, sample, on_logits)
        metrics = TokenMetrics()
        out: List[int] = []
        ids = [int(t) for t in prompt_tokens][: max(seq_len - pos, 0)]
        if ids:
            next_token = transformer.prefill(ids, pos)
            pos += len(ids)
            pos = _lookup_decode(transformer, ids + [int(next_token)], pos, min(max_new_tokens, max(seq_len - pos, 0)), stop, speculate,
                                 metrics, out, True, draw=True)
        metrics.report()
        return out, pos, metrics
    for tok in prompt_tokens:                       # handle_user_turn, generation.rs:116-123
        if pos >= seq_len:
            break
        logits = np.array(transformer.forward(tok, pos), copy=True)
        if on_logits is not None:
            on_logits(tok, pos, logits)
        next_token = sample(logits)
        pos += 1
    metrics = TokenMetrics()
    out: List[int] = []
    if lookup is not None:
        # lookup=(ngram, draft_len): the assistant turn through prompt-lookup speculative decoding, the turn's prompt as corpus
        _check_lookup(lookup, sample, on_logits)
        if prompt_tokens:
            history = [int(t) for t in prompt_tokens] + [int(next_token)]
            pos = _lookup_decode(transformer, history, pos, min(max_new_tokens, max(seq_len - pos, 0)), stop, lookup, metrics, out, True)
        metrics.report()
        return out, pos, metrics
    while len(out) < max_new_tokens and pos < seq_len:   # handle_assistant_turn, generation.rs:127-151
        if next_token in stop:
            break
        metrics.start_generation()
        out.append(next_token)
        logits = np.array(transformer.forward(next_token, pos), copy=True)
        if on_logits is not None:
            on_logits(next_token, pos, logits)
        next_token = sample(logits)
        metrics.increment_token()
        pos += 1
    metrics.report()
    return out, pos, metrics
