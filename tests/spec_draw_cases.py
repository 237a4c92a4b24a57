"""The inputs the tests of section 2d (draft verification under the sampler) share: the GPU lookup test runs exactly these
cases, and the CPU test shows on the C oracle that each of them accepts a draft and rejects one.

Shapes: the three of test_speculative.py the C oracle decodes in about a second.  The 151,936-entry-vocabulary shapes are covered by
the q3_verify_draw tests, which need no oracle.  Synthetic checkpoints have near-flat logits, so at these temperatures a
draft is only ever right when the corpus already holds the sampled text: the corpus is the reference output itself with
every 7th token altered ("G7"), which gives accepted drafts up to each altered token and a rejection there."""

# shape -> (checkpoint seed, first token, context length; 0 = the checkpoint's)   (test_speculative.MODELS)
ORACLE_MODELS = {
    "tiny-g64": (99, 3, 0),
    "small-hd128": (21, 17, 0),
    "small-longctx": (99, 3, 512),
}
# (temperature, top-p): multinomial, nucleus, a temperature below 1
SAMPLERS = [(1.0, 1.0), (1.0, 0.9), (0.7, 0.95)]
SEEDS = [42, 0x9E3779B97F4A7C15]
N_REF = 60
# (ngram, draft_len, first_pos)
LOOKUPS = [(2, 8, 0), (1, 31, 5)]


def g7(G, vocab):
    return [(g + 1) % vocab if i % 7 == 6 else g for i, g in enumerate(G)]


def lookup_cases():
    """(shape, temperature, top-p, seed, ngram, draft_len, first_pos); the corpus is g7(G)"""
    return [(name, T, p, seed, ngram, d, p0) for name in ORACLE_MODELS for (T, p) in SAMPLERS for seed in SEEDS for (ngram, d, p0) in LOOKUPS]


def case_id(c):
    return f"{c[0]}-t{c[1]}-p{c[2]}-s{c[3] & 0xffff}-g{c[4]}-d{c[5]}-p{c[6]}"
