"""The inputs the tests of section 2f (column passes under the sampler) share: the GPU test runs exactly these requests, and the
CPU test shows on the C oracle that each of them tells the chat rule from its neighbours -- the other seed, the draws made
without the prompt's discarded coins, and the argmax.

The rule: request r with prompt P, sampler (T, p) and seed s yields the tokens of `chat` on an engine of its own -- one sample
drawn and discarded per prompt position but the last (generation.rs:116-123), then the decode loop (generation.rs:127-151)."""
import numpy as np

# shape -> batch context (test_batch_cols.SHAPES): k_attn_gqa with a 512-entry vocabulary; k_attn_gqa2<2> with 2,048 entries; 4 query
# heads per kv head, 16,384 entries and a radix-sorted nucleus
SHAPES = {"tiny-g64": 0, "small-hd128": 0, "qwen3-4b-dims-l2": 512}
CKPT_SEED = 2468
# (temperature, top-p): multinomial, nucleus, a temperature below 1; and the greedy setting (top-p is not read)
SAMPLERS = [(1.0, 1.0), (1.0, 0.9), (0.7, 0.95)]
GREEDY = (0.0, 0.9)
SEEDS = [42, 0x9E3779B97F4A7C15]
# request r: a prompt of PROMPT_LEN[r] tokens, N_NEW[r] new tokens (3 .. 12); 33 and 40 do not fit one pass of 32 columns
PROMPT_LEN = (1, 2, 5, 33, 40)
N_NEW = (3, 12, 7, 5, 9)
SLOT_COUNTS = (1, 3, 8)


def prompts(vocab_size):
    return [[int(t) for t in np.random.default_rng(900 + r).integers(0, vocab_size, n)] for r, n in enumerate(PROMPT_LEN)]


def request_seeds(which):
    """seed of every request: the two seeds alternate, starting with SEEDS[which]; request_seeds(1 - which) swaps them"""
    return [SEEDS[(which + r) % 2] for r in range(len(PROMPT_LEN))]


def sampler_id(s):
    return f"t{s[0]}-p{s[1]}"
