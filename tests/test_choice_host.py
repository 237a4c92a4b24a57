"""Choice logits (include/qwen3_hip.h section 2k): what can be checked without a GPU -- the entry point's first refusal and its
place in the ABI, the header's arithmetic restated in numpy (tests/choice_ref.py) against the C oracle's classifier, the host-side
output modes of generation.choose, the prompts generation.rerank builds, and the command line's parser."""
import ctypes as C
import os

import numpy as np
import pytest

import choice_ref
from conftest import ROOT, assert_biteq, golden_path


def test_a_null_engine_is_refused_before_anything_touches_the_gpu(q3):
    lib = q3.load_library()
    lens = (C.c_size_t * 1)(3)
    toks = (C.c_int32 * 3)(1, 2, 3)
    cand = (C.c_int32 * 2)(0, 1)
    out = (C.c_float * 2)()
    assert lib.q3_choice_many(None, toks, lens, 1, cand, 2, 0, out, None) == -3
    assert b"null engine" in lib.q3_last_error()


def test_the_symbol_is_exported_declared_and_listed(q3):
    assert "q3_choice_many" in q3.EXPORTED_SYMBOLS and hasattr(q3.load_library(), "q3_choice_many")
    header = open(os.path.join(ROOT, "include", "qwen3_hip.h")).read()
    assert "int q3_choice_many(q3_engine* e," in header
    for name, value in (("Q3_CHOICE_PREFIX", q3.CHOICE_PREFIX), ("Q3_CHOICE_PER_REQUEST", q3.CHOICE_PER_REQUEST), ("Q3_CHOICE_MAX", q3.CHOICE_MAX)):
        assert f"#define {name} " in header
        assert int(header.split(f"#define {name} ")[1].split()[0].rstrip("u")) == value
    assert q3.CHOICE_PREFIX == q3.EMBED_PREFIX


@pytest.mark.parametrize("name", ["tiny.bin", "tiny-untied.bin"])
def test_the_header_arithmetic_is_the_oracles_classifier(oracle, name):
    """tap_x() of the last forward -- the final RMSNorm's output -- through choice_ref with the checkpoint's classifier rows equals the
    oracle's logits at those ids, bit for bit"""
    path = golden_path(name)
    om = oracle.OracleModel(path)
    V = om.get_config().vocab_size
    wq, ws, G = choice_ref.classifier(path)
    assert wq.shape[0] == V
    for prompt, ids in (([5], [0, V - 1]), ([1, 2, 3, 4], [V - 1, 17, 17, 0, 100]), ([200, 17, 17, 3, 90, 41, 8], [0, 1, 2, V - 2, V - 1, 33])):
        om.reset()
        for pos, tok in enumerate(prompt):
            want = np.array(om.forward(tok, pos), copy=True)
        got = choice_ref.logits(om.tap_x(), wq, ws, ids, G)
        assert_biteq(got, want[ids], f"{name}: prompt of {len(prompt)} tokens")


def test_choice_ref_quantizer_on_hand_made_vectors():
    # a zero group gives a zero scale and zero codes; halves round away from zero; the maximum becomes 127
    y = np.zeros(128, dtype=np.float32)
    y[64:] = np.linspace(-1.0, 1.0, 64, dtype=np.float32)
    y[64], y[65], y[66] = 127.0, 0.5, -2.5
    q, s = choice_ref.quantize(y, 64)
    assert s[0] == 0.0 and not q[:64].any()
    assert s[1] == np.float32(1.0) and (q[64], q[65], q[66]) == (127, 1, -3)


class _Stub:
    """a transformer whose choice_many returns hand-made logits and records its call"""

    def __init__(self, logits):
        self.logits = np.asarray(logits, dtype=np.float32)
        self.calls, self.prefix = [], []

    def batch_prefix_get(self):
        return self.prefix

    def batch_prefix_set(self, p):
        self.prefix = list(p)

    def choice_many(self, prompts, candidates, use_prefix=False):
        self.calls.append(([list(p) for p in prompts], list(candidates), use_prefix))
        return self.logits[:len(prompts)], None


def test_the_host_output_modes(q3):
    k = 5
    rows = np.array([[3.25] * k, [-800.0, 0.0, -800.0, -800.0, -800.0], [1.0, 2.0, 3.0, 4.0, 5.0]], dtype=np.float32)
    prompts = [[1], [2], [3]]
    raw = q3.choose(_Stub(rows), prompts, [1, 2, 3, 4, 5])
    assert raw.dtype == np.float32 and np.array_equal(raw, rows)
    with np.errstate(over="raise", invalid="raise"):                     # a gap of 800 does not overflow: exp(-800) is exactly 0
        p = q3.choose(_Stub(rows), prompts, [1, 2, 3, 4, 5], output="softmax")
        lp = q3.choose(_Stub(rows[[0, 2]]), prompts[:2], [1, 2, 3, 4, 5], output="log_softmax")
    assert p.dtype == np.float64 and lp.dtype == np.float64
    assert np.array_equal(p[0], np.full(k, 1.0 / k))                     # equal logits give 1/k
    assert np.array_equal(p[1], np.array([0.0, 1.0, 0.0, 0.0, 0.0]))
    two = q3.choose(_Stub([[-800.0, 0.0]]), [[1]], [7, 8], output="softmax")
    assert np.array_equal(two, np.array([[0.0, 1.0]]))
    assert np.all(np.abs(np.exp(lp).sum(axis=1) - 1.0) <= k * 2.0 ** -52)
    assert np.all(np.abs(np.exp(lp) - p[[0, 2]]) <= 2.0 ** -50)
    with pytest.raises(ValueError):
        q3.choose(_Stub(rows), prompts, [1, 2], output="probs")
    with pytest.raises(ValueError):
        q3.choose(_Stub(rows), [[1], []], [1, 2])
    # NaN and all -inf rows propagate as numpy does it
    odd = q3.choose(_Stub([[np.nan, 1.0], [-np.inf, -np.inf], [-np.inf, 0.0]]), prompts, [1, 2], output="softmax")
    assert np.isnan(odd[0]).all() and np.isnan(odd[1]).all() and np.array_equal(odd[2], np.array([0.0, 1.0]))


@pytest.fixture(scope="module")
def tokenizer(q3, tmp_path_factory):
    from qwen3_rs_amd import tokenizer as tk
    from test_tokenizer_cli import make_tokenizer_json
    d = str(tmp_path_factory.mktemp("choice_tok"))
    n_vocab = make_tokenizer_json(d)
    path = os.path.join(d, "model.bin")
    tk.export_tokenizer(d, path, 1, 2)
    return tk.Tokenizer(path, n_vocab)


def test_rerank_builds_the_template_and_asks_for_no_and_yes(q3, tokenizer):
    tok = tokenizer
    docs = ["hello world", "world hello hello", "hell"]
    stub = _Stub([[0.0, 0.0], [1.0, 3.0], [800.0, 0.0]])
    got = q3.rerank(stub, tok, "hello?", docs, yes="hello", no="or")
    assert got.dtype == np.float64 and got.shape == (3,)
    assert got[0] == 0.5 and got[2] == 0.0 and abs(got[1] - 1.0 / (1.0 + np.exp(-2.0))) <= 2.0 ** -52
    (suffixes, cands, use_prefix), = stub.calls
    assert cands == tok.encode("or") + tok.encode("hello") and len(cands) == 2            # [no, yes]
    strings = [q3.RERANK_TEMPLATE.format(instruction=q3.RERANK_INSTRUCTION, query="hello?", document=d) for d in docs]
    head = ('<|im_start|>system\nJudge whether the Document meets the requirements based on the Query and the Instruct provided. '
            'Note that the answer can only be "yes" or "no".<|im_end|>\n<|im_start|>user\n'
            '<Instruct>: Given a web search query, retrieve relevant passages that answer the query\n<Query>: hello?\n<Document>: ')
    tail = "<|im_end|>\n<|im_start|>assistant\n<think>\n\n</think>\n\n"
    assert strings == [head + d + tail for d in docs]
    full = [tok.encode(s) for s in strings]                                               # whole strings, tokenized once each
    k = q3.common_prefix_len(full)
    assert use_prefix and stub.prefix == full[0][:k] and suffixes == [p[k:] for p in full]
    assert k >= len(tok.encode(head)) - 1 and full[0][0] == tok.str_lookup("<|im_start|>")
    # an instruction of the caller's takes the default's place
    stub2 = _Stub([[0.0, 0.0]] * 3)
    q3.rerank(stub2, tok, "q", docs, instruction="hello", yes="hello", no="or")
    own = tok.encode(q3.RERANK_TEMPLATE.format(instruction="hello", query="q", document=docs[0]))
    assert stub2.prefix + stub2.calls[0][0][0] == own


def test_rerank_refuses_answer_words_of_several_tokens(q3, tokenizer):
    assert len(tokenizer.encode("yes")) == 3
    with pytest.raises(ValueError):
        q3.rerank(_Stub([[0.0, 0.0]]), tokenizer, "q", ["d"])                            # "yes" is three byte tokens here
    with pytest.raises(ValueError):
        q3.rerank(_Stub([[0.0, 0.0]]), tokenizer, "q", ["d"], yes="hello", no="")


def test_the_command_line_knows_the_rerank_verb(q3):
    from qwen3_rs_amd import cli
    a = cli.build_parser().parse_args(["rerank", "model.bin", "-q", "what", "-d", "one", "-d", "two", "--instruct", "Given", "--yes", "Y", "--no", "N",
                                       "--streams", "4", "-c", "128", "-o", "out.npy"])
    assert (a.cmd, a.checkpoint, a.query, a.document, a.instruct) == ("rerank", "model.bin", "what", ["one", "two"], "Given")
    assert (a.yes, a.no, a.streams, a.context, a.output) == ("Y", "N", 4, 128, "out.npy")
    b = cli.build_parser().parse_args(["rerank", "model.bin", "-q", "what", "-d", "one"])
    assert (b.instruct, b.yes, b.no, b.output, b.context) == (None, "yes", "no", None, None)
