"""The batched engine under call sequences (tests/seq_model.py): every public call that touches the shared BatchCtx -- its shared plan,
its cached column and dense plans with their graphs, its grow-only device buffers, its allocate-on-first-use blocks -- in seeded
orders in which every kind of call follows every other, the buffers grow behind cached plans and the batched state is started over
with other shapes.  After every op its outputs are compared with the C oracle (logits and embeddings bit for bit), every cache the op
does not name with a copy taken before it, and the rows it fills with the oracle's.  tests/test_call_sequences_host.py holds the
sequences to what they have to contain.
The settings sequences (seq_model.SETTING_KINDS) put the engine-wide settings of sections 2m to 2q -- top_k, gen_logprobs, penalties,
the logit-bias table -- among those calls: every loop op runs under the settings in force, its records are read and held to the
reference behind it, and the four getters are compared after every op.
The guide sequences (seq_model.GUIDE_KINDS) add the dense guide of section 2r, the sparse guide of 2s and the stop automaton of 2t:
every loop op runs under the automata in force -- tokens, n_out, the -1 fill behind the last token, the stats of
q3_cols_schedule(prompt_len, n_emit), the records on the raw row and the rng state are the reference's -- the arrays grow behind
cached plans, each guide form replaces the other under kept plans, the batched state is started over under both, and the three
getters are compared after every op."""
import numpy as np
import pytest

import edge_ckpt
import seq_model as sm

pytestmark = pytest.mark.gpu

EDGE_SEED = sm.EDGE_SEED          # the seed that also runs on the edge-valued checkpoint (tests/test_call_sequences_host.py: it holds
                                  # choice_many and score_many; tied classifier rows make the score argmax the odd row there)


@pytest.fixture(scope="module")
def models(q3, oracle, tmp_path_factory):
    """edit -> (checkpoint path, Reference): one synthetic checkpoint of the shape and its `all` edit, one oracle trie each, shared by
    every case and never changed"""
    made = {}

    def get(edit=None):
        if edit not in made:
            path = str(tmp_path_factory.mktemp("seq") / f"{sm.NAME}-{edit}.bin")
            shape = sm.shape(q3)
            q3.checkpoint.write_synthetic_checkpoint(path, shape, seed=edge_ckpt.SEED if edit else 4321)
            if edit:
                mm = np.memmap(path, dtype=np.uint8, mode="r+")
                for fn in edge_ckpt.EDITS[edit]:
                    fn(mm, shape)
                mm.flush()
                del mm
            made[edit] = (path, sm.Reference(oracle, path))
        return made[edit]
    return get


def engine(q3, path, graph=True):
    b = q3.TransformerBuilder(path).with_ctx_length(sm.SEQ)
    return (b if graph else b.with_graph(False)).build()


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("seed", sm.SEEDS)
def test_sequence(q3, models, seed, graph):
    path, ref = models()
    with engine(q3, path, graph) as t:
        sm.run(t, sm.make_sequence(seed), ref, seed)


def test_sequence_on_an_edge_valued_checkpoint(q3, models):
    path, ref = models("all")
    with engine(q3, path) as t:
        sm.run(t, sm.make_sequence(EDGE_SEED), ref, EDGE_SEED)


def test_two_engines_interleaved_op_by_op(q3, models):
    """test_two_engines_are_independent taken to the batched state: the same sequence on two engines of one process, op by op in turn"""
    path, ref = models()
    seed = sm.SEEDS[-1]
    with engine(q3, path) as a, engine(q3, path, graph=False) as b:
        sm.run([a, b], sm.make_sequence(seed), ref, seed)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("seed", sm.SETTING_SEEDS)
def test_settings_sequence(q3, models, seed, graph):
    path, ref = models()
    with engine(q3, path, graph) as t:
        sm.run(t, sm.make_settings_sequence(seed), ref, seed)


def test_settings_sequence_on_an_edge_valued_checkpoint(q3, models):
    """tied classifier rows: the ties go to the higher index in the argmax key of a penalised or adjusted row, among the top-k
    survivors and in the tops of the records alike"""
    path, ref = models("all")
    with engine(q3, path) as t:
        sm.run(t, sm.make_settings_sequence(sm.SETTING_EDGE_SEED), ref, sm.SETTING_EDGE_SEED)


def test_settings_on_two_engines_interleaved_op_by_op(q3, models):
    """the settings are an engine's own: the same settings sequence on two engines of one process, one with graphs and one without"""
    path, ref = models()
    seed = sm.SETTING_SEEDS[-1]
    with engine(q3, path) as a, engine(q3, path, graph=False) as b:
        sm.run([a, b], sm.make_settings_sequence(seed), ref, seed)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("seed", sm.GUIDE_SEEDS)
def test_guide_sequence(q3, models, seed, graph):
    path, ref = models()
    with engine(q3, path, graph) as t:
        sm.run(t, sm.make_guide_sequence(seed), ref, seed)


def test_guide_sequence_on_an_edge_valued_checkpoint(q3, models):
    """tied classifier rows meet the -inf keys of the mask: among the allowed tokens the ties go to the higher index, and a row with
    no finite entry commits V - 1"""
    path, ref = models("all")
    with engine(q3, path) as t:
        sm.run(t, sm.make_guide_sequence(sm.GUIDE_EDGE_SEED), ref, sm.GUIDE_EDGE_SEED)


def test_guides_on_two_engines_interleaved_op_by_op(q3, models):
    """the guide and the stop automaton are an engine's own: the same guide sequence on two engines of one process, one with graphs
    and one without"""
    path, ref = models()
    seed = sm.GUIDE_SEEDS[-1]
    with engine(q3, path) as a, engine(q3, path, graph=False) as b:
        sm.run([a, b], sm.make_guide_sequence(seed), ref, seed)
