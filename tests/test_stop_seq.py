"""Stop sequences in the device loop (include/qwen3_hip.h section 2t): q3_generate_many_stop and q3_generate_many_prefix under a
stop automaton.  A request that ends where a sequence is complete is a request with n_new = n_emit, so the yardstick is the
existing loop -- generate_many_greedy / generate_many_sampled -- called at the cap for the tokens and with n_new = n_emit for the
passes, and nothing here has a tolerance.

The synthetic checkpoints emit nothing on purpose: stop_seq_ref.pick_stop_seqs chooses the stop list from the rows at the cap and
check_pick asserts its conditions: a one-token sequence ends a request at y_0; a sequence of two tokens ends a request inside its
row, its tokens in different passes; a request never ends; passes are saved; and a RESET sequence -- the last token at the cap of a
request that never ends, then y_0 of the request that takes its slot next, found nowhere contiguously -- under which the next
occupant must not end at y_0.  Checked with the CPU oracle for the checkpoint seed and prompts used here (two-token reset
sequences suffice everywhere):
  tiny-g64    greedy   [[82], [187, 123], [244, 398]]      n_emit 2, 10, 10, 1, 10, 10, 10    reset: slot 1, request 1 then 5; 11 passes saved
  tiny-g64    sampled  [[49], [187, 123], [162, 180]]      n_emit 2, 10, 1, 10, 10, 10, 10    reset: slot 0, request 4 then 6;  8 passes saved
  small-hd128 greedy   [[11], [1717, 404], [861, 1660]]    n_emit 2, 10, 1, 10, 10, 10, 10    reset: slot 0, request 4 then 6;  8 passes saved
  small-hd128 sampled  [[834], [1717, 404], [1384, 1704]]  n_emit 2, 1, 10, 10, 10, 10, 10    reset: slot 0, request 4 then 6;  8 passes saved
  qwen3-4b-dims-l2 sampled (ctx 512)  [[466], [2614, 8906], [15575, 2894]]  n_emit 2, 10, 10, 10, 10, 1, 10  reset: slot 1, request 1 then 4;  9 passes saved"""
import ctypes as C

import numpy as np
import pytest

import cols_sim
import stop_seq_ref as ref
from cols_stop_cases import CAP, CKPT_SEED, PROMPT_LEN, SEEDS, SHAPES, SLOTS, TEMPERATURE, TOPP, n_emit_of, prompts
from conftest import assert_biteq

pytestmark = pytest.mark.gpu

SAMPLER = (list(TEMPERATURE), TOPP, list(SEEDS))
N = len(PROMPT_LEN)
NAMES = ["tiny-g64", "small-hd128"]
PREFIX = {"tiny-g64": 7, "small-hd128": 33}


class Model:
    """One synthetic checkpoint, its requests and what the existing loops make of them at the cap: computed once, never changed."""

    def __init__(self, q3, name, path):
        self.q3, self.name, self.path, self.ctx = q3, name, path, SHAPES[name]
        self.shape = q3.checkpoint.SHAPES[name]
        q3.checkpoint.write_synthetic_checkpoint(path, self.shape, seed=CKPT_SEED)
        self.V = self.shape.vocab_size
        self.prompts = prompts(self.V)
        self._at_cap = {}

    def batch_engine(self, slots=SLOTS):
        t = self.q3.TransformerBuilder(self.path).with_ctx_length(self.ctx or None).build()
        t.batch_init(slots)
        return t

    def at_cap(self, sampled):
        """(rows of the existing loop at the cap, the stop list picked from them, n_emit)"""
        if sampled not in self._at_cap:
            with self.batch_engine() as t:
                rows, stats = (t.generate_many_sampled(self.prompts, [CAP] * N, *SAMPLER) if sampled
                               else t.generate_many_greedy(self.prompts, [CAP] * N))
            assert stats.passes == cols_sim.schedule(PROMPT_LEN, [CAP] * N, SLOTS)[1].passes
            got = ref.pick_stop_seqs(rows)
            assert got is not None, f"no stop list ends the rows in every way: {rows}"
            ref.check_pick(rows, *got)
            self._at_cap[sampled] = (rows, got[0], got[1])
        return self._at_cap[sampled]

    def automaton(self, seqs):
        return self.q3.stop_automaton(seqs, self.V)


@pytest.fixture(scope="module")
def models(q3, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Model(q3, name, str(tmp_path_factory.mktemp("stopseq") / f"{name}.bin"))
        return made[name]
    return get


def tup(stats):
    return (stats.passes, stats.live_columns, stats.prompt_columns, stats.decode_columns)


def check_call(t, m, stop_tokens, sampler, rows, emit, what, fn=None, prompts_=None):
    """one call of the stop loop against the rows at the cap: tokens up to the cut, n_out, -1 behind; returns the stats"""
    fn = fn or t.generate_many_stop
    out, n_out, stats = fn(m.prompts if prompts_ is None else prompts_, [CAP] * N, stop_tokens, sampler, raw=True)
    assert n_out == emit, what
    for r in range(N):
        got = out[r * CAP:(r + 1) * CAP]
        assert got[:emit[r]] == rows[r][:emit[r]], f"{what}: request {r}"
        assert got[emit[r]:] == [-1] * (CAP - emit[r]), f"{what}: request {r} behind its last token"
    return stats


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("name", NAMES)
def test_equals_the_loop_with_n_emit(q3, models, name, sampled):
    """with n_stop == 0: the automaton alone ends the requests.  The reset case is among them: the slot's previous occupant left
    it mid-match and the next one starts from its own start state"""
    m = models(name)
    rows, seqs, emit = m.at_cap(sampled)
    sampler = SAMPLER if sampled else None
    _, wstats = cols_sim.schedule(PROMPT_LEN, emit, SLOTS)
    with m.batch_engine() as t:
        t.set_stop_sequences(m.automaton(seqs))
        for k in range(2):                                   # the second call finds the slots' states as the first left them
            stats = check_call(t, m, [], sampler, rows, emit, f"call {k}")
            assert tup(stats) == tuple(wstats)
        want, lstats = t.generate_many_sampled(m.prompts, emit, *SAMPLER) if sampled else t.generate_many_greedy(m.prompts, emit)
        assert want == [r[:e] for r, e in zip(rows, emit)]
        assert tup(lstats) == tuple(wstats)
        cut, cstats = t.generate_many_stop(m.prompts, [CAP] * N, [], sampler)
        assert cut == want and tup(cstats) == tuple(wstats)
        # the loops without a device scheduler do not read the setting
        full, fstats = t.generate_many_sampled(m.prompts, [CAP] * N, *SAMPLER) if sampled else t.generate_many_greedy(m.prompts, [CAP] * N)
        assert full == rows and fstats.passes == cols_sim.schedule(PROMPT_LEN, [CAP] * N, SLOTS)[1].passes


@pytest.mark.parametrize("name", NAMES)
def test_sequences_and_stop_tokens_together(q3, models, name):
    """the earlier of the two ends the request"""
    m = models(name)
    for sampled in (False, True):
        rows, seqs, emit = m.at_cap(sampled)
        never = [r for r in range(N) if emit[r] == CAP]
        inner = next(r for r in range(N) if 1 < emit[r] < CAP)
        # a stop token in front of the sequence's last token in one request, and in the middle of a request no sequence ends
        stop = sorted({rows[inner][0], rows[never[0]][4]})
        both = ref.n_emit_rows(rows, seqs, stop)
        assert both[inner] == 1 < emit[inner] and both[never[0]] <= 5 and both != emit and both != n_emit_of(rows, stop)
        with m.batch_engine() as t:
            t.set_stop_sequences(m.automaton(seqs))
            stats = check_call(t, m, stop, SAMPLER if sampled else None, rows, both, "sequences and stop tokens")
            assert tup(stats) == tuple(cols_sim.schedule(PROMPT_LEN, both, SLOTS)[1])


@pytest.mark.parametrize("name", NAMES)
def test_per_request_starts(q3, models, name):
    """start -1: that request has no stop sequences and runs to the cap"""
    m = models(name)
    rows, seqs, emit = m.at_cap(False)
    ended = [r for r in range(N) if emit[r] < CAP]
    starts = [0] * N
    starts[ended[0]] = -1
    want = ref.n_emit_rows(rows, seqs, (), starts)
    assert want[ended[0]] == CAP and want[ended[1]] == emit[ended[1]] < CAP
    with m.batch_engine() as t:
        t.set_stop_sequences(m.automaton(seqs), starts)
        stats = check_call(t, m, [], None, rows, want, "per-request starts")
        assert tup(stats) == tuple(cols_sim.schedule(PROMPT_LEN, want, SLOTS)[1])
        t.set_stop_sequences(m.automaton(seqs), [-1] * N)
        stats = check_call(t, m, [], None, rows, [CAP] * N, "every request opts out")
        assert tup(stats) == tuple(cols_sim.schedule(PROMPT_LEN, [CAP] * N, SLOTS)[1])
        # another number of requests than start states: refused like a guide
        with pytest.raises(IndexError, match="q3_stop_seq_set holds"):
            t.generate_many_stop(m.prompts[:3], [CAP] * 3, [])
        with pytest.raises(IndexError, match="q3_stop_seq_set holds"):
            t.generate_many_greedy(m.prompts[:3], [CAP] * 3)


@pytest.mark.parametrize("name", NAMES)
def test_through_the_prefix_loop(q3, models, name):
    """suffixes behind a resident prefix: the automaton sees generated tokens only, and with n_stop == 0 the call takes the stop loop"""
    m = models(name)
    P = PREFIX[name]
    prefix = [int(t) for t in np.random.default_rng(5200).integers(0, m.V, P)]
    for sampled in (False, True):
        sampler = SAMPLER if sampled else None
        with m.batch_engine() as t:
            t.batch_prefix_set(prefix)
            rows, stats = t.generate_many_prefix(m.prompts, [CAP] * N, [], sampler)          # today's path: no automaton, the tabled loop
            assert stats.passes == cols_sim.schedule(PROMPT_LEN, [CAP] * N, SLOTS)[1].passes
            # a one-token sequence from some y_0, a two-token sequence from inside another row, and one made of the prefix's last
            # token and a y_0 that would match only if prompt tokens moved the state
            a = next(r for r in range(N) if rows[r][1:3] != [rows[r][0]] * 2)
            b = next(r for r in range(N) if r != a and rows[r][0] != rows[a][0])
            seqs = [[rows[b][0]], rows[a][1:3]]
            lure = [prefix[-1], rows[a][0]]
            if not ref.occurs(rows, lure) and lure not in seqs:
                seqs.append(lure)
            emit = ref.n_emit_rows(rows, seqs)
            assert emit[b] == 1 and 1 < emit[a] <= 3 and any(e == CAP for e in emit)
            t.set_stop_sequences(m.automaton(seqs))
            wstats = cols_sim.schedule(PROMPT_LEN, emit, SLOTS)[1]
            for k in range(2):
                stats = check_call(t, m, [], sampler, rows, emit, f"prefix call {k}", fn=t.generate_many_prefix)
                assert tup(stats) == tuple(wstats)
            # ... and the full prompts through the stop loop give the same rows
            full = [prefix + p for p in m.prompts]
            if max(len(p) for p in full) + CAP - 1 <= t._batch_ctx:
                check_call(t, m, [], sampler, rows, emit, "full prompts", prompts_=full)


@pytest.mark.parametrize("name", NAMES)
def test_set_clear_set_again(q3, models, name):
    m = models(name)
    rows, seqs, emit = m.at_cap(False)
    srows, sseqs, semit = m.at_cap(True)
    stop = [rows[4][2]]
    today = n_emit_of(rows, stop)
    L = q3.load_library()
    with m.batch_engine() as t:
        assert t.get_stop_sequences() == (None, [])
        before = check_call(t, m, stop, None, rows, today, "no automaton yet")
        a = m.automaton(seqs)
        t.set_stop_sequences(a)
        assert t.get_stop_sequences() == (a, [0])
        check_call(t, m, [], None, rows, emit, "set")
        # a refused call changes nothing
        sz = C.c_size_t
        bad = np.array([a.n_states], dtype=np.int32)
        rc = L.q3_stop_seq_set(t._h, a.default.ctypes.data_as(C.c_void_p), a.offsets.astype(np.uint32).ctypes.data_as(C.c_void_p), None, a.n_states, 0, m.V,
                               bad.ctypes.data_as(C.POINTER(C.c_int32)), 1)
        assert rc == -3
        with pytest.raises(q3.Q3Error, match="vocab_size") as ei:
            t.set_stop_sequences(q3.stop_automaton(seqs, m.V + 1))
        assert ei.value.code == -3
        ns, ne, nst = sz(0), sz(0), sz(0)
        assert L.q3_stop_seq_get(t._h, C.byref(ns), C.byref(ne), C.byref(nst)) == 0 and (ns.value, ne.value, nst.value) == (a.n_states, a.n_edges, 1)
        check_call(t, m, [], None, rows, emit, "behind a refused set")
        t.set_stop_sequences(None)
        assert t.get_stop_sequences() == (None, [])
        after = check_call(t, m, stop, None, rows, today, "cleared")
        assert tup(after) == tup(before) == tuple(cols_sim.schedule(PROMPT_LEN, today, SLOTS)[1])
        check_call(t, m, [], None, rows, [CAP] * N, "cleared, no stop list")
        t.set_stop_sequences(m.automaton(sseqs))                                  # another automaton: its tables replace the first
        check_call(t, m, [], SAMPLER, srows, semit, "set again, sampled")
        t.set_stop_sequences(a)
        check_call(t, m, [], None, rows, emit, "and the first again")
        t.batch_init(SLOTS)                                                       # the setting is the engine's: a new batched state uploads it again
        check_call(t, m, [], None, rows, emit, "behind batch_init")


@pytest.mark.parametrize("name", NAMES)
def test_beside_a_dense_guide_and_logprobs(q3, models, name):
    """rows and records up to n_emit equal those without the automaton"""
    m = models(name)
    rows, _, _ = m.at_cap(False)
    # a dense guide of two states that forbids every row's y_0 and y_2 in both: the guided rows differ from the unguided ones
    nxt = np.zeros((2, m.V), dtype=np.int16)
    nxt[0, :] = 1
    nxt[:, sorted({r[0] for r in rows} | {r[2] for r in rows})] = -1
    with m.batch_engine() as t:
        t.set_guide(nxt, 0)
        t.set_gen_logprobs(2)
        grows, _ = t.generate_many_stop(m.prompts, [CAP] * N, [])
        assert all(g[0] != r[0] for g, r in zip(grows, rows))
        grecs = t.read_gen_logprobs()
        a = next(r for r in range(N) if grows[r][1:3] != [grows[r][0]] * 2)
        seqs = [grows[a][1:3]] + [[grows[b][0]] for b in range(N) if b != a and grows[b][0] != grows[a][0]][:1]
        emit = ref.n_emit_rows(grows, seqs)
        assert 1 < emit[a] <= 3 and 1 in emit and CAP in emit
        t.set_stop_sequences(m.automaton(seqs))
        stats = check_call(t, m, [], None, grows, emit, "guide, logprobs and automaton")
        assert tup(stats) == tuple(cols_sim.schedule(PROMPT_LEN, emit, SLOTS)[1])
        recs = t.read_gen_logprobs()
        for r in range(N):
            for got, want, what in zip(recs[r], grecs[r], ("records", "tops", "ranks")):
                assert len(got) == emit[r]
                assert got.tobytes() == want[:emit[r]].tobytes(), f"request {r}: {what}"


class Tok:
    """a tokenizer of the test's own: token v spells <v>"""

    def __init__(self, V):
        self.vocab = [f"<{v}>".encode() for v in range(V)]


@pytest.mark.parametrize("name", NAMES)
def test_generate_many_front_end(q3, models, name):
    m = models(name)
    tk = Tok(m.V)
    with m.batch_engine() as t:
        for sampled in (False, True):
            rows, seqs, emit = m.at_cap(sampled)
            sampler = SAMPLER if sampled else None
            cap_passes = cols_sim.schedule(PROMPT_LEN, [CAP] * N, SLOTS)[1].passes
            # token lists
            want, wstats = q3.generate_many(t, m.prompts, CAP, stop=seqs, sampler=sampler)
            got, stats = q3.generate_many(t, m.prompts, CAP, stop=seqs, sampler=sampler, stop_on_device=True)
            assert got == want == [r[:e] for r, e in zip(rows, emit)]
            assert wstats.passes == cap_passes > stats.passes == cols_sim.schedule(PROMPT_LEN, emit, SLOTS)[1].passes
            # strings: the sequences spelled out, the two-token one cut inside its second token -- it ends mid-token
            strings = ["".join(f"<{v}>" for v in q) for q in seqs]
            strings[1] = strings[1][:-2]
            semit = [ref.n_emit_strings(r, tk.vocab, strings) for r in rows]
            assert all(s <= e for s, e in zip(semit, emit)) and semit[[i for i, e in enumerate(emit) if 1 < e < CAP][0]] > 1
            want, _ = q3.generate_many(t, m.prompts, CAP, stop=strings, tokenizer=tk, sampler=sampler)
            got, stats = q3.generate_many(t, m.prompts, CAP, stop=strings, tokenizer=tk, sampler=sampler, stop_on_device=True)
            assert got == want == [r[:e] for r, e in zip(rows, semit)]
            assert stats.passes == cols_sim.schedule(PROMPT_LEN, semit, SLOTS)[1].passes
            # per request, with stop tokens beside them
            per = [None if r % 2 else seqs for r in range(N)]
            stop_tokens = [rows[1][3]]
            both = ref.n_emit_rows(rows, seqs, stop_tokens, [-1 if r % 2 else 0 for r in range(N)])
            want, _ = q3.generate_many(t, m.prompts, CAP, stop_tokens=stop_tokens, stop=per, sampler=sampler)
            got, stats = q3.generate_many(t, m.prompts, CAP, stop_tokens=stop_tokens, stop=per, sampler=sampler, stop_on_device=True)
            assert got == want == [r[:e] for r, e in zip(rows, both)]
            assert stats.passes == cols_sim.schedule(PROMPT_LEN, both, SLOTS)[1].passes
            assert t.get_stop_sequences() == (None, [])                           # put back
        assert q3.cut_at_stop("<1><22><3>", ["<22>", "<3>"]) == "<1>"
        with pytest.raises(ValueError):
            q3.generate_many(t, m.prompts, CAP, stop=m.at_cap(False)[1], stop_on_device=True, dense_min=8)


def test_sampled_on_4b_dims(q3, models):
    """the real layer dimensions and a vocabulary of 16,384 at a context of 512, under the samplers"""
    m = models("qwen3-4b-dims-l2")
    rows, seqs, emit = m.at_cap(True)
    with m.batch_engine() as t:
        t.set_stop_sequences(m.automaton(seqs))
        stats = check_call(t, m, [], SAMPLER, rows, emit, "4b dims")
        assert tup(stats) == tuple(cols_sim.schedule(PROMPT_LEN, emit, SLOTS)[1])
