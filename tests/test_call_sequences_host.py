"""What the call sequences of tests/seq_model.py contain, asserted on the host: these are caps on what tests/test_call_sequences.py may
leave out, not measurements.  Every ordered pair of op kinds is adjacent somewhere, every grow-only buffer of the batched state is
re-allocated behind cached plans, a score chunk is the first user of a column-plan width, the score and choice calls have the shapes
at which their kernels take another path, the batched state is started over with other shapes, and the harness itself catches
injected leaks (run() over seq_model.FakeEngine, no GPU anywhere)."""
import pytest

import seq_model as sm


@pytest.fixture(scope="module")
def sequences(q3):
    return {seed: sm.make_sequence(seed) for seed in sm.SEEDS}


@pytest.fixture(scope="module")
def reference(q3, oracle, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("seq_host") / "m.bin")
    q3.checkpoint.write_synthetic_checkpoint(path, sm.shape(q3), seed=4321)
    return sm.Reference(oracle, path)


def test_the_generator_is_deterministic(q3):
    assert sm._sequence(sm.SEEDS[0], sm.N_OPS, frozenset()) == sm._sequence(sm.SEEDS[0], sm.N_OPS, frozenset())
    assert repr(sm.make_sequence(sm.SEEDS[1])) == repr(sm.make_sequence(sm.SEEDS[1]))
    assert eval(repr(sm.make_sequence(sm.SEEDS[1])[:40])) == sm.make_sequence(sm.SEEDS[1])[:40]          # the literal of a failure message


def test_every_kind_and_every_ordered_pair(sequences, capsys):
    assert len(sm.ILLEGAL) * 10 <= len(sm.ALL_PAIRS), "more than a tenth of the pairs are listed as illegal"
    assert set(sm.ILLEGAL) <= set(sm.ALL_PAIRS)
    count = {}
    for ops in sequences.values():
        assert all(o["op"] in sm.KINDS for o in ops)
        for a, b in zip(ops, ops[1:]):
            count[(a["op"], b["op"])] = count.get((a["op"], b["op"]), 0) + 1
    w = max(len(k) for k in sm.KINDS)
    with capsys.disabled():
        print(f"\nadjacent pairs over seeds {sm.SEEDS} (row: the op in front, columns in the same order; 9 = nine or more; '.' = illegal):")
        for a in sm.KINDS:
            print(f"{a:>{w}} " + " ".join("." if (a, b) in sm.ILLEGAL else str(min(count.get((a, b), 0), 9)) for b in sm.KINDS))
        print(f"{len(count)} of {len(sm.ALL_PAIRS)} pairs occur, {len(sm.ILLEGAL)} are illegal:")
        for (a, b), why in sorted(sm.ILLEGAL.items()):
            print(f"  {a} -> {b}: {why}")
    assert not set(count) & set(sm.ILLEGAL), sorted(set(count) & set(sm.ILLEGAL))
    missing = [p for p in sm.ALL_PAIRS if p not in count and p not in sm.ILLEGAL]
    assert not missing, f"{len(missing)} legal pairs never adjacent: {missing[:20]}"


def walk(ops):
    """per op: (epoch, what seq_model.needs says of it, the batched shape and samplers in front of it)"""
    streams = ctx = epoch = 0
    sampling, prefix_len = False, 0
    out = []
    for op in ops:
        k = op["op"]
        if k == "batch_init":
            epoch += 1
            streams, ctx, sampling, prefix_len = op["streams"], op["ctx"] or sm.SEQ, False, 0
        rows, stop = None, ()
        if k in ("generate_many_stop", "generate_many_prefix") and op["stop_at"]:
            # the stop loop's passes depend on the tokens; its buffers do not (cols_req, cols_prompts, cols_out by the request list)
            rows, stop = [[0] * sm.CAT[i][2] for i in op["reqs"]], (1,)
        out.append((epoch, sm.needs(op, streams, sampling, prefix_len, rows, stop) if not k.startswith("refused") else None, streams, ctx))
        if k == "set_batch_sampler_on":
            sampling = True
        elif k == "set_batch_sampler_off":
            sampling = False
        elif k == "batch_prefix_set":
            prefix_len = op["prompt"][1]
    return out


def test_every_grow_only_buffer_grows_twice_behind_cached_plans(sequences, capsys):
    for seed, ops in sequences.items():
        info = walk(ops)
        grown = {b: [] for b in sm.BUFFERS}
        best = {b: 0 for b in sm.BUFFERS}            # the largest need of the sequence so far
        cap = {}                                      # of the epoch: what the engine holds
        cols_built, dense_built, cols_hit, dense_hit = set(), set(), False, False
        last_epoch = 0
        for i, (epoch, nd, _, _) in enumerate(info):
            if epoch != last_epoch:
                cap, cols_built, dense_built, cols_hit, dense_hit, last_epoch = {}, set(), set(), False, False, epoch
            if nd is None:
                continue
            for b, n in nd["need"].items():
                if n > best[b] and cap.get(b, 0) > 0 and cols_hit and dense_hit:
                    # more than every earlier call of the sequence asked for, over a buffer this batched state holds already (freed and
                    # allocated again), behind plans that were cached while it was small -- and a smaller call of the same kind follows
                    later = [j for j in range(i + 1, len(ops)) if info[j][0] == epoch and ops[j]["op"] == ops[i]["op"] and info[j][1]
                             and 0 < info[j][1]["need"].get(b, 0) < n]
                    if later:
                        grown[b].append(i)
                best[b] = max(best[b], n)
                if b == "att_pf" and n > cap.get(b, 0):
                    dense_built = set()               # dense_att_grow drops the kept block plans
                cap[b] = max(cap.get(b, 0), n)
            cols_hit |= bool(nd["cols"] & cols_built)
            dense_hit |= bool(nd["dense"] & dense_built)
            cols_built |= nd["cols"]
            dense_built |= nd["dense"]
        with capsys.disabled():
            print(f"\nseed {seed}: calls that grow a buffer behind cached plans, a smaller one following: "
                  + ", ".join(f"{b} {len(v)}" for b, v in grown.items()), end="")
        for b, v in grown.items():
            assert len(v) >= 2, f"seed {seed}: {b} grows {len(v)} times ({v})"


def test_a_score_chunk_is_the_first_use_of_a_column_plan_width(sequences, capsys):
    """q3_score_many takes the column plan of a chunk's width with plan_get inside the walk's grow callback: per seed, a chunk's
    (non-draw, width) plan is one no earlier op of the epoch has used -- not the walk of the score op itself either -- and a column pass
    or narrow block of that width follows in the epoch, on the plan the chunk has made"""
    for seed, ops in sequences.items():
        info = walk(ops)
        built, last_epoch, found = set(), 0, []
        for i, (epoch, nd, _, _) in enumerate(info):
            if epoch != last_epoch:
                built, last_epoch = set(), epoch
            if nd is None:
                continue
            for key in sorted(nd.get("chunk_cols", set()) - built):
                later = [j for j in range(i + 1, len(ops)) if info[j][0] == epoch and info[j][1] and key in info[j][1]["cols"]
                         and key not in info[j][1].get("chunk_cols", ())]
                if later:
                    found.append((i, sm.WIDTHS[key[1]], later[0]))
            built |= nd["cols"]
        with capsys.disabled():
            print(f"\nseed {seed}: (score op, width first used by its chunk, the first column pass of that width behind it): {found}", end="")
        assert found, seed


def test_score_and_choice_shapes(sequences):
    scored, skipped, gathered, wide_scored = set(), 0, 0, set()
    drawn_behind = per_request_parts = False
    ks, froms = set(), set()
    for seed, ops in sequences.items():
        info = walk(ops)
        sampling = False
        for i, op in enumerate(ops):
            k = op["op"]
            if k in sm.SCORE:
                streams = info[i][2]
                for _, wide, cols in sm.score_blocks(op, streams):
                    scored.add(len(cols))
                    if wide:
                        wide_scored.add(len(cols))
                chunks = sm.score_chunks(op, streams)
                skipped += sum(1 for _, same in chunks if same)
                gathered += sum(1 for _, same in chunks if not same)
                nxt = ops[i + 1]["op"] if i + 1 < len(ops) else None
                drawn_behind |= sampling and (nxt in sm.NEED_DRAWS or nxt == "batch_step_cols_draw")
                lens, _ = sm.op_requests(op)
                for n, f in zip(lens, op["score_from"] or [1] * len(lens)):
                    froms |= {"one token"} if n == 1 else {"1"} if f == 1 else {"n"} if f == n else {"n - 1"} if f == n - 1 else {"between"}
            if k in sm.CHOICE:
                ks.add(op["cand"][0])
                per_request_parts |= op["cand"][1] and op["cand"][0] > sm.CHOICE_PART
                flat = sm.flat_candidates(op)
                assert all(0 <= t < sm.VOCAB for t in flat)
                for row in (sm.candidates(op) if op["cand"][1] else [flat]):
                    assert len(row) == op["cand"][0]
                    if len(row) >= 2:
                        assert 0 in row and sm.VOCAB - 1 in row
                    if len(row) >= 5:
                        assert len(set(row)) < len(row)
            if k == "set_batch_sampler_on":
                sampling = True
            elif k in ("set_batch_sampler_off", "batch_init"):
                sampling = False
    # chunk edges behind dense blocks: one chunk short of full, one full, a full one and a chunk of one, three or more
    assert {31, 32, 33} <= wide_scored and max(wide_scored) >= 65, sorted(wide_scored)
    assert {31, 32, 33} <= scored
    assert skipped and gathered, (skipped, gathered)
    assert drawn_behind, "no score op under a sampling batch with a drawing op right behind it"
    assert {1, 2, 5, 33, 70} <= ks and per_request_parts, ks
    assert froms == {"one token", "1", "n", "n - 1", "between"}, froms


def test_state_changes(sequences):
    # the sequence that also runs on the edge-valued checkpoint holds both new calls, under a prefix too
    assert {"choice_many", "score_many", "choice_many_prefix", "score_many_prefix"} <= {o["op"] for o in sequences[sm.EDGE_SEED]}
    for seed, ops in sequences.items():
        inits = [o for o in ops if o["op"] == "batch_init"]
        assert ops[0]["op"] == "batch_init"
        assert sum(a["streams"] != b["streams"] for a, b in zip(inits, inits[1:])) >= 2, seed
        assert sum((a["ctx"] or sm.SEQ) != (b["ctx"] or sm.SEQ) for a, b in zip(inits, inits[1:])) >= 1, seed
        kinds = [o["op"] for o in ops]
        flips = [k for k in kinds if k in ("set_batch_sampler_on", "set_batch_sampler_off", "batch_init")]
        on_off = sum(1 for a, b in zip(flips, flips[1:]) if a == "set_batch_sampler_on" and b == "set_batch_sampler_off")
        assert on_off >= 2 and kinds.count("set_batch_sampler_on") >= 2, (seed, on_off)
        # a dense call (a wide block) in front of a q3_batch_init and behind it: dense_cap is fixed twice
        wide = [bool(nd and nd["dense"]) for _, nd, _, _ in walk(ops)]
        at = [i for i, k in enumerate(kinds) if k == "batch_init"][1:]
        assert any(any(wide[:i]) and any(wide[i:]) for i in at), seed
        # sizes go small - large - small - larger - small
        sizes = [len(o["reqs"]) for o in ops if o["op"] in sm.MANY]
        assert min(sizes) <= 3 and max(sizes) >= 50 and sizes[-1] <= 3
        for kind in ("choice_many", "score_many"):
            sizes = [len(o["reqs"]) for o in ops if o["op"] == kind]
            big = [i for i, n in enumerate(sizes) if n >= 18]
            assert sizes[0] <= 3 and sizes[-1] <= 3 and max(sizes) >= 50, (seed, kind, sizes)
            assert any(sizes[i] < 50 and any(n <= 3 for n in sizes[i:j]) and sizes[j] >= 50 for i in big for j in big if j > i), (seed, kind, sizes)
        assert max(sm.CAT[i][1] for o in ops if o["op"] in sm.MANY for i in o["reqs"]) == 120


def test_the_harness_passes_the_fake_engine_and_catches_the_leaks(sequences, reference, capsys):
    for seed, ops in sequences.items():
        sm.run(sm.FakeEngine(reference), ops, reference, seed)
    with capsys.disabled():
        print(f"\n{reference.forwards} oracle forwards for {sum(len(o) for o in sequences.values())} ops")
    for leak in sm.LEAKS:
        caught = {}
        for seed, ops in sequences.items():
            try:
                sm.run(sm.FakeEngine(reference, leak=leak), ops, reference, seed)
            except AssertionError as err:
                msg = str(err)
                assert msg.startswith(f"seed {seed}, engine 0, op ") and "\nops = [" in msg
                at = int(msg.split("op ")[1].split(" ")[0])
                assert eval(msg.split("\nops = ")[1]) == ops[:at + 1]             # the literal reproduces the sequence up to the failure
                caught[seed] = (at, ops[at]["op"])
                # the first op at which the leaked state can be observed through the API, and no earlier.  A carried sampler state
                # shows only where it draws another token than the seed would: at that op or at a later one of the same kind
                first = first_visible(leak, ops)
                assert at == first or (leak == "sampler" and at > first and ops[at]["op"] == "generate_many_sampled"), \
                    f"leak {leak!r}, seed {seed}: reported at op {at}, visible from op {first}"
        with capsys.disabled():
            print(f"leak {leak!r} caught at (op, kind) per seed: {caught}")
        assert caught, f"leak {leak!r} passes on every seed"
        if leak in ("slot_rng", "stale_cand"):       # caught on every seed that can show it
            assert set(caught) == {seed for seed, ops in sequences.items() if first_visible(leak, ops) is not None}, leak


def first_visible(leak, ops):
    """the first op behind which state that leaked is observable through the API"""
    if leak == "prefix":         # q3_batch_prefix_get behind the first q3_batch_init with a prefix resident
        resident = False
        for i, o in enumerate(ops):
            if o["op"] == "batch_init" and resident:
                return i
            resident = (resident or o["op"] == "batch_prefix_set") and o["op"] != "batch_init"
    if leak == "length":         # the first batch_reset_kv over a slot that holds rows
        filled = False
        for i, o in enumerate(ops):
            if o["op"] == "batch_reset_kv" and filled:
                return i
            if o["op"] == "batch_init":
                filled = False
            elif not o["op"].startswith(("refused", "set_")) and o["op"] not in ("batch_reset_kv", "reset_kv", "forward", "generate_greedy",
                                                                                   "prefill_batched", "verify", "verify_draw", "generate_lookup",
                                                                                   "generate_lookup_draw"):
                filled = True
    if leak == "sampler":        # the first generate_many_sampled in which a sampled request enters a slot that a sampled request has left
                                 # a state in: one of an earlier call, or the slot's occupant in front of it in the same call
        state, streams = set(), 0
        for i, o in enumerate(ops):
            if o["op"] == "batch_init":
                state, streams = set(), o["streams"]
            if o["op"] == "generate_many_sampled":
                lens, n_new = sm.op_requests(o)
                occ = sm.many_plan(lens, n_new, streams)["occupants"]
                sampled = {s: [r for r in rs if sm.CAT[o["reqs"][r]][3] > 0] for s, rs in occ.items()}
                if any(rs and (s in state or len(rs) > 1) for s, rs in sampled.items()):
                    return i
                state |= {s for s, rs in sampled.items() if rs}
    if leak == "stale_cand":     # the first choice call whose candidates differ from the previous one's at an index both have
        prev = []
        for i, o in enumerate(ops):
            if o["op"] == "batch_init":
                prev = []
            if o["op"] in sm.CHOICE:
                flat = sm.flat_candidates(o)
                if any(a != b for a, b in zip(flat, prev)):
                    return i
                prev = flat
    if leak == "slot_rng":       # the first op that draws from a slot's known state behind a choice or score call on that slot
        moved, streams, sampling = set(), 0, False
        for i, o in enumerate(ops):
            k = o["op"]
            if k in ("batch_init", "set_batch_sampler_on", "set_batch_sampler_off"):
                moved, sampling = set(), k == "set_batch_sampler_on"
                streams = o["streams"] if k == "batch_init" else streams
            elif k in sm.CHOICE + sm.SCORE:
                moved |= set(range(min(len(o["reqs"]), streams)))
            elif sampling and k in sm.NEED_DRAWS + ("batch_step_cols_draw",):
                if moved & set(o["slots"] if k == "batch_step_cols_draw" else range(len(o.get("tokens") or o["first"]))):
                    return i
    return None
