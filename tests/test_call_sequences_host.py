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


# ---------------------------------------------------------------------------------------------------------------------------------
# the settings dimension (include/qwen3_hip.h sections 2m to 2q): seq_model.SETTING_KINDS among the kinds above
# ---------------------------------------------------------------------------------------------------------------------------------
DIGESTS = {     # sha256 of repr(make_sequence(seed)), taken on the commit in front of the settings dimension: the pair matrix is what it was
    11: "4d26709c8664306e778e3935a9a79ee3731cc9791167a553be0de85ea8850acf", 12: "8f61442e23a555efdbcb9cddb7762a2497c88d289fd50912a62fcd5aff472bb8",
    13: "41e7a79d99faddfde6dccaa81fc0af81896052396cb734edf1c8c9369becd5e1", 14: "9e9d1748b9ba0c5cda6ffca017c83244765417bbeac585650c41272d55c6fd8e",
    15: "cdd530f7a7bfb5e54d4f0b486f339f23bd39a643dd461f38ec7abbe62938ac64", 16: "b91985aa91249373f3ba4a5d1eabdf76506eedb2caa2367134fe9ed169b9ce7c",
    17: "c91d2c4bb98a9e2f2e4161cf204c7b6c21af20c35f82527b8ee6682fba607353", 18: "c4f859fa9092c7a6d09daf99028cbc6106ddec695abd20795bb40f1e0931eda7",
    19: "1392baa1e8b453a6a9db6f560c4598440b3e550b45983f7c7311e2280f296702", 20: "e73478e01c08389f201268a7551a82724fdcb88d09bf41823c700a34844c6c16",
    21: "662ba61668959c62606c6c8a938bf95aea9c3755c4601b1d409a32c3db9874fb", 22: "561bf964657cec81481be031f1421f812d180a565c4d69e42fe5d84440b55f30",
}
SETTINGS = ("top_k", "genlp", "pen", "bias")


def test_the_twelve_sequences_are_what_they_were(sequences):
    import hashlib
    assert set(DIGESTS) == set(sm.SEEDS)
    for seed, ops in sequences.items():
        assert hashlib.sha256(repr(ops).encode()).hexdigest() == DIGESTS[seed], seed
    assert not set(sm.SETTING_KINDS) & set(sm.KINDS) and len(sm.CAT) == 115 and len(sm.KINDS) == 45
    assert [c[2] for c in sm.CAT[91:]] and all(6 <= c[2] <= 12 and 2 <= c[1] <= 40 for c in sm.CAT[91:])
    assert {2, 40} <= {c[1] for c in sm.CAT[91:]}


@pytest.fixture(scope="module")
def ssequences(q3):
    return {seed: sm.make_settings_sequence(seed) for seed in sm.SETTING_SEEDS}


def swalk(ops):
    """per op: dict(epoch, st = the settings in force in front of it, on = the settings that are on, nd = seq_model.needs with the
    forms of a loop op, streams, draw = a loop op runs sampled plans)"""
    st = sm.settings_walk(ops)
    streams = epoch = 0
    sampling, prefix_len = False, 0
    out = []
    for i, op in enumerate(ops):
        k = op["op"]
        before = streams
        if k == "batch_init":
            epoch += 1
            streams, sampling, prefix_len = op["streams"], False, 0
        rows, stop = None, ()
        if k in ("generate_many_stop", "generate_many_prefix") and op["stop_at"]:
            rows, stop = [[0] * sm.CAT[j][2] for j in op["reqs"]], (1,)
        known = k in sm.KINDS or k in ("score_top_many", "score_top_many_prefix")
        table = ops[st[i]["table"]] if st[i]["table"] is not None else None
        nd = sm.needs(op, streams, sampling, prefix_len, rows, stop, st=st[i], table=table) if known and not k.startswith("refused") else None
        s = st[i]
        on = tuple(n for n, v in zip(SETTINGS, (s["top_k"] > 0, s["genlp"] >= 0, any(s["pen"]), s["table"] is not None)) if v)
        out.append(dict(epoch=epoch, st=s, on=on, nd=nd, streams=streams, before=before, draw=k == "generate_many_sampled" or bool(op.get("sampled")),
                        form=table["form"] if table else "off"))
        if k == "set_batch_sampler_on":
            sampling = True
        elif k == "set_batch_sampler_off":
            sampling = False
        elif k == "batch_prefix_set":
            prefix_len = op["prompt"][1]
    return out


def value_of(info, name):
    s = info["st"]
    return {"top_k": s["top_k"], "genlp": s["genlp"], "pen": s["pen"], "bias": info["form"]}[name]


def test_the_setting_kinds_and_their_values(ssequences):
    seen = {k: set() for k in sm.SETTING_KINDS}
    per_modes, longest, untils, zeros = set(), 0, 0, set()
    for seed, ops in ssequences.items():
        assert all(o["op"] in sm.KINDS + sm.SETTING_KINDS for o in ops)
        assert eval(repr(ops)) == ops                      # the literal of a failure message
        assert ops == sm.make_settings_sequence(seed)
        for o in ops:
            k = o["op"]
            if k in seen:
                seen[k].add(o.get("k", o.get("n", (o.get("p"), o.get("f")) if k == "set_penalties" else o.get("bad"))) if k != "set_logit_bias" else o["form"])
            if k == "set_logit_bias" and o["form"] != "off":
                lens, modes = sm.table_lens(o)
                longest = max(longest, max(lens))
                if o["form"] == "per":
                    per_modes |= set(modes)
    assert seen["set_top_k"] == set(sm.TOP_KS) == {0, 1, 5, 20, 64}
    assert seen["set_gen_logprobs"] == set(sm.GEN_LPS) == {-1, 0, 3, 64}
    pens = seen["set_penalties"]
    assert pens == set(sm.PENALTIES) and (0.0, 0.0) in pens and len(pens) >= 4
    assert any(p < 0 for p, f in pens) and any(f < 0 for p, f in pens) and any(p > 0 and f > 0 for p, f in pens)
    assert all(-2 <= v <= 2 for pf in pens for v in pf)
    assert seen["set_logit_bias"] == set(sm.BIAS_FORMS) and per_modes == {0, 1} and longest >= 300
    assert seen["refused_set_top_k"] == {65, -1} and seen["refused_set_gen_logprobs"] == {-2, 65}
    assert seen["refused_set_penalties"] == {"2.5", "nan"} and seen["refused_set_logit_bias"] == {"twice", "vocab", "inf", "allow"}
    assert seen["refused_score_top"] == {0, 65}
    assert {1, 5, 64} <= seen["score_top_many"] | seen["score_top_many_prefix"] and seen["score_top_many_prefix"]
    assert seen["read_gen_logprobs"] and seen["refused_bias_lists"]


def test_the_reads_of_the_records(ssequences):
    """read_gen_logprobs stands where it is refused for each of the header's reasons, right behind a loop op with records and behind
    ops of other kinds with the records still there"""
    seen, behind = set(), set()
    for ops in ssequences.values():
        left = "none"
        for i, (op, f) in enumerate(zip(ops, swalk(ops))):
            k = op["op"]
            if k == "batch_init":
                left = "none"                                   # no loop call under the setting since q3_batch_init
            elif k in sm.MANY:
                left = "records" if f["st"]["genlp"] >= 0 else "off"
            elif k in ("refused_stop", "refused_bias_lists"):
                left = "failed"
            elif k == "read_gen_logprobs":
                seen.add(left)
                if left == "records":
                    behind.add("loop" if ops[i - 1]["op"] in sm.MANY else "read" if ops[i - 1]["op"] == k else "setter" if ops[i - 1]["op"] in sm.SETTERS else "other")
    assert seen == {"none", "off", "failed", "records"}, seen
    assert behind == {"loop", "read", "setter", "other"} or behind >= {"loop", "setter", "other"}, behind


def test_every_loop_variant_under_every_value_class(ssequences, capsys):
    ran = set()                     # (kind, sampled, the state of the four settings by value class)
    forms, hits = {}, {}
    for seed, ops in ssequences.items():
        info = swalk(ops)
        built = {}
        for i, (op, f) in enumerate(zip(ops, info)):
            if op["op"] not in sm.MANY:
                continue
            ran.add((op["op"], f["draw"], tuple(value_of(f, n) for n in SETTINGS)))
            for key in f["nd"]["forms"]:
                at = (seed, f["epoch"]) + key
                built[at] = built.get(at, 0) + 1
        for at, n in built.items():
            forms[at[2:6]] = forms.get(at[2:6], 0) + 1
            if n >= 2:
                hits[at[2:6]] = hits.get(at[2:6], 0) + 1
    off = (0, -1, (0.0, 0.0), "off")
    missing = []
    for kind, sampled in sm.VARIANTS:
        alone = ([(v,) + off[1:] for v in sm.TOP_KS[1:]] + [(0, v) + off[2:] for v in sm.GEN_LPS[1:]] + [off[:2] + (v, "off") for v in sm.PENALTIES[1:]]
                 + [off[:3] + (v,) for v in sm.BIAS_FORMS[1:]])
        missing += [(kind, sampled, s) for s in alone if (kind, sampled, s) not in ran]
        on = lambda s: tuple(a != b for a, b in zip(s, off))
        masks = {on(s) for k, d, s in ran if (k, d) == (kind, sampled)}
        missing += [(kind, sampled, m) for m in [tuple(i in (a, b) for i in range(4)) for a in range(4) for b in range(a + 1, 4)] + [(True,) * 4] if m not in masks]
    assert not missing, f"{len(missing)} (loop kind, sampled, state) never run: {missing[:10]}"
    # the column plans by their key.  The library keeps top_k on sampled plans alone (plan_get clears PlanKey::topk on a greedy
    # plan), so 27 forms exist, not 36: the nine (draw 0, topk 1) cannot be reached by any sequence.
    exist = {(d, t, g, p) for d in (False, True) for t in (False, True) for g in range(3) for p in range(3) if d or not t}
    with capsys.disabled():
        print(f"\ncolumn-plan forms (draw, topk, genlp, pen) reached, with the (seed, epoch, width)s that run them: "
              + ", ".join(f"{tuple(int(v) for v in k)}: {n}" for k, n in sorted(forms.items())))
        print(f"{len(forms)} of the {len(exist)} forms that exist; not reached: {sorted(tuple(int(v) for v in k) for k in exist - set(forms))}")
    assert set(forms) <= exist and len(forms) >= 27
    assert set(hits) == set(forms), f"forms never run a second time on a kept plan: {sorted(set(forms) - set(hits))}"


def test_every_transition_under_kept_plans(ssequences, capsys):
    found, pairs = {}, set()
    for seed, ops in ssequences.items():
        info = swalk(ops)
        pairs |= sm.pairs_of(ops)
        built, epoch = set(), 0
        reuse_at, new_at = {}, {}               # per loop op: does it run a kept (form, width), does it build one
        snap = {}
        for i, (op, f) in enumerate(zip(ops, info)):
            if f["epoch"] != epoch:
                built, epoch = set(), f["epoch"]
            snap[i] = set(built)
            if op["op"] in sm.MANY:
                reuse_at[i], new_at[i] = bool(f["nd"]["forms"] & built), bool(f["nd"]["forms"] - built)
                built |= f["nd"]["forms"]
        for i, op in enumerate(ops[:-1]):
            if op["op"] not in sm.SETTERS:
                continue
            name = SETTINGS[sm.SETTERS.index(op["op"])]
            off = {"top_k": 0, "genlp": -1, "pen": (0.0, 0.0), "bias": "off"}[name]
            a, b = value_of(info[i], name), value_of(info[i + 1], name)
            what = "off->on" if a == off != b else "on->off" if a != off == b else "on->other" if a != b or (name == "bias" and a != off) else None
            if what is None:
                continue
            # the column plans of both neighbouring forms exist in the epoch (on either draw side)
            both = any({sm.form_of(d, info[i]["st"]), sm.form_of(d, info[i + 1]["st"])} <= {k[:4] for k in snap[i]} for d in (False, True))
            end = next((j for j in range(i + 1, len(ops)) if ops[j]["op"] in (op["op"], "batch_init")), len(ops))
            loops = [j for j in range(i + 1, end) if j in reuse_at]
            if both and any(reuse_at[j] for j in loops) and any(new_at[j] for j in loops):
                found.setdefault((name, what), []).append((seed, i))
    with capsys.disabled():
        print("\ntransitions under kept plans of both forms, a loop op on kept widths and one that builds a width behind them: "
              + ", ".join(f"{n} {w}: {len(v)}" for (n, w), v in sorted(found.items())))
    for name in SETTINGS:
        for what in ("off->on", "on->other", "on->off"):
            assert (name, what) in found, (name, what)
    missing = [(a, b) for a in sm.SETTING_KINDS for b in sm.MANY if (a, b) not in pairs] + [(b, a) for a in sm.SETTING_KINDS for b in sm.MANY if (b, a) not in pairs]
    assert not missing, f"{len(missing)} (setting kind, loop kind) pairs never adjacent: {missing}"


def test_every_setting_in_force_across_state_changes(ssequences):
    across = {}
    quiet = set()
    for seed, ops in ssequences.items():
        info = swalk(ops)
        for i, (op, f) in enumerate(zip(ops, info)):
            k = op["op"]
            later = any(o["op"] in sm.MANY for o in ops[i + 1:])
            if k == "batch_init" and i and later:
                for name in f["on"]:
                    across.setdefault((name, "batch_init"), set()).add("larger" if op["streams"] > f["before"] else "other" if op["streams"] != f["before"] else "same")
            if k in ("set_sampler", "set_batch_sampler_on", "set_batch_sampler_off", "batch_reset_kv") and later:
                for name in f["on"]:
                    across.setdefault((name, k), set()).add("x")
            if len(f["on"]) == 4 and len(info[min(i + 1, len(ops) - 1)]["on"]) == 4 and later:
                quiet.add(k)
    for name in SETTINGS:
        assert {"larger", "other"} <= across.get((name, "batch_init"), set()), (name, across.get((name, "batch_init")))
        for k in ("set_sampler", "set_batch_sampler_on", "set_batch_sampler_off", "batch_reset_kv"):
            assert (name, k) in across, (name, k)
    missing = [k for k in sm.KINDS if k not in sm.MANY and k not in quiet]
    assert not missing, f"kinds that never run under all four settings: {missing}"


def test_the_settings_buffers_grow_twice_behind_cached_plans(ssequences, capsys):
    """the rule of test_every_grow_only_buffer_grows_twice_behind_cached_plans for the per-call buffers of sections 2m, 2o and 2q"""
    for seed, ops in ssequences.items():
        info = swalk(ops)
        grown = {b: [] for b in sm.SETTING_BUFFERS}
        best = {}
        cap = {}
        cols_built, dense_built, cols_hit, dense_hit = set(), set(), False, False
        last_epoch = 0
        for i, f in enumerate(info):
            epoch, nd = f["epoch"], f["nd"]
            if epoch != last_epoch:
                cap, cols_built, dense_built, cols_hit, dense_hit, last_epoch = {}, set(), set(), False, False, epoch
            if nd is None:
                continue
            plans = nd.get("forms") or nd["cols"]
            for b, n in nd["need"].items():
                if b in grown and n > best.get(b, 0) and cap.get(b, 0) > 0 and cols_hit and dense_hit:
                    later = [j for j in range(i + 1, len(ops)) if info[j]["epoch"] == epoch and ops[j]["op"] == ops[i]["op"] and info[j]["nd"]
                             and 0 < info[j]["nd"]["need"].get(b, 0) < n]
                    if later:
                        grown[b].append(i)
                best[b] = max(best.get(b, 0), n)
                if b == "att_pf" and n > cap.get(b, 0):
                    dense_built = set()
                cap[b] = max(cap.get(b, 0), n)
            cols_hit |= bool(plans & cols_built)
            dense_hit |= bool(nd["dense"] & dense_built)
            cols_built |= plans
            dense_built |= nd["dense"]
        with capsys.disabled():
            print(f"\nseed {seed}: calls that grow a settings buffer behind cached plans, a smaller one following: " + ", ".join(f"{b} {len(v)}" for b, v in grown.items()), end="")
        for b, v in grown.items():
            assert len(v) >= 2, f"seed {seed}: {b} grows {len(v)} times ({v})"


def test_slots_are_reused_under_penalties(ssequences):
    reused = per_request = 0
    for ops in ssequences.values():
        for op, f in zip(ops, swalk(ops)):
            if op["op"] in sm.MANY and "pen" in f["on"] and len(op["reqs"]) > f["streams"]:
                reused += 1
                per_request += f["form"] == "per"
    assert reused >= 10 and per_request >= 4, (reused, per_request)


def test_the_settings_bind(ssequences, reference, capsys):
    """non-vacuity, from Reference alone: the penalties, the tables and top_k change the rows of the ops that run under them"""
    pen = pen_differs = twice = table = sampled_k = k_differs = 0
    for seed, ops in ssequences.items():
        tables = sm.Tables(ops, reference)
        for j, (op, f) in enumerate(zip(ops, swalk(ops))):
            if op["op"] not in sm.MANY:
                continue
            rows = tables.rows(j)
            if "pen" in f["on"]:
                pen += 1
                pen_differs += rows != tables.rows(j, pen=(0.0, 0.0))
                twice += any(len(set(r)) < len(r) for r in rows)
            if "bias" in f["on"]:
                table += 1
                assert rows != tables.rows(j, table=False), f"seed {seed}, op {j}: the table changes nothing"
                assert all(a != b for a, b in zip(rows, tables.rows(j, table=False))), f"seed {seed}, op {j}: a request the table leaves alone"
            if f["draw"] and f["st"]["top_k"] in (1, 5) and any(sm.CAT[i][3] > 0 for i in op["reqs"]):
                sampled_k += 1
                k_differs += rows != tables.rows(j, top_k=0)
    with capsys.disabled():
        print(f"\nloop ops under penalties: {pen}, rows differ from (0, 0) in {pen_differs}, a count reaches 2 in {twice}; under a table: {table}, all differ; "
              f"sampled under top_k 1 or 5: {sampled_k}, rows differ from top_k 0 in {k_differs}")
    assert pen and 2 * pen_differs >= pen and twice >= 10
    assert table and sampled_k and 2 * k_differs >= sampled_k


def test_the_harness_catches_the_settings_leaks(ssequences, reference, capsys):
    import time
    t0 = time.time()
    for seed, ops in ssequences.items():
        sm.run(sm.FakeEngine(reference), ops, reference, seed)
    with capsys.disabled():
        print(f"\n{sum(len(o) for o in ssequences.values())} ops on the fake engine in {time.time() - t0:.1f} s")
    for leak in sm.SETTING_LEAKS:
        caught = {}
        for seed, ops in ssequences.items():
            try:
                sm.run(sm.FakeEngine(reference, leak=leak), ops, reference, seed)
            except AssertionError as err:
                msg = str(err)
                assert msg.startswith(f"seed {seed}, engine 0, op ") and "\nops = [" in msg
                at = int(msg.split("op ")[1].split(" ")[0])
                assert eval(msg.split("\nops = ")[1]) == ops[:at + 1]
                caught[seed] = (at, ops[at]["op"])
        with capsys.disabled():
            print(f"leak {leak!r} first shows at (op, kind) per seed: {caught}")
        assert len(caught) >= 4, f"leak {leak!r} shows in {len(caught)} of {len(ssequences)} seeds"
        for seed, (at, _) in caught.items():            # where the leaked state can be told from the ops alone: at that op, no later
            first = settings_first_visible(leak, ssequences[seed])
            assert first is None or at == first, f"leak {leak!r}, seed {seed}: reported at op {at}, visible from op {first}"


def settings_first_visible(leak, ops):
    """the first op behind which the leaked state is observable through the API, for the leaks whose place the ops alone tell"""
    info = swalk(ops)
    if leak == "topk_init":              # q3_sampler_get_top_k behind the first q3_batch_init under top_k > 0
        return next((i for i, o in enumerate(ops) if o["op"] == "batch_init" and info[i]["st"]["top_k"] > 0), None)
    if leak == "score_top_shared":       # the first score call with tops behind a loop op with tops in the same batched state
        tops = False
        for i, o in enumerate(ops):
            if o["op"] == "batch_init":
                tops = False
            elif o["op"] in sm.MANY:
                tops = info[i]["st"]["genlp"] > 0
            elif o["op"] in ("score_top_many", "score_top_many_prefix") and tops:
                return i
    if leak == "genlp_penalised":        # the first loop op with records under penalties or a table: its sums are the adjusted row's
        return next((i for i, o in enumerate(ops) if o["op"] in sm.MANY and info[i]["st"]["genlp"] >= 0 and {"pen", "bias"} & set(info[i]["on"])), None)
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# the guide dimension (include/qwen3_hip.h sections 2r to 2t): seq_model.GUIDE_KINDS among the kinds above
# ---------------------------------------------------------------------------------------------------------------------------------
SETTING_DIGESTS = {     # sha256 of repr(make_settings_sequence(seed)), taken on the commit in front of the guide dimension
    31: "228ab07a8d31334a95b12e9c3d5895505e6bba3a771efbcbd0f3c992d7278488", 32: "c85babe5281ba38e66b1917b2c46f49155e3a40453ce7b5e488fd79182f4babb",
    33: "3593a99e74f5da32f61ffa01c24124385b1bdaf7e35395ef4db19ff994d0d49f", 34: "253ed416273c314674b3216bf10a065e21ef91c71b122a290e536b7e3a65f746",
    35: "648d86aa2b4ad152984d5d38e53731c997bcc037775d8c5da23a92a9bcfe443f", 36: "4c2e186cf8db4b951808fdb7d3a91f7e76aa8c3d163248eab8987cc50d8dfb5c",
}
GUIDED = ("guide", "stop")
PLAIN = ("generate_many_greedy", "generate_many_sampled", "generate_many_dense")
SCHED = ("generate_many_stop", "generate_many_prefix")


@pytest.fixture(scope="module")
def gsequences(q3):
    return {seed: sm.make_guide_sequence(seed) for seed in sm.GUIDE_SEEDS}


@pytest.fixture(scope="module")
def gtables(gsequences, reference):
    return {seed: sm.Tables(ops, reference) for seed, ops in gsequences.items()}


def gwalk(ops):
    """swalk, with the guide and the stop automaton: gform "dense" / "sparse" / None and guide = the form of the automaton in force,
    stop = the form of the stop automaton in force ("off": none), gi / si = the setter ops that hold"""
    out = swalk(ops)
    for f in out:
        s = f["st"]
        f.update(gform=s["gform"], guide=ops[s["guide"]]["form"] if s["guide"] is not None else "off", gi=s["guide"],
                 stop=ops[s["stop"]]["form"] if s["stop"] is not None else "off", si=s["stop"])
        f["on"] = f["on"] + tuple(n for n in GUIDED if f[n] != "off")
    return out


def test_the_six_settings_sequences_are_what_they_were(ssequences, gsequences):
    import hashlib
    assert set(SETTING_DIGESTS) == set(sm.SETTING_SEEDS)
    for seed, ops in ssequences.items():
        assert hashlib.sha256(repr(ops).encode()).hexdigest() == SETTING_DIGESTS[seed], seed
    assert not set(sm.GUIDE_KINDS) & set(sm.KINDS + sm.SETTING_KINDS) and len(sm.CAT) == 115 and len(sm.KINDS) == 45 and len(sm.SETTING_KINDS) == 13
    assert 4 <= len(sm.GUIDE_SEEDS) <= 6 and not set(sm.GUIDE_SEEDS) & set(sm.SEEDS + sm.SETTING_SEEDS)
    longest = max(len(ops) for ops in ssequences.values())
    for seed, ops in gsequences.items():
        assert ops == sm.make_guide_sequence(seed) and sm._guide_sequence(seed) == sm._guide_sequence(seed)     # deterministic
        assert eval(repr(ops)) == ops                          # the literal of a failure message
        assert all(o["op"] in sm.KINDS + sm.SETTING_KINDS + sm.GUIDE_KINDS for o in ops)
        assert len(ops) <= longest, (seed, len(ops), longest)


def test_the_guide_kinds_their_forms_and_refusals(gsequences, capsys):
    seen = {k: set() for k in sm.GUIDE_KINDS}
    pairs = set()
    for ops in gsequences.values():
        pairs |= sm.pairs_of(ops)
        for o in ops:
            if o["op"] in seen:
                seen[o["op"]].add(o.get("form") or o.get("bad") or o.get("of"))
    with capsys.disabled():
        print("\nguide kinds: " + ", ".join(f"{k} {sum(o['op'] == k for ops in gsequences.values() for o in ops)}" for k in sm.GUIDE_KINDS))
    assert seen["set_guide"] == set(sm.GUIDE_FORMS) and seen["set_guide_sparse"] == set(sm.SPARSE_FORMS) and seen["set_stop_seq"] == set(sm.STOP_FORMS)
    assert {"off", "all", "trie", "cycle", "per", "big"} == set(sm.GUIDE_FORMS) and {"dflt", "half"} <= set(sm.SPARSE_FORMS)
    assert {"hit1", "hit2", "hit3", "overlap", "never", "per", "any", "big", "off"} == set(sm.STOP_FORMS)
    for k, vals in sm.GUIDE_REFUSALS.items():
        assert seen[k] == set(vals), (k, seen[k])
    assert {"dead", "start", "vocab"} <= set(sm.GUIDE_REFUSALS["refused_set_guide"]) and {"dead", "ascend", "row_off", "start", "vocab"} <= set(sm.GUIDE_REFUSALS["refused_set_guide_sparse"])
    assert {"ascend", "row_off", "start", "vocab"} <= set(sm.GUIDE_REFUSALS["refused_set_stop_seq"])
    assert seen["refused_guide_starts"] == {"dense", "sparse", "stop"}
    missing = [(a, b) for a in sm.GUIDE_SETTERS for b in sm.MANY if (a, b) not in pairs] + [(b, a) for a in sm.GUIDE_SETTERS for b in sm.MANY if (b, a) not in pairs]
    assert not missing, f"{len(missing)} (setter, loop kind) pairs never adjacent: {missing}"
    # the big forms are big: the dense table has 1,024 states and more, the sparse form grows all three arrays over every small form
    assert min(sm.GUIDE_BIG.values()) >= 1024 and min(s * k for s, k in sm.SPARSE_BIG.values()) > 2 * sm.VOCAB


def test_every_loop_variant_under_every_guide_and_stop_form(gsequences, capsys):
    ran = set()                     # (kind, sampled, (guide kind, form), stop form, the earlier settings that are on)
    forms, hits = {}, {}
    for seed, ops in gsequences.items():
        built = {}
        for op, f in zip(ops, gwalk(ops)):
            if op["op"] not in sm.MANY:
                continue
            ran.add((op["op"], f["draw"], (f["gform"] or "off", f["guide"]), f["stop"], tuple(n for n in f["on"] if n in SETTINGS)))
            for key in f["nd"]["forms"]:
                at = (seed, f["epoch"]) + key
                built[at] = built.get(at, 0) + 1
        for at, n in built.items():
            forms[at[2:6]] = forms.get(at[2:6], 0) + 1
            if n >= 2:
                hits[at[2:6]] = hits.get(at[2:6], 0) + 1
    missing = []
    for kind, sampled in sm.VARIANTS:
        mine = {s[2:] for s in ran if s[:2] == (kind, sampled)}
        alone = ([(("dense", f), "off", ()) for f in sm.GUIDE_FORMS[1:-1]] + [(("sparse", f), "off", ()) for f in sm.SPARSE_FORMS[1:-1]]
                 + [(("off", "off"), f, ()) for f in sm.STOP_FORMS[1:-1]])
        missing += [(kind, sampled, s) for s in alone if s not in mine]
        # the forms "big" run where the arrays grow: the two guides under every variant, the stop automaton alone under the two loops
        # that read it and beside the sparse guide under the three that do not
        missing += [(kind, sampled, g, "big") for g in ("dense", "sparse") if not any(s[0] == (g, "big") for s in mine)]
        missing += [(kind, sampled, "stop big") for _ in (0,) if not any(s[1] == "big" and (kind in PLAIN or s[0][0] == "off") for s in mine)]
        missing += [(kind, sampled, "guide x stop") for _ in (0,) if not any(s[0][0] != "off" and s[1] != "off" and s[0][1] != "big" for s in mine)]
        missing += [(kind, sampled, "guide x " + n) for n in SETTINGS if not any(s[0][0] != "off" and n in s[2] for s in mine)]
    assert not missing, f"{len(missing)} (loop kind, sampled, state) never run: {missing[:10]}"
    # the column plans by their key: under a guide the penalty axis reads 3 (dense) or 4 (sparse) whatever the table and the penalties,
    # and a greedy plan has no top_k (as for the 27 earlier forms): 2 x 3 x 3 = 18 forms exist
    exist = {(d, t, g, p) for d in (False, True) for t in (False, True) for g in range(3) for p in (3, 4) if d or not t}
    guided = {k: n for k, n in forms.items() if k[3] >= 3}
    with capsys.disabled():
        print(f"\ncolumn-plan forms (draw, topk, genlp, pen) under a guide, with the (seed, epoch, width)s that run them: "
              + ", ".join(f"{tuple(int(v) for v in k)}: {n}" for k, n in sorted(guided.items())))
        print(f"{len(guided)} of the {len(exist)} forms that exist; not reached: {sorted(tuple(int(v) for v in k) for k in exist - set(guided))}")
    assert len(exist) == 18 and set(guided) == exist
    assert exist <= set(hits), f"forms never run a second time on a kept plan: {sorted(exist - set(hits))}"


def test_guide_and_stop_transitions_under_kept_plans(gsequences, capsys):
    found = {}
    for seed, ops in gsequences.items():
        info = gwalk(ops)
        built, epoch, sched_ran = set(), 0, False
        reuse_at, new_at, snap, sched_before = {}, {}, {}, {}
        for i, (op, f) in enumerate(zip(ops, info)):
            if f["epoch"] != epoch:
                built, epoch, sched_ran = set(), f["epoch"], False
            snap[i], sched_before[i] = set(built), sched_ran
            if op["op"] in sm.MANY:
                reuse_at[i], new_at[i] = bool(f["nd"]["forms"] & built), bool(f["nd"]["forms"] - built)
                built |= f["nd"]["forms"]
                sched_ran |= op["op"] in SCHED
        for i, op in enumerate(ops[:-1]):
            a, b = info[i], info[i + 1]
            if op["op"] in ("set_guide", "set_guide_sparse"):
                what = ("off->on" if a["gform"] is None and b["gform"] else "on->off" if a["gform"] and b["gform"] is None else
                        None if a["gform"] is None else "on->other table" if a["gform"] == b["gform"] else f"{a['gform']}->{b['gform']}")
                if what is None:
                    continue
                # the column plans of both neighbouring forms exist in the epoch (on either draw side)
                both = any({sm.form_of(d, a["st"]), sm.form_of(d, b["st"])} <= {k[:4] for k in snap[i]} for d in (False, True))
                end = next((j for j in range(i + 1, len(ops)) if ops[j]["op"] in ("set_guide", "set_guide_sparse", "batch_init")), len(ops))
                loops = [j for j in range(i + 1, end) if j in reuse_at]
                if both and any(reuse_at[j] for j in loops) and any(new_at[j] for j in loops):
                    found.setdefault(("guide", what), []).append((seed, i))
            elif op["op"] == "set_stop_seq":
                what = "off->on" if a["stop"] == "off" != b["stop"] else "on->off" if a["stop"] != "off" == b["stop"] else "on->other" if a["stop"] != "off" else None
                if what is None:
                    continue
                # no plan key changes with the stop automaton: the scheduler kernel does.  The epoch has run a loop with a device
                # scheduler, and two more follow the switch: one on kept widths and one that builds a width (and captures its graph) while
                # the scheduler kernel of the new setting is in force
                end = next((j for j in range(i + 1, len(ops)) if ops[j]["op"] in ("set_stop_seq", "batch_init")), len(ops))
                loops = [j for j in range(i + 1, end) if ops[j]["op"] in SCHED]
                if sched_before[i] and len(loops) >= 2 and any(reuse_at[j] for j in loops) and any(new_at[j] for j in loops):
                    found.setdefault(("stop", what), []).append((seed, i))
    with capsys.disabled():
        print("\nguide and stop transitions under kept plans, loop ops on kept widths and on new ones behind them: "
              + ", ".join(f"{n} {w}: {len(v)}" for (n, w), v in sorted(found.items())))
    for what in ("off->on", "on->other table", "dense->sparse", "sparse->dense", "on->off"):
        assert len({s for s, _ in found.get(("guide", what), [])}) == len(gsequences), (what, found.get(("guide", what)))
    for what in ("off->on", "on->other", "on->off"):
        assert len({s for s, _ in found.get(("stop", what), [])}) == len(gsequences), (what, found.get(("stop", what)))


def guide_needs(op, f, tables):
    """what a loop op asks of the grow-only arrays of sections 2r to 2t (guide_call_begin, guide_sp_call_begin, stop_seq_call_begin)"""
    need = {}
    if f["gi"] is not None:
        need.update(tables.guide(f["gi"]).sizes())
    if f["si"] is not None and op["op"] in SCHED:
        a, starts = tables.stop(f["si"])
        need.update(stop_seq_dflt=a.default.size, stop_seq_off=a.default.size + 1, stop_seq_edges=max(a.tokens.size, 1), stop_seq_start=len(starts))
    return need


def test_the_guide_buffers_grow_twice_behind_cached_plans(gsequences, gtables, capsys):
    """the rule of test_the_settings_buffers_grow_twice_behind_cached_plans for the arrays of the two guides and the stop automaton"""
    for seed, ops in gsequences.items():
        info = gwalk(ops)
        needs = [guide_needs(op, f, gtables[seed]) if op["op"] in sm.MANY else {} for op, f in zip(ops, info)]
        grown = {b: [] for b in sm.GUIDE_BUFFERS}
        best, cap = {}, {}
        cols_built, dense_built, cols_hit, dense_hit = set(), set(), False, False
        last_epoch = 0
        for i, f in enumerate(info):
            epoch, nd = f["epoch"], f["nd"]
            if epoch != last_epoch:
                cap, cols_built, dense_built, cols_hit, dense_hit, last_epoch = {}, set(), set(), False, False, epoch
            if nd is None:
                continue
            for b, n in needs[i].items():
                if n > best.get(b, 0) and cap.get(b, 0) > 0 and cols_hit and dense_hit:
                    later = [j for j in range(i + 1, len(ops)) if info[j]["epoch"] == epoch and ops[j]["op"] == ops[i]["op"] and 0 < needs[j].get(b, 0) < n]
                    if later:
                        grown[b].append(i)
                best[b] = max(best.get(b, 0), n)
                cap[b] = max(cap.get(b, 0), n)
            if nd["need"].get("att_pf", 0) > cap.get("att_pf", 0):
                dense_built, cap["att_pf"] = set(), nd["need"]["att_pf"]
            plans = nd.get("forms") or nd["cols"]
            cols_hit |= bool(plans & cols_built)
            dense_hit |= bool(nd["dense"] & dense_built)
            cols_built |= plans
            dense_built |= nd["dense"]
        with capsys.disabled():
            print(f"\nseed {seed}: calls that grow an array of the guides or the stop automaton behind cached plans, a smaller one following: "
                  + ", ".join(f"{b} {len(v)}" for b, v in grown.items()), end="")
        for b, v in grown.items():
            assert len(v) >= 2, f"seed {seed}: {b} grows {len(v)} times ({v})"


def test_guide_and_stop_in_force_across_state_changes(gsequences):
    across, quiet = {}, set()
    for seed, ops in gsequences.items():
        info = gwalk(ops)
        for i, (op, f) in enumerate(zip(ops, info)):
            k = op["op"]
            # in force across the op: set in front of it, and a loop op that reads it follows under the very same setter op
            idx = dict(guide="gi", stop="si")
            on = [n for n in GUIDED if f[idx[n]] is not None and any(
                o["op"] in (sm.MANY if n == "guide" else SCHED) and info[j][idx[n]] == f[idx[n]] for j, o in enumerate(ops[i + 1:], i + 1))]
            if k == "batch_init" and i:
                for name in on:
                    across.setdefault((name, "batch_init"), set()).add("larger" if op["streams"] > f["before"] else "other" if op["streams"] != f["before"] else "same")
            if k in ("set_sampler", "set_batch_sampler_on", "set_batch_sampler_off", "batch_reset_kv") + sm.SETTERS:
                for name in on:
                    across.setdefault((name, k), set()).add("x")
            if len(on) == 2:
                quiet.add(k)
    for name in GUIDED:
        assert {"larger", "other"} <= across.get((name, "batch_init"), set()), (name, across.get((name, "batch_init")))
        for k in ("set_sampler", "set_batch_sampler_on", "set_batch_sampler_off", "batch_reset_kv"):
            assert (name, k) in across, (name, k)
    for k in sm.SETTERS:                                        # the guide holds across the setters of the four earlier settings
        assert ("guide", k) in across, k
    missing = [k for k in sm.KINDS if k not in sm.MANY and k not in quiet]
    assert not missing, f"kinds that never run under a guide and a stop automaton: {missing}"


def test_slots_are_reused_under_guides_and_stop_automata(gsequences, gtables, capsys):
    reused = per_request = ended = 0
    for seed, ops in gsequences.items():
        for j, (op, f) in enumerate(zip(ops, gwalk(ops))):
            if op["op"] not in sm.MANY:
                continue
            if f["guide"] != "off" and len(op["reqs"]) > f["streams"]:
                reused += 1
                per_request += f["guide"] in ("per", "big")
            if f["stop"] != "off" and op["op"] in SCHED and len(op["reqs"]) > f["streams"]:
                lens, n_new = sm.op_requests(op)
                emit, by_seq = gtables[seed].emits(j), gtables[seed].seq_emits(j)
                occ = sm.many_plan(lens, n_new, f["streams"], emit=emit)["occupants"]
                # ended early by a completed sequence (not by a stop token in front of it), and not the slot's last occupant
                ended += any(emit[r] == by_seq[r] < n_new[r] for rs in occ.values() for r in rs[:-1])
    with capsys.disabled():
        print(f"\nloop ops under a guide with more requests than slots: {reused}, {per_request} of them with one start per request; loops with a "
              f"device scheduler under a stop automaton in which a completed sequence ends a request early and another takes its slot: {ended}")
    assert reused >= 10 and per_request >= 4 and ended >= 6, (reused, per_request, ended)


def test_the_guides_and_the_stop_automata_bind(gsequences, gtables, capsys):
    """non-vacuity, from Reference alone"""
    import stop_seq_ref
    guided = else_branch = compete = early_min = per_guides = 0
    fall_back = {}                                              # seed -> requests that complete B two tokens deep in A
    stops = {}                                                  # (seed, set_stop_seq op) -> requests a sequence ends before their cap
    for seed, ops in gsequences.items():
        t = gtables[seed]
        for j, (op, f) in enumerate(zip(ops, gwalk(ops))):
            if op["op"] not in sm.MANY:
                continue
            if f["gi"] is not None:
                gd = t.guide(f["gi"])
                if f["guide"] == "per":          # one request unguided, at least two that start in different states
                    per_guides += 1
                    assert -1 in gd.starts and len(set(gd.starts) - {-1}) >= 2 and len(gd.starts) == len(op["reqs"]), (seed, j, gd.starts)
                whole = t.rows(j, cut=False)
                for r, (row, free) in enumerate(zip(whole, t.rows(j, guide=False, cut=False))):
                    s = gd.start_of(r)
                    if s < 0:
                        assert row == free, f"seed {seed}, op {j}: start -1 and the guide changes request {r}"
                        continue
                    assert f["guide"] == "all" or row != free, f"seed {seed}, op {j}: the guide leaves request {r} alone"
                    guided += 1
                    for tok in row:
                        else_branch += int(gd.row(s)[tok]) < 0
                        s = gd.step(s, tok)
            if f["si"] is not None and op["op"] in SCHED:
                a, starts = t.stop(f["si"])
                whole, n_new = t.rows(j, cut=False), sm.op_requests(op)[1]
                stop_tokens = t.stop_tokens(j)
                emit, cuts = t.emits(j), [len(sm.cut_at_stop(r, stop_tokens)) for r in whole]
                per = [starts[0] if len(starts) == 1 else starts[r] for r in range(len(whole))]
                by_seq = [1 if a.seqs is None else stop_seq_ref.n_emit_seqs(row, a.seqs) if s >= 0 else len(row) for row, s in zip(whole, per)]
                assert by_seq == t.seq_emits(j)
                if f["stop"] == "overlap":       # the request ends with B = [b, c] behind a, b of an A = [a, b, x]: the fall-back edge is taken
                    three = [q for q in a.seqs if len(q) == 3]
                    fall_back[seed] = fall_back.get(seed, 0) + sum(
                        e == q < k and q >= 3 and any(row[q - 3:q - 1] == A[:2] and row[q - 2:q] in a.seqs for A in three)
                        for row, e, q, k in zip(whole, emit, by_seq, n_new))
                assert emit == [min(c, q) for c, q in zip(cuts, by_seq)]
                n = sum(q < k and q <= c for q, k, c in zip(by_seq, n_new, cuts))
                stops[(seed, f["si"])] = stops.get((seed, f["si"]), 0) + n
                assert f["stop"] != "never" or by_seq == n_new, f"seed {seed}, op {j}: a sequence no request produces ends a request"
                compete += any(c < k and q < k for c, q, k in zip(cuts, by_seq, n_new))
                lists = t.get(f["st"]["table"])[0] if f["st"]["table"] is not None else []
                until = max([e[2] for e in (lists[0] if len(lists) == 1 else [])] + [0])
                early_min += any(q < until for q in by_seq)
    by_form, vain = {}, []
    for (seed, i), n in stops.items():
        form = gsequences[seed][i]["form"]
        if form != "never":
            by_form[form] = by_form.get(form, 0) + (n > 0)
            vain += [(seed, i, form)] * (n == 0)
    with capsys.disabled():
        print(f"\nguided requests: {guided}, every one differs from its unguided row (form all apart); else branch of the state step taken {else_branch} times; "
              f"stop automata that end a request before its cap, by form: {by_form}; in vain: {vain}; ops with a stop token and a sequence competing "
              f"in one request: {compete}; ops under min_tokens with a sequence that completes in front of it: {early_min}")
        print(f"requests that end over the fall-back edge of an overlap automaton, per seed: {fall_back}; loop ops under per-request guide starts: {per_guides}")
    assert guided and else_branch >= 1 and compete >= 1 and early_min >= 1 and per_guides >= 8
    assert all(fall_back.get(seed, 0) >= 1 for seed in gsequences), fall_back
    assert set(by_form) >= set(sm.STOP_FORMS[1:]) - {"never"} and all(n > 0 for n in by_form.values())
    assert 10 * len(vain) <= len(stops), vain


def test_the_harness_catches_the_guide_leaks(gsequences, reference, capsys):
    import time
    t0 = time.time()
    for seed, ops in gsequences.items():
        sm.run(sm.FakeEngine(reference), ops, reference, seed)
    with capsys.disabled():
        print(f"\n{sum(len(o) for o in gsequences.values())} ops on the fake engine in {time.time() - t0:.1f} s")
    for leak in sm.GUIDE_LEAKS:
        caught = {}
        for seed, ops in gsequences.items():
            try:
                sm.run(sm.FakeEngine(reference, leak=leak), ops, reference, seed)
            except AssertionError as err:
                msg = str(err)
                assert msg.startswith(f"seed {seed}, engine 0, op ") and "\nops = [" in msg
                at = int(msg.split("op ")[1].split(" ")[0])
                assert eval(msg.split("\nops = ")[1]) == ops[:at + 1]
                caught[seed] = (at, ops[at]["op"])
        with capsys.disabled():
            print(f"leak {leak!r} first shows at (op, kind) per seed: {caught}")
        assert len(caught) >= (4 if len(gsequences) >= 5 else len(gsequences)), f"leak {leak!r} shows in {len(caught)} of {len(gsequences)} seeds"
        for seed, ops in gsequences.items():            # where the leaked state can be told from the ops alone: at that op, no later
            first = guide_first_visible(leak, ops)
            assert first is None or caught.get(seed, (None,))[0] == first, f"leak {leak!r}, seed {seed}: reported at {caught.get(seed)}, visible from op {first}"


def guide_first_visible(leak, ops):
    """the first op behind which the leaked state is observable through the API, for the leaks whose place the ops alone tell"""
    info = gwalk(ops)
    if leak in ("guide_init_dropped", "stop_init_dropped"):     # the getter behind the first q3_batch_init under the automaton
        name = leak.split("_")[0]
        return next((i for i, o in enumerate(ops) if o["op"] == "batch_init" and info[i][name] != "off"), None)
    if leak == "guide_both_forms":       # q3_guide_get behind the first q3_guide_set_sparse over a dense guide
        return next((i for i, o in enumerate(ops) if o["op"] == "set_guide_sparse" and o["form"] != "off" and info[i]["gform"] == "dense"), None)
    if leak == "stop_in_plain_loops":    # the first loop without a device scheduler under an automaton made to end its requests
        return next((i for i, o in enumerate(ops) if o["op"] in PLAIN and info[i]["stop"] in ("hit1", "hit2", "hit3", "any", "big")), None)
    return None
