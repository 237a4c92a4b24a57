"""The schedule of q3_generate_many_greedy restated in Python (include/qwen3_hip.h section 2e), written from the header's five
rules and nothing else.  Pure function of the request lengths: the tests compare q3_cols_schedule with it entry for entry."""
from collections import namedtuple

COLS_MAX = 32

Stats = namedtuple("Stats", "passes live_columns prompt_columns decode_columns")


def schedule(prompt_len, n_new, max_streams):
    """-> ([(pass, slot, pos, request), ...] in column order, Stats)"""
    assert len(prompt_len) == len(n_new) and all(p >= 1 for p in prompt_len) and all(k >= 1 for k in n_new)
    slots = [None] * max_streams          # per slot: None or {"req", "fed" (prompt tokens through a pass), "g" (tokens produced)}
    queue = list(range(len(prompt_len)))
    table, n_pass, n_prompt, n_decode = [], 0, 0, 0
    while queue or any(s is not None for s in slots):
        # 1. admit
        for i in range(max_streams):
            if slots[i] is None and queue:
                slots[i] = {"req": queue.pop(0), "fed": 0, "g": 0}
        cols = []
        # 2. decode columns first
        decoding = [i for i in range(max_streams) if slots[i] is not None and slots[i]["fed"] == prompt_len[slots[i]["req"]]]
        for i in decoding:
            s = slots[i]
            cols.append((n_pass, i, prompt_len[s["req"]] + s["g"] - 1, s["req"]))
        n_decode += len(decoding)
        # 3. prompt columns fill the rest
        runs = {}
        for i in range(max_streams):
            s = slots[i]
            if s is None or i in decoding:
                continue
            take = min(prompt_len[s["req"]] - s["fed"], COLS_MAX - len(cols))
            if take <= 0:
                continue
            cols.extend((n_pass, i, s["fed"] + k, s["req"]) for k in range(take))
            runs[i] = take
            n_prompt += take
        # 4. phase changes, 5. finished requests
        for i in decoding:
            slots[i]["g"] += 1
        for i, take in runs.items():
            s = slots[i]
            s["fed"] += take
            if s["fed"] == prompt_len[s["req"]]:
                s["g"] = 1
        for i in range(max_streams):
            if slots[i] is not None and slots[i]["g"] == n_new[slots[i]["req"]]:
                slots[i] = None
        assert 1 <= len(cols) <= COLS_MAX
        table.extend(cols)
        n_pass += 1
    return table, Stats(n_pass, len(table), n_prompt, n_decode)
