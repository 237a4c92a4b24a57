"""The packing rule of q3_dense_pack restated in Python (include/qwen3_hip.h section 2g), written from the header's three rules and
nothing else.  Pure function of the run lengths: the tests compare q3_dense_pack with it entry for entry."""
from collections import namedtuple

ALIGN = 8

Stats = namedtuple("Stats", "blocks live_columns pad_columns")


def pack(run_len, block_cap):
    """-> ([(block, first column, run, offset in the run), ...] in order, Stats, [columns of every piece])"""
    assert run_len and all(n >= 1 for n in run_len) and block_cap >= 16 and block_cap % 16 == 0
    table, lens, widths = [], [], []
    block, end = 0, 0                    # the current block and the column behind its last piece (0: nothing in it yet)
    for r, n in enumerate(run_len):
        off = 0
        while off < n:
            start = -(-end // ALIGN) * ALIGN
            if start >= block_cap:       # nothing left in the block
                widths.append(start)
                block, end, start = block + 1, 0, 0
            take = min(n - off, block_cap - start)
            table.append((block, start, r, off))
            lens.append(take)
            off += take
            end = start + take
            if off < n:                  # the rest continues as the first piece of the next block
                widths.append(-(-end // ALIGN) * ALIGN)
                block, end = block + 1, 0
    if end:
        widths.append(-(-end // ALIGN) * ALIGN)
    live = sum(run_len)
    return table, Stats(len(widths), live, sum(widths) - live), lens
