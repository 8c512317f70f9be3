"""The merge contract of include/tvz_gap_rates_shards.h restated with plain Python: the reference of the
tvz_align_candidates_rates_merge tests.  No code under test is imported here: a dict of per-id (best, -rate) maxima, a
`sorted()` over tuples and the totals rule."""
import numpy as np

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
PAD = (-1, 0, 0)


def order_key(row):
    """the contract's order: best descending, then video_id ascending"""
    return (-row[1], row[0])


def merge_query(lists, c):
    """`lists`: per list its c + 1 rows of (video_id, best, rate_index), in any order -> the c + 1 merged rows"""
    totals = [int(rows[c][1]) for rows in lists]
    if any(t == INT32_MIN for t in totals):
        return [PAD] * c + [(-1, INT32_MIN, 0)]
    per_id = {}
    for rows in lists:
        for v, best, rate in rows[:c]:
            if v >= 0:                                                  # the largest best, at the smallest rate index
                per_id[int(v)] = max(per_id.get(int(v), (-1, 0)), (int(best), -int(rate)))
    live = sorted(((v, b, -r) for v, (b, r) in per_id.items()), key=order_key)[:c]
    total = min(sum(abs(t) for t in totals), INT32_MAX)
    if any(t < 0 for t in totals):
        total = -total if total else INT32_MIN                          # (a negated zero)
    return live + [PAD] * (c - len(live)) + [(-1, total, 0)]


def merge(blocks):
    """int32 [R, Q, c + 1, 3] -> int32 [Q, c + 1, 3]"""
    blocks = np.asarray(blocks)
    R, Q, c1, _ = blocks.shape
    out = np.zeros((Q, c1, 3), dtype=np.int32)
    for q in range(Q):
        out[q] = merge_query([blocks[r, q].tolist() for r in range(R)], c1 - 1)
    return out


def merge_grouped(blocks, group=16):
    """the same over any number of lists, `group` at a time and the groups' answers again: what associativity claims"""
    blocks = np.asarray(blocks)
    while blocks.shape[0] > group:
        blocks = np.stack([merge(blocks[i:i + group]) for i in range(0, blocks.shape[0], group)])
    return merge(blocks)
