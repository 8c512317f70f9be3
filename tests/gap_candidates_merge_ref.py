"""The merge contract of include/tvz_gap_shards.h restated with plain Python: the reference of the
tvz_align_candidates_merge tests.  No code under test is imported here: a `sorted()` over tuples and the totals rule."""
import numpy as np

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
PAD = (-1, 0)


def order_key(row):
    """the contract's order: count descending, then video_id ascending"""
    return (-row[1], row[0])


def merge_query(lists, c):
    """`lists`: per list its c + 1 rows of (video_id, count) -> the c + 1 merged rows"""
    totals = [int(rows[c][1]) for rows in lists]
    if any(t == INT32_MIN for t in totals):
        return [PAD] * c + [(-1, INT32_MIN)]
    live = sorted(((int(v), int(n)) for rows in lists for v, n in rows[:c] if v >= 0), key=order_key)[:c]
    total = min(sum(abs(t) for t in totals), INT32_MAX)
    if any(t < 0 for t in totals):
        total = -total
    return live + [PAD] * (c - len(live)) + [(-1, total)]


def merge(blocks):
    """int32 [R, Q, c + 1, 2] -> int32 [Q, c + 1, 2]"""
    blocks = np.asarray(blocks)
    R, Q, c1, _ = blocks.shape
    out = np.zeros((Q, c1, 2), dtype=np.int32)
    for q in range(Q):
        out[q] = merge_query([blocks[r, q].tolist() for r in range(R)], c1 - 1)
    return out


def merge_grouped(blocks, group=16):
    """the same over any number of lists, `group` at a time and the groups' answers again: what associativity claims"""
    blocks = np.asarray(blocks)
    while blocks.shape[0] > group:
        blocks = np.stack([merge(blocks[i:i + group]) for i in range(0, blocks.shape[0], group)])
    return merge(blocks)


def is_sorted(block):
    """Is every query's list of int32 [Q, c + 1, 2] sorted by the contract's order with the padding last - the merge's
    precondition?"""
    block = np.asarray(block)
    c = block.shape[1] - 1
    for rows in block[:, :c].tolist():
        live = [tuple(r) for r in rows if r[0] >= 0]
        if [tuple(r) for r in rows[:len(live)]] != live or live != sorted(live, key=order_key):
            return False
        if any(tuple(r) != PAD for r in rows[len(live):]):
            return False
    return True
