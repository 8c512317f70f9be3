"""Plain-Python restatement of the merge of tvz_align_wide_topk blocks over shards (tvz_align_wide_topk_merge,
include/tvz.h), written from the contract on top of tests/align_wide_ref.py and tests/align_topk_ref.py:

  blocks int[R, Q, k + 1, 4], queries (host lists), contain -> rows int64[Q, k, 4], totals int64[Q]
  - a row with video_id < 0 is padding wherever it stands; so is one whose u is 0 under the call's score kind
    (u = nv + row_len - min(votes, nv, row_len), or min(nv, row_len) with `contain`);
  - the k smallest of the rest by corpus.align_wide_order_key(row, nv, contain), nv = the query's non-NaN count; equal
    rows are all kept;
  - total = the lists' n_hits summed, clamped to INT32_MAX;
  - refused (all padding, total INT32_MIN) when a list's n_hits is negative or the query is longer than 4,095.

And the small split table the sharded tests share (split_table).
"""
import numpy as np

from tests import align_topk_ref as atr, align_wide_ref as awr
from tvidz_amd import corpus as tc

INT32_MAX = (1 << 31) - 1
EPS = 1 / 30
GRID = 324000                               # three hours of 1/30 s
SHIFTS = (-100000, -40000, -2500, -2048, 2048, 3000, 50000, 100000)     # bins of 1/30 s: 68 s .. 56 min


def sorted_rows(rows, nv, contain=False):
    """live rows of one query in the contract's order"""
    live = []
    for r in rows:
        vid, row_len, _bin, votes = (int(x) for x in r)
        v = min(votes, int(nv), row_len)
        u = min(int(nv), row_len) if contain else int(nv) + row_len - v
        if vid < 0 or u == 0:
            continue
        live.append((vid, row_len, _bin, votes))
    return sorted(live, key=lambda r: tc.align_wide_order_key(r, nv, contain))


def merge_ref(blocks, queries, contain=False):
    blocks = np.asarray(blocks, dtype=np.int64)
    R, Q, k1, _ = blocks.shape
    k = k1 - 1
    rows = np.zeros((Q, k, 4), dtype=np.int64)
    rows[:, :, 0] = -1
    totals = np.zeros(Q, dtype=np.int64)
    for q in range(Q):
        n_hits = [int(blocks[r, q, k, 1]) for r in range(R)]
        if any(n < 0 for n in n_hits) or len(list(queries[q])) > atr.MAX_LEN:
            totals[q] = atr.REFUSED
            continue
        totals[q] = min(sum(n_hits), INT32_MAX)
        union = [row for r in range(R) for row in blocks[r, q, :k].tolist()]
        best = sorted_rows(union, atr.n_valid(queries[q]), contain)[:k]
        if best:
            rows[q, :len(best)] = best
    return rows, totals


def block_of(rows, nv, k, contain=False, n_hits=None):
    """One list as tvz_align_wide_topk writes it: the k best of `rows` in order, padding, then (-1, n_hits, 0, 0)."""
    out = np.zeros((k + 1, 4), dtype=np.int64)
    out[:, 0] = -1
    live = sorted_rows(rows, nv, contain)
    for i, r in enumerate(live[:k]):
        out[i] = r
    out[k, 1] = len(live) if n_hits is None else n_hits
    return out


def split_table():
    """-> (rows, queries).  300 rows of 0..40 cuts on a 1/30 s grid over three hours; some video ids stand on two
    rows.  Three base rows of 40 cuts (video ids 3000..3002, rows 0, 3 and 6) lie in the middle hour; 48 rows (3 j + 1)
    are copies of them shifted by SHIFTS bins - both signs, every one beyond the bounded search's 2,047; 12 rows
    (3 j + 2) are 20-cut excerpts of a base row, shifted likewise, every other one with two cuts dropped and six
    added (so that it contains less of a query but resembles a 20-cut query more).  Queries: a base row as it is (its
    copies score 2^20 either way, its excerpts only by containment), a 20-cut excerpt of another moved by 7 bins (the
    Jaccard prefers the altered excerpts, the containment the whole rows), the third with NaNs, an empty and a
    NaN-only one."""
    rng = np.random.default_rng(11)
    rows = []
    for r in range(300):
        n = int(rng.integers(0, 41))
        rows.append((1000 + (r if r % 25 else r // 2), (np.sort(rng.choice(GRID, size=n, replace=False)) / 30.0).tolist()))
    base = [np.sort(rng.choice(np.arange(GRID // 3, 2 * GRID // 3), size=40, replace=False)) for _ in range(3)]
    for i, b in enumerate(base):
        rows[3 * i] = (3000 + i, (b / 30.0).tolist())
    for j in range(48):
        rows[3 * j + 1] = (2000 + j // 2, ((base[j % 3] + SHIFTS[j % len(SHIFTS)]) / 30.0).tolist())
    for j in range(12):
        cuts = base[j % 3][10:30] + SHIFTS[(3 * j + 1) % len(SHIFTS)]
        if j % 2:
            cuts = np.sort(np.concatenate([cuts[2:], cuts[-1] + 1000 + 17 * np.arange(6)]))      # 18 of the 20, 6 others
        rows[3 * j + 2] = (2500 + j, (cuts / 30.0).tolist())
    queries = [(base[0] / 30.0).tolist(), ((base[1][10:30] + 7) / 30.0).tolist(),
               (base[2] / 30.0).tolist() + [float("nan")] * 2, [], [float("nan")] * 3]
    return rows, queries


def aligned_whole(rows, queries, eps=EPS, max_offset=None):
    """align_wide_ref of every query against the WHOLE table, once: a shard's is a selection of its rows."""
    max_offset = awr.MAX_B * eps if max_offset is None else max_offset
    return [awr.align_wide_ref(rows, q, eps, max_offset) for q in queries]
