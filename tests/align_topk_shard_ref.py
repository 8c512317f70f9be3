"""Plain-Python restatement of the merge of tvz_align_topk blocks over shards (tvz_align_topk_merge, include/tvz.h),
on top of tests/align_topk_ref.py.  It is the host merge service.ShardedCorpus.align_topk used to run, kept here as
the reference: the union of the lists' rows sorted by corpus.align_order_key, with the total and refusal rules.

  blocks int[R, Q, k + 1, 4], queries (host lists) -> rows int64[Q, k, 4], totals int64[Q]
  - a row with video_id < 0 is padding wherever it stands; so is one whose u = nv + row_len - min(votes, nv, row_len)
    is 0;
  - the k smallest of the rest by align_order_key(row, nv), nv = the query's non-NaN count; equal rows are all kept;
  - total = the lists' n_hits summed, clamped to INT32_MAX;
  - refused (all padding, total INT32_MIN) when a list's n_hits is negative or the query is longer than 4,095.
"""
import numpy as np

from tests import align_topk_ref as atr
from tvidz_amd import corpus as tc

INT32_MAX = (1 << 31) - 1


def sorted_rows(rows, nv):
    """live rows of one query in the contract's order"""
    live = []
    for r in rows:
        vid, row_len, _bin, votes = (int(x) for x in r)
        if vid < 0 or int(nv) + row_len - min(votes, int(nv), row_len) == 0:
            continue
        live.append((vid, row_len, _bin, votes))
    return sorted(live, key=lambda r: tc.align_order_key(r, nv))


def merge_ref(blocks, queries):
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
        best = sorted_rows([row for r in range(R) for row in blocks[r, q, :k].tolist()], atr.n_valid(queries[q]))[:k]
        if best:
            rows[q, :len(best)] = best
    return rows, totals


def block_of(rows, nv, k, n_hits=None):
    """One list as tvz_align_topk writes it: the k best of `rows` in order, padding, then (-1, n_hits, 0, 0)."""
    out = np.zeros((k + 1, 4), dtype=np.int64)
    out[:, 0] = -1
    live = sorted_rows(rows, nv)
    for i, r in enumerate(live[:k]):
        out[i] = r
    out[k, 1] = len(live) if n_hits is None else n_hits
    return out


def merge_of_parts(parts, queries):
    """parts = [(rows int[Q, k, 4], totals int[Q])] as DeviceCorpus.align_topk returns them, one per shard."""
    blocks = []
    for rows, totals in parts:
        rows = np.asarray(rows, dtype=np.int64)
        tail = np.zeros((rows.shape[0], 1, 4), dtype=np.int64)
        tail[:, 0, 0] = -1
        tail[:, 0, 1] = totals
        blocks.append(np.concatenate([rows, tail], axis=1))
    return merge_ref(np.stack(blocks), queries)


def split_table():
    """300 rows of 0..40 cuts on a 1/30 s grid; some video ids stand on two rows; 70 rows (3 j + 1) are shifted copies
    of three base rows, which - one as it is, one shifted, one with NaNs - are the queries, next to an empty and a
    NaN-only one"""
    rng = np.random.default_rng(7)
    rows = []
    for r in range(300):
        n = int(rng.integers(0, 41))
        rows.append((1000 + (r if r % 25 else r // 2), np.sort(rng.choice(9000, size=n, replace=False) / 30.0).tolist()))
    base = [rows[i][1] for i in range(300) if i % 3 != 1 and len(rows[i][1]) >= 20][:3]
    for j in range(70):
        rows[3 * j + 1] = (2000 + j // 2, (np.asarray(base[j % 3]) + (j % 11 - 5) / 30.0).tolist())
    queries = [base[0], (np.asarray(base[1]) + 4 / 30).tolist(), base[2] + [float("nan")] * 2, [], [float("nan")] * 3]
    return rows, queries
