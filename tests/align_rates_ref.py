"""Plain numpy restatement of tvz_align_rates_topk and tvz_align_rates_topk_merge, written from their contract in
include/tvz.h on top of tests/align_wide_ref.py (the votes and bins of one rate) and tests/align_topk_ref.py (n_valid,
the refusal's total).  It never imports the code under test.

  * at rate i every query value is x' = x * rho_i - numpy's product of two float64 is the ONE IEEE multiplication
    rounded to nearest - and the pair (c, x) votes into floor((c - x') / eps + 0.5) when that lies in [-B, B]:
    align_wide_ref(rows, q * rho_i, ...);
  * per row the rate with the MOST raw votes in its best bin, the smaller index on equal votes; no votes at any rate:
    rate 0, bin 0;
  * v = min(votes, nv, row_len) with nv = the query's non-NaN count whatever the rate; u = nv + row_len - v, or
    min(nv, row_len) with `contain`; s = (v << 20) // u; hit <=> v >= min_votes and s >= min_score and video_id !=
    exclude_id;
  * sorted by the tuple (-s, video_id, best_bin, row_len, votes, rate_index) - a tuple comparison, no packing;
  * the block int64[k + 1, 5]: k rows (video_id, row_len, best_bin, votes, rate_index), padding (-1, 0, 0, 0, 0), then
    (-1, n_hits, 0, 0, 0), n_hits = INT32_MIN for a refused query.
"""
import numpy as np

from tests import align_topk_ref as atr, align_wide_ref as awr

MAX_RATES = 8
INT32_MAX = (1 << 31) - 1


def align_rates_ref(rows, query, eps, max_offset, rates):
    """-> int64 [len(rows), 5]: (video_id, row_len, best_bin, votes in the best bin, rate_index)."""
    assert 1 <= len(rates) <= MAX_RATES
    q = np.asarray(list(query), dtype=np.float64).reshape(-1)
    out = np.zeros((len(rows), 5), dtype=np.int64)
    for i, rho in enumerate(rates):
        with np.errstate(over="ignore", invalid="ignore"):
            scaled = q * np.float64(rho)
        a = awr.align_wide_ref(rows, scaled, eps, max_offset)
        if i == 0:
            out[:, :4] = a
            continue
        better = a[:, 3] > out[:, 3]                      # strictly more votes: a tie keeps the smaller index
        out[better, :4] = a[better]
        out[better, 4] = i
    return out


def hits_of(aligned, nv, min_votes=1, min_score=0, contain=False, exclude_id=None):
    """aligned = align_rates_ref's int64[R, 5] for one query -> the sorted list of (key tuple, output row)."""
    hits = []
    for vid, row_len, best_bin, votes, rate in np.asarray(aligned).tolist():
        v, s = awr.score(votes, nv, row_len, contain)
        if v >= min_votes and s >= min_score and (exclude_id is None or vid != exclude_id):
            hits.append(((-s, vid, best_bin, row_len, votes, rate), (vid, row_len, best_bin, votes, rate)))
    hits.sort()
    return hits


def block_of(hits, k, refused=False):
    out = np.zeros((k + 1, 5), dtype=np.int64)
    out[:, 0] = -1
    if refused:
        out[k, 1] = atr.REFUSED
        return out
    for i, (_, row) in enumerate(hits[:k]):
        out[i] = row
    out[k, 1] = len(hits)
    return out


def topk_rates_ref(rows, queries, eps, max_offset, rates, k, min_votes=1, min_score=0, contain=False, exclude_ids=None,
                   max_query_len=None, aligned=None):
    """-> int64[Q, k + 1, 5].  `aligned` (optional): align_rates_ref's outputs per query, computed once by the caller."""
    lens = [len(list(q)) for q in queries]
    if max_query_len is None:
        max_query_len = min(max(lens, default=0), atr.MAX_LEN)
    out = np.zeros((len(queries), k + 1, 5), dtype=np.int64)
    for i, q in enumerate(queries):
        if lens[i] > max_query_len:
            out[i] = block_of([], k, refused=True)
            continue
        a = aligned[i] if aligned is not None else align_rates_ref(rows, q, eps, max_offset, rates)
        ex = None if exclude_ids is None else int(exclude_ids[i])
        out[i] = block_of(hits_of(a, atr.n_valid(q), min_votes, min_score, contain, ex), k)
    return out


# ---- the merge -----------------------------------------------------------------------------------------------------
def sorted_rows(rows, nv, contain=False):
    """live rows of one query in the contract's order: a row with video_id < 0 is padding wherever it stands, and so is
    one whose u is 0 under the score kind; the rate index is the sixth field of the order and nothing else"""
    live = []
    for r in rows:
        vid, row_len, _bin, votes, rate = (int(x) for x in r)
        v = min(votes, int(nv), row_len)
        u = min(int(nv), row_len) if contain else int(nv) + row_len - v
        if vid < 0 or u == 0:
            continue
        live.append(((-((v << 20) // u), vid, _bin, row_len, votes, rate), (vid, row_len, _bin, votes, rate)))
    live.sort()
    return [row for _, row in live]


def merge_ref(blocks, queries, contain=False):
    """blocks int[R, Q, k + 1, 5], queries (host lists) -> rows int64[Q, k, 5], totals int64[Q]"""
    blocks = np.asarray(blocks, dtype=np.int64)
    R, Q, k1, _ = blocks.shape
    k = k1 - 1
    rows = np.zeros((Q, k, 5), dtype=np.int64)
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


def merge_block_of(rows, nv, k, contain=False, n_hits=None):
    """One list as tvz_align_rates_topk writes it: the k best of `rows` in order, padding, then (-1, n_hits, 0, 0, 0)."""
    out = np.zeros((k + 1, 5), dtype=np.int64)
    out[:, 0] = -1
    live = sorted_rows(rows, nv, contain)
    for i, r in enumerate(live[:k]):
        out[i] = r
    out[k, 1] = len(live) if n_hits is None else n_hits
    return out


# ---- the case that tells one rounding of the product from a fused multiply-subtract ---------------------------------
def no_fma_case():
    """-> (c, x, rho, eps, j): x * rho is inexact, c = fl(x * rho) + (j - 0.5) * eps exactly, so the contract's
    (c - fl(x * rho)) / eps + 0.5 is the integer j and the pair votes into bin j.  The product rounds DOWN here
    (fl(x * rho) < x * rho), so a fused c - x * rho, rounded once, is smaller than (j - 0.5) * eps and lands in bin
    j - 1.  tests/test_align_rates_cpu.py asserts all of this with fractions."""
    eps = 1.0 / 64                             # dyadic: (j - 0.5) * eps and the sum below are exact
    x, rho, j = 777.7, 0.96, 37
    p = np.float64(x) * np.float64(rho)
    c = float(p) + (j - 0.5) * eps
    return c, x, rho, eps, j
