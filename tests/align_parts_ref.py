"""Plain numpy restatement of tvz_align_parts, written from its contract in include/tvz.h: brute force over the whole
key x value matrix of every (query, candidate row) pair - no window, no run, no search.  It imports the row rule
(align_ref.row_set), the sorted query of tests/align_span_ref.py and the bin count of tests/align_wide_ref.py, never
the code under test.

  * s = the query's non-NaN values sorted ascending, m of them; at rate rho x'_t = s[t] * rho (numpy's product of two
    float64: the ONE IEEE multiplication); the pair (key c, index t) votes into floor((c - x'_t) / eps + 0.5);
  * the best bin of a set of pairs: most votes inside [-B, B], then the smaller |bin|, then the negative one;
  * part 0: per rate the best bin over ALL pairs; the rate with the most votes, the smaller index on a tie (no vote
    at any rate: rate 0);
  * part i >= 1, at that rate: the ALLOWED pairs have t outside every earlier [t_first, t_last] and c outside every
    earlier [c_lo, c_hi]; their best bin; t_first / t_last / c_lo / c_hi over the allowed pairs at that bin; nq = the
    indices of [t_first, t_last] outside the earlier index ranges, nr = the row's keys of [c_lo, c_hi] outside the
    earlier key ranges;
  * a part is reported iff votes >= min_votes; the first that fails ends the list, and so does max_parts;
  * among the rows of one id: most part-0 votes, then the earlier row;
  * the pair's block int64[1 + max_parts, 6]: (video_id, row_len, rate_index, n_parts, n_rows, m), then (bin, votes,
    t_first, t_last, nq, nr) per reported part and zeros behind them.
"""
import numpy as np

from tests.align_ref import row_set
from tests.align_span_ref import sorted_query
from tests.align_wide_ref import MAX_LEN, n_bins

REFUSED = -(1 << 31)
MAX_PARTS = 4
MAX_ROWS = 8


def bins_of(c, s, eps, rho):
    """-> float64 [len(c), len(s)]: every pair's bin (NaN or infinite where the pair never votes)."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = s * np.float64(rho)
        return np.floor((c[:, None] - x[None, :]) / eps + 0.5)


def best_bin(b, allowed, B):
    """-> (bin, votes) over the allowed pairs whose bin lies in [-B, B]; (0, 0) without a vote."""
    with np.errstate(invalid="ignore"):
        ok = allowed & (b >= -B) & (b <= B)
    if not ok.any():
        return 0, 0
    bins, votes = np.unique(b[ok].astype(np.int64), return_counts=True)
    i = np.lexsort((bins, np.abs(bins), -votes))[0]
    return int(bins[i]), int(votes[i])


def row_parts(keys, query, eps, max_offset, rates, min_votes, max_parts):
    """One candidate row -> (row_len, rate_index, part-0 votes, parts): parts = the REPORTED ones, each (bin, votes,
    t_first, t_last, nq, nr)."""
    assert 1 <= max_parts <= MAX_PARTS and min_votes >= 1 and 1 <= len(rates) <= 8
    B = n_bins(eps, max_offset)
    c, s = row_set(keys), sorted_query(query)
    if c.size == 0 or s.size == 0:
        return int(c.size), 0, 0, []
    everything = np.ones((c.size, s.size), dtype=bool)
    rate, votes0 = 0, 0
    for i, rho in enumerate(rates):
        _, v = best_bin(bins_of(c, s, eps, rho), everything, B)
        if v > votes0:                                    # strictly more: a tie keeps the smaller index
            rate, votes0 = i, v
    b = bins_of(c, s, eps, rates[rate])
    t_free, c_free = np.ones(s.size, dtype=bool), np.ones(c.size, dtype=bool)
    parts = []
    for _ in range(max_parts):
        allowed = c_free[:, None] & t_free[None, :]
        bn, v = best_bin(b, allowed, B)
        if v < min_votes:
            break
        ki, ti = np.nonzero(allowed & (b == float(bn)))
        assert ti.size == v
        t_first, t_last, c_lo, c_hi = int(ti.min()), int(ti.max()), c[ki].min(), c[ki].max()
        in_t = np.zeros(s.size, dtype=bool)
        in_t[t_first:t_last + 1] = True
        in_c = (c >= c_lo) & (c <= c_hi)
        parts.append((bn, v, t_first, t_last, int((in_t & t_free).sum()), int((in_c & c_free).sum())))
        t_free &= ~in_t
        c_free &= ~in_c
    return int(c.size), rate, votes0, parts


def pair_ref(rows, query, video_id, eps, max_offset, rates, min_votes, max_parts, max_query_len=MAX_LEN):
    """rows: the table as (video_id, keys) in table order -> int64 [1 + max_parts, 6]."""
    out = np.zeros((1 + max_parts, 6), dtype=np.int64)
    n = len(list(query))
    refused = n > min(max_query_len, MAX_LEN)
    out[0, 5] = 0 if refused else sorted_query(query).size
    if video_id < 0:
        out[0, 0] = -1
        return out
    out[0, 0] = video_id
    cand = [keys for vid, keys in rows if int(vid) == int(video_id)]
    out[0, 4] = len(cand)
    if refused or len(cand) > MAX_ROWS:
        out[0, 3] = REFUSED
        return out
    best = None
    for keys in cand:                                     # in table order: strictly more votes replaces
        r = row_parts(keys, query, eps, max_offset, rates, min_votes, max_parts)
        if best is None or r[2] > best[2]:
            best = r
    if best is None:
        return out
    row_len, rate, _, parts = best
    out[0, 1:4] = (row_len, rate, len(parts))
    for i, p in enumerate(parts):
        out[1 + i] = p
    return out


def align_parts_ref(rows, queries, video_ids, eps, max_offset, rates=(1.0,), min_votes=1, max_parts=MAX_PARTS,
                    max_query_len=None):
    """-> int64 [Q, k, 1 + max_parts, 6]; video_ids [Q][k]."""
    lens = [len(list(q)) for q in queries]
    if max_query_len is None:
        max_query_len = min(max(lens, default=0), MAX_LEN)
    ids = np.asarray(video_ids, dtype=np.int64).reshape(len(queries), -1)
    out = np.zeros((len(queries), ids.shape[1], 1 + max_parts, 6), dtype=np.int64)
    for q, query in enumerate(queries):
        for j in range(ids.shape[1]):
            out[q, j] = pair_ref(rows, query, int(ids[q, j]), eps, max_offset, rates, min_votes, max_parts, max_query_len)
    return out


def merge_shards_ref(answers):
    """Per pair, among the shards that hold a row of the id, the answer with the most part-0 votes (as reported: 0
    without a reported part), the lower shard on a tie; shard 0's where none holds one; n_rows summed; a pair any shard
    refused stays refused.  answers: int [R, Q, k, 1 + P, 6] -> int64 [Q, k, 1 + P, 6]."""
    a = np.asarray(answers, dtype=np.int64)
    out = a[0].copy()
    for q in range(a.shape[1]):
        for j in range(a.shape[2]):
            best = None
            for r in range(a.shape[0]):
                if a[r, q, j, 0, 4] > 0 and (best is None or a[r, q, j, 1, 1] > a[best, q, j, 1, 1]):
                    best = r
            best = 0 if best is None else best
            out[q, j] = a[best, q, j]
            out[q, j, 0, 4] = a[:, q, j, 0, 4].sum()
            if (a[:, q, j, 0, 3] == REFUSED).any():
                out[q, j, 1:] = 0
                out[q, j, 0, 1:4] = (0, 0, REFUSED)
    return out
