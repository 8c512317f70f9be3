"""Plain numpy restatement of tvz_align_parts_flags, written from its contract in include/tvz_parts_flags.h: brute force
over the whole key x value matrix of every (query, candidate row) pair - no window, no carry, no run, no search.  It
imports the row rule (align_ref.row_set), the sorted query of tests/align_span_ref.py and the bin count of
tests/align_wide_ref.py, never the code under test, and shares no function with tests/align_parts_ref.py, which it is
compared against with the flag clear.

  * s = the query's non-NaN values sorted ascending; at rate rho x'_t = s[t] * rho (ONE IEEE multiplication); the pair
    (key c, index t) votes into floor((c - x'_t) / eps + 0.5);
  * for a part i the ALLOWED pairs: all of them for part 0; for i >= 1 those with t outside every earlier [t_first,
    t_last] and c outside every earlier [c_lo, c_hi];
  * h_i[b], b in [-B, B]: the allowed pairs of bin b, by np.unique; 0 outside.  J_i[b] = h_i[b] + h_i[b + 1] with
    TWO_BINS, h_i[b] without;
  * the best: a lexsort on (-J, -h, |b|, b) over the bins with allowed votes;
  * part 0: per rate the best, the rate with the most J, the smaller index on a tie; later parts at that rate;
  * P_i = the allowed pairs in bin b, and with TWO_BINS in bin b + 1 where b + 1 <= B; t_first / t_last / c_lo / c_hi
    over P_i, nq_i / nr_i the indices / keys inside them and outside the earlier ranges; |P_i| = J;
  * a part is reported iff J >= min_votes; the first that fails ends the list, and so does max_parts;
  * among the rows of one id: most part-0 J, then the earlier row; the refused, absent and no-pair forms and the block
    int64[1 + max_parts, 6] as tvz_align_parts has them.
"""
import numpy as np

from tests.align_ref import row_set
from tests.align_span_ref import sorted_query
from tests.align_wide_ref import MAX_LEN, n_bins

TWO_BINS = 8
REFUSED = -(1 << 31)
MAX_PARTS = 4
MAX_ROWS = 8


def pair_bins(c, s, eps, rho, B):
    """-> (float64 [len(c), len(s)] every pair's bin, bool mask of the pairs inside [-B, B])"""
    with np.errstate(over="ignore", invalid="ignore"):
        b = np.floor((c[:, None] - (s * np.float64(rho))[None, :]) / eps + 0.5)
        return b, (b >= -B) & (b <= B)


def best_of(b, voting, two_bins):
    """voting: the allowed pairs inside the range -> (bin, J, h); (0, 0, 0) without one"""
    if not voting.any():
        return 0, 0, 0
    bins, h = np.unique(b[voting].astype(np.int64), return_counts=True)
    count = dict(zip(bins.tolist(), h.tolist()))
    J = np.array([n + (count.get(x + 1, 0) if two_bins else 0) for x, n in count.items()], dtype=np.int64)
    i = np.lexsort((bins, np.abs(bins), -h, -J))[0]                 # the last key is the primary one
    return int(bins[i]), int(J[i]), int(h[i])


def row_parts(keys, query, eps, max_offset, rates, min_votes, max_parts, flags=0):
    """One candidate row -> (row_len, rate_index, part-0 J, parts): the REPORTED parts, each (bin, J, t_first, t_last,
    nq, nr)"""
    assert flags in (0, TWO_BINS) and 1 <= max_parts <= MAX_PARTS and min_votes >= 1 and 1 <= len(rates) <= 8
    two = flags == TWO_BINS
    B = n_bins(eps, max_offset)
    c, s = row_set(keys), sorted_query(query)
    if c.size == 0 or s.size == 0:
        return int(c.size), 0, 0, []
    rate, votes0 = 0, 0
    for i, rho in enumerate(rates):
        b, ok = pair_bins(c, s, eps, rho, B)
        J = best_of(b, ok, two)[1]
        if J > votes0:                                              # strictly more: a tie keeps the smaller index
            rate, votes0 = i, J
    b, ok = pair_bins(c, s, eps, rates[rate], B)
    t_free, c_free = np.ones(s.size, dtype=bool), np.ones(c.size, dtype=bool)
    parts = []
    for _ in range(max_parts):
        voting = ok & c_free[:, None] & t_free[None, :]
        bn, J, _ = best_of(b, voting, two)
        if J < min_votes:
            break
        in_window = (b == float(bn)) | (b == float(bn + 1)) if two else (b == float(bn))
        ki, ti = np.nonzero(voting & in_window)                     # (`voting` keeps b + 1 inside [-B, B])
        assert ti.size == J, (ti.size, J)
        t_first, t_last, c_lo, c_hi = int(ti.min()), int(ti.max()), c[ki].min(), c[ki].max()
        in_t = np.zeros(s.size, dtype=bool)
        in_t[t_first:t_last + 1] = True
        in_c = (c >= c_lo) & (c <= c_hi)
        parts.append((bn, J, t_first, t_last, int((in_t & t_free).sum()), int((in_c & c_free).sum())))
        t_free &= ~in_t
        c_free &= ~in_c
    return int(c.size), rate, votes0, parts


def pair_ref(rows, query, video_id, eps, max_offset, rates, min_votes, max_parts, flags=0, max_query_len=MAX_LEN):
    """rows: the table as (video_id, keys) in table order -> int64 [1 + max_parts, 6]"""
    out = np.zeros((1 + max_parts, 6), dtype=np.int64)
    refused = len(list(query)) > min(max_query_len, MAX_LEN)
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
    for keys in cand:                                               # in table order: strictly more votes replaces
        r = row_parts(keys, query, eps, max_offset, rates, min_votes, max_parts, flags)
        if best is None or r[2] > best[2]:
            best = r
    if best is None:
        return out
    row_len, rate, _, parts = best
    out[0, 1:4] = (row_len, rate, len(parts))
    for i, p in enumerate(parts):
        out[1 + i] = p
    return out


def align_parts_flags_ref(rows, queries, video_ids, eps, max_offset, rates=(1.0,), min_votes=1, max_parts=MAX_PARTS,
                          flags=0, max_query_len=None):
    """-> int64 [Q, k, 1 + max_parts, 6]; video_ids [Q][k]"""
    lens = [len(list(q)) for q in queries]
    if max_query_len is None:
        max_query_len = min(max(lens, default=0), MAX_LEN)
    ids = np.asarray(video_ids, dtype=np.int64).reshape(len(queries), -1)
    out = np.zeros((len(queries), ids.shape[1], 1 + max_parts, 6), dtype=np.int64)
    for q, query in enumerate(queries):
        for j in range(ids.shape[1]):
            out[q, j] = pair_ref(rows, query, int(ids[q, j]), eps, max_offset, rates, min_votes, max_parts, flags,
                                 max_query_len)
    return out


def double_loop(keys, query, eps, max_offset, rho, min_votes, max_parts, number=float):
    """One row at ONE rate with TWO_BINS by a double loop in plain Python numbers -> the reported parts.  `number`:
    float (the IEEE arithmetic of the contract) or fractions.Fraction (exact: for a case whose every quotient lies far
    from a bin's edge, where both must agree)."""
    import math
    B = n_bins(eps, max_offset)
    s = sorted(x for x in query if x == x)
    c = [x for x in row_set(keys).tolist() if not math.isinf(x)]
    pairs = []
    for ci in c:
        for t, x in enumerate(s):
            if math.isinf(x):
                continue
            d = math.floor((number(ci) - number(x) * number(rho)) / number(eps) + number(1) / 2)
            if -B <= d <= B:
                pairs.append((ci, t, d))
    t_gone, c_gone, parts = [], [], []
    t_ok = lambda t: all(not (a <= t <= z) for a, z in t_gone)      # noqa: E731
    c_ok = lambda x: all(not (a <= x <= z) for a, z in c_gone)      # noqa: E731
    for _ in range(max_parts):
        allowed = [(ci, t, d) for ci, t, d in pairs if t_ok(t) and c_ok(ci)]
        h = {}
        for _, _, d in allowed:
            h[d] = h.get(d, 0) + 1
        if not h:
            break
        J, hb, _, b = min((-(n + h.get(d + 1, 0)), -n, abs(d), d) for d, n in h.items())
        if -J < min_votes:
            break
        P = [(ci, t) for ci, t, d in allowed if d in (b, b + 1)]
        tf, tl = min(t for _, t in P), max(t for _, t in P)
        lo, hi = min(x for x, _ in P), max(x for x, _ in P)
        parts.append((b, -J, tf, tl, sum(1 for t in range(tf, tl + 1) if t_ok(t)),
                      sum(1 for x in row_set(keys).tolist() if lo <= x <= hi and c_ok(x))))
        t_gone.append((tf, tl))
        c_gone.append((lo, hi))
    return parts
