"""Plain numpy restatement of tvz_align_span_topk and tvz_align_span_topk_merge, written from their contract in
include/tvz.h on top of tests/align_rates_ref.py (the row's best bin, votes and rate) and tests/align_wide_ref.py (the
two global scores).  It never imports the code under test.

  * for a row the rates reference has chosen (best_bin, rate_index); s = the query's non-NaN values sorted ascending,
    x'_t = s[t] * rho (numpy's product of two float64: the ONE IEEE multiplication);
  * P = ALL pairs (row key c, index t) with floor((c - x'_t) / eps + 0.5) == best_bin, by brute force over the whole
    key x value matrix - no run, no search; |P| must be the rates reference's votes;
  * t_first / t_last = min / max t over P, nq = t_last - t_first + 1; c_lo / c_hi = min / max key over P, nr = the
    row's keys in [c_lo, c_hi];
  * score: the Jaccard or the containment of align_wide_ref.score, or with `local` v = min(votes, nq, nr),
    s = (v << 20) // (nq + nr - v); `contain` and `local` together are refused;
  * hit <=> v >= min_votes and s >= min_score and video_id != exclude_id, v and s of the call's kind;
  * sorted by the tuple (-s, video_id, best_bin, row_len, votes, rate_index, t_first, t_last, nr);
  * the block int64[k + 1, 8]: k rows, padding (-1, 0, ...), then (-1, n_hits, 0, ...), INT32_MIN for a refused query.
"""
import numpy as np

from tests import align_rates_ref as arr, align_topk_ref as atr, align_wide_ref as awr
from tests.align_ref import row_set

LOCAL = 2
CONTAIN = 1
INT32_MAX = (1 << 31) - 1
T_MAX = 4094                                   # the largest index of a query of 4,095 values


def sorted_query(query):
    q = np.asarray(list(query), dtype=np.float64).reshape(-1)
    return np.sort(q[~np.isnan(q)])


def pairs_of(keys, query, eps, best_bin, rho):
    """-> (key indexes, t indexes) of P, over the whole matrix."""
    c = row_set(keys)
    s = sorted_query(query)
    if c.size == 0 or s.size == 0:
        return c, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        x = s * np.float64(rho)
        b = np.floor((c[:, None] - x[None, :]) / eps + 0.5)
    ki, ti = np.nonzero(b == float(best_bin))
    return c, ki, ti


def span_of(keys, query, eps, best_bin, rho):
    """-> (|P|, t_first, t_last, nr); all zero where P is empty."""
    c, ki, ti = pairs_of(keys, query, eps, best_bin, rho)
    if ti.size == 0:
        return 0, 0, 0, 0
    c_lo, c_hi = c[ki].min(), c[ki].max()
    return int(ti.size), int(ti.min()), int(ti.max()), int(((c >= c_lo) & (c <= c_hi)).sum())


def align_span_ref(rows, query, eps, max_offset, rates):
    """-> int64 [len(rows), 8]: align_rates_ref's five columns, then (t_first, t_last, nr); a row without votes has
    zeros there (it is never a hit)."""
    a = arr.align_rates_ref(rows, query, eps, max_offset, rates)
    out = np.zeros((len(rows), 8), dtype=np.int64)
    out[:, :5] = a
    for i, (_, keys) in enumerate(rows):
        if a[i, 3] == 0:
            continue
        n, t_first, t_last, nr = span_of(keys, query, eps, int(a[i, 2]), rates[int(a[i, 4])])
        assert n == a[i, 3], (i, n, a[i].tolist())                  # |P| is the raw votes
        out[i, 5:] = (t_first, t_last, nr)
    return out


def local_score(votes, nq, nr):
    """-> (v, s); (0, 0) where a side is empty."""
    votes, nq, nr = int(votes), int(nq), int(nr)
    if nq <= 0 or nr <= 0:
        return 0, 0
    v = min(votes, nq, nr)
    return v, (v << 20) // (nq + nr - v)


def score_of(row, nv, contain=False, local=False):
    assert not (contain and local)
    vid, row_len, _bin, votes, _rate, t_first, t_last, nr = (int(x) for x in row)
    if local:
        return local_score(votes, t_last - t_first + 1, nr)
    return awr.score(votes, nv, row_len, contain)


def hits_of(aligned, nv, min_votes=1, min_score=0, contain=False, local=False, exclude_id=None):
    hits = []
    for row in np.asarray(aligned).tolist():
        if row[3] == 0:
            continue                                                 # no votes: no span, never a hit (min_votes >= 1)
        v, s = score_of(row, nv, contain, local)
        if v >= min_votes and s >= min_score and (exclude_id is None or row[0] != exclude_id):
            hits.append(((-s, row[0], row[2], row[1], row[3], row[4], row[5], row[6], row[7]), tuple(row)))
    hits.sort()
    return hits


def block_of(hits, k, refused=False):
    out = np.zeros((k + 1, 8), dtype=np.int64)
    out[:, 0] = -1
    if refused:
        out[k, 1] = atr.REFUSED
        return out
    for i, (_, row) in enumerate(hits[:k]):
        out[i] = row
    out[k, 1] = len(hits)
    return out


def topk_span_ref(rows, queries, eps, max_offset, rates, k, min_votes=1, min_score=0, contain=False, local=False,
                  exclude_ids=None, max_query_len=None, aligned=None):
    """-> int64[Q, k + 1, 8].  `aligned` (optional): align_span_ref's outputs per query, computed once by the caller."""
    lens = [len(list(q)) for q in queries]
    if max_query_len is None:
        max_query_len = min(max(lens, default=0), atr.MAX_LEN)
    out = np.zeros((len(queries), k + 1, 8), dtype=np.int64)
    for i, q in enumerate(queries):
        if lens[i] > max_query_len:
            out[i] = block_of([], k, refused=True)
            continue
        a = aligned[i] if aligned is not None else align_span_ref(rows, q, eps, max_offset, rates)
        ex = None if exclude_ids is None else int(exclude_ids[i])
        out[i] = block_of(hits_of(a, atr.n_valid(q), min_votes, min_score, contain, local, ex), k)
    return out


# ---- the merge -----------------------------------------------------------------------------------------------------
def sorted_rows(rows, nv, contain=False, local=False):
    """live rows of one query in the contract's order.  Padding wherever it stands: video_id < 0; t_first or t_last
    outside 0..4094; under `local` nq <= 0 or nr <= 0; otherwise u = 0 under the score kind.  votes is an unsigned
    32-bit count."""
    assert not (contain and local)
    live = []
    for r in rows:
        vid, row_len, _bin, votes, rate, t_first, t_last, nr = (int(x) for x in r)
        if vid < 0 or not (0 <= t_first <= T_MAX and 0 <= t_last <= T_MAX):
            continue
        uvotes = votes & 0xffffffff
        if local:
            nq = t_last - t_first + 1
            if nq <= 0 or nr <= 0:
                continue
            v = min(uvotes, nq, nr)
            s = (v << 20) // (nq + nr - v)
        else:
            v = min(uvotes, int(nv), row_len & 0xffffffff)
            u = min(int(nv), row_len) if contain else int(nv) + row_len - v
            if u == 0:
                continue
            s = (v << 20) // u
        live.append(((-s, vid, _bin, row_len, votes, rate, t_first, t_last, nr), tuple(int(x) for x in r)))
    live.sort()
    return [row for _, row in live]


def merge_ref(blocks, queries, contain=False, local=False):
    """blocks int[R, Q, k + 1, 8], queries (host lists) -> rows int64[Q, k, 8], totals int64[Q]"""
    blocks = np.asarray(blocks, dtype=np.int64)
    R, Q, k1, _ = blocks.shape
    k = k1 - 1
    rows = np.zeros((Q, k, 8), dtype=np.int64)
    rows[:, :, 0] = -1
    totals = np.zeros(Q, dtype=np.int64)
    for q in range(Q):
        n_hits = [int(blocks[r, q, k, 1]) for r in range(R)]
        if any(n < 0 for n in n_hits) or len(list(queries[q])) > atr.MAX_LEN:
            totals[q] = atr.REFUSED
            continue
        totals[q] = min(sum(n_hits), INT32_MAX)
        union = [row for r in range(R) for row in blocks[r, q, :k].tolist()]
        best = sorted_rows(union, atr.n_valid(queries[q]), contain, local)[:k]
        if best:
            rows[q, :len(best)] = best
    return rows, totals


def merge_block_of(rows, nv, k, contain=False, local=False, n_hits=None):
    """One list as tvz_align_span_topk writes it: the k best of `rows` in order, padding, then (-1, n_hits, 0, ...)."""
    out = np.zeros((k + 1, 8), dtype=np.int64)
    out[:, 0] = -1
    live = sorted_rows(rows, nv, contain, local)
    for i, r in enumerate(live[:k]):
        out[i] = r
    out[k, 1] = len(live) if n_hits is None else n_hits
    return out


# ---- the copy that is partial on both sides ------------------------------------------------------------------------
def compilation_case(seed=400, shift=-1234.5 + 1 / 90, rate=1.0):
    """-> (film, upload, clip, shift): a stored film of 400 cuts on a 30 fps grid in two hours, and an upload of 400
    cuts - a compilation - that holds 20 consecutive cuts of the film (film[190:210], `clip`) as (clip - shift) / rate,
    between 380 cuts of its own: 100 before 1,200 s and 280 after 9,000 s, so that no pair of theirs with a cut of the
    film (1..7,200 s) lies at the shift at the rates 1.0 and 0.96 (film - rate x own is above -1,199 s or below -1,440
    s).  stored = rate x upload + shift for the clip's cuts; the upload comes sorted, as cuts do."""
    rng = np.random.default_rng(seed)
    film = np.sort(rng.choice(np.arange(30, 30 * 7200), size=400, replace=False)) / 30.0
    clip = film[190:210]
    moved = (clip - shift) / rate
    assert 1200.0 < moved[0] and moved[-1] < 9000.0 and -1440.0 < shift < -1199.0 and rate in (1.0, 0.96)
    own = np.concatenate([rng.choice(np.arange(30, 30 * 1200), size=100, replace=False),
                          rng.choice(np.arange(30 * 9000, 30 * 16000), size=280, replace=False)]) / 30.0 + 0.0123
    upload = np.sort(np.concatenate([own, moved]))
    return film.tolist(), upload.tolist(), clip.tolist(), shift
