"""Plain numpy restatement of tvz_align_wide_topk, written from its contract in include/tvz.h.  It imports only the
row rule (align_ref.row_set) and the block writer (align_topk_ref.block_of / n_valid), never the code under test.

  * B = floor(max_offset / eps + 0.5), anything in 0..MAX_B;
  * every (row key c, non-NaN query value x) pair votes once into floor((c - x) / eps + 0.5) when that lies in
    [-B, B] (never when it is NaN or infinite) - ALL pairs, no window, no run;
  * best bin: a lexsort of (-votes, |bin|, bin) over the whole range (no votes at all: bin 0, 0 votes);
  * v = min(votes, nv, row_len); u = nv + row_len - v, or min(nv, row_len) with `contain`; s = (v << 20) // u;
  * hit <=> v >= min_votes and s >= min_score and video_id != exclude_id;
  * sorted by the tuple (-s, video_id, best_bin, row_len, votes) - a tuple comparison, no packing.
"""
import math

import numpy as np

from tests.align_ref import row_set
from tests.align_topk_ref import block_of, n_valid

MAX_B = 1 << 22
MAX_LEN = 4095
ONE = 1 << 20


def n_bins(eps, max_offset):
    return int(math.floor(max_offset / eps + 0.5))


def align_wide_ref(rows, query, eps, max_offset, chunk_pairs=1 << 22):
    """-> int64 [len(rows), 4]: (video_id, row_len, best_bin, votes in the best bin)."""
    B = n_bins(eps, max_offset)
    assert 0 <= B <= MAX_B
    nb = 2 * B + 1
    q = np.asarray(list(query), dtype=np.float64).reshape(-1)
    q = q[~np.isnan(q)]
    sets = [row_set(ts) for _, ts in rows]
    R = len(rows)
    out = np.zeros((R, 4), dtype=np.int64)
    out[:, 0] = [int(v) for v, _ in rows]
    out[:, 1] = [len(s) for s in sets]
    if R == 0 or q.size == 0:
        return out
    r0 = 0
    while r0 < R:
        r1, pairs = r0, 0
        while r1 < R and (r1 == r0 or pairs + len(sets[r1]) * q.size <= chunk_pairs):
            pairs += len(sets[r1]) * q.size
            r1 += 1
        lens = np.array([len(s) for s in sets[r0:r1]], dtype=np.int64)
        if lens.sum():
            c = np.concatenate(sets[r0:r1])
            ri = np.repeat(np.arange(r0, r1, dtype=np.int64), lens)
            with np.errstate(invalid="ignore", over="ignore"):
                b = np.floor((c[:, None] - q[None, :]) / eps + 0.5)
                ok = (b >= -B) & (b <= B)
            rr = np.broadcast_to(ri[:, None], b.shape)[ok]
            bins = b[ok].astype(np.int64)
            codes, votes = np.unique(rr * nb + (bins + B), return_counts=True)
            if codes.size:
                row_u, bin_u = codes // nb, codes % nb - B
                order = np.lexsort((bin_u, np.abs(bin_u), -votes, row_u))     # last key is the primary one
                ro = row_u[order]
                first = order[np.r_[True, ro[1:] != ro[:-1]]]
                out[row_u[first], 2] = bin_u[first]
                out[row_u[first], 3] = votes[first]
        r0 = r1
    return out


def score(votes, nv, row_len, contain=False):
    v = min(int(votes), int(nv), int(row_len))
    u = min(int(nv), int(row_len)) if contain else int(nv) + int(row_len) - v
    return v, ((v << 20) // u if u > 0 else 0)


def hits_of(aligned, nv, min_votes=1, min_score=0, contain=False, exclude_id=None):
    """aligned = align_wide_ref's int64[R, 4] for one query -> the sorted list of (key tuple, output row)."""
    hits = []
    for vid, row_len, best_bin, votes in np.asarray(aligned)[:, :4].tolist():
        v, s = score(votes, nv, row_len, contain)
        if v >= min_votes and s >= min_score and (exclude_id is None or vid != exclude_id):
            hits.append(((-s, vid, best_bin, row_len, votes), (vid, row_len, best_bin, votes)))
    hits.sort()
    return hits


def topk_wide_ref(rows, queries, eps, max_offset, k, min_votes=1, min_score=0, contain=False, exclude_ids=None,
                  max_query_len=None, aligned=None):
    """-> int64[Q, k + 1, 4].  `aligned` (optional): align_wide_ref's outputs per query, computed once by the caller."""
    lens = [len(list(q)) for q in queries]
    if max_query_len is None:
        max_query_len = min(max(lens, default=0), MAX_LEN)
    out = np.zeros((len(queries), k + 1, 4), dtype=np.int64)
    for i, q in enumerate(queries):
        if lens[i] > max_query_len:
            out[i] = block_of([], k, refused=True)
            continue
        a = aligned[i] if aligned is not None else align_wide_ref(rows, q, eps, max_offset)
        ex = None if exclude_ids is None else int(exclude_ids[i])
        out[i] = block_of(hits_of(a, n_valid(q), min_votes, min_score, contain, ex), k)
    return out


def brute_force(rows, query, eps, max_offset):
    """A double loop over (row key, query value) in plain Python floats: -> [(video_id, row_len, best_bin, votes)]."""
    B = n_bins(eps, max_offset)
    res = []
    for vid, ts in rows:
        keys = row_set(ts).tolist()
        hist = {}
        for c in keys:
            for x in query:
                if x != x:
                    continue
                t = c - x
                if t != t or math.isinf(t):
                    continue
                t = t / eps + 0.5
                if math.isinf(t):
                    continue
                d = math.floor(t)
                if -B <= d <= B:
                    hist[d] = hist.get(d, 0) + 1
        best = min(((-n, abs(b), b) for b, n in hist.items()), default=(0, 0, 0))   # most votes, smaller |bin|, negative
        res.append((int(vid), len(keys), best[2], -best[0]))
    return res
