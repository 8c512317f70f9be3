"""Plain-Python restatement of tvz_align_topk, written from its contract in include/tvz.h on top of
tests/align_ref.align_ref (votes and bins; imported, not edited):

  votes -> v = min(votes, nv, row_len), u = nv + row_len - v, s = (v << 20) // u
        -> hit <=> v >= min_votes and s >= min_score and video_id != exclude_id
        -> sort by the tuple (-s, video_id, best_bin, row_len, votes)   (a tuple comparison: no packing here)
        -> block int64[k + 1, 4]: the k best as (video_id, row_len, best_bin, votes), padding (-1, 0, 0, 0),
           then (-1, n_hits, 0, 0); n_hits = INT32_MIN and all padding for a query longer than max_query_len.
"""
import numpy as np

from tests import align_ref as ar

ONE = 1 << 20
REFUSED = -(1 << 31)
MAX_LEN = 4095


def n_valid(query):
    q = np.asarray(list(query), dtype=np.float64).reshape(-1)
    return int(np.count_nonzero(~np.isnan(q)))


def score(votes, nv, row_len):
    v = min(int(votes), int(nv), int(row_len))
    u = int(nv) + int(row_len) - v
    return v, ((v << 20) // u if u > 0 else 0)


def pack_word(s, video_id, best_bin):
    """The 64-bit word of the contract (the reference never sorts by it; tests/test_align_topk_cpu.py shows that
    it orders as the tuple does)."""
    return ((ONE - s) << 43) | (int(video_id) << 12) | (int(best_bin) + 2048)


def hits_of(aligned, nv, min_votes=1, min_score=0, exclude_id=None):
    """aligned = align_ref's int64[R, 5] for one query -> the sorted list of (key tuple, output row)."""
    hits = []
    for vid, row_len, best_bin, votes, _zero in aligned.tolist():
        v, s = score(votes, nv, row_len)
        if v >= min_votes and s >= min_score and (exclude_id is None or vid != exclude_id):
            hits.append(((-s, vid, best_bin, row_len, votes), (vid, row_len, best_bin, votes)))
    hits.sort()
    return hits


def block_of(hits, k, refused=False):
    out = np.zeros((k + 1, 4), dtype=np.int64)
    out[:, 0] = -1
    if refused:
        out[k, 1] = REFUSED
        return out
    for i, (_, row) in enumerate(hits[:k]):
        out[i] = row
    out[k, 1] = len(hits)
    return out


def topk_ref(rows, queries, eps, max_offset, k, min_votes=1, min_score=0, exclude_ids=None, max_query_len=None,
             aligned=None):
    """-> int64[Q, k + 1, 4].  `aligned` (optional): align_ref's outputs per query, computed once by the caller."""
    lens = [len(list(q)) for q in queries]
    if max_query_len is None:
        max_query_len = min(max(lens, default=0), MAX_LEN)
    out = np.zeros((len(queries), k + 1, 4), dtype=np.int64)
    for i, q in enumerate(queries):
        if lens[i] > max_query_len:
            out[i] = block_of([], k, refused=True)
            continue
        a = aligned[i] if aligned is not None else ar.align_ref(rows, q, eps, max_offset)
        ex = None if exclude_ids is None else int(exclude_ids[i])
        out[i] = block_of(hits_of(a, n_valid(q), min_votes, min_score, ex), k)
    return out


def brute_force(rows, query, eps, max_offset):
    """A double loop over (row key, query value) in plain Python floats: -> [(video_id, row_len, best_bin, votes)]."""
    import math
    B = ar.n_bins(eps, max_offset)
    res = []
    for vid, ts in rows:
        keys = ar.row_set(ts).tolist()
        hist = {}
        for c in keys:
            for x in query:
                if x != x:
                    continue
                t = c - x
                if t != t or math.isinf(t):
                    continue
                d = math.floor(t / eps + 0.5)
                if -B <= d <= B:
                    hist[d] = hist.get(d, 0) + 1
        best = min(((-n, abs(b), b) for b, n in hist.items()), default=(0, 0, 0))   # most votes, smaller |bin|, negative
        res.append((int(vid), len(keys), best[2], -best[0]))
    return res


def voting_run(c, s, eps, B):
    """Indices t of the sorted query s whose value votes for key c, by the vote's own expression."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.floor((c - s) / eps + 0.5)
    return np.flatnonzero((d >= -B) & (d <= B))
