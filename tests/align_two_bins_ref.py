"""Plain numpy restatement of TVZ_ALIGN_TWO_BINS on tvz_align_wide_topk, tvz_align_rates_topk and tvz_align_span_topk,
written from the flag's contract in include/tvz.h.  It imports the row rule (align_ref.row_set), n_valid and the block
writers, and the score and order helpers of the three forms' references - never the code under test.

  * at rate rho every non-NaN query value is x' = x * rho (numpy's product of two float64: ONE IEEE multiplication);
  * h[b] = the (row key c, x') pairs with floor((c - x') / eps + 0.5) == b, b in [-B, B] - ALL pairs, no window, no
    run - by np.unique; outside [-B, B] h is 0;
  * J[b] = h[b] + h[b + 1];
  * the best window: a lexsort on (-J, -h, |b|, b) over the bins with votes (a window whose lower bin is empty never
    wins: b + 1 has the same J and h > 0); no votes at all: bin 0, 0 votes;
  * per row the rate with the most J, the smaller index on a tie;
  * the span: P = the pairs in bin b or b + 1 (b + 1 > B holds none); t_first / t_last = min / max index of the
    sorted query over P, c_lo / c_hi = min / max key over P, nr = the row's keys in [c_lo, c_hi]; |P| = J[b];
  * scores, the hit test, the orders and the blocks: those of the three forms' references, fed (best_bin, J).
"""
import math

import numpy as np

from tests import align_rates_ref as arr, align_span_ref as asr, align_topk_ref as atr, align_wide_ref as awr
from tests.align_ref import row_set

TWO_BINS = 8
FORMS = ("wide", "rates", "span")
COLS = {"wide": 4, "rates": 5, "span": 8}


def bins_of(keys, s, eps, B, rho=1.0):
    """-> (c, bin matrix as float64 [len(c), len(s)], ok mask): every pair's bin at the rate rho"""
    c = row_set(keys)
    with np.errstate(over="ignore", invalid="ignore"):
        x = s * np.float64(rho)
        b = np.floor((c[:, None] - x[None, :]) / eps + 0.5)
        ok = (b >= -B) & (b <= B)
    return c, b, ok


def best_window(bins):
    """bins: the int64 bins of every voting pair -> (best_bin, J, h of the best bin); (0, 0, 0) without votes"""
    if bins.size == 0:
        return 0, 0, 0
    b, h = np.unique(bins, return_counts=True)
    at = np.searchsorted(b, b + 1)
    at_c = np.minimum(at, b.size - 1)
    up = np.where((at < b.size) & (b[at_c] == b + 1), h[at_c], 0)
    J = h + up
    first = np.lexsort((b, np.abs(b), -h, -J))[0]                   # last key is the primary one
    return int(b[first]), int(J[first]), int(h[first])


def align_two_bins_ref(rows, query, eps, max_offset, rates=(1.0,)):
    """-> int64 [len(rows), 8]: (video_id, row_len, best_bin = the window's lower bin, votes = J, rate_index, t_first,
    t_last, nr); a row without votes has zeros from column 2 on."""
    B = awr.n_bins(eps, max_offset)
    assert 0 <= B <= awr.MAX_B and 1 <= len(rates) <= arr.MAX_RATES
    s = asr.sorted_query(query)
    out = np.zeros((len(rows), 8), dtype=np.int64)
    for i, (vid, keys) in enumerate(rows):
        out[i, 0] = int(vid)
        out[i, 1] = len(row_set(keys))
        if out[i, 1] == 0 or s.size == 0:
            continue
        best = None
        for ri, rho in enumerate(rates):
            c, b, ok = bins_of(keys, s, eps, B, rho)
            bb, J, _ = best_window(b[ok].astype(np.int64))
            if best is None or J > best[1]:                         # strictly more: a tie keeps the smaller index
                best = (bb, J, ri, c, b, ok)
        bb, J, ri, c, b, ok = best
        if J == 0:
            continue
        ki, ti = np.nonzero(ok & ((b == float(bb)) | (b == float(bb + 1))))
        assert ti.size == J, (i, ti.size, J)                        # |P| is the window's count
        c_lo, c_hi = c[ki].min(), c[ki].max()
        out[i, 2:] = (bb, J, ri, ti.min(), ti.max(), ((c >= c_lo) & (c <= c_hi)).sum())
    return out


def hits_of(form, aligned, nv, min_votes=1, min_score=0, contain=False, local=False, exclude_id=None):
    if form == "wide":
        return awr.hits_of(np.asarray(aligned)[:, :4], nv, min_votes, min_score, contain, exclude_id)
    if form == "rates":
        return arr.hits_of(np.asarray(aligned)[:, :5], nv, min_votes, min_score, contain, exclude_id)
    return asr.hits_of(aligned, nv, min_votes, min_score, contain, local, exclude_id)


def block_of(form, hits, k, refused=False):
    return {"wide": atr.block_of, "rates": arr.block_of, "span": asr.block_of}[form](hits, k, refused=refused)


def topk_two_bins_ref(form, rows, queries, eps, max_offset, k, rates=(1.0,), min_votes=1, min_score=0, contain=False,
                      local=False, exclude_ids=None, max_query_len=None, aligned=None):
    """-> int64[Q, k + 1, COLS[form]].  `aligned` (optional): align_two_bins_ref's outputs per query, computed once by
    the caller (with the call's rates; the wide form's are (1.0,))."""
    assert form in FORMS and (local is False or form == "span")
    lens = [len(list(q)) for q in queries]
    if max_query_len is None:
        max_query_len = min(max(lens, default=0), atr.MAX_LEN)
    out = np.zeros((len(queries), k + 1, COLS[form]), dtype=np.int64)
    for i, q in enumerate(queries):
        if lens[i] > max_query_len:
            out[i] = block_of(form, [], k, refused=True)
            continue
        a = aligned[i] if aligned is not None else align_two_bins_ref(rows, q, eps, max_offset, rates)
        ex = None if exclude_ids is None else int(exclude_ids[i])
        out[i] = block_of(form, hits_of(form, a, atr.n_valid(q), min_votes, min_score, contain, local, ex), k)
    return out


def brute_force(rows, query, eps, max_offset, rho=1.0):
    """A double loop over (row key, query value) in plain Python floats at one rate -> [(video_id, row_len, best_bin, J,
    t_first, t_last, nr)], the last three zero without votes."""
    B = awr.n_bins(eps, max_offset)
    s = sorted(x for x in query if x == x)
    res = []
    for vid, ts in rows:
        keys = row_set(ts).tolist()
        hist, where = {}, {}
        for c in keys:
            for t, x in enumerate(s):
                d = c - x * rho
                if d != d or math.isinf(d):
                    continue
                d = d / eps + 0.5
                if math.isinf(d):
                    continue
                d = math.floor(d)
                if -B <= d <= B:
                    hist[d] = hist.get(d, 0) + 1
                    where.setdefault(d, []).append((c, t))
        if not hist:
            res.append((int(vid), len(keys), 0, 0, 0, 0, 0))
            continue
        J, h, _, b = min((-(n + hist.get(b + 1, 0)), -n, abs(b), b) for b, n in hist.items())
        pairs = where[b] + where.get(b + 1, [])
        c_lo, c_hi = min(c for c, _ in pairs), max(c for c, _ in pairs)
        res.append((int(vid), len(keys), b, -J, min(t for _, t in pairs), max(t for _, t in pairs),
                    sum(1 for c in keys if c_lo <= c <= c_hi)))
    return res


# ---- the copy re-timed to another frame grid --------------------------------------------------------------------------
def retimed_case(seed=7, shift=123.4567, n=200, fps=30, to_fps=25):
    """-> (stored, upload): `n` cuts on a `fps` grid with gaps of 1 to 8 s, and the same cuts moved by -shift and
    rounded to the nearest frame of a `to_fps` grid (a re-encode at another frame rate), printed as %.6g - so stored -
    upload is the shift +- half a frame of the new grid, which at eps = 1 / fps spreads over two bins or three."""
    rng = np.random.default_rng(seed)
    stored = np.cumsum(rng.integers(fps, 8 * fps + 1, size=n)) / float(fps)
    upload = np.round((stored - shift) * to_fps) / float(to_fps)
    upload = np.array([float("%.6g" % x) for x in upload])
    return stored.tolist(), upload.tolist()
