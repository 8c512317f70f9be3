"""Plain float64 restatement of the tolerant match (tvz_find_duplicates_tol / tvz_match_tol), written from its
contract in include/tvz.h, in two forms that must agree:

  * match(i, r) <=> q[i] is not NaN and some key of row r has key == q[i] or fabs(q[i] - key) <= tol, with
    q[i] - key ONE IEEE double subtraction (numpy float64 arithmetic is exactly that);
  * count = #{i : match(i, r)} (query multiplicity counts; a row key may serve several q[i]);
  * kth = index of the min_match-th matching query element (NEVER if count < min_match, -1 if min_match <= 0);
  * hit <=> count >= min_match and video_id != exclude_id.

`brute` tests every (query element, row key) pair.  `searchsorted` tests, for every query element, only the two
row keys numerically next to it (the keys that match one value are contiguous in numeric order, because
fl(q - key) never increases as key grows) - fast enough for the 100k-row corpus.
"""
import numpy as np

NEVER = 0x7FFFFFFF


def row_set(ts):
    """A row as the corpus keeps it: NaN dropped, -0.0 folded to +0.0, each value once, numerically sorted."""
    c = np.asarray(list(ts), dtype=np.float64).reshape(-1)
    c = c[~np.isnan(c)]
    c = np.where(c == 0.0, 0.0, c)
    return np.unique(c)


def _kth(mask, min_match):
    if min_match <= 0:
        return -1
    idx = np.flatnonzero(mask)
    return int(idx[min_match - 1]) if idx.size >= min_match else NEVER


def match_mask_brute(q, row, tol):
    """bool[len(q)]: which query elements match the row (every pair tested)."""
    q = np.asarray(q, dtype=np.float64)
    row = np.asarray(row, dtype=np.float64)
    if q.size == 0 or row.size == 0:
        return np.zeros(q.size, dtype=bool)
    with np.errstate(invalid="ignore"):
        d = q[:, None] - row[None, :]
        m = (q[:, None] == row[None, :]) | (np.abs(d) <= tol)
    return m.any(axis=1)


def match_mask_sorted(q, row_sorted, tol):
    """The same from the two numeric neighbours of each query value in the (numerically sorted) row."""
    q = np.asarray(q, dtype=np.float64)
    r = np.asarray(row_sorted, dtype=np.float64)
    out = np.zeros(q.size, dtype=bool)
    if q.size == 0 or r.size == 0:
        return out
    live = ~np.isnan(q)
    ql = q[live]
    j = np.searchsorted(r, ql, side="left")             # first key >= q
    hit = np.zeros(ql.size, dtype=bool)
    with np.errstate(invalid="ignore"):
        for jj in (j, j - 1):
            ok = (jj >= 0) & (jj < r.size)
            k = r[np.clip(jj, 0, r.size - 1)]
            hit |= ok & ((ql == k) | (np.abs(ql - k) <= tol))
    out[live] = hit
    return out


def find_duplicates_tol(rows, query, tol, min_match, exclude_id=-1, form="brute"):
    """rows: [(video_id, timestamps)] -> sorted [(video_id, count, kth)] of the hits (as the library returns them)."""
    q = np.asarray(list(query), dtype=np.float64).reshape(-1)
    out = []
    for vid, ts in rows:
        r = row_set(ts)
        m = match_mask_brute(q, r, tol) if form == "brute" else match_mask_sorted(q, r, tol)
        cnt = int(m.sum())
        if cnt >= min_match and int(vid) != (exclude_id if exclude_id >= 0 else -1):
            out.append((int(vid), cnt, _kth(m, min_match)))
    return sorted(out)


def find_duplicates_tol_csr(ids, offsets, keys, query, tol, min_match, exclude_id=-1):
    """The searchsorted form over a CSR corpus (synth.synth_timestamp_corpus): for large corpora."""
    return find_duplicates_tol(((int(ids[c]), keys[offsets[c]:offsets[c + 1]]) for c in range(len(ids))),
                               query, tol, min_match, exclude_id, form="sorted")


def pts_time(pts, tb_num, tb_den):
    """showinfo's printed pts_time: pts x time_base, printed with %.6g and read back as float64."""
    return float("%.6g" % (pts * tb_num / tb_den))


def edge_rows_and_queries():
    """Hand-made edge cases: (name, rows, query, tol)."""
    inf, nan = float("inf"), float("nan")
    tiny = 5e-324
    t = 0.001
    return [
        ("query NaN", [(1, [1.0, 2.0])], [nan, 1.0, nan, 2.0005], t),
        ("+-inf rows and query", [(1, [inf, -inf, 3.0]), (2, [inf]), (3, [1e308])], [inf, -inf, 3.0, 1.7976931348623157e308], t),
        ("-0.0 vs +0.0", [(1, [-0.0, 5.0]), (2, [0.0])], [0.0, -0.0, 5e-4], t),
        ("negative keys, windows straddling 0", [(1, [-2.0, -1.0, -0.0005, 0.0004, 1.0]), (2, [-0.0009, 0.0009])],
         [-1.0005, -0.0002, 0.0, 0.0002, 0.9995, -2.001], t),
        ("negative only rows", [(1, [-3.0, -2.0, -1.0]), (2, [-0.5])], [-2.0004, -1.0, -0.5, -3.0, 0.0], t),
        ("subnormal keys", [(1, [tiny, 2 * tiny, -tiny]), (2, [1e-310])], [0.0, tiny, 3 * tiny, -2 * tiny], 0.0),
        ("subnormal tol", [(1, [tiny, 4 * tiny, -tiny]), (2, [0.0])], [0.0, 2 * tiny, 6 * tiny, -3 * tiny], tiny),
        ("exactly at tol and one ulp beyond", [(1, [10.0])], [10.0 + t, 10.0 - t, np.nextafter(10.0 + t, 20.0),
                                                            np.nextafter(10.0 - t, 0.0)], t),
        ("repeated query value", [(1, [1.0, 7.0])], [1.0, 1.0, 1.0005, 1.0, 7.0], t),
        ("two row keys in one window (counted once)", [(1, [5.0, 5.0004, 5.0008])], [5.0004, 9.0], t),
        ("one key in two windows (counted twice)", [(1, [5.0])], [4.9995, 5.0005, 6.0], t),
        ("empty query", [(1, [1.0]), (2, [])], [], t),
        ("empty rows", [(1, []), (2, [nan])], [1.0, 2.0], t),
        ("large tol spans everything", [(1, [-100.0, 0.0, 100.0]), (2, [50.0])], [-1000.0, -50.0, 0.0, 1e5, -0.0], 200.0),
    ]
