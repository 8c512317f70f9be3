"""The contract of include/tvz_gap.h restated in numpy: the reference of the tvz_align_candidates tests.  No code under
test is imported here.  `candidates` goes through all positions, all 8 variants, counts through Python sets and a
lexsort on (-count, video_id); `candidates_loops` is the same contract as a plain double loop over (query, row), and
tests/test_gap_candidates_cpu.py checks one against the other."""
import math

import numpy as np

MAX_BIN = (1 << 17) - 1
MAX_PROBES = 4095
REFUSED = -(1 << 31)


def stored_values(timestamps):
    """a row as the handle keeps it: sorted ascending, distinct, NaN dropped, -0.0 folded"""
    a = np.asarray(timestamps, dtype=np.float64).reshape(-1)
    a = a[~np.isnan(a)] + 0.0
    return np.unique(a)


def query_values(timestamps):
    """a query as the alignment calls sort it: ascending, NaNs skipped, duplicates kept, -0.0 folded"""
    a = np.asarray(timestamps, dtype=np.float64).reshape(-1)
    return np.sort(a[~np.isnan(a)] + 0.0, kind="stable")


def ratios(s, gap_eps):
    """r_i = (s[i+1] - s[i]) / gap_eps: one subtraction, one true division"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (s[1:] - s[:-1]) / np.float64(gap_eps)


def valid(b):
    return (b >= 0.0) & (b <= MAX_BIN)            # NaN fails both


def code(g0, g1, g2):
    return int(g0) + (int(g1) << 17) + (int(g2) << 34)


def stored_codes(timestamps, gap_eps):
    """the SET of codes of a stored row"""
    s = stored_values(timestamps)
    if s.size < 4:
        return set()
    with np.errstate(invalid="ignore"):
        b = np.floor(ratios(s, gap_eps) + 0.5)
    ok = valid(b)
    return {code(b[i], b[i + 1], b[i + 2]) for i in range(s.size - 3) if ok[i] and ok[i + 1] and ok[i + 2]}


def probes(timestamps, gap_eps):
    """the probes of a query, with multiplicity, in slot order; None where a slot's choice has an invalid bin"""
    s = query_values(timestamps)
    out = []
    if s.size < 4:
        return out
    a = np.floor(ratios(s, gap_eps))
    for i in range(s.size - 3):
        for v in range(8):
            g = [a[i + j] + ((v >> j) & 1) for j in range(3)]
            out.append(code(*g) if all(valid(x) for x in g) else None)
    return out


def refused(timestamps, max_query_len):
    n = len(timestamps)
    m = query_values(timestamps).size
    return n > max_query_len or 8 * (m - 3) > MAX_PROBES


def counts(rows, query, gap_eps):
    """count(q, r) for every row: the probes of the query, with multiplicity, that are in the row's code set"""
    p = [x for x in probes(query, gap_eps) if x is not None]
    return [sum(1 for x in p if x in cs) for cs in (stored_codes(k, gap_eps) for _, k in rows)]


def block_of(ids, cnt, c, cap, min_count, exclude_id):
    ids, cnt = np.asarray(ids, dtype=np.int64), np.asarray(cnt, dtype=np.int64)
    keep = (cnt >= min_count) & (ids != exclude_id)
    ids, cnt = ids[keep], cnt[keep]
    order = np.lexsort((ids, -cnt))
    out = np.zeros((c + 1, 2), dtype=np.int32)
    out[:, 0] = -1
    n = min(c, order.size)
    out[:n, 0], out[:n, 1] = ids[order[:n]], cnt[order[:n]]
    total = int(order.size)
    out[c, 1] = (-total if total else REFUSED) if total > cap else total
    return out


def candidates(rows, queries, gap_eps, c, min_count=2, cap=4096, exclude_ids=None, max_query_len=None):
    """-> int32 [Q, c + 1, 2], the block of tvz_align_candidates.  Where a total exceeds `cap` the library's rows may be
    inexact: the callers compare the totals row only there."""
    if max_query_len is None:
        max_query_len = max([len(q) for q in queries] + [0])
    sets = [stored_codes(k, gap_eps) for _, k in rows]
    ids = [i for i, _ in rows]
    out = np.zeros((len(queries), c + 1, 2), dtype=np.int32)
    for qi, q in enumerate(queries):
        if refused(q, max_query_len):
            out[qi, :, 0], out[qi, c, 1] = -1, REFUSED
            continue
        p = [x for x in probes(q, gap_eps) if x is not None]
        cnt = [sum(1 for x in p if x in cs) for cs in sets]
        out[qi] = block_of(ids, cnt, c, cap, min_count, -1 if exclude_ids is None else exclude_ids[qi])
    return out


def candidates_loops(rows, queries, gap_eps, c, min_count=2, cap=4096, exclude_ids=None, max_query_len=None):
    """the same contract with Python floats and plain loops: no sets, no numpy arithmetic, an insertion into a sorted
    list instead of the lexsort"""
    if max_query_len is None:
        max_query_len = max([len(q) for q in queries] + [0])

    def bin_ok(b):
        return 0.0 <= b <= MAX_BIN

    def div(d):
        if math.isnan(d):
            return d
        return d / gap_eps

    out = np.zeros((len(queries), c + 1, 2), dtype=np.int32)
    for qi, q in enumerate(queries):
        s = sorted(float(x) + 0.0 for x in q if not math.isnan(float(x)))
        out[qi, :, 0] = -1
        if len(q) > max_query_len or 8 * (len(s) - 3) > MAX_PROBES:
            out[qi, c, 1] = REFUSED
            continue
        kept = []
        for vid, keys in rows:
            k = sorted({float(x) + 0.0 for x in keys if not math.isnan(float(x))})
            if vid == (-1 if exclude_ids is None else exclude_ids[qi]):
                continue
            n = 0
            for i in range(len(s) - 3):
                ra = []
                for j in range(3):
                    with np.errstate(invalid="ignore"):
                        d = float(np.float64(s[i + j + 1]) - np.float64(s[i + j]))
                    r = div(d)
                    ra.append(math.floor(r) if math.isfinite(r) else float("nan"))
                for v in range(8):
                    g = [ra[j] + ((v >> j) & 1) for j in range(3)]
                    if not all(bin_ok(x) for x in g):
                        continue
                    hit = False
                    for t in range(len(k) - 3):
                        same = True
                        for j in range(3):
                            with np.errstate(invalid="ignore"):
                                d = float(np.float64(k[t + j + 1]) - np.float64(k[t + j]))
                            r = div(d)
                            b = math.floor(r + 0.5) if math.isfinite(r) else float("nan")
                            if not bin_ok(b) or b != g[j]:
                                same = False
                                break
                        if same:
                            hit = True
                            break
                    n += hit
            if n >= min_count:
                kept.append((-n, vid))
        kept.sort()
        for i, (neg, vid) in enumerate(kept[:c]):
            out[qi, i] = (vid, -neg)
        total = len(kept)
        out[qi, c, 1] = (-total if total else REFUSED) if total > cap else total
    return out
