"""The contract of include/tvz_gap_long.h restated in numpy on top of tests/gap_candidates_ref.py: the reference of the
tvz_align_candidates_long tests.  No code under test is imported here.  `candidates` counts through Python sets - a
probe's segment is its position's, slot // 8 // 511 -; `candidates_loops` is the same contract as a plain double loop
over (query, row) that cuts the sorted query into runs of 511 positions first, and
tests/test_gap_candidates_long_cpu.py checks one against the other."""
import math

import numpy as np

from tests import gap_candidates_ref as ref

SEG_POSITIONS = 511
MAX_LEN = 4095
REFUSED = ref.REFUSED
INT32_MAX = (1 << 31) - 1


def segments(m):
    """S(m) = ceil((m - 3) / 511) of a query of m sorted values; 0 below 4 values"""
    return 0 if m < 4 else -(-(m - 3) // SEG_POSITIONS)


def lists_per_query(max_query_len):
    return max(segments(min(max_query_len, MAX_LEN)), 1)


def refused(timestamps, max_query_len):
    return len(timestamps) > max_query_len


def segment_counts(rows, query, gap_eps, sets=None):
    """-> int64 [S, n_rows]: c_s(q, row), the probes of segment s, with multiplicity, that are in the row's code set"""
    p = ref.probes(query, gap_eps)
    S = segments(ref.query_values(query).size)
    if sets is None:
        sets = [ref.stored_codes(k, gap_eps) for _, k in rows]
    where = {}
    for r, cs in enumerate(sets):
        for x in cs:
            where.setdefault(x, []).append(r)
    out = np.zeros((S, len(rows)), dtype=np.int64)
    for slot, x in enumerate(p):
        if x is None:
            continue
        for r in where.get(x, ()):
            out[slot // 8 // SEG_POSITIONS, r] += 1
    return out


def sums_of(ids, seg, min_count, exclude_id):
    """-> (dict id -> count(q, id), the hits per segment's list)"""
    ids = np.asarray(ids, dtype=np.int64)
    hit = (seg >= min_count) & (ids != exclude_id)[None, :]
    sums = {}
    for s, r in zip(*np.nonzero(hit)):
        sums[int(ids[r])] = sums.get(int(ids[r]), 0) + int(seg[s, r])
    return sums, hit.sum(axis=1)


def block_of(ids, seg, c, cap, min_count, exclude_id):
    """ids [n_rows], seg int64 [S, n_rows] -> the block int32 [c + 1, 2]"""
    sums, per_list = sums_of(ids, seg, min_count, exclude_id)
    order = sorted(sums.items(), key=lambda kv: (-kv[1], kv[0]))
    out = np.zeros((c + 1, 2), dtype=np.int32)
    out[:, 0] = -1
    for i, (vid, n) in enumerate(order[:c]):
        out[i] = (vid, n)
    if (per_list > cap).any():
        t = min(int(per_list.sum()), INT32_MAX)
        out[c, 1] = -t if t else REFUSED
    else:
        out[c, 1] = min(len(order), INT32_MAX)
    return out


def candidates(rows, queries, gap_eps, c, min_count=2, cap=4096, exclude_ids=None, max_query_len=None):
    """-> int32 [Q, c + 1, 2], the block of tvz_align_candidates_long.  Where a segment's list exceeds `cap` the
    library's rows may be inexact: the one test of that compares the last row and bounds the others."""
    if max_query_len is None:
        max_query_len = min(max([len(q) for q in queries] + [0]), MAX_LEN)
    ids = [i for i, _ in rows]
    sets = [ref.stored_codes(k, gap_eps) for _, k in rows]
    out = np.zeros((len(queries), c + 1, 2), dtype=np.int32)
    for qi, q in enumerate(queries):
        if refused(q, max_query_len):
            out[qi, :, 0], out[qi, c, 1] = -1, REFUSED
            continue
        out[qi] = block_of(ids, segment_counts(rows, q, gap_eps, sets), c, cap, min_count,
                           -1 if exclude_ids is None else exclude_ids[qi])
    return out


def true_sums(rows, query, gap_eps, min_count=2, exclude_id=-1):
    """-> dict id -> count(q, id) with no capacity: what a reported count may not exceed"""
    return sums_of([i for i, _ in rows], segment_counts(rows, query, gap_eps), min_count, exclude_id)[0]


def candidates_loops(rows, queries, gap_eps, c, min_count=2, cap=4096, exclude_ids=None, max_query_len=None):
    """the same contract with Python floats and plain loops: the sorted query is cut into runs of 511 positions, every
    run counted against every row position by position, the sums kept in a sorted list"""
    if max_query_len is None:
        max_query_len = min(max([len(q) for q in queries] + [0]), MAX_LEN)

    def bin_ok(b):
        return 0.0 <= b <= ref.MAX_BIN

    def bins(vals, rounded):
        out = []
        for j in range(len(vals) - 1):
            with np.errstate(invalid="ignore", over="ignore"):
                d = float(np.float64(vals[j + 1]) - np.float64(vals[j]))
                r = d if math.isnan(d) else float(np.float64(d) / np.float64(gap_eps))
            if not math.isfinite(r):
                out.append(float("nan"))
            else:
                out.append(math.floor(r + 0.5) if rounded else math.floor(r))
        return out

    stored = []
    for vid, keys in rows:
        k = sorted({float(x) + 0.0 for x in keys if not math.isnan(float(x))})
        b = bins(k, True)
        stored.append((vid, {(b[t], b[t + 1], b[t + 2]) for t in range(len(k) - 3)
                             if bin_ok(b[t]) and bin_ok(b[t + 1]) and bin_ok(b[t + 2])}))
    out = np.zeros((len(queries), c + 1, 2), dtype=np.int32)
    for qi, q in enumerate(queries):
        out[qi, :, 0] = -1
        if len(q) > max_query_len:
            out[qi, c, 1] = REFUSED
            continue
        s = sorted(float(x) + 0.0 for x in q if not math.isnan(float(x)))
        a = bins(s, False)
        n_pos = max(len(s) - 3, 0)
        excl = -1 if exclude_ids is None else exclude_ids[qi]
        sums, hits_total, over = {}, 0, False
        for first in range(0, n_pos, SEG_POSITIONS):
            in_list = 0
            for vid, triples in stored:
                if vid == excl:
                    continue
                n = 0
                for i in range(first, min(first + SEG_POSITIONS, n_pos)):
                    for v in range(8):
                        g = tuple(a[i + j] + ((v >> j) & 1) for j in range(3))
                        if all(bin_ok(x) for x in g) and g in triples:
                            n += 1
                if n >= min_count:
                    sums[vid] = sums.get(vid, 0) + n
                    in_list += 1
            hits_total += in_list
            over = over or in_list > cap
        kept = sorted((-n, vid) for vid, n in sums.items())
        for i, (neg, vid) in enumerate(kept[:c]):
            out[qi, i] = (vid, -neg)
        if over:
            out[qi, c, 1] = -min(hits_total, INT32_MAX) if hits_total else REFUSED
        else:
            out[qi, c, 1] = len(kept)
    return out
