"""The contract of include/tvz_gap_rates.h restated in numpy on top of tests/gap_candidates_ref.py: scale the sorted
query by ONE multiplication, then that reference's probes word for word; a per-id maximum with a Python dict, then a
lexsort on (-best, video_id).  No code under test is imported here.  `candidates_rates_loops` is the same contract as
plain loops over (query, rate, row) with Python floats; tests/test_gap_candidates_rates_cpu.py checks one against the
other."""
import math
from collections import Counter

import numpy as np

from tests import gap_candidates_ref as ref

REFUSED = ref.REFUSED
MAX_RATES = 8


def scaled(timestamps, rho):
    """x' = x * rho on the sorted query: one IEEE multiplication per value (a positive rate keeps the order)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return ref.query_values(timestamps) * np.float64(rho)


def probes(timestamps, gap_eps, rho):
    """the probes of a query at the rate rho: tests/gap_candidates_ref.py's probes of the scaled values"""
    return ref.probes(scaled(timestamps, rho), gap_eps)


def count_matrix(rows, queries, gap_eps, rates, max_query_len=None):
    """-> per query None (refused) or an int64 array [n_rates, n_rows]: count_i(q, row)"""
    if max_query_len is None:
        max_query_len = max([len(q) for q in queries] + [0])
    sets = [ref.stored_codes(k, gap_eps) for _, k in rows]
    out = []
    for q in queries:
        if ref.refused(q, max_query_len):
            out.append(None)
            continue
        m = np.zeros((len(rates), len(rows)), dtype=np.int64)
        for i, rho in enumerate(rates):
            p = Counter(x for x in probes(q, gap_eps, rho) if x is not None)
            for r, codes in enumerate(sets):
                m[i, r] = sum(p[x] for x in codes if x in p)
        out.append(m)
    return out


def block_of(ids, m, c, cap, min_count, exclude_id):
    """one query's block int32 [c + 1, 3] from its count matrix"""
    out = np.zeros((c + 1, 3), dtype=np.int32)
    out[:, 0] = -1
    if m is None:
        out[c, 1] = REFUSED
        return out
    best = {}                                                  # id -> (best, rate_index)
    n_pairs, over = 0, False
    for i in range(m.shape[0]):
        listed = 0
        for r, vid in enumerate(ids):
            n = int(m[i, r])
            if n < min_count or vid == exclude_id:
                continue
            listed += 1
            if vid not in best or n > best[vid][0]:            # (rates in ascending index: a tie keeps the smaller)
                best[vid] = (n, i)
        n_pairs += listed
        over = over or listed > cap
    vids = np.asarray(sorted(best), dtype=np.int64)
    cnt = np.asarray([best[v][0] for v in vids], dtype=np.int64)
    order = np.lexsort((vids, -cnt))[:c]
    for j, o in enumerate(order):
        out[j] = (vids[o], cnt[o], best[int(vids[o])][1])
    total = min(n_pairs, 0x7FFFFFFF)
    out[c, 1] = (-total if total else REFUSED) if over else total
    return out


def blocks(rows, matrix, c, min_count=2, cap=4096, exclude_ids=None):
    ids = [i for i, _ in rows]
    return np.stack([block_of(ids, m, c, cap, min_count, -1 if exclude_ids is None else exclude_ids[q])
                     for q, m in enumerate(matrix)]) if matrix else np.zeros((0, c + 1, 3), dtype=np.int32)


def candidates_rates(rows, queries, gap_eps, rates, c, min_count=2, cap=4096, exclude_ids=None, max_query_len=None):
    """-> int32 [Q, c + 1, 3], the block of tvz_align_candidates_rates.  Where a rate's list exceeds `cap` the library's
    rows may be inexact: the callers compare the totals row only there."""
    assert 1 <= len(rates) <= MAX_RATES and all(0.0 < r < math.inf for r in rates)
    return blocks(rows, count_matrix(rows, queries, gap_eps, rates, max_query_len), c, min_count, cap, exclude_ids)


def candidates_rates_loops(rows, queries, gap_eps, rates, c, min_count=2, cap=4096, exclude_ids=None, max_query_len=None):
    """the same contract with Python floats and plain loops: no sets, no Counter, no numpy arithmetic but the single
    operations the contract names; an insertion into a sorted list instead of the lexsort"""
    if max_query_len is None:
        max_query_len = max([len(q) for q in queries] + [0])

    def bins(values, half):
        out = []
        for lo, hi in zip(values[:-1], values[1:]):
            with np.errstate(invalid="ignore", over="ignore"):
                d = float(np.float64(hi) - np.float64(lo))
                r = d if math.isnan(d) else float(np.float64(d) / np.float64(gap_eps))
            b = math.floor(r + half) if math.isfinite(r) else float("nan")
            out.append(b)
        return out

    def ok(b):
        return 0.0 <= b <= ref.MAX_BIN

    stored = []
    for vid, keys in rows:
        k = sorted({float(x) + 0.0 for x in keys if not math.isnan(float(x))})
        b = bins(k, 0.5) if len(k) >= 4 else []
        stored.append([(b[t], b[t + 1], b[t + 2]) for t in range(len(b) - 2) if ok(b[t]) and ok(b[t + 1]) and ok(b[t + 2])])
    out = np.zeros((len(queries), c + 1, 3), dtype=np.int32)
    for qi, q in enumerate(queries):
        out[qi, :, 0] = -1
        s = sorted(float(x) + 0.0 for x in q if not math.isnan(float(x)))
        if len(q) > max_query_len or 8 * (len(s) - 3) > ref.MAX_PROBES:
            out[qi, c, 1] = REFUSED
            continue
        excl = -1 if exclude_ids is None else exclude_ids[qi]
        best, n_pairs, over = [], 0, False                     # best: [vid, count, rate]
        for i, rho in enumerate(rates):
            with np.errstate(invalid="ignore", over="ignore"):
                x = [float(np.float64(v) * np.float64(rho)) for v in s]
            a = bins(x, 0.0) if len(x) >= 4 else []
            listed = 0
            for (vid, _), triples in zip(rows, stored):
                n = 0
                for t in range(len(a) - 2):
                    for v in range(8):
                        g = (a[t] + (v & 1), a[t + 1] + ((v >> 1) & 1), a[t + 2] + ((v >> 2) & 1))
                        if ok(g[0]) and ok(g[1]) and ok(g[2]):
                            n += any(g == tr for tr in triples)
                if n < min_count or vid == excl:
                    continue
                listed += 1
                for e in best:
                    if e[0] == vid:
                        if n > e[1]:
                            e[1], e[2] = n, i
                        break
                else:
                    best.append([vid, n, i])
            n_pairs += listed
            over = over or listed > cap
        kept = sorted((-n, vid, i) for vid, n, i in best)
        for j, (neg, vid, i) in enumerate(kept[:c]):
            out[qi, j] = (vid, -neg, i)
        out[qi, c, 1] = (-n_pairs if n_pairs else REFUSED) if over else n_pairs
    return out
