"""tvz_align_topk without a GPU: the reference (tests/align_topk_ref.py) against a brute-force double loop, the
packed word against the tuple order it stands for, the integer threshold the inspector derives from its float one,
the contiguous-run property the sweep's window search rests on, and the declarations."""
import itertools
import math
import os
import re

import numpy as np
import pytest

from tests import align_ref as ar
from tests import align_topk_ref as atr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_equals_a_brute_force_double_loop():
    rng = np.random.default_rng(41)
    for trial in range(12):
        grid = np.arange(0, 400) / 10.0
        rows = [(int(v), rng.choice(grid, size=int(rng.integers(0, 25)), replace=True).tolist())
                for v in rng.permutation(60)[:30]]
        rows.append((int(rows[0][0]), rows[0][1]))                       # two rows of one video id, identical
        rows.append((int(rows[1][0]), rows[1][1][:-1] if rows[1][1] else [1.0]))
        q = (rng.choice(grid, size=int(rng.integers(1, 20)), replace=True) + rng.integers(-3, 4) / 10.0).tolist()
        if trial % 3 == 0:
            q.insert(1, float("nan"))
        eps, mo = [(0.1, 0.5), (0.05, 1.0), (0.2, 0.0)][trial % 3]
        k, min_votes, ex = [(1, 1, None), (5, 2, rows[2][0]), (64, 1, None)][trial % 3]
        nv = atr.n_valid(q)
        bf = atr.brute_force(rows, q, eps, mo)
        aligned = ar.align_ref(rows, q, eps, mo)
        assert [tuple(r[:4]) for r in aligned.tolist()] == bf
        hits = []
        for vid, row_len, best_bin, votes in bf:
            v = min(votes, nv, row_len)
            if v >= min_votes and vid != ex:
                s = (v << 20) // (nv + row_len - v)
                hits.append((-s, vid, best_bin, row_len, votes))
        hits.sort()
        got = atr.topk_ref(rows, [q], eps, mo, k, min_votes=min_votes, exclude_ids=None if ex is None else [ex])[0]
        assert got[k].tolist() == [-1, len(hits), 0, 0]
        exp = [[h[1], h[3], h[2], h[4]] for h in hits[:k]] + [[-1, 0, 0, 0]] * max(0, k - len(hits))
        assert got[:k].tolist() == exp
        # min_score at the score of the last kept hit keeps it (the equality edge) and drops what is below
        if hits:
            s_k = -hits[min(k, len(hits)) - 1][0]
            got = atr.topk_ref(rows, [q], eps, mo, k, min_votes=min_votes, min_score=s_k,
                               exclude_ids=None if ex is None else [ex])[0]
            assert got[k, 1] == sum(1 for h in hits if -h[0] >= s_k) >= min(k, len(hits))


def test_refused_empty_and_nan_only_queries():
    rows = [(1, [1.0, 2.0]), (2, [])]
    got = atr.topk_ref(rows, [[], [float("nan")], [1.0] * 5, [1.0, 2.0]], 0.1, 1.0, 3, max_query_len=4)
    assert got[0, 3].tolist() == got[1, 3].tolist() == [-1, 0, 0, 0]
    assert got[2].tolist() == [[-1, 0, 0, 0]] * 3 + [[-1, atr.REFUSED, 0, 0]]
    assert got[3].tolist() == [[1, 2, 0, 2], [-1, 0, 0, 0], [-1, 0, 0, 0], [-1, 1, 0, 0]]


def test_the_packed_word_orders_as_the_tuple():
    scores = (0, 1, atr.ONE // 2, atr.ONE - 1, atr.ONE)
    vids = (0, 1, 4096, 2 ** 31 - 2, 2 ** 31 - 1)
    bins = (-2047, -1, 0, 1, 2047)
    items = list(itertools.product(scores, vids, bins))
    words = [atr.pack_word(*it) for it in items]
    assert all(0 <= w < 2 ** 64 - 1 for w in words) and len(set(words)) == len(items)      # fits; never the padding
    by_word = [it for _, it in sorted(zip(words, items))]
    assert by_word == sorted(items, key=lambda it: (-it[0], it[1], it[2]))
    # the fields come back out
    for w, (s, vid, b) in zip(words, items):
        assert (atr.ONE - (w >> 43), (w >> 12) & 0x7FFFFFFF, (w & 0xFFF) - 2048) == (s, vid, b)


def test_the_integer_threshold_never_drops_what_the_float_filter_keeps():
    js = sorted({0.0, 1.0, 0.8, 0.5, 1 / 3, 2 / 3, 0.999999, 1e-9, 0.25, 0.75, 0.1}
                | {i / 97 for i in range(98)} | {a / b for b in range(1, 40) for a in range(b + 1)})
    u = np.arange(1, 601, dtype=np.int64)
    for j in js:
        thr = math.floor(j * atr.ONE)
        for v in range(0, 601):
            uu = u[u >= max(v, 1)]
            keep = v / uu.astype(np.float64) >= j
            s = (v << 20) // uu
            assert (s[keep] >= thr).all(), (j, v)


def test_align_score_is_the_references():
    from tvidz_amd import corpus as tc
    rng = np.random.default_rng(3)
    for votes, nv, row_len in rng.integers(0, 5000, size=(2000, 3)).tolist() + [[0, 0, 0], [7, 0, 0], [9, 4095, 1]]:
        assert tc.align_score(votes, nv, row_len) == atr.score(votes, nv, row_len)[1]
    assert tc.ALIGN_SCORE_ONE == atr.ONE and tc.ALIGN_REFUSED == atr.REFUSED


@pytest.mark.parametrize("case", ar.edge_cases(), ids=lambda c: c[0])
def test_the_voting_query_values_are_one_run_of_the_sorted_query(case):
    """For every row key of every edge case and call: the indices of the sorted query that vote are contiguous, and
    the values in front of the run are exactly those the sweep's search predicate calls 'left'."""
    _, rows, calls = case
    keys = np.unique(np.concatenate([ar.row_set(ts) for _, ts in rows] + [np.zeros(0)]))
    for q, eps, mo in calls:
        B = ar.n_bins(eps, mo)
        s = np.asarray(list(q), dtype=np.float64).reshape(-1)
        s = np.sort(s[~np.isnan(s)])
        if s.size == 0:
            continue
        for c in keys.tolist():
            run = atr.voting_run(c, s, eps, B)
            if run.size:
                assert run[-1] - run[0] + 1 == run.size, (c, eps, mo)
            with np.errstate(invalid="ignore", over="ignore"):
                d = np.floor((c - s) / eps + 0.5)
            left = (d > B) | (np.isnan(d) & ((s < c) | ((s == c) & (s < 0))))
            n_left = int(np.count_nonzero(left))
            assert left[:n_left].all() and not left[n_left:].any(), (c, eps, mo)         # a prefix
            if run.size:
                assert run[0] == n_left
            else:                                                                         # nothing behind it votes
                assert n_left == s.size or not (d[n_left] >= -B)


def test_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tvz.h")).read(), flags=re.S)
    assert re.search(r"size_t\s+tvz_align_topk_workspace_bytes\s*\(\s*int32_t Q,\s*int32_t max_query_len,\s*"
                     r"int64_t total_query_keys,\s*int32_t k\s*\)\s*;", src)
    m = re.search(r"int\s+tvz_align_topk\s*\(([^)]*)\)\s*;", src)
    assert m and [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == [
        "c", "d_queries", "d_q_offsets", "Q", "max_query_len", "eps", "max_offset", "min_votes", "min_score",
        "d_exclude_ids", "k", "d_out", "d_workspace", "workspace_bytes", "hip_stream"]
    assert src.index("tvz_align_topk(") > src.index("tvz_align(")
    from tvidz_amd import _lib, corpus as tc
    lib = _lib.load()
    assert _lib.VERSION == 404 and lib.tvz_version() == 404
    for name, n_args in (("tvz_align_topk_workspace_bytes", 4), ("tvz_align_topk", 15)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args
    # the formula of the header: sorted queries + totals + max(6080, 95 Q) lists of k words and k payloads
    for Q, L, keys, k in ((1, 200, 200, 16), (64, 200, 0, 16), (70, 4095, 9000, 64), (1, 0, 0, 1)):
        got = tc.align_topk_workspace_bytes(Q, L, keys, k)
        parts = tc.tol_workspace_bytes(Q, L, max(keys or Q * L, L)) + 4 * Q + max(6080, 95 * Q) * k * 16
        assert parts <= got <= parts + 8 * 256, (Q, L, keys, k, got, parts)
    assert tc.align_topk_workspace_bytes(-1, 1, 0, 1) == 0 and tc.align_topk_workspace_bytes(1, 1, 0, 0) == 0
