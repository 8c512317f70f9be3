"""The reference of tvz_align_wide_topk (tests/align_wide_ref.py) checked without a GPU: against a double loop in
plain Python floats, against the bounded call's reference wherever the bounded call is defined, and the two score
kinds' ranges.  The GPU parity tests (tests/test_align_wide_gpu.py) compare the library with this reference."""
import numpy as np

from tests import align_ref as ar
from tests import align_topk_ref as atr
from tests import align_wide_ref as awr


def test_reference_equals_a_double_loop():
    rng = np.random.default_rng(11)
    rows = [(v, rng.uniform(0, 7200, size=int(rng.integers(0, 9))).tolist()) for v in range(1, 41)]
    rows += [(50, [float("nan"), 10.0, -0.0, 0.0]), (51, [float("inf"), -float("inf"), 3.0]), (52, [1e300, 7.0])]
    query = rng.uniform(0, 7200, size=7).tolist() + [float("nan"), 7.0]                 # 43 rows x 9 values
    for eps, mo in ((1 / 30, awr.MAX_B / 30), (0.001, awr.MAX_B * 0.001), (1 / 64, 100.0), (0.5, 0.0)):
        got = awr.align_wide_ref(rows, query, eps, mo)
        assert [tuple(r) for r in got.tolist()] == awr.brute_force(rows, query, eps, mo), (eps, mo)
    # votes far apart, equal counts: the smaller |bin|, then the negative one, over the whole range
    rows = [(1, [100.0 + 3.0, 100.0 - 40000.0]), (2, [100.0 + 50000.0, 100.0 - 50000.0])]
    got = awr.align_wide_ref(rows, [100.0], 1 / 64, awr.MAX_B / 64)
    assert got.tolist() == [[1, 2, 192, 1], [2, 2, -3_200_000, 1]] == [list(r) for r in awr.brute_force(rows, [100.0], 1 / 64, awr.MAX_B / 64)]


def test_reference_equals_the_bounded_reference_on_its_edge_cases():
    """flags = 0 and B <= 2047: the block of tvz_align_topk, bit for bit (the 20,000-row grid case by a slice)."""
    n_calls = 0
    for name, rows, calls in ar.edge_cases():
        if name == "grid_stride":
            rows = rows[:300] + rows[ar.GRID_WAVES:ar.GRID_WAVES + 300] + rows[2 * ar.GRID_WAVES:2 * ar.GRID_WAVES + 300]
        if name == "boundary":
            rows = rows[::7]
        for q, eps, mo in calls:
            assert ar.n_bins(eps, mo) <= 2047
            a = ar.align_ref(rows, q, eps, mo)
            w = awr.align_wide_ref(rows, q, eps, mo)
            assert (a[:, :4] == w).all(), (name, eps, mo)
            for k, kw in ((1, {}), (16, {"min_votes": 2}), (64, {"min_score": atr.ONE // 3})):
                old = atr.topk_ref(rows, [list(q)], eps, mo, k, aligned=[a], **kw)
                new = awr.topk_wide_ref(rows, [list(q)], eps, mo, k, aligned=[w], **kw)
                assert (old == new).all(), (name, eps, mo, k, kw)
                n_calls += 1
    assert n_calls > 60


def test_both_scores_are_in_range():
    """0 <= s <= 2^20 for both kinds, u >= 1 whenever v >= 1, containment >= Jaccard, and the excerpt of the issue:
    20 aligned cuts of a 400-cut film."""
    for votes in (0, 1, 2, 19, 20, 21, 400, 5000, 1 << 31):
        for nv in (0, 1, 2, 20, 400, 4095):
            for row_len in (0, 1, 2, 20, 400, 100_000):
                vj, sj = awr.score(votes, nv, row_len)
                vc, sc = awr.score(votes, nv, row_len, contain=True)
                assert vj == vc == min(votes, nv, row_len)
                assert 0 <= sj <= sc <= awr.ONE, (votes, nv, row_len)
                if vj >= 1:
                    assert min(nv, row_len) >= vj >= 1 and nv + row_len - vj >= 1
                    assert sc == (vj << 20) // min(nv, row_len) and sj == (vj << 20) // (nv + row_len - vj)
                assert sj == atr.score(votes, nv, row_len)[1]
    assert awr.score(20, 20, 400, contain=True)[1] == awr.ONE and awr.score(20, 20, 400)[1] == awr.ONE // 20


def test_order_is_the_tuple_with_a_signed_bin():
    aligned = np.array([[9, 1, 5000, 1], [9, 1, -5000, 1], [3, 1, 4_000_000, 1], [9, 2, -5000, 1], [9, 1, -5000, 2]])
    hits = awr.hits_of(aligned, nv=1)
    assert [h[1] for h in hits] == [(3, 1, 4_000_000, 1), (9, 1, -5000, 1), (9, 1, -5000, 2), (9, 1, 5000, 1), (9, 2, -5000, 1)]
    assert awr.topk_wide_ref([], [[1.0] * 5], 0.1, 1.0, 3, max_query_len=4)[0].tolist() == \
        [[-1, 0, 0, 0]] * 3 + [[-1, atr.REFUSED, 0, 0]]
