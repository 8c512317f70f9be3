"""tests/align_ref.py (the plain restatement of tvz_align the GPU parity test compares against) checked
on the CPU: against exact rational arithmetic, against oracle.align_py, and for the power of its
near-boundary case set.  Also the tolerant Jaccard the Inspector derives from the score."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle
from tests import align_ref as ar


def _align_exact(rows, query, eps, max_offset):
    """tvz_align's contract in Fractions: no rounding anywhere."""
    E, M = Fraction(eps), Fraction(max_offset)
    B = math.floor(M / E + Fraction(1, 2))
    q = [Fraction(x) for x in query if not math.isnan(x)]
    out = []
    for vid, ts in rows:
        keys = sorted({Fraction(x) for x in ts if not math.isnan(x)})
        hist = {}
        for c in keys:
            for x in q:
                b = math.floor((c - x) / E + Fraction(1, 2))
                if -B <= b <= B:
                    hist[b] = hist.get(b, 0) + 1
        best_bin, best_votes = 0, hist.get(0, 0)
        for b, v in hist.items():
            if (v, -abs(b), -b) > (best_votes, -abs(best_bin), -best_bin):
                best_bin, best_votes = b, v
        out.append((int(vid), len(keys), best_bin, best_votes, hist.get(0, 0)))
    return out


def _tuples(a):
    return [tuple(int(x) for x in r) for r in a]


def _dyadic_cases():
    """eps a power of two, keys and query values multiples of 2^-10: every float64 step of the
    contract is exact.  Rows at exact half-bin differences, both signs, pin round-half-up."""
    rng = np.random.default_rng(77)
    cases = []
    for eps in (2.0 ** -5, 0.125, 0.5, 1.0, 4.0):
        q = [0.0, 1.0, 1.0, -3.0, 2.5]
        half = [(k + 0.5) * eps for k in range(-6, 6)]
        rows = [(1, [x + d for x in (0.0, 1.0) for d in half]), (2, [d for d in half if d > 0]),
                (3, [d for d in half if d < 0]), (4, [-0.0, 0.0, -3.0]), (5, [])]
        for v in range(6, 40):
            n = int(rng.integers(1, 30))
            rows.append((v, (rng.integers(-8192, 8192, size=n) / 1024.0).tolist()))
        for mo in (0.0, 0.4 * eps, 3 * eps, 5.5 * eps, 40 * eps):
            cases.append((rows, q, eps, mo))
        cases.append((rows, (rng.integers(-4096, 4096, size=25) / 1024.0).tolist(), eps, 7 * eps))
    return cases


def test_reference_equals_exact_rational_arithmetic_on_dyadic_inputs():
    n_half = 0
    for rows, q, eps, mo in _dyadic_cases():
        got = _tuples(ar.align_ref(rows, q, eps, mo))
        assert got == _align_exact(rows, q, eps, mo), (eps, mo)
        n_half += sum(1 for r in got if r[0] in (2, 3) and r[3] > 0)
    assert n_half > 0
    # round half up, both signs: +2.5 bins -> 3, -2.5 bins -> -2
    assert _tuples(ar.align_ref([(1, [2.5])], [0.0], 1.0, 5.0)) == [(1, 1, 3, 1, 0)]
    assert _tuples(ar.align_ref([(1, [-2.5])], [0.0], 1.0, 5.0)) == [(1, 1, -2, 1, 0)]
    assert _tuples(ar.align_ref([(1, [-0.5, 0.5])], [0.0], 1.0, 5.0)) == [(1, 2, 0, 1, 1)]


@pytest.mark.parametrize("case", ar.edge_cases(), ids=lambda c: c[0])
def test_oracle_restatement_equals_reference_on_every_edge_case(case):
    """oracle.align_py (bit-packed tie order) and align_ref (sorted tuples) were written separately:
    on every case the GPU parity test runs they must agree."""
    _, rows, calls = case
    for q, eps, mo in calls:
        exp = _tuples(ar.align_ref(rows, q, eps, mo))
        with np.errstate(invalid="ignore"):                 # inf - inf in the special keys
            assert oracle.align_py(rows, q, eps, mo) == exp, (eps, mo)


def test_boundary_set_tells_division_from_reciprocal_multiplication():
    """The near-boundary keys of ar.boundary_case() are decided by the correctly rounded division: the
    same contract computed with (c - q) * (1 / eps) lands some of them in another bin."""
    _, rows, calls = ar.boundary_case()
    moved = 0
    for q, eps, mo in calls:
        a = ar.align_ref(rows, q, eps, mo)
        b = ar.align_ref(rows, q, eps, mo, reciprocal=True)
        moved += int((a != b).any(axis=1).sum())
    assert moved > 0
    # and the set straddles every half-bin boundary it names: both neighbouring bins occur
    a = ar.align_ref(rows, [0.0], 0.1, 8.1)
    assert len(set(a[:, 2].tolist())) > 100


def test_reference_edge_semantics():
    inf, nan = float("inf"), float("nan")
    # a row is a set: duplicates once, NaN dropped, -0.0 == +0.0; query duplicates each vote
    assert _tuples(ar.align_ref([(3, [1.0, 1.0, nan, -0.0, 0.0])], [1.0, 1.0, nan], 0.1, 1.0)) == [(3, 2, 0, 2, 2)]
    # no votes (empty row, empty / NaN-only query, infinite differences): bin 0, zero votes
    for rows, q in (([(1, [])], [0.0]), ([(1, [0.0])], []), ([(1, [0.0])], [nan]), ([(1, [inf])], [inf])):
        assert _tuples(ar.align_ref(rows, q, 0.1, 1.0)) == [(1, len(ar.row_set(rows[0][1])), 0, 0, 0)]
    # ties: smaller |bin|, then the negative one
    assert _tuples(ar.align_ref([(1, [2.0, -2.0]), (2, [1.0, -2.0]), (3, [-1.0, 1.0])], [0.0], 1.0, 5.0)) == \
        [(1, 2, -2, 1, 0), (2, 2, 1, 1, 0), (3, 2, -1, 1, 0)]
    # the chunking of rows does not change anything
    _, rows, calls = ar.grid_stride_case(3000)
    q, eps, mo = calls[0]
    assert np.array_equal(ar.align_ref(rows, q, eps, mo), ar.align_ref(rows, q, eps, mo, chunk_pairs=50))


# ---- the tolerant Jaccard of Inspector(near_duplicates=True) --------------------------------------
def _near_run(cuts_a, cuts_b):
    from tests.fakes import CutReader, OracleCorpus, cut_inspector
    from tvidz_amd import db as tdb
    store = tdb.Store("sqlite://", corpus=OracleCorpus())
    cuts = {"a.y4m": cuts_a, "b.y4m": cuts_b}
    ins = cut_inspector(store, device="cuda:0", near_duplicates=True, near_eps=1 / 30, near_max_offset=30.0,
                        frame_source=lambda bucket, key, filename, uid: (CutReader(cuts[key], frames=1200), None))
    try:
        return ins.analyze_file("videos", "a.y4m"), ins.analyze_file("videos", "b.y4m")
    finally:
        store.close()


@pytest.mark.parametrize("a,b", [([20.0, 20.0 + 1 / 60], [10.0, 10.0 + 1 / 60]),   # 60 fps, cuts on consecutive frames
                                 ([20.0, 20.01], [10.0, 10.01])])                   # votes = 4: denominator 0
def test_near_duplicates_jaccard_never_exceeds_one(a, b):
    """votes counts (query, row) pairs, so with cuts closer than eps it exceeds either cut count; the
    Jaccard is taken from min(votes, n, row_len): the analysis ends `done` and reports at most 1."""
    rows = [(1, a)]
    assert oracle.align_py(rows, b, 1 / 30, 30.0)[0][3] > 2
    ra, rb = _near_run(a, b)
    assert ra["status"] == "done" and rb["status"] == "done", rb
    assert ra["near_duplicates"] == []
    assert [d["video_id"] for d in rb["near_duplicates"]] == [1]
    nd = rb["near_duplicates"][0]
    assert nd["jaccard"] == 1.0 and abs(nd["shift_seconds"] - 10.0) < 1e-9
