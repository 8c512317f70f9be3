"""The near-duplicate differential's generator is worth running - shown without a device, on the seeds and the case count
of tests/test_near_fuzz_gpu.py: the cases are deterministic and inside every call's contract; the references alone
already reach every mechanism the GPU test's last assertion names; on tiny cases the vectorised references agree with
the double loops beside them; and the cases tell seven subtly wrong kernels from a right one - each perturbation, a small
wrapper around the references, changes at least one expected block of the slice."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import (align_parts_ref as apr, align_parts_two_bins_ref as apf, align_rates_ref as arr, align_ref as ar,
                   align_span_ref as asr, align_topk_ref as atr, align_two_bins_ref as atb, align_wide_ref as awr,
                   gap_candidates_rates_ref as gcrr, gap_candidates_ref as gcr, near_fuzz_cases as nf)
from tests.test_near_fuzz_gpu import CASES, SEEDS, reached


@pytest.fixture(scope="module")
def baseline():
    """-> {seed: (counters, {(case, step): expected blocks})}: the generator and the references as they stand, once"""
    out = {}
    for seed in SEEDS:
        stats = nf.new_stats()
        out[seed] = stats, {(ci, si): exp for ci, si, _, exp in nf.walk(seed, CASES, stats=stats)}
    return out


def test_the_same_seed_gives_the_same_cases():
    for seed in SEEDS:
        a = [nf.case_digest(c) for c in nf.cases(seed, CASES)]
        b = [nf.case_digest(c) for c in nf.cases(seed, CASES)]
        assert a == b and len(set(a)) == CASES
        assert a[:5] == [nf.case_digest(c) for c in nf.cases(seed, 5)]         # a shorter run is a prefix
    assert nf.case_digest(next(nf.cases(SEEDS[0], 1))) != nf.case_digest(next(nf.cases(SEEDS[1], 1)))


def test_every_drawn_parameter_is_inside_the_contract():
    seen = {"widest": 0, "zero": 0, "one": 0, "multi": 0, "multi_edge": 0}
    for seed in SEEDS:
        for case in nf.cases(seed, CASES):
            nf.check_case(case)
            seen[case["b_kind"]] += 1
            B = case["B"]
            assert 0 <= B <= awr.MAX_B and awr.n_bins(case["eps"], nf.Expect(case).mo) == B
            assert 2 * awr.n_bins(case["eps"], nf.bounded_offset(case)) + 1 <= ar.MAX_BINS
            if case["b_kind"] == "multi_edge":
                assert (2 * B + 1) % nf.WINDOW in (1, nf.WINDOW - 1)
            assert 1 <= len(case["rates"]) <= arr.MAX_RATES and all(0.0 < r < math.inf for r in case["rates"])
            assert len(case["uploads"]) in (1, 2, 5, 17)
    assert all(seen.values()), seen
    # the check itself refuses what the library refuses
    case = next(nf.cases(SEEDS[0], 1))
    for bad in (dict(form="span", k=16, min_votes=1, min_score=0, contain=True, local=True, two_bins=False, exclude_ids=None),
                dict(form="topk", k=65, min_votes=1, min_score=0, contain=False, local=False, two_bins=False, exclude_ids=None),
                dict(form="candidates", c=16, cap=5, min_count=1, exclude_ids=None)):
        with pytest.raises(ValueError):
            nf.check_case(dict(case, steps=[dict(op="gap", gap_eps=0.02), dict(op="call", **bad)]))


def test_the_references_alone_reach_every_mechanism(baseline):
    totals = {}
    for seed in SEEDS:
        nf.add_stats(totals, baseline[seed][0])
    print(totals)
    assert totals["cases"] == CASES * len(SEEDS) and not reached(totals), (reached(totals), totals)


def test_vectorised_references_agree_with_the_double_loops_on_tiny_cases():
    checked = 0
    for case in nf.cases(SEEDS[0], CASES):
        rows = [(v, k.tolist()) for v, k in case["rows"]]
        if sum(len(k) for _, k in rows) > 150:
            continue
        ex = nf.Expect(case)
        eps, mo, rho = case["eps"], ex.mo, case["rates"][-1]
        for u in case["uploads"]:
            q = u.tolist()
            if len(q) > 60:
                continue
            assert awr.brute_force(rows, q, eps, mo) == [tuple(r) for r in awr.align_wide_ref(rows, q, eps, mo).tolist()]
            assert atr.brute_force(rows, q, eps, ex.mo_b) == [tuple(r[:4]) for r in ar.align_ref(rows, q, eps, ex.mo_b).tolist()]
            two = atb.align_two_bins_ref(rows, q, eps, mo, (rho,))
            assert atb.brute_force(rows, q, eps, mo, rho) == [tuple(int(x) for x in r[[0, 1, 2, 3, 5, 6, 7]]) for r in two]
            for _, keys in rows[:4]:
                assert apf.double_loop(keys, q, eps, mo, rho, 1, 3) == apf.row_parts(keys, q, eps, mo, [rho], 1, 3, apf.TWO_BINS)[3]
            checked += 1
        qs = [u.tolist() for u in case["uploads"] if u.size <= 40][:3]
        if qs:
            kw = dict(min_count=1, cap=4, exclude_ids=[rows[0][0]] * len(qs))
            assert (gcr.candidates_loops(rows, qs, case["gap_eps"], 4, **kw) == gcr.candidates(rows, qs, case["gap_eps"], 4, **kw)).all()
            assert (gcrr.candidates_rates_loops(rows, qs, case["gap_eps"], case["rates"][:2], 4, **kw) ==
                    gcrr.candidates_rates(rows, qs, case["gap_eps"], case["rates"][:2], 4, **kw)).all()
    assert checked >= 15, checked


# ------------------------------------------------------------------------------------------ the perturbed references
def recip(rows, q, eps, mo):
    """(a) (c - x) * (1 / eps) instead of the division"""
    return ar.align_ref(rows, q, eps, mo, reciprocal=True)


def fused_bins(keys, s, eps, B, rho, fuse=True):
    """The bins of every pair with c - x * rho rounded ONCE (a fused multiply-subtract).  The fused difference is within
    an ulp of the contract's, so a bin can only move where the quotient lies next to an integer: those pairs alone are
    recomputed, with fractions for the one rounding."""
    c, b, _ = atb.bins_of(keys, s, eps, B, rho)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (c[:, None] - (s * np.float64(rho))[None, :]) / eps + 0.5
        near = np.isfinite(y) & (np.abs(y) < 2.0 ** 31) & (np.abs(y - np.round(y)) < 1e-6)
    for i, j in np.argwhere(near):
        d = float(Fraction(float(c[i])) - Fraction(float(s[j])) * Fraction(float(rho))) if fuse else \
            float(c[i]) - float(np.float64(s[j]) * np.float64(rho))
        b[i, j] = math.floor(d / eps + 0.5)
    with np.errstate(invalid="ignore"):
        return c, b, (b >= -B) & (b <= B)


def rates_by_rows(rows, query, eps, mo, rates, bins):
    """tests/align_rates_ref.align_rates_ref's answer from per-row bin matrices and align_parts_ref.best_bin"""
    B, s = awr.n_bins(eps, mo), asr.sorted_query(query)
    out = np.zeros((len(rows), 5), dtype=np.int64)
    for i, (vid, keys) in enumerate(rows):
        out[i, :2] = (int(vid), ar.row_set(keys).size)
        if out[i, 1] == 0 or s.size == 0:
            continue
        for ri, rho in enumerate(rates):
            _, b, ok = bins(keys, s, eps, B, rho)
            bn, v = apr.best_bin(b, ok, B)
            if v > out[i, 3]:                                   # strictly more: a tie keeps the smaller index
                out[i, 2:] = (bn, v, ri)
    return out


def rates_fused(rows, query, eps, mo, rates):
    """(b) the product x * rho fused into the subtraction"""
    return rates_by_rows(rows, query, eps, mo, rates, fused_bins)


def wide_plus_b(rows, query, eps, mo):
    """(c) the tie between +b and -b goes to +b"""
    a = awr.align_wide_ref(rows, query, eps, mo).copy()
    for i, (_, keys) in enumerate(rows):
        b = int(a[i, 2])
        if a[i, 3] > 0 and b < 0 and asr.pairs_of(keys, query, eps, -b, 1.0)[1].size == a[i, 3]:
            a[i, 2] = -b
    return a


def rates_later_on_tie(rows, query, eps, mo, rates):
    """(d) equal votes at two rates: the LARGER index - the reference over the reversed list, the index turned back"""
    a = arr.align_rates_ref(rows, query, eps, mo, list(rates)[::-1]).copy()
    voted = a[:, 3] > 0
    a[voted, 4] = len(rates) - 1 - a[voted, 4]
    a[~voted, 4] = 0
    return a


def two_bins_window_edge(rows, query, eps, mo, rates=(1.0,)):
    """(e) beyond one window of the walk, the window count loses its upper bin where the lower bin is the last slot of
    a 1,024-bin window counted from -B (columns 0..4 only: the wide and rates forms)"""
    B, s = awr.n_bins(eps, mo), asr.sorted_query(query)
    out = np.zeros((len(rows), 8), dtype=np.int64)
    for i, (vid, keys) in enumerate(rows):
        out[i, :2] = (int(vid), ar.row_set(keys).size)
        if out[i, 1] == 0 or s.size == 0:
            continue
        for ri, rho in enumerate(rates):
            _, b, ok = atb.bins_of(keys, s, eps, B, rho)
            if not ok.any():
                continue
            u, h = np.unique(b[ok].astype(np.int64), return_counts=True)
            count = dict(zip(u.tolist(), h.tolist()))
            up = np.array([count.get(x + 1, 0) for x in u.tolist()])
            if B > nf.ONE_WINDOW_B:
                up[(u + B) % nf.WINDOW == nf.WINDOW - 1] = 0
            J = h + up
            first = np.lexsort((u, np.abs(u), -h, -J))[0]
            if J[first] > out[i, 3]:
                out[i, 2:5] = (u[first], J[first], ri)
    return out


def parts_keep_votes(ref):
    """(f) the walk does not take the first part's votes out: every later part finds part 0 again"""
    def parts(rows, queries, ids, eps, mo, rates, **kw):
        out = ref(rows, queries, ids, eps, mo, rates, **kw).copy()
        found = out[:, :, 0, 3] >= 1
        out[:, :, 2:][found] = out[:, :, 1:2][found]
        out[:, :, 0, 3][found] = kw["max_parts"]
        return out
    return parts


def candidates_unsorted(rows, queries, gap_eps, c, **kw):
    """(g) the gaps of the upload as it came, not sorted"""
    keep = gcr.query_values
    gcr.query_values = lambda ts: (lambda a: a[~np.isnan(a)] + 0.0)(np.asarray(ts, dtype=np.float64).reshape(-1))
    try:
        return gcr.candidates(rows, queries, gap_eps, c, **kw)
    finally:
        gcr.query_values = keep


PERTURBED = {
    "a_reciprocal": (dict(align=recip), ("topk",)),
    "b_fused_product": (dict(rates=rates_fused), ("rates",)),
    "c_tie_to_plus_b": (dict(wide=wide_plus_b), ("wide",)),
    "d_rate_tie_to_the_larger_index": (dict(rates=rates_later_on_tie), ("rates",)),
    "e_two_bin_window_edge": (dict(two_bins=two_bins_window_edge), ("wide", "rates")),
    "f_parts_keep_votes": (dict(parts=parts_keep_votes(apr.align_parts_ref), parts_flags=parts_keep_votes(apf.align_parts_flags_ref)),
                           ("parts", "parts_flags")),
    "g_unsorted_gap_codes": (dict(candidates=candidates_unsorted), ("candidates",)),
}


def test_the_wrappers_without_their_perturbation_are_the_references():
    """rates_by_rows with the contract's bins, and with the un-fused difference recomputed next to the integers, is
    align_rates_ref; two_bins_window_edge inside one window is align_two_bins_ref's first five columns"""
    n = 0
    for case in nf.cases(SEEDS[1], 12):
        ex = nf.Expect(case)
        rows = [(v, k.tolist()) for v, k in case["rows"]][:20]
        for u in case["uploads"][:2]:
            want = arr.align_rates_ref(rows, u.tolist(), case["eps"], ex.mo, case["rates"])
            assert (rates_by_rows(rows, u.tolist(), case["eps"], ex.mo, case["rates"], atb.bins_of) == want).all()
            unfused = lambda *a: fused_bins(*a, fuse=False)                     # noqa: E731
            assert (rates_by_rows(rows, u.tolist(), case["eps"], ex.mo, case["rates"], unfused) == want).all()
            if case["B"] <= nf.ONE_WINDOW_B:
                two = atb.align_two_bins_ref(rows, u.tolist(), case["eps"], ex.mo, case["rates"])
                assert (two_bins_window_edge(rows, u.tolist(), case["eps"], ex.mo, case["rates"])[:, :5] == two[:, :5]).all()
            n += 1
    assert n >= 12


@pytest.mark.parametrize("name", sorted(PERTURBED))
def test_the_cases_tell_a_subtly_wrong_kernel_from_a_right_one(baseline, name):
    swapped, forms = PERTURBED[name]
    refs = nf.refs_with(**swapped)
    caught = None
    for seed in SEEDS:
        for ci, si, p, exp in nf.walk(seed, CASES, refs=refs, only=forms):
            if name.startswith("e_") and (not p["two_bins"]):
                continue
            want = baseline[seed][1][ci, si]["block"]
            if not np.array_equal(exp["block"], want):
                caught = dict(seed=seed, case=ci, call=si, form=nf.form_name(p))
                break
        if caught:
            break
    print(name, caught)
    assert caught, f"no case of the slice tells {name} from the references"
