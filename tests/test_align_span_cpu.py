"""tvz_align_span_topk without a GPU: the reference of tests/align_span_ref.py against exact rational arithmetic and
against the rates reference, the copy that is partial on both sides under the three scores, the workspace formula of
include/tvz.h, the binding's table against the header, the refusals that come before anything touches a device, the
inspector's argument checks, and the gfx950 code objects read with the metadata readers of tests/test_codeobj_cpu.py."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

from tests import align_rates_ref as arr, align_ref as ar, align_span_ref as asr, align_topk_ref as atr, align_wide_ref as awr
from tests.test_align_rates_cpu import _exact_bin, _prototype
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)
from tvidz_amd import _lib, build as tbuild, corpus as tc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tvz.h")
EXPORTS = ("tvz_align_span_topk_workspace_bytes", "tvz_align_span_topk", "tvz_align_span_topk_merge",
           "tvz_align_span_topk_shards")
NEW = ("22ts_aligns_sweep_kernelE", "23ts_aligns_reduce_kernelE", "22ts_aligns_merge_kernelE")
OLD = ("20ts_align_topk_kernelE", "27ts_align_topk_reduce_kernelE", "22ts_alignw_sweep_kernelE",
       "23ts_alignw_reduce_kernelE", "26ts_align_topk_merge_kernelE", "22ts_alignw_merge_kernelE", "15ts_align_kernelE",
       "22ts_alignr_sweep_kernelE", "23ts_alignr_reduce_kernelE", "22ts_alignr_merge_kernelE")
EPS = 1 / 30
ONE = 1 << 20


# ------------------------------------------------------------------------------------------------ the reference
def _table():
    """rows of 0..130 keys in two hours; row 3 (40 keys) is the one the queries are made from"""
    rng = np.random.default_rng(1313)
    rows = [(100 + i, np.sort(rng.uniform(0.0, 7200.0, size=n)).tolist())
            for i, n in enumerate([0, 1, 9, 40, 36, 65, 130, 17])]
    rows[2] = (rows[2][0], rows[2][1] + [float("inf"), -float("inf")])
    return rows


def _queries(rows):
    base = np.asarray(rows[3][1])
    return [((base - 12.3) / 0.96).tolist(), (base[8:30] - 12.3).tolist() + [float("nan"), 50.0, 50.0],
            (np.asarray(rows[6][1])[::3] + 1000.0).tolist()]


def test_reference_spans_equal_exact_rational_arithmetic():
    rows = _table()
    rates = (1.0, 0.96)
    checked = 0
    for q in _queries(rows):
        a = asr.align_span_ref(rows, q, EPS, awr.MAX_B * EPS, rates)               # (asserts |P| == votes per row)
        assert (a[:, :5] == arr.align_rates_ref(rows, q, EPS, awr.MAX_B * EPS, rates)).all()
        s = sorted(x for x in q if x == x)
        for (vid, keys), row in zip(rows, a.tolist()):
            if row[3] == 0:
                assert row[5:] == [0, 0, 0]
                continue
            rho, best = rates[row[4]], row[2]
            keys = sorted(set(c for c in keys if math.isfinite(c)))
            pairs = [(c, t) for c in keys for t, x in enumerate(s) if math.isfinite(x) and _exact_bin(c, x, rho, EPS) == best]
            assert len(pairs) == row[3], (vid, row)
            ts, cs = [t for _, t in pairs], [c for c, _ in pairs]
            nr = sum(1 for c in keys if min(cs) <= c <= max(cs))
            assert row[5:] == [min(ts), max(ts), nr], (vid, row)
            # the three scores in fractions
            nv, rl, votes, nq = len(s), row[1], row[3], max(ts) - min(ts) + 1
            v = min(votes, nv, rl)
            assert asr.score_of(row, nv) == (v, math.floor(F(v << 20, nv + rl - v)))
            assert asr.score_of(row, nv, contain=True) == (v, math.floor(F(v << 20, min(nv, rl))))
            vl = min(votes, nq, nr)
            assert asr.score_of(row, nv, local=True) == (vl, math.floor(F(vl << 20, nq + nr - vl)))
            assert tc.align_local_score(votes, nq, nr) == asr.score_of(row, nv, local=True)[1]
            checked += 1
    assert checked >= 12


def test_reference_without_local_is_the_rates_reference():
    rows = _table()
    queries = _queries(rows)
    for rates in ((1.0,), (1.0, 0.96)):
        for contain in (False, True):
            rated = arr.topk_rates_ref(rows, queries, EPS, awr.MAX_B * EPS, rates, 16, contain=contain)
            span = asr.topk_span_ref(rows, queries, EPS, awr.MAX_B * EPS, rates, 16, contain=contain)
            assert (span[:, :, :5] == rated).all()
    # the order's last three fields, and the Python key
    rows8 = np.array([[7, 4, 3, 4, 0, 2, 9, 5], [7, 4, 3, 4, 0, 2, 8, 6], [7, 4, 3, 4, 0, 1, 9, 9], [7, 4, 3, 4, 0, 2, 8, 5]])
    hits = [h[1] for h in asr.hits_of(rows8, 40)]
    assert [h[5:] for h in hits] == [(1, 9, 9), (2, 8, 5), (2, 8, 6), (2, 9, 5)]
    assert hits == sorted((tuple(r) for r in rows8.tolist()), key=lambda r: tc.align_span_order_key(r, 40))
    local = [h[1] for h in asr.hits_of(rows8, 40, local=True)]
    assert local == sorted((tuple(r) for r in rows8.tolist()), key=lambda r: tc.align_span_order_key(r, 40, local=True))
    assert local[0][5:] == (2, 8, 5)                                               # nq 7, nr 5: the best local score
    with pytest.raises(ValueError):
        tc.align_span_order_key(rows8[0], 40, contain=True, local=True)


def test_the_compilation_case_is_found_by_the_local_score_alone():
    film, upload, clip, shift = asr.compilation_case()
    assert len(film) == len(upload) == 400 and len(clip) == 20
    rows = [(1, film)]
    (row,) = asr.align_span_ref(rows, upload, EPS, awr.MAX_B * EPS, (1.0,)).tolist()
    s = sorted(upload)
    assert row[:5] == [1, 400, math.floor(shift / EPS + 0.5), 20, 0]
    assert [s[row[5]] + shift, s[row[6]] + shift] == pytest.approx([clip[0], clip[-1]], abs=EPS) and row[7] == 20
    assert row[6] - row[5] + 1 == 20
    assert asr.score_of(row, 400)[1] == (20 << 20) // 780 < ONE // 10
    assert asr.score_of(row, 400, contain=True)[1] == (20 << 20) // 400 < ONE // 10
    assert asr.score_of(row, 400, local=True) == (20, ONE)
    for kw, found in ((dict(), False), (dict(contain=True), False), (dict(local=True), True)):
        block = asr.topk_span_ref(rows, [upload], EPS, awr.MAX_B * EPS, (1.0,), 4, min_votes=8, min_score=ONE // 2, **kw)
        assert (block[0, 4, 1] == 1) == found and (block[0, 0, 0] == 1) == found, kw


def test_one_vote_scores_one_under_local():
    rows = [(1, [10.0, 500.0, 900.0])]
    (row,) = asr.align_span_ref(rows, [3.0, 77.0], 0.5, 100.0, (1.0,)).tolist()
    assert row[3] == 1 and row[6] == row[5] and row[7] == 1 and asr.score_of(row, 2, local=True) == (1, ONE)


# ------------------------------------------------------------------------------------------------- the C ABI
def test_the_four_exports_are_in_the_library_and_match_the_header():
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    defined = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", tbuild.SO], text=True).splitlines()
               if ln.strip()}
    assert set(EXPORTS) <= defined, sorted(set(EXPORTS) - defined)
    text = open(HEADER).read()
    for name in EXPORTS:
        assert _lib.SIGNATURES[name] == _prototype(text, name), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_span_", "_rates_")], name
    assert re.search(r"^#define TVZ_ALIGN_LOCAL 2u\b", text, re.M) and tc.ALIGN_LOCAL == asr.LOCAL == 2
    assert _lib.VERSION == 404 and _lib.load().tvz_version() == 404                # new exports only


def test_the_workspace_is_the_rates_formula_at_32_bytes_per_kept_hit():
    text = open(HEADER).read()
    assert re.search(r"max\(6080, 95 Q\) x k x 32", text)                          # the formula the header states
    lib = _lib.load()

    def up(n):
        return (n + 255) & ~255

    for Q, L, keys, k in ((1, 200, 0, 16), (16, 4095, 0, 64), (70, 40, 1234, 1), (1, 0, 0, 1), (64, 40, 0, 16)):
        span = tc.align_span_topk_workspace_bytes(Q, L, keys, k)
        rated = tc.align_rates_topk_workspace_bytes(Q, L, keys, k)
        assert span == lib.tvz_align_span_topk_workspace_bytes(Q, L, keys, k)
        lists = max(6080, 95 * Q) * k
        assert span - rated == 2 * up(lists * 4), (Q, L, keys, k)                  # the index pairs and the key counts
        total = keys if keys > 0 else Q * L
        raw = lib.tvz_match_tol_workspace_bytes(Q, L, max(total, L)) + 4 * Q + lists * 32
        assert raw <= span < raw + 8 * 256, (Q, L, keys, k, span, raw)
    assert lib.tvz_align_span_topk_workspace_bytes(1, 10, 0, 0) == 0 == lib.tvz_align_span_topk_workspace_bytes(-1, 10, 0, 1)


def test_refusals_that_need_no_device():
    """The rate list and the flags are refused before the handle is looked at; the other limits are checked with a
    NULL handle's refusal behind them, so the order shows in the message."""
    lib = _lib.load()
    good = (C.c_double * 2)(1.0, 0.96)

    def call(rates=good, n=2, flags=0, k=16, L=4, min_votes=1):
        rc = lib.tvz_align_span_topk(None, None, None, 1, L, 1 / 30, 1.0, rates, n, min_votes, 0, flags, None, k, None, None,
                                     0, None)
        rs = lib.tvz_align_span_topk_shards(None, 1, None, None, 1, L, 1 / 30, 1.0, rates, n, min_votes, 0, flags, None, k,
                                            None, None, None, None, 0, None)
        assert rc == rs, (rc, rs)
        return rc, lib.tvz_last_error()

    rc, msg = call(flags=tc.ALIGN_CONTAIN | tc.ALIGN_LOCAL)
    assert rc == ar.ERR_INVALID and b"TVZ_ALIGN_CONTAIN and TVZ_ALIGN_LOCAL" in msg
    rc, msg = call(flags=4)
    assert rc == ar.ERR_INVALID and b"unknown flag bits 0x4" in msg
    assert call(flags=0x80000000)[0] == ar.ERR_INVALID
    assert call(rates=good, n=0)[0] == ar.ERR_UNSUPPORTED and call(rates=(C.c_double * 9)(*[1.0] * 9), n=9)[0] == ar.ERR_UNSUPPORTED
    assert b"TVZ_ALIGN_MAX_RATES" in lib.tvz_last_error()
    assert call(rates=None, n=1)[0] == ar.ERR_INVALID
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        rc, msg = call(rates=(C.c_double * 2)(1.0, bad))
        assert rc == ar.ERR_INVALID and b"rate 1" in msg, (bad, msg)
    # a bad rate list is named before bad flags, and both before the handle
    rc, msg = call(rates=(C.c_double * 2)(1.0, -1.0), flags=3)
    assert rc == ar.ERR_INVALID and b"rate 1" in msg
    # the limits that need no device either
    assert call(k=0)[0] == ar.ERR_UNSUPPORTED and call(k=65)[0] == ar.ERR_UNSUPPORTED
    rc, msg = call(L=4096)
    assert rc == ar.ERR_UNSUPPORTED and b"max_query_len 4096" in msg
    rc, msg = call(min_votes=0)
    assert rc == ar.ERR_INVALID and b"min_votes 0" in msg
    for flags in (0, tc.ALIGN_CONTAIN, tc.ALIGN_LOCAL):                            # good ones: refused for the handle
        rc, msg = call(flags=flags)
        assert rc == ar.ERR_INVALID and b"rate" not in msg and b"flag" not in msg, msg
    # the merge refuses its limits and flags without a device too
    for n_lists, k, flags, want in ((0, 4, 0, ar.ERR_UNSUPPORTED), (17, 4, 0, ar.ERR_UNSUPPORTED), (3, 0, 0, ar.ERR_UNSUPPORTED),
                                    (3, 65, 0, ar.ERR_UNSUPPORTED), (3, 4, 3, ar.ERR_INVALID), (3, 4, 4, ar.ERR_INVALID)):
        assert lib.tvz_align_span_topk_merge(None, n_lists, 1, k, flags, None, None, None, None, None) == want, (n_lists, k, flags)
    # the existing calls keep refusing bit 2 (their flag check follows the handle's: a NULL handle says so first, and the
    # merges, which take no handle, say it here)
    for name in ("tvz_align_wide_topk_merge", "tvz_align_rates_topk_merge"):
        assert getattr(lib, name)(None, 3, 1, 4, 2, None, None, None, None, None) == ar.ERR_INVALID
        assert b"unknown flag bits 0x2" in lib.tvz_last_error(), name
    assert lib.tvz_align_rates_topk(None, None, None, 1, 4, 1 / 30, 1.0, good, 2, 1, 0, 2, None, 16, None, None, 0,
                                    None) == ar.ERR_INVALID
    assert lib.tvz_align_wide_topk(None, None, None, 1, 4, 1 / 30, 1.0, 1, 0, 2, None, 16, None, None, 0, None) == ar.ERR_INVALID


# ---------------------------------------------------------------------------------------------- the inspector
class _SpanCorpus:
    """answers with one hit of 20 votes over query indexes 3..22 and 20 row keys, or refuses"""

    def __init__(self, refuse=False):
        self.refuse, self.calls = refuse, []

    def align(self, timestamps, eps=0.1, max_offset=60.0):
        return np.array([[42, 400, -30, 20, 0]], dtype=np.int32)

    def align_topk(self, queries, **kw):
        return np.zeros((len(queries), kw["k"], 4), dtype=np.int32), np.zeros(len(queries), dtype=np.int32)

    align_wide_topk = align_topk

    def align_rates_topk(self, queries, **kw):
        raise AssertionError("the span call was asked for")

    def align_span_topk(self, queries, **kw):
        self.calls.append(kw)
        rows = np.zeros((len(queries), kw["k"], 8), dtype=np.int32)
        rows[:, :, 0] = -1
        rows[:, 0] = (42, 400, -30, 20, len(kw["rates"]) - 1, 3, 22, 20)
        totals = np.full(len(queries), atr.REFUSED if self.refuse else 1, dtype=np.int64)
        return rows, totals


class _Store:
    def __init__(self, corpus):
        self.corpus = corpus

    def get_video_by_id(self, vid):
        return None


def test_inspector_span_arguments():
    from tvidz_amd import inspector as insp

    ok = dict(device="cuda:0", near_duplicates=True, near_top_k=8, near_any_offset=True)
    new = lambda corpus=None, **kw: insp.Inspector(_Store(corpus or _SpanCorpus()), **kw)       # noqa: E731
    with pytest.raises(ValueError, match="near_any_offset"):
        new(device="cuda:0", near_duplicates=True, near_top_k=8, near_score="local", near_min_votes=8)
    with pytest.raises(ValueError, match="near_min_votes >= 2"):
        new(near_score="local", near_min_votes=1, **ok)
    with pytest.raises(ValueError, match="near_min_votes >= 2"):
        new(near_score="local", **ok)
    with pytest.raises(ValueError, match="near_top_k"):
        new(device="cuda:0", near_duplicates=True, near_spans=True)
    with pytest.raises(ValueError, match="near_score"):
        new(near_score="span", **ok)
    corpus = _SpanCorpus()
    wide_only = type("WideOnly", (), {"align": corpus.align, "align_topk": corpus.align_topk,
                                      "align_wide_topk": corpus.align_topk})
    with pytest.raises(RuntimeError, match="align_span_topk"):
        new(wide_only(), near_spans=True, **ok)
    # neither option: nothing changes
    ins = new(**ok)
    assert ins.near_spans is False and ins.near_score == "jaccard"
    # near_spans with the Jaccard: the span fields, no rate, rates (1.0,)
    cuts = [100.0 - i for i in range(40)] + [float("nan")]                        # unsorted, one NaN
    s = sorted(x for x in cuts if x == x)
    ins = new(corpus, near_spans=True, near_jaccard=0.01, **ok)
    (near,) = ins._near(7, cuts)
    assert corpus.calls[-1]["rates"] == (1.0,) and corpus.calls[-1]["local"] is False and corpus.calls[-1]["exclude_ids"] == [7]
    shift = -30 * ins.near_eps
    assert near["upload_span"] == [s[3], s[22]] and near["stored_span"] == [s[3] + shift, s[22] + shift]
    assert "rate" not in near and "local" not in near and near["video_id"] == 42
    # local with rates: the score inside the span, the rate in the stored span
    ins = new(corpus, near_score="local", near_min_votes=8, near_rates=(1.0, 0.96), near_jaccard=0.9, **ok)
    (near,) = ins._near(7, cuts)
    assert corpus.calls[-1]["rates"] == (1.0, 0.96) and corpus.calls[-1]["local"] is True and corpus.calls[-1]["min_votes"] == 8
    assert near["local"] == 1.0 and near["rate"] == 0.96 and near["jaccard"] == round(20 / (41 + 400 - 20), 4)
    assert near["stored_span"] == [0.96 * s[3] + shift, 0.96 * s[22] + shift]
    ins = new(corpus, near_score="local", near_min_votes=21, near_jaccard=0.9, **ok)
    assert ins._near(7, cuts) == []                                                # v = 20 below near_min_votes
    # a refused query falls back to the walk: no span fields, and a "local" report has no entries
    refusing = _SpanCorpus(refuse=True)
    ins = new(refusing, near_spans=True, near_jaccard=0.01, **ok)
    (near,) = ins._near(7, cuts)
    assert "upload_span" not in near and "stored_span" not in near and "rate" not in near
    ins = new(refusing, near_score="local", near_min_votes=2, near_jaccard=0.01, **ok)
    assert ins._near(7, cuts) == []


# -------------------------------------------------------------------------------------------- the code objects
def test_new_kernels_exist_once_and_the_existing_ones_still_do(kernels):  # noqa: F811
    for name in NEW + OLD:
        assert len([n for n in kernels if name in n]) == 1, (name, sorted(n for n in kernels if "align" in n))


def test_new_kernels_have_no_scratch_and_no_spills(kernels):  # noqa: F811
    for name in NEW:
        (k,) = [k for n, k in kernels.items() if name in n]
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (name, k)


def test_the_span_sweeps_lds(kernels):  # noqa: F811
    (k,) = [k for n, k in kernels.items() if NEW[0] in n]
    # static: the block-end merge's 4 x 64 kept hits of 32 B + the hit counter; with the largest dynamic part (a query
    # of 4,095 values, one window of 4,096 bins) still inside a workgroup's 160 KiB
    assert 4 * 64 * 32 <= k[".group_segment_fixed_size"] <= 4 * 64 * 32 + 64, k[".group_segment_fixed_size"]
    assert k[".group_segment_fixed_size"] + 4095 * 8 + 4 * (4096 * 6 + 4) <= 160 * 1024
    assert k[".max_flat_workgroup_size"] == 256
    (k,) = [k for n, k in kernels.items() if NEW[1] in n]
    assert 16 * 64 * 32 <= k[".group_segment_fixed_size"] <= 16 * 64 * 32 + 64 and k[".max_flat_workgroup_size"] == 1024
    (k,) = [k for n, k in kernels.items() if NEW[2] in n]
    assert k[".group_segment_fixed_size"] == 0 and k[".max_flat_workgroup_size"] == 256
