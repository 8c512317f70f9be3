"""tvz_align_rates_topk without a GPU: the reference of tests/align_rates_ref.py against exact rational arithmetic and
against the wide reference, the case that tells the contract's two roundings from a fused multiply-subtract, the
workspace formula of include/tvz.h, the binding's table against the header, the rate list's refusals (they come before
anything touches a device), the inspector's argument checks, and the gfx950 code objects read with the metadata
readers of tests/test_codeobj_cpu.py."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

from tests import align_rates_ref as arr, align_ref as ar, align_topk_ref as atr, align_wide_ref as awr
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)
from tvidz_amd import _lib, build as tbuild, corpus as tc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tvz.h")
EXPORTS = ("tvz_align_rates_topk_workspace_bytes", "tvz_align_rates_topk", "tvz_align_rates_topk_merge",
           "tvz_align_rates_topk_shards")
RATES8 = (0.96, 1.0, 25 / 24, 1001 / 1000, 1000 / 1001, 1.25, 0.8, 2.0)
NEW = ("22ts_alignr_sweep_kernelE", "23ts_alignr_reduce_kernelE", "22ts_alignr_merge_kernelE")
OLD = ("20ts_align_topk_kernelE", "27ts_align_topk_reduce_kernelE", "22ts_alignw_sweep_kernelE",
       "23ts_alignw_reduce_kernelE", "26ts_align_topk_merge_kernelE", "22ts_alignw_merge_kernelE", "15ts_align_kernelE")


# ------------------------------------------------------------------------------------------------ the reference
def _exact_bin(c, x, rho, eps):
    """The contract's bin in rational arithmetic with its roundings made explicit: Fraction -> float rounds
    correctly, so every step is the IEEE operation."""
    p = float(F(x) * F(rho))                            # fl(x * rho)
    d = float(F(c) - F(p))                              # fl(c - p)
    t = float(F(d) / F(eps))                            # fl(d / eps)
    return math.floor(float(F(t) + F(1, 2)))            # floor(fl(t + 0.5))


def test_reference_votes_equal_exact_rational_arithmetic():
    rng = np.random.default_rng(5)
    eps = 1 / 30
    pairs = 0
    for rho in RATES8:
        xs = rng.uniform(0.0, 7200.0, size=6)
        for x in xs.tolist():
            # keys around rho * x + shift, some of them a hair from a bin's edge
            for shift_bins in (-70000.5, -3.5, 0.0, 0.5, 41.5, 90001.0):
                c = float(x * rho + shift_bins * eps)
                got = arr.align_rates_ref([(1, [c])], [x], eps, awr.MAX_B * eps, (rho,))
                assert got[0].tolist() == [1, 1, _exact_bin(c, x, rho, eps), 1, 0], (c, x, rho)
                pairs += 1
    assert pairs >= 36


def test_reference_at_rate_one_is_the_wide_reference():
    for name, rows, calls in ar.edge_cases():
        if name in ("grid_stride", "long_rows"):
            continue                                                               # (large: nothing more to see)
        for q, eps, mo in calls[:4]:
            for contain in (False, True):
                wide = awr.topk_wide_ref(rows, [list(q)], eps, mo, 16, contain=contain)
                rated = arr.topk_rates_ref(rows, [list(q)], eps, mo, (1.0,), 16, contain=contain)
                assert (rated[:, :, :4] == wide).all() and (rated[:, :, 4] == 0).all(), (name, eps, mo)


def test_reference_keeps_the_rate_with_most_votes_and_the_smaller_index_on_a_tie():
    eps = 1 / 64
    q = [100.0 + 3 * i for i in range(8)]
    row_a = [x * 0.5 + 10.0 for x in q]                                            # all 8 at rate 0.5
    row_b = [x + 20.0 for x in q]                                                  # all 8 at rate 1.0
    row_c = [q[0] + 5.0]                                                           # one key: one vote at every rate
    rows = [(1, row_a), (2, row_b), (3, row_c)]
    a = arr.align_rates_ref(rows, q, eps, awr.MAX_B * eps, (1.0, 0.5, 0.5))
    assert a[0].tolist() == [1, 8, 640, 8, 1]                                      # the repeated rate: its first index
    assert a[1].tolist() == [2, 8, 1280, 8, 0]
    assert a[2, 3] == 1 and a[2, 4] == 0                                           # a tie: the smaller index
    a = arr.align_rates_ref(rows, q, eps, awr.MAX_B * eps, (0.5, 1.0))
    assert a[0, 4] == 0 and a[1, 4] == 1 and a[2, 4] == 0
    # the order's sixth field: rows equal in five fields come out by the rate's index
    hits = arr.hits_of(np.array([[7, 4, 3, 4, 2], [7, 4, 3, 4, 0], [7, 4, 3, 4, 1]]), 4)
    assert [h[1][4] for h in hits] == [0, 1, 2]


def test_the_no_fma_case_discriminates():
    c, x, rho, eps, j = arr.no_fma_case()
    exact = F(x) * F(rho)
    p = x * rho
    assert F(p) != exact and F(p) < exact                                          # inexact, rounded down
    assert F(c) == F(p) + (F(j) - F(1, 2)) * F(eps)                                # c is exact
    # the contract: two roundings
    assert (c - p) / eps + 0.5 == float(j) and _exact_bin(c, x, rho, eps) == j
    assert arr.align_rates_ref([(1, [c])], [x], eps, 100.0, (rho,))[0].tolist() == [1, 1, j, 1, 0]
    # a fused multiply-subtract: c - x * rho rounded ONCE lands in another bin
    fused = float(F(c) - exact)
    assert math.floor(fused / eps + 0.5) == j - 1


# ------------------------------------------------------------------------------------------------- the C ABI
def _ctype(decl):
    decl = decl.strip()
    if "*" in decl:
        return C.c_void_p
    base = re.sub(r"\bconst\b", "", decl).split()[0]
    return {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "double": C.c_double,
            "size_t": C.c_size_t}[base]


def _prototype(text, name):
    m = re.search(r"^(\w+)\s+" + name + r"\(([^;]*?)\);", text, re.M | re.S)
    assert m, name
    return _ctype(m.group(1)), [_ctype(p) for p in m.group(2).split(",")]


def test_the_four_exports_are_in_the_library_and_match_the_header():
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    defined = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", tbuild.SO], text=True).splitlines()
               if ln.strip()}
    assert set(EXPORTS) <= defined, sorted(set(EXPORTS) - defined)
    text = open(HEADER).read()
    for name in EXPORTS:
        assert _lib.SIGNATURES[name] == _prototype(text, name), name
    # the wide forms with the host's rate list behind max_offset: one pointer and one int32 more
    for rated, wide in (("tvz_align_rates_topk", "tvz_align_wide_topk"),
                        ("tvz_align_rates_topk_shards", "tvz_align_wide_topk_shards")):
        r, w = _lib.SIGNATURES[rated][1], _lib.SIGNATURES[wide][1]
        at = max(i for i, t in enumerate(w) if t is C.c_double) + 1
        assert r == w[:at] + [C.c_void_p, C.c_int32] + w[at:], rated
    assert _lib.SIGNATURES["tvz_align_rates_topk_merge"] == _lib.SIGNATURES["tvz_align_wide_topk_merge"]
    assert re.search(r"^#define TVZ_ALIGN_MAX_RATES 8\b", text, re.M) and tc.ALIGN_MAX_RATES == arr.MAX_RATES == 8
    assert _lib.VERSION == 404 and _lib.load().tvz_version() == 404                # new exports only


def test_the_workspace_is_the_wide_formula_at_24_bytes_per_kept_hit():
    text = open(HEADER).read()
    assert re.search(r"max\(6080, 95 Q\) x k x 24", text)                          # the formula the header states
    lib = _lib.load()

    def up(n):
        return (n + 255) & ~255

    for Q, L, keys, k in ((1, 200, 0, 16), (16, 4095, 0, 64), (70, 40, 1234, 1), (1, 0, 0, 1), (64, 40, 0, 16)):
        rated = tc.align_rates_topk_workspace_bytes(Q, L, keys, k)
        wide = tc.align_wide_topk_workspace_bytes(Q, L, keys, k)
        assert rated == lib.tvz_align_rates_topk_workspace_bytes(Q, L, keys, k)
        lists = max(6080, 95 * Q) * k
        assert rated - wide == up(lists * 4), (Q, L, keys, k)                      # the fourth array: the rate indexes
        # the whole formula: the sorted queries + the totals + 24 bytes per kept hit + alignment (the base and each of
        # the five parts, below 256 B each)
        total = keys if keys > 0 else Q * L
        raw = lib.tvz_match_tol_workspace_bytes(Q, L, max(total, L)) + 4 * Q + lists * 24
        assert raw <= rated < raw + 6 * 256, (Q, L, keys, k, rated, raw)
    assert lib.tvz_align_rates_topk_workspace_bytes(1, 10, 0, 0) == 0 == lib.tvz_align_rates_topk_workspace_bytes(-1, 10, 0, 1)


def test_the_rate_list_is_refused_before_anything_else():
    """n_rates outside 1..8: unsupported; a NULL list or a rate that is NaN, infinite, zero or negative: invalid - said
    before the handle is looked at, so with or without a GPU."""
    lib = _lib.load()

    def call(rates, n=None):
        h = (C.c_double * max(len(rates), 1))(*rates) if rates is not None else None
        n = len(rates) if n is None else n
        rc = lib.tvz_align_rates_topk(None, None, None, 1, 4, 1 / 30, 1.0, h, n, 1, 0, 0, None, 16, None, None, 0, None)
        rs = lib.tvz_align_rates_topk_shards(None, 1, None, None, 1, 4, 1 / 30, 1.0, h, n, 1, 0, 0, None, 16, None, None,
                                             None, None, 0, None)
        assert rc == rs
        return rc, lib.tvz_last_error()

    assert call([], 0)[0] == ar.ERR_UNSUPPORTED and call([1.0] * 9)[0] == ar.ERR_UNSUPPORTED
    assert call([1.0], -1)[0] == ar.ERR_UNSUPPORTED
    assert b"TVZ_ALIGN_MAX_RATES" in call([1.0] * 9)[1]
    assert call(None, 1)[0] == ar.ERR_INVALID
    for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -0.0, -1.0):
        rc, msg = call([1.0, bad])
        assert rc == ar.ERR_INVALID and b"rate 1" in msg, (bad, msg)
    rc, msg = call([1.0, 0.96])                                                     # a good list: refused for the handle
    assert rc == ar.ERR_INVALID and b"rate" not in msg


# ---------------------------------------------------------------------------------------------- the inspector
class _WideOnlyCorpus:
    def align(self, timestamps, eps=0.1, max_offset=60.0):
        return np.zeros((0, 5), dtype=np.int32)

    def align_topk(self, queries, **kw):
        return np.zeros((len(queries), kw["k"], 4), dtype=np.int32), np.zeros(len(queries), dtype=np.int32)

    def align_wide_topk(self, queries, **kw):
        return self.align_topk(queries, **kw)


class _RatesCorpus(_WideOnlyCorpus):
    """answers with one hit at rate index 1, or refuses (a total below zero) when told to"""

    def __init__(self, refuse=False):
        self.refuse, self.calls = refuse, []

    def align_rates_topk(self, queries, **kw):
        self.calls.append(kw)
        rows = np.zeros((len(queries), kw["k"], 5), dtype=np.int32)
        rows[:, :, 0] = -1
        rows[:, 0] = (42, 4, -30, 4, 1)
        totals = np.full(len(queries), atr.REFUSED if self.refuse else 1, dtype=np.int64)
        return rows, totals


class _Store:
    def __init__(self, corpus):
        self.corpus = corpus

    def get_video_by_id(self, vid):
        return None


def test_inspector_near_rates_arguments():
    from tvidz_amd import inspector as insp

    ok = dict(device="cuda:0", near_duplicates=True, near_top_k=8, near_any_offset=True)
    for bad in ((), (1.0,) * 9, (1.0, 0.0), (-1.0,), (float("nan"),), (float("inf"),)):
        with pytest.raises(ValueError, match="near_rates"):
            insp.Inspector(_Store(_RatesCorpus()), near_rates=bad, **ok)
    with pytest.raises(ValueError, match="near_any_offset"):
        insp.Inspector(_Store(_RatesCorpus()), device="cuda:0", near_duplicates=True, near_top_k=8, near_rates=(1.0,))
    with pytest.raises(ValueError, match="near_top_k"):
        insp.Inspector(_Store(_RatesCorpus()), device="cuda:0", near_duplicates=True, near_rates=(1.0,))
    with pytest.raises(RuntimeError, match="align_rates_topk"):
        insp.Inspector(_Store(_WideOnlyCorpus()), near_rates=(1.0, 0.96), **ok)
    # the default changes nothing; a list is kept as floats in the caller's order
    assert insp.Inspector(_Store(_WideOnlyCorpus()), **ok).near_rates is None
    corpus = _RatesCorpus()
    ins = insp.Inspector(_Store(corpus), near_rates=[1, 0.96], near_jaccard=0.5, **ok)
    assert ins.near_rates == (1.0, 0.96)
    # the report: the fifth column is the rate's index, and the entry says the rate
    (near,) = ins._near(7, [1.0, 2.0, 3.0, 4.0])
    assert near["video_id"] == 42 and near["rate"] == 0.96 and near["jaccard"] == 1.0
    assert near["shift_seconds"] == -30 * ins.near_eps
    assert corpus.calls[0]["rates"] == (1.0, 0.96) and corpus.calls[0]["exclude_ids"] == [7]
    assert corpus.calls[0]["max_offset"] is None and corpus.calls[0]["k"] == 8
    # a refused query falls back to the walk at rate 1: no entry has a rate
    ins = insp.Inspector(_Store(_RatesCorpus(refuse=True)), near_rates=(1.0, 0.96), **ok)
    rows, rated = ins._near_rows(7, [1.0, 2.0, 3.0, 4.0])
    assert not rated and len(rows) == 0


# -------------------------------------------------------------------------------------------- the code objects
def test_new_kernels_exist_once_and_the_existing_ones_still_do(kernels):  # noqa: F811
    for name in NEW + OLD:
        assert len([n for n in kernels if name in n]) == 1, (name, sorted(n for n in kernels if "align" in n))


def test_new_kernels_have_no_scratch_and_no_spills(kernels):  # noqa: F811
    for name in NEW:
        (k,) = [k for n, k in kernels.items() if name in n]
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (name, k)


def test_the_rate_sweeps_registers_and_lds(kernels):  # noqa: F811
    (k,) = [k for n, k in kernels.items() if NEW[0] in n]
    # reported: 78 VGPRs -> six waves per SIMD, where the wide sweep's 70 give seven; the LDS sets the occupancy of every
    # call of more than ~600 bins (tests/test_align_wide_codeobj_cpu.py), and it is the wide sweep's + 4 B per kept
    # hit of the block-end merge: static 4 x 64 x 24 B + the hit counter; dynamic LDS unchanged - the rates are kernel
    # arguments
    assert k[".vgpr_count"] <= 80, k[".vgpr_count"]
    assert 4 * 64 * 24 <= k[".group_segment_fixed_size"] <= 4 * 64 * 24 + 64, k[".group_segment_fixed_size"]
    assert k[".group_segment_fixed_size"] + 4095 * 8 + 4 * (4096 * 6 + 4) <= 160 * 1024
    assert k[".max_flat_workgroup_size"] == 256
    (k,) = [k for n, k in kernels.items() if NEW[1] in n]
    assert k[".vgpr_count"] <= 64 and k[".max_flat_workgroup_size"] == 1024
    assert 16 * 64 * 24 <= k[".group_segment_fixed_size"] <= 16 * 64 * 24 + 64
    (k,) = [k for n, k in kernels.items() if NEW[2] in n]
    assert k[".vgpr_count"] <= 64 and k[".group_segment_fixed_size"] == 0 and k[".max_flat_workgroup_size"] == 256
