"""The build-regime cases of the inverted index (tests/index_build_cases.py), checked without a GPU: the restated sizing
assumes the constants and the rules that the sources hold, every shape lands in the regime it is named for - first build
and hinted rebuild, and again after the mutations - the generators keep their promises (sorted rows, the roles of the
common keys, exact counts), the references agree with each other, and no query has more hits than the GPU test's cap."""
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import index_build_cases as cases
from tests import tol_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tvidz_amd", "csrc")
with open(os.path.join(CSRC, "tvz_handle.h")) as _f:
    HANDLE = _f.read()
with open(os.path.join(CSRC, "tvz_index_kernels.h")) as _f:
    KERNELS = _f.read()
with open(os.path.join(CSRC, "tvz_index_build.h")) as _f:
    BUILD = " ".join(_f.read().split())

NAMES = list(cases.SHAPES)


def _const(src, name):
    m = re.search(r"constexpr\s+(?:int|int64_t)\s+" + name + r"\s*=\s*([0-9* ]+);", src)
    assert m, name
    v = 1
    for f in m.group(1).split("*"):
        v *= int(f)
    return v


def _hits(c, q, mm):
    cnt, kth = oracle.match_kth_csr(q, c.offs, c.keys, mm, sorted_unique=True)
    r = np.flatnonzero(cnt >= mm)
    return sorted(zip(c.ids[r].tolist(), cnt[r].tolist(), kth[r].tolist()))


def test_assumed_constants_are_the_ones_in_the_sources():
    C = cases.CONSTANTS
    assert _const(KERNELS, "kIxMaxParts") == C["kIxMaxParts"] == 4096
    assert _const(KERNELS, "kIxStagePairs") == C["kIxStagePairs"] == 8192
    assert _const(HANDLE, "kIxSliceBytes") == C["kIxSliceBytes"] == 32768
    assert _const(HANDLE, "kIxSliceBytesMax") == C["kIxSliceBytesMax"] == 131072
    assert _const(HANDLE, "kIxDirLoadPct") == C["kIxDirLoadPct"] == 25
    assert _const(HANDLE, "kIxSliceLdsFloor") == C["kIxSliceLdsFloor"] == 40960
    assert _const(HANDLE, "kLdsPerWorkgroup") == cases.LDS_PER_WORKGROUP
    m = re.search(r"#define TVZ_IX_SUB_LOG2 (\d+)", KERNELS)
    assert m and int(m.group(1)) == C["TVZ_IX_SUB_LOG2"] == 14
    assert _const(HANDLE, "kIndexMinDelta") == 512 and "std::max<int64_t>(kIndexMinDelta, n_main / 256)" in BUILD
    assert cases.delta_trigger(cases.ROWS_2) == 512 and cases.delta_trigger(cases.ROWS_57) == 3600


def test_the_layout_query_is_declared_bound_and_refuses_null():
    import ctypes as C
    from tvidz_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "tvz.h")) as f:
        assert re.search(r"\bint\s+tvz_corpus_index_layout\s*\(tvz_corpus \*c, int64_t out\[8\]\);", f.read())
    assert "tvz_corpus_index_layout" in _lib.SIGNATURES and hasattr(lib, "tvz_corpus_index_layout")
    out = (C.c_int64 * 8)(*range(1, 9))
    assert lib.tvz_corpus_index_layout(None, out) == -1 and list(out) == list(range(1, 9))      # nothing written
    assert b"NULL" in lib.tvz_last_error()


def test_the_sizing_rules_are_the_ones_restated():
    """The lines of build_classic that `layout` restates, as text: a change of the rule fails here first."""
    assert "inline int ix_ks(int n_sub) { return n_sub <= 1 ? 0 : (n_sub + 7) & ~7; }" in KERNELS
    assert "inline int ix_entry_bytes(int ks) { return 16 + 2 * ks; }" in KERNELS
    for line in (
        "while (((int64_t)2 << sl) * es <= kIxSliceBytes && sl < lg) ++sl;",
        "while ((((int64_t)1 << lg) >> sl) > kIxMaxParts && ((int64_t)2 << sl) * es <= kIxSliceBytesMax) ++sl;",
        "return (((int64_t)1 << lg) >> sl) <= kIxMaxParts && ((int64_t)es << sl) <= kIxSliceBytesMax;",
        "int lg = 10; while ((double)((int64_t)1 << lg) * kIxDirLoadPct < 100.0 * distinct && lg < 30) ++lg;",
        "if (!partitionable(lg) && partitionable(lg - 1) && (double)((int64_t)1 << (lg - 1)) >= 2.0 * distinct) --lg;",
        "log2 = size_for((double)hint.distinct * (double)live_keys / (double)hint.post * 1.25);",
        "log2 = size_for((double)guess);",
        "while (((int64_t)1 << log2) < live_keys / 8) ++log2;",
        "slice_log2 = 6; while (((int64_t)2 << slice_log2) * es <= kIxSliceBytes && slice_log2 < log2) ++slice_log2;",
        "while ((dn >> slice_log2) > kIxMaxParts && ((int64_t)2 << slice_log2) * es <= kIxSliceBytesMax) ++slice_log2;",
        "partitioned = n_parts <= kIxMaxParts && post_cap < (int64_t)0xfffffff0LL &&",
        "if (!partitioned) slice_log2 = log2;",
        "if (!info.failed && (int64_t)info.n_distinct * 2 <= dn) {",
        "if (!shrunk && (fit + 1 < log2 || fit > log2)) { log2 = fit; shrunk = true; continue; }",
        "d.partitioned = partitioned;",
    ):
        assert line in BUILD, line
    # what the rule gives where the documents state it: 1 M rows, 62 sub-indexes, 144-byte entries, exactly 4,096 slices
    assert cases.ix_entry_bytes(cases.ix_ks(62)) == 144 and cases.ix_entry_bytes(cases.ix_ks(19)) == 64
    lay = cases.layout(1_000_000, 2_000_000, 600_000, hint=(2_000_000, 600_000))
    assert lay == cases.Layout(144, 21, 9, 1)
    # a small corpus of repeated keys: slices of 32 KB, fewer than kIxMaxParts
    assert cases.layout(300_000, 1_000_000, 40_000) == cases.Layout(64, 18, 9, 1)


@pytest.mark.parametrize("name", NAMES)
def test_every_shape_lands_in_the_regime_it_is_named_for(name):
    s, c, C = cases.SHAPES[name], cases.corpus(name), cases.CONSTANTS
    live, distinct = cases.counts(c)
    trace = []
    first = cases.layout(s.rows, live, distinct, trace=trace)
    rebuilt = cases.layout(s.rows, live, distinct, hint=(live, distinct))
    assert first == s.first and rebuilt == s.rebuilt
    es = first.entry_bytes
    assert es == (32 if name in cases.TWO_SUB else 144) and cases.n_sub(s.rows) == (2 if name in cases.TWO_SUB else 57)
    for lay in (first, rebuilt):
        slice_bytes, parts = es << lay.slice_log2, 1 << (lay.log2 - lay.slice_log2)
        if name == "wide_unpartitioned":
            assert not lay.partitioned and lay.slice_log2 == lay.log2
            assert not cases.partitionable(lay.log2, es)
            continue
        # the large slices, exactly as many as the partition kernels hold, each within the LDS of one block
        assert lay.partitioned and parts == C["kIxMaxParts"]
        assert slice_bytes == {"slice64k": 65536, "slice128k": 131072, "slice128k_half_load": 131072,
                               "wide_partitioned": 73728}[name]
        assert cases.slice_lds_bytes(lay) == slice_bytes > C["kIxSliceLdsFloor"]
        assert cases.slice_lds_bytes(lay) + 1024 <= cases.LDS_PER_WORKGROUP         # + the kernels' static arrays
        assert cases.scatter_lds_bytes(lay) + 1024 <= cases.LDS_PER_WORKGROUP
        assert distinct * 2 <= 1 << lay.log2
    if name in ("slice128k_half_load", "wide_partitioned"):
        # the size for load 0.25 cannot be built slice by slice: size_for steps down to load <= 0.5
        assert (1 << first.log2) * C["kIxDirLoadPct"] < 100 * distinct
        assert not cases.partitionable(first.log2 + 1, es) and cases.partitionable(first.log2, es)
    if name in ("slice64k", "slice128k"):
        assert (1 << first.log2) * C["kIxDirLoadPct"] >= 100 * distinct
    if name == "wide_unpartitioned":
        # the first upload meets both builds: crowded partitioned attempts, then the unpartitioned count twice
        assert [p for _, p in trace] == [True] * 4 + [False] * 2 and trace[-1][0] == 23 and trace[0][0] == 18
    # the device footprint the GPU module's docstring states, in GB
    gb = lambda lay: round(cases.footprint_bytes(lay) / 1e9, 1)
    assert (gb(first), gb(rebuilt)) == {"slice64k": (0.8, 0.8), "slice128k": (1.6, 1.6), "slice128k_half_load": (1.6, 1.6),
                                        "wide_partitioned": (0.9, 0.9), "wide_unpartitioned": (5.8, 11.5)}[name]
    # the cell directory of a 1 ms cell is guessed from the key directory's count: the same regime
    posts, cells = cases.cell_counts(c, 0.001)
    assert 0 < distinct - cells < 100 and posts <= live
    cl = cases.layout(s.rows, live, cells, guess=distinct)
    assert cl == first
    assert cases.layout(s.rows, live, cells, hint=(posts, cells)) == rebuilt


@pytest.mark.parametrize("name", NAMES)
def test_the_generators_keep_their_promises(name):
    s, c = cases.SHAPES[name], cases.corpus(name)
    n, subs = s.rows, cases.n_sub(s.rows)
    assert c.ids.size == n and c.offs.size == n + 1 and c.offs[-1] == c.keys.size
    assert (c.ids == np.arange(1, n + 1)).all()
    lens = np.diff(c.offs)
    row = np.repeat(np.arange(n), lens)
    inside = row[1:] == row[:-1]
    assert (np.diff(c.keys)[inside] > 0).all()                       # every row sorted, no repeats
    assert not np.isnan(c.keys).any() and not (np.signbit(c.keys) & (c.keys == 0)).any() and (c.keys > 0).all()
    assert lens.min() >= s.own and lens.max() <= s.own + 1 + 8 + 4
    own = c.keys[c.keys > cases.OWN_BASE]
    grid = (own - cases.OWN_BASE) / cases.OWN_STEP
    assert ((grid == np.round(grid)) | (np.abs(grid - np.floor(grid) - cases.NEAR / cases.OWN_STEP) < 1e-6)).all()
    # the common keys: ~1 % of the rows, and every role
    common = c.keys < cases.OWN_BASE
    assert set(np.unique(c.keys[common])) <= set(cases.POOL)
    carriers = np.unique(row[common])
    assert 0.009 * n < carriers.size < 0.012 * n + 200
    sub_of = lambda p: np.unique(row[c.keys == cases.POOL[p]] >> 14)
    assert sub_of(cases.P_EVERY).tolist() == list(range(subs))
    assert sub_of(cases.P_FIRST).tolist() == [0]
    assert sub_of(cases.P_LAST).tolist() == [subs - 1]
    assert sub_of(cases.P_MID).tolist() == [subs // 2]
    assert sub_of(cases.P_LONG).tolist() == [cases.long_sub(s)]
    assert (c.keys == cases.POOL[cases.P_LONG]).sum() == cases.LONG_POSTINGS > 64
    # two keys of one row in one 1 ms cell
    cell = np.floor(c.keys / 0.001)
    assert (inside & (np.diff(cell) == 0)).sum() >= 3
    live, distinct = cases.counts(c)
    assert live == c.keys.size and distinct == len(set(c.keys.tolist()))
    # deterministic
    cases.corpus.cache_clear()
    again = cases.corpus(name)
    assert (again.offs == c.offs).all() and (again.keys == c.keys).all()


@pytest.mark.parametrize("name", NAMES)
def test_queries_fit_the_cap_and_reach_every_mode(name):
    s, c, qs = cases.SHAPES[name], cases.corpus(name), cases.queries(name)
    assert len(qs) <= 8
    most = 0
    for qi, q in enumerate(qs):
        h1 = _hits(c, q, 1)                                          # min_match 1 has the most hits
        assert len(h1) <= cases.HIT_CAP, (qi, len(h1))
        most = max(most, len(h1))
    assert most > 100                                                # (the pool query)
    for qi in (0, 1, 2):                                             # copies of two rows: both hit at min_match 2
        ids = [v for v, _, _ in _hits(c, qs[qi], 2)]
        sp = cases.special_rows(s)
        pair = [(sp[0], sp[1]), (sp[2], sp[3]), (sp[4], sp[0])][qi]
        assert set(int(c.ids[r]) for r in pair) <= set(ids)
    assert len(_hits(c, qs[3], 6)) >= 3                              # the rows that hold eight common keys
    assert all(cnt == 3 for _, cnt, _ in _hits(c, qs[4], 2)) and len(_hits(c, qs[4], 2)) >= cases.n_sub(s.rows)
    assert _hits(c, qs[5], 1) == []
    if name in cases.TWO_SUB:
        assert len(_hits(c, qs[0], 3)) >= 2
    if name in cases.MUTATED:
        replaced, appended = cases.mutations(name)
        e = cases.edit(c, replaced, appended)
        for q in qs:
            assert len(_hits(e, q, 2)) <= cases.HIT_CAP
        assert len(_hits(e, qs[0], 2)) > len(_hits(c, qs[0], 2)) + 10          # the copies are found


@pytest.mark.parametrize("name", cases.MUTATED)
def test_the_edited_corpus_and_the_rebuild_it_triggers(name):
    s, c = cases.SHAPES[name], cases.corpus(name)
    replaced, appended = cases.mutations(name)
    assert 35 <= len(replaced) <= 45 and len(appended) == 40
    rows = sorted(replaced)
    assert rows[0] < 16384 and rows[-1] >= (cases.n_sub(s.rows) - 1) * 16384 and {16383, 16384} <= set(rows)
    assert sum(1 for k in replaced.values() if len(k) == 0) == 4
    for r in (16383, 16384):                                         # rows the queries copy: their postings go stale
        assert r in cases.special_rows(s) and not np.array_equal(replaced[r], cases.row_keys(c, r))
    e = cases.edit(c, replaced, appended)
    assert e.ids.size == s.rows + 40 and (e.ids[s.rows:] == s.rows + 1 + np.arange(40)).all()
    for r in (0, 5, s.rows - 1):
        assert (cases.row_keys(e, r) == cases.row_keys(c, r)).all()
    for r, k in replaced.items():
        assert (cases.row_keys(e, r) == k).all()
    assert (cases.row_keys(e, s.rows + 3) == appended[3][1]).all()
    # fillers until the delta table crosses its trigger: the background rebuild stays in the regime
    trigger = cases.delta_trigger(s.rows)
    assert trigger == (512 if name in cases.TWO_SUB else 3600)
    fill = [(s.rows + 100 + i, cases.filler(i)) for i in range(trigger)]
    f = cases.edit(e, {}, fill)
    live0, distinct0 = cases.counts(c)
    live, distinct = cases.counts(f)
    lay = cases.layout(f.ids.size, live, distinct, hint=(live0, distinct0))
    assert lay == s.rebuilt
    qkeys = np.concatenate(cases.queries(name))
    assert not np.isin(np.concatenate([k for _, k in fill]), qkeys).any()


def test_the_tolerant_reference_agrees_with_the_restated_contract():
    """tol_expected (the whole corpus at once) against tests/tol_ref.py (row by row) on a corpus small enough for both."""
    c = cases.corpus("slice64k")
    r0, r1 = 16384 - 300, 16384 + 300
    sub = cases.Corpus(c.ids[r0:r1], c.offs[r0:r1 + 1] - c.offs[r0], c.keys[c.offs[r0]:c.offs[r1]])
    qs = cases.queries("slice64k")
    near = cases.row_keys(c, 16383)
    qs = qs + [near + 0.0003, near - 0.0005, np.array([near[-1] + 0.0005, near[-1] + 0.00051, float("nan")])]
    some = 0
    for q in qs:
        for tol in (0.0005, 0.0):
            for mm in (1, 2):
                exp = tol_ref.find_duplicates_tol_csr(sub.ids, sub.offs, sub.keys, q, tol, mm)
                assert cases.tol_expected(sub, q, tol, mm) == exp
                some += len(exp)
    assert some > 50
