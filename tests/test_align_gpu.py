"""GPU parity of tvz_align (ts_align_kernel) with tests/align_ref.py, full rows, bit-exact, at the
kernel's edges: the grid-stride loop, rows longer than a wave, special keys, the bin-count limits
and refusals, near-boundary differences, ties, the table after every kind of mutation, and the
output capacity of the ABI (a row count read under the handle's lock, nothing written past
out_rows)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from tests import align_ref as ar
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -0x5A5A5A5A


@pytest.fixture(scope="module")
def dc():
    c = tc.DeviceCorpus(0)
    yield c
    c.close()


def _expect_equal(got, exp, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, (what, f"{bad.size} rows differ", got[bad[:4]].tolist(), exp[bad[:4]].tolist())


def _check(dc, rows, q, eps, mo, by_id=False):
    got = dc.align(q, eps=eps, max_offset=mo)
    assert got.dtype == np.int32
    exp = ar.align_ref(rows, q, eps, mo)
    if by_id:                                      # video ids unique: the same rows, whatever their order
        got, exp = got[np.argsort(got[:, 0], kind="stable")], exp[np.argsort(exp[:, 0], kind="stable")]
    _expect_equal(got, exp, (eps, mo, len(q)))
    return got


def _raw_align(dc, q, eps, mo, out, out_rows, stream=None):
    """tvz_align through the C ABI: -> (return code, *n_rows or None if untouched)."""
    n_rows = C.c_int64(-7)
    s = stream if stream is not None else torch.cuda.current_stream(DEV)
    rc = _lib.load().tvz_align(dc._h, q.data_ptr() if q.numel() else None, q.numel(), float(eps), float(mo),
                               out.data_ptr(), int(out_rows), C.byref(n_rows), s.cuda_stream)
    return rc, (None if n_rows.value == -7 else n_rows.value)


@pytest.mark.parametrize("case", ar.edge_cases(), ids=lambda c: c[0])
def test_edge_cases_bit_exact(dc, case):
    name, rows, calls = case
    dc.upload(rows)
    for q, eps, mo in calls:
        got = _check(dc, rows, q, eps, mo)
        if name == "grid_stride":
            # the premise: each wave's second row has no vote, its first and third rows do
            w = ar.GRID_WAVES
            assert len(rows) > 2 * w and (got[:w, 3] > 0).all() and (got[2 * w:, 3] > 0).all()
            assert (got[w:2 * w, 2:] == 0).all()
        if name == "bin_limits" and mo == 2047 / 64:
            assert got[:6, 2].tolist() == [2047, -2047, 0, 0, -2047, 2046]
        if name == "ties" and q == [0.0]:
            assert got[:7, 2].tolist() == [-2, 1, -1, -1, 0, 4, 0] and got[6, 3] == 0


def test_refusals_write_nothing(dc):
    """2B+1 > 4096 bins, eps <= 0 or NaN, max_offset NaN, infinite or negative: refused before any
    launch, with the error include/tvz.h names, nothing written, no row count reported."""
    rows = [(v, [float(v), v + 0.5]) for v in range(1, 41)]
    dc.upload(rows)
    q = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, device=DEV)
    out = torch.full((40, 5), SENTINEL, dtype=torch.int32, device=DEV)
    for eps, mo, code in ar.REFUSALS:
        assert _raw_align(dc, q, eps, mo, out, 40) == (code, None), (eps, mo)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    # the largest bin count accepted, right next to the refused one
    assert _raw_align(dc, q, 1 / 64, 2047.49 / 64, out, 40) == (0, 40)
    torch.cuda.synchronize()
    _expect_equal(out.cpu().numpy(), ar.align_ref(rows, [1.0, 2.0, 3.0], 1 / 64, 2047.49 / 64), "B = 2047")


def test_output_capacity_contract(dc):
    """out_rows = 60 of a 100-row table into a 100-row buffer: rows 60-99 stay untouched, *n_rows is 100,
    rows 0-59 are the table's first 60."""
    rng = np.random.default_rng(9)
    rows = [(v, np.round(rng.uniform(0, 100, int(rng.integers(1, 90))), 3).tolist()) for v in range(1, 101)]
    dc.upload(rows)
    qh = np.asarray(rows[3][1][:20]) + 0.2
    q = torch.as_tensor(qh).to(DEV)
    out = torch.full((100, 5), SENTINEL, dtype=torch.int32, device=DEV)
    assert _raw_align(dc, q, 0.1, 3.0, out, 60) == (0, 100)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[60:] == SENTINEL).all()
    exp = ar.align_ref(rows, qh, 0.1, 3.0)
    _expect_equal(got[:60], exp[:60], "first 60 rows")
    # out_rows = 0 writes nothing and still reports the count; the Python call returns every row
    assert _raw_align(dc, q, 0.1, 3.0, out, 0) == (0, 100)
    _expect_equal(dc.align(qh, eps=0.1, max_offset=3.0), exp, "all rows")


def test_align_while_another_thread_upserts(dc):
    """One thread upserts 300 new videos while another aligns over and over: every result is one
    snapshot of the table - between the row counts before and after, the old rows first and in
    order, every row equal to the reference of that video."""
    rng = np.random.default_rng(31)
    grid = np.arange(1, 30_001) / 30.0
    base = [(v, np.sort(rng.choice(grid, size=int(rng.integers(1, 60)), replace=False)).tolist())
            for v in range(1, 101)]
    new = [(v, np.sort(rng.choice(grid, size=int(rng.integers(1, 60)), replace=False)).tolist())
           for v in range(1001, 1301)]
    q = (np.asarray(base[0][1] + new[10][1]) + 2 / 30).tolist()
    eps, mo = 1 / 30, 1.0
    exp = {int(r[0]): r for r in ar.align_ref(base + new, q, eps, mo)}
    dc.upload(base)
    stop, results, errs = threading.Event(), [], []

    def aligner():
        try:
            while not stop.is_set() or not results:
                results.append(dc.align(q, eps=eps, max_offset=mo))
        except Exception as e:                                            # pragma: no cover
            errs.append(e)

    t = threading.Thread(target=aligner)
    t.start()
    try:
        for v, ts in new:
            dc.upsert(v, ts)
    finally:
        stop.set()
        t.join(120)
    assert not errs, errs[:1]
    results.append(dc.align(q, eps=eps, max_offset=mo))
    assert len(results[-1]) == 400
    for res in results:
        assert 100 <= len(res) <= 400
        assert res[:100, 0].tolist() == list(range(1, 101))
        assert res[100:, 0].tolist() == list(range(1001, 1001 + len(res) - 100))
        _expect_equal(res, np.stack([exp[int(v)] for v in res[:, 0]]), "snapshot")


def test_after_mutations(dc):
    """Replacing upserts, new rows, emptied rows, an arena compaction, build_index, clear, and a call
    on another stream right after an upsert: always the reference over the current table."""
    rng = np.random.default_rng(17)
    grid = np.arange(1, 20_001) / 30.0
    rows = {v: np.sort(rng.choice(grid, size=int(rng.integers(2, 40)), replace=False)).tolist()
            for v in range(1, 301)}
    dc.upload(list(rows.items()))
    q = (np.asarray(rows[7][:12] + rows[8][:5]) + 3 / 30).tolist()
    eps, mo = 1 / 30, 2.0

    def check():
        return _check(dc, list(rows.items()), q, eps, mo, by_id=True)

    check()
    for v in (3, 7, 100):                                                  # replacing upserts
        rows[v] = np.sort(rng.choice(grid, size=int(rng.integers(5, 90)), replace=False)).tolist()
        dc.upsert(v, rows[v])
    rows[11] = (np.asarray(q) - 1 / 30).tolist()
    dc.upsert(11, rows[11])
    assert check()[10, 2:4].tolist() == [-1, len(q)]
    for v in range(301, 321):                                              # new rows
        rows[v] = np.sort(rng.choice(grid, size=int(rng.integers(1, 200)), replace=False)).tolist()
        dc.upsert(v, rows[v])
    check()
    for v in (5, 301):                                                     # emptied rows
        rows[v] = []
        dc.upsert(v, [])
    check()
    _, _, arena0 = dc.stats()                                              # arena compaction
    compacted = False
    for it in range(400):
        v = 20 + it % 5
        rows[v] = np.sort(rng.choice(grid, size=500, replace=False)).tolist()
        dc.upsert(v, rows[v])
        arena = dc.stats()[2]
        compacted = compacted or arena < arena0
        arena0 = arena
        if compacted:
            break
    assert compacted
    check()
    dc.build_index()
    check()
    # another stream, right after an upsert
    rows[9] = (np.asarray(q) + 2 / 30).tolist()
    dc.upsert(9, rows[9])
    s2 = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s2):
        got = check()
    assert got[8, 2:4].tolist() == [2, len(q)]
    dc.clear()
    assert dc.align(q, eps=eps, max_offset=mo).shape == (0, 5)
    out = torch.full((4, 5), SENTINEL, dtype=torch.int32, device=DEV)
    assert _raw_align(dc, torch.as_tensor(np.asarray(q)).to(DEV), eps, mo, out, 4) == (0, 0)
    rows = {1: rows[7], 2: []}
    dc.upload(list(rows.items()))
    check()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


def test_sharded_corpus_align_and_near_duplicates(tmp_path):
    """service.ShardedCorpus.align = DeviceCorpus.align over the same table, as a multiset of rows; and
    Inspector(near_duplicates=True) over the sharded store reports what it reports over one handle."""
    from tests.fakes import CutReader, cut_inspector
    from tvidz_amd import db as tdb, service

    rng = np.random.default_rng(23)
    grid = np.arange(1, 20_001) / 30.0
    rows = [(v, np.sort(rng.choice(grid, size=int(rng.integers(1, 50)), replace=False)).tolist())
            for v in range(1, 501)]
    q = (np.asarray(rows[40][1]) - 4 / 30).tolist()
    sc = service.ShardedCorpus(0, n_shards=8, k=8)
    one = tc.DeviceCorpus(0)
    try:
        for c in (sc, one):
            c.upload(rows)
            c.upsert(777, q)
            c.upsert(12, rows[0][1])
        a = sc.align(q, eps=1 / 30, max_offset=5.0)
        b = one.align(q, eps=1 / 30, max_offset=5.0)
        assert a.shape == b.shape == (501, 5)
        assert sorted(map(tuple, a.tolist())) == sorted(map(tuple, b.tolist()))
    finally:
        sc.close()
        one.close()

    cuts = {"a.y4m": [1.0, 2.5, 4.0, 7.3, 9.9, 12.0], "c.y4m": [0.7, 3.3, 5.1, 8.8],
            "b.y4m": [x + 7 / 30 for x in [1.0, 2.5, 4.0, 7.3, 9.9, 12.0]]}
    reports = []
    for corpus in (service.ShardedCorpus(0, n_shards=8, k=8), tc.DeviceCorpus(0)):
        store = tdb.Store(f"sqlite:///{tmp_path}/{len(reports)}.db", corpus=corpus)
        ins = cut_inspector(store, device=DEV, near_duplicates=True,
                            frame_source=lambda bucket, key, filename, uid: (CutReader(cuts[key], frames=600), None))
        try:
            res = [ins.analyze_file("videos", k) for k in ("a.y4m", "c.y4m", "b.y4m")]
        finally:
            store.close()                      # closes the corpus too
        assert all(r["status"] == "done" for r in res), res
        reports.append([r["near_duplicates"] for r in res])
    assert reports[0] == reports[1]
    nd = reports[0][2]
    assert [d["filename"] for d in nd] == ["a.y4m"] and nd[0]["jaccard"] == 1.0
    assert abs(nd[0]["shift_seconds"] + 7 / 30) < 1e-9
