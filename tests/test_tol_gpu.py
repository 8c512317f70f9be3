"""GPU parity of the opt-in tolerant match (tvz_find_duplicates_tol / tvz_match_tol), bit-exact on ids, counts and
kth: at tol 0 against the exact path, above against the restatement of its contract (tests/tol_ref.py), at every
internal query-length boundary, after mutations, batched, sharded and end to end through the Inspector."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest
import torch

from tests import tol_ref
from tvidz_amd import _lib, corpus as tc, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEVER = tc.KTH_NEVER
LDS_KEYS = 8192                    # tvz_tol_kernels.h kTolLdsKeys: longer sorted queries are searched in device memory


def _load(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return json.load(f)


def _rows(corpus):
    return [(int(v), [float("nan") if x is None else float(x) for x in t]) for v, t in corpus]


def _tol(dc, q, tol, mm, excl=-1, cap=None, fill=None):
    """tvz_find_duplicates_tol through ctypes (also at tol 0, which DeviceCorpus sends to the exact call):
    -> ([(video_id, count, kth)] of the first min(n, cap), n)."""
    lib = _lib.load()
    q = np.ascontiguousarray(np.asarray(q, dtype=np.float64))
    cap = max(dc.stats()[0], 1) if cap is None else cap
    ids = np.full(max(cap, 1), -7 if fill is None else fill, dtype=np.int32)
    cnt, kth = ids.copy(), ids.copy()
    n = C.c_int64(-7)
    _lib.check(lib.tvz_find_duplicates_tol(dc._h, C.c_void_p(q.ctypes.data) if q.size else None, q.size, float(tol),
                                           int(mm), int(excl), cap, C.c_void_p(ids.ctypes.data),
                                           C.c_void_p(cnt.ctypes.data), C.c_void_p(kth.ctypes.data), C.byref(n)))
    m = min(n.value, cap)
    return list(zip(ids[:m].tolist(), cnt[:m].tolist(), kth[:m].tolist())), n.value


def _check(dc, rows, q, tol, mm, excl=-1, form="brute"):
    exp = tol_ref.find_duplicates_tol(rows, q, tol, mm, excl, form=form)
    got, n = _tol(dc, q, tol, mm, excl)
    assert n == len(exp) and got == exp, (tol, mm, excl, got[:8], exp[:8])
    return got


@pytest.fixture(scope="module")
def dc():
    c = tc.DeviceCorpus(0)
    yield c
    c.close()


# ---- 1. tol 0 is the exact path ---------------------------------------------------------------------------------
def test_tol_zero_equals_the_exact_path_on_the_golden_fixtures(dc, golden_dir):
    g = _load(golden_dir, "match_kat.json")
    for case in g["cases"] + [g["nan_case"]]:
        dc.upload(_rows(case["corpus"]))
        q = [float("nan") if x is None else x for x in case["query"]]
        got, _ = _tol(dc, q, 0.0, case["min_match"])
        assert got == dc.find_duplicates(q, case["min_match"], with_kth=True), case["name"]
        assert [(v, c) for v, c, _ in got] == [tuple(e) for e in case["expected"]], case["name"]
    g = _load(golden_dir, "match_random.json")
    last = None
    for case in g["cases"]:
        if case["corpus_ref"] != last:
            dc.upload(_rows(g["corpora"][str(case["corpus_ref"])]))
            last = case["corpus_ref"]
        got, _ = _tol(dc, case["query"], 0.0, case["min_match"])
        assert got == dc.find_duplicates(case["query"], case["min_match"], with_kth=True), case["name"]
        assert [(v, c) for v, c, _ in got] == [tuple(e) for e in case["expected"]], case["name"]
    g = _load(golden_dir, "match_streaming.json")
    for case in g["cases"]:
        dc.upload(_rows(case["corpus"]))
        dedup = []
        for ts in case["stream"]:
            if not dedup or ts != dedup[-1]:
                dedup.append(ts)
        got, _ = _tol(dc, dedup, 0.0, case["min_match"], case["self_id"])
        assert got == dc.find_duplicates(dedup, case["min_match"], exclude_id=case["self_id"], with_kth=True)
        if got:
            kstar = min(k for _, _, k in got)
            assert sorted(v for v, _, k in got if k == kstar) == case["dup_ids"], case["name"]
            assert dedup[:kstar + 1] == case["scene_timestamps"], case["name"]


@pytest.mark.parametrize("C,mean_len,seed", [(300, 40, 1), (3000, 200, 2), (800, 120, 3)])
def test_tol_zero_equals_the_exact_path_on_random_corpora(dc, C, mean_len, seed):
    ids, offs, keys = synth.synth_timestamp_corpus(C, seed=seed, mean_len=mean_len, dup_frac=0.05, frag_frac=0.05)
    dc.upload_csr(ids, offs, keys)
    rng = np.random.default_rng(seed)
    for t in range(12):
        r = int(rng.integers(0, C))
        q = keys[offs[r]:offs[r + 1]].tolist()
        if t % 3 == 1:
            q = q[: max(1, len(q) // 3)] + rng.choice(keys, size=20).tolist()
        if t % 3 == 2:
            q = rng.choice(keys, size=int(rng.integers(0, 300))).tolist()
        for mm in (-1, 0, 1, 2, 3, 5, 6, 9):
            excl = int(ids[r]) if t % 2 else -1
            assert _tol(dc, q, 0.0, mm, excl)[0] == dc.find_duplicates(q, mm, exclude_id=excl, with_kth=True)


# ---- 2. tol > 0 against the restatement -------------------------------------------------------------------------
def _grid_corpus(rng, n_rows, tb_den):
    """Rows of cut times from 24/25/30 fps frame grids as a container with time base 1/tb_den prints them."""
    rows = []
    for v in range(n_rows):
        fps = [24, 25, 30][v % 3]
        fr = np.sort(rng.choice(np.arange(1, 600 * fps), size=int(rng.integers(1, 120)), replace=False))
        rows.append((v + 1, [tol_ref.pts_time(int(round(f * tb_den / fps)), 1, tb_den) for f in fr]))
    return rows


@pytest.mark.parametrize("tb_den", [1000, 15360, 90000])
def test_frame_grid_corpora_against_the_restatement(dc, tb_den):
    rng = np.random.default_rng(tb_den)
    rows = _grid_corpus(rng, 240, tb_den)
    dc.upload(rows)
    for t in range(10):
        v = int(rng.integers(0, len(rows)))
        fps = [24, 25, 30][v % 3]
        # the same video remuxed into another time base, or re-cut to another frame rate, or unrelated
        other = [1000, 15360, 90000][t % 3]
        q = [tol_ref.pts_time(int(round(round(x * fps) * other / fps)), 1, other) for x in rows[v][1]]
        if t % 4 == 3:
            q = [tol_ref.pts_time(int(np.ceil(x * 25 - 1e-9)), 1, 25) for x in rows[v][1]]
        if t % 5 == 4:
            q = rng.uniform(0, 600, size=150).tolist()
        for tol in (0.0005, 0.001, 1 / 60, 0.1):
            for mm in (1, 2, 3, 6):
                _check(dc, rows, q, tol, mm, excl=(v + 1) if t % 2 else -1, form="sorted")


@pytest.mark.parametrize("mm", [-1, 0, 1, 2, 5, 6, 40])
def test_edge_cases_against_the_restatement(dc, mm):
    for name, rows, q, tol in tol_ref.edge_rows_and_queries():
        dc.upload(rows)
        for excl in (-1, 1):
            _check(dc, rows, q, tol, mm, excl)


def test_cap_truncation_reports_the_true_count(dc):
    rows = [(v, [1.0, 2.0, 3.0 + v * 1e-4]) for v in range(50)]
    dc.upload(rows)
    exp = tol_ref.find_duplicates_tol(rows, [1.0002, 3.0], 0.001, 1)
    assert len(exp) == 50
    for cap in (0, 1, 7, 50, 64):
        got, n = _tol(dc, [1.0002, 3.0], 0.001, 1, cap=cap)
        assert n == 50 and got == exp[:cap]


def test_block_hit_list_past_its_stage(dc):
    """test_match_gpu's case through match_tol (the sweep: no cell postings): every block of ts_match_tol_kernel goes
    past its 256-entry stage, at min_match 6 the hits go through the tolerant fix-up walk, and a small cap clips the
    flush."""
    from tests.test_match_gpu import check_past_the_stage, past_the_stage_case
    ids, offs, keys, queries, excl, kth = past_the_stage_case()
    dc.upload_csr(ids, offs, keys)
    d_q, d_off, max_len = tc.pack_queries(queries, DEV)
    d_ex = torch.tensor(excl, dtype=torch.int32, device=DEV)

    def run(mm, cap):
        hits, n = dc.match_tol(d_q, d_off, max_len, 0.001, mm, cap, d_exclude_ids=d_ex)
        torch.cuda.synchronize()
        return hits.cpu().numpy(), n.cpu().numpy()
    check_past_the_stage(run, ids, excl, kth)


# ---- 3. query lengths across every internal boundary ------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, LDS_KEYS - 1, LDS_KEYS, LDS_KEYS + 1, 10000])
def test_query_lengths_across_the_boundaries(dc, n):
    rng = np.random.default_rng(n)
    rows = _grid_corpus(rng, 120, 1000)
    dc.upload(rows)
    q = rng.uniform(-5, 600, size=n)
    q[: min(n, 60)] = np.asarray(rows[7][1] * 60)[: min(n, 60)] + 0.0003
    if n > 3:
        q[1] = np.nan
    for tol, mm in ((0.001, 2), (0.02, 1), (0.001, 6), (0.0, 3)):
        got = _check(dc, rows, q.tolist(), tol, mm, excl=3, form="sorted")
        if tol == 0.0:
            assert got == dc.find_duplicates(q.tolist(), mm, exclude_id=3, with_kth=True)
    # the batched form: every query of the launch in LDS, or (max_query_len above the LDS table) in device memory
    qs = [q.tolist(), q[: max(1, n // 2)].tolist(), rows[5][1]]
    d_q, d_off, max_len = tc.pack_queries(qs, DEV)
    hits, hn = dc.match_tol(d_q, d_off, max_len, 0.001, 2, len(rows))
    torch.cuda.synchronize()
    hits, hn = hits.cpu().numpy(), hn.cpu().numpy()
    for i, qq in enumerate(qs):
        exp = tol_ref.find_duplicates_tol(rows, qq, 0.001, 2, form="sorted")
        assert hn[i] == len(exp) and sorted(tuple(int(x) for x in h) for h in hits[i, :hn[i]]) == exp


# ---- 4. after mutation -----------------------------------------------------------------------------------------
def test_index_plus_delta_after_upserts_and_clear(dc):
    rng = np.random.default_rng(11)
    ids, offs, keys = synth.synth_timestamp_corpus(6000, seed=5, mean_len=60)
    dc.upload_csr(ids, offs, keys)
    assert dc.index_stats()["indexed_rows"] == 6000
    rows = {int(ids[c]): keys[offs[c]:offs[c + 1]].tolist() for c in range(len(ids))}
    for v in rng.choice(ids, size=40, replace=False):
        rows[int(v)] = (np.asarray(rows[int(v)]) + 0.0004).tolist()    # replaced rows (delta table)
        dc.upsert(int(v), rows[int(v)])
    for v in range(900001, 900021):                                     # new rows
        rows[v] = np.sort(rng.uniform(0, 600, 50)).tolist()
        dc.upsert(v, rows[v])
    assert dc.index_stats()["delta_rows"] > 0
    table = sorted(rows.items())
    for v in (900003, int(ids[17])):
        q = (np.asarray(rows[v]) - 0.0007).tolist()
        exp = tol_ref.find_duplicates_tol(table, q, 0.001, 2, form="sorted")
        got, n = _tol(dc, q, 0.001, 2)
        assert got == exp and n == len(exp) and any(h[0] == v for h in got)
    dc.clear()
    assert _tol(dc, rows[900003], 0.001, 1) == ([], 0)
    dc.upsert(5, [1.0, 2.0])
    assert _tol(dc, [1.0004, 2.0004], 0.001, 2) == ([(5, 2, 1)], 1)


def test_read_your_writes_with_upserts_racing_on_another_thread(dc):
    ids, offs, keys = synth.synth_timestamp_corpus(2000, seed=8, mean_len=40)
    dc.upload_csr(ids, offs, keys)
    stop = threading.Event()
    errors = []

    def writer():
        rng = np.random.default_rng(1)
        try:
            i = 0
            while not stop.is_set():
                dc.upsert(800000 + (i % 300), np.sort(rng.uniform(0, 600, 40)).tolist())
                dc.find_duplicates(rng.uniform(0, 600, 40).tolist(), 2, tolerance=0.01)
                i += 1
        except Exception as e:          # pragma: no cover - reported below
            errors.append(e)

    th = threading.Thread(target=writer)
    th.start()
    try:
        rng = np.random.default_rng(2)
        for i in range(60):
            fp = np.sort(rng.uniform(0, 600, 30)) + 1000.0 * (i + 1)      # nobody else's times
            dc.upsert(700000 + i, fp.tolist())
            got, _ = _tol(dc, (fp + 0.0005).tolist(), 0.001, 2, cap=4096)
            assert (700000 + i, 30, 1) in got, (i, got)
    finally:
        stop.set()
        th.join()
    assert not errors, errors


# ---- 5. batch --------------------------------------------------------------------------------------------------
def test_batch_equals_single_calls_and_topk(dc):
    rng = np.random.default_rng(21)
    rows = _grid_corpus(rng, 400, 15360)
    dc.upload(rows)
    qs = []
    for t in range(23):
        v = int(rng.integers(0, len(rows)))
        q = (np.asarray(rows[v][1]) + rng.choice([0.0, 0.0003, -0.0004])).tolist()
        qs.append(q if t % 5 else rng.uniform(0, 600, 80).tolist())
    qs.append([])
    excl = [int(rng.integers(0, 400)) for _ in qs]
    d_q, d_off, max_len = tc.pack_queries(qs, DEV)
    d_ex = torch.tensor(excl, dtype=torch.int32, device=DEV)
    for tol, mm in ((0.001, 2), (0.02, 1), (0.001, 4), (0.001, 7), (0.001, 0)):
        hits, hn = dc.match_tol(d_q, d_off, max_len, tol, mm, len(rows), d_exclude_ids=d_ex)
        top = tc.topk(hits, hn, 8)
        torch.cuda.synchronize()
        h, n, tp = hits.cpu().numpy(), hn.cpu().numpy(), top.cpu().numpy()
        for i, q in enumerate(qs):
            single, ns = _tol(dc, q, tol, mm, excl[i])
            assert n[i] == ns and sorted(tuple(int(x) for x in e) for e in h[i, :n[i]]) == single, (tol, mm, i)
            best = sorted(single, key=lambda e: (e[2], e[0], e[1]))[:8]
            best += [(-1, 0, NEVER)] * (8 - len(best))
            assert [tuple(int(x) for x in e) for e in tp[i]] == best, (tol, mm, i)


def test_batch_overflow_and_too_long_queries_are_flagged(dc):
    rows = [(v, [1.0, 2.0, 3.0]) for v in range(100)]
    dc.upload(rows)
    qs = [[1.0003, 2.0], [1.0] * 10, [2.0]]
    d_q, d_off, _ = tc.pack_queries(qs, DEV)
    hits, hn = dc.match_tol(d_q, d_off, 5, 0.001, 1, 16)            # max_query_len 5 is not an upper bound
    torch.cuda.synchronize()
    n = hn.cpu().numpy()
    assert n[0] == 100 and n[1] == np.iinfo(np.int32).min and n[2] == 100
    got = {tuple(int(x) for x in e) for e in hits.cpu().numpy()[0]}
    assert len(got) == 16 and got <= set(tol_ref.find_duplicates_tol(rows, qs[0], 0.001, 1))


# ---- 6. refusals -----------------------------------------------------------------------------------------------
def test_invalid_tolerances_write_nothing(dc):
    dc.upload([(1, [1.0, 2.0])])
    for bad in (-0.001, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(RuntimeError, match="tol must be finite"):
            _tol(dc, [1.0], bad, 1, fill=-5)
        ids = np.full(4, -5, dtype=np.int32)
        n = C.c_int64(-5)
        rc = _lib.load().tvz_find_duplicates_tol(dc._h, C.c_void_p(np.array([1.0]).ctypes.data), 1, bad, 1, -1, 4,
                                                 C.c_void_p(ids.ctypes.data), C.c_void_p(ids.ctypes.data), None,
                                                 C.byref(n))
        assert rc == -1 and n.value == -5 and (ids == -5).all()
        d_q, d_off, ml = tc.pack_queries([[1.0]], DEV)
        out_h = torch.full((1, 4, 3), -5, dtype=torch.int32, device=DEV)
        out_n = torch.full((1,), -5, dtype=torch.int32, device=DEV)
        with pytest.raises(RuntimeError, match="tol must be finite"):
            dc.match_tol(d_q, d_off, ml, bad, 1, 4, out_hits=out_h, out_n=out_n)
        torch.cuda.synchronize()
        assert (out_h == -5).all() and (out_n == -5).all()
        with pytest.raises(RuntimeError, match="tol must be finite"):
            dc.find_duplicates([1.0], 1, tolerance=bad)


def test_workspace_without_room_is_refused(dc):
    dc.upload([(1, [1.0])])
    d_q, d_off, ml = tc.pack_queries([[1.0]] * 4, DEV)
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    hits = torch.empty((4, 4, 3), dtype=torch.int32, device=DEV)
    n = torch.full((4,), -5, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    rc = lib.tvz_match_tol(dc._h, d_q.data_ptr(), d_off.data_ptr(), 4, ml, 0.001, 1, None, 4, hits.data_ptr(),
                           n.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == -5 and b"bytes missing" in lib.tvz_last_error()
    torch.cuda.synchronize()
    assert (n == -5).all()
    need = tc.tol_workspace_bytes(4, ml, d_q.numel())
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    _lib.check(lib.tvz_match_tol(dc._h, d_q.data_ptr(), d_off.data_ptr(), 4, ml, 0.001, 1, None, 4, hits.data_ptr(),
                                 n.data_ptr(), ws.data_ptr(), ws.numel(), None))
    torch.cuda.synchronize()
    assert (n == 1).all()


# ---- 7. scale --------------------------------------------------------------------------------------------------
def test_config3_corpus_with_sampled_queries():
    ids, offs, keys = synth.synth_timestamp_corpus(100_000)
    dc = tc.DeviceCorpus(0)
    try:
        dc.upload_csr(ids, offs, keys)
        rng = np.random.default_rng(3)
        for t in range(3):
            r = int(rng.integers(0, len(ids)))
            q = keys[offs[r]:offs[r + 1]] + (0.0003 if t else 0.0)
            if t == 2:
                q = np.sort(rng.uniform(600, 7200, 200))
            for tol in (0.001, 0.1):
                exp = tol_ref.find_duplicates_tol_csr(ids, offs, keys, q, tol, 2, exclude_id=int(ids[(r + 1) % len(ids)]))
                got = dc.find_duplicates(q.tolist(), 2, exclude_id=int(ids[(r + 1) % len(ids)]), with_kth=True,
                                         tolerance=tol)
                assert got == exp, (t, tol, len(got), len(exp))
    finally:
        dc.close()


# ---- 8. end to end through the Inspector -----------------------------------------------------------------------
def test_inspector_flags_a_millisecond_remux_only_with_a_tolerance(tmp_path):
    """A 30 fps original in Y4M and a copy whose container reports time base 1/1000 and pts round(i*1000/30): cut
    frames not divisible by 3 print a different pts_time (1.13333 against 1.133), so the exact verdict misses the
    copy; match_tolerance=0.001 finds it and truncates its cut list at the same kth the exact verdict gives an
    identical copy (min_match 2: two cuts)."""
    from tests.test_inspector_gpu import H, W, T, _clip, _oracle_cuts
    from tvidz_amd import db as tdb, feeder, inspector as insp

    luma = _clip(7, [34, 91, 172, 241])
    exp = _oracle_cuts(luma)
    assert [round(x * 30) for x in exp] == [34, 91, 172, 241]

    h_, w_, t_ = H, W, T

    class MkvReader:
        H, W, bitdepth, total_frames = h_, w_, 8, t_
        time_base = (1, 1000)

        def __init__(self):
            self.t = 0

        def read_into(self, out):
            n = min(out.shape[0], T - self.t)
            out[:n] = luma[self.t:self.t + n]
            self.t += n
            return n

        def pts_of(self, n):
            return round(n * 1000 / 30)

        def close(self):
            pass

    copy_cuts = [tol_ref.pts_time(round(i * 1000 / 30), 1, 1000) for i in (34, 91, 172, 241)]
    assert all(a != b for a, b in zip(copy_cuts, exp))
    for tol, dup in ((0.0, False), (0.001, True)):
        store = tdb.Store(f"sqlite:///{tmp_path}/t{int(dup)}.db", device=0)
        files = {"1700000060-orig.y4m": str(tmp_path / "orig.y4m")}
        feeder.write_y4m(files["1700000060-orig.y4m"], luma)

        def source(bucket, key, filename, uid):
            return (MkvReader(), None) if key.endswith(".mkv") else (feeder.Y4MReader(files[key]), None)
        ins = insp.Inspector(store, device=DEV, frame_source=source, batch=64, match_tolerance=tol)
        try:
            r1 = ins.analyze_file("videos", "1700000060-orig.y4m")
            assert r1["status"] == "done" and r1["scene_cuts"] == exp
            r2 = ins.analyze_file("videos", "1700000061-copy.mkv")
            assert r2["status"] == "done", r2
            if dup:
                assert r2["scene_cuts"] == copy_cuts[:2] and r2["duplicates"] == ["orig.y4m"], r2
            else:
                assert r2["scene_cuts"] == copy_cuts and r2["duplicates"] == [], r2
        finally:
            ins.close()
            store.close()


def test_inspector_refuses_a_tolerance_the_corpus_cannot_answer(tmp_path):
    from tvidz_amd import inspector as insp

    class NoTolCorpus:
        def find_duplicates(self, q, mm, exclude_id=-1, with_kth=False):
            return []

    class StoreStub:
        corpus = NoTolCorpus()

    with pytest.raises(RuntimeError, match="no tolerant match"):
        insp.Inspector(StoreStub(), device=DEV, match_tolerance=0.001)
    with pytest.raises(ValueError):
        insp.Inspector(StoreStub(), device=DEV, match_tolerance=float("nan"))
    insp.Inspector(StoreStub(), device=DEV).close()                  # the default asks for nothing


# ---- 9. shards -------------------------------------------------------------------------------------------------
def test_sharded_corpus_gives_the_single_handle_answers(dc):
    from tvidz_amd import service
    rng = np.random.default_rng(9)
    rows = _grid_corpus(rng, 500, 90000)
    dc.upload(rows)
    sc = service.ShardedCorpus(0, n_shards=8, k=8)
    try:
        sc.upload(rows)
        for t in range(8):
            v = int(rng.integers(0, len(rows)))
            q = (np.asarray(rows[v][1]) + 0.0004 * (t % 3)).tolist()
            for tol, mm in ((0.001, 2), (0.1, 2), (0.001, 6)):
                excl = rows[v][0] if t % 2 else -1
                single = dc.find_duplicates(q, mm, exclude_id=excl, with_kth=True, tolerance=tol)
                assert sc.find_duplicates(q, mm, exclude_id=excl, with_kth=True, tolerance=tol) == single
                assert sc.find_duplicates(q, mm, exclude_id=excl, tolerance=tol) == [(a, b) for a, b, _ in single]
    finally:
        sc.close()
