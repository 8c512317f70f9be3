"""The near-duplicate search over a sharded table without a GPU: gloo at world sizes 2 and 3 with the numpy backend of
tests/near_fakes.py.  sharded.ShardedMatcher.align_topk must be identical on every rank and equal to the restatement
of tvz_align_topk on the WHOLE table; a service.RankCorpus tick that carries near asks, top-k asks and an exact ask at
once answers each as it would alone; near asks that differ in eps do not share a batch; a near ask with a bad
parameter raises in the caller and the loop keeps running.  Then the sizing function's invariants and the launcher's
--near-* switches (refused before a child starts; a two-rank launch on fakes reports the field through the front)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import align_topk_ref as atr, align_topk_shard_ref as asr
from tests.fakes import OracleBackend, OracleCorpus
from tests.near_fakes import NearBackend, free_port_run, notify, upload_key, wait_done
from tvidz_amd import corpus as tc, service, sharded

EPS, MAX_OFFSET = 1 / 30, 3.0
NAN = float("nan")


def _small_table():
    rows, queries = asr.split_table()
    rows = rows[:45]                                                 # 15 of them shifted copies of the queries
    return rows, queries + [[float(i) for i in range(50)]]           # the last one is over-long at max_query_len = 45


def _expected(rows, queries, k, **kw):
    block = atr.topk_ref(rows, queries, EPS, MAX_OFFSET, k, max_query_len=45, **kw)
    return block[:, :k], block[:, k, 1]


def _pack(queries):
    lens = [len(q) for q in queries]
    flat = np.asarray([x for q in queries for x in q] or [0.0], dtype=np.float64)
    return torch.from_numpy(flat), torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _run(target, world):
    port = free_port_run()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in procs]
    [p.join(300) for p in procs]
    assert all(not p.is_alive() for p in procs), "a rank hung"
    res = sorted(q.get(timeout=5) for _ in range(world))
    assert res == [(r, "ok") for r in range(world)], res
    assert all(p.exitcode == 0 for p in procs)


# ---- sharded.ShardedMatcher.align_topk ---------------------------------------------------------------------------
def _matcher_worker(rank, world, port, out):
    _init(rank, world, port)
    try:
        rows, queries = _small_table()
        sm = sharded.ShardedMatcher(NearBackend(*tc.rows_to_csr(rows[rank::world])), k=16, cap=64)
        assert sm.world == world and sm.supports_align_topk
        d_q, d_off = _pack(queries)
        excl = [rows[1][0]] + [-1] * (len(queries) - 1)
        for k, kw in ((1, {}), (5, {}), (64, {}), (5, dict(min_votes=2, min_score=atr.ONE // 4, exclude_ids=excl))):
            mkw = dict(kw)
            if "exclude_ids" in mkw:
                mkw["d_exclude_ids"] = torch.tensor(mkw.pop("exclude_ids"), dtype=torch.int32)
            got_rows, got_totals = sm.align_topk(d_q, d_off, 45, eps=EPS, max_offset=MAX_OFFSET, k=k, **mkw)
            exp_rows, exp_totals = _expected(rows, queries, k, **kw)
            assert got_rows.dtype == torch.int32 and tuple(got_rows.shape) == (len(queries), k, 4)
            assert (got_rows.numpy() == exp_rows).all() and (got_totals.numpy() == exp_totals).all(), (rank, k)
            everyone = [None] * world
            dist.all_gather_object(everyone, (got_rows.tolist(), got_totals.tolist()))
            assert all(e == everyone[0] for e in everyone)                       # identical on every rank
        assert exp_totals[-1] == atr.REFUSED and _expected(rows, queries, 5)[1][0] > 5
        # a backend without the form is refused by name
        plain = sharded.ShardedMatcher(OracleBackend(*tc.rows_to_csr(rows[rank::world])), k=4, cap=64)
        assert plain.supports_align_topk is False and plain.align_forms == ()
        with pytest.raises(RuntimeError, match=f"OracleBackend has no {tc.FORM_BOUNDED.stem}"):
            plain.align_topk(d_q, d_off, 45, eps=EPS, max_offset=MAX_OFFSET, k=4)
        out.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        out.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_matcher_align_topk_equals_the_whole_table(world):
    _run(_matcher_worker, world)


# ---- service.RankCorpus: ASK_NEAR in the tick --------------------------------------------------------------------
def _rank_worker(rank, world, port, out):
    _init(rank, world, port)
    rc = None
    try:
        rows, queries = _small_table()
        shard = OracleCorpus()
        g = dist.new_group(backend="gloo")                            # the tick thread's own group
        backend = NearBackend(live=shard)
        rc = service.RankCorpus(shard, sharded.ShardedMatcher(backend, k=8, cap=64, group=g), group=g, xdev="cpu",
                                tick_s=0.01)
        rc.upload(rows)                                               # video_id mod world
        dist.barrier()
        # (1) the public call, alone: the whole table's answer, the over-long query refused without travelling
        k = 5
        exp_rows, exp_totals = _expected(rows, queries, k)
        got_rows, got_totals = rc.align_topk(queries, eps=EPS, max_offset=MAX_OFFSET, k=k, max_query_len=45)
        assert got_rows.dtype == np.int32 and got_rows.shape == (len(queries), k, 4)
        assert (got_rows == exp_rows).all() and (got_totals == exp_totals).all() and got_totals[-1] == tc.ALIGN_REFUSED
        assert all(c[0] <= world * (len(queries) - 1) for c in backend.near_calls)   # it never reached a matcher
        excl = [rows[1][0]] + [-1] * (len(queries) - 1)
        kw = dict(min_votes=2, min_score=atr.ONE // 4, exclude_ids=excl)
        got = rc.align_topk(queries, eps=EPS, max_offset=MAX_OFFSET, k=k, max_query_len=45, **kw)
        exp = _expected(rows, queries, k, **kw)
        assert (got[0] == exp[0]).all() and (got[1] == exp[1]).all()
        # (2) one tick's worth of asks of every kind, pending at once on every rank: two near asks with one eps, one
        #     with another, a top-k ask and an exact ask - each answered as it is alone
        qa, qb = np.asarray(queries[rank % 2]), np.asarray(queries[2])
        near1 = service.check_near(tc.FORM_BOUNDED, EPS, MAX_OFFSET, 4, 1, 0)
        near2 = service.check_near(tc.FORM_BOUNDED, 2 * EPS, MAX_OFFSET, 4, 1, 0)
        dup = np.asarray(rows[1][1])
        asks = [(qa, 0, -1, service.ASK_NEAR, 0.0, near1), (dup, 2, -1, service.ASK_TOPK, 0.0, None),
                (qb, 0, rows[4][0], service.ASK_NEAR, 0.0, near1), (dup, 2, -1, service.ASK_EXACT, 0.0, None),
                (qa, 0, -1, service.ASK_NEAR, 0.0, near2)]
        alone = [rc._ask_all([a])[0] for a in asks]
        dist.barrier()
        n0 = len(backend.near_calls)
        together = rc._ask_all(asks)
        dist.barrier()
        for a, (x, y) in zip(asks, zip(alone, together)):
            if a[3] == service.ASK_EXACT:
                assert x == y and len(x) >= 1
            else:
                assert (x[0] == y[0]).all() and x[1] == y[1]
        for i, eps, ex in ((0, EPS, None), (2, EPS, [rows[4][0]]), (4, 2 * EPS, None)):
            block = atr.topk_ref(rows, [asks[i][0].tolist()], eps, MAX_OFFSET, 4, exclude_ids=ex)
            assert (together[i][0] == block[0, :4]).all() and together[i][1] == block[0, 4, 1]
        assert together[1][1] >= 1 and together[1][0][0][0] == rows[1][0]       # the top-k ask found the row it copies
        # every rank answered ALL near asks of all ranks, never mixing the two eps in one batch
        calls = backend.near_calls[n0:]
        assert {c[1] for c in calls} == {EPS, 2 * EPS} and all(c[3] == 4 for c in calls)
        assert sum(c[0] for c in calls if c[1] == EPS) == 2 * world and sum(c[0] for c in calls if c[1] == 2 * EPS) == world
        # (3) refused in the caller, before the tick: nothing reaches a matcher, the loop keeps running
        n1, ticks = len(backend.near_calls), rc.busy_ticks
        if rank == 0:
            for bad in (dict(eps=0.0), dict(eps=NAN), dict(max_offset=-1.0), dict(max_offset=1000.0), dict(k=0), dict(k=65),
                        dict(min_votes=0), dict(min_score=-1), dict(min_score=atr.ONE + 1), dict(exclude_ids=[1, 2])):
                with pytest.raises(ValueError):
                    rc.align_topk([queries[0]], **{**dict(eps=EPS, max_offset=MAX_OFFSET, k=4), **bad})
            long_rows, long_totals = rc.align_topk([[0.5] * 4096], eps=EPS, max_offset=MAX_OFFSET, k=4)
            assert long_totals.tolist() == [tc.ALIGN_REFUSED] and (long_rows[:, :, 0] == -1).all()
            assert len(backend.near_calls) == n1 and rc.busy_ticks == ticks
        dist.barrier()
        got = rc.align_topk([queries[1]], eps=EPS, max_offset=MAX_OFFSET, k=k)
        assert (got[0][0] == exp_rows[1]).all() and rc.broken is None
        dist.barrier()
        out.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        out.put((rank, repr(e)))
        raise
    finally:
        if rc is not None:
            rc.close()
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_rank_corpus_answers_near_topk_and_exact_asks_of_one_tick(world):
    _run(_rank_worker, world)


def test_one_tick_calls_the_matcher_in_sorted_order():
    """World size 1: one tick that holds an exact ask, a top-k ask, a tolerant top-k ask and two near asks with
    different parameters, handed over in an order that is NOT the sorted one.  The matcher hears match_topk per
    (min_match, tolerance) in sorted order - `tolerance` named only where it is non-zero - and then align for align_topk
    per (eps, max_offset, k, min_votes, min_score) in sorted order: every rank makes its collective calls in this order."""
    from tests.tol_fakes import TolBackend, TolCorpus

    class Backend(NearBackend, TolBackend):
        pass

    calls = []

    class Recorder(sharded.ShardedMatcher):
        def match_topk(self, d_q, d_off, max_len, min_match, d_excl=None, **kw):
            calls.append(("match_topk", int(min_match), dict(kw)))
            return super().match_topk(d_q, d_off, max_len, min_match, d_excl, **kw)

        def align(self, form, d_q, d_off, max_len, *, eps, max_offset, k, min_votes, min_score, d_exclude_ids=None):
            calls.append((form.stem, eps, max_offset, k, min_votes, min_score))
            return super().align(form, d_q, d_off, max_len, eps=eps, max_offset=max_offset, k=k, min_votes=min_votes,
                                 min_score=min_score, d_exclude_ids=d_exclude_ids)

    rows, queries = _small_table()
    shard = TolCorpus()
    rc = service.RankCorpus(shard, Recorder(Backend(live=shard), k=8, cap=64), xdev="cpu", tick_s=0.01)
    try:
        rc.upload(rows)
        dup, q = np.asarray(rows[1][1]), np.asarray(queries[0])
        near1 = service.check_near(tc.FORM_BOUNDED, EPS, MAX_OFFSET, 4, 1, 0)
        near2 = service.check_near(tc.FORM_BOUNDED, 2 * EPS, MAX_OFFSET, 4, 1, 0)
        asks = [(dup, 2, -1, service.ASK_EXACT, 0.0, None), (q, 0, -1, service.ASK_NEAR, 0.0, near2),
                (dup, 3, -1, service.ASK_TOPK, 0.0, None), (q, 0, -1, service.ASK_NEAR, 0.0, near1),
                (dup, 2, -1, service.ASK_TOPK, 0.5, None)]
        busy = rc.busy_ticks
        answers = rc._ask_all(asks)
        assert rc.busy_ticks == busy + 1                                 # one tick held them all
        assert calls == [("match_topk", 2, {"tolerance": 0.5}), ("match_topk", 3, {}),
                         ("align_topk", EPS, MAX_OFFSET, 4, 1, 0), ("align_topk", 2 * EPS, MAX_OFFSET, 4, 1, 0)]
        assert answers[0] and answers[0][0][0] == rows[1][0]             # the exact ask found the row it copies
        assert answers[2][0][0][0] == rows[1][0] and rows[1][0] in answers[4][0][:, 0] and rc.broken is None
    finally:
        rc.close()


def test_a_rank_corpus_whose_matcher_cannot_align_refuses_in_the_caller(tmp_path):
    from tests.fakes import cut_inspector
    from tvidz_amd import db as tdb
    shard = OracleCorpus()
    rc = service.RankCorpus(shard, sharded.ShardedMatcher(OracleBackend(live=shard), k=4, cap=64), xdev="cpu")
    try:
        with pytest.raises(RuntimeError, match="no align_topk"):
            rc.align_topk([[1.0, 2.0]], eps=EPS, max_offset=MAX_OFFSET, k=4)
        assert rc.find_duplicates([1.0], 1) == [] and rc.broken is None
    finally:
        rc.close()
    # the driver takes near_top_k over a rank corpus that can, and reports a cut-shifted copy at world size 1
    shard = OracleCorpus()
    rc = service.RankCorpus(shard, sharded.ShardedMatcher(NearBackend(live=shard), k=4, cap=64), xdev="cpu")
    store = tdb.Store(f"sqlite:///{tmp_path}/t.db", corpus=rc, census=False)
    from tests.fakes import CutReader
    cuts = {"a.y4m": [1.0, 2.5, 4.0, 7.3, 9.9, 12.0], "b.y4m": [x + 7 / 30 for x in [1.0, 2.5, 4.0, 7.3, 9.9, 12.0]]}
    ins = cut_inspector(store, device="cuda:0", near_duplicates=True, near_top_k=4,
                        frame_source=lambda bucket, key, filename, uid: (CutReader(cuts[key], frames=600), None))
    try:
        res = [ins.analyze_file("videos", k) for k in ("a.y4m", "b.y4m")]
        assert all(r["status"] == "done" for r in res), res
        assert res[0]["near_duplicates"] == [] and [d["filename"] for d in res[1]["near_duplicates"]] == ["a.y4m"]
        assert res[1]["near_duplicates"][0]["jaccard"] == 1.0
    finally:
        store.close()
        rc.close()


# ---- sizing-function invariants (no GPU: the functions only compute) -----------------------------------------------
def test_sharded_workspace_size_invariants():
    grid = [(Q, L, k, n) for Q in (0, 1, 2, 7, 64) for L in (0, 1, 40, 4095) for k in (1, 2, 16, 64) for n in (0, 1, 2, 8, 16)]
    for Q, L, k, n in grid:
        size = tc.align_topk_sharded_workspace_bytes(Q, L, 0, k, n)
        plain = tc.align_topk_workspace_bytes(Q, L, 0, k)
        blocks = (1 + max(n, 1)) * Q * (k + 1) * 16
        assert plain + blocks <= size <= plain + blocks + 2 * 256, (Q, L, k, n)
        assert tc.align_topk_sharded_workspace_bytes(Q + 1, L, 0, k, n) >= size
        assert tc.align_topk_sharded_workspace_bytes(Q, L + 1, 0, k, n) >= size
        assert k == 64 or tc.align_topk_sharded_workspace_bytes(Q, L, 0, k + 1, n) >= size
        assert tc.align_topk_sharded_workspace_bytes(Q, L, 0, k, n + 1) >= size
        assert tc.align_topk_sharded_workspace_bytes(Q, L, Q * L + 100, k, n) >= size
    assert tc.align_topk_sharded_workspace_bytes(1, 1, 0, 0, 1) == 0 and tc.align_topk_sharded_workspace_bytes(-1, 1, 0, 1, 1) == 0


def test_the_binding_knows_the_new_exports():
    from tvidz_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tvz.h")).read()
    for name in ("tvz_align_topk_merge", "tvz_align_topk_shards", "tvz_align_topk_sharded_workspace_bytes",
                 "tvz_align_topk_sharded"):
        assert name in _lib.SIGNATURES and f" {name}(" in text and hasattr(_lib.load(), name)
    assert _lib.VERSION == 404 and _lib.load().tvz_version() == 404


# ---- the launcher ---------------------------------------------------------------------------------------------------
def test_near_top_k_is_checked_before_any_child_starts(monkeypatch, tmp_path):
    started = []

    class FakePopen:
        def __init__(self, cmd, env=None):
            self.args = cmd
            started.append(cmd)

        def poll(self):
            return 0

    monkeypatch.setattr(subprocess, "Popen", FakePopen)
    monkeypatch.setattr(service.RankService, "_wait_ready", lambda self, timeout: None)
    url = f"sqlite:///{tmp_path}/t.db"
    kw = dict(base_port=5900, backend="gloo", parts="m:f", k=4, cap=64, workers=8, tick_s=0.002)
    for bad in (65, -1, 1000):
        with pytest.raises(ValueError, match="near_top_k"):
            service.RankService(2, url, near_top_k=bad, **kw)
    with pytest.raises(ValueError, match="bins"):
        service.RankService(2, url, near_top_k=4, near_eps=0.001, near_max_offset=30.0, **kw)
    with pytest.raises(ValueError, match="near_top_k"):
        service.main(["--ranks", "2", "--db", url, "--near-top-k", "65"])
    assert started == []
    off = service.RankService(2, url, **kw)
    assert not any(x.startswith("--near") for p in off.procs for x in p.args)          # without the flag: as before
    on = service.RankService(2, url, near_top_k=4, near_jaccard=0.5, **kw)
    for p in on.procs:
        assert p.args[-8:] == ["--near-top-k", "4", "--near-eps", repr(1.0 / 30), "--near-max-offset", "30.0",
                               "--near-jaccard", "0.5"]
    assert service.near_kwargs(type("A", (), {"near_top_k": 0})()) == {}


def test_two_rank_launch_reports_near_duplicates_through_the_front(tmp_path):
    """`--near-top-k 4` on two gloo ranks made of fakes: a cut-shifted copy of a library video that lives on the OTHER
    rank is reported in the upload's record, read through the front as tests/test_service_launch_cpu.py reads it."""
    import requests
    from werkzeug.serving import make_server
    _key, _notify, _wait_done = upload_key, notify, wait_done
    PORT = free_port_run(3)                                            # the front, then one port per rank
    cuts = [1.0, 2.5, 4.0, 7.3, 9.9, 12.0]
    shifted = [c + 0.2 for c in cuts]                                  # six bins of 1/30 s; no cut in common
    names, i = {}, 0
    while len(names) < 2:                                              # the original on rank 0, its copy on rank 1
        n, i = f"v{i}", i + 1
        c = cuts if not names else shifted
        if service.owner_rank(service.clean_name(_key(n, c)), 2) == len(names):
            names[n] = c
    (orig, _), (copy, _) = names.items()
    s = service.RankService(2, f"sqlite:///{tmp_path}/t.db", base_port=PORT, backend="gloo",
                            parts="tests.near_fakes:near_rank_parts", k=4, cap=64, workers=4, tick_s=0.002, ready_timeout=300,
                            near_top_k=4, env={"PYTHONPATH": os.path.dirname(os.path.dirname(os.path.abspath(__file__)))})
    srv = make_server("127.0.0.1", PORT, service.create_front(s.urls), threaded=True)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    base = f"http://127.0.0.1:{PORT}"
    try:
        recs = {}
        for n, c in names.items():
            key = _key(n, c)
            _notify(base, key)
            recs[n] = _wait_done(base, key.split("/")[-1])
            assert recs[n]["status"] == "done" and recs[n]["duplicates"] == [], recs[n]
        assert recs[orig]["near_duplicates"] == []
        near = recs[copy]["near_duplicates"]
        assert [d["filename"] for d in near] == [service.clean_name(_key(orig, cuts))] and near[0]["jaccard"] == 1.0
        assert abs(near[0]["shift_seconds"] + 0.2) < 1e-9 or abs(near[0]["shift_seconds"] - 0.2) < 1e-9
        info = requests.get(f"{base}/ranks", timeout=10).json()["ranks"]
        assert all(r["broken"] is None for r in info) and [r["rows"] for r in info] == [1, 1] and s.dead() == []
    finally:
        srv.shutdown()
        s.stop()
