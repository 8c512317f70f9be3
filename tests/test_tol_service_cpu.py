"""The tolerant match through the N-rank service at world size 2 on gloo (CPU): service.RankCorpus over the tolerant
stand-ins of tests/tol_fakes.py (tests/fakes.py's oracle shard and backend + the restatement tests/tol_ref.py).
Checked against tol_ref on the WHOLE table: exact and tolerant asks of both ranks in the same ticks, two tolerances
and two min_match at once, a tie set beyond k (the exact round, WITH its tolerance), db.find_duplicates' shape; a
corpus that cannot match tolerantly refuses in the caller and strands nobody; the Inspector accepts a RankCorpus that
can; the launcher's --match-tolerance reaches the driver of every rank and changes nothing at 0."""
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest
import requests
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import tol_ref
from tests.fakes import OracleBackend, OracleCorpus
from tests.tol_fakes import TolBackend, TolCorpus
from tvidz_amd import service, sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(n=60, seed=9):
    """Rows of cut times on a 30 fps grid as a 1/90000 container prints them (ids 1..n)."""
    rng = np.random.default_rng(seed)
    rows = []
    for v in range(n):
        fr = np.sort(rng.choice(np.arange(1, 9000), size=int(rng.integers(6, 40)), replace=False))
        rows.append((v + 1, [tol_ref.pts_time(int(f) * 3000, 1, 90000) for f in fr]))
    return rows


def _remux(ts):
    """The same cuts as a container with time base 1/1000 prints them (<= 0.34 ms away)."""
    return [tol_ref.pts_time(int(round(t * 1000)), 1, 1000) for t in ts]


def _check_with_kth(got, exp, k):
    top = sorted(exp, key=lambda h: (h[2], h[0], h[1]))
    assert sorted(got) == sorted(top[:len(got)]) and (len(got) == len(exp) or len(got) >= k), (got, exp)
    kstar = min((h[2] for h in exp), default=None)
    assert sorted(h[0] for h in got if h[2] == kstar) == sorted(h[0] for h in exp if h[2] == kstar), (got, exp)
    assert set(got) <= set(exp)


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _worker(rank, world, port, out):
    _init(rank, world, port)
    rc = None
    try:
        table = _table()
        shard = TolCorpus()
        g = dist.new_group(backend="gloo")          # the tick thread's own group (tests/test_service_cpu.py)
        backend = TolBackend(live=shard)
        matcher = sharded.ShardedMatcher(backend, k=8, cap=64, group=g)
        assert matcher.supports_tolerance
        rc = service.RankCorpus(shard, matcher, group=g, xdev="cpu", tick_s=0.02)
        assert rc.supports_tolerance
        rc.upload(table)
        dist.barrier()
        # (1) exact and tolerant asks from twelve threads per rank, started together: two tolerances (and 0) and two
        #     min_match share ticks; every ask gets the whole-table answer of ITS tolerance
        rng = np.random.default_rng(3 + rank)
        asks = []
        for i in range(12):
            v = int(rng.integers(0, len(table)))
            q = _remux(table[v][1]) if i % 4 else list(table[v][1])
            asks.append((q, (2, 1)[i % 2], table[(v + 1) % len(table)][0] if i % 3 == 0 else -1, (0.0, 0.001, 0.02)[i % 3]))
        errs = []
        ticks0 = rc.busy_ticks

        def ask(i):
            try:
                q, mm, excl, tol = asks[i]
                exp = tol_ref.find_duplicates_tol(table, q, tol, mm, excl)
                _check_with_kth(rc.find_duplicates(q, mm, exclude_id=excl, with_kth=True, tolerance=tol), exp, 8)
            except Exception as e:                                        # pragma: no cover
                errs.append(repr(e))
        th = [threading.Thread(target=ask, args=(i,)) for i in range(12)]
        [t.start() for t in th]
        [t.join(120) for t in th]
        assert not errs, errs[:2]
        dist.barrier()
        seen = {(mm, tol) for _, mm, tol in backend.tolerant_calls}
        assert seen == {(1, 0.001), (2, 0.001), (1, 0.02), (2, 0.02)}, seen     # batched per (min_match, tolerance)
        assert any(Q > 1 for Q, _, _ in backend.tolerant_calls)                  # ... and asks did share a batch
        assert rc.busy_ticks - ticks0 < 24                                       # 24 asks of two ranks in fewer ticks
        # the remux of a row is found with a tolerance only (the row's own cuts are off the millisecond grid)
        v = 5
        q = [b for a, b in zip(table[v][1], _remux(table[v][1])) if a != b]    # (cut frames not divisible by 3)
        assert len(q) >= 2
        assert not any(h[0] == table[v][0] for h in rc.find_duplicates(q, 2, with_kth=True))
        got = rc.find_duplicates(q, 2, with_kth=True, tolerance=0.001)
        assert (table[v][0], len(q), 1) in got
        dist.barrier()
        # (2) a tie set beyond k at a tolerance: 24 shifted copies over both ranks share kth 1 with k = 8 -> the exact
        #     round, with the ask's tolerance (at 0 it would find the five unshifted ones only)
        copy_ts = [8000.25 + i for i in range(6)]
        for j in range(12):
            vid = 20000 + 2 * j + rank
            rc.upsert(vid, [t + 0.0001 * (vid % 5) for t in copy_ts])
        dist.barrier()
        full = table + [(20000 + i, [t + 0.0001 * (i % 5) for t in copy_ts]) for i in range(24)]
        before = rc.exact_asks
        got = rc.find_duplicates(copy_ts, 2, exclude_id=20000 + rank, with_kth=True, tolerance=0.001)
        exp = tol_ref.find_duplicates_tol(full, copy_ts, 0.001, 2, 20000 + rank)
        assert len(exp) == 23 and got == exp and all(h[2] == 1 for h in got), (rank, got, exp)
        assert rc.exact_asks == before + 1
        assert len(rc.find_duplicates(copy_ts, 2, exclude_id=20000 + rank, with_kth=True)) == 4 + (rank != 0)
        # (3) db.find_duplicates' shape (every row with its count) beyond k; min_match outside 1..5 and a query of
        #     more than 4,095 timestamps: the exact round, with the tolerance
        pairs = rc.find_duplicates(copy_ts, 2, tolerance=0.001)
        assert pairs == [(v_, c) for v_, c, _ in tol_ref.find_duplicates_tol(full, copy_ts, 0.001, 2)] and len(pairs) == 24
        small = rc.find_duplicates(q, 2, tolerance=0.001)                      # fits k: read off the top-k
        assert small == [(v_, c) for v_, c, _ in tol_ref.find_duplicates_tol(full, q, 0.001, 2)] and small
        got = rc.find_duplicates(copy_ts, 6, with_kth=True, tolerance=0.001)
        assert got == tol_ref.find_duplicates_tol(full, copy_ts, 0.001, 6) and len(got) == 24
        longq = [-1.0 - i for i in range(4200)] + [t + 0.0003 for t in copy_ts]
        got = rc.find_duplicates(longq, 2, with_kth=True, tolerance=0.001)
        assert got == tol_ref.find_duplicates_tol(full, longq, 0.001, 2, form="sorted") and len(got) == 24
        assert rc.find_duplicates([], 2, with_kth=True, tolerance=0.001) == []
        for bad in (float("nan"), float("inf"), -0.001):
            with pytest.raises(ValueError):
                rc.find_duplicates(copy_ts, 2, tolerance=bad)
        dist.barrier()
        assert rc.broken is None
        out.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        out.put((rank, repr(e)))
        raise
    finally:
        if rc is not None:
            rc.close()
        dist.destroy_process_group()


def _run_world2(target, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    [p.join(300) for p in procs]
    assert all(not p.is_alive() for p in procs), "a rank hung"
    res = sorted(q.get(timeout=5) for _ in range(2))
    assert res == [(0, "ok"), (1, "ok")], res
    assert all(p.exitcode == 0 for p in procs)


def test_tolerant_and_exact_asks_share_the_tick_exchange_world2():
    _run_world2(_worker, 29800 + os.getpid() % 40)


def _refusing_worker(rank, world, port, out):
    _init(rank, world, port)
    try:
        rows = [(10 + i, [float(i), float(i) + 0.5, 100.25]) for i in range(8)]
        for shard, backend in ((OracleCorpus(), TolBackend), (TolCorpus(), OracleBackend)):
            g = dist.new_group(backend="gloo")
            matcher = sharded.ShardedMatcher(backend(live=shard), k=4, cap=64, group=g)
            rc = service.RankCorpus(shard, matcher, group=g, xdev="cpu", tick_s=0.002)
            assert rc.supports_tolerance is False
            rc.upload(rows)
            dist.barrier()
            if rank == 0:
                # refused by name in the CALLING thread, before anything enters the exchange ...
                with pytest.raises(RuntimeError, match="no tolerant match"):
                    rc.find_duplicates([100.2504, 1.0], 1, with_kth=True, tolerance=0.001)
                with pytest.raises(RuntimeError, match="no tolerant match"):
                    rc.find_duplicates([100.2504, 1.0], 1, tolerance=0.001)
            # ... so the other rank's exact asks (and this rank's) keep being answered
            assert len(rc.find_duplicates([100.25, 1.0, 1.5], 1)) == 8
            assert rc.find_duplicates([3.0, 3.5], 2, with_kth=True) == [(13, 2, 1)]
            dist.barrier()
            assert rc.broken is None
            rc.close()                                                     # still collective, still returns
        # the matcher itself refuses too, should somebody reach it directly
        m = sharded.ShardedMatcher(OracleBackend(live=OracleCorpus()), k=4, cap=64, group=dist.new_group(backend="gloo"))
        assert m.supports_tolerance is False
        import torch
        with pytest.raises(RuntimeError, match="no tolerant match"):
            m.submit(torch.zeros(1, dtype=torch.float64), torch.tensor([0, 1]), 1, 1, None, tolerance=0.001)
        out.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        out.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_a_corpus_that_cannot_match_tolerantly_refuses_in_the_caller_and_strands_nobody():
    _run_world2(_refusing_worker, 29850 + os.getpid() % 40)


def test_inspector_takes_a_tolerance_over_a_rank_corpus_that_can(tmp_path):
    from tests.fakes import cut_inspector
    from tvidz_amd import db as tdb
    for shard, ok in ((TolCorpus(), True), (OracleCorpus(), False)):
        rc = service.RankCorpus(shard, sharded.ShardedMatcher(TolBackend(live=shard), k=4, cap=64), xdev="cpu")
        store = tdb.Store(f"sqlite:///{tmp_path}/t{int(ok)}.db", corpus=rc, census=False)
        try:
            if ok:
                ins = cut_inspector(store, device="cuda:0", match_tolerance=0.001)
                assert ins.match_tolerance == 0.001
                ins.close()
            else:
                with pytest.raises(RuntimeError, match="no tolerant match"):
                    cut_inspector(store, device="cuda:0", match_tolerance=0.001)
            cut_inspector(store, device="cuda:0").close()                  # the default asks for nothing
        finally:
            store.close()
            rc.close()


# ---- the launcher -------------------------------------------------------------------------------------------------
def test_the_child_command_line_changes_only_with_a_tolerance(monkeypatch, tmp_path):
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
    s = service.RankService(2, url, **kw)
    mp_ = s.procs[0].args[s.procs[0].args.index("--master-port") + 1]
    today = [[sys.executable, "-m", "tvidz_amd.service", "--child", "--rank", str(r), "--ranks", "2", "--master-port", mp_,
              "--http-port", str(5901 + r), "--db", url, "--backend", "gloo", "--device", str(r), "--k", "4", "--cap", "64",
              "--workers", "8", "--tick-s", "0.002", "--parent-pid", str(os.getpid()), "--parts", "m:f"] for r in range(2)]
    assert [p.args for p in s.procs] == today
    assert [p.args for p in service.RankService(2, url, match_tolerance=0.0, **kw).procs] != [] and "--match-tolerance" not in started[-1]
    s = service.RankService(2, url, match_tolerance=0.001, **kw)
    for r, p in enumerate(s.procs):
        mp2 = p.args[p.args.index("--master-port") + 1]
        assert p.args == [mp2 if x == mp_ else x for x in today[r]] + ["--match-tolerance", "0.001"]
    n = len(started)
    for bad in (float("nan"), float("inf"), -1.0):                         # Inspector's rule, before any rank starts
        with pytest.raises(ValueError, match="match_tolerance"):
            service.RankService(2, url, match_tolerance=bad, **kw)
    assert len(started) == n


PORT = 6100 + os.getpid() % 300


def _key(name, cuts, stamp=1700000000):
    return f"videos/{stamp}-{name}__{'_'.join(str(int(round(c * 1e6))) for c in cuts)}.mp4"


def _notify(base, key):
    r = requests.post(f"{base}/notify", json={"Records": [{"s3": {"bucket": {"name": "videos"}, "object": {"key": key}}}]},
                      timeout=30)
    assert r.status_code == 200 and r.json() == {"status": "Analysis started", "file": key}


def _wait_done(base, filename, timeout=60):
    deadline = time.time() + timeout
    while time.time() < deadline:
        rec = requests.get(f"{base}/status/{filename}", timeout=30).json()
        if rec.get("status") in ("done", "error"):
            return rec
        time.sleep(0.05)
    raise AssertionError(f"{filename} never finished")


def test_two_rank_service_with_a_match_tolerance_flags_a_remuxed_copy(tmp_path):
    s = service.RankService(2, f"sqlite:///{tmp_path}/t.db", base_port=PORT, backend="gloo",
                            parts="tests.tol_fakes:tol_rank_parts", k=4, cap=64, workers=8, tick_s=0.002, ready_timeout=300,
                            match_tolerance=0.001, env={"PYTHONPATH": ROOT})
    from werkzeug.serving import make_server
    srv = make_server("127.0.0.1", PORT, service.create_front(s.urls), threaded=True)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    base = f"http://127.0.0.1:{PORT}"
    try:
        assert all("--match-tolerance" in p.args for p in s.procs)
        # originals at 30 fps (cut frames not divisible by 3: 1.133333 against the remux's 1.133), on both ranks
        origs, per_rank, i = {}, [0, 0], 0
        while len(origs) < 4:
            frames = [f + 300 * len(origs) for f in (34, 91, 172, 241)]
            cuts = [float("%.6g" % (f / 30)) for f in frames]
            name, i = f"orig{len(origs)}v{i}", i + 1
            r = service.owner_rank(service.clean_name(_key(name, cuts)), 2)
            if per_rank[r] < 2:
                per_rank[r] += 1
                origs[name] = cuts
        for name, cuts in origs.items():
            key = _key(name, cuts)
            _notify(base, key)
            rec = _wait_done(base, key.split("/")[-1])
            assert rec["status"] == "done" and rec["scene_cuts"] == cuts and rec["duplicates"] == [], rec
        for name, cuts in origs.items():
            copy = _remux(cuts)
            assert all(a != b and abs(a - b) < 0.001 for a, b in zip(copy, cuts))
            key = _key(f"remux_of_{name}", copy, stamp=1700000100)
            _notify(base, key)
            rec = _wait_done(base, key.split("/")[-1])
            # flagged at its 2nd cut and truncated there, whichever rank holds the original
            assert rec["status"] == "done" and rec["scene_cuts"] == copy[:2], rec
            assert rec["duplicates"] == [service.clean_name(_key(name, cuts))], rec
        uniq = [5000.5, 5001.25, 5003.0]
        key = _key("unique", uniq, stamp=1700000200)
        _notify(base, key)
        rec = _wait_done(base, key.split("/")[-1])
        assert rec["status"] == "done" and rec["scene_cuts"] == uniq and rec["duplicates"] == [], rec
        info = requests.get(f"{base}/ranks", timeout=10).json()["ranks"]
        assert all(r["broken"] is None for r in info) and s.dead() == []
    finally:
        srv.shutdown()
        s.stop()


def test_create_schema_leaves_a_sqlite_file_in_wal_mode(tmp_path):
    """The launcher's parent switches the file to WAL once (db.create_schema): two rank processes issuing the switch
    at the same moment from Store's connect hook lost one of them to "database is locked" at start-up - about one
    start in four of the two-rank launches here.  On a file that is in WAL mode the ranks' pragma changes nothing."""
    import sqlite3
    from tvidz_amd import db as tdb
    path = tmp_path / "t.db"
    tdb.create_schema(f"sqlite:///{path}")
    con = sqlite3.connect(str(path))
    try:
        assert con.execute("PRAGMA journal_mode").fetchone()[0] == "wal"
        assert {"videos", "video_timestamps"} <= {r[0] for r in con.execute("select name from sqlite_master")}
    finally:
        con.close()
    tdb.create_schema("sqlite://")                                         # in memory: nothing to switch, no error
