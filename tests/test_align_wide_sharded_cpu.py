"""The near-duplicate search at any shift over a sharded table without a GPU.  The reference merge
(tests/align_wide_shard_ref.py) of per-shard blocks equals the restatement of tvz_align_wide_topk on the WHOLE table,
for both score kinds; over gloo at world sizes 2 and 3, with the numpy backend of tests/near_fakes.py,
sharded.ShardedMatcher.align_wide_topk is identical on every rank and equal to it, and a service.RankCorpus tick that
carries wide near asks of both score kinds, a bounded near ask, a top-k ask and an exact ask answers each as it would
alone; what the library would refuse is refused in the caller; the launcher passes --near-any-offset, --near-score and
--near-min-votes on and rejects them without --near-top-k."""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import align_topk_ref as atr, align_wide_ref as awr, align_wide_shard_ref as wsr
from tests.fakes import OracleCorpus
from tests.near_fakes import NearBackend, free_port_run
from tvidz_amd import corpus as tc, service, sharded

EPS = wsr.EPS
WIDEST = awr.MAX_B * EPS
NAN = float("nan")


# ---- the reference merge against the whole table ---------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    rows, queries = wsr.split_table()
    queries = queries + [[float(i) for i in range(50)]]              # over-long at max_query_len = 45
    return rows, queries, wsr.aligned_whole(rows, queries)


@pytest.mark.parametrize("contain", [False, True])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_reference_merge_of_shard_blocks_equals_the_whole_table(table, contain, k):
    rows, queries, aligned = table
    kw = dict(min_votes=2, contain=contain, max_query_len=45)
    whole = awr.topk_wide_ref(rows, queries, EPS, WIDEST, k, aligned=aligned, **kw)
    assert whole[0, 0, 0] >= 0 and whole[-1, k, 1] == atr.REFUSED and whole[3, k, 1] == 0
    for R in (1, 2, 3, 8):
        blocks = np.stack([awr.topk_wide_ref(rows[r::R], queries, EPS, WIDEST, k, aligned=[a[r::R] for a in aligned], **kw)
                           for r in range(R)])
        got_rows, got_totals = wsr.merge_ref(blocks, queries, contain)
        assert (got_rows == whole[:, :k]).all() and (got_totals == whole[:, k, 1]).all(), (R, k, contain)


def test_the_table_holds_what_the_wide_search_is_for(table):
    """Copies beyond the bounded search's 2,047 bins at both signs, and a query the two score kinds order differently."""
    rows, queries, aligned = table
    jac = awr.topk_wide_ref(rows, queries, EPS, WIDEST, 8, min_votes=2, aligned=aligned, max_query_len=45)
    con = awr.topk_wide_ref(rows, queries, EPS, WIDEST, 8, min_votes=2, contain=True, aligned=aligned, max_query_len=45)
    bins = jac[0, :8, 2]
    assert (np.abs(bins) > 2047).all() and (bins < 0).any() and (bins > 0).any()
    assert (jac[1, :8] != con[1, :8]).any() and sorted(jac[1, :4, 0].tolist()) != sorted(con[1, :4, 0].tolist())


# ---- gloo --------------------------------------------------------------------------------------------------------
def _small_table():
    rows, queries = wsr.split_table()
    return rows[:60], queries + [[float(i) for i in range(50)]]      # bases, 20 shifted copies, 12 excerpts


def _expected(rows, queries, k, **kw):
    block = awr.topk_wide_ref(rows, queries, EPS, kw.pop("max_offset", WIDEST), k, max_query_len=45, **kw)
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


def _matcher_worker(rank, world, port, out):
    _init(rank, world, port)
    try:
        rows, queries = _small_table()
        sm = sharded.ShardedMatcher(NearBackend(*tc.rows_to_csr(rows[rank::world])), k=16, cap=64)
        assert sm.world == world and sm.supports_align_wide and sm.supports_align_topk
        d_q, d_off = _pack(queries)
        excl = [rows[1][0]] + [-1] * (len(queries) - 1)
        cases = [(k, dict(contain=c)) for k in (1, 5, 64) for c in (False, True)]
        cases += [(5, dict(min_votes=2, min_score=atr.ONE // 4, exclude_ids=excl, contain=True)), (5, dict(max_offset=80.0))]
        for k, kw in cases:
            mkw = dict(kw)
            if "exclude_ids" in mkw:
                mkw["d_exclude_ids"] = torch.tensor(mkw.pop("exclude_ids"), dtype=torch.int32)
            got_rows, got_totals = sm.align_wide_topk(d_q, d_off, 45, eps=EPS, k=k, **mkw)
            exp_rows, exp_totals = _expected(rows, queries, k, **kw)
            assert got_rows.dtype == torch.int32 and tuple(got_rows.shape) == (len(queries), k, 4)
            assert (got_rows.numpy() == exp_rows).all() and (got_totals.numpy() == exp_totals).all(), (rank, k, kw)
            everyone = [None] * world
            dist.all_gather_object(everyone, (got_rows.tolist(), got_totals.tolist()))
            assert all(e == everyone[0] for e in everyone)                       # identical on every rank
        assert exp_totals[-1] == atr.REFUSED and np.abs(_expected(rows, queries, 5)[0][0, :, 2]).min() > 2047
        # a backend with the bounded pair only is refused by name
        plain = sharded.ShardedMatcher(NearBackend(*tc.rows_to_csr(rows[rank::world]), align_forms=(tc.FORM_BOUNDED,)),
                                       k=4, cap=64)
        assert plain.supports_align_wide is False and plain.supports_align_topk is True
        with pytest.raises(RuntimeError, match=f"NearBackend has no {tc.FORM_WIDE.stem}"):
            plain.align_wide_topk(d_q, d_off, 45, eps=EPS, k=4)
        out.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        out.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_matcher_align_wide_topk_equals_the_whole_table(world):
    _run(_matcher_worker, world)


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
        assert rc.supports_align_wide
        rc.upload(rows)                                               # video_id mod world
        dist.barrier()
        # (1) the public call, alone: the whole table's answer for both score kinds, the over-long query refused
        #     without travelling
        k = 5
        for contain in (False, True):
            exp_rows, exp_totals = _expected(rows, queries, k, contain=contain)
            got_rows, got_totals = rc.align_wide_topk(queries, eps=EPS, k=k, contain=contain, max_query_len=45)
            assert got_rows.dtype == np.int32 and got_rows.shape == (len(queries), k, 4)
            assert (got_rows == exp_rows).all() and (got_totals == exp_totals).all() and got_totals[-1] == tc.ALIGN_REFUSED
        dist.barrier()                                                # every rank's asks are answered: nobody asks again
        calls = list(backend.wide_calls)                              # before everybody has looked
        dist.barrier()
        assert all(c[0] <= world * (len(queries) - 1) for c in calls)                 # it never reached a matcher
        assert all(c[2] == tc.ALIGN_WIDE_MAX_B * EPS for c in calls), calls          # max_offset=None: the widest
        excl = [rows[1][0]] + [-1] * (len(queries) - 1)
        kw = dict(min_votes=2, min_score=atr.ONE // 4, exclude_ids=excl, contain=True)
        got = rc.align_wide_topk(queries, eps=EPS, max_offset=4000.0, k=k, max_query_len=45, **kw)
        exp = _expected(rows, queries, k, max_offset=4000.0, **kw)
        assert (got[0] == exp[0]).all() and (got[1] == exp[1]).all()
        # (2) one tick's worth of asks of every kind, pending at once on every rank: wide near asks of both score kinds,
        #     a bounded near ask, a top-k ask and an exact ask - each answered as it is alone
        qa, qb = np.asarray(queries[rank % 2]), np.asarray(queries[1])
        wide_j = service.check_near(tc.FORM_WIDE, EPS, None, 4, 1, 0, False)
        wide_c = service.check_near(tc.FORM_WIDE, EPS, None, 4, 1, 0, True)
        near = service.check_near(tc.FORM_BOUNDED, EPS, 3.0, 4, 1, 0)
        dup = np.asarray(rows[1][1])
        asks = [(qa, 0, -1, service.ASK_NEAR_WIDE, 0.0, wide_j), (dup, 2, -1, service.ASK_TOPK, 0.0, None),
                (qb, 0, rows[4][0], service.ASK_NEAR_WIDE, 0.0, wide_c), (dup, 2, -1, service.ASK_EXACT, 0.0, None),
                (qa, 0, -1, service.ASK_NEAR, 0.0, near), (qb, 0, -1, service.ASK_NEAR_WIDE, 0.0, wide_j),
                (qa, 0, -1, service.ASK_NEAR_WIDE, 0.0, wide_c)]
        alone = [rc._ask_all([a])[0] for a in asks]
        dist.barrier()
        n0, m0 = len(backend.wide_calls), len(backend.near_calls)
        together = rc._ask_all(asks)
        dist.barrier()
        for a, (x, y) in zip(asks, zip(alone, together)):
            if a[3] == service.ASK_EXACT:
                assert x == y and len(x) >= 1
            else:
                assert (x[0] == y[0]).all() and x[1] == y[1]
        for i, contain, ex in ((0, False, None), (2, True, [rows[4][0]]), (5, False, None), (6, True, None)):
            block = awr.topk_wide_ref(rows, [asks[i][0].tolist()], EPS, WIDEST, 4, contain=contain, exclude_ids=ex)
            assert (together[i][0] == block[0, :4]).all() and together[i][1] == block[0, 4, 1], i
        block = atr.topk_ref(rows, [qa.tolist()], EPS, 3.0, 4)
        assert (together[4][0] == block[0, :4]).all() and together[4][1] == block[0, 4, 1]
        assert together[1][1] >= 1 and together[1][0][0][0] == rows[1][0]       # the top-k ask found the row it copies
        # every rank answered ALL wide asks of all ranks, never mixing the two score kinds in one batch
        calls = backend.wide_calls[n0:]
        assert {c[6] for c in calls} == {False, True} and all(c[3] == 4 for c in calls)
        assert sum(c[0] for c in calls if c[6]) == 2 * world and sum(c[0] for c in calls if not c[6]) == 2 * world
        assert sum(c[0] for c in backend.near_calls[m0:]) == world
        # (3) refused in the caller, before the tick: nothing reaches a matcher, the loop keeps running
        n1, ticks = len(backend.wide_calls), rc.busy_ticks
        if rank == 0:
            too_wide = (tc.ALIGN_WIDE_MAX_B + 1) * EPS
            for bad in (dict(eps=0.0), dict(eps=NAN), dict(max_offset=-1.0), dict(max_offset=too_wide),
                        dict(max_offset=float("inf")), dict(max_offset=NAN), dict(k=0), dict(k=65), dict(min_votes=0),
                        dict(min_score=-1), dict(min_score=atr.ONE + 1), dict(exclude_ids=[1, 2])):
                with pytest.raises(ValueError):
                    rc.align_wide_topk([queries[0]], **{**dict(eps=EPS, k=4), **bad})
            long_rows, long_totals = rc.align_wide_topk([[0.5] * 4096], eps=EPS, k=4)
            assert long_totals.tolist() == [tc.ALIGN_REFUSED] and (long_rows[:, :, 0] == -1).all()
            assert len(backend.wide_calls) == n1 and rc.busy_ticks == ticks
        dist.barrier()
        got = rc.align_wide_topk([queries[1]], eps=EPS, max_offset=tc.ALIGN_WIDE_MAX_B * EPS, k=k)   # the limit itself
        assert (got[0][0] == _expected(rows, queries, k)[0][1]).all() and rc.broken is None
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
def test_rank_corpus_answers_wide_near_and_every_other_ask_of_one_tick(world):
    _run(_rank_worker, world)


def test_one_tick_calls_align_wide_topk_after_align_topk_in_sorted_order():
    """World size 1: the matcher hears align_topk per set of near parameters and THEN align_wide_topk per (the five
    parameters, flags) in sorted order, whatever order the asks came in: every rank makes its collective calls so."""
    calls = []

    class Recorder(sharded.ShardedMatcher):
        def align(self, form, d_q, d_off, max_len, **kw):
            if form == tc.FORM_BOUNDED:
                calls.append((form.stem, kw["eps"], kw["k"]))
            else:
                calls.append((form.stem, kw["eps"], kw["max_offset"], kw["k"], kw["min_votes"], kw["contain"]))
            return super().align(form, d_q, d_off, max_len, **kw)

    rows, queries = _small_table()
    shard = OracleCorpus()
    rc = service.RankCorpus(shard, Recorder(NearBackend(live=shard), k=8, cap=64), xdev="cpu", tick_s=0.01)
    try:
        rc.upload(rows)
        q = np.asarray(queries[0])
        c2 = service.check_near(tc.FORM_WIDE, EPS, None, 4, 2, 0, True)
        j2 = service.check_near(tc.FORM_WIDE, EPS, None, 4, 2, 0, False)
        j1 = service.check_near(tc.FORM_WIDE, EPS, 100.0, 4, 1, 0, False)
        near = service.check_near(tc.FORM_BOUNDED, EPS, 3.0, 4, 1, 0)
        assert c2[:5] == j2[:5] and (c2[5], j2[5]) == (tc.ALIGN_CONTAIN, 0)
        asks = [(q, 0, -1, service.ASK_NEAR_WIDE, 0.0, c2), (q, 0, -1, service.ASK_NEAR, 0.0, near),
                (q, 0, -1, service.ASK_NEAR_WIDE, 0.0, j1), (q, 0, -1, service.ASK_NEAR_WIDE, 0.0, j2),
                (q, 0, -1, service.ASK_NEAR_WIDE, 0.0, c2)]
        busy = rc.busy_ticks
        answers = rc._ask_all(asks)
        assert rc.busy_ticks == busy + 1                                 # one tick held them all
        assert calls == [("align_topk", EPS, 4), ("align_wide_topk", EPS, 100.0, 4, 1, False),
                         ("align_wide_topk", EPS, WIDEST, 4, 2, False), ("align_wide_topk", EPS, WIDEST, 4, 2, True)]
        assert (answers[0][0] == answers[4][0]).all() and abs(int(answers[3][0][0][2])) > 2047 and rc.broken is None
    finally:
        rc.close()


def test_a_rank_corpus_whose_matcher_has_no_wide_form_refuses_in_the_caller(tmp_path):
    from tests.fakes import CutReader, cut_inspector
    from tvidz_amd import db as tdb
    shard = OracleCorpus()
    rc = service.RankCorpus(shard, sharded.ShardedMatcher(NearBackend(live=shard, align_forms=(tc.FORM_BOUNDED,)), k=4, cap=64),
                            xdev="cpu")
    try:
        assert rc.supports_align_wide is False
        with pytest.raises(RuntimeError, match="no align_wide_topk"):
            rc.align_wide_topk([[1.0, 2.0]], eps=EPS, k=4)
        rows, totals = rc.align_topk([[1.0, 2.0]], eps=EPS, max_offset=3.0, k=4)      # the bounded search is still there
        assert totals.tolist() == [0] and rc.broken is None
    finally:
        rc.close()
    # the driver takes near_any_offset over a rank corpus that can, and reports the excerpt of a longer upload whose
    # cuts moved by minutes, which neither the bounded search nor the Jaccard finds
    shard = OracleCorpus()
    rc = service.RankCorpus(shard, sharded.ShardedMatcher(NearBackend(live=shard), k=4, cap=64), xdev="cpu")
    store = tdb.Store(f"sqlite:///{tmp_path}/t.db", corpus=rc, census=False)
    film = [100.0 + 7.0 * i + 0.05 * i * i for i in range(40)]                       # no two gaps alike: one shift aligns
    cuts = {"film.y4m": film, "clip.y4m": [c - 150.0 for c in film[12:32]]}          # 4,500 bins of 1/30 s
    ins = cut_inspector(store, device="cuda:0", near_duplicates=True, near_top_k=4, near_any_offset=True,
                        near_score="containment", near_min_votes=5,
                        frame_source=lambda bucket, key, filename, uid: (CutReader(cuts[key], frames=12000), None))
    try:
        res = [ins.analyze_file("videos", k) for k in ("film.y4m", "clip.y4m")]
        assert all(r["status"] == "done" for r in res), res
        assert res[0]["near_duplicates"] == [] and [d["filename"] for d in res[1]["near_duplicates"]] == ["film.y4m"]
        near = res[1]["near_duplicates"][0]
        assert near["containment"] == 1.0 and near["jaccard"] == 0.5 and abs(near["shift_seconds"] - 150.0) < 1 / 30
    finally:
        store.close()
        rc.close()


# ---- sizing and binding (no GPU: the functions only compute) --------------------------------------------------------
def test_the_wide_sharded_sizing_function_is_monotone():
    for Q, L, k, n in [(Q, L, k, n) for Q in (0, 1, 7, 64) for L in (0, 1, 40, 4095) for k in (1, 16, 64) for n in (0, 1, 8, 16)]:
        size = tc.align_wide_topk_sharded_workspace_bytes(Q, L, 0, k, n)
        assert size >= tc.align_wide_topk_workspace_bytes(Q, L, 0, k) + (1 + max(n, 1)) * Q * (k + 1) * 16
        assert size >= tc.align_topk_sharded_workspace_bytes(Q, L, 0, k, n)          # 20 bytes per kept hit, not 16
        assert tc.align_wide_topk_sharded_workspace_bytes(Q + 1, L, 0, k, n) >= size
        assert tc.align_wide_topk_sharded_workspace_bytes(Q, L, 0, k, n + 1) >= size
        assert tc.align_wide_topk_sharded_workspace_bytes(Q, L, Q * L + 100, k, n) >= size
    assert tc.align_wide_topk_sharded_workspace_bytes(1, 1, 0, 0, 1) == 0
    assert tc.align_wide_topk_sharded_workspace_bytes(-1, 1, 0, 1, 1) == 0


# ---- the launcher ---------------------------------------------------------------------------------------------------
def test_the_launcher_passes_the_wide_switches_on_and_needs_near_top_k(monkeypatch, tmp_path):
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
    for bad in (dict(near_any_offset=True), dict(near_score="containment", near_any_offset=True), dict(near_min_votes=3)):
        with pytest.raises(ValueError, match="needs --near-top-k"):
            service.RankService(2, url, **bad, **kw)
    with pytest.raises(ValueError, match="needs --near-any-offset"):
        service.RankService(2, url, near_top_k=4, near_score="containment", **kw)
    with pytest.raises(ValueError, match="near_score"):
        service.RankService(2, url, near_top_k=4, near_any_offset=True, near_score="cosine", **kw)
    with pytest.raises(ValueError, match="near_min_votes"):
        service.RankService(2, url, near_top_k=4, near_min_votes=0, **kw)
    for argv in (["--near-any-offset"], ["--near-min-votes", "2"], ["--near-any-offset", "--near-score", "containment"]):
        with pytest.raises(ValueError, match="needs --near-top-k"):
            service.main(["--ranks", "2", "--db", url] + argv)
    assert started == []
    plain = service.RankService(2, url, near_top_k=4, **kw)                         # the three at their defaults: as before
    assert all(p.args[-2:] == ["--near-jaccard", "0.8"] for p in plain.procs)
    on = service.RankService(2, url, near_top_k=4, near_any_offset=True, near_score="containment", near_min_votes=5, **kw)
    for p in on.procs:
        assert p.args[-5:] == ["--near-any-offset", "--near-score", "containment", "--near-min-votes", "5"]
        assert p.args[-13:-11] == ["--near-top-k", "4"]
    # ... and a rank process hands them to its driver
    A = type("A", (), dict(near_top_k=4, near_eps=EPS, near_max_offset=30.0, near_jaccard=0.8, near_any_offset=True,
                           near_score="containment", near_min_votes=5))
    got = service.near_kwargs(A())
    assert got["near_any_offset"] is True and got["near_score"] == "containment" and got["near_min_votes"] == 5
    B = type("B", (), dict(near_top_k=4, near_eps=EPS, near_max_offset=30.0, near_jaccard=0.8))
    assert set(service.near_kwargs(B())) == {"near_duplicates", "near_top_k", "near_eps", "near_max_offset", "near_jaccard"}
    assert service.near_kwargs(type("C", (), {"near_top_k": 0, "near_any_offset": True})()) == {}
