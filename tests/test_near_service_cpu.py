"""The searches with rates and spans and the parts call through the rank service without a GPU: over gloo at world sizes
2 and 3, with the numpy backends of tests/near_service_fakes.py, service.RankCorpus.align_rates_topk, align_span_topk and
align_parts equal the restatements on the WHOLE table; one tick that holds every ask kind makes the same matcher calls in
the same order on every rank - ascending kind, sorted parameters, rate lists told apart, the parts asks last; what the
library would refuse is refused in the caller, an over-long query never travels, and the Inspector refuses a rank corpus
whose matcher lacks a form when it is built; the launcher passes --near-rates, --near-spans, --near-score local and
--near-parts on and refuses their bad combinations before any rank starts; the new sizing functions are monotone; the new
prototypes of include/tvz.h and the binding's table agree."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import align_parts_cases as cs, align_parts_ref as apr, align_rates_ref as arr, align_span_ref as asr
from tests.fakes import OracleCorpus
from tests.near_fakes import free_port_run
from tests.near_service_fakes import NearServiceBackend, RatedBackend
from tests.test_align_rates_cpu import _prototype
from tvidz_amd import _lib, build as tbuild, corpus as tc, service, sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tvz.h")
EPS = cs.EPS
WIDEST = tc.ALIGN_WIDE_MAX_B * EPS
L = 129
RATES = (1.0, 0.96)
NEW_EXPORTS = ("tvz_align_rates_topk_sharded_workspace_bytes", "tvz_align_rates_topk_sharded",
               "tvz_align_span_topk_sharded_workspace_bytes", "tvz_align_span_topk_sharded", "tvz_align_parts_merge",
               "tvz_align_parts_shards", "tvz_align_parts_sharded_workspace_bytes", "tvz_align_parts_sharded")


def _table():
    rows, uploads = cs.table(), cs.uploads()
    queries = [uploads[n] for n in ("inserted", "parts24", "fps_inserted", "special")] + [[float(i) for i in range(150)]]
    return rows, queries                                             # the last query is over-long at max_query_len = L


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


def _every_kind(rows, queries, rank=0):
    """asks of every kind, two parameter sets for the kinds with a rate list, in an order that depends on the rank"""
    qa, qb = np.asarray(queries[0]), np.asarray(queries[1])
    dup = np.asarray(rows[15][1])                                    # the film itself: an exact duplicate
    six = lambda form, k=4, min_votes=1, **kw: service.check_near(form, EPS, None, k, min_votes, 0, **kw)      # noqa: E731
    r1, r2, r3 = (service.check_near_rates(r) for r in ((1.0,), RATES, (0.96, 1.0)))
    ids = lambda *v: tuple(float(x) for x in v)                      # noqa: E731
    parts_a = service.check_near(tc.FORM_SPAN, EPS, None, 3, 1, 0) + r2 + (2,)
    parts_b = service.check_near(tc.FORM_SPAN, EPS, None, 3, 1, 0) + r1 + (4,)
    asks = [(qa, 0, -1, service.ASK_PARTS, 0.0, parts_a + ids(cs.FILM, cs.NINE_ROWS, -1)),
            (qa, 0, -1, service.ASK_NEAR_SPAN, 0.0, six(tc.FORM_SPAN, min_votes=4, local=True) + r2),
            (dup, 2, -1, service.ASK_TOPK, 0.0, None),
            (qb, 0, -1, service.ASK_NEAR_RATES, 0.0, six(tc.FORM_RATES) + r3),
            (qa, 0, -1, service.ASK_NEAR_WIDE, 0.0, six(tc.FORM_WIDE)),
            (qa, 0, cs.FILM, service.ASK_NEAR_RATES, 0.0, six(tc.FORM_RATES) + r2),
            (dup, 2, -1, service.ASK_EXACT, 0.0, None),
            (qb, 0, -1, service.ASK_PARTS, 0.0, parts_b + ids(cs.LONG700, cs.ABSENT, cs.SECOND_BETTER)),
            (qb, 0, -1, service.ASK_NEAR_SPAN, 0.0, six(tc.FORM_SPAN) + r1),
            (qa, 0, -1, service.ASK_NEAR, 0.0, service.check_near(tc.FORM_BOUNDED, EPS, 3.0, 4, 1, 0)),
            (qb, 0, -1, service.ASK_PARTS, 0.0, parts_a + ids(cs.EQUAL_ROWS, cs.FILM, cs.SPECIAL)),
            (qb, 0, -1, service.ASK_NEAR_RATES, 0.0, six(tc.FORM_RATES) + r2)]
    return asks[rank % len(asks):] + asks[:rank % len(asks)]


def _expected_of(ask, rows):
    """the whole-table reference's answer to one ask of a search with rates, with spans or of a parts call"""
    q, _, excl, kind, _, near = ask
    k, min_votes, flags, n = int(near[2]), int(near[3]), int(near[5]), int(near[6])
    rates, ex = tuple(near[7:7 + n]), None if excl < 0 else [excl]
    if kind == service.ASK_NEAR_RATES:
        block = arr.topk_rates_ref(rows, [q.tolist()], EPS, WIDEST, rates, k, min_votes, exclude_ids=ex)
    elif kind == service.ASK_NEAR_SPAN:
        block = asr.topk_span_ref(rows, [q.tolist()], EPS, WIDEST, rates, k, min_votes, local=bool(flags & tc.ALIGN_LOCAL),
                                  exclude_ids=ex)
    else:
        return apr.align_parts_ref(rows, [q.tolist()], [[int(v) for v in near[16:16 + k]]], EPS, WIDEST, rates, min_votes,
                                   int(near[15]))[0]
    return block[0, :k], block[0, k, 1]


def _rank_worker(rank, world, port, out):
    _init(rank, world, port)
    rc = None
    try:
        rows, queries = _table()
        shard = OracleCorpus()
        g = dist.new_group(backend="gloo")                            # the tick thread's own group
        backend = NearServiceBackend(live=shard)
        rc = service.RankCorpus(shard, sharded.ShardedMatcher(backend, k=8, cap=64, group=g), group=g, xdev="cpu", tick_s=0.01)
        assert rc.supports_align_wide and rc.supports_align_rates and rc.supports_align_span and rc.supports_align_parts
        rc.upload(rows)                                               # video_id mod world
        dist.barrier()
        # (1) the three public calls, alone: the whole table's answers, the over-long query refused without travelling
        k = 5
        excl = [cs.FILM] + [-1] * (len(queries) - 1)
        exp = arr.topk_rates_ref(rows, queries, EPS, WIDEST, RATES, k, contain=True, exclude_ids=excl, max_query_len=L)
        got_rows, got_totals = rc.align_rates_topk(queries, eps=EPS, rates=RATES, k=k, contain=True, exclude_ids=excl, max_query_len=L)
        assert got_rows.dtype == np.int32 and got_rows.shape == (len(queries), k, 5)
        assert (got_rows == exp[:, :k]).all() and (got_totals == exp[:, k, 1]).all() and got_totals[-1] == tc.ALIGN_REFUSED
        for kw in (dict(), dict(local=True, min_votes=4), dict(contain=True)):
            exp = asr.topk_span_ref(rows, queries, EPS, WIDEST, RATES, k, max_query_len=L, **kw)
            got_rows, got_totals = rc.align_span_topk(queries, eps=EPS, rates=RATES, k=k, max_query_len=L, **kw)
            assert got_rows.shape == (len(queries), k, 8) and (got_rows == exp[:, :k]).all() and (got_totals == exp[:, k, 1]).all(), kw
        ids = [list(cs.IDS)] * len(queries)
        exp = apr.align_parts_ref(rows, queries, ids, EPS, WIDEST, RATES, 1, 3, max_query_len=L)
        got = rc.align_parts(queries, ids, eps=EPS, rates=RATES, min_votes=1, max_parts=3, max_query_len=L)
        assert got.dtype == np.int32 and got.shape == exp.shape
        # every pair of a query that travelled is the whole table's answer (all rows of an id lie on one rank); the
        # over-long query's pairs read n_rows = 0 and m = 0, because no rank looked
        assert (got[:-1] == exp[:-1]).all()
        nine = cs.IDS.index(cs.NINE_ROWS)
        assert got[0, nine, 0].tolist() == [cs.NINE_ROWS, 0, 0, tc.ALIGN_REFUSED, 9, 129] and got[0, 0, 0, 3] == 2
        assert got[-1, :, 0].tolist() == [[v, 0, 0, tc.ALIGN_REFUSED if v >= 0 else 0, 0, 0] for v in cs.IDS]
        assert (got[-1, :, 1:] == 0).all() and (exp[-1, :, 0, 3] == np.where(np.asarray(cs.IDS) >= 0, tc.ALIGN_REFUSED, 0)).all()
        dist.barrier()                                                # every rank's asks are answered: nobody asks again
        calls = list(backend.calls)
        dist.barrier()
        assert all(c[1] <= world * (len(queries) - 1) for c in calls)                 # the over-long query never reached a matcher
        # (2) asks of every kind, pending at once on every rank in another order: each is answered as it is alone, and the
        #     matcher calls are the same, in the same order, on every rank
        asks = _every_kind(rows, queries, rank)
        alone = [rc._ask_all([a])[0] for a in asks]
        dist.barrier()
        together = rc._ask_all(asks)
        # (a rank's own asks may be answered before the tick's last calls are made: one more tick, which starts when that one
        # has ended everywhere, before the calls are compared)
        rc._ask(asks[0][0], 2, -1, service.ASK_TOPK)
        dist.barrier()
        for a, x, y in zip(asks, alone, together):
            if a[3] == service.ASK_EXACT:
                assert x == y and len(x) >= 1
            elif a[3] == service.ASK_PARTS:
                assert (x == y).all() and (y == _expected_of(a, rows)).all(), a[5]
            else:
                assert (x[0] == y[0]).all() and x[1] == y[1]
                if a[3] in (service.ASK_NEAR_RATES, service.ASK_NEAR_SPAN):
                    e_rows, e_total = _expected_of(a, rows)
                    assert (y[0] == e_rows).all() and y[1] == e_total, a[5]
        everyone = [None] * world
        dist.all_gather_object(everyone, list(backend.calls))          # every call since the start: the ticks are collective
        assert all(e == everyone[0] for e in everyone) and len(everyone[0]) >= 9 + 8
        assert {c[0] for c in everyone[0]} == {"align_topk", "align_wide_topk", "align_rates_topk", "align_span_topk", "align_parts"}
        # (3) refused in the caller, before the tick: nothing reaches a matcher, the loop keeps running
        n1, ticks = len(backend.calls), rc.busy_ticks
        if rank == 0:
            q = [queries[1]]
            for call in (lambda: rc.align_rates_topk(q, eps=EPS, rates=(), k=4),
                         lambda: rc.align_rates_topk(q, eps=EPS, rates=[1.0] * 9, k=4),
                         lambda: rc.align_rates_topk(q, eps=EPS, rates=(1.0, float("nan")), k=4),
                         lambda: rc.align_span_topk(q, eps=EPS, rates=(1.0, 0.0), k=4),
                         lambda: rc.align_span_topk(q, eps=EPS, rates=(float("inf"),), k=4),
                         lambda: rc.align_span_topk(q, eps=EPS, k=4, contain=True, local=True),
                         lambda: rc.align_span_topk(q, eps=EPS, k=65),
                         lambda: rc.align_span_topk(q, eps=EPS, k=4, min_votes=0),
                         lambda: rc.align_span_topk(q, eps=0.0, k=4),
                         lambda: rc.align_span_topk(q, eps=EPS, max_offset=(tc.ALIGN_WIDE_MAX_B + 1) * EPS, k=4),
                         lambda: rc.align_parts(q, [[1]], eps=EPS, min_votes=0, max_parts=2),
                         lambda: rc.align_parts(q, [[1]], eps=EPS, min_votes=1, max_parts=0),
                         lambda: rc.align_parts(q, [[1]], eps=EPS, min_votes=1, max_parts=5),
                         lambda: rc.align_parts(q, [[1] * 65], eps=EPS, min_votes=1, max_parts=2),
                         lambda: rc.align_parts(q, [[1], [2]], eps=EPS, min_votes=1, max_parts=2),
                         lambda: rc.align_parts(q, [[1 << 31]], eps=EPS, min_votes=1, max_parts=2),
                         lambda: rc.align_parts(q, [[1]], eps=EPS, rates=(), min_votes=1, max_parts=2),
                         lambda: rc.align_parts(q, [[1]], eps=EPS, max_offset=-1.0, min_votes=1, max_parts=2)):
                with pytest.raises(ValueError):
                    call()
            long_rows, long_totals = rc.align_span_topk([[0.5] * 4096], eps=EPS, k=4)
            assert long_totals.tolist() == [tc.ALIGN_REFUSED] and (long_rows[:, :, 0] == -1).all()
            assert len(backend.calls) == n1 and rc.busy_ticks == ticks
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


@pytest.mark.parametrize("world", [2, 3])
def test_rank_corpus_answers_rates_spans_and_parts_as_the_whole_table(world):
    _run(_rank_worker, world)


def test_one_tick_makes_its_calls_by_ascending_kind_then_sorted_parameters_the_parts_last():
    """World size 1: whatever order the asks came in, the matcher hears the searches by ascending kind, per kind by the
    sorted parameter tuples - the rate list is part of them: (1.0, 0.96) and (0.96, 1.0) are two calls - and then the
    parts calls; every rank reads the same headers, so every rank makes its collective calls so."""
    rows, queries = _table()
    shard = OracleCorpus()
    backend = NearServiceBackend(live=shard)
    rc = service.RankCorpus(shard, sharded.ShardedMatcher(backend, k=8, cap=64), xdev="cpu", tick_s=0.01)
    try:
        rc.upload(rows)
        asks = _every_kind(rows, queries, rank=5)
        busy = rc.busy_ticks
        rc._ask_all(asks)
        assert rc.busy_ticks == busy + 1                                 # one tick held them all
        got = [(what, n, par) for what, n, par in backend.calls]
        wide = (EPS, WIDEST, 4, 1, 0, False)
        assert got == [
            ("align_topk", 1, (EPS, 3.0, 4, 1, 0, False)),
            ("align_wide_topk", 1, (EPS, WIDEST, 4, 1, 0, False)),
            ("align_rates_topk", 1, wide + (False, (0.96, 1.0))),
            ("align_rates_topk", 2, wide + (False, (1.0, 0.96))),
            ("align_span_topk", 1, wide + (False, (1.0,))),
            ("align_span_topk", 1, (EPS, WIDEST, 4, 4, 0, False, True, (1.0, 0.96))),
            ("align_parts", 1, (EPS, WIDEST, 3, 1, (1.0,), 4)),
            ("align_parts", 2, (EPS, WIDEST, 3, 1, (1.0, 0.96), 2))], got
        assert rc.broken is None
    finally:
        rc.close()


def test_a_rank_corpus_whose_matcher_lacks_a_form_refuses_in_the_caller_and_the_inspector_when_it_is_built():
    from tvidz_amd import inspector as insp
    shard = OracleCorpus()
    two = sharded.ShardedMatcher(RatedBackend(live=shard, align_forms=(tc.FORM_BOUNDED, tc.FORM_WIDE)), k=4, cap=64)
    no_parts = sharded.ShardedMatcher(RatedBackend(live=shard), k=4, cap=64)
    assert two.supports_align_rates is False and two.supports_align_span is False and two.supports_align_parts is False
    assert no_parts.supports_align_rates and no_parts.supports_align_span and no_parts.supports_align_parts is False
    with pytest.raises(RuntimeError, match="RatedBackend has no align_parts"):
        no_parts.parts(None, None, 4, None, eps=EPS, min_votes=1, max_parts=2)
    base = dict(device="cuda:0", near_duplicates=True, near_top_k=4, near_any_offset=True)
    rc = service.RankCorpus(shard, two, xdev="cpu")
    try:
        assert rc.supports_align_wide and not rc.supports_align_rates and not rc.supports_align_span and not rc.supports_align_parts
        ticks = rc.busy_ticks
        with pytest.raises(RuntimeError, match="no align_rates_topk"):
            rc.align_rates_topk([[1.0, 2.0]], eps=EPS, rates=RATES, k=4)
        with pytest.raises(RuntimeError, match="no align_span_topk"):
            rc.align_span_topk([[1.0, 2.0]], eps=EPS, k=4)
        with pytest.raises(RuntimeError, match="no align_parts"):
            rc.align_parts([[1.0, 2.0]], [[1]], eps=EPS, min_votes=1, max_parts=2)
        assert rc.busy_ticks == ticks and rc.broken is None
        store = type("Store", (), {"corpus": rc})()
        insp.Inspector(store, **base)                                                # the wide search is there
        for kw, word in ((dict(near_rates=RATES), "align_rates_topk"), (dict(near_spans=True), "align_span_topk"),
                         (dict(near_score="local", near_min_votes=2), "align_span_topk")):
            with pytest.raises(RuntimeError, match=word):
                insp.Inspector(store, **base, **kw)
    finally:
        rc.close()
    rc = service.RankCorpus(shard, no_parts, xdev="cpu")
    try:
        store = type("Store", (), {"corpus": rc})()
        insp.Inspector(store, near_rates=RATES, near_score="local", near_min_votes=2, **base)
        with pytest.raises(RuntimeError, match="align_parts"):
            insp.Inspector(store, near_score="local", near_min_votes=2, near_parts=2, **base)
    finally:
        rc.close()
    rc = service.RankCorpus(shard, sharded.ShardedMatcher(RatedBackend(live=shard, align_forms=(tc.FORM_BOUNDED,)), k=4, cap=64),
                            xdev="cpu")
    try:
        with pytest.raises(RuntimeError, match="align_wide_topk"):
            insp.Inspector(type("Store", (), {"corpus": rc})(), **base)
    finally:
        rc.close()


def test_the_inspector_over_a_rank_corpus_reports_the_rate_the_clip_and_the_parts(tmp_path):
    """The three copies the service could not find: through Inspector._near over a one-rank RankCorpus on the stand-ins."""
    from tvidz_amd import inspector as insp
    rows, _ = _table()
    film400, compilation, clip, shift = asr.compilation_case()
    shard = OracleCorpus()
    rc = service.RankCorpus(shard, sharded.ShardedMatcher(NearServiceBackend(live=shard), k=8, cap=64), xdev="cpu")
    try:
        rc.upload(rows + [(500, film400)])
        store = type("Store", (), {"corpus": rc, "get_video_by_id": lambda self, vid: None})()
        base = dict(device="cuda:0", near_duplicates=True, near_top_k=8, near_any_offset=True)
        fast = [x * 24.0 / 25.0 + 12.3 for x in cs.film()]
        (fps,) = insp.Inspector(store, near_rates=(1.0, 25.0 / 24.0), **base)._near(424242, fast)
        assert fps["video_id"] == cs.FILM and fps["rate"] == 25.0 / 24.0 and fps["jaccard"] == 1.0
        assert insp.Inspector(store, **base)._near(424242, fast) == []
        local = dict(base, near_score="local", near_min_votes=8)
        (found,) = insp.Inspector(store, near_jaccard=0.5, **local)._near(424242, compilation)
        assert found["video_id"] == 500 and found["local"] == 1.0 and abs(found["shift_seconds"] - shift) <= EPS
        assert insp.Inspector(store, near_jaccard=0.5, **dict(local, near_score="containment"))._near(424242, compilation) == []
        (ins,) = insp.Inspector(store, near_jaccard=0.9, near_parts=2, **local)._near(424242, cs.uploads()["inserted"])
        assert ins["video_id"] == cs.FILM and [p["votes"] for p in ins["parts"]] == [60, 60] and ins["parts_score"] == 1.0
        assert [p["shift_seconds"] for p in ins["parts"]] == [0.0, -1419 * EPS] and rc.broken is None
    finally:
        rc.close()


# ---- sizing and binding (no GPU: the functions only compute) --------------------------------------------------------
def test_the_new_sizing_functions_are_monotone_and_zero_where_the_plain_ones_are():
    for sharded_size, plain, bytes_per_row in ((tc.align_rates_topk_sharded_workspace_bytes, tc.align_rates_topk_workspace_bytes, 20),
                                               (tc.align_span_topk_sharded_workspace_bytes, tc.align_span_topk_workspace_bytes, 32)):
        for Q, length, k, n in [(Q, length, k, n) for Q in (0, 1, 7, 64) for length in (0, 1, 40, 4095) for k in (1, 16, 64)
                                for n in (0, 1, 8, 16)]:
            size = sharded_size(Q, length, 0, k, n)
            blocks = (1 + max(n, 1)) * Q * (k + 1) * bytes_per_row
            assert plain(Q, length, 0, k) + blocks <= size <= plain(Q, length, 0, k) + blocks + 2 * 256
            assert sharded_size(Q + 1, length, 0, k, n) >= size and sharded_size(Q, length + 1, 0, k, n) >= size
            assert k == 64 or sharded_size(Q, length, 0, k + 1, n) >= size
            assert sharded_size(Q, length, 0, k, n + 1) >= size and sharded_size(Q, length, Q * length + 100, k, n) >= size
        for bad in ((-1, 1, 0, 1), (1, -1, 0, 1), (1, 1, -1, 1), (1, 1, 0, 0)):
            assert plain(*bad) == 0 and sharded_size(*bad, 1) == 0, bad
        assert sharded_size(1, 1, 0, 1, -1) == 0
    sized, plain = tc.align_parts_sharded_workspace_bytes, tc.align_parts_workspace_bytes
    for Q, length, k, P, n in [(Q, length, k, P, n) for Q in (0, 1, 7, 64) for length in (0, 40, 4095) for k in (1, 16, 64)
                               for P in (1, 2, 4) for n in (0, 1, 16)]:
        size = sized(Q, length, 0, k, P, n)
        blocks = (1 + max(n, 1)) * Q * k * (1 + P) * 24
        assert plain(Q, length, 0, k, P) + blocks <= size <= plain(Q, length, 0, k, P) + blocks + 2 * 256
        assert sized(Q + 1, length, 0, k, P, n) >= size and sized(Q, length + 1, 0, k, P, n) >= size
        assert sized(Q, length, 0, k + 1, P, n) >= size and (P == 4 or sized(Q, length, 0, k, P + 1, n) >= size)
        assert sized(Q, length, 0, k, P, n + 1) >= size and sized(Q, length, Q * length + 100, k, P, n) >= size
    for bad in ((-1, 10, 0, 1, 1), (1, -1, 0, 1, 1), (1, 10, -1, 1, 1), (1, 10, 0, 0, 1), (1, 10, 0, 1, 0), (1, 10, 0, 1, 5)):
        assert plain(*bad) == 0 and sized(*bad, 1) == 0, bad
    assert sized(1, 10, 0, 1, 1, -1) == 0


def test_the_new_exports_are_in_the_library_and_match_the_header():
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    defined = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", tbuild.SO], text=True).splitlines()
               if ln.strip()}
    assert set(NEW_EXPORTS) <= defined, sorted(set(NEW_EXPORTS) - defined)
    text = open(HEADER).read()
    for name in NEW_EXPORTS:
        assert _lib.SIGNATURES[name] == _prototype(text, name), name
    # a sharded call takes its unsharded call's arguments with the communicator behind the handle and the merge's two
    # outputs (one for the parts call) in place of the block
    P = _lib.SIGNATURES["tvz_align_parts"][1]
    for stem in ("tvz_align_rates_topk", "tvz_align_span_topk"):
        plain, shard = _lib.SIGNATURES[stem][1], _lib.SIGNATURES[stem + "_sharded"][1]
        assert shard == plain[:1] + [plain[0]] + plain[1:-4] + [plain[-4]] + plain[-4:], stem
        assert _lib.SIGNATURES[stem + "_sharded_workspace_bytes"] == _lib.SIGNATURES["tvz_align_wide_topk_sharded_workspace_bytes"]
    assert _lib.SIGNATURES["tvz_align_parts_sharded"][1] == P[:1] + [P[0]] + P[1:]
    assert all(f.rccl for f in tc.ALIGN_FORMS) and sharded.RcclShardedMatcher.align_forms == tc.ALIGN_FORMS
    assert sharded.HipBackend.align_forms == tc.ALIGN_FORMS and sharded.RcclShardedMatcher.supports_align_parts is True
    assert _lib.VERSION == 404 and _lib.load().tvz_version() == 404                # new exports only
    # the two kinds the service had keep their table; the walk's table holds all four, the parts kind behind them
    assert service.NEAR_FORMS == {service.ASK_NEAR: tc.FORM_BOUNDED, service.ASK_NEAR_WIDE: tc.FORM_WIDE}
    assert sorted(service.TICK_FORMS) == [2, 3, 4, 5] and service.ASK_PARTS == 6 and set(service.TICK_FORMS.values()) == set(tc.ALIGN_FORMS)
    assert service.ASK_HEADER == 5 + 6 + 1 + 8 + 1 + 64


# ---- the launcher ---------------------------------------------------------------------------------------------------
def test_the_launcher_passes_the_four_new_switches_on_and_refuses_their_bad_combinations(monkeypatch, tmp_path):
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
    wide = dict(near_top_k=4, near_any_offset=True)
    for bad, word in ((dict(near_rates=RATES), "needs --near-top-k"), (dict(near_spans=True), "needs --near-top-k"),
                      (dict(near_parts=2), "needs --near-top-k"), (dict(near_top_k=4, near_rates=RATES), "--near-rates needs --near-any-offset"),
                      (dict(near_top_k=4, near_spans=True), "--near-spans needs --near-any-offset"),
                      (dict(near_top_k=4, near_score="local", near_min_votes=2), "--near-score local needs --near-any-offset"),
                      (dict(wide, near_score="local"), "needs --near-min-votes >= 2"),
                      (dict(wide, near_parts=2), "needs --near-score local"),
                      (dict(wide, near_parts=2, near_score="containment"), "needs --near-score local"),
                      (dict(wide, near_parts=1, near_score="local", near_min_votes=2), "near_parts must be 0"),
                      (dict(wide, near_parts=5, near_score="local", near_min_votes=2), "near_parts must be 0"),
                      (dict(wide, near_rates=[1.0] * 9), "rates must be 1..8"), (dict(wide, near_rates=(1.0, -1.0)), "rates must be 1..8"),
                      (dict(wide, near_rates="1.0,fast"), "near_rates"), (dict(wide, near_score="cosine"), "near_score")):
        with pytest.raises(ValueError, match=word):
            service.RankService(2, url, **bad, **kw)
    for argv, word in ((["--near-rates", "1.0,0.96"], "needs --near-top-k"), (["--near-spans"], "needs --near-top-k"),
                       (["--near-parts", "2"], "needs --near-top-k"),
                       (["--near-top-k", "4", "--near-any-offset", "--near-parts", "2"], "needs --near-score local"),
                       (["--near-top-k", "4", "--near-any-offset", "--near-score", "local"], "needs --near-min-votes >= 2")):
        with pytest.raises(ValueError, match=word):
            service.main(["--ranks", "2", "--db", url] + argv)
    assert started == []
    # at their defaults the new switches add nothing; given, they stand behind the earlier ones
    plain = service.RankService(2, url, near_top_k=4, near_any_offset=True, near_min_votes=5, **kw)
    assert all(p.args[-3:] == ["--near-any-offset", "--near-min-votes", "5"] for p in plain.procs)
    on = service.RankService(2, url, near_top_k=4, near_any_offset=True, near_score="local", near_min_votes=8, near_rates=RATES,
                             near_spans=True, near_parts=3, **kw)
    for p in on.procs:
        assert p.args[-10:] == ["--near-any-offset", "--near-score", "local", "--near-min-votes", "8", "--near-rates", "1.0,0.96",
                                "--near-spans", "--near-parts", "3"]
    # ... a rank process parses them and hands them to its driver as Inspector takes them
    import argparse
    seen = {}
    monkeypatch.setattr(service, "_child_main", lambda a: seen.update(vars(a)) or 0)
    assert service.main(["--child"] + on.procs[0].args[on.procs[0].args.index("--near-top-k"):]) == 0
    got = service.near_kwargs(argparse.Namespace(**seen))
    assert got["near_rates"] == RATES and got["near_spans"] is True and got["near_parts"] == 3 and got["near_score"] == "local"
    assert got["near_min_votes"] == 8 and got["near_any_offset"] is True and got["near_top_k"] == 4
    B = type("B", (), dict(near_top_k=4, near_eps=EPS, near_max_offset=30.0, near_jaccard=0.8, near_rates="", near_spans=False,
                           near_parts=0))
    assert set(service.near_kwargs(B())) == {"near_duplicates", "near_top_k", "near_eps", "near_max_offset", "near_jaccard"}
    assert service.near_kwargs(type("C", (), {"near_top_k": 0, "near_rates": "1.0", "near_parts": 2})()) == {}
