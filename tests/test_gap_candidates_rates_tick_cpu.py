"""The rank tick's ask kind 8 (ASK_CANDIDATES_RATES) over gloo at world sizes 2 and 3 with a fake matcher
(tests/gap_candidates_rates_service_fakes.py): RankCorpus.align_candidates_rates against the reference over the whole
table; kinds 7 and 8, parts and search asks in one tick, with the same matcher calls in the same order on every rank -
the rates calls behind the kind-7 calls, in sorted parameter order, asks that agree sharing one call, two rate lists
giving two calls; the split into consecutive runs where the asks of one parameter set times n_rates exceed one call's
probe lists (service.CAND_RATES_MAX_LISTS patched small on every rank); the caller's refusals; an over-long query."""
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import gap_candidates_cases as cs, gap_candidates_rates_cases as rc, gap_candidates_rates_ref as rr
from tests.near_fakes import free_port_run
from tvidz_amd import corpus as tc, service, sharded

EPS = cs.GAP_EPS
L = 129
RA, RB = (1.0, rc.SLOW), (1.0, rc.QUARTER, rc.FAST)


def _tick_table():
    up = cs.uploads()
    queries = [up[n] for n in ("shifted", "excerpt", "twin", "stranger", "three")] + [cs.long_query(515, 2)[:L]] + \
        [[float(i) for i in range(150)]]
    return cs.table(), queries                                       # the last query is over-long at max_query_len = L


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


def _rated(c, rates, min_count=1, cap=4096):
    return (EPS, 0.0, c, min_count, cap, 0) + service.check_near_rates(rates)


def _mixed_asks(rows, queries, rank):
    """asks of kind 8 in three parameter sets (two rate lists) among asks of kind 7, a parts and a search ask and a top-k
    ask, in an order that depends on the rank"""
    from tests import align_parts_cases as pc
    qa, qb = np.asarray(queries[0]), np.asarray(queries[1])
    r1 = service.check_near_rates((1.0,))
    parts = service.check_near(tc.FORM_SPAN, pc.EPS, None, 2, 1, 0) + r1 + (2,)
    asks = [(qa, 0, -1, service.ASK_CANDIDATES_RATES, 0.0, _rated(4, RB)),
            (qb, 0, -1, service.ASK_PARTS, 0.0, parts + (float(cs.FILM), -1.0)),
            (qb, 0, cs.FILM, service.ASK_CANDIDATES_RATES, 0.0, _rated(4, RA)),
            (qa, 0, -1, service.ASK_CANDIDATES, 0.0, (EPS, 0.0, 16, 1, 4096)),
            (qa, 0, -1, service.ASK_NEAR_WIDE, 0.0, service.check_near(tc.FORM_WIDE, pc.EPS, None, 4, 1, 0)),
            (qa, 0, -1, service.ASK_CANDIDATES_RATES, 0.0, _rated(4, RA)),
            (np.asarray(rows[15][1]), 2, -1, service.ASK_TOPK, 0.0, None),
            (qb, 0, -1, service.ASK_CANDIDATES_RATES, 0.0, _rated(16, RA, 6))]
    return asks[rank % len(asks):] + asks[:rank % len(asks)]


def _expected(rows, a):
    _, _, c, min_count, cap, _, n = a[5][:7]
    rates = tuple(a[5][7:7 + n])
    return rr.candidates_rates(rows, [a[0].tolist()], EPS, rates, c, min_count=min_count, cap=cap,
                               exclude_ids=None if a[2] < 0 else [a[2]])[0], c


def _rank_worker(rank, world, port, out):
    from tests.gap_candidates_rates_service_fakes import CandidatesRatesBackend
    from tests.gap_candidates_service_fakes import CandidatesBackend, GapOracleCorpus
    _init(rank, world, port)
    rk = None
    try:
        rows, queries = _tick_table()
        shard = GapOracleCorpus()
        g = dist.new_group(backend="gloo")                            # the tick thread's own group
        backend = CandidatesRatesBackend(live=shard)
        rk = service.RankCorpus(shard, sharded.ShardedMatcher(backend, k=8, cap=64, group=g), group=g, xdev="cpu", tick_s=0.01)
        assert rk.supports_align_candidate_rates and rk.supports_align_candidates
        rk.upload(rows)                                               # video_id mod world
        with pytest.raises(RuntimeError, match="keeps no gap codes"):
            rk.align_candidates_rates(queries[:1], RA, c=16)
        rk.set_gap_index(EPS)
        dist.barrier()
        # (1) the public call, alone: the whole table's answer; the over-long query is refused without travelling
        excl = [cs.FILM] + [-1] * (len(queries) - 1)
        for c, min_count, rates in ((16, 1, RA), (1, 2, RB), (64, 1, RB)):
            exp = rr.candidates_rates(rows, queries, EPS, rates, c, min_count=min_count, exclude_ids=excl, max_query_len=L)
            ids, counts, rate_indexes, totals = rk.align_candidates_rates(queries, rates, c=c, min_count=min_count,
                                                                          exclude_ids=excl, max_query_len=L)
            assert ids.dtype == np.int32 and ids.shape == counts.shape == rate_indexes.shape == (len(queries), c)
            assert totals.dtype == np.int32 and totals.shape == (len(queries),)
            assert (ids == exp[:, :c, 0]).all() and (counts == exp[:, :c, 1]).all() and (rate_indexes == exp[:, :c, 2]).all()
            assert (totals == exp[:, c, 1]).all(), (c, min_count)
            assert totals[-1] == tc.ALIGN_CANDIDATES_REFUSED and (ids[-1] == -1).all() and (counts[-1] == 0).all()
        dist.barrier()
        calls = list(backend.calls)
        dist.barrier()
        assert all(c[1] <= world * (len(queries) - 1) for c in calls)                 # the over-long query never reached a matcher
        # (2) mixed asks pending at once on every rank, in another order on each: every ask is answered as it is alone
        asks = _mixed_asks(rows, queries, rank)
        alone = [rk._ask_all([a])[0] for a in asks]
        dist.barrier()
        together = rk._ask_all(asks)
        rk._ask(asks[0][0], 2, -1, service.ASK_TOPK)                  # one more tick: the last one has ended everywhere
        dist.barrier()
        for a, x, y in zip(asks, alone, together):
            if a[3] == service.ASK_PARTS:
                assert (x == y).all()
            else:
                assert (np.asarray(x[0]) == np.asarray(y[0])).all() and x[1] == y[1]
            if a[3] == service.ASK_CANDIDATES_RATES:
                exp, c = _expected(rows, a)
                assert y[0].shape == (c, 3) and (y[0] == exp[:c]).all() and y[1] == exp[c, 1], a[5]
        # ... and once more from rank 0 alone, so that ONE tick holds exactly these asks: its calls can be counted
        n0 = len(backend.calls)
        dist.barrier()
        if rank == 0:
            rk._ask_all(asks)
        dist.barrier()
        rk._ask(asks[0][0], 2, -1, service.ASK_TOPK)
        dist.barrier()
        everyone = [None] * world
        dist.all_gather_object(everyone, list(backend.calls))
        assert all(e == everyone[0] for e in everyone)                              # the same calls, in the same order
        tick = [c for c in everyone[0][n0:] if c[0] != "match_topk"]
        kinds = [c[0] for c in tick]
        rated = [c for c in tick if c[0] == "align_candidates_rates"]
        # sorted parameters: (C, min_count, cap, n_rates, the rates) - two rate lists at C = 4 are two calls
        assert [c[2] for c in rated] == [(EPS, 4, 1, 4096, RA), (EPS, 4, 1, 4096, RB), (EPS, 16, 6, 4096, RA)]
        assert [c[1] for c in rated] == [2, 1, 1]                                   # asks that agree share one call
        assert kinds.count("align_candidates") == 1 and kinds.count("align_parts") == 1 and "align_wide_topk" in kinds
        first_rated = kinds.index("align_candidates_rates")
        assert kinds.index("align_parts") < kinds.index("align_candidates") < first_rated       # behind the kind-7 calls
        assert all(k == "align_candidates_rates" for k in kinds[first_rated:])
        # (3) the split: one call takes CAND_RATES_MAX_LISTS probe lists.  7 lists at 3 rates are runs of 2 asks: five asks
        #     of one parameter set go as 2 + 2 + 1, in the asks' order, and every ask gets its own answer
        service.CAND_RATES_MAX_LISTS = 7                              # (this process's copy: every rank patches alike)
        dist.barrier()
        five = [(np.asarray(queries[i]), 0, -1, service.ASK_CANDIDATES_RATES, 0.0, _rated(4, RB)) for i in (0, 1, 2, 3, 1)]
        n1 = len(backend.calls)
        dist.barrier()
        if rank == 0:
            got = rk._ask_all(five)
            for a, y in zip(five, got):
                exp, c = _expected(rows, a)
                assert (y[0] == exp[:c]).all() and y[1] == exp[c, 1]
        dist.barrier()
        rk._ask(asks[0][0], 2, -1, service.ASK_TOPK)
        dist.barrier()
        split = [c for c in backend.calls[n1:] if c[0] == "align_candidates_rates"]
        assert [c[1] for c in split] == [2, 2, 1] and all(c[2] == (EPS, 4, 1, 4096, RB) for c in split)
        everyone = [None] * world
        dist.all_gather_object(everyone, split)
        assert all(e == everyone[0] for e in everyone)                              # the same split on every rank
        service.CAND_RATES_MAX_LISTS = 65535
        dist.barrier()
        # (4) refused in the caller, before the tick: nothing reaches a matcher, the loop keeps running
        n2, ticks = len(backend.calls), rk.busy_ticks
        if rank == 0:
            q = [queries[1]]
            for call in (lambda: rk.align_candidates_rates(q, RA, c=0), lambda: rk.align_candidates_rates(q, RA, c=65),
                         lambda: rk.align_candidates_rates(q, RA, c=16, cap=15), lambda: rk.align_candidates_rates(q, RA, c=16, min_count=0),
                         lambda: rk.align_candidates_rates(q, (), c=16), lambda: rk.align_candidates_rates(q, (1.0,) * 9, c=16),
                         lambda: rk.align_candidates_rates(q, (1.0, float("nan")), c=16), lambda: rk.align_candidates_rates(q, (0.0,), c=16),
                         lambda: rk.align_candidates_rates(q, RA, c=16, exclude_ids=[1, 2])):
                with pytest.raises(ValueError):
                    call()
            no_call = service.RankCorpus.__new__(service.RankCorpus)
            no_call.shard, no_call.matcher = shard, sharded.ShardedMatcher(CandidatesBackend(live=shard), k=8, cap=64, group=g)
            assert not no_call.supports_align_candidate_rates
            with pytest.raises(RuntimeError, match="has no align_candidates_rates"):
                service.RankCorpus.align_candidates_rates(no_call, q, RA, c=16)
            ids, counts, rate_indexes, totals = rk.align_candidates_rates([[0.5] * 4096], RA, c=4)
            assert totals.tolist() == [tc.ALIGN_CANDIDATES_REFUSED] and (ids == -1).all() and (counts == 0).all() \
                and (rate_indexes == 0).all()
            assert len(backend.calls) == n2 and rk.busy_ticks == ticks
        dist.barrier()
        assert rk.broken is None
        out.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        out.put((rank, repr(e)))
        raise
    finally:
        if rk is not None:
            rk.close()
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_the_tick_answers_candidates_asks_with_rates_over_gloo(world):
    _run(_rank_worker, world)
