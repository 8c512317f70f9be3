"""GPU parity of the tolerant match that keeps the per-shard top-k inside the sweep (tvz_match_tol_topk /
tvz_match_tol_sharded) and of the service route built on it: bit-exact on ids, counts, kth, order, padding and
totals against the restatement of the contract (tests/tol_ref.py) sorted by (kth, video_id, count), first k,
total = its length.  Every block any case produces is also checked for the precondition of tvz_topk_merge:
ascending in (kth, video_id, count), padding last."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from tests import tol_ref
from tests.test_tol_gpu import _grid_corpus, _load, _rows
from tvidz_amd import _lib, corpus as tc, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEVER = tc.KTH_NEVER
PAD = (-1, 0, NEVER)
INT32_MIN = int(np.iinfo(np.int32).min)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _order(e):
    return (e[2], e[0], e[1])


def _block(hits, k):
    """The [k+1] rows the contract promises for a query whose hits are `hits` [(video_id, count, kth)]."""
    best = sorted(hits, key=_order)[:k]
    return best + [PAD] * (k - len(best)) + [(-1, len(hits), NEVER)]


def _expected(rows, q, tol, mm, excl, k, form="sorted"):
    return _block(tol_ref.find_duplicates_tol(rows, q, tol, mm, excl, form=form), k)


def _tuples(block):
    return [tuple(int(x) for x in r) for r in block]


def _assert_mergeable(block):
    """tvz_topk_merge's precondition: the k rows ascending in (kth, video_id, count), every padding row last."""
    rows, tail = block[:-1], block[-1]
    real = [r for r in rows if r != PAD]
    assert rows == real + [PAD] * (len(rows) - len(real)), block
    assert real == sorted(real, key=_order), block
    assert tail[0] == -1 and tail[2] == NEVER, block


def _topk(dc, qs, tol, mm, k, excl=None, max_len=None, **kw):
    """match_tol_topk of a batch -> [Q] lists of k + 1 tuples (each checked for the merge's precondition)."""
    d_q, d_off, ml = tc.pack_queries(qs, DEV)
    d_ex = torch.tensor(excl, dtype=torch.int32, device=DEV) if excl is not None else None
    out = dc.match_tol_topk(d_q, d_off, ml if max_len is None else max_len, tol, mm, k, d_exclude_ids=d_ex, **kw)
    torch.cuda.synchronize()
    blocks = [_tuples(b) for b in out.cpu().numpy()]
    for b in blocks:
        _assert_mergeable(b)
    return blocks


@pytest.fixture(scope="module")
def dc():
    c = tc.DeviceCorpus(0)
    yield c
    c.close()


# ---- 1. the hand-made edge cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", [1, 2, 3, 4, 5])
def test_edge_cases_against_the_restatement(dc, mm):
    for name, rows, q, tol in tol_ref.edge_rows_and_queries():
        dc.upload(rows)
        for k in (1, 16, 64):
            for excl in (-1, 1):
                got = _topk(dc, [q], tol, mm, k, excl=[excl])[0]
                assert got == _expected(rows, q, tol, mm, excl, k, form="brute"), (name, mm, k, excl, got)


# ---- 2. tol 0 is the exact path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,mean_len,seed", [(300, 40, 1), (3000, 200, 2)])
def test_tol_zero_equals_match_topk_row_for_row(dc, C_, mean_len, seed):
    ids, offs, keys = synth.synth_timestamp_corpus(C_, seed=seed, mean_len=mean_len, dup_frac=0.05, frag_frac=0.05)
    dc.upload_csr(ids, offs, keys)
    rng = np.random.default_rng(seed)
    qs, excl = [], []
    for t in range(24):
        r = int(rng.integers(0, C_))
        q = keys[offs[r]:offs[r + 1]].tolist()
        if t % 3 == 1:
            q = q[: max(1, len(q) // 3)] + rng.choice(keys, size=20).tolist()
        if t % 3 == 2:
            q = rng.choice(keys, size=int(rng.integers(0, 300))).tolist()
        qs.append(q)
        excl.append(int(ids[r]) if t % 2 else -1)
    d_q, d_off, ml = tc.pack_queries(qs, DEV)
    d_ex = torch.tensor(excl, dtype=torch.int32, device=DEV)
    for mm in (1, 2, 3, 5):
        for k in (1, 16, 64):
            exact = dc.match_topk(d_q, d_off, ml, mm, C_, k, d_exclude_ids=d_ex)      # cap = every row: no overflow
            torch.cuda.synchronize()
            exact = exact.cpu().numpy()
            assert (exact[:, k, 1] >= 0).all()
            got = _topk(dc, qs, 0.0, mm, k, excl=excl)
            assert got == [_tuples(b) for b in exact], (mm, k)


def test_tol_zero_gives_the_reference_verdicts_on_the_golden_fixtures(dc, golden_dir):
    k = 64

    def verdict(q, mm, excl=-1):
        if not 1 <= mm <= 5:                                   # refused by name; the service sends these elsewhere
            with pytest.raises(RuntimeError, match="min_match"):
                _topk(dc, [q], 0.0, mm, k, excl=[excl])
            return None
        b = _topk(dc, [q], 0.0, mm, k, excl=[excl])[0]
        assert b[k][1] <= k
        return sorted(r for r in b[:k] if r != PAD)

    g = _load(golden_dir, "match_kat.json")
    for case in g["cases"] + [g["nan_case"]]:
        dc.upload(_rows(case["corpus"]))
        q = [float("nan") if x is None else x for x in case["query"]]
        got = verdict(q, case["min_match"])
        if got is not None:
            assert got == dc.find_duplicates(q, case["min_match"], with_kth=True), case["name"]
            assert [(v, c) for v, c, _ in got] == [tuple(e) for e in case["expected"]], case["name"]
    g = _load(golden_dir, "match_random.json")
    last = None
    for case in g["cases"]:
        if case["corpus_ref"] != last:
            dc.upload(_rows(g["corpora"][str(case["corpus_ref"])]))
            last = case["corpus_ref"]
        got = verdict(case["query"], case["min_match"])
        if got is not None:
            assert [(v, c) for v, c, _ in got] == [tuple(e) for e in case["expected"]], case["name"]
    g = _load(golden_dir, "match_streaming.json")
    for case in g["cases"]:
        dc.upload(_rows(case["corpus"]))
        dedup = []
        for ts in case["stream"]:
            if not dedup or ts != dedup[-1]:
                dedup.append(ts)
        got = verdict(dedup, case["min_match"], case["self_id"])
        if got:
            kstar = min(kk for _, _, kk in got)
            assert sorted(v for v, _, kk in got if kk == kstar) == case["dup_ids"], case["name"]
            assert dedup[:kstar + 1] == case["scene_timestamps"], case["name"]


# ---- 3. more hits than any list held, tie sets beyond k ----------------------------------------------------------
def _big_grid():
    rows = _grid_corpus(np.random.default_rng(41), 8000, 90000)
    q = (np.asarray(rows[4][1]) + 0.0004).tolist()
    assert len(q) == 114
    return rows, q


def test_more_hits_than_any_list_and_a_tie_set_beyond_k(dc):
    rows, q = _big_grid()
    dc.upload(rows)
    ref = {(tol, mm): tol_ref.find_duplicates_tol(rows, q, tol, mm, form="sorted")
           for tol, mm in ((0.1, 1), (0.1, 2), (0.1, 5), (0.001, 1), (0.001, 2))}
    # the inputs do what the case is for: more hits than the default caps, more rows tied at the best kth than k
    assert len(ref[(0.1, 2)]) > 4096
    assert len(ref[(0.1, 1)]) > 4096 and sum(1 for h in ref[(0.1, 1)] if h[2] == 0) > 64
    assert len(ref[(0.1, 5)]) > 64 and len(ref[(0.001, 1)]) > 64 and len(ref[(0.001, 2)]) > 64
    for (tol, mm), hits in ref.items():
        for k in (1, 16, 64):
            got = _topk(dc, [q], tol, mm, k)[0]
            assert got[k][1] == len(hits) and got[k][1] > 0, (tol, mm, k, got[k])
            assert got == _block(hits, k), (tol, mm, k)


def test_every_row_hits_with_the_same_count_and_kth(dc):
    rows = [(v, [100.0 + 0.0002 * (v % 5), 200.0]) for v in range(3000)]
    dc.upload(rows)
    q = [100.0004, 200.0003]
    for k in (1, 16, 64):
        got = _topk(dc, [q], 0.001, 2, k)[0]
        assert got == [(v, 2, 1) for v in range(k)] + [(-1, 3000, NEVER)], (k, got)
    assert got == _expected(rows, q, 0.001, 2, -1, 64)


# ---- 4. batches --------------------------------------------------------------------------------------------------
def _batch_rows(rng):
    rows = _grid_corpus(rng, 260, 15360)
    rows.append((9001, [7.0]))                                               # 1 key
    rows.append((9002, np.sort(rng.uniform(0, 600, 128)).tolist()))          # one 128-key step exactly
    rows.append((9003, np.sort(rng.uniform(0, 600, 129)).tolist()))          # one key into the second step
    rows.append((9004, np.sort(rng.uniform(-50, 600, 5000)).tolist()))       # several thousand keys
    rows.append((9005, rows[3][1]))                                          # the same video twice: equal words,
    rows.append((9005, rows[3][1]))                                          #   both kept
    rows.append((9006, []))
    return rows


@pytest.mark.parametrize("Q", [1, 3, 64, 1100])
def test_batches_against_the_restatement(dc, Q):
    rng = np.random.default_rng(100 + Q)
    rows = _batch_rows(rng)
    dc.upload(rows)
    long_q = rng.uniform(-50, 600, 4095)
    long_q[:100] = np.asarray((rows[9][1] * 100)[:100]) + 0.0003
    distinct = [
        (np.asarray(rows[3][1]) + 0.0003).tolist(),                          # meets the duplicated video
        [],                                                                  # 0 timestamps
        [7.0004],                                                            # 1 timestamp
        long_q.tolist(),                                                     # 4,095 timestamps
        [float("nan")] * 30,                                                 # all NaN
        [x if i % 2 else float("nan") for i, x in enumerate(rows[20][1] * 2)],   # half NaN, every value twice
        rng.uniform(0, 600, 300).tolist(),
        (np.asarray(rows[263][1][:400]) - 0.0002).tolist(),                  # meets the 5,000-key row
    ] + [(np.asarray(rows[int(v)][1]) + rng.choice([0.0, 0.0003, -0.0004])).tolist()
         for v in rng.integers(0, 260, 12)]
    pick = [int(i) for i in (np.arange(Q) % len(distinct))] if Q >= len(distinct) else [0, 3, 5][:Q]
    qs = [distinct[i] for i in pick]
    excl = [rows[int(rng.integers(0, 4))][0] if j % 3 == 0 else -1 for j in range(Q)]
    if Q > 3:
        excl[0] = 9005                                                       # ... and both excluded here
    for tol, mm, k in ((0.001, 2, 16), (0.02, 1, 64), (0.001, 4, 1)):
        got = _topk(dc, qs, tol, mm, k, excl=excl)
        memo = {}
        for j in range(Q):
            key = (pick[j], excl[j])
            if key not in memo:
                memo[key] = _expected(rows, qs[j], tol, mm, excl[j], k)
            assert got[j] == memo[key], (Q, tol, mm, k, j, pick[j], got[j][:4], memo[key][:4])
    # the duplicated video: two equal words, both kept, next to each other
    b = _topk(dc, [distinct[0]], 0.001, 2, 16)[0]
    assert sum(1 for r in b[:16] if r[0] == 9005) == 2


# ---- 5. after mutations ------------------------------------------------------------------------------------------
def test_after_upserts_a_rebuild_clear_and_on_one_row(dc):
    rng = np.random.default_rng(11)
    ids, offs, keys = synth.synth_timestamp_corpus(6000, seed=5, mean_len=60)
    dc.upload_csr(ids, offs, keys)
    builds0 = dc.index_stats()["builds"]
    rows = {int(ids[c]): keys[offs[c]:offs[c + 1]].tolist() for c in range(len(ids))}
    for v in rng.choice(ids, size=40, replace=False):
        rows[int(v)] = (np.asarray(rows[int(v)]) + 0.0004).tolist()        # replaced rows (delta table)
        dc.upsert(int(v), rows[int(v)])
    for v in range(900001, 900021):                                         # new rows
        rows[v] = np.sort(rng.uniform(0, 600, 50)).tolist()
        dc.upsert(v, rows[v])
    assert dc.index_stats()["delta_rows"] > 0
    table = sorted(rows.items())
    probes = (900003, int(ids[17]))
    for v in probes:
        q = (np.asarray(rows[v]) - 0.0007).tolist()
        got = _topk(dc, [q], 0.001, 2, 16)[0]
        assert got == _expected(table, q, 0.001, 2, -1, 16) and any(r[0] == v for r in got)
    for v in range(910000, 911200):                                         # enough appends for background rebuilds
        rows[v] = np.sort(rng.uniform(0, 600, 20)).tolist()
        dc.upsert(v, rows[v])
    assert dc.index_stats()["builds"] > builds0
    table = sorted(rows.items())
    for v in probes + (910777,):
        q = (np.asarray(rows[v]) - 0.0007).tolist()
        got = _topk(dc, [q], 0.001, 2, 16)[0]
        assert got == _expected(table, q, 0.001, 2, -1, 16) and any(r[0] == v for r in got)
    dc.clear()
    assert _topk(dc, [rows[900003], []], 0.001, 1, 4) == [[PAD] * 4 + [(-1, 0, NEVER)]] * 2
    dc.upsert(5, [1.0, 2.0])
    assert _topk(dc, [[1.0004, 2.0004]], 0.001, 2, 4)[0] == [(5, 2, 1)] + [PAD] * 3 + [(-1, 1, NEVER)]
    fresh = tc.DeviceCorpus(0)                                               # a handle that never held a row
    try:
        assert _topk(fresh, [[1.0]], 0.001, 1, 2)[0] == [PAD] * 2 + [(-1, 0, NEVER)]
    finally:
        fresh.close()


# ---- 6. eight shard handles on one GPU ---------------------------------------------------------------------------
def test_eight_shards_merge_into_the_whole_tables_topk(dc):
    rng = np.random.default_rng(9)
    rows = _grid_corpus(rng, 2000, 90000)
    shards = [tc.DeviceCorpus(0) for _ in range(8)]
    try:
        for r, s in enumerate(shards):
            s.upload(rows[r::8])
        qs = [(np.asarray(rows[int(v)][1]) + 0.0004 * (t % 3)).tolist() for t, v in enumerate(rng.integers(0, 2000, 12))]
        excl = [rows[7][0] if t % 2 else -1 for t in range(len(qs))]
        d_q, d_off, ml = tc.pack_queries(qs, DEV)
        d_ex = torch.tensor(excl, dtype=torch.int32, device=DEV)
        for tol, mm, k in ((0.001, 2, 8), (0.1, 1, 16), (0.1, 2, 64)):
            blocks = torch.stack([s.match_tol_topk(d_q, d_off, ml, tol, mm, k, d_exclude_ids=d_ex) for s in shards])
            merged, totals = tc.topk_merge(blocks.contiguous(), k)
            torch.cuda.synchronize()
            for sb in blocks.cpu().numpy():
                for b in sb:
                    _assert_mergeable(_tuples(b))
            merged, totals = merged.cpu().numpy(), totals.cpu().numpy()
            for j, q in enumerate(qs):
                exp = _expected(rows, q, tol, mm, excl[j], k)
                assert _tuples(merged[j]) == exp[:k] and int(totals[j]) == exp[k][1], (tol, mm, k, j)
    finally:
        for s in shards:
            s.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------
def _raw_call(dc, d_q, d_off, Q, max_len, tol, mm, k, out, ws):
    lib = _lib.load()
    rc = lib.tvz_match_tol_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), Q, max_len, tol, mm, None, k,
                                out.data_ptr(), ws.data_ptr() if ws is not None else None,
                                ws.numel() if ws is not None else 0, None)
    return rc, lib.tvz_last_error()


def test_refusals_write_nothing(dc):
    dc.upload([(1, [1.0, 2.0]), (2, [1.0])])
    d_q, d_off, ml = tc.pack_queries([[1.0], [2.0]], DEV)
    ws = torch.empty(tc.tol_topk_workspace_bytes(2, 4096, 0, 64), dtype=torch.uint8, device=DEV)
    out = torch.full((2, 66, 3), -5, dtype=torch.int32, device=DEV)
    cases = [((float("nan"), 1, 4, ml), -1, b"tol must be finite"), ((float("inf"), 1, 4, ml), -1, b"tol must be finite"),
             ((-0.001, 1, 4, ml), -1, b"tol must be finite"),
             ((0.001, 0, 4, ml), -4, b"min_match"), ((0.001, 6, 4, ml), -4, b"min_match"),
             ((0.001, 1, 0, ml), -4, b"k="), ((0.001, 1, 65, ml), -4, b"k="),
             ((0.001, 1, 4, 4096), -4, b"max_query_len")]
    for (tol, mm, k, max_len), want, msg in cases:
        rc, err = _raw_call(dc, d_q, d_off, 2, max_len, tol, mm, k, out, ws)
        assert rc == want and msg in err, (tol, mm, k, max_len, rc, err)
    small = torch.empty(64, dtype=torch.uint8, device=DEV)
    rc, err = _raw_call(dc, d_q, d_off, 2, ml, 0.001, 1, 4, out, small)
    assert rc == -5 and b"bytes missing" in err, (rc, err)
    rc, err = _raw_call(dc, d_q, d_off, 2, ml, 0.001, 1, 4, out, None)
    assert rc == -5 and b"bytes missing" in err, (rc, err)
    torch.cuda.synchronize()
    assert (out == -5).all()
    with pytest.raises(RuntimeError, match="tol must be finite"):
        dc.match_tol_topk(d_q, d_off, ml, float("nan"), 1, 4)
    need = tc.tol_topk_workspace_bytes(2, ml, d_q.numel(), 4)
    exact_ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc, err = _raw_call(dc, d_q, d_off, 2, ml, 0.001, 1, 4, out, exact_ws)
    torch.cuda.synchronize()
    assert rc == 0, err
    got = out.cpu().numpy().reshape(-1)[:2 * 5 * 3].reshape(2, 5, 3)          # k = 4: [Q][k+1][3] from the start
    assert _tuples(got[0][:5]) == [(1, 1, 0), (2, 1, 0), PAD, PAD, (-1, 2, NEVER)]
    assert _tuples(got[1][:5]) == [(1, 1, 0), PAD, PAD, PAD, (-1, 1, NEVER)]


def test_a_query_longer_than_max_query_len_is_flagged_alone(dc):
    rows = [(v, [1.0, 2.0, 3.0]) for v in range(100)]
    dc.upload(rows)
    qs = [[1.0003, 2.0], [1.0] * 10, [2.0]]
    got = _topk(dc, qs, 0.001, 1, 8, max_len=5)                 # max_query_len 5 is not an upper bound
    assert got[1] == [PAD] * 8 + [(-1, INT32_MIN, NEVER)]
    assert got[0] == _expected(rows, qs[0], 0.001, 1, -1, 8) and got[0][8][1] == 100
    assert got[2] == _expected(rows, qs[2], 0.001, 1, -1, 8) and got[2][8][1] == 100


# ---- 7. tvz_match_tol_sharded at world size 1 through RCCL -------------------------------------------------------
def test_match_tol_sharded_through_rccl_world_size_1():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tol_comm_child.py")], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    rng = np.random.default_rng(77)
    rows = _grid_corpus(rng, 1500, 90000)
    picks = [int(v) for v in rng.integers(0, len(rows), 10)]
    assert picks == res["picks"]
    k, mm = 16, 2
    for tol in (0.001, 0.1):
        got = res["sharded"][str(tol)]
        for t, v in enumerate(picks):
            q = (np.asarray(rows[v][1]) + 0.0004 * (t % 3)).tolist()
            exp = _expected(rows, q, tol, mm, res["excl"][t], k)
            assert [tuple(r) for r in got["merged"][t]] == exp[:k] and got["totals"][t] == exp[k][1] >= 0, (tol, t)
        assert res["local"][str(tol)] is True              # = match_tol_topk + tvz_topk_merge
    assert res["batches_differ"] is True
    assert res["matcher_equal"] is True                    # RcclShardedMatcher.match_topk(..., tolerance=t), 0 in between
    assert res["streaming_equal"] is True                  # ... and with a batch in flight behind the other


# ---- 9. RankCorpus on one GPU over RcclShardedMatcher ------------------------------------------------------------
def test_rank_corpus_on_one_gpu_with_concurrent_tolerant_and_exact_asks():
    from tvidz_amd import service, sharded
    rows, big_q = _big_grid()
    whole = tc.DeviceCorpus(0)
    shard = tc.DeviceCorpus(0)
    comm = sharded.make_comm(0)
    matcher = sharded.RcclShardedMatcher(shard, comm, k=64, cap=2048)
    rc = service.RankCorpus(shard, matcher, xdev="cuda:0", tick_s=0.001)
    try:
        assert rc.supports_tolerance
        whole.upload(rows)
        rc.upload(rows)
        rng = np.random.default_rng(5)
        asks = []
        for i in range(24):
            v = int(rng.integers(0, len(rows)))
            q = (np.asarray(rows[v][1]) + (0.0, 0.0003, -0.0004)[i % 3]).tolist()
            asks.append((q, (2, 1, 3)[i % 3], rows[(v + 1) % len(rows)][0] if i % 2 else -1, (0.0, 0.001, 0.02, 0.0)[i % 4]))
        errs = []

        def ask(i):
            try:
                q, mm, excl, tol = asks[i]
                exp = whole.find_duplicates(q, mm, exclude_id=excl, with_kth=True, tolerance=tol)
                got = rc.find_duplicates(q, mm, exclude_id=excl, with_kth=True, tolerance=tol)
                kstar = min((h[2] for h in exp), default=None)
                assert sorted(h[0] for h in got if h[2] == kstar) == sorted(h[0] for h in exp if h[2] == kstar), i
                assert set(got) <= set(exp)
                pairs = rc.find_duplicates(q, mm, exclude_id=excl, tolerance=tol)       # db.find_duplicates: every row
                assert pairs == [(v_, c) for v_, c, _ in exp], i
            except Exception as e:                                        # pragma: no cover
                errs.append(repr(e))
        th = [threading.Thread(target=ask, args=(i,)) for i in range(24)]
        [t.start() for t in th]
        [t.join(180) for t in th]
        assert not errs, errs[:2]
        # the tie set beyond k of section 3: 164 rows at kth 0 with k = 64 -> the exact round, the answer complete
        before = rc.exact_asks
        exp = whole.find_duplicates(big_q, 1, with_kth=True, tolerance=0.1)
        assert exp == tol_ref.find_duplicates_tol(rows, big_q, 0.1, 1, form="sorted")
        assert sum(1 for h in exp if h[2] == 0) > 64
        got = rc.find_duplicates(big_q, 1, with_kth=True, tolerance=0.1)
        assert rc.exact_asks == before + 1 and got == exp
        # more hits than k but a conclusive verdict: read off the top-k, no exact round
        exp = whole.find_duplicates(big_q, 2, with_kth=True, tolerance=0.1)
        kstar = min(h[2] for h in exp)
        assert len(exp) > 4096 and sum(1 for h in exp if h[2] == kstar) <= 64
        before = rc.exact_asks
        got = rc.find_duplicates(big_q, 2, with_kth=True, tolerance=0.1)
        assert rc.exact_asks == before and len(got) == 64 and set(got) <= set(exp)
        assert sorted(h for h in got if h[2] == kstar) == sorted(h for h in exp if h[2] == kstar)
        ts = [8000.5 + i for i in range(5)]
        rc.upsert(80001, ts)                              # ingested here: seen by the next tolerant ask
        assert rc.find_duplicates([t + 0.0004 for t in ts[:3]], 2, with_kth=True, tolerance=0.001) == [(80001, 3, 1)]
        assert rc.find_duplicates([t + 0.0004 for t in ts[:3]], 2, with_kth=True) == []
        assert rc.broken is None
    finally:
        rc.close()
        comm.close()
        whole.close()


# ---- 10. end to end ----------------------------------------------------------------------------------------------
def test_inspector_over_a_rank_corpus_flags_a_millisecond_remux_only_with_a_tolerance(tmp_path):
    """tests/test_tol_gpu.py's millisecond-remux pair through db.Store(url, corpus=RankCorpus(...)): the copy is
    flagged and truncated at the same kth with match_tolerance=0.001, not with 0."""
    from tests.test_inspector_gpu import H, W, T, _clip, _oracle_cuts
    from tvidz_amd import db as tdb, feeder, inspector as insp, service, sharded

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
        shard = tc.DeviceCorpus(0)
        comm = sharded.make_comm(0)
        rc = service.RankCorpus(shard, sharded.RcclShardedMatcher(shard, comm, k=16, cap=1024), xdev="cuda:0", tick_s=0.001)
        store = tdb.Store(f"sqlite:///{tmp_path}/t{int(dup)}.db", corpus=rc, census=False)
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
            assert rc.broken is None and rc.busy_ticks >= 1
        finally:
            ins.close()
            store.close()
            rc.close()
            comm.close()


def test_rank_service_launcher_on_one_gpu_with_a_match_tolerance(tmp_path):
    """`python -m tvidz_amd.service --ranks 1 --match-tolerance 0.001` in the shape of
    tests/test_service_gpu.py::test_rank_service_launcher_on_one_gpu: ONE fresh rank process, the front's HTTP
    surface; a remux of an earlier upload (time base 1/1000) is flagged at its 2nd cut."""
    import time
    import requests
    from werkzeug.serving import make_server
    from oracle import oracle
    from tvidz_amd import service

    port = 6400 + os.getpid() % 200
    svc = service.RankService(1, f"sqlite:///{tmp_path}/t.db", base_port=port, parts="tests.tol_fakes:gpu_tol_rank_parts",
                              k=16, cap=1024, workers=8, ready_timeout=240, match_tolerance=0.001,
                              env={"PYTHONPATH": ROOT})
    srv = make_server("127.0.0.1", port, service.create_front(svc.urls), threaded=True)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    base = f"http://127.0.0.1:{port}"
    try:
        assert svc.procs[0].args[-2:] == ["--match-tolerance", "0.001"]

        def key(name, pts0, cuts, stamp=1700000000):
            return f"videos/{stamp}-{name}__{pts0}__{'_'.join(map(str, cuts))}.y4m"

        def notify(k):
            r = requests.post(f"{base}/notify", timeout=30,
                              json={"Records": [{"s3": {"bucket": {"name": "videos"}, "object": {"key": k}}}]})
            assert r.status_code == 200, r.text

        def wait(k, timeout=120):
            fn, end = k.split("/")[-1], time.time() + timeout
            while time.time() < end:
                rec = requests.get(f"{base}/status/{fn}", timeout=30).json()
                if rec.get("status") in ("done", "error"):
                    return rec
                time.sleep(0.05)
            raise AssertionError(f"{fn} never finished")

        clips = {"a": (1000, [7, 19, 33, 50]), "b": (5000, [5, 21, 40])}
        for name, (pts0, cuts) in clips.items():
            k = key(name, pts0, cuts)
            notify(k)
            rec = wait(k)
            assert rec["status"] == "done" and rec["duplicates"] == [], rec
            assert rec["scene_cuts"] == [oracle.pts_time_value(pts0 + c, 1, 30, 0) for c in cuts], rec
        pts0, cuts = clips["a"]
        remux = [oracle.pts_time_value(round((pts0 + c) * 1000 / 30), 1, 1000, 0) for c in cuts]
        orig = [oracle.pts_time_value(pts0 + c, 1, 30, 0) for c in cuts]
        assert remux[0] != orig[0] and remux[1] != orig[1] and all(abs(a - b) < 0.001 for a, b in zip(remux, orig))
        k = key("a_remux", pts0, cuts, stamp=1700000050)
        notify(k)
        rec = wait(k)
        assert rec["status"] == "done" and rec["scene_cuts"] == remux[:2], rec
        assert rec["duplicates"] == [service.clean_name(key("a", pts0, cuts))], rec
        info = requests.get(f"{base}/ranks", timeout=30).json()["ranks"][0]
        assert info["rows"] == 3 and info["broken"] is None and svc.dead() == []
    finally:
        srv.shutdown()
        svc.stop()


# ---- 11. many rows per 16-lane group: the threshold and the compaction INSIDE the row loop ------------------------
def _lattice_corpus(rng, n_rows):
    """Cheap rows that mostly hit: 3..8 cuts each from a lattice of 120 half-second marks, jittered by < 40 ms, ids
    1..n_rows in order; the last 300 rows repeat earlier rows under THEIR ids (equal words, both kept)."""
    marks = np.arange(120) * 0.5 + 10.0
    rows = []
    for v in range(n_rows - 300):
        pick = np.sort(rng.choice(120, size=int(rng.integers(3, 9)), replace=False))
        rows.append((v + 1, (marks[pick] + rng.integers(-40, 41, size=pick.size) / 1000.0).tolist()))
    for j in range(300):
        rows.append(rows[(j * 97) % (n_rows - 300)])
    return rows


def _hits_all_mm(rows_sets, q, tol, mms, excl):
    """tol_ref's verdicts for several min_match from ONE mask per row (match_mask_sorted, as find_duplicates_tol)."""
    q = np.asarray(q, dtype=np.float64)
    out = {mm: [] for mm in mms}
    for vid, r in rows_sets:
        if vid == excl:
            continue
        m = tol_ref.match_mask_sorted(q, r, tol)
        cnt = int(m.sum())
        if cnt:
            idx = np.flatnonzero(m)
            for mm in mms:
                if cnt >= mm:
                    out[mm].append((vid, cnt, int(idx[mm - 1])))
    return out


def test_many_rows_per_group_fill_the_stage_inside_the_loop(dc):
    """60,000 rows at Q = 64: the sweep runs 95 row blocks per query, so every 16-lane group walks about forty rows
    and a wave about 160 - with most rows hitting at 0.1 s a wave's stage fills several times INSIDE the row loop,
    its k-th word becomes a threshold and later hits are dropped against it (both kth modes, k 1 / 16 / 64, an
    exclusion, equal words)."""
    rng = np.random.default_rng(2024)
    n_rows, Q, blocks = 60_000, 64, 95
    rows = _lattice_corpus(rng, n_rows)
    dc.upload(rows)
    rows_sets = [(v, tol_ref.row_set(t)) for v, t in rows]
    marks = np.arange(120) * 0.5 + 10.0
    distinct = []
    for t in range(8):
        pick = rng.permutation(120)[:90]                                   # unsorted: kth is a position in THIS order
        distinct.append((marks[pick] + rng.integers(-40, 41, size=90) / 1000.0).tolist())
    distinct.append(rows[11][1] + rows[11][1])                             # every value twice
    excl_of = [-1, rows[5][0], rows[(3 * 97) % (n_rows - 300)][0]]         # the last one: a video that is there twice
    ref = {}
    for d in range(len(distinct)):
        for e in (excl_of if d < 2 else excl_of[:1]):
            ref[(d, e)] = _hits_all_mm(rows_sets, distinct[d], 0.1, (1, 2, 5), e)
    # the inputs do what the case is for.  A wave sees ceil(rows / (95 * 4)) <= 158 rows, a group <= 40 of them; with
    # more hits than 64 per wave on AVERAGE some wave must compact inside its loop even at k = 64 (before its list is
    # full nothing is dropped, and the stage is compacted once it holds more than 60), and afterwards its threshold
    # is live for the rest of its rows
    waves = blocks * 4
    for (d, e), by_mm in ref.items():
        if d < 8:
            assert len(by_mm[1]) > 64 * waves and len(by_mm[2]) > 64 * waves, (d, e, len(by_mm[1]), len(by_mm[2]))
            assert len(by_mm[5]) > 16 * waves, (d, e, len(by_mm[5]))
    h1 = ref[(0, -1)][1]
    assert len(h1) != len({(v, c, kk) for v, c, kk in h1})                 # equal words among the hits
    order = [(d, e) for (d, e) in ref]
    pick = [order[j % len(order)] for j in range(Q)]
    qs = [distinct[d] for d, _ in pick]
    excl = [e for _, e in pick]
    for mm in (1, 2, 5):
        for k in (1, 16, 64):
            got = _topk(dc, qs, 0.1, mm, k, excl=excl)
            for j in range(Q):
                assert got[j] == _block(ref[pick[j]][mm], k), (mm, k, j, pick[j], got[j][:3], got[j][k])
