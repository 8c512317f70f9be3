"""GPU parity: HIP corpus matcher (through the C ABI) vs the oracle and the golden fixtures
generated from the reference's own db.find_duplicates (bit-exact: integer/index work)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import topk_ref
from tvidz_amd import _lib, corpus as tc, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEVER = tc.KTH_NEVER


def _load(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return json.load(f)


def _rows(corpus):
    return [(int(v), [float("nan") if x is None else float(x) for x in t]) for v, t in corpus]


@pytest.fixture(scope="module")
def dc():
    c = tc.DeviceCorpus(0)
    yield c
    c.close()


def test_reference_kat_test_app_66_83(dc):
    dc.upload([(1, [1.0, 2.0, 3.0, 4.0, 5.0]), (2, [10.0, 20.0, 30.0, 40.0, 50.0])])
    dups = dc.find_duplicates([10.0, 20.0, 30.0, 40.0, 50.0], min_match=5)
    assert (1, 0) not in dups and (2, 5) in dups
    dc.upsert(3, [1.0, 2.0, 3.0, 4.0, 5.0])
    dups = dc.find_duplicates([1.0, 2.0, 3.0, 4.0, 5.0], min_match=5)
    assert (1, 5) in dups and (3, 5) in dups and len(dups) == 2


def test_golden_kat(dc, golden_dir):
    g = _load(golden_dir, "match_kat.json")
    for case in g["cases"] + [g["nan_case"]]:
        dc.upload(_rows(case["corpus"]))
        q = [float("nan") if x is None else x for x in case["query"]]
        got = dc.find_duplicates(q, case["min_match"])
        assert got == [tuple(e) for e in case["expected"]], case["name"]


def test_golden_random(dc, golden_dir):
    g = _load(golden_dir, "match_random.json")
    last = None
    for case in g["cases"]:
        if case["corpus_ref"] != last:
            dc.upload(_rows(g["corpora"][str(case["corpus_ref"])]))
            last = case["corpus_ref"]
        got = dc.find_duplicates(case["query"], case["min_match"])
        assert got == [tuple(e) for e in case["expected"]], case["name"]


def test_golden_streaming_verdicts(dc, golden_dir):
    """One call with kth replaces the per-prefix loop of app.py:231-255."""
    g = _load(golden_dir, "match_streaming.json")
    for case in g["cases"]:
        dc.upload(_rows(case["corpus"]))
        dedup = []
        for ts in case["stream"]:
            if not dedup or ts != dedup[-1]:
                dedup.append(ts)
        hits = dc.find_duplicates(dedup, case["min_match"], exclude_id=case["self_id"], with_kth=True)
        assert all(v != case["self_id"] for v, _, _ in hits)
        if not hits:
            assert case["dup_ids"] == [] and case["scene_timestamps"] == dedup
            continue
        kstar = min(k for _, _, k in hits)
        assert sorted(v for v, _, k in hits if k == kstar) == case["dup_ids"], case["name"]
        assert dedup[:kstar + 1] == case["scene_timestamps"], case["name"]
        # and the prefix query at k* returns exactly the reference's (id, count) pairs
        pref = dc.find_duplicates(dedup[:kstar + 1], case["min_match"], exclude_id=case["self_id"])
        assert pref == [tuple(e) for e in case["dups"]]


def _check_batch(dc, ids, offs, keys, queries, min_match, excl=None, cap=None, algo=_lib.ALGO_AUTO):
    d_q, d_off, max_len = tc.pack_queries(queries, DEV)
    C = len(ids)
    cap = cap or max(C, 1)
    d_ex = torch.tensor(excl, dtype=torch.int32, device=DEV) if excl is not None else None
    hits, n = dc.match(d_q, d_off, max_len, min_match, cap, d_exclude_ids=d_ex, algo=algo)
    torch.cuda.synchronize()
    hits, n = hits.cpu().numpy(), n.cpu().numpy()
    for qi, q in enumerate(queries):
        cnt, kth = oracle.match_kth_csr(np.asarray(q, dtype=np.float64), offs, keys, min_match)
        exp = sorted((int(ids[c]), int(cnt[c]), int(kth[c])) for c in range(C)
                     if cnt[c] >= min_match and (excl is None or ids[c] != excl[qi]))
        assert n[qi] == len(exp), (qi, n[qi], len(exp))
        got = sorted(tuple(int(x) for x in h) for h in hits[qi, :min(n[qi], cap)])
        if n[qi] > cap:                      # overflow: an arbitrary subset of the true hits is kept
            assert len(got) == cap and set(got) <= set(exp)
        else:
            assert got == exp
    return hits, n


@pytest.mark.parametrize("C,mean_len,Q,mm", [(300, 40, 9, 2), (2000, 200, 16, 2), (500, 200, 5, 1),
                                             (64, 12, 7, 3), (1000, 200, 4, 5), (17, 5, 3, 0),
                                             (1500, 200, 12, 6), (600, 200, 6, 9), (800, 200, 5, 40)])
def test_batched_match_vs_oracle(dc, C, mean_len, Q, mm):
    ids, offs, keys = synth.synth_timestamp_corpus(C, seed=C + mm, mean_len=mean_len, dup_frac=0.05,
                                                   frag_frac=0.05)
    dc.upload_csr(ids, offs, keys)
    queries = synth.synth_queries(ids, offs, keys, Q, seed=Q, mean_len=mean_len)
    queries[0] = np.concatenate([queries[0], queries[0][:7]])        # multiplicity
    if Q > 2:
        queries[2] = np.zeros(0)                                      # empty query
    _check_batch(dc, ids, offs, keys, queries, mm)
    excl = [int(ids[(7 * i) % C]) for i in range(Q)]
    _check_batch(dc, ids, offs, keys, queries, mm, excl=excl)
    if mm >= 1:       # an indexed handle answers EVERY min_match >= 1 from the index (> 5: count + kth fix-up)
        assert dc.index_stats()["indexed_rows"] == C
        _, n = _check_batch(dc, ids, offs, keys, queries, mm, excl=excl, algo=_lib.ALGO_INDEX)
        assert mm < 6 or int(n.max()) >= 1            # the duplicates of the synthetic corpus reach min_match
    # every sweep kernel gives the same hits (the per-call `algo` never changes results)
    for algo in (_lib.ALGO_Q1, _lib.ALGO_TILE, _lib.ALGO_JOIN):
        _check_batch(dc, ids, offs, keys, queries, mm, excl=excl, algo=algo)
        _check_batch(dc, ids, offs, keys, queries[:1], mm, algo=algo)


def test_ragged_rows_and_long_queries(dc):
    rng = np.random.default_rng(9)
    rows = []
    for v in range(200):
        L = int(rng.choice([0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 257, 1000]))
        rows.append((v + 10, np.round(rng.uniform(0, 500, L), 2).tolist()))
    dc.upload(rows)
    ids, offs, keys = tc.rows_to_csr(rows)
    queries = [np.round(rng.uniform(0, 500, n), 2) for n in (1, 16, 17, 300, 1500, 4095)]
    for mm in (1, 2, 4, 5, 6, 9):
        _check_batch(dc, ids, offs, keys, queries, mm)
        _check_batch(dc, ids, offs, keys, queries, mm, algo=_lib.ALGO_Q1)
        _check_batch(dc, ids, offs, keys, queries, mm, algo=_lib.ALGO_TILE)


def test_queries_longer_than_a_tile(dc):
    """find_duplicates has no length limit (the reference has none): > 4095 timestamps take the
    sorted-query path (batches: test_batches_with_queries_longer_than_a_tile)."""
    rng = np.random.default_rng(77)
    rows = []
    for v in range(300):
        L = int(rng.choice([0, 1, 5, 40, 300, 5000]))
        rows.append((v + 1, np.round(rng.uniform(0, 2000, L), 1).tolist()))
    dc.upload(rows)
    ids, offs, keys = tc.rows_to_csr(rows)
    for n in (4096, 5000, 12000):
        q = np.round(rng.uniform(0, 2000, n), 1)
        q[10:14] = [np.nan, -0.0, 0.0, q[9]]
        for mm in (0, 1, 2, 7, 300):
            cnt, kth = oracle.match_kth_csr(q, offs, keys, mm)
            exp = sorted((int(ids[c]), int(cnt[c]), int(kth[c])) for c in range(len(ids))
                         if cnt[c] >= mm and ids[c] != 5)
            assert dc.find_duplicates(q, mm, exclude_id=5, with_kth=True) == exp, (n, mm)


def test_batches_with_queries_longer_than_a_tile(dc):
    """db.py:87 puts no limit on len(new_timestamps), and neither do the batched calls: queries of
    4096 and 12000 timestamps in one batch with short, empty and exactly-4095 ones - every algorithm
    choice for the short ones, exclusions, min_match below / inside / above the index's range,
    an empty and a non-empty delta table, the hit lists and the per-shard top-k block."""
    rng = np.random.default_rng(78)
    rows = []
    for v in range(400):
        L = int(rng.choice([0, 1, 5, 40, 300, 2000]))
        rows.append((v + 1, np.round(rng.uniform(0, 2000, L), 1).tolist()))
    dc.upload(rows)
    lens = (4096, 50, 12000, 0, 4095, 300, 4097, 7)
    queries = [np.round(rng.uniform(0, 2000, n), 1) for n in lens]
    queries[0][10:14] = [np.nan, -0.0, 0.0, queries[0][9]]
    queries[5] = np.asarray((rows[40][1] + rows[41][1] + rows[42][1])[:300], dtype=np.float64)
    excl = [5, 6, 7, 8, 9, 41, 11, 12]
    d_q, d_off, max_len = tc.pack_queries(queries, DEV)
    d_ex = torch.tensor(excl, dtype=torch.int32, device=DEV)

    def expected(rows_, mm):                              # the oracle once per (table, min_match)
        ids, offs, keys = tc.rows_to_csr(rows_)
        out = []
        for q in queries:
            cnt, kth = oracle.match_kth_csr(np.asarray(q, dtype=np.float64), offs, keys, mm)
            out.append([(int(ids[c]), int(cnt[c]), int(kth[c])) for c in range(len(ids)) if cnt[c] >= mm])
        return out

    def check(exp, mm, algo, use_excl, cap):
        hits, n = dc.match(d_q, d_off, max_len, mm, cap, d_exclude_ids=d_ex if use_excl else None, algo=algo)
        torch.cuda.synchronize()
        hits, n = hits.cpu().numpy(), n.cpu().numpy()
        for qi in range(len(queries)):
            e = sorted(h for h in exp[qi] if not use_excl or h[0] != excl[qi])
            assert n[qi] == len(e), (mm, algo, qi, int(n[qi]), len(e))
            got = sorted(tuple(int(x) for x in h) for h in hits[qi, :min(n[qi], cap)])
            assert (got == e) if n[qi] <= cap else (len(got) == cap and set(got) <= set(e)), (mm, algo, qi)
    for mm in (0, 1, 2, 5, 7):
        exp = expected(rows, mm)
        for algo in (_lib.ALGO_AUTO, _lib.ALGO_TILE, _lib.ALGO_JOIN, _lib.ALGO_Q1) + ((_lib.ALGO_INDEX,) if mm >= 1 else ()):
            check(exp, mm, algo, False, len(rows))
            check(exp, mm, algo, True, 40)
    # rows replaced / added since the index build (delta table) are found by the long queries too
    rows2 = list(rows)
    rows2[3] = (rows[3][0], queries[2][100:160].tolist())
    rows2.append((999_001, queries[0][:50].tolist()))
    dc.upsert(rows2[3][0], rows2[3][1])
    dc.upsert(999_001, rows2[-1][1])
    for mm in (2, 6):
        exp = expected(rows2, mm)
        check(exp, mm, _lib.ALGO_AUTO, False, len(rows2))
        check(exp, mm, _lib.ALGO_TILE, True, len(rows2))
    # per-shard top-k block over such a batch
    K = 8
    exp = expected(rows2, 2)
    blk = dc.match_topk(d_q, d_off, max_len, 2, len(rows2), K)
    torch.cuda.synchronize()
    blk = blk.cpu().numpy()
    for qi in range(len(queries)):
        e = sorted(exp[qi], key=lambda h: (h[2], h[0], h[1]))
        want = e[:K] + [(-1, 0, tc.KTH_NEVER)] * (K - min(K, len(e)))
        assert [tuple(int(x) for x in r) for r in blk[qi, :K]] == want, qi
        assert int(blk[qi, K, 1]) == len(e)
    # The long queries' scratch is a tail of the CALLER's workspace - the call allocates nothing (VERDICT r4 item 7:
    # hipMalloc / hipFree on a match call synchronised the whole device).  Sized for one long query only (no key
    # count given), this batch of three is refused by name, with the bytes it needs; sized with the key count it runs.
    small = torch.empty(tc.workspace_bytes(len(queries), max_len), dtype=torch.uint8, device=DEV)
    oh = torch.empty((len(queries), 64, 3), dtype=torch.int32, device=DEV)
    on = torch.empty(len(queries), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="tvz_match_workspace_bytes_long"):       # (the library's own refusal, through the C ABI)
        _lib.check(dc.lib.tvz_match(dc._h, d_q.data_ptr(), d_off.data_ptr(), len(queries), max_len, 2, None, 64,
                                    oh.data_ptr(), on.data_ptr(), small.data_ptr(), small.numel(), _lib.ALGO_AUTO,
                                    torch.cuda.current_stream().cuda_stream))
    assert tc.workspace_bytes(len(queries), max_len, total_query_keys=d_q.numel()) > small.numel()
    right = torch.empty(tc.workspace_bytes(len(queries), max_len, total_query_keys=d_q.numel()), dtype=torch.uint8, device=DEV)
    h1, n1 = dc.match(d_q, d_off, max_len, 2, len(rows2), workspace=right)
    h2, n2 = dc.match(d_q, d_off, max_len, 2, len(rows2))
    assert (n1 == n2).all() and sorted(map(tuple, h1[2, :int(n1[2])].tolist())) == sorted(map(tuple, h2[2, :int(n2[2])].tolist()))


def test_a_long_query_batch_does_not_stall_lookups_on_another_stream(dc):
    """A batch with queries of more than 4,095 timestamps used to hipMalloc / hipFree its scratch and synchronise per
    long query: every other stream's work waited for it.  Now it is one read-back of the offsets and a chain of
    launches.  A second thread keeps answering single lookups (tvz_find_duplicates: ~20 us) while 40 such batches
    run: none of them may take long."""
    import threading
    import time
    rng = np.random.default_rng(5)
    rows = [(v + 1, np.round(rng.uniform(0, 5000, 200), 1).tolist()) for v in range(6000)]
    dc.upload(rows)
    queries = [np.round(rng.uniform(0, 5000, n), 1) for n in (6000, 200, 9000, 150, 5000, 4096)]
    d_q, d_off, max_len = tc.pack_queries(queries, DEV)
    ws = torch.empty(tc.workspace_bytes(len(queries), max_len, total_query_keys=d_q.numel()), dtype=torch.uint8, device=DEV)
    st = torch.cuda.Stream(DEV)
    probe = np.asarray(rows[17][1][:60])
    for _ in range(20):
        dc.find_duplicates(probe, 2)
    quiet = []
    for _ in range(300):
        t = time.perf_counter(); dc.find_duplicates(probe, 2); quiet.append(time.perf_counter() - t)
    stop, lat = threading.Event(), []

    def lookups():
        while not stop.is_set():
            t = time.perf_counter(); dc.find_duplicates(probe, 2); lat.append(time.perf_counter() - t)
    th = threading.Thread(target=lookups)
    th.start()
    ref = None
    for i in range(40):
        h, n = dc.match(d_q, d_off, max_len, 2, 512, workspace=ws, stream=st)
        st.synchronize()
        ref = n.clone() if ref is None else ref
        assert (n == ref).all()
    stop.set()
    th.join()
    assert len(lat) > 100
    # a long batch's kernels share the GPU with the lookups (that is allowed to cost a few hundred microseconds);
    # a device-wide synchronisation per long query was milliseconds per lookup
    assert float(np.median(lat)) < 20 * float(np.median(quiet)) + 2e-4, (np.median(lat), np.median(quiet))
    assert float(np.percentile(lat, 99)) < 5e-3, np.percentile(lat, 99)


def test_hit_list_overflow_reports_true_count(dc):
    ids, offs, keys = synth.synth_timestamp_corpus(400, seed=2, mean_len=30)
    dc.upload_csr(ids, offs, keys)
    d_q, d_off, max_len = tc.pack_queries([keys[:60]], DEV)
    hits, n = dc.match(d_q, d_off, max_len, 0, cap=10)   # min_match 0: every row is a hit
    torch.cuda.synchronize()
    assert int(n[0]) == 400
    assert (hits[0, :, 0] >= 1).all()


def past_the_stage_case():
    """70,000 rows that are ALL hits of 8 queries: row i (video id i) holds six shared timestamps and one of its own;
    query j is the shared six, rotated by j, with two values that match nothing put in at places that depend on j.  A sweep gives a query
    256 blocks of 16 row groups, 274 rows each here, and a block stages 256 hits in LDS: every block goes past its stage.
    -> (ids, offsets, keys, queries, exclude ids, {min_match: [kth per query]})."""
    C, Q = 70_000, 8
    assert C > 256 * 256
    shared = [10.0, 20.0, 30.0, 40.0, 50.0, 60.0]
    ids = np.arange(1, C + 1, dtype=np.int32)
    keys = np.empty((C, 7))
    keys[:, :6] = shared
    keys[:, 6] = 1000.0 + ids
    queries = []
    for j in range(Q):
        q = shared[j % 6:] + shared[:j % 6]
        q.insert(j % 3, -1.0 - j)
        q.insert(3 + j % 5, -100.0 - j)
        queries.append(q)
    kth = {mm: [[i for i, v in enumerate(q) if v in shared][mm - 1] for q in queries] for mm in (1, 3, 6)}
    assert all(len(set(k)) > 1 for k in kth.values())         # kth differs between the queries
    return ids, np.arange(C + 1, dtype=np.int64) * 7, keys.reshape(-1), queries, [1 + 1000 * j for j in range(Q)], kth


def check_past_the_stage(run, ids, excl, kth):
    """run(min_match, cap) -> (hits [Q, cap, 3], n [Q]) as numpy arrays."""
    C = len(ids)
    for mm in (1, 3, 6):                         # two smallest positions / five smallest / count + the fix-up walk
        hits, n = run(mm, C)
        for j, e in enumerate(excl):
            assert n[j] == C - 1, (mm, j, n[j])
            h = hits[j, :C - 1]
            assert np.array_equal(np.sort(h[:, 0]), ids[ids != e]), (mm, j)
            assert (h[:, 1] == 6).all() and (h[:, 2] == kth[mm][j]).all(), (mm, j)
    hits, n = run(3, 1000)                       # the flush clipped to cap
    for j, e in enumerate(excl):
        assert n[j] == C - 1, (j, n[j])
        h = hits[j]
        assert len(np.unique(h[:, 0])) == 1000 and (h[:, 0] >= 1).all() and (h[:, 0] <= C).all() and (h[:, 0] != e).all(), j
        assert (h[:, 1] == 6).all() and (h[:, 2] == kth[3][j]).all(), j


def test_block_hit_list_past_its_stage(dc):
    ids, offs, keys, queries, excl, kth = past_the_stage_case()
    dc.upload_csr(ids, offs, keys)
    d_q, d_off, max_len = tc.pack_queries(queries, DEV)
    d_ex = torch.tensor(excl, dtype=torch.int32, device=DEV)

    def run(mm, cap):
        hits, n = dc.match(d_q, d_off, max_len, mm, cap, d_exclude_ids=d_ex, algo=_lib.ALGO_Q1)
        torch.cuda.synchronize()
        return hits.cpu().numpy(), n.cpu().numpy()
    check_past_the_stage(run, ids, excl, kth)


def test_upsert_replaces_first_row_and_compacts(dc):
    dc.upload([(1, [1.0, 2.0]), (2, [3.0, 4.0]), (1, [9.0])])     # duplicate video_id rows allowed
    assert dc.find_duplicates([9.0, 1.0], 1) == [(1, 1), (1, 1)]
    dc.upsert(1, [5.0, 6.0, 7.0])                                    # replaces the FIRST row of id 1
    assert dc.find_duplicates([5.0, 6.0, 9.0], 1) == [(1, 1), (1, 2)]
    prefix = []
    for i in range(3000):                                            # growing prefix, as app.py:234
        prefix.append(100.0 + i)
        if i % 50 == 0:
            dc.upsert(7, prefix)
    dc.upsert(7, prefix)
    n_rows, n_keys, arena = dc.stats()
    assert n_rows == 4 and n_keys == 3 + 2 + 1 + 3000
    assert arena < 4 * n_keys + 8192                                # dead prefixes were collected
    assert dc.find_duplicates(prefix[-3:], 3) == [(7, 3)]
    dc.clear()
    assert dc.stats()[0] == 0 and dc.find_duplicates([1.0], 0) == []


def test_topk_order_and_padding(dc):
    ids, offs, keys = synth.synth_timestamp_corpus(3000, seed=4, mean_len=60, dup_frac=0.05)
    dc.upload_csr(ids, offs, keys)
    queries = synth.synth_queries(ids, offs, keys, 6, seed=3, mean_len=60)
    d_q, d_off, max_len = tc.pack_queries(queries, DEV)
    for cap in (3000, 40):
        hits, n = dc.match(d_q, d_off, max_len, 1, cap)
        for k in (1, 8, 64):
            top = tc.topk(hits, n, k).cpu().numpy()
            hh, nn = hits.cpu().numpy(), n.cpu().numpy()
            for qi in range(len(queries)):
                lst = [tuple(int(x) for x in h) for h in hh[qi, :min(nn[qi], cap)]]
                exp = sorted(lst, key=lambda h: (h[2], h[0], h[1]))[:k]
                exp += [(-1, 0, NEVER)] * (k - len(exp))
                assert [tuple(int(x) for x in r) for r in top[qi]] == exp


def test_topk_merges_gathered_shards(dc):
    rng = np.random.default_rng(1)
    R, Q, k = 4, 5, 8
    lists = np.full((R, Q, k, 3), 0, dtype=np.int32)
    for r in range(R):
        for q in range(Q):
            m = int(rng.integers(0, k + 1))
            ent = sorted(((int(rng.integers(0, 6)), int(rng.integers(1, 10**6)), int(rng.integers(1, 9)))
                          for _ in range(m)))
            for j in range(k):
                lists[r, q, j] = (ent[j][1], ent[j][2], ent[j][0]) if j < m else (-1, 0, NEVER)
    out = tc.topk(torch.from_numpy(lists).to(DEV), None, k).cpu().numpy()
    for q in range(Q):
        flat = [tuple(int(x) for x in e) for r in range(R) for e in lists[r, q] if e[0] >= 0]
        exp = sorted(flat, key=lambda h: (h[2], h[0], h[1]))[:k]
        exp += [(-1, 0, NEVER)] * (k - len(exp))
        assert [tuple(int(x) for x in r) for r in out[q]] == exp


@pytest.mark.parametrize("R,k", [(8, 16), (16, 64), (3, 1), (8, 40), (20, 64)])
def test_merge_of_gathered_rank_blocks(dc, R, k):
    """tvz_topk_merge over [R, Q, k+1, 3] blocks as the all-gather delivers them: order (kth, video_id, count),
    padding, totals = sum of |n| negated when any shard overflowed; ties of hundreds of entries in one kth (true
    duplicates on every rank).  The dispatch (launch_topk_lists): up to 16 ranks and k <= 64 - the first four
    shapes here - are a k-way merge of the SORTED blocks (ts_topk_merge_sorted_kernel); (20, 64) is 1280 entries,
    more than the one-wave kernel's 1024, and goes to the block kernel (ts_topk_kernel).  The one-wave kernel's
    merges (more than 16 ranks, R*k <= 1024) and its k-rounds path are in tests/test_topk_edges_gpu.py."""
    rng = np.random.default_rng(R * 100 + k)
    Q = 37
    g = np.zeros((R, Q, k + 1, 3), dtype=np.int32)
    exp_tot = []
    for q in range(Q):
        tot, over = 0, False
        style = q % 4           # 0: spread kth, 1: everything kth == 3 (a big tie), 2: sparse, 3: empty
        for r in range(R):
            m = {0: k, 1: k, 2: int(rng.integers(0, 3)), 3: 0}[style]
            ent = []
            for _ in range(m):
                kth = 3 if style == 1 else int(rng.integers(0, 50))
                ent.append((kth, int(rng.integers(0, 2000)), int(rng.integers(1, 9))))
            ent.sort()
            for j in range(k):
                g[r, q, j] = (ent[j][1], ent[j][2], ent[j][0]) if j < m else (-1, 0, NEVER)
            n = m + int(rng.integers(0, 5))
            neg = bool(rng.random() < 0.15) and n > 0
            g[r, q, k] = (-1, -n if neg else n, NEVER)
            tot += n
            over = over or neg
        exp_tot.append(-tot if over else tot)
    merged, totals = tc.topk_merge(torch.from_numpy(g).to(DEV), k)
    merged, totals = merged.cpu().numpy(), totals.cpu().numpy()
    assert totals.tolist() == exp_tot
    for q in range(Q):
        flat = [tuple(int(x) for x in e) for r in range(R) for e in g[r, q, :k] if e[0] >= 0]
        exp = sorted(flat, key=lambda h: (h[2], h[0], h[1]))[:k]
        exp += [(-1, 0, NEVER)] * (k - len(exp))
        assert [tuple(int(x) for x in r) for r in merged[q]] == exp, q


def test_every_producer_of_rank_blocks_meets_the_sorted_merge_precondition(dc):
    """tvz_topk_merge (<= 16 ranks, k <= 64) is a k-way merge of SORTED lists: every gathered block must be in
    ascending (kth, video_id, count) order with its padding last (a block that is not would be
    mis-merged silently).  Here every producer of such a block in the library is asked for one - the lookup that
    keeps the top-k (block kernel, two queries per block, one wave per query), with a delta table behind it (the
    mode-3 pair merge), the sweeps + the select kernels for k <= 16 and k > 16, k beyond the fused lookup's 64, a
    batch with a refused query - each block is checked for the order, and the blocks of ALL producers, stacked as
    ranks, are merged and compared with a plain sort."""
    rng = np.random.default_rng(12)
    grid = np.arange(1, 3001) / 4.0
    rows = [(v + 1, rng.choice(grid, size=int(rng.integers(10, 60)), replace=False).tolist()) for v in range(5000)]
    dc.upload(rows)
    Q = 33
    queries = [rng.choice(grid, size=int(rng.integers(20, 120)), replace=False) for _ in range(Q)]
    queries[4] = np.zeros(0)
    d_q, d_off, max_len = tc.pack_queries(queries, DEV)

    def sorted_ok(blk, k):
        for q in range(blk.shape[0]):
            ent = [tuple(int(x) for x in e) for e in blk[q, :k]]
            real = [e for e in ent if e[0] >= 0]
            assert ent[:len(real)] == real, ("padding in the middle", q)
            assert real == sorted(real, key=lambda h: (h[2], h[0], h[1])), ("not ascending", q)

    for k in (8, 40):
        blocks = {}
        for name, algo in (("block", _lib.ALGO_NO_WAVE | _lib.ALGO_NO_PAIR), ("pair", _lib.ALGO_PAIR), ("wave", _lib.ALGO_WAVE),
                           ("tile+select", _lib.ALGO_TILE), ("join+select", _lib.ALGO_JOIN)):
            blocks[name] = dc.match_topk(d_q, d_off, max_len, 2, 4096, k, algo=algo).cpu().numpy()
        # a refused query: max_query_len understated for query 7 -> padding + the poisoned total, still a valid list
        short = max(len(q) for i, q in enumerate(queries) if i != 7)
        if len(queries[7]) <= short:
            queries7 = np.concatenate([queries[7], rng.choice(grid, size=short + 5 - len(queries[7]))])
            d_q7, d_off7, _ = tc.pack_queries(queries[:7] + [queries7] + queries[8:], DEV)
        else:
            d_q7, d_off7 = d_q, d_off
        blocks["refused"] = dc.match_topk(d_q7, d_off7, short, 2, 4096, k, algo=_lib.ALGO_NO_WAVE).cpu().numpy()
        assert tuple(blocks["refused"][7, 0]) == (-1, 0, NEVER) and blocks["refused"][7, k, 1] == np.iinfo(np.int32).min
        for name, b in blocks.items():
            sorted_ok(b, k)
            if name != "refused":
                assert (b == blocks["block"]).all(), name
        g = np.stack([blocks[n] for n in ("block", "wave", "tile+select", "refused")])
        merged, totals = tc.topk_merge(torch.from_numpy(g).to(DEV), k)
        merged, totals = merged.cpu().numpy(), totals.cpu().numpy()
        for q in range(Q):
            flat = [tuple(int(x) for x in e) for r in range(g.shape[0]) for e in g[r, q, :k] if e[0] >= 0]
            exp = sorted(flat, key=lambda h: (h[2], h[0], h[1]))[:k]
            exp += [(-1, 0, NEVER)] * (k - len(exp))
            assert [tuple(int(x) for x in r) for r in merged[q]] == exp, (k, q)
            # totals by the header's rule (tvz.h, tvz_topk_merge and tvz_match_tol_sharded's paragraph on refused queries)
            assert int(totals[q]) == topk_ref.merge([[tuple(int(x) for x in e) for e in g[r, q]] for r in range(g.shape[0])], k)[1], (k, q)
        assert int(totals[7]) == -(2**31 - 1)               # three true counts + the refused rank's INT32_MIN: saturated, negated
    # with a delta table: the lookup's block and the delta sweep's are merged pairwise (mode 3) - still sorted;
    # and k beyond the fused lookup's 64 (the unfused pipeline)
    for j in range(40):
        dc.upsert(rows[j][0], rows[j][1][::2])
        dc.upsert(900_000 + j, queries[j % Q][:30].tolist())
    assert dc.index_stats()["delta_rows"] > 0
    for k, algo in ((8, 0), (40, 0), (8, _lib.ALGO_WAVE), (100, 0)):
        sorted_ok(dc.match_topk(d_q, d_off, max_len, 2, 4096, k, algo=algo).cpu().numpy(), k)


def test_concurrent_find_duplicates_threads(dc):
    import threading
    ids, offs, keys = synth.synth_timestamp_corpus(1500, seed=8, mean_len=50, dup_frac=0.05)
    dc.upload_csr(ids, offs, keys)
    queries = synth.synth_queries(ids, offs, keys, 8, seed=5, mean_len=50)
    exp = []
    for q in queries:
        cnt, kth = oracle.match_kth_csr(q, offs, keys, 2)
        exp.append(sorted((int(ids[c]), int(cnt[c])) for c in range(len(ids)) if cnt[c] >= 2))
    errs = []

    def work(i):
        try:
            for _ in range(20):
                assert dc.find_duplicates(queries[i], 2) == exp[i]
        except Exception as e:  # pragma: no cover
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    [t.start() for t in th]; [t.join() for t in th]
    assert not errs


def test_config3_size_round_trip_property(dc):
    """BASELINE config 3 size (1 query vs 5k videos x ~200 cuts): every row is found by its own
    timestamps with count == len(row), kth == min_match-1 (size-independent property)."""
    ids, offs, keys = synth.synth_timestamp_corpus(5000, seed=synth.CORPUS_SEED)
    dc.upload_csr(ids, offs, keys)
    for c in (0, 17, 4999):
        row = keys[offs[c]:offs[c + 1]]
        hits = dc.find_duplicates(row, min_match=len(row), with_kth=True)
        assert (int(ids[c]), len(row), len(row) - 1) in hits
        cnt, kth = oracle.match_kth_csr(row, offs, keys, 2)
        exp = sorted((int(ids[i]), int(cnt[i]), int(kth[i])) for i in range(5000) if cnt[i] >= 2)
        assert dc.find_duplicates(row, 2, with_kth=True) == exp


def test_sharded_pipeline_on_one_gpu(dc):
    """The N-rank data path (shard -> match -> topk_shard -> [all-gather] -> topk_merge) with the
    real HIP backend, the ranks being R corpus handles on this one GPU; the gather is a stack."""
    from tvidz_amd import sharded
    C, Q, k, mm = 3000, 12, 16, 2
    ids, offs, keys = synth.synth_timestamp_corpus(C, seed=31, mean_len=60, dup_frac=0.03)
    queries = synth.synth_queries(ids, offs, keys, Q, seed=4, mean_len=60)
    d_q, d_off, max_len = tc.pack_queries(queries, DEV)
    excl = torch.tensor([int(ids[(5 * i) % C]) for i in range(Q)], dtype=torch.int32, device=DEV)
    for R in (1, 3, 8):
        blocks = []
        for r in range(R):
            s_ids, s_offs, s_keys = sharded.shard_csr(ids, offs, keys, r, R)
            shard = tc.DeviceCorpus(0)
            shard.upload_csr(s_ids, s_offs, s_keys)
            hits, n = shard.match(d_q, d_off, max_len, mm, 64, d_exclude_ids=excl)
            blocks.append(tc.topk_shard(hits, n, k))
            torch.cuda.synchronize()
            shard.close()
        merged, totals = tc.topk_merge(torch.stack(blocks).contiguous(), k)
        merged, totals = merged.cpu().numpy(), totals.cpu().numpy()
        for qi, q in enumerate(queries):
            cnt, kth = oracle.match_kth_csr(q, offs, keys, mm)
            rows = [(int(ids[c]), int(cnt[c]), int(kth[c])) for c in range(C)
                    if cnt[c] >= mm and ids[c] != int(excl[qi])]
            assert int(totals[qi]) == len(rows)          # cap 64 is never exceeded per shard here
            exp = sorted(rows, key=lambda h: (h[2], h[0], h[1]))[:k]
            exp += [(-1, 0, NEVER)] * (k - len(exp))
            assert [tuple(int(x) for x in r) for r in merged[qi]] == exp, (R, qi)
        v = sharded.verdicts_from_topk(merged)
        for qi, q in enumerate(queries):
            cnt, kth = oracle.match_kth_csr(q, offs, keys, mm)
            kstar, dup = oracle.verdict_from_kth(ids, kth, self_id=int(excl[qi]))
            if not v[qi][2]:
                assert (v[qi][0], v[qi][1]) == (kstar, dup)


def test_opt_in_alignment_score_detects_a_cut_shifted_copy(dc):
    """tvz_align is an extra (no reference counterpart): checked against its own restatement,
    and on the configs[0] situation the exact matcher rejects (a cut-shifted copy)."""
    rng = np.random.default_rng(12)
    base = np.sort(np.round(rng.uniform(0, 300, 40), 4))
    rows = [(1, base.tolist()), (2, (base + 7 / 30).tolist()), (3, np.sort(rng.uniform(0, 300, 35)).tolist()),
            (4, []), (5, (base[:20] - 2.5).tolist() + [float("nan")]), (6, [5.0, 5.0, 5.0])]
    dc.upload(rows)
    for eps, mo in ((0.1, 10.0), (1 / 30, 5.0), (0.5, 60.0)):
        got = [tuple(int(x) for x in r) for r in dc.align(base, eps=eps, max_offset=mo)]
        assert got == oracle.align_py(rows, base, eps, mo), (eps, mo)
    res = {r[0]: r for r in dc.align(base, eps=1 / 30, max_offset=5.0)}
    assert res[1][2] == 0 and res[1][3] == 40                 # itself: no shift, all cuts
    assert res[2][2] == 7 and res[2][3] >= 38                 # shifted by 7 frames: found
    assert dc.find_duplicates(base, 2) == [(1, 40)]           # exact verdict unchanged: only itself
    assert res[3][3] <= 6 and res[4][3] == 0
    jacc = res[2][3] / (len(base) + res[2][1] - res[2][3])
    assert jacc > 0.9


def test_property_random_small_corpora_special_values(dc):
    """Seeded property test: tiny key alphabets force heavy collisions, multiplicities, duplicate
    video ids, special values; every (min_match, exclude) combination must equal the oracle."""
    rng = np.random.default_rng(2025)
    alphabet = np.array([0.0, -0.0, 1.0, 1.5, 2.0, 1e-300, 5e-324, 1e300, np.inf, -np.inf, np.nan,
                         12.3457, 12.3456, 123.457, 0.1 + 0.2, 0.3, -7.25, 4503599627370497.0])
    for trial in range(25):
        C = int(rng.integers(1, 40))
        rows = []
        for c in range(C):
            L = int(rng.integers(0, 12))
            rows.append((int(rng.integers(1, 15)), alphabet[rng.integers(0, len(alphabet), L)].tolist()))
        dc.upload(rows)
        ids, offs, keys = tc.rows_to_csr(rows)
        Q = int(rng.integers(1, 20))
        queries = [alphabet[rng.integers(0, len(alphabet), int(rng.integers(0, 25)))] for _ in range(Q)]
        for mm in (-1, 0, 1, 2, 3, 5, 6, 7):
            excl = [int(rng.integers(1, 15)) for _ in range(Q)] if trial % 2 else None
            _check_batch(dc, ids, offs, keys, queries, mm, excl=excl)
            _check_batch(dc, ids, offs, keys, queries, mm, excl=excl,
                         algo=(_lib.ALGO_Q1, _lib.ALGO_TILE, _lib.ALGO_JOIN)[trial % 3])
            for q0 in queries[:3]:          # the one-launch host path, every min_match
                exp = sorted(h for h in oracle.find_duplicates_c(rows, q0.tolist(), mm))
                assert dc.find_duplicates(q0, mm) == exp, (trial, mm)
        q0 = queries[0]
        assert dc.find_duplicates(q0, 1) == sorted(oracle.find_duplicates_c(rows, q0.tolist(), 1))


def test_upserts_concurrent_with_matches(dc):
    """app.py:234-235 from many upload threads: add_timestamps (upsert) races find_duplicates; every
    answer must be consistent with SOME prefix state of the mutating rows (never garbage)."""
    import threading
    ids, offs, keys = synth.synth_timestamp_corpus(800, seed=6, mean_len=40)
    dc.upload_csr(ids, offs, keys)
    base = keys[offs[3]:offs[4]].copy()                     # row of video ids[3]
    stop = threading.Event()
    errs = []

    def writer(vid):
        try:
            prefix = []
            for i in range(300):
                prefix.append(1000.0 * (vid - 90000) + 1e6 + i * 0.5)
                dc.upsert(vid, prefix)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    def reader():
        try:
            while not stop.is_set():
                got = dict(dc.find_duplicates(base, 2))
                assert got.get(int(ids[3])) == len(base)    # the static row is always found intact
                for v in (90001, 90002, 90003):
                    b = 1000.0 * (v - 90000) + 1e6
                    got2 = dict(dc.find_duplicates([b, b + 0.5, b + 1.0], 1))
                    assert set(got2) <= {v} and got2.get(v, 0) in (0, 1, 2, 3)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    rd = [threading.Thread(target=reader) for _ in range(3)]
    wr = [threading.Thread(target=writer, args=(v,)) for v in (90001, 90002, 90003)]
    [t.start() for t in rd + wr]
    [t.join() for t in wr]
    stop.set()
    [t.join() for t in rd]
    assert not errs, errs
    for v in (90001, 90002, 90003):
        assert dc.find_duplicates([1000.0 * (v - 90000) + 1e6 + 0.5 * i for i in range(300)], 300) == [(v, 300)]


def test_wrong_max_query_len_is_flagged_not_truncated(dc):
    dc.upload([(1, [1.0, 2.0, 3.0])])
    queries = [np.arange(300, dtype=np.float64)] * 16           # 4800 entries for one 16-query tile
    d_q, d_off, max_len = tc.pack_queries(queries, DEV)
    hits, n = dc.match(d_q, d_off, 200, 1, 8, algo=_lib.ALGO_TILE)   # lying about the bound
    torch.cuda.synchronize()
    assert (n.cpu().numpy() == np.iinfo(np.int32).min).all()
    hits, n = dc.match(d_q, d_off, max_len, 1, 8)                # honest bound: correct answer
    torch.cuda.synchronize()
    assert (n.cpu().numpy() == 1).all() and (hits[:, 0, 1].cpu().numpy() == 3).all()


@pytest.mark.parametrize("C,mean_len,Q,mm", [(1500, 60, 40, 2), (900, 200, 130, 2), (400, 30, 300, 1),
                                             (2500, 40, 257, 2), (64, 12, 33, 0)])
def test_hash_join_path_vs_oracle_and_tile_kernel(dc, C, mean_len, Q, mm):
    """Q >= 32 with min_match <= 2 takes the hash-join kernels; same hits as the oracle and as the
    LDS tile kernel (both forced through the per-call `algo`)."""
    ids, offs, keys = synth.synth_timestamp_corpus(C, seed=C + Q, mean_len=mean_len, dup_frac=0.05,
                                                   frag_frac=0.05)
    dc.upload_csr(ids, offs, keys)
    queries = synth.synth_queries(ids, offs, keys, Q, seed=Q + 1, mean_len=mean_len)
    queries[0] = np.concatenate([queries[0], queries[0][:9]])       # multiplicity
    queries[3] = np.zeros(0)
    queries[5] = queries[4].copy()                                   # the same video twice in a batch
    excl = [int(ids[(11 * i) % C]) for i in range(Q)]
    h1, n1 = _check_batch(dc, ids, offs, keys, queries, mm, excl=excl, algo=_lib.ALGO_JOIN)
    _check_batch(dc, ids, offs, keys, queries, mm, cap=7, algo=_lib.ALGO_JOIN)   # overflow: true counts kept
    h0, n0 = _check_batch(dc, ids, offs, keys, queries, mm, excl=excl, algo=_lib.ALGO_TILE)
    assert (n0 == n1).all()


def test_hash_join_and_q1_flag_wrong_bound(dc):
    dc.upload([(1, [1.0, 2.0, 3.0])])
    queries = [np.arange(50, dtype=np.float64)] * 40
    d_q, d_off, max_len = tc.pack_queries(queries, DEV)
    hits, n = dc.match(d_q, d_off, 20, 1, 8, algo=_lib.ALGO_JOIN)
    torch.cuda.synchronize()
    assert (n.cpu().numpy() < 0).all()
    hits, n = dc.match(d_q, d_off, max_len, 1, 8, algo=_lib.ALGO_JOIN)
    torch.cuda.synchronize()
    assert (n.cpu().numpy() == 1).all() and (hits[:, 0, 1].cpu().numpy() == 3).all()
    # the per-query sweep sizes its LDS table from max_query_len: a 2000-key query against a
    # table sized for 20 keys is flagged, not truncated
    big = [np.arange(2000, dtype=np.float64)] * 2
    d_q, d_off, max_len = tc.pack_queries(big, DEV)
    hits, n = dc.match(d_q, d_off, 20, 1, 8, algo=_lib.ALGO_Q1)
    torch.cuda.synchronize()
    assert (n.cpu().numpy() == np.iinfo(np.int32).min).all()
    hits, n = dc.match(d_q, d_off, max_len, 1, 8, algo=_lib.ALGO_Q1)
    torch.cuda.synchronize()
    assert (n.cpu().numpy() == 1).all() and (hits[:, 0, 1].cpu().numpy() == 3).all()
    # the join without its tables is refused loudly when asked for explicitly
    small_ws = torch.empty(1024, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        dc.match(d_q, d_off, max_len, 1, 8, algo=_lib.ALGO_JOIN, workspace=small_ws)


def test_shard_overflow_is_signalled_by_negative_totals(dc):
    ids, offs, keys = synth.synth_timestamp_corpus(600, seed=3, mean_len=30)
    dc.upload_csr(ids, offs, keys)
    d_q, d_off, max_len = tc.pack_queries([keys[:40], keys[100:140]], DEV)
    hits, n = dc.match(d_q, d_off, max_len, 0, cap=50)          # min_match 0: 600 hits per query > cap
    block = tc.topk_shard(hits, n, 8)
    merged, totals = tc.topk_merge(block.unsqueeze(0).contiguous(), 8)
    torch.cuda.synchronize()
    assert block[:, 8, 1].cpu().tolist() == [-600, -600]
    assert totals.cpu().tolist() == [-600, -600]
    hits, n = dc.match(d_q, d_off, max_len, 0, cap=600)         # enough room: positive again
    merged, totals = tc.topk_merge(tc.topk_shard(hits, n, 8).unsqueeze(0).contiguous(), 8)
    assert totals.cpu().tolist() == [600, 600]


def test_match_topk_one_call_equals_match_then_topk(dc):
    """tvz_match_topk (sweep + histogram-select top-k behind one call, hit lists in the caller's
    workspace) == tvz_match followed by tvz_topk_shard == the oracle's ordering, for every kernel,
    for long lists (kth histogram path), ties inside one kth bin, and overflowing capacities."""
    C, Q, mm = 6000, 24, 1
    rng = np.random.default_rng(21)
    grid = np.arange(1, 2001) / 8.0                       # a small alphabet: thousands of hits per query
    rows = []
    for c in range(C):
        r = rng.choice(grid, size=int(rng.integers(5, 40)), replace=False)
        if rng.random() < 0.5:
            r = np.append(r, 777.125)                      # half the rows share one key: a huge kth tie
        rows.append((c + 1, r.tolist()))
    dc.upload(rows)
    ids, offs, keys = tc.rows_to_csr(rows)
    queries = [rng.choice(grid, size=int(rng.integers(20, 160)), replace=False) for _ in range(Q)]
    queries[1] = np.array([777.125] * 3)                  # every hit has kth == 0: ~3000 ties in one bin
    queries[2] = np.zeros(0)
    d_q, d_off, max_len = tc.pack_queries(queries, DEV)
    excl = torch.tensor([int(ids[(5 * i) % C]) for i in range(Q)], dtype=torch.int32, device=DEV)
    exp_rows = []
    for qi, q in enumerate(queries):
        cnt, kth = oracle.match_kth_csr(q, offs, keys, mm)
        exp_rows.append([(int(ids[c]), int(cnt[c]), int(kth[c])) for c in range(C)
                         if cnt[c] >= mm and ids[c] != int(excl[qi])])
    assert len(exp_rows[1]) > 2500 and len({r[2] for r in exp_rows[1]}) == 1
    assert max(len(r) for r in exp_rows) > 1500          # long enough for the histogram path
    for algo in (_lib.ALGO_AUTO, _lib.ALGO_Q1, _lib.ALGO_TILE, _lib.ALGO_JOIN):
        for k, cap in ((16, C), (1, C), (64, C), (16, 300), (256, C), (700, C),   # k > 256: the wide select
                       (16, 1024), (64, 1025), (16, 256), (8, 512)):         # list lengths at the one-wave kernel's limits
            ws = torch.empty(tc.workspace_bytes(Q, max_len, cap, k), dtype=torch.uint8, device=DEV)
            out = dc.match_topk(d_q, d_off, max_len, mm, cap, k, d_exclude_ids=excl, workspace=ws, algo=algo)
            torch.cuda.synchronize()
            out = out.cpu().numpy()
            for qi in range(Q):
                rows = exp_rows[qi]
                tot = int(out[qi, k, 1])
                assert tuple(out[qi, k][[0, 2]]) == (-1, NEVER)
                if len(rows) <= cap:
                    assert tot == len(rows)
                    exp = sorted(rows, key=lambda h: (h[2], h[0], h[1]))[:k]
                    exp += [(-1, 0, NEVER)] * (k - len(exp))
                    assert [tuple(int(x) for x in r) for r in out[qi, :k]] == exp, (algo, k, cap, qi)
                else:
                    assert tot == -len(rows)             # overflow is signalled, entries are real hits
                    got = [tuple(int(x) for x in r) for r in out[qi, :k] if r[0] >= 0]
                    assert set(got) <= set(rows) and len(got) == min(k, cap)
    with pytest.raises(RuntimeError, match="workspace"):
        dc.match_topk(d_q, d_off, max_len, mm, C, 16, workspace=torch.empty(4096, dtype=torch.uint8, device=DEV))


def test_two_threads_run_hash_joins_concurrently(dc):
    """two callers on different streams used to be handed the same hash-join
    tables.  Scratch is now the caller's workspace: concurrent join batches stay exact."""
    import threading
    C, Q = 3000, 96
    ids, offs, keys = synth.synth_timestamp_corpus(C, seed=5, mean_len=60, dup_frac=0.05)
    dc.upload_csr(ids, offs, keys)
    sets = [synth.synth_queries(ids, offs, keys, Q, seed=100 + t, mean_len=60) for t in range(2)]
    exp = []
    for qs in sets:
        e = []
        for q in qs:
            cnt, kth = oracle.match_kth_csr(q, offs, keys, 2)
            e.append(sorted((int(ids[c]), int(cnt[c]), int(kth[c])) for c in range(C) if cnt[c] >= 2))
        exp.append(e)
    errs = []

    def work(t):
        try:
            st = torch.cuda.Stream()
            d_q, d_off, max_len = tc.pack_queries(sets[t], DEV)
            ws = torch.empty(tc.workspace_bytes(Q, max_len), dtype=torch.uint8, device=DEV)
            hits = torch.empty((Q, C, 3), dtype=torch.int32, device=DEV)
            n = torch.empty(Q, dtype=torch.int32, device=DEV)
            torch.cuda.synchronize()
            for _ in range(25):
                dc.match(d_q, d_off, max_len, 2, C, out_hits=hits, out_n=n, stream=st, workspace=ws,
                         algo=_lib.ALGO_JOIN)
                st.synchronize()
                hh, nn = hits.cpu().numpy(), n.cpu().numpy()
                for qi in range(Q):
                    assert sorted(map(tuple, hh[qi, :nn[qi]].tolist())) == exp[t][qi], (t, qi)
        except Exception as e:  # pragma: no cover
            errs.append(e)
    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    [t.start() for t in th]; [t.join() for t in th]
    assert not errs, errs


def test_upsert_is_stream_ordered_and_read_your_writes(dc):
    """tvz_corpus_upsert returns without draining matches in flight; a match enqueued after it
    (any stream) sees the new row; negative video ids are refused (they mark padding)."""
    ids, offs, keys = synth.synth_timestamp_corpus(4000, seed=12, mean_len=80)
    dc.upload_csr(ids, offs, keys)
    d_q, d_off, max_len = tc.pack_queries([np.arange(50) * 0.25 + 9e5], DEV)
    st = torch.cuda.Stream()
    prefix = []
    for i in range(60):
        prefix.append(9e5 + 0.25 * i)
        dc.upsert(777777, prefix)
        got = dc.find_duplicates(prefix, 1)
        assert got == [(777777, len(prefix))], i
        hits, n = dc.match(d_q, d_off, max_len, 1, 16, stream=st)       # a user stream: also ordered
        st.synchronize()
        assert int(n[0]) == 1 and hits[0, 0].tolist() == [777777, min(len(prefix), 50), 0]
    with pytest.raises(RuntimeError, match="negative video_id"):
        dc.upsert(-5, [1.0])
    with pytest.raises(RuntimeError, match="negative video_id"):
        dc.upload([(-1, [1.0])])
    dc.reserve(50000, 4000000)                                           # explicit pre-sizing
    assert dc.find_duplicates(prefix[:3], 3) == [(777777, 3)]
