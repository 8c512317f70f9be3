"""GPU parity of tvz_align_topk (ts_align_topk_kernel + ts_align_topk_reduce_kernel) with tests/align_topk_ref.py:
whole [Q, k + 1, 4] blocks, bit-exact, every case - the edge cases of tests/align_ref.py as batches, the batch's own
edges, two rows of one video id, refusals, the table after mutations, agreement with tvz_align's own output, the
sharded form and the inspector's near_top_k."""

import numpy as np
import pytest
import torch

from tests import align_ref as ar
from tests import align_topk_ref as atr
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -0x5A5A5A5A
ERR_WORKSPACE = -5
KS = (1, 16, 64)


@pytest.fixture(scope="module")
def dc():
    c = tc.DeviceCorpus(0)
    yield c
    c.close()


def _raw(dc, queries, eps, mo, k, min_votes=1, min_score=0, exclude_ids=None, max_query_len=None, out=None,
         ws_short=0, stream=None):
    """tvz_align_topk through the C ABI -> (return code, the [Q, k + 1, 4] device block)."""
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    Q = len(queries)
    L = min(longest, atr.MAX_LEN) if max_query_len is None else max_query_len
    if out is None:
        out = torch.full((Q, max(k, 0) + 1, 4), SENTINEL, dtype=torch.int32, device=DEV)
    need = tc.align_topk_workspace_bytes(Q, min(max(L, 0), atr.MAX_LEN), d_q.numel(), min(max(k, 1), 64)) - ws_short
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    d_ex = None if exclude_ids is None else torch.as_tensor(np.asarray(exclude_ids, dtype=np.int32)).to(DEV)
    s = stream if stream is not None else torch.cuda.current_stream(DEV)
    rc = _lib.load().tvz_align_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), Q, int(L), float(eps), float(mo),
                                    int(min_votes), int(min_score), d_ex.data_ptr() if d_ex is not None else None,
                                    int(k), out.data_ptr(), ws.data_ptr(), need, s.cuda_stream)
    s.synchronize()
    return rc, out


def _expect_blocks(got, exp, what):
    got = np.asarray(got, dtype=np.int64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere((got != exp).any(axis=2))
    assert bad.size == 0, (what, f"{len(bad)} rows differ", [(q, r, got[q, r].tolist(), exp[q, r].tolist())
                                                             for q, r in bad[:4].tolist()])


def _check(dc, rows, queries, eps, mo, k, aligned=None, **kw):
    exp = atr.topk_ref(rows, queries, eps, mo, k, aligned=aligned, **kw)
    rc, out = _raw(dc, queries, eps, mo, k, **kw)
    assert rc == 0, _lib.load().tvz_last_error()
    _expect_blocks(out.cpu().numpy(), exp, (eps, mo, k, kw))
    return exp


def _kth_scores(aligned, queries, k, limit=3):
    """The exact score of the k-th hit (the last one where there are fewer) of the batch's queries: a few distinct."""
    out = []
    for a, q in zip(aligned, queries):
        hits = atr.hits_of(a, atr.n_valid(q))
        if hits:
            out.append(-hits[min(k, len(hits)) - 1][0][0])
    return sorted(set(out))[-limit:]


@pytest.mark.parametrize("case", ar.edge_cases(), ids=lambda c: c[0])
def test_edge_cases_as_batches_bit_exact(dc, case):
    name, rows, calls = case
    dc.upload(rows)
    batches = {}
    for q, eps, mo in calls:                                   # all calls that share (eps, max_offset): one batch
        batches.setdefault((eps, mo), []).append(list(q))
    for (eps, mo), queries in batches.items():
        aligned = [ar.align_ref(rows, q, eps, mo) for q in queries]          # once per batch, shared below
        for k in KS:
            exp = _check(dc, rows, queries, eps, mo, k, aligned=aligned)
            for s_k in _kth_scores(aligned, queries, k):                     # the equality edge
                _check(dc, rows, queries, eps, mo, k, aligned=aligned, min_score=s_k)
            if name == "grid_stride":
                assert exp[0, k, 1] == 11_808                               # far more hits than k, 11,796 of them tied
            if name == "boundary":
                assert 3_024 <= exp[0, k, 1] <= 5_760
        # the Python call returns the same rows and totals
        got_rows, got_totals = dc.align_topk(queries, eps=eps, max_offset=mo, k=16)
        exp = atr.topk_ref(rows, queries, eps, mo, 16, aligned=aligned)
        assert got_rows.dtype == got_totals.dtype == np.int32
        _expect_blocks(got_rows, exp[:, :16], "rows of the Python call")
        assert got_totals.tolist() == exp[:, 16, 1].tolist()


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(77)
    grid = np.arange(1, 9_001) / 30.0
    return [(v, np.sort(rng.choice(grid, size=int(rng.integers(1, 40)), replace=False)).tolist()) for v in range(1, 121)]


def test_batch_edges(dc, table):
    """One batch: an empty query, a NaN-only one, one of 4,095 values, one longer than max_query_len (refused, its
    neighbours untouched) among shifted copies of stored rows - Q = 70; Q = 1; exclusion given and NULL."""
    rng = np.random.default_rng(78)
    dc.upload(table)
    eps, mo = 1 / 30, 2.0
    long_q = (rng.choice(np.arange(1, 9_001), size=4095, replace=False) / 30.0 + 1 / 30).tolist()
    too_long = long_q + [1.0]
    queries = [[], [float("nan")] * 3, long_q, too_long]
    queries += [(np.asarray(table[i][1]) + (i % 7 - 3) / 30).tolist() for i in range(66)]
    assert len(queries) == 70
    aligned = [ar.align_ref(table, q, eps, mo) if len(q) <= 4095 else None for q in queries]
    for k in (1, 16):
        exp = _check(dc, table, queries, eps, mo, k, aligned=aligned, max_query_len=4095)
        assert exp[0, k].tolist() == exp[1, k].tolist() == [-1, 0, 0, 0]
        assert exp[3, k].tolist() == [-1, atr.REFUSED, 0, 0] and exp[2, k, 1] > 0 and exp[4, k, 1] > 0
    # exclusion: every shifted copy's own row is its rank 0; excluded, it vanishes and the total drops by one row
    free = atr.topk_ref(table, queries, eps, mo, 16, aligned=aligned, max_query_len=4095)
    ex = [-1, -1, -1, -1] + [table[i][0] for i in range(66)]
    assert all(free[4 + i, 0, 0] == table[i][0] for i in range(66))
    exp = _check(dc, table, queries, eps, mo, 16, aligned=aligned, max_query_len=4095, exclude_ids=ex)
    assert (exp[4:, 16, 1] == free[4:, 16, 1] - 1).all() and not (exp[4:, :16, 0] == np.asarray(ex[4:])[:, None]).any()
    # Q = 1, with and without exclusion, with a vote threshold
    for kw in ({}, {"exclude_ids": [ex[9]]}, {"min_votes": 3}):
        _check(dc, table, [queries[9]], eps, mo, 16, aligned=[aligned[9]], **kw)


def test_two_rows_with_one_video_id(dc):
    """Identical rows are both kept; rows of one id with one word are ordered by (row_len, votes)."""
    far = (np.arange(2, 2_003) * 10.0).tolist()                     # one key near the query, the rest far from it
    rows = [(9, [5.0, 6.0, 7.5]), (9, [5.0, 6.0, 7.5]), (3, [5.0, 6.0]), (9, [5.0, 6.0, 7.5, 9.0]),
            (4, [1.0] + far[:2000]), (4, [1.0] + far[:1999]),        # u = 2001 and 2000: 2^20 // u = 524 for both
            (4, [1.0, 1.01] + far[:1999]),                           # ... and two votes in the bin where the others have one
            (2, [])]
    dc.upload(rows)
    for k in (1, 2, 3, 16):
        exp = _check(dc, rows, [[5.0, 6.0, 7.5], [1.0]], 0.1, 1.0, k)
    assert exp[0, :4].tolist() == [[9, 3, 0, 3], [9, 3, 0, 3], [9, 4, 0, 3], [3, 2, 0, 2]]
    assert exp[1, :4].tolist() == [[4, 2000, 0, 1], [4, 2001, 0, 1], [4, 2001, 0, 2], [-1, 0, 0, 0]]


def test_refusals_write_nothing(dc, table):
    dc.upload(table)
    q = [table[3][1]]
    out = torch.full((1, 17, 4), SENTINEL, dtype=torch.int32, device=DEV)
    for eps, mo, code in ar.REFUSALS:
        assert _raw(dc, q, eps, mo, 16, out=out)[0] == code, (eps, mo)
    invalid, unsupported = ar.ERR_INVALID, ar.ERR_UNSUPPORTED
    assert _raw(dc, q, 0.1, 1.0, 16, min_votes=0, out=out)[0] == invalid
    assert _raw(dc, q, 0.1, 1.0, 16, min_score=-1, out=out)[0] == invalid
    assert _raw(dc, q, 0.1, 1.0, 16, min_score=atr.ONE + 1, out=out)[0] == invalid
    assert _raw(dc, q, 0.1, 1.0, 0, out=out)[0] == unsupported
    assert _raw(dc, q, 0.1, 1.0, 65, out=out)[0] == unsupported
    assert _raw(dc, q, 0.1, 1.0, 16, max_query_len=4096, out=out)[0] == unsupported
    assert _raw(dc, q, 0.1, 1.0, 16, ws_short=1, out=out)[0] == ERR_WORKSPACE
    assert b"1 bytes missing" in _lib.load().tvz_last_error()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    # right next to the refused ones: the largest bin count, k and score threshold are served
    for kw in ({"eps": 1 / 64, "mo": 2047.49 / 64, "k": 64}, {"eps": 0.1, "mo": 1.0, "k": 16, "min_score": atr.ONE}):
        _check(dc, table, q, kw.pop("eps"), kw.pop("mo"), kw.pop("k"), **kw)


def test_after_mutations(dc):
    """A replacing upsert, a new row, an emptied row, build_index, clear, and a call on another stream right after
    an upsert: always the reference over the current table."""
    rng = np.random.default_rng(17)
    grid = np.arange(1, 20_001) / 30.0
    rows = {v: np.sort(rng.choice(grid, size=int(rng.integers(2, 40)), replace=False)).tolist() for v in range(1, 201)}
    dc.upload(list(rows.items()))
    qs = [(np.asarray(rows[7][:12] + rows[8][:5]) + 3 / 30).tolist(), rows[30]]
    eps, mo = 1 / 30, 2.0

    def check(**kw):
        table = sorted(rows.items())                             # ids are unique: the order of the table is free
        return _check(dc, table, qs, eps, mo, 16, **kw)

    check()
    rows[7] = np.sort(rng.choice(grid, size=60, replace=False)).tolist()          # a replacing upsert
    dc.upsert(7, rows[7])
    rows[11] = (np.asarray(qs[0]) - 1 / 30).tolist()
    dc.upsert(11, rows[11])
    assert check()[0, 0].tolist() == [11, len(qs[0]), -1, len(qs[0])]
    rows[301] = np.sort(rng.choice(grid, size=150, replace=False)).tolist()       # a new row
    dc.upsert(301, rows[301])
    check()
    rows[30] = []                                                                  # an emptied row
    dc.upsert(30, [])
    check()
    dc.build_index()
    check()
    rows[9] = (np.asarray(qs[0]) + 2 / 30).tolist()                                # another stream, right after an upsert
    dc.upsert(9, rows[9])
    s2 = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s2):
        exp = check()
    assert exp[0, 0].tolist() == [9, len(qs[0]), 2, len(qs[0])]
    dc.clear()
    rows.clear()
    assert check()[:, 16].tolist() == [[-1, 0, 0, 0]] * 2


def test_agrees_with_tvz_align_on_a_random_table(dc):
    rng = np.random.default_rng(5)
    grid = np.arange(1, 30_001) / 30.0
    rows = [(v, np.sort(rng.choice(grid, size=int(rng.integers(1, 80)), replace=False)).tolist())
            for v in rng.permutation(5000)[:500].tolist()]
    dc.upload(rows)
    queries = [(np.asarray(rows[i][1]) + s / 30).tolist() for i, s in ((3, 2), (100, -5), (499, 0))]
    eps, mo = 1 / 30, 5.0
    aligned = [dc.align(q, eps=eps, max_offset=mo).astype(np.int64) for q in queries]      # tvz_align's own output
    for k, kw in ((16, {}), (64, {"min_votes": 2}), (5, {"min_score": atr.ONE // 8})):
        _check(dc, rows, queries, eps, mo, k, aligned=aligned, **kw)


def test_sharded_corpus_equals_one_handle(table):
    from tvidz_amd import service
    rng = np.random.default_rng(6)
    rows = list(table) + [(500 + i, (np.asarray(table[5][1]) + i / 30).tolist()) for i in range(40)]
    queries = [table[5][1], (np.asarray(table[17][1]) - 2 / 30).tolist(), [], rng.uniform(0, 300, 4096).tolist()]
    sc, one = service.ShardedCorpus(0, n_shards=8, k=8), tc.DeviceCorpus(0)
    try:
        for c in (sc, one):
            c.upload(rows)
            c.upsert(777, queries[1])
        for kw in ({"k": 8}, {"k": 8, "min_score": atr.ONE // 2, "exclude_ids": [table[5][0], 777, -1, -1]},
                   {"k": 3, "min_votes": 2}):
            a = sc.align_topk(queries, eps=1 / 30, max_offset=3.0, max_query_len=4095, **kw)
            b = one.align_topk(queries, eps=1 / 30, max_offset=3.0, max_query_len=4095, **kw)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), kw
        # the premise: more than k hits, from several shards, and the refused query stays refused
        assert b[1][0] > 8 and len({int(v) % 8 for v in b[0][0][:, 0]}) > 1 and b[1][3] == tc.ALIGN_REFUSED == a[1][3]
    finally:
        sc.close()
        one.close()


class _NoTopkCorpus:
    def align(self, timestamps, eps=0.1, max_offset=60.0):
        return np.zeros((0, 5), dtype=np.int32)


class _NoTopkStore:
    corpus = _NoTopkCorpus()


def test_inspector_near_top_k(tmp_path):
    from tests.fakes import CutReader, cut_inspector
    from tvidz_amd import db as tdb, inspector as insp, service

    with pytest.raises(RuntimeError, match="align_topk"):
        insp.Inspector(_NoTopkStore(), device=DEV, near_duplicates=True, near_top_k=8)

    # the three-clip scenario of tests/test_align_gpu.py::test_sharded_corpus_align_and_near_duplicates
    cuts = {"a.y4m": [1.0, 2.5, 4.0, 7.3, 9.9, 12.0], "c.y4m": [0.7, 3.3, 5.1, 8.8],
            "b.y4m": [x + 7 / 30 for x in [1.0, 2.5, 4.0, 7.3, 9.9, 12.0]]}
    reports = []
    for n, (corpus, top_k) in enumerate(((tc.DeviceCorpus(0), None), (tc.DeviceCorpus(0), 8),
                                         (service.ShardedCorpus(0, n_shards=8, k=8), 8))):
        store = tdb.Store(f"sqlite:///{tmp_path}/{n}.db", corpus=corpus)
        ins = cut_inspector(store, device=DEV, near_duplicates=True, near_top_k=top_k,
                            frame_source=lambda bucket, key, filename, uid: (CutReader(cuts[key], frames=600), None))
        try:
            res = [ins.analyze_file("videos", k) for k in ("a.y4m", "c.y4m", "b.y4m")]
        finally:
            store.close()                      # closes the corpus too
        assert all(r["status"] == "done" for r in res), res
        reports.append([r["near_duplicates"] for r in res])
    assert reports[0] == reports[1] == reports[2]
    assert [d["filename"] for d in reports[0][2]] == ["a.y4m"] and reports[0][2][0]["jaccard"] == 1.0

    # 12 shifted copies stored: exactly the 8 best are reported, in order
    base = (np.arange(1, 41) * 2.5 + 0.1).tolist()
    store = tdb.Store(f"sqlite:///{tmp_path}/copies.db", corpus=tc.DeviceCorpus(0))
    try:
        for i in range(1, 13):
            v = store.add_video(f"copy{i}.y4m")
            store.add_timestamps(v.id, [x + i / 30 for x in base[:40 - i % 5]])
        for j in range(5):                                         # and rows that are no near duplicates
            v = store.add_video(f"other{j}.y4m")
            store.add_timestamps(v.id, [x + 0.7 * j for x in base[::3]])
        me = store.add_video("upload.y4m")
        store.add_timestamps(me.id, base)
        walk = insp.Inspector(store, device=DEV, near_duplicates=True)
        top8 = insp.Inspector(store, device=DEV, near_duplicates=True, near_top_k=8)
        try:
            full = walk._near(me.id, base)
            assert len(full) == 12 and all(d["filename"].startswith("copy") for d in full)
            assert top8._near(me.id, base) == full[:8]
        finally:
            walk.close()
            top8.close()
    finally:
        store.close()
