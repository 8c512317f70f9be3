"""The near-duplicate search over a SHARDED table on the GPU: the merge kernel on hand-made blocks against the
plain-Python merge (tests/align_topk_shard_ref.py), tvz_align_topk_shards on a split table against tvz_align_topk on
the whole one (the existing, already-tested answer), the RCCL form at world size 1, the workspace's bounds,
service.ShardedCorpus.align_topk against the reference merge of its shards' own answers, and the Inspector over a
one-rank RankCorpus against a plain DeviceCorpus."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import align_topk_ref as atr, align_topk_shard_ref as asr
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0x5A5A5A5A
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
NAN = float("nan")
ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -4, -5           # include/tvz.h


# ---- 1. the merge kernel on hand-made blocks -------------------------------------------------------------------
def _merge(blocks, queries, call=None):
    """blocks int[R, Q, k+1, 4] -> (rows, totals) of tvz_align_topk_merge over outputs poisoned first"""
    blocks = np.ascontiguousarray(blocks, dtype=np.int32)
    R, Q, k1, _ = blocks.shape
    d_b = torch.from_numpy(blocks).to(DEV)
    d_q, d_off, _ = tc.pack_queries(queries, DEV)
    rows = torch.full((Q, k1 - 1, 4), POISON, dtype=torch.int32, device=DEV)
    totals = torch.full((Q,), POISON, dtype=torch.int32, device=DEV)
    rc = (call or _lib.load().tvz_align_topk_merge)(d_b.data_ptr(), R, Q, k1 - 1, d_q.data_ptr(), d_off.data_ptr(),
                                                   rows.data_ptr(), totals.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, rows.cpu().numpy().astype(np.int64), totals.cpu().numpy().astype(np.int64)


def _check_merge(blocks, queries):
    rc, rows, totals = _merge(blocks, queries)
    assert rc == 0, _lib.load().tvz_last_error()
    exp_rows, exp_totals = asr.merge_ref(blocks, queries)
    assert (totals == exp_totals).all(), (totals, exp_totals)
    assert (rows == exp_rows).all(), [(q, rows[q].tolist(), exp_rows[q].tolist()) for q in range(len(queries))
                                      if not (rows[q] == exp_rows[q]).all()][:1]
    return rows, totals


def _blocks(lists, queries, k):
    """lists[r][q] = the rows list r holds for query q (any order; sorted here as the contract demands)"""
    nv = [atr.n_valid(q) for q in queries]
    return np.stack([np.stack([asr.block_of(lists[r][q], nv[q], k) for q in range(len(queries))])
                     for r in range(len(lists))])


QUERIES5 = [[float(i) for i in range(10)],                       # nv = 10
            [float(i) if i % 2 else NAN for i in range(20)],     # nv = 10 < len = 20
            [],                                                  # empty
            [NAN] * 7,                                           # NaN-only: nv = 0
            [0.5 * i for i in range(33)]]


@pytest.mark.parametrize("n_lists,k", [(1, 1), (2, 2), (3, 63), (16, 64), (16, 1), (1, 64), (3, 2), (2, 63)])
def test_merge_of_interleaved_hits(n_lists, k):
    """random hits interleaved across the lists, few video ids (so that words collide across lists), every query kind
    of QUERIES5, lists from empty to full"""
    rng = np.random.default_rng(100 * n_lists + k)
    lists = [[[(int(rng.integers(0, 12)), int(rng.integers(0, 41)), int(rng.integers(-5, 6)), int(rng.integers(0, 50)))
               for _ in range(int(rng.integers(0, 2 * k + 1)))] for _ in QUERIES5] for _ in range(n_lists)]
    _check_merge(_blocks(lists, QUERIES5, k), QUERIES5)


@pytest.mark.parametrize("n_lists,k", [(1, 1), (3, 2), (16, 64)])
def test_merge_of_padding_only_and_of_one_full_list(n_lists, k):
    q = QUERIES5[:3]
    empty = [[[] for _ in q] for _ in range(n_lists)]
    rows, totals = _check_merge(_blocks(empty, q, k), q)
    assert (rows[:, :, 0] == -1).all() and (totals == 0).all()
    full = [[[] for _ in q] for _ in range(n_lists)]
    full[n_lists - 1] = [[(v, 10 + v % 7, v % 3 - 1, 1 + v % 9) for v in range(k + 3)] for _ in q]   # the LAST list, > k hits
    rows, totals = _check_merge(_blocks(full, q, k), q)
    assert (rows[0, :, 0] >= 0).all() and totals[0] == k + 3


def test_merge_ties_by_row_len_then_votes_and_identical_rows():
    q = [[float(i) for i in range(4000)]]                          # nv = 4000: (1 << 20) // 7999 == (1 << 20) // 8000
    assert tc.align_score(1, 4000, 4000) == tc.align_score(1, 4000, 4001)
    by_len = [[[(7, 4001, 3, 1)]], [[(7, 4000, 3, 1)]]]            # one word, row_len differs: the shorter row first
    rows, _ = _check_merge(_blocks(by_len, q, 2), q)
    assert rows[0].tolist() == [[7, 4000, 3, 1], [7, 4001, 3, 1]]
    by_votes = [[[(7, 4000, 3, 6000)]], [[(7, 4000, 3, 5000)]]]    # v = min(votes, nv, row_len) = 4000 for both
    rows, _ = _check_merge(_blocks(by_votes, q, 2), q)
    assert rows[0].tolist() == [[7, 4000, 3, 5000], [7, 4000, 3, 6000]]
    same = [[[(7, 4000, 3, 9), (8, 10, 0, 1)]], [[(7, 4000, 3, 9)]], [[(7, 4000, 3, 9)]]]
    rows, totals = _check_merge(_blocks(same, q, 4), q)            # the identical row of three lists: all three kept
    assert rows[0].tolist() == [[7, 4000, 3, 9]] * 3 + [[8, 10, 0, 1]] and totals[0] == 4
    rows, _ = _check_merge(_blocks(same, q, 2), q)
    assert rows[0].tolist() == [[7, 4000, 3, 9]] * 2


def test_merge_orders_by_nv_not_by_length():
    q = [QUERIES5[1]]                                              # 20 values, 10 of them NaN
    a, b = (1, 10, 0, 10), (2, 20, 0, 18)
    assert tc.align_order_key(a, 10) < tc.align_order_key(b, 10) and tc.align_order_key(b, 20) < tc.align_order_key(a, 20)
    rows, _ = _check_merge(_blocks([[[b]], [[a]]], q, 1), q)
    assert rows[0].tolist() == [list(a)]


def test_merge_at_nv_4095_and_refusal_of_4096():
    q = [[float(i) for i in range(4095)], [float(i) for i in range(4096)], [1.0, 2.0]]
    lists = [[[(v, 4095 - v, 1, 4095 - 2 * v) for v in range(5)], [(3, 5, 0, 5)], [(3, 2, 0, 2)]],
             [[(v + 2, 4095, -1, 4000 + v) for v in range(5)], [(4, 5, 0, 5)], [(9, 2, 1, 1)]]]
    rows, totals = _check_merge(_blocks(lists, q, 3), q)
    assert totals.tolist() == [10, INT32_MIN, 2] and (rows[1, :, 0] == -1).all() and rows[0, 0].tolist() == [0, 4095, 1, 4095]


def test_merge_refuses_a_query_some_list_refused_and_clamps_totals():
    q = QUERIES5[:1] * 3
    lists = [[[(1, 10, 0, 10)], [(2, 10, 0, 9)], [(3, 10, 0, 8)]], [[(4, 10, 0, 7)], [(5, 10, 0, 6)], [(6, 10, 0, 5)]],
             [[], [], []]]
    blocks = _blocks(lists, q, 2)
    blocks[1, 1] = asr.block_of([], 10, 2, n_hits=INT32_MIN)       # list 1 refused query 1
    blocks[0, 2, 2, 1], blocks[2, 2, 2, 1] = INT32_MAX, 5          # query 2: the sum passes 2^31 - 1
    rows, totals = _check_merge(blocks, q)
    assert totals.tolist() == [2, INT32_MIN, INT32_MAX]
    assert (rows[1, :, 0] == -1).all() and rows[0, :, 0].tolist() == [1, 4] and rows[2, :, 0].tolist() == [3, 6]


def test_merge_takes_a_row_without_union_and_padding_in_the_middle_as_padding():
    q = [[NAN, NAN], [1.0, 2.0, 3.0]]                              # nv = 0: a row of length 0 has u = 0
    blocks = np.zeros((2, 2, 4, 4), dtype=np.int64)
    blocks[:, :, :, 0] = -1
    blocks[0, 0, :3] = [(5, 0, 0, 0), (6, 3, 0, 2), (-1, 0, 0, 0)]  # u = 0; a live row (score 0); padding
    blocks[1, 0, :3] = [(-1, 0, 0, 0), (4, 7, 1, 1), (5, 0, 0, 3)]  # padding IN FRONT of a live row; u = 0 again
    blocks[0, 1, :3] = [(1, 3, 0, 3), (-1, 0, 0, 0), (2, 3, 0, 1)]  # padding between two sorted live rows
    blocks[:, :, 3, 1] = 2
    rows, totals = _check_merge(blocks, q)
    assert rows[0, :, 0].tolist() == [4, 6, -1] and rows[1, :, 0].tolist() == [1, 2, -1] and totals.tolist() == [4, 4]


def test_merge_refusals_write_nothing():
    lib = _lib.load()
    q = QUERIES5[:2]
    for n_lists, k, want in ((17, 4, ERR_UNSUPPORTED), (0, 4, ERR_UNSUPPORTED), (2, 65, ERR_UNSUPPORTED), (2, 0, ERR_UNSUPPORTED)):
        blocks = np.zeros((max(n_lists, 1), 2, k + 1, 4), dtype=np.int64)

        def call(b, R, Q, kk, *rest, n_lists=n_lists):
            return lib.tvz_align_topk_merge(b, n_lists, Q, kk, *rest)
        rc, rows, totals = _merge(blocks, q, call)
        assert rc == want, (n_lists, k, rc, lib.tvz_last_error())
        assert (rows == POISON).all() and (totals == POISON).all()
    blocks = np.zeros((2, 2, 5, 4), dtype=np.int64)
    for null_at in (0, 4, 5, 6, 7):
        def call(*a, null_at=null_at):
            a = list(a)
            a[null_at] = None
            return lib.tvz_align_topk_merge(*a)
        rc, rows, totals = _merge(blocks, q, call)
        assert rc == ERR_INVALID and (rows == POISON).all() and (totals == POISON).all(), null_at
    rc, rows, totals = _merge(blocks, q, lambda b, R, Q, *rest: lib.tvz_align_topk_merge(b, R, -1, *rest))
    assert rc == ERR_INVALID and (rows == POISON).all()
    rc, rows, totals = _merge(blocks, q, lambda b, R, Q, *rest: lib.tvz_align_topk_merge(b, R, 0, *rest))
    assert rc == 0 and (rows == POISON).all() and (totals == POISON).all()        # Q = 0: nothing to do


# ---- 2. split equivalence: the test that carries the feature -------------------------------------------------------
EPS, MAX_OFFSET = 1 / 30, 3.0


_table = asr.split_table


def _upload_split(rows, R):
    shards = [tc.DeviceCorpus(0) for _ in range(R)]
    for r, s in enumerate(shards):
        s.upload(rows[r::R])
    return shards


def _shards_call(shards, queries, k, max_query_len=None, **kw):
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    max_len = min(longest, 4095) if max_query_len is None else max_query_len
    ws = torch.empty(tc.align_topk_workspace_bytes(len(queries), max_len, d_q.numel(), k), dtype=torch.uint8, device=DEV)
    blocks, rows, totals = tc.align_topk_shards(shards, d_q, d_off, max_len, eps=EPS, max_offset=MAX_OFFSET, k=k,
                                                workspace=ws, **kw)
    torch.cuda.synchronize()
    return blocks.cpu().numpy(), rows.cpu().numpy(), totals.cpu().numpy()


@pytest.fixture(scope="module")
def split_world():
    rows, queries = _table()
    one = tc.DeviceCorpus(0)
    one.upload(rows)
    splits = {R: _upload_split(rows, R) for R in (1, 2, 3, 8)}
    answers = {k: one.align_topk(queries, eps=EPS, max_offset=MAX_OFFSET, k=k) for k in (1, 5, 64)}
    yield rows, queries, one, splits, answers
    for s in [one] + [h for v in splits.values() for h in v]:
        s.close()


@pytest.mark.parametrize("R", [1, 2, 3, 8])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_shards_equal_one_handle(split_world, R, k):
    rows, queries, one, splits, answers = split_world
    exp_rows, exp_totals = answers[k]
    assert exp_totals[0] > 64                                      # the premise: more hits than any k here
    _, got_rows, got_totals = _shards_call(splits[R], queries, k)
    assert (got_totals == exp_totals).all(), (got_totals, exp_totals)
    assert (got_rows == exp_rows).all()


def test_shards_with_empty_and_short_shards_and_a_refused_query(split_world):
    rows, queries, one, splits, answers = split_world
    few = [rows[i] for i in (1, 4, 7, 10, 13)]                     # shifted copies of the queries: 5 rows over 8 shards
    one5, shards = tc.DeviceCorpus(0), _upload_split(few, 8)
    try:
        one5.upload(few)
        assert [s.stats()[0] for s in shards] == [1, 1, 1, 1, 1, 0, 0, 0]
        batch = queries + [[float(i) for i in range(50)]]          # over-long at max_query_len = 45: refused everywhere
        for k in (1, 5, 64):
            exp_rows, exp_totals = one5.align_topk(batch, eps=EPS, max_offset=MAX_OFFSET, k=k, max_query_len=45)
            blocks, got_rows, got_totals = _shards_call(shards, batch, k, max_query_len=45)
            assert (got_rows == exp_rows).all() and (got_totals == exp_totals).all()
            assert got_totals[-1] == INT32_MIN and (blocks[:, -1, k, 1] == INT32_MIN).all()
            assert got_totals[0] >= 1
        exp = one5.align_topk(batch, eps=EPS, max_offset=MAX_OFFSET, k=5, max_query_len=45, min_votes=2,
                              min_score=atr.ONE // 4, exclude_ids=[few[0][0], -1, -1, -1, -1, -1])
        ex = torch.tensor([few[0][0], -1, -1, -1, -1, -1], dtype=torch.int32, device=DEV)
        _, got_rows, got_totals = _shards_call(shards, batch, 5, max_query_len=45, min_votes=2, min_score=atr.ONE // 4,
                                               d_exclude_ids=ex)
        assert (got_rows == exp[0]).all() and (got_totals == exp[1]).all()
    finally:
        for s in [one5] + shards:
            s.close()


def test_shards_refuse_before_anything_is_written(split_world):
    rows, queries, one, splits, answers = split_world
    lib = _lib.load()
    shards = splits[2]
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    Q, k = len(queries), 4
    ws = torch.empty(tc.align_topk_workspace_bytes(Q, longest, d_q.numel(), k), dtype=torch.uint8, device=DEV)
    handles = (C.c_void_p * 2)(*[s._h for s in shards])
    for kw, want in (({"eps": 0.0}, ERR_INVALID), ({"max_offset": 1000.0}, ERR_UNSUPPORTED), ({"k": 65}, ERR_UNSUPPORTED),
                     ({"min_votes": 0}, ERR_INVALID), ({"min_score": -1}, ERR_INVALID), ({"max_len": 4096}, ERR_UNSUPPORTED),
                     ({"ws_bytes": 1024}, ERR_WORKSPACE), ({"n": 17}, ERR_UNSUPPORTED)):
        blocks = torch.full((2, Q, k + 1, 4), POISON, dtype=torch.int32, device=DEV)
        out = torch.full((Q, k, 4), POISON, dtype=torch.int32, device=DEV)
        totals = torch.full((Q,), POISON, dtype=torch.int32, device=DEV)
        rc = lib.tvz_align_topk_shards(handles, kw.get("n", 2), d_q.data_ptr(), d_off.data_ptr(), Q, kw.get("max_len", longest),
                                       kw.get("eps", EPS), kw.get("max_offset", MAX_OFFSET), kw.get("min_votes", 1),
                                       kw.get("min_score", 0), None, kw.get("k", k), blocks.data_ptr(), out.data_ptr(),
                                       totals.data_ptr(), ws.data_ptr(), kw.get("ws_bytes", ws.numel()),
                                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == want, (kw, rc, lib.tvz_last_error())
        assert bool((blocks == POISON).all()) and bool((out == POISON).all()) and bool((totals == POISON).all()), kw


# ---- 3. + 6. the RCCL form at world size 1, in a fresh child process ----------------------------------------------
@pytest.fixture(scope="module")
def comm_child(tmp_path_factory):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "near_comm_child.py"),
                          str(tmp_path_factory.mktemp("near"))], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=600)
    if out.returncode == 3 and "RCCL is not available" in out.stdout:
        pytest.skip("RCCL is not available")
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_align_topk_sharded_through_rccl_world_size_1(comm_child):
    res = comm_child
    assert res["premise_hits"] > 5                                 # more hits than k = 5 for the first query
    for name in ("k5", "k64", "k5_filtered"):
        assert res[name]["rows"] == res[name]["one_rows"] and res[name]["totals"] == res[name]["one_totals"], name
    assert res["k5"]["totals"][-1] == INT32_MIN                    # the over-long query stays refused
    assert res["matcher_equal"] is True and res["matcher_slots_equal"] is True
    # its workspace (tvz_align_topk_sharded_workspace_bytes): exact and misaligned slices stay inside, one byte short
    assert res["workspace_bounds_ok"] == [True, True, True]
    rc, msg = res["workspace_short"]
    assert rc == ERR_WORKSPACE and " 1 bytes missing" in msg and "tvz_align_topk_sharded_workspace_bytes" in msg, msg


def test_inspector_over_a_one_rank_rank_corpus(comm_child):
    res = comm_child
    assert res["near_rank"] == res["near_plain"]
    assert [d["filename"] for d in res["near_plain"][2]] == ["a.y4m"] and res["near_plain"][2][0]["jaccard"] == 1.0
    assert res["near_bad_param"] == "ValueError" and res["rank_broken"] is None


# ---- 4. workspace bounds --------------------------------------------------------------------------------------------
def test_sharded_workspace_sizes_are_what_the_calls_need(split_world):
    """tests/test_workspace_bounds_gpu.py's method for tvz_align_topk_shards (one handle's workspace serves all): an
    exactly sized, deliberately misaligned slice of a poisoned buffer gives the same answers with nothing written
    outside it; one byte short is TVZ_ERR_WORKSPACE and names the missing byte."""
    rows, queries, one, splits, answers = split_world
    lib = _lib.load()
    k, lead = 5, 4096
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    Q = len(queries)
    n = tc.align_topk_workspace_bytes(Q, longest, d_q.numel(), k)
    exp_rows, exp_totals = answers[k]
    for extra in (0, 8, 248):
        buf = torch.full((lead + 256 + n + lead,), 0xA5, dtype=torch.uint8, device=DEV)
        lo, hi = lead + extra, lead + extra + n
        _, got_rows, got_totals = tc.align_topk_shards(splits[3], d_q, d_off, longest, eps=EPS, max_offset=MAX_OFFSET, k=k,
                                                       workspace=buf[lo:hi])
        torch.cuda.synchronize()
        assert bool((buf[:lo] == 0xA5).all()) and bool((buf[hi:] == 0xA5).all()), extra
        assert (got_rows.cpu().numpy() == exp_rows).all() and (got_totals.cpu().numpy() == exp_totals).all()
    # the least the call takes: the fixed parts and ONE query of max_query_len values (between that and `n` queries
    # that do not fit are refused one by one); one byte below it the call is refused and says so
    least = tc.align_topk_workspace_bytes(Q, longest, longest, k)
    assert least <= n
    with pytest.raises(RuntimeError, match=r"libtvz error -5: .*\b1 bytes missing"):
        tc.align_topk_shards(splits[3], d_q, d_off, longest, eps=EPS, max_offset=MAX_OFFSET, k=k,
                             workspace=torch.empty(least, dtype=torch.uint8, device=DEV)[:least - 1])
    assert lib.tvz_align_topk_sharded_workspace_bytes(Q, longest, d_q.numel(), k, 1) >= n + 2 * Q * (k + 1) * 16


# ---- 5. service.ShardedCorpus.align_topk ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_shards", [8, 20])
def test_sharded_corpus_equals_the_reference_merge_of_its_shards(n_shards):
    from tvidz_amd import service
    rows, queries = _table()
    sc = service.ShardedCorpus(0, n_shards=n_shards, k=8)
    try:
        sc.upload(rows)
        batch = queries + [[float(i) for i in range(4096)]]
        excl = [rows[11][0], -1, -1, -1, -1, -1]
        for kw in ({"k": 8}, {"k": 3, "min_votes": 2, "exclude_ids": excl}, {"k": 64, "min_score": atr.ONE // 2}):
            parts = [s.align_topk(batch, eps=EPS, max_offset=MAX_OFFSET, max_query_len=4095, **kw) for s in sc.shards]
            exp_rows, exp_totals = asr.merge_of_parts(parts, batch)
            got = sc.align_topk(batch, eps=EPS, max_offset=MAX_OFFSET, max_query_len=4095, **kw)
            assert got[0].dtype == np.int32 and got[0].shape == (len(batch), kw["k"], 4) and got[1].shape == (len(batch),)
            assert (got[0] == exp_rows).all() and (got[1] == exp_totals).all(), kw
            # tensor-pair input
            d_q, d_off, _ = tc.pack_queries(batch, DEV)
            kw2 = dict(kw)
            if "exclude_ids" in kw2:
                kw2["exclude_ids"] = torch.tensor(excl, dtype=torch.int32, device=DEV)
            got2 = sc.align_topk((d_q, d_off), eps=EPS, max_offset=MAX_OFFSET, max_query_len=4095, **kw2)
            assert (got2[0] == exp_rows).all() and (got2[1] == exp_totals).all(), kw
        assert exp_totals[0] > 8 and exp_totals[-1] == INT32_MIN
    finally:
        sc.close()
