"""The near-duplicate search at any shift over a SHARDED table on the GPU.  Every comparison is exact integer equality.
The wide merge kernel on hand-made blocks against the plain-Python merge (tests/align_wide_shard_ref.py) - bins beyond
the bounded merge's 12-bit word, both score kinds, padding, ties, limits, refusals - and against the bounded merge where
both apply; tvz_align_wide_topk_shards on a split table against one handle that holds all rows and against the CPU
restatement of tvz_align_wide_topk; service.ShardedCorpus.align_wide_topk with and without grouping; the RCCL form at
world size 1 and the Inspector over a one-rank RankCorpus in a fresh child process (tests/near_wide_comm_child.py); the
Inspector over a ShardedCorpus."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import align_topk_ref as atr, align_wide_ref as awr, align_wide_shard_ref as wsr
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0x5A5A5A5A
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
NAN = float("nan")
ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -4, -5           # include/tvz.h
MAX_B = tc.ALIGN_WIDE_MAX_B
EPS = wsr.EPS
WIDEST = awr.MAX_B * EPS


# ---- 1. the merge kernel on hand-made blocks -------------------------------------------------------------------
def _merge(blocks, queries, flags=0, call=None):
    """blocks int[R, Q, k+1, 4] -> (rc, rows, totals) of tvz_align_wide_topk_merge over outputs poisoned first"""
    blocks = np.ascontiguousarray(blocks, dtype=np.int32)
    R, Q, k1, _ = blocks.shape
    d_b = torch.from_numpy(blocks).to(DEV)
    d_q, d_off, _ = tc.pack_queries(queries, DEV)
    rows = torch.full((Q, k1 - 1, 4), POISON, dtype=torch.int32, device=DEV)
    totals = torch.full((Q,), POISON, dtype=torch.int32, device=DEV)
    rc = (call or _lib.load().tvz_align_wide_topk_merge)(d_b.data_ptr(), R, Q, k1 - 1, flags, d_q.data_ptr(), d_off.data_ptr(),
                                                        rows.data_ptr(), totals.data_ptr(),
                                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, rows.cpu().numpy().astype(np.int64), totals.cpu().numpy().astype(np.int64)


def _check_merge(blocks, queries, contain=False):
    rc, rows, totals = _merge(blocks, queries, tc.ALIGN_CONTAIN if contain else 0)
    assert rc == 0, _lib.load().tvz_last_error()
    exp_rows, exp_totals = wsr.merge_ref(blocks, queries, contain)
    assert (totals == exp_totals).all(), (totals, exp_totals)
    assert (rows == exp_rows).all(), [(q, rows[q].tolist(), exp_rows[q].tolist()) for q in range(len(queries))
                                      if not (rows[q] == exp_rows[q]).all()][:1]
    return rows, totals


def _blocks(lists, queries, k, contain=False):
    """lists[r][q] = the rows list r holds for query q (any order; sorted here as the contract demands)"""
    nv = [atr.n_valid(q) for q in queries]
    return np.stack([np.stack([wsr.block_of(lists[r][q], nv[q], k, contain) for q in range(len(queries))])
                     for r in range(len(lists))])


QUERIES5 = [[float(i) for i in range(10)],                       # nv = 10
            [float(i) if i % 2 else NAN for i in range(20)],     # nv = 10 < len = 20
            [],                                                  # empty
            [NAN] * 7,                                           # NaN-only: nv = 0
            [0.5 * i for i in range(33)]]


@pytest.mark.parametrize("contain", [False, True])
@pytest.mark.parametrize("Q", [1, 5])
@pytest.mark.parametrize("n_lists,k", [(1, 1), (2, 2), (3, 63), (5, 5), (16, 64), (16, 1), (1, 64)])
def test_merge_of_interleaved_hits(n_lists, k, Q, contain):
    """random hits interleaved across the lists, few video ids and few distinct bins over the whole +-2^22 (so that
    ids and scores collide across lists and the bin decides), every query kind of QUERIES5, lists from empty to full"""
    rng = np.random.default_rng(1000 * n_lists + 10 * k + Q)
    bins = [-MAX_B, -MAX_B + 1, -2049, -2048, -2047, -1, 0, 1, 2047, 2048, 70000, MAX_B - 1, MAX_B]
    queries = QUERIES5[:Q]
    lists = [[[(int(rng.integers(0, 12)), int(rng.integers(0, 41)), bins[int(rng.integers(0, len(bins)))],
                int(rng.integers(0, 50))) for _ in range(int(rng.integers(0, 2 * k + 1)))] for _ in queries]
             for _ in range(n_lists)]
    _check_merge(_blocks(lists, queries, k, contain), queries, contain)


def test_bins_beyond_the_bounded_word():
    """One video id, one row_len, one vote count - one score - at the bins +-2^22, +-2,048 and 0, spread over three
    lists: the wide merge returns them by the signed bin.  The bounded merge of the same blocks cannot: its word holds a
    bin of 12 bits."""
    q = [[float(i) for i in range(10)]]
    hits = [(7, 10, b, 10) for b in (MAX_B, -2048, 0, 2048, -MAX_B)]
    lists = [[[hits[0], hits[3]]], [[hits[1], hits[4]]], [[hits[2]]]]
    for contain in (False, True):
        blocks = _blocks(lists, q, 5, contain)
        rows, totals = _check_merge(blocks, q, contain)
        assert rows[0, :, 2].tolist() == [-MAX_B, -2048, 0, 2048, MAX_B] and totals[0] == 5
        rows, _ = _check_merge(_blocks(lists, q, 2, contain), q, contain)
        assert rows[0, :, 2].tolist() == [-MAX_B, -2048]
    d_q, d_off, _ = tc.pack_queries(q, DEV)
    blocks = _blocks(lists, q, 5)
    b_rows, b_totals = tc.align_topk_merge(torch.from_numpy(blocks.astype(np.int32)).to(DEV), 5, d_q, d_off)
    torch.cuda.synchronize()
    exp_rows, _ = wsr.merge_ref(blocks, q)
    assert (b_rows.cpu().numpy() != exp_rows).any()                 # why the bounded merge cannot stand in for this one
    assert sorted(b_rows.cpu().numpy()[0, :, 2].tolist()) != [-MAX_B, -2048, 0, 2048, MAX_B]


def test_the_two_score_kinds_order_differently():
    q = [[float(i) for i in range(20)]]                            # nv = 20
    a, b = (1, 40, 90000, 20), (2, 24, -90000, 18)                 # Jaccard 20/40 < 18/26; containment 20/20 > 18/20
    assert tc.align_wide_order_key(b, 20) < tc.align_wide_order_key(a, 20)
    assert tc.align_wide_order_key(a, 20, True) < tc.align_wide_order_key(b, 20, True)
    lists = [[[a]], [[b]]]
    rows, _ = _check_merge(_blocks(lists, q, 1, False), q, False)
    assert rows[0].tolist() == [list(b)]
    rows, _ = _check_merge(_blocks(lists, q, 1, True), q, True)
    assert rows[0].tolist() == [list(a)]
    rows, _ = _check_merge(_blocks(lists, q, 2, True), q, True)
    assert rows[0].tolist() == [list(a), list(b)]


def test_padding_in_the_middle_a_row_without_union_and_a_nan_only_query():
    q = [[1.0, 2.0, 3.0], [NAN, NAN], [1.0, 2.0, 3.0]]
    blocks = np.zeros((2, 3, 4, 4), dtype=np.int64)
    blocks[:, :, :, 0] = -1
    blocks[0, 0, :3] = [(1, 3, 5000, 3), (-1, 0, 0, 0), (2, 3, -5000, 1)]   # padding between two sorted live rows
    blocks[1, 0, :3] = [(-1, 0, 0, 0), (4, 3, MAX_B, 2), (-1, 0, 0, 0)]     # padding IN FRONT of a live row
    blocks[0, 1, :3] = [(5, 0, 0, 0), (6, 3, 0, 2), (-1, 0, 0, 0)]          # nv = 0: u = 0 for row_len 0, and for containment
    blocks[1, 1, :3] = [(-1, 0, 0, 0), (4, 7, 1, 1), (5, 0, 0, 3)]
    blocks[0, 2, :3] = [(8, 3, 0, 3), (9, 0, 0, 0), (-1, 0, 0, 0)]          # row_len 0: live by the Jaccard (score 0) only
    blocks[:, :, 3, 1] = 3
    rows, totals = _check_merge(blocks, q, False)
    assert rows[0, :, 0].tolist() == [1, 4, 2] and rows[1, :, 0].tolist() == [4, 6, -1] and rows[2, :, 0].tolist() == [8, 9, -1]
    assert totals.tolist() == [6, 6, 6]
    rows, totals = _check_merge(blocks, q, True)
    assert rows[0, :, 0].tolist() == [1, 4, 2]
    assert (rows[1, :, 0] == -1).all() and totals[1] == 6           # the NaN-only query: all padding, the total is the sum
    assert rows[2, :, 0].tolist() == [8, -1, -1]                    # row_len = 0 under containment: padding


def test_the_tie_chain_and_identical_rows():
    q = [[float(i) for i in range(4000)]]                          # nv = 4000: (1 << 20) // 7999 == (1 << 20) // 8000
    assert tc.align_score(1, 4000, 4000) == tc.align_score(1, 4000, 4001)
    by_bin = [[[(7, 4000, 2048, 1)]], [[(7, 4000, -MAX_B, 1)]], [[(7, 4000, -2048, 1)]]]     # one score, one id: the bin
    rows, _ = _check_merge(_blocks(by_bin, q, 3), q)
    assert rows[0, :, 2].tolist() == [-MAX_B, -2048, 2048]
    by_len = [[[(7, 4001, 3000, 1)]], [[(7, 4000, 3000, 1)]]]      # then row_len: the shorter row first
    rows, _ = _check_merge(_blocks(by_len, q, 2), q)
    assert rows[0].tolist() == [[7, 4000, 3000, 1], [7, 4001, 3000, 1]]
    bin_first = [[[(7, 4000, 3001, 1)]], [[(7, 4001, 3000, 1)]]]   # ... but only behind the bin
    rows, _ = _check_merge(_blocks(bin_first, q, 2), q)
    assert rows[0].tolist() == [[7, 4001, 3000, 1], [7, 4000, 3001, 1]]
    by_votes = [[[(7, 4000, 3000, 6000)]], [[(7, 4000, 3000, 5000)]]]      # v = min(votes, nv, row_len) = 4000 for both
    for contain in (False, True):
        rows, _ = _check_merge(_blocks(by_votes, q, 2, contain), q, contain)
        assert rows[0].tolist() == [[7, 4000, 3000, 5000], [7, 4000, 3000, 6000]]
    same = [[[(7, 4000, -70000, 9), (8, 10, 0, 1)]], [[(7, 4000, -70000, 9)]], [[(7, 4000, -70000, 9)]]]
    rows, totals = _check_merge(_blocks(same, q, 4), q)            # the identical row of three lists: all three kept
    assert rows[0].tolist() == [[7, 4000, -70000, 9]] * 3 + [[8, 10, 0, 1]] and totals[0] == 4
    rows, _ = _check_merge(_blocks(same, q, 2), q)
    assert rows[0].tolist() == [[7, 4000, -70000, 9]] * 2


def test_nv_4095_is_taken_4096_values_are_refused():
    q = [[float(i) for i in range(4095)], [float(i) for i in range(4096)], [1.0, 2.0]]
    lists = [[[(v, 4095 - v, MAX_B - v, 4095 - 2 * v) for v in range(5)], [(3, 5, 0, 5)], [(3, 2, 0, 2)]],
             [[(v + 2, 4095, -MAX_B, 4000 + v) for v in range(5)], [(4, 5, 0, 5)], [(9, 2, 1, 1)]]]
    for contain in (False, True):
        rows, totals = _check_merge(_blocks(lists, q, 3, contain), q, contain)
        assert totals.tolist() == [10, INT32_MIN, 2] and (rows[1, :, 0] == -1).all()
        assert rows[0, 0].tolist() == [0, 4095, MAX_B, 4095]


def test_a_refused_list_refuses_the_query_and_totals_clamp():
    q = QUERIES5[:1] * 3
    lists = [[[(1, 10, 0, 10)], [(2, 10, 0, 9)], [(3, 10, 0, 8)]], [[(4, 10, 0, 7)], [(5, 10, 0, 6)], [(6, 10, 0, 5)]],
             [[], [], []]]
    blocks = _blocks(lists, q, 2)
    blocks[1, 1] = wsr.block_of([], 10, 2, n_hits=INT32_MIN)       # list 1 refused query 1
    blocks[0, 2, 2, 1], blocks[2, 2, 2, 1] = INT32_MAX, 5          # query 2: the sum passes 2^31 - 1
    rows, totals = _check_merge(blocks, q)
    assert totals.tolist() == [2, INT32_MIN, INT32_MAX]
    assert (rows[1, :, 0] == -1).all() and rows[0, :, 0].tolist() == [1, 4] and rows[2, :, 0].tolist() == [3, 6]


def test_merge_refusals_write_nothing():
    lib = _lib.load()
    q = QUERIES5[:2]
    for n_lists, k, want in ((17, 4, ERR_UNSUPPORTED), (0, 4, ERR_UNSUPPORTED), (2, 65, ERR_UNSUPPORTED), (2, 0, ERR_UNSUPPORTED)):
        blocks = np.zeros((max(n_lists, 1), 2, k + 1, 4), dtype=np.int64)

        def call(b, R, Q, kk, *rest, n_lists=n_lists):
            return lib.tvz_align_wide_topk_merge(b, n_lists, Q, kk, *rest)
        rc, rows, totals = _merge(blocks, q, 0, call)
        assert rc == want, (n_lists, k, rc, lib.tvz_last_error())
        assert (rows == POISON).all() and (totals == POISON).all()
    blocks = np.zeros((2, 2, 5, 4), dtype=np.int64)
    for flags in (2, 3, 1 << 31):                                   # any bit but TVZ_ALIGN_CONTAIN
        rc, rows, totals = _merge(blocks, q, flags)
        assert rc == ERR_INVALID and b"flag" in lib.tvz_last_error() and (rows == POISON).all() and (totals == POISON).all()
    for at in (0, 7):                                              # the blocks, d_topk: 4 bytes off a 16-byte boundary
        def call(*a, at=at):
            a = list(a)
            a[at] += 4
            return lib.tvz_align_wide_topk_merge(*a)
        rc, rows, totals = _merge(blocks, q, 0, call)
        assert rc == ERR_INVALID and b"aligned" in lib.tvz_last_error(), at
        assert (rows == POISON).all() and (totals == POISON).all()
    for null_at in (0, 5, 6, 7, 8):
        def call(*a, null_at=null_at):
            a = list(a)
            a[null_at] = None
            return lib.tvz_align_wide_topk_merge(*a)
        rc, rows, totals = _merge(blocks, q, 0, call)
        assert rc == ERR_INVALID and (rows == POISON).all() and (totals == POISON).all(), null_at
    rc, rows, totals = _merge(blocks, q, 0, lambda b, R, Q, *rest: lib.tvz_align_wide_topk_merge(b, R, -1, *rest))
    assert rc == ERR_INVALID and (rows == POISON).all()
    rc, rows, totals = _merge(blocks, q, 0, lambda b, R, Q, *rest: lib.tvz_align_wide_topk_merge(b, R, 0, *rest))
    assert rc == 0 and (rows == POISON).all() and (totals == POISON).all()        # Q = 0: nothing to do


@pytest.mark.parametrize("n_lists,k", [(1, 1), (3, 63), (5, 5), (16, 64)])
def test_within_the_bounded_word_the_two_merges_agree_bit_for_bit(n_lists, k):
    rng = np.random.default_rng(7 * n_lists + k)
    lists = [[[(int(rng.integers(0, 12)), int(rng.integers(0, 41)), int(rng.integers(-2047, 2048)), int(rng.integers(0, 50)))
               for _ in range(int(rng.integers(0, 2 * k + 1)))] for _ in QUERIES5] for _ in range(n_lists)]
    blocks = _blocks(lists, QUERIES5, k)
    rows, totals = _check_merge(blocks, QUERIES5)
    d_q, d_off, _ = tc.pack_queries(QUERIES5, DEV)
    b_rows, b_totals = tc.align_topk_merge(torch.from_numpy(blocks.astype(np.int32)).to(DEV), k, d_q, d_off)
    torch.cuda.synchronize()
    assert (b_rows.cpu().numpy() == rows).all() and (b_totals.cpu().numpy() == totals).all()
    assert np.abs(rows[:, :, 2]).max() > 5                          # (bins that a word of fewer bits would lose)


# ---- 2. the split table ---------------------------------------------------------------------------------------------
def _upload_split(rows, R):
    shards = [tc.DeviceCorpus(0) for _ in range(R)]
    for r, s in enumerate(shards):
        s.upload(rows[r::R])
    return shards


def _shards_call(shards, queries, k, max_query_len=None, **kw):
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    max_len = min(longest, 4095) if max_query_len is None else max_query_len
    ws = torch.empty(tc.align_wide_topk_workspace_bytes(len(queries), max_len, d_q.numel(), k), dtype=torch.uint8, device=DEV)
    blocks, rows, totals = tc.align_wide_topk_shards(shards, d_q, d_off, max_len, eps=EPS, k=k, workspace=ws, **kw)
    torch.cuda.synchronize()
    return blocks.cpu().numpy(), rows.cpu().numpy(), totals.cpu().numpy()


@pytest.fixture(scope="module")
def split_world():
    rows, queries = wsr.split_table()
    batch = queries + [[float(i) for i in range(50)]]              # over-long at max_query_len = 45: refused everywhere
    aligned = wsr.aligned_whole(rows, batch)                        # the CPU reference's votes, once
    one = tc.DeviceCorpus(0)
    one.upload(rows)
    splits = {R: _upload_split(rows, R) for R in (1, 2, 3, 8)}
    yield rows, batch, aligned, one, splits
    for s in [one] + [h for v in splits.values() for h in v]:
        s.close()


@pytest.mark.parametrize("contain", [False, True])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_shards_equal_one_handle_and_the_reference(split_world, k, contain):
    rows, batch, aligned, one, splits = split_world
    kw = dict(contain=contain)
    ref = awr.topk_wide_ref(rows, batch, EPS, WIDEST, k, aligned=aligned, max_query_len=45, **kw)
    one_rows, one_totals = one.align_wide_topk(batch, eps=EPS, k=k, max_query_len=45, **kw)
    assert (one_rows == ref[:, :k]).all() and (one_totals == ref[:, k, 1]).all()
    assert ref[0, k, 1] > 64 and ref[-1, k, 1] == INT32_MIN and np.abs(ref[0, :k, 2]).max() > 2047  # the premises
    for R in (1, 2, 3, 8):
        blocks, got_rows, got_totals = _shards_call(splits[R], batch, k, max_query_len=45, **kw)
        assert (got_totals == one_totals).all(), (R, got_totals, one_totals)
        assert (got_rows == one_rows).all(), R
        assert (blocks[:, -1, k, 1] == INT32_MIN).all()            # the over-long query: refused by every shard


def test_shards_with_empty_and_short_shards_and_an_excluded_id(split_world):
    rows, batch, aligned, one, splits = split_world
    pick = (0, 1, 4, 7, 2)                                         # a base row, three shifted copies, an excerpt
    few = [rows[i] for i in pick]
    one5, shards = tc.DeviceCorpus(0), _upload_split(few, 8)
    try:
        one5.upload(few)
        assert [s.stats()[0] for s in shards] == [1, 1, 1, 1, 1, 0, 0, 0]
        sel = [a[list(pick)] for a in aligned]
        excl = [few[1][0], -1, -1, -1, -1, -1]
        ex = torch.tensor(excl, dtype=torch.int32, device=DEV)
        for contain in (False, True):
            for k in (1, 5, 64):                                   # every shard is shorter than k = 5 and k = 64
                ref = awr.topk_wide_ref(few, batch, EPS, WIDEST, k, contain=contain, aligned=sel, max_query_len=45)
                exp_rows, exp_totals = one5.align_wide_topk(batch, eps=EPS, k=k, contain=contain, max_query_len=45)
                blocks, got_rows, got_totals = _shards_call(shards, batch, k, max_query_len=45, contain=contain)
                assert (got_rows == exp_rows).all() and (got_totals == exp_totals).all()
                assert (got_rows == ref[:, :k]).all() and (got_totals == ref[:, k, 1]).all()
                assert got_totals[-1] == INT32_MIN and (blocks[:, -1, k, 1] == INT32_MIN).all() and got_totals[0] == 5
            kw = dict(min_votes=2, min_score=atr.ONE // 4, contain=contain)
            ref = awr.topk_wide_ref(few, batch, EPS, WIDEST, 5, exclude_ids=excl, aligned=sel, max_query_len=45, **kw)
            _, got_rows, got_totals = _shards_call(shards, batch, 5, max_query_len=45, d_exclude_ids=ex, **kw)
            assert (got_rows == ref[:, :5]).all() and (got_totals == ref[:, 5, 1]).all()
            plain = awr.topk_wide_ref(few, batch, EPS, WIDEST, 5, aligned=sel, max_query_len=45, **kw)
            assert few[1][0] in plain[0, :5, 0] and few[1][0] not in got_rows[0, :, 0]
        # a narrower search: the copies beyond max_offset are not found
        ref = awr.topk_wide_ref(few, batch, EPS, 100.0, 5, max_query_len=45)
        _, got_rows, got_totals = _shards_call(shards, batch, 5, max_query_len=45, max_offset=100.0)
        assert (got_rows == ref[:, :5]).all() and (got_totals == ref[:, 5, 1]).all()
    finally:
        for s in [one5] + shards:
            s.close()


def test_shards_refuse_before_anything_is_written(split_world):
    rows, batch, aligned, one, splits = split_world
    lib = _lib.load()
    shards = splits[2]
    queries = batch[:5]
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    Q, k = len(queries), 4
    ws = torch.empty(tc.align_wide_topk_workspace_bytes(Q, longest, d_q.numel(), k), dtype=torch.uint8, device=DEV)
    handles = (C.c_void_p * 2)(*[s._h for s in shards])
    for kw, want in (({"eps": 0.0}, ERR_INVALID), ({"max_offset": (MAX_B + 1) * EPS}, ERR_UNSUPPORTED), ({"k": 65}, ERR_UNSUPPORTED),
                     ({"min_votes": 0}, ERR_INVALID), ({"min_score": -1}, ERR_INVALID), ({"max_len": 4096}, ERR_UNSUPPORTED),
                     ({"ws_bytes": 1024}, ERR_WORKSPACE), ({"n": 17}, ERR_UNSUPPORTED), ({"n": 0}, ERR_INVALID),
                     ({"flags": 2}, ERR_INVALID), ({"blocks_off": 4}, ERR_INVALID)):
        blocks = torch.full((2, Q, k + 1, 4), POISON, dtype=torch.int32, device=DEV)
        out = torch.full((Q, k, 4), POISON, dtype=torch.int32, device=DEV)
        totals = torch.full((Q,), POISON, dtype=torch.int32, device=DEV)
        rc = lib.tvz_align_wide_topk_shards(handles, kw.get("n", 2), d_q.data_ptr(), d_off.data_ptr(), Q, kw.get("max_len", longest),
                                            kw.get("eps", EPS), kw.get("max_offset", WIDEST), kw.get("min_votes", 1),
                                            kw.get("min_score", 0), kw.get("flags", 0), None, kw.get("k", k),
                                            blocks.data_ptr() + kw.get("blocks_off", 0), out.data_ptr(), totals.data_ptr(),
                                            ws.data_ptr(), kw.get("ws_bytes", ws.numel()),
                                            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == want, (kw, rc, lib.tvz_last_error())
        assert bool((blocks == POISON).all()) and bool((out == POISON).all()) and bool((totals == POISON).all()), kw


# ---- 3. service.ShardedCorpus.align_wide_topk ----------------------------------------------------------------------
@pytest.mark.parametrize("n_shards", [8, 20])
def test_sharded_corpus_equals_the_reference(split_world, n_shards):
    from tvidz_amd import service
    rows, batch, aligned, one, splits = split_world
    sc = service.ShardedCorpus(0, n_shards=n_shards, k=8)
    try:
        assert sc.supports_align_wide is True
        sc.upload(rows)
        excl = [rows[1][0], -1, -1, -1, -1, -1]
        for kw in ({"k": 8}, {"k": 8, "contain": True, "min_votes": 3}, {"k": 3, "min_votes": 2, "exclude_ids": excl},
                   {"k": 64, "min_score": atr.ONE // 2, "contain": True}):
            ref = awr.topk_wide_ref(rows, batch, EPS, WIDEST, aligned=aligned, max_query_len=45, **kw)
            k = kw["k"]
            got = sc.align_wide_topk(batch, eps=EPS, max_query_len=45, **kw)
            assert got[0].dtype == np.int32 and got[0].shape == (len(batch), k, 4) and got[1].shape == (len(batch),)
            assert (got[0] == ref[:, :k]).all() and (got[1] == ref[:, k, 1]).all(), kw
            # tensor-pair input
            d_q, d_off, _ = tc.pack_queries(batch, DEV)
            kw2 = dict(kw)
            if "exclude_ids" in kw2:
                kw2["exclude_ids"] = torch.tensor(excl, dtype=torch.int32, device=DEV)
            got2 = sc.align_wide_topk((d_q, d_off), eps=EPS, max_offset=WIDEST, max_query_len=45, **kw2)
            assert (got2[0] == ref[:, :k]).all() and (got2[1] == ref[:, k, 1]).all(), kw
        assert ref[-1, k, 1] == INT32_MIN
    finally:
        sc.close()


# ---- 4. the Inspector over a ShardedCorpus --------------------------------------------------------------------------
FILM = [100.0 + 7.0 * i + 0.05 * i * i for i in range(40)]          # no two gaps alike: one shift aligns the excerpt
CUTS = {"film.y4m": FILM, "other.y4m": [3.0 + 11.0 * i + 0.07 * i * i for i in range(30)],
        "clip.y4m": [c - 150.0 for c in FILM[12:32]]}              # 20 of the film's cuts, 4,500 bins of 1/30 s earlier


def test_inspector_finds_an_excerpt_on_another_shard_beyond_2047_bins(tmp_path):
    from tests.fakes import CutReader, cut_inspector
    from tvidz_amd import db as tdb, service
    sc = service.ShardedCorpus(0, n_shards=8, k=8)
    store = tdb.Store(f"sqlite:///{tmp_path}/t.db", corpus=sc)
    ins = cut_inspector(store, device=DEV, near_duplicates=True, near_top_k=4, near_any_offset=True,
                        near_score="containment", near_min_votes=5,
                        frame_source=lambda bucket, key, filename, uid: (CutReader(CUTS[key], frames=12000), None))
    try:
        res = [ins.analyze_file("videos", k) for k in ("film.y4m", "other.y4m", "clip.y4m")]
        assert all(r["status"] == "done" and r["duplicates"] == [] for r in res), res
        assert res[0]["near_duplicates"] == [] and res[1]["near_duplicates"] == []
        (near,) = res[2]["near_duplicates"]
        assert near["filename"] == "film.y4m" and near["containment"] == 1.0 and near["jaccard"] == 0.5
        assert abs(near["shift_seconds"] - 150.0) < 1 / 30 and near["shift_seconds"] / EPS > 2047
        film_id = near["video_id"]
        homes = [r for r, s in enumerate(sc.shards) if s.stats()[0]]
        assert len(homes) == 3 and sc._shard_of(film_id) in homes           # three uploads, three shards: the film's is another
        # the bounded search of the same driver does not reach it: it finds the clip's own row alone
        rows, totals = sc.align_topk([CUTS["clip.y4m"]], eps=EPS, max_offset=30.0, k=4, min_votes=5)
        assert totals.tolist() == [1] and film_id not in rows[0, :, 0] and rows[0, 0, 2:].tolist() == [0, 20]
    finally:
        store.close()                      # closes the corpus too


# ---- 5. the RCCL form at world size 1 and the one-rank RankCorpus, in a fresh child process ---------------------------
@pytest.fixture(scope="module")
def comm_child(tmp_path_factory):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "near_wide_comm_child.py"),
                          str(tmp_path_factory.mktemp("near_wide"))], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_align_wide_topk_sharded_through_rccl_world_size_1(comm_child):
    res = comm_child
    assert res["premise_hits"] > 5 and res["premise_bin"] > 2047    # more hits than k = 5, found beyond the bounded word
    for name in ("k5", "k64", "k5_contain", "k5_filtered"):
        assert res[name]["rows"] == res[name]["one_rows"] and res[name]["totals"] == res[name]["one_totals"], name
    assert res["k5"]["rows"] != res["k5_contain"]["rows"]
    assert res["k5"]["totals"][-1] == INT32_MIN                    # the over-long query stays refused
    assert res["matcher_equal"] is True and res["matcher_slots_equal"] is True
    # its workspace (tvz_align_wide_topk_sharded_workspace_bytes): exact and misaligned slices stay inside; the exact
    # size of the least the call takes succeeds, one byte below it is TVZ_ERR_WORKSPACE
    assert res["workspace_bounds_ok"] == [True, True, True]
    assert res["workspace_exact"] == [0, True, 0]
    rc, msg = res["workspace_short"]
    assert rc == ERR_WORKSPACE and " 1 bytes missing" in msg and "tvz_align_wide_topk_sharded_workspace_bytes" in msg, msg
    rc, msg = res["unknown_flag"]
    assert rc == ERR_INVALID and "flag" in msg


def test_inspector_over_a_one_rank_rank_corpus(comm_child):
    res = comm_child
    assert res["near_rank"] == res["near_plain"]
    (near,) = res["near_rank"][2]
    assert near["filename"] == "film.y4m" and near["containment"] == 1.0 and near["jaccard"] == 0.5
    assert abs(near["shift_seconds"] - 150.0) < 1 / 30
    assert res["near_rank"][0] == [] and res["near_rank"][1] == []
    assert res["near_bad_param"] == "ValueError" and res["rank_broken"] is None
