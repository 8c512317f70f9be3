"""Four lives of one corpus handle, each through every GPU resource the handle owns - the match events, the mutation
and build streams, the pinned upsert ring, both directories of both index generations, the build's scratch and its
pinned swap buffers (re-allocated by a larger reservation) - and what tvz_corpus_destroy leaves behind.

Every result is compared exactly with the restatements (oracle.find_duplicates_py, tests/tol_ref.py); the device's free
memory after the fourth close may lie below the one after the first (which absorbs the runtime's one-time allocations)
by at most ALLOWANCE.

ALLOWANCE = the largest drift of this same file on the commit before (hand-written frees) + 64 KiB.  64 KiB is less than
any row, key, directory, postings or snapshot buffer of this handle (rows: 6.4 MB at this reservation, keys: 16 MiB,
a bucket directory: 256 buckets x 128 B = 32 KiB at the least, plus its external area), so one such buffer leaked per
life - three between the two readings - fails the test.  A leaked 4 KiB counter array would not.
NOT MEASURED YET: no GPU could be had while this test was written, neither for the three runs on the commit before nor
for this one.  PARENT_DRIFT = 0 stands for "a handle that frees everything leaves nothing": replace it by the largest
of three measured drifts (the test prints every reading) before trusting a failure that is smaller than a buffer.
"""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import tol_ref
from tvidz_amd import corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CELL, TOL = 0.01, 0.001
PARENT_DRIFT = 0                     # bytes: see above
ALLOWANCE = PARENT_DRIFT + 64 * 1024


def _rows(rng, first_id, n):
    grid = np.arange(1, 3000) / 25.0
    rows = [(first_id + i, rng.choice(grid, size=8, replace=False).tolist()) for i in range(n)]
    for i in range(0, n - 1, 7):                              # near duplicates: six of eight timestamps shared
        rows[i + 1] = (rows[i + 1][0], rows[i][1][:6] + rows[i + 1][1][6:])
    return rows


def _one_life(uploaded, upserted, asks, batch, want):
    h = tc.DeviceCorpus(0)
    try:
        h.upload(uploaded)                                    # one sub-index: the bucket directory
        h.set_tol_index(CELL)                                 # rebuilt, now with the classic cell directory beside it
        h.reserve(400_000, 1_000_000)                         # the delta capacity grows: new pinned swap buffers
        for vid, ts in upserted:                              # past delta_trigger = 512: a background rebuild and a swap
            h.upsert(vid, ts)
        for q, exact, near, tolerant in asks:
            assert sorted(h.find_duplicates(q, 5)) == exact
            assert sorted(h.find_duplicates(near, 5, with_kth=True, tolerance=TOL)) == tolerant
        d_q, d_off, ml = tc.pack_queries(batch, DEV)
        hits, n = h.match_tol(d_q, d_off, ml, TOL, 2, 2048)   # the new generation's cell directory + the delta sweep
        torch.cuda.synchronize()
        hits, n = hits.cpu().numpy(), n.cpu().numpy()
        got = [(int(n[i]), sorted(map(tuple, hits[i, :int(n[i])].tolist()))) for i in range(len(batch))]
        assert got == want
        st, tst = h.index_stats(), h.tol_index_stats()
        assert st["builds"] >= 3 and tst["builds"] >= 2 and st["delta_rows"] < 600, (st, tst)
        assert tst["cell"] == CELL and tst["postings"] > 0 and st["indexed_rows"] > 600
    finally:
        h.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def test_four_lives_of_a_handle_leave_nothing_behind():
    rng = np.random.default_rng(5)
    uploaded, upserted = _rows(rng, 1, 600), _rows(rng, 100_001, 600)
    rows_now = uploaded + upserted
    asks = []
    for vid, ts in (uploaded[7], upserted[595]):              # one row of the index, one the delta table holds
        near = (np.asarray(ts) + 0.0004).tolist()
        asks.append((ts, sorted(oracle.find_duplicates_py(rows_now, ts, 5)),
                     near, tol_ref.find_duplicates_tol(rows_now, near, TOL, 5, -1, form="sorted")))
        assert (vid, 8) in asks[-1][1] and (vid, 8, 4) in asks[-1][3]
    assert len(asks[0][1]) > 1 and len(asks[0][3]) > 1        # (uploaded[7] and its near duplicate)
    batch = [(np.asarray(rows_now[i][1]) + 0.0004).tolist() for i in (0, 300, 700, 1199)]
    want = []
    for q in batch:
        exp = tol_ref.find_duplicates_tol(rows_now, q, TOL, 2, -1, form="sorted")
        want.append((len(exp), exp))
    free = [_one_life(uploaded, upserted, asks, batch, want) for _ in range(4)]
    drift = free[0] - free[3]
    print(f"free device memory after each close: {free}; drift first to fourth: {drift} bytes (allowance {ALLOWANCE})")
    assert drift <= ALLOWANCE, (free, drift)
