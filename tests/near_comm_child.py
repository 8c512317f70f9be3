"""Child process of tests/test_align_topk_sharded_gpu.py: creates the libtvz RCCL communicator BEFORE its first GPU
call (as tests/comm_child.py does), then runs at world size 1
  - tvz_align_topk_sharded against tvz_align_topk on the same handle, through corpus.Comm and through
    sharded.RcclShardedMatcher (every side stream), and its workspace's bounds;
  - the Inspector with near_top_k = 4 over a one-rank service.RankCorpus(RcclShardedMatcher) against the same driver
    over a plain DeviceCorpus,
and prints the results as JSON.  argv[1]: a directory for the SQLite files."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (import only: no GPU call yet)

from tests import align_topk_ref as atr, align_topk_shard_ref as asr  # noqa: E402
from tvidz_amd import corpus as tc, sharded  # noqa: E402

try:
    comm = tc.Comm(tc.Comm.unique_id(), 1, 0, 0)       # ncclCommInitRank: the first GPU call of this process
except RuntimeError as e:
    if "RCCL is not available" in str(e):
        print("RCCL is not available")
        sys.exit(3)
    raise
dev = torch.device("cuda:0")
EPS, MAX_OFFSET = 1 / 30, 3.0
rows, queries = asr.split_table()
batch = queries + [[float(i) for i in range(50)]]      # over-long at max_query_len = 45
dc = tc.DeviceCorpus(0)
dc.upload(rows)
d_q, d_off, _ = tc.pack_queries(batch, dev)
out = {}
excl = [rows[1][0], -1, -1, -1, -1, -1]
d_ex = torch.tensor(excl, dtype=torch.int32, device=dev)
for name, k, kw, dkw in (("k5", 5, {}, {}), ("k64", 64, {}, {}),
                         ("k5_filtered", 5, dict(min_votes=2, min_score=atr.ONE // 4, exclude_ids=excl),
                          dict(min_votes=2, min_score=atr.ONE // 4, d_exclude_ids=d_ex))):
    one_rows, one_totals = dc.align_topk(batch, eps=EPS, max_offset=MAX_OFFSET, k=k, max_query_len=45, **kw)
    r, t = comm.align_topk_sharded(dc, d_q, d_off, 45, eps=EPS, max_offset=MAX_OFFSET, k=k, **dkw)
    torch.cuda.synchronize()
    out[name] = {"rows": r.cpu().tolist(), "totals": t.cpu().tolist(), "one_rows": one_rows.tolist(),
                 "one_totals": one_totals.tolist()}
out["premise_hits"] = int(out["k5"]["one_totals"][0])
# the matcher: every side stream in turn, each answer equal to the plain call's
sm = sharded.RcclShardedMatcher(dc, comm, k=16, cap=64)
want_r, want_t = torch.tensor(out["k5"]["rows"], dtype=torch.int32), torch.tensor(out["k5"]["totals"], dtype=torch.int32)
same = []
for _ in range(3):
    r, t = sm.align_topk(d_q, d_off, 45, eps=EPS, max_offset=MAX_OFFSET, k=5)
    torch.cuda.synchronize()
    same.append(torch.equal(r.cpu(), want_r) and torch.equal(t.cpu(), want_t))
out["matcher_equal"] = bool(same[0])
out["matcher_slots_equal"] = bool(all(same))
# the workspace: exactly sized and misaligned inside a poisoned buffer; one byte short
n = tc.align_topk_sharded_workspace_bytes(len(batch), 45, d_q.numel(), 5, 1)
bounds = []
for extra in (0, 8, 248):
    buf = torch.full((4096 + 256 + n + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    lo, hi = 4096 + extra, 4096 + extra + n
    r, t = comm.align_topk_sharded(dc, d_q, d_off, 45, eps=EPS, max_offset=MAX_OFFSET, k=5, workspace=buf[lo:hi])
    torch.cuda.synchronize()
    bounds.append(bool((buf[:lo] == 0xA5).all()) and bool((buf[hi:] == 0xA5).all()) and torch.equal(r.cpu(), want_r)
                  and torch.equal(t.cpu(), want_t))
out["workspace_bounds_ok"] = bounds
# one byte below the least the call takes - the fixed parts, the blocks and ONE query of max_query_len values (a
# workspace between that and `n` is taken: queries that do not fit it are refused one by one).  The library call
# itself: corpus.Comm checks the size before it would.
from tvidz_amd import _lib  # noqa: E402
n = tc.align_topk_sharded_workspace_bytes(len(batch), 45, 45, 5, 1)
ws = torch.empty(n, dtype=torch.uint8, device=dev)
r5, t5 = torch.empty((len(batch), 5, 4), dtype=torch.int32, device=dev), torch.empty(len(batch), dtype=torch.int32, device=dev)
rc_short = comm.lib.tvz_align_topk_sharded(dc._h, comm._h, d_q.data_ptr(), d_off.data_ptr(), len(batch), 45, EPS, MAX_OFFSET,
                                           1, 0, None, 5, r5.data_ptr(), t5.data_ptr(), ws.data_ptr(), n - 1,
                                           torch.cuda.current_stream().cuda_stream)
out["workspace_short"] = [int(rc_short), (_lib.load().tvz_last_error() or b"").decode()]
dc.close()

# ---- the driver: Inspector(near_top_k=4) over a plain DeviceCorpus and over a one-rank RankCorpus -------------------
from tests.fakes import CutReader, cut_inspector  # noqa: E402
from tvidz_amd import db as tdb, service  # noqa: E402

cuts = {"a.y4m": [1.0, 2.5, 4.0, 7.3, 9.9, 12.0], "c.y4m": [0.7, 3.3, 5.1, 8.8],
        "b.y4m": [x + 7 / 30 for x in [1.0, 2.5, 4.0, 7.3, 9.9, 12.0]]}      # b = a, cut-shifted by seven frames


def run(corpus, name):
    store = tdb.Store(f"sqlite:///{sys.argv[1]}/{name}.db", corpus=corpus)
    ins = cut_inspector(store, device="cuda:0", near_duplicates=True, near_top_k=4,
                        frame_source=lambda bucket, key, filename, uid: (CutReader(cuts[key], frames=600), None))
    try:
        res = [ins.analyze_file("videos", k) for k in ("a.y4m", "c.y4m", "b.y4m")]
        assert all(r["status"] == "done" for r in res), res
        return [r["near_duplicates"] for r in res]
    finally:
        store.close()                      # closes the corpus too


out["near_plain"] = run(tc.DeviceCorpus(0), "plain")
shard = tc.DeviceCorpus(0)
rc = service.RankCorpus(shard, sharded.RcclShardedMatcher(shard, comm, k=8, cap=64), xdev="cpu")
try:
    rc.align_topk([[1.0, 2.0]], eps=0.0, max_offset=1.0, k=4)
    out["near_bad_param"] = "accepted"
except ValueError:
    out["near_bad_param"] = "ValueError"
out["near_rank"] = run(rc, "rank")
out["rank_broken"] = repr(rc.broken) if rc.broken else None
comm.close()
print("RESULT " + json.dumps(out))
