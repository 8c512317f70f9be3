"""Child process of tests/test_align_wide_sharded_gpu.py: creates the libtvz RCCL communicator BEFORE its first GPU
call (as tests/near_comm_child.py does), then runs at world size 1
  - tvz_align_wide_topk_sharded against tvz_align_wide_topk on the same handle, through corpus.Comm and through
    sharded.RcclShardedMatcher (every side stream), both score kinds, and its workspace's bounds;
  - the Inspector with near_any_offset and the containment score over a one-rank service.RankCorpus(RcclShardedMatcher)
    against the same driver over a plain DeviceCorpus,
and prints the results as JSON.  argv[1]: a directory for the SQLite files."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (import only: no GPU call yet)

from tests import align_topk_ref as atr, align_wide_shard_ref as wsr  # noqa: E402
from tvidz_amd import _lib, corpus as tc, sharded  # noqa: E402

comm = tc.Comm(tc.Comm.unique_id(), 1, 0, 0)           # ncclCommInitRank: the first GPU call of this process
dev = torch.device("cuda:0")
EPS = wsr.EPS
rows, queries = wsr.split_table()
batch = queries + [[float(i) for i in range(50)]]      # over-long at max_query_len = 45
dc = tc.DeviceCorpus(0)
dc.upload(rows)
d_q, d_off, _ = tc.pack_queries(batch, dev)
Q = len(batch)
out = {}
excl = [rows[1][0], -1, -1, -1, -1, -1]
d_ex = torch.tensor(excl, dtype=torch.int32, device=dev)
for name, k, kw, dkw in (("k5", 5, {}, {}), ("k64", 64, {}, {}), ("k5_contain", 5, dict(contain=True), dict(contain=True)),
                         ("k5_filtered", 5, dict(min_votes=2, min_score=atr.ONE // 4, contain=True, exclude_ids=excl),
                          dict(min_votes=2, min_score=atr.ONE // 4, contain=True, d_exclude_ids=d_ex))):
    one_rows, one_totals = dc.align_wide_topk(batch, eps=EPS, k=k, max_query_len=45, **kw)
    r, t = comm.align_wide_topk_sharded(dc, d_q, d_off, 45, eps=EPS, k=k, **dkw)
    torch.cuda.synchronize()
    out[name] = {"rows": r.cpu().tolist(), "totals": t.cpu().tolist(), "one_rows": one_rows.tolist(),
                 "one_totals": one_totals.tolist()}
out["premise_hits"] = int(out["k5"]["one_totals"][0])
out["premise_bin"] = max(abs(int(r[2])) for r in out["k5"]["one_rows"][0])
# the matcher: every side stream in turn, each answer equal to the plain call's
sm = sharded.RcclShardedMatcher(dc, comm, k=16, cap=64)
want_r, want_t = torch.tensor(out["k5"]["rows"], dtype=torch.int32), torch.tensor(out["k5"]["totals"], dtype=torch.int32)
same = []
for _ in range(3):
    r, t = sm.align_wide_topk(d_q, d_off, 45, eps=EPS, k=5)
    torch.cuda.synchronize()
    same.append(torch.equal(r.cpu(), want_r) and torch.equal(t.cpu(), want_t))
out["matcher_equal"] = bool(same[0]) and sm.supports_align_wide is True
out["matcher_slots_equal"] = bool(all(same))
# the workspace: exactly sized and misaligned inside a poisoned buffer
n = tc.align_wide_topk_sharded_workspace_bytes(Q, 45, d_q.numel(), 5, 1)
bounds = []
for extra in (0, 8, 248):
    buf = torch.full((4096 + 256 + n + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    lo, hi = 4096 + extra, 4096 + extra + n
    r, t = comm.align_wide_topk_sharded(dc, d_q, d_off, 45, eps=EPS, k=5, workspace=buf[lo:hi])
    torch.cuda.synchronize()
    bounds.append(bool((buf[:lo] == 0xA5).all()) and bool((buf[hi:] == 0xA5).all()) and torch.equal(r.cpu(), want_r)
                  and torch.equal(t.cpu(), want_t))
out["workspace_bounds_ok"] = bounds


def raw_call(ws_ptr, ws_bytes, r5, t5, flags=0):
    """The library call itself: corpus.Comm checks the size before it would."""
    return comm.lib.tvz_align_wide_topk_sharded(dc._h, comm._h, d_q.data_ptr(), d_off.data_ptr(), Q, 45, EPS,
                                                tc.ALIGN_WIDE_MAX_B * EPS, 1, 0, flags, None, 5, r5.data_ptr(), t5.data_ptr(),
                                                ws_ptr, ws_bytes, torch.cuda.current_stream().cuda_stream)


# the size the sizing function gives for these queries succeeds; one byte below the least the call takes - the fixed
# parts, the blocks and ONE query of max_query_len values (a workspace between that and the full size is taken: queries
# that do not fit it are refused one by one) - is refused
ws = torch.empty(n, dtype=torch.uint8, device=dev)
r5, t5 = torch.empty((Q, 5, 4), dtype=torch.int32, device=dev), torch.empty(Q, dtype=torch.int32, device=dev)
rc_exact = raw_call(ws.data_ptr(), n, r5, t5)
torch.cuda.synchronize()
out["workspace_exact"] = [int(rc_exact), bool(torch.equal(r5.cpu(), want_r) and torch.equal(t5.cpu(), want_t))]
least = tc.align_wide_topk_sharded_workspace_bytes(Q, 45, 45, 5, 1)
out["workspace_exact"].append(int(raw_call(ws.data_ptr(), least, r5, t5)))
torch.cuda.synchronize()
rc_short = raw_call(ws.data_ptr(), least - 1, r5, t5)
out["workspace_short"] = [int(rc_short), (_lib.load().tvz_last_error() or b"").decode()]
rc_flag = raw_call(ws.data_ptr(), n, r5, t5, flags=2)
out["unknown_flag"] = [int(rc_flag), (_lib.load().tvz_last_error() or b"").decode()]
torch.cuda.synchronize()
dc.close()

# ---- the driver: Inspector(near_any_offset=True) over a plain DeviceCorpus and over a one-rank RankCorpus -----------
from tests.fakes import CutReader, cut_inspector  # noqa: E402
from tvidz_amd import db as tdb, service  # noqa: E402

film = [100.0 + 7.0 * i + 0.05 * i * i for i in range(40)]                   # no two gaps alike: one shift aligns
cuts = {"film.y4m": film, "other.y4m": [3.0 + 11.0 * i + 0.07 * i * i for i in range(30)],
        "clip.y4m": [c - 150.0 for c in film[12:32]]}                         # 20 of its cuts, 4,500 bins of 1/30 s earlier


def run(corpus, name):
    store = tdb.Store(f"sqlite:///{sys.argv[1]}/{name}.db", corpus=corpus)
    ins = cut_inspector(store, device="cuda:0", near_duplicates=True, near_top_k=4, near_any_offset=True,
                        near_score="containment", near_min_votes=5,
                        frame_source=lambda bucket, key, filename, uid: (CutReader(cuts[key], frames=12000), None))
    try:
        res = [ins.analyze_file("videos", k) for k in ("film.y4m", "other.y4m", "clip.y4m")]
        assert all(r["status"] == "done" for r in res), res
        return [r["near_duplicates"] for r in res]
    finally:
        store.close()                      # closes the corpus too


out["near_plain"] = run(tc.DeviceCorpus(0), "plain")
shard = tc.DeviceCorpus(0)
rc = service.RankCorpus(shard, sharded.RcclShardedMatcher(shard, comm, k=8, cap=64), xdev="cpu")
try:
    rc.align_wide_topk([[1.0, 2.0]], eps=EPS, max_offset=(tc.ALIGN_WIDE_MAX_B + 1) * EPS, k=4)
    out["near_bad_param"] = "accepted"
except ValueError:
    out["near_bad_param"] = "ValueError"
out["near_rank"] = run(rc, "rank")
out["rank_broken"] = repr(rc.broken) if rc.broken else None
comm.close()
print("RESULT " + json.dumps(out))
