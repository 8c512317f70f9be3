"""Child process of tests/test_gap_candidates_service_gpu.py: creates the libtvz RCCL communicator BEFORE its first GPU
call (as tests/near_service_comm_child.py does), then runs at world size 1
  - tvz_align_candidates_sharded against the plain call on the same handle, through corpus.Comm and through
    sharded.RcclShardedMatcher (every side stream), with its workspace's bounds and the refusals that come behind the
    plain call's;
  - the Inspector with near_candidates over a one-rank service.RankCorpus(RcclShardedMatcher) against the same driver
    over a plain DeviceCorpus,
and prints the results as JSON."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (import only: no GPU call yet)

from tests import gap_candidates_cases as cs  # noqa: E402
from tvidz_amd import corpus as tc, sharded  # noqa: E402

comm = tc.Comm(tc.Comm.unique_id(), 1, 0, 0)           # ncclCommInitRank: the first GPU call of this process
dev = torch.device("cuda:0")
EPS = cs.GAP_EPS
rows, uploads = cs.table() + cs.counting_table(65), cs.uploads()
batch = [uploads[n] for n in ("shifted", "excerpt", "twin", "special", "stranger")] + [cs.counting_query(), cs.long_query(515, 2)]
dc = tc.DeviceCorpus(0)
dc.upload(rows)
dc.set_gap_index(EPS)
d_q, d_off, L = tc.pack_queries(batch, dev)
Q = len(batch)
lib = comm.lib
out = {"equal": {}, "premise": {}}
excl = [cs.FILM, -1, cs.TWIN, -1, -1, 5000, -1]
d_ex = torch.tensor(excl, dtype=torch.int32, device=dev)
err = lambda: (lib.tvz_last_error() or b"").decode()                            # noqa: E731


def same(a, b):
    return bool(torch.equal(torch.as_tensor(np.asarray(a)), torch.as_tensor(np.asarray(b))))


# ---- 1. the sharded call equals the plain call bit for bit -----------------------------------------------------------
for c in (1, 16, 64):
    for name, kw in (("plain", dict(min_count=1)), ("min_count 6", dict(min_count=6)), ("cap 64", dict(min_count=1, cap=64)),
                     ("excluded", dict(min_count=1, d_exclude_ids=d_ex))):
        one = dc.align_candidates_block(d_q, d_off, L, c=c, **kw)
        got = comm.align_candidates_sharded(dc, d_q, d_off, L, c=c, **kw)
        torch.cuda.synchronize()
        out["equal"][f"C={c} {name}"] = same(got.cpu(), one.cpu()) and tuple(got.shape) == (Q, c + 1, 2)
        if c == 16:
            h = one.cpu().numpy()
            out["premise"][name] = {"totals": h[:, c, 1].tolist(), "first": h[:, 0].tolist()}
empty = comm.align_candidates_sharded(dc, d_q[:0], d_off[:1], 0, c=4)
out["equal"]["no query"] = tuple(empty.shape) == (0, 5, 2)

# ---- 2. the matcher: every side stream in turn --------------------------------------------------------------------------
sm = sharded.RcclShardedMatcher(dc, comm, k=16, cap=64)
out["matcher_supports"] = bool(sm.supports_align_candidates)
want = dc.align_candidates_block(d_q, d_off, L, c=16, min_count=1, d_exclude_ids=d_ex).cpu()
slots = []
for _ in range(3):
    got = sm.candidates(d_q, d_off, L, c=16, min_count=1, d_exclude_ids=d_ex)
    torch.cuda.synchronize()
    slots.append(same(got.cpu(), want))
out["matcher_slots_equal"] = slots

# ---- 3. the workspace: exactly the sharded sizing function's bytes inside a poisoned buffer; one byte less; refusals ----
stream = lambda: torch.cuda.current_stream().cuda_stream                        # noqa: E731
C16, CAP = 16, 128


def raw(comm_h, ws_ptr, ws_bytes, out_t, c=C16, cap=CAP, min_count=1, handle=None):
    return lib.tvz_align_candidates_sharded(dc._h if handle is None else handle, comm_h, d_q.data_ptr(), d_off.data_ptr(), Q, int(L),
                                            min_count, None, cap, c, out_t.data_ptr() if out_t is not None else None, ws_ptr, ws_bytes,
                                            stream())


SENT = -0x5A5A5A5A
want = dc.align_candidates_block(d_q, d_off, L, c=C16, min_count=1, cap=CAP).cpu()
n = tc.align_candidates_sharded_workspace_bytes(Q, L, d_q.numel(), CAP, C16, 1)
least = tc.align_candidates_sharded_workspace_bytes(Q, L, L, CAP, C16, 1)
res = []
for extra in (0, 8, 248):
    buf = torch.full((4096 + 256 + n + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    lo = 4096 + (-(buf.data_ptr() + 4096)) % 256 + extra
    o = torch.full((Q + 2, C16 + 1, 2), SENT, dtype=torch.int32, device=dev)
    rc = raw(comm._h, buf.data_ptr() + lo, n, o[1:Q + 1])
    torch.cuda.synchronize()
    res.append(rc == 0 and bool((buf[:lo] == 0xA5).all()) and bool((buf[lo + n:] == 0xA5).all()) and same(o[1:Q + 1].cpu(), want)
               and bool((o[0] == SENT).all()) and bool((o[Q + 1] == SENT).all()))
ws = torch.empty(n, dtype=torch.uint8, device=dev)
o = torch.full((Q, C16 + 1, 2), SENT, dtype=torch.int32, device=dev)
refusals = {}
refusals["short"] = [raw(comm._h, ws.data_ptr(), least - 1, o), err()]
refusals["full_short"] = [raw(comm._h, ws.data_ptr(), 0, o), err()]
refusals["null_comm"] = [raw(None, ws.data_ptr(), n, o), err()]
refusals["null_comm_and_c65"] = [raw(None, ws.data_ptr(), n, o, c=65, cap=100), err()]
refusals["null_comm_and_cap"] = [raw(None, ws.data_ptr(), n, o, cap=3), err()]
refusals["null_comm_and_min_count"] = [raw(None, ws.data_ptr(), n, o, min_count=0), err()]
refusals["null_comm_and_short"] = [raw(None, ws.data_ptr(), least - 1, o), err()]
refusals["null_out"] = [raw(comm._h, ws.data_ptr(), n, None), err()]
nogap = tc.DeviceCorpus(0)
nogap.upload(rows[:5])
refusals["null_comm_and_no_codes"] = [raw(None, ws.data_ptr(), n, o, handle=nogap._h), err()]
nogap.close()
torch.cuda.synchronize()
refusals["nothing_written"] = bool((o == SENT).all())
refusals["least_ok"] = raw(comm._h, ws.data_ptr(), least, o)
torch.cuda.synchronize()
out["bounds"] = {"exact": res, "sizes": [n, least, tc.align_candidates_workspace_bytes(Q, L, d_q.numel(), CAP, C16)], **refusals}

# ---- 4. the driver: Inspector._near over a plain DeviceCorpus and over a one-rank RankCorpus --------------------------
from tvidz_amd import inspector as insp, service  # noqa: E402

base = dict(device="cuda:0", near_duplicates=True, near_top_k=8, near_any_offset=True, near_candidates=16, near_gap_eps=EPS)
scenarios = {f"{name} {i}": (uploads[name], dict(base, **kw))
             for name in ("inserted", "shifted", "removed", "excerpt", "stranger")
             for i, kw in enumerate((dict(near_score="local", near_min_votes=8, near_jaccard=0.9, near_parts=2),
                                     dict(near_score="jaccard", near_jaccard=0.3)))}
scenarios["refused upload"] = (cs.long_query(600, 4), dict(base, near_score="jaccard", near_jaccard=0.3))


def run(corpus):
    class Store:
        def get_video_by_id(self, vid):
            return None
    Store.corpus = corpus
    return {name: insp.Inspector(Store(), **kw)._near(424242, upload) for name, (upload, kw) in scenarios.items()}


out["near_plain"] = run(dc)
shard = tc.DeviceCorpus(0)
rc = service.RankCorpus(shard, sharded.RcclShardedMatcher(shard, comm, k=8, cap=64), xdev="cpu")
rc.upload(rows)
out["rank_supports"] = [rc.supports_align_candidates, rc.supports_align_parts]
out["near_rank"] = run(rc)
out["rank_gap_stats"] = rc.gap_index_stats()
r1, t1 = dc.align_candidates(batch, c=16, min_count=1, exclude_ids=excl)
r2, t2 = rc.align_candidates(batch, c=16, min_count=1, exclude_ids=excl)
out["rank_equals_plain"] = same(r1, r2) and same(t1, t2)
ticks = rc.busy_ticks
refused = []
for call in (lambda: rc.align_candidates([[1.0, 2.0]], c=0), lambda: rc.align_candidates([[1.0, 2.0]], c=16, cap=15),
             lambda: rc.align_candidates([[1.0, 2.0]], c=16, min_count=0)):
    try:
        call()
        refused.append("accepted")
    except ValueError:
        refused.append("ValueError")
long_rows, long_totals = rc.align_candidates([[0.5] * 4096], c=4)
out["caller"] = {"refused": refused, "long_totals": long_totals.tolist(), "long_rows_padding": bool((long_rows == (-1, 0)).all()),
                 "ticks_unchanged": rc.busy_ticks == ticks}
out["rank_broken"] = repr(rc.broken) if rc.broken else None
rc.close()
dc.close()
comm.close()
print("RESULT " + json.dumps(out))
