"""Child process of tests/test_gap_candidates_rates_service_gpu.py: creates the libtvz RCCL communicator BEFORE its first
GPU call (as tests/gap_candidates_comm_child.py does), then runs at world size 1
  - tvz_align_candidates_rates_sharded against the plain rates call on the same handle, through corpus.Comm and through
    sharded.RcclShardedMatcher (every side stream), the workspace one byte short and the NULL communicator behind the
    plain refusals;
  - the Inspector with near_candidate_rates over a one-rank service.RankCorpus(RcclShardedMatcher) against the same
    driver over a plain DeviceCorpus, and RankCorpus.align_candidates_rates through the tick,
and prints the results as JSON."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (import only: no GPU call yet)

from tests import gap_candidates_rates_cases as rc  # noqa: E402
from tvidz_amd import corpus as tc, sharded  # noqa: E402

comm = tc.Comm(tc.Comm.unique_id(), 1, 0, 0)           # ncclCommInitRank: the first GPU call of this process
dev = torch.device("cuda:0")
EPS = rc.GAP_EPS
rows, batch, excl = rc.table(), rc.queries(), rc.exclusions()
dc = tc.DeviceCorpus(0)
dc.upload(rows)
dc.set_gap_index(EPS)
d_q, d_off, L = tc.pack_queries(batch, dev)
Q = len(batch)
lib = comm.lib
out = {"equal": {}}
d_ex = torch.tensor(excl, dtype=torch.int32, device=dev)
err = lambda: (lib.tvz_last_error() or b"").decode()                            # noqa: E731


def same(a, b):
    return bool(torch.equal(torch.as_tensor(np.asarray(a)), torch.as_tensor(np.asarray(b))))


# ---- 1. the sharded call equals the plain rates call bit for bit -----------------------------------------------------
for rates in (rc.RATES1, rc.RATES3, rc.RATES8):
    for c in (1, 16, 64):
        for name, kw in (("plain", dict(min_count=1)), ("min_count 6", dict(min_count=6)),
                         ("excluded", dict(min_count=1, d_exclude_ids=d_ex))):
            one = dc.align_candidates_rates_block(d_q, d_off, L, rates, c=c, **kw)
            got = comm.align_candidates_rates_sharded(dc, d_q, d_off, L, rates, c=c, **kw)
            torch.cuda.synchronize()
            out["equal"][f"R={len(rates)} C={c} {name}"] = same(got.cpu(), one.cpu()) and tuple(got.shape) == (Q, c + 1, 3)
empty = comm.align_candidates_rates_sharded(dc, d_q[:0], d_off[:1], 0, rc.RATES3, c=4)
out["equal"]["no query"] = tuple(empty.shape) == (0, 5, 3)
out["first"] = dc.align_candidates_rates_block(d_q, d_off, L, rc.RATES3, c=16, min_count=1).cpu().numpy()[:, 0].tolist()

# ---- 2. the matcher: every side stream in turn -----------------------------------------------------------------------
sm = sharded.RcclShardedMatcher(dc, comm, k=16, cap=64)
out["matcher_supports"] = bool(sm.supports_align_candidate_rates)
want = dc.align_candidates_rates_block(d_q, d_off, L, rc.RATES3, c=16, min_count=1, d_exclude_ids=d_ex).cpu()
slots = []
for _ in range(3):
    got = sm.candidates_rates(d_q, d_off, L, rc.RATES3, c=16, min_count=1, d_exclude_ids=d_ex)
    torch.cuda.synchronize()
    slots.append(same(got.cpu(), want))
out["matcher_slots_equal"] = slots

# ---- 3. the workspace one byte short; the refusals behind the plain call's -------------------------------------------
import ctypes as C  # noqa: E402

stream = lambda: torch.cuda.current_stream().cuda_stream                        # noqa: E731
C16, CAP = 16, 128
h3 = (C.c_double * 3)(*rc.RATES3)


def raw(comm_h, ws_ptr, ws_bytes, out_t, c=C16, cap=CAP, min_count=1, handle=None, rates=h3, n_rates=3):
    return lib.tvz_align_candidates_rates_sharded(dc._h if handle is None else handle, comm_h, d_q.data_ptr(), d_off.data_ptr(), Q,
                                                  int(L), rates, n_rates, min_count, None, cap, c,
                                                  out_t.data_ptr() if out_t is not None else None, ws_ptr, ws_bytes, stream())


SENT = -0x5A5A5A5A
want = dc.align_candidates_rates_block(d_q, d_off, L, rc.RATES3, c=C16, min_count=1, cap=CAP).cpu()
n = tc.align_candidates_rates_sharded_workspace_bytes(Q, L, d_q.numel(), 3, CAP, C16, 1)
least = tc.align_candidates_rates_sharded_workspace_bytes(Q, L, L, 3, CAP, C16, 1)
res = []
for extra in (0, 8, 248):
    buf = torch.full((4096 + 256 + n + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    lo = 4096 + (-(buf.data_ptr() + 4096)) % 256 + extra
    o = torch.full((Q + 2, C16 + 1, 3), SENT, dtype=torch.int32, device=dev)
    rc_ = raw(comm._h, buf.data_ptr() + lo, n, o[1:Q + 1])
    torch.cuda.synchronize()
    res.append(rc_ == 0 and bool((buf[:lo] == 0xA5).all()) and bool((buf[lo + n:] == 0xA5).all()) and same(o[1:Q + 1].cpu(), want)
               and bool((o[0] == SENT).all()) and bool((o[Q + 1] == SENT).all()))
ws = torch.empty(n, dtype=torch.uint8, device=dev)
o = torch.full((Q, C16 + 1, 3), SENT, dtype=torch.int32, device=dev)
refusals = {}
refusals["short"] = [raw(comm._h, ws.data_ptr(), least - 1, o), err()]
refusals["null_comm"] = [raw(None, ws.data_ptr(), n, o), err()]
refusals["null_comm_and_c65"] = [raw(None, ws.data_ptr(), n, o, c=65, cap=100), err()]
refusals["null_comm_and_rates"] = [raw(None, ws.data_ptr(), n, o, n_rates=9), err()]
refusals["null_comm_and_short"] = [raw(None, ws.data_ptr(), least - 1, o), err()]
refusals["null_out"] = [raw(comm._h, ws.data_ptr(), n, None), err()]
nogap = tc.DeviceCorpus(0)
nogap.upload(rows[:5])
refusals["null_comm_and_no_codes"] = [raw(None, ws.data_ptr(), n, o, handle=nogap._h), err()]
nogap.close()
torch.cuda.synchronize()
refusals["nothing_written"] = bool((o == SENT).all())
out["bounds"] = {"exact": res, "sizes": [n, least, tc.align_candidates_rates_workspace_bytes(Q, L, d_q.numel(), 3, CAP, C16)],
                 **refusals}

# ---- 4. the driver: Inspector._near over a plain DeviceCorpus and over a one-rank RankCorpus -------------------------
from tvidz_amd import inspector as insp, service  # noqa: E402

up = rc.uploads()
base = dict(device="cuda:0", near_duplicates=True, near_top_k=8, near_any_offset=True, near_candidates=16, near_gap_eps=EPS,
            near_rates=rc.RATES3, near_candidate_rates=True)
scenarios = {f"{name} {i}": (up[name], dict(base, **kw))
             for name in ("slow", "fast", "plain", "triple")
             for i, kw in enumerate((dict(near_score="local", near_min_votes=8, near_jaccard=0.9),
                                     dict(near_score="jaccard", near_jaccard=0.3)))}


def run(corpus):
    class Store:
        def get_video_by_id(self, vid):
            return None
    Store.corpus = corpus
    return {name: insp.Inspector(Store(), **kw)._near(424242, upload) for name, (upload, kw) in scenarios.items()}


out["near_plain"] = run(dc)
shard = tc.DeviceCorpus(0)
rk = service.RankCorpus(shard, sharded.RcclShardedMatcher(shard, comm, k=8, cap=64), xdev="cpu")
rk.upload(rows)
out["rank_supports"] = [rk.supports_align_candidates, rk.supports_align_candidate_rates]
out["near_rank"] = run(rk)
a = dc.align_candidates_rates(batch, rc.RATES8, c=16, min_count=1, exclude_ids=excl)
b = rk.align_candidates_rates(batch, rc.RATES8, c=16, min_count=1, exclude_ids=excl)
out["rank_equals_plain"] = all(same(x, y) for x, y in zip(a, b)) and len(b) == 4
ticks = rk.busy_ticks
refused = []
for call in (lambda: rk.align_candidates_rates([[1.0, 2.0]], (1.0,), c=0), lambda: rk.align_candidates_rates([[1.0, 2.0]], (1.0,), c=16, cap=15),
             lambda: rk.align_candidates_rates([[1.0, 2.0]], (1.0,), c=16, min_count=0),
             lambda: rk.align_candidates_rates([[1.0, 2.0]], (), c=16), lambda: rk.align_candidates_rates([[1.0, 2.0]], (1.0, -1.0), c=16)):
    try:
        call()
        refused.append("accepted")
    except ValueError:
        refused.append("ValueError")
ids, counts, rate_indexes, totals = rk.align_candidates_rates([[0.5] * 4096], (1.0, 0.96), c=4)
out["caller"] = {"refused": refused, "long_totals": totals.tolist(),
                 "long_rows_padding": bool((ids == -1).all() and (counts == 0).all() and (rate_indexes == 0).all()),
                 "ticks_unchanged": rk.busy_ticks == ticks}
out["rank_broken"] = repr(rk.broken) if rk.broken else None
rk.close()
dc.close()
comm.close()
print("RESULT " + json.dumps(out))
