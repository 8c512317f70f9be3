"""Child process of tests/test_tol_topk_gpu.py: creates the libtvz RCCL communicator BEFORE its first GPU call (a
fresh python: a process that has touched the GPU is never exec'ed over), runs the tolerant sharded match through
the C ABI at world size 1 (tvz_match_tol_sharded) and prints what it got as JSON."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (import only: no GPU call yet)

from tests.test_tol_gpu import _grid_corpus  # noqa: E402
from tvidz_amd import corpus as tc, sharded  # noqa: E402

uid = tc.Comm.unique_id()                      # ncclGetUniqueId: no GPU involved
comm = tc.Comm(uid, 1, 0, 0)                   # ncclCommInitRank: the first GPU call of this process
K, MM = 16, 2
rng = np.random.default_rng(77)
rows = _grid_corpus(rng, 1500, 90000)
picks = [int(v) for v in rng.integers(0, len(rows), 10)]
queries = [(np.asarray(rows[v][1]) + 0.0004 * (t % 3)).tolist() for t, v in enumerate(picks)]
queries_b = [(np.asarray(rows[(v + 7) % len(rows)][1]) - 0.0003).tolist() for v in picks]
excl_ids = [rows[v][0] if t % 2 else -1 for t, v in enumerate(picks)]
dev = torch.device("cuda:0")
dc = tc.DeviceCorpus(0)
dc.upload(rows)
d_q, d_off, max_len = tc.pack_queries(queries, dev)
d_qb, d_offb, max_len_b = tc.pack_queries(queries_b, dev)
excl = torch.tensor(excl_ids, dtype=torch.int32, device=dev)
out = {"picks": picks, "excl": excl_ids, "sharded": {}, "local": {}}
answers = {}
for tol in (0.001, 0.1):
    merged, totals = comm.match_tol_sharded(dc, d_q, d_off, max_len, tol, MM, K, d_exclude_ids=excl)
    torch.cuda.synchronize()
    out["sharded"][str(tol)] = {"merged": merged.cpu().tolist(), "totals": totals.cpu().tolist()}
    # the same from its parts: the local block through tvz_topk_merge
    block = dc.match_tol_topk(d_q, d_off, max_len, tol, MM, K, d_exclude_ids=excl)
    m2, t2 = tc.topk_merge(block.unsqueeze(0).contiguous(), K)
    torch.cuda.synchronize()
    out["local"][str(tol)] = bool(torch.equal(m2, merged) and torch.equal(t2, totals))
    answers[("a", tol)] = (merged.clone(), totals.clone())
    mb, tb = comm.match_tol_sharded(dc, d_qb, d_offb, max_len_b, tol, MM, K, d_exclude_ids=excl)
    torch.cuda.synchronize()
    answers[("b", tol)] = (mb.clone(), tb.clone())
for name, (q_, off_, ml_) in (("a", (d_q, d_off, max_len)), ("b", (d_qb, d_offb, max_len_b))):
    me, te = comm.match_sharded(dc, q_, off_, ml_, MM, len(rows), K, d_exclude_ids=excl)
    torch.cuda.synchronize()
    answers[(name, 0.0)] = (me.clone(), te.clone())
out["batches_differ"] = not torch.equal(answers[("a", 0.001)][0], answers[("b", 0.001)][0])
# the matcher: tolerant batches of two tolerances interleaved with tolerance-0 batches over its rotating slots;
# every ticket must carry ITS batch's answer
sm = sharded.RcclShardedMatcher(dc, comm, k=K, cap=len(rows))
batches = {"a": (d_q, d_off, max_len), "b": (d_qb, d_offb, max_len_b)}
plan = [("a", 0.001), ("b", 0.0), ("a", 0.1), ("b", 0.001), ("a", 0.0), ("b", 0.1), ("a", 0.001), ("a", 0.0), ("b", 0.1)]
ok = sm.supports_tolerance
for name, tol in plan:                                           # one at a time
    m, t = sm.match_topk(*batches[name], MM, excl, tolerance=tol)
    torch.cuda.synchronize()
    ok = ok and torch.equal(m, answers[(name, tol)][0]) and torch.equal(t, answers[(name, tol)][1])
out["matcher_equal"] = bool(ok)
ok, ticket, want = True, None, None
for name, tol in plan:                                           # streaming: one batch in flight behind the other
    nxt = sm.submit(*batches[name], MM, excl, inputs_ready=True, tolerance=tol)
    if ticket is not None:
        m, t = sm.finish(ticket, host=True)
        ok = ok and torch.equal(m, answers[want][0]) and torch.equal(t, answers[want][1])
    ticket, want = nxt, (name, tol)
m, t = sm.finish(ticket, host=True)
ok = ok and torch.equal(m, answers[want][0]) and torch.equal(t, answers[want][1])
out["streaming_equal"] = bool(ok)
comm.close()
dc.close()
print("RESULT " + json.dumps(out))
