"""Child process of tests/test_comm_gpu.py: creates the libtvz RCCL communicator BEFORE its first
GPU call (a process that has touched the GPU must not be re-exec'd, so this is a fresh python),
runs the sharded match through the C ABI at world size 1 and prints the merged result as JSON."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (import only: no GPU call yet)

from tvidz_amd import corpus as tc, sharded, synth  # noqa: E402

uid = tc.Comm.unique_id()                      # ncclGetUniqueId: no GPU involved
comm = tc.Comm(uid, 1, 0, 0)                   # ncclCommInitRank: the first GPU call of this process
C, Q, k, mm = 3000, 12, 16, 2
ids, offs, keys = synth.synth_timestamp_corpus(C, seed=31, mean_len=60, dup_frac=0.03)
queries = synth.synth_queries(ids, offs, keys, Q, seed=4, mean_len=60)
dev = torch.device("cuda:0")
dc = tc.DeviceCorpus(0)
dc.upload_csr(ids, offs, keys)
d_q, d_off, max_len = tc.pack_queries(queries, dev)
excl = torch.tensor([int(ids[(5 * i) % C]) for i in range(Q)], dtype=torch.int32, device=dev)
merged, totals = comm.match_sharded(dc, d_q, d_off, max_len, mm, 64, k, d_exclude_ids=excl)
torch.cuda.synchronize()
out = {"merged": merged.cpu().tolist(), "totals": totals.cpu().tolist()}
# the pipelined form: three batches in flight over two streams, each equal to the plain call
sm = sharded.RcclShardedMatcher(dc, comm, k=k, cap=64)
tickets = [sm.submit(d_q, d_off, max_len, mm, excl) for _ in range(3)]
same = True
for t in tickets:
    m2, t2 = sm.finish(t)
    torch.cuda.synchronize()
    same = same and torch.equal(m2, merged) and torch.equal(t2, totals)
out["pipelined_equal"] = bool(same)
# the streaming form (bench.py): no wait on the caller's stream, results read after a host-side wait;
# two different batches alternate, every ticket must carry ITS batch's answer
queries_b = synth.synth_queries(ids, offs, keys, Q, seed=9, mean_len=60)
d_qb, d_offb, max_len_b = tc.pack_queries(queries_b, dev)
merged_b, totals_b = comm.match_sharded(dc, d_qb, d_offb, max_len_b, mm, 64, k, d_exclude_ids=excl)
torch.cuda.synchronize()
batches = [(d_q, d_off, max_len, merged, totals), (d_qb, d_offb, max_len_b, merged_b, totals_b)]
stream_ok = not torch.equal(merged, merged_b)
ticket, want = None, None
for i in range(7):
    b = batches[i % 2]
    nxt = sm.submit(b[0], b[1], b[2], mm, excl, inputs_ready=True)
    if ticket is not None:
        m4, t4 = sm.finish(ticket, host=True)
        stream_ok = stream_ok and torch.equal(m4, want[3]) and torch.equal(t4, want[4])
    ticket, want = nxt, b
m4, t4 = sm.finish(ticket, host=True)
stream_ok = stream_ok and torch.equal(m4, want[3]) and torch.equal(t4, want[4])
out["streaming_equal"] = bool(stream_ok)
# a truncated shard list is signalled through the all-gather by a negative total
m3, t3 = comm.match_sharded(dc, d_q, d_off, max_len, 0, 50, 8)
torch.cuda.synchronize()
out["overflow_totals"] = t3.cpu().tolist()
# RcclShardedMatcher's slots and plans: a fixed sequence of calls over two side streams, every answer equal to the
# one-shot call's for the same inputs (an 8-row shard, Q = 3, then Q = 2)
rows8 = [(100 + i, [50.0 * i + 1.5 * j for j in range(6)]) for i in range(8)]
dc8 = tc.DeviceCorpus(0)
dc8.upload(rows8)
qa = [rows8[0][1], [t + 0.3 for t in rows8[1][1]], rows8[2][1][:3] + rows8[3][1][:3]]     # the second: only tolerantly
a_q, a_off, a_len = tc.pack_queries(qa, dev)
b_q, b_off, b_len = tc.pack_queries([rows8[4][1], rows8[5][1]], dev)
a_ex = torch.tensor([-1, -1, rows8[3][0]], dtype=torch.int32, device=dev)
k8, near8 = 4, dict(eps=0.1, max_offset=3.0, k=3)


def _host(pair):
    torch.cuda.synchronize()
    return [t.cpu().tolist() for t in pair]


want_a = _host(comm.match_sharded(dc8, a_q, a_off, a_len, 2, 8, k8, d_exclude_ids=a_ex))
want_b = _host(comm.match_sharded(dc8, b_q, b_off, b_len, 2, 8, k8))
want_tol = _host(comm.match_tol_sharded(dc8, a_q, a_off, a_len, 0.5, 2, k8, d_exclude_ids=a_ex))
want_near = _host(comm.align_topk_sharded(dc8, a_q, a_off, a_len, d_exclude_ids=a_ex, **near8))
sm8 = sharded.RcclShardedMatcher(dc8, comm, k=k8, cap=8, n_streams=2)
steps = [("a", want_a, lambda: sm8.match_topk(a_q, a_off, a_len, 2, a_ex))] * 3          # the third: a plan hit
steps += [("b", want_b, lambda: sm8.match_topk(b_q, b_off, b_len, 2)),                   # Q = 2: outputs re-made, plans dropped
          ("a tolerant", want_tol, lambda: sm8.match_topk(a_q, a_off, a_len, 2, a_ex, tolerance=0.5)),
          ("near", want_near, lambda: sm8.align_topk(a_q, a_off, a_len, d_exclude_ids=a_ex, **near8)),
          ("a again", want_a, lambda: sm8.match_topk(a_q, a_off, a_len, 2, a_ex))]
out["slot_sequence"] = [[name, _host(step()) == want] for name, want, step in steps]
out["slot_premises"] = {"exact_finds_0_and_2": [want_a[1][0] >= 1, want_a[1][1], want_a[1][2] >= 1],
                        "tolerant_finds_1": want_tol[1][1] >= 1, "near_finds_1": want_near[1][1] >= 1,
                        "b_differs": want_b != want_a, "plans": len(sm8._plans)}
# corpus.py's one prelude through the three wrappers that need a communicator (tests/prelude_cases.py says what)
from tests import prelude_cases as pc  # noqa: E402
four = tc.DeviceCorpus(0)
four.upload(pc.ROWS)
out["prelude_failures"] = {name: pc.failures(name, *spec) for name, spec in pc.wrappers([four], comm).items()}
four.close()
dc8.close()
comm.close()
dc.close()
print("RESULT " + json.dumps(out))
