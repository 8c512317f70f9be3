#!/usr/bin/env python3
"""The tolerant match that keeps the per-shard top-k inside the sweep (tvz_match_tol_topk) against what it replaces,
at config 3: 100k rows x ~200 cuts (synth_timestamp_corpus(100_000)), 64 queries of 200 timestamps (a corpus row
shifted by 0.3 ms), min_match 2, tol in {0.001, 0.1}, k in {16, 64}.  In ONE process, A and B alternating after a
warm-up, device events over REPS repetitions each:

  A  tvz_match_tol with a cap no list overflows (the largest hits_n is read first) + tvz_topk_shard;
  B  tvz_match_tol_topk.

B's blocks are compared with A's before anything is timed.  Bar: B's median is not above A's median by more than the
spread A shows between its own repetitions in this run (its interquartile range; min and max are printed too).
Also recorded, without a bar: the workspace bytes of both, and the host-to-host time of a RankCorpus tolerant ask
(RcclShardedMatcher at world size 1: tick, staging, tvz_match_tol_sharded, one device-to-host copy) at tol 0.1.

    python profiles/tol_topk.py [--q 16]        # JSON lines
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o t -- python profiles/tol_topk.py --trace
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tvidz_amd import corpus as tc, service, sharded, synth  # noqa: E402

TRACE = "--trace" in sys.argv
# --q N: another batch size.  At Q = 16 both forms sweep with 256 row blocks per query (A: q1_blocks, B: 6080 / 16 = 380
# capped by it), at Q = 64 A keeps 256 and B's workspace bound leaves it 95: the pair separates the kernel from its grid
Q_ARG = int(sys.argv[sys.argv.index("--q") + 1]) if "--q" in sys.argv else 64
REPS = 5 if TRACE else 24
comm = sharded.make_comm(0)                    # the communicator first: before this process's first GPU call
dev = torch.device("cuda:0")
Crows, Q, MM = 100_000, Q_ARG, 2
ids, offs, keys = synth.synth_timestamp_corpus(Crows)
dc = tc.DeviceCorpus(0)
dc.upload_csr(ids, offs, keys)
rng = np.random.default_rng(7)
picks = rng.choice(np.flatnonzero(np.diff(offs) >= 200), size=Q, replace=False)
queries = [(keys[offs[r]:offs[r] + 200] + 0.0003).tolist() for r in picks]
d_q, d_off, ml = tc.pack_queries(queries, dev)
st = torch.cuda.Stream(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    st.synchronize()
    return a.elapsed_time(b) * 1000.0


def quartiles(x):
    q = statistics.quantiles(x, n=4)
    return q[0], q[2]


for tol in (0.001, 0.1):
    # the largest hit list, read first: A's cap
    probe_n = torch.empty(Q, dtype=torch.int32, device=dev)
    dc.match_tol(d_q, d_off, ml, tol, MM, 1, out_n=probe_n, stream=st)
    st.synchronize()
    cap = int(probe_n.max().item())
    hits = torch.empty((Q, cap, 3), dtype=torch.int32, device=dev)
    hn = torch.empty(Q, dtype=torch.int32, device=dev)
    ws_a = torch.empty(tc.tol_workspace_bytes(Q, ml, d_q.numel()), dtype=torch.uint8, device=dev)
    for k in (16, 64):
        ws_b = torch.empty(tc.tol_topk_workspace_bytes(Q, ml, d_q.numel(), k), dtype=torch.uint8, device=dev)
        out_b = torch.empty((Q, k + 1, 3), dtype=torch.int32, device=dev)
        res = {}

        def run_a():
            dc.match_tol(d_q, d_off, ml, tol, MM, cap, out_hits=hits, out_n=hn, stream=st, workspace=ws_a)
            res["a"] = tc.topk_shard(hits, hn, k, stream=st)

        def run_b():
            res["b"] = dc.match_tol_topk(d_q, d_off, ml, tol, MM, k, out=out_b, stream=st, workspace=ws_b)

        run_a()
        run_b()
        st.synchronize()
        equal = bool(torch.equal(res["a"], res["b"]))
        if not equal:
            print(json.dumps({"tol": tol, "k": k, "blocks_equal": False}), flush=True)
            sys.exit(1)
        for _ in range(3):                                       # warm-up, alternating
            run_a()
            run_b()
        st.synchronize()
        ta, tb = [], []
        for _ in range(REPS):
            ta.append(timed(run_a))
            tb.append(timed(run_b))
        a25, a75 = quartiles(ta)
        med_a, med_b = statistics.median(ta), statistics.median(tb)
        print(json.dumps({
            "rows": Crows, "Q": Q, "query_len": 200, "min_match": MM, "tol": tol, "k": k, "reps": REPS,
            "blocks_equal": equal, "largest_hit_list": cap, "hits_total": int(hn.sum().item()),
            "A_match_tol_plus_topk_shard_us": {"median": round(med_a, 1), "min": round(min(ta), 1),
                                               "max": round(max(ta), 1), "iqr": round(a75 - a25, 1)},
            "B_match_tol_topk_us": {"median": round(med_b, 1), "min": round(min(tb), 1), "max": round(max(tb), 1)},
            "B_minus_A_us": round(med_b - med_a, 1), "B_over_A": round(med_b / med_a, 3),
            "bar_B_within_A_iqr": bool(med_b <= med_a + (a75 - a25)),
            "workspace_bytes_A": int(ws_a.numel() + hits.numel() * 4 + hn.numel() * 4 + Q * (k + 1) * 12),
            "workspace_bytes_A_at_cap_4096": int(ws_a.numel() + Q * 4096 * 12 + Q * 4 + Q * (k + 1) * 12),
            "workspace_bytes_B": int(ws_b.numel()),
        }), flush=True)

# host to host through the service's rank corpus (world size 1), the tolerant ask of one upload at a time
shard = tc.DeviceCorpus(0)
shard.upload_csr(ids, offs, keys)
rc = service.RankCorpus(shard, sharded.RcclShardedMatcher(shard, comm, k=64, cap=4096, priority=-1), xdev="cpu",
                        tick_s=0.0005)
try:
    for tol in (0.001, 0.1):
        for q in queries[:4]:
            rc.find_duplicates(q, MM, with_kth=True, tolerance=tol)
        before, ts = rc.exact_asks, []
        for i in range(8 if TRACE else 60):
            q = queries[i % 8]
            t0 = time.perf_counter()
            got = rc.find_duplicates(q, MM, with_kth=True, tolerance=tol)
            ts.append((time.perf_counter() - t0) * 1e6)
        print(json.dumps({"rank_corpus_tolerant_ask_host_to_host_us": {"median": round(statistics.median(ts), 1),
                                                                      "min": round(min(ts), 1), "max": round(max(ts), 1)},
                          "tol": tol, "k": 64, "rows_returned_last": len(got), "exact_rounds": rc.exact_asks - before,
                          "asks": len(ts)}), flush=True)
finally:
    rc.close()
    comm.close()
    dc.close()
