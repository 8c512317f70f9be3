#!/usr/bin/env python3
"""The opt-in tolerant match at config 3: 100k rows x ~200 cuts (synth_timestamp_corpus(100_000)), queries of 200
timestamps (a corpus row shifted by 0.3 ms - a remux), tol in {0.001, 0.1}, min_match 2.  In ONE process:

  * tvz_find_duplicates_tol host to host (median of 300 calls, ctypes, preallocated outputs);
  * tvz_match_tol, one query on a stream (event-timed: the query-sort kernel + the sweep);
  * tvz_match(..., TVZ_ALGO_Q1) on the same queries: the exact sweep that streams the same bytes;
  * tvz_match_tol at Q = 64.

Algorithmic bytes of one sweep = 16 B per row entry + 8 B per arena key (each read once per query); the share of
8 TB/s is bytes / time.  Kernel times come from a run of its own under the kernel trace:

    python profiles/tol_sweep.py                 # timings (JSON lines)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o t -- python profiles/tol_sweep.py --trace
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tvidz_amd import _lib, corpus as tc, synth  # noqa: E402

TRACE = "--trace" in sys.argv
dev = torch.device("cuda:0")
Crows = 100_000
ids, offs, keys = synth.synth_timestamp_corpus(Crows)
dc = tc.DeviceCorpus(0)
dc.upload_csr(ids, offs, keys)
lib = _lib.load()
rng = np.random.default_rng(7)
picks = rng.choice(np.flatnonzero(np.diff(offs) >= 200), size=64, replace=False)
queries = [(keys[offs[r]:offs[r] + 200] + 0.0003).tolist() for r in picks]
bytes_swept = 16 * Crows + 8 * int(offs[-1])
st = torch.cuda.Stream(dev)


def ev_time(fn, reps):
    """per-call GPU time on `st` (event pairs), median over reps, after 5 warm-up calls"""
    for _ in range(5):
        fn()
    st.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        st.synchronize()
        out.append(a.elapsed_time(b) * 1000.0)
    return statistics.median(out)


def host_to_host(q, tol, reps):
    qa = np.ascontiguousarray(np.asarray(q, dtype=np.float64))
    cap = Crows
    o_ids, o_cnt, o_kth = (np.empty(cap, dtype=np.int32) for _ in range(3))
    n = C.c_int64()
    args = (dc._h, C.c_void_p(qa.ctypes.data), qa.size, float(tol), 2, -1, cap, C.c_void_p(o_ids.ctypes.data),
            C.c_void_p(o_cnt.ctypes.data), C.c_void_p(o_kth.ctypes.data), C.byref(n))
    for _ in range(10):
        _lib.check(lib.tvz_find_duplicates_tol(*args))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        lib.tvz_find_duplicates_tol(*args)
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts), int(n.value)


reps = 20 if TRACE else 300
for tol in (0.001, 0.1):
    h2h = [host_to_host(q, tol, reps // 4 if i else reps) for i, q in enumerate(queries[:4])]
    one = queries[0]
    d_q, d_off, ml = tc.pack_queries([one], dev)
    hits = torch.empty((1, Crows, 3), dtype=torch.int32, device=dev)
    hn = torch.empty(1, dtype=torch.int32, device=dev)
    ws_t = torch.empty(tc.tol_workspace_bytes(1, ml, d_q.numel()), dtype=torch.uint8, device=dev)
    ws_q = torch.empty(max(tc.workspace_bytes(1, ml), 256), dtype=torch.uint8, device=dev)
    t_tol1 = ev_time(lambda: dc.match_tol(d_q, d_off, ml, tol, 2, Crows, out_hits=hits, out_n=hn, stream=st,
                                          workspace=ws_t), reps // 4)
    n_tol1 = int(hn.cpu()[0])
    t_q1 = ev_time(lambda: dc.match(d_q, d_off, ml, 2, Crows, out_hits=hits, out_n=hn, stream=st, workspace=ws_q,
                                    algo=_lib.ALGO_Q1), reps // 4)
    n_q1 = int(hn.cpu()[0])
    d_q64, d_off64, ml64 = tc.pack_queries(queries, dev)
    hits64 = torch.empty((64, 4096, 3), dtype=torch.int32, device=dev)
    hn64 = torch.empty(64, dtype=torch.int32, device=dev)
    ws64 = torch.empty(tc.tol_workspace_bytes(64, ml64, d_q64.numel()), dtype=torch.uint8, device=dev)
    t_tol64 = ev_time(lambda: dc.match_tol(d_q64, d_off64, ml64, tol, 2, 4096, out_hits=hits64, out_n=hn64,
                                           stream=st, workspace=ws64), max(3, reps // 20))
    print(json.dumps({
        "rows": Crows, "keys": int(offs[-1]), "query_len": 200, "tol": tol, "min_match": 2,
        "find_duplicates_tol_host_to_host_us_median": round(h2h[0][0], 1),
        "find_duplicates_tol_host_to_host_us_other_queries": [round(x[0], 1) for x in h2h[1:]],
        "hits_per_query": [x[1] for x in h2h],
        "match_tol_Q1_event_us": round(t_tol1, 1), "match_tol_Q1_hits": n_tol1,
        "exact_q1_sweep_event_us": round(t_q1, 1), "exact_q1_hits": n_q1,
        "tol_over_exact_q1": round(t_tol1 / t_q1, 2),
        "algorithmic_bytes": bytes_swept,
        "match_tol_Q1_share_of_8TBps": round(bytes_swept / (t_tol1 * 1e-6) / 8e12, 3),
        "match_tol_Q64_event_us": round(t_tol64, 1),
        "match_tol_Q64_us_per_query": round(t_tol64 / 64, 2),
        "match_tol_Q64_share_of_8TBps": round(64 * bytes_swept / (t_tol64 * 1e-6) / 8e12, 3),
    }), flush=True)
dc.close()
