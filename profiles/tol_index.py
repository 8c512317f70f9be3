#!/usr/bin/env python3
"""The tolerant top-k match through cell postings (tvz_corpus_tol_index) against the sweep it replaces, at config 3:
100k rows x ~200 cuts (synth_timestamp_corpus(100_000)), queries of 200 timestamps (a corpus row shifted by 0.3 ms),
min_match 2, k = 16.  In ONE process, on two handles with the same corpus, A and B alternating after a warm-up, device
events over REPS repetitions each:

  A  tvz_match_tol_topk on the handle WITHOUT cell postings: the sweep of every row (the path before this change);
  B  the same call on the handle with tvz_corpus_tol_index(cell = tol).

Q in {64, 4096}, tol in {0.001, 0.1}.  B's blocks are compared with A's before anything is timed.
Bar (tol 0.001, Q = 64): B's median is at most one third of A's.  Printed beside the times: hits per query (the
blocks' totals) and candidates per query - the rows pass A marks twice, recomputed on the host from the keys for a
sample of queries (nothing on the device counts them).  Also recorded: build_index() host to host with and without
cell postings, and the device memory the postings add.

    python profiles/tol_index.py                 # JSON lines
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o t -- python profiles/tol_index.py --trace
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tvidz_amd import corpus as tc, synth  # noqa: E402

TRACE = "--trace" in sys.argv
REPS = 4 if TRACE else 24
dev = torch.device("cuda:0")
Crows, MM, K = 100_000, 2, 16
ids, offs, keys = synth.synth_timestamp_corpus(Crows)
row_of_key = np.repeat(np.arange(Crows, dtype=np.int64), np.diff(offs))
st = torch.cuda.Stream(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    st.synchronize()
    return a.elapsed_time(b) * 1000.0


def summary(x):
    q = statistics.quantiles(x, n=4)
    return {"median": round(statistics.median(x), 1), "min": round(min(x), 1), "max": round(max(x), 1),
            "iqr": round(q[2] - q[0], 1)}


def cell_of(x, w):
    with np.errstate(over="ignore"):
        return np.clip(np.floor(np.asarray(x, dtype=np.float64) / w), -2.0 ** 40, 2.0 ** 40).astype(np.int64)


def host_candidates(queries, tol, w):
    """Rows marked at least twice by pass A (min_match 2), per query: every (element, cell of its probe range) marks the
    rows that own a key in the cell, once per (cell, row)."""
    ck = cell_of(keys, w)
    pair = np.unique(ck * (1 << 20) + row_of_key)            # (cell, row) once; rows < 2^20
    pc, pr = pair >> 20, pair & ((1 << 20) - 1)
    out = []
    for q in queries:
        q = np.asarray(q, dtype=np.float64)
        m = w * 2.0 ** -10
        lo, hi = cell_of((q - tol) - m, w), cell_of((q + tol) + m, w)
        marks = np.zeros(Crows, dtype=np.int32)
        for a, b in zip(lo, hi):
            s, e = np.searchsorted(pc, a, side="left"), np.searchsorted(pc, b, side="right")
            np.add.at(marks, pr[s:e], 1)
        out.append(int((marks >= 2).sum()))
    return out


plain = tc.DeviceCorpus(0)
plain.upload_csr(ids, offs, keys)
cells = tc.DeviceCorpus(0)
cells.upload_csr(ids, offs, keys)
torch.cuda.synchronize()


def build_ms(h, n=5):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        h.build_index()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


for tol in (0.001, 0.1):
    free0 = torch.cuda.mem_get_info(dev)[0]
    cells.set_tol_index(tol)                                  # cell = tol: builds the postings now
    torch.cuda.synchronize()
    added = free0 - torch.cuda.mem_get_info(dev)[0]
    stt = cells.tol_index_stats()
    print(json.dumps({"cell": tol, "cells_in_use": stt["cells"], "cell_postings": stt["postings"], "keys": int(len(keys)),
                      "device_bytes_added_by_the_first_build_with_postings": int(added),
                      "build_index_ms_without_postings": build_ms(plain), "build_index_ms_with_postings": build_ms(cells)}),
          flush=True)
    for Q in (64, 4096):
        rng = np.random.default_rng(7)
        long_rows = np.flatnonzero(np.diff(offs) >= 200)
        picks = rng.choice(long_rows, size=Q, replace=Q > len(long_rows))
        queries = [(keys[offs[r]:offs[r] + 200] + 0.0003).tolist() for r in picks]
        d_q, d_off, ml = tc.pack_queries(queries, dev)
        ws = torch.empty(tc.tol_topk_workspace_bytes(Q, ml, d_q.numel(), K), dtype=torch.uint8, device=dev)
        out_a = torch.empty((Q, K + 1, 3), dtype=torch.int32, device=dev)
        out_b = torch.empty((Q, K + 1, 3), dtype=torch.int32, device=dev)

        def run_a():
            plain.match_tol_topk(d_q, d_off, ml, tol, MM, K, out=out_a, stream=st, workspace=ws)

        def run_b():
            cells.match_tol_topk(d_q, d_off, ml, tol, MM, K, out=out_b, stream=st, workspace=ws)

        run_a()
        run_b()
        st.synchronize()
        equal = bool(torch.equal(out_a, out_b))
        if not equal:
            print(json.dumps({"tol": tol, "Q": Q, "blocks_equal": False}), flush=True)
            sys.exit(1)
        for _ in range(2):
            run_a()
            run_b()
        st.synchronize()
        ta, tb = [], []
        for _ in range(REPS):
            ta.append(timed(run_a))
            tb.append(timed(run_b))
        hits = out_b[:, K, 1].cpu().numpy()
        cand = host_candidates(queries[:8], tol, tol)
        sa, sb = summary(ta), summary(tb)
        rec = {"rows": Crows, "Q": Q, "query_len": 200, "min_match": MM, "k": K, "tol": tol, "cell": tol, "reps": REPS,
               "blocks_equal": equal, "A_sweep_us": sa, "B_cell_postings_us": sb,
               "B_over_A": round(sb["median"] / sa["median"], 3), "A_over_B": round(sa["median"] / sb["median"], 2),
               "hits_per_query": {"mean": round(float(hits.mean()), 1), "min": int(hits.min()), "max": int(hits.max())},
               "candidates_per_query_first_8": cand}
        if tol == 0.001 and Q == 64:
            rec["bar_B_at_most_a_third_of_A"] = bool(sb["median"] * 3.0 <= sa["median"])
        print(json.dumps(rec), flush=True)
plain.close()
cells.close()
