#!/usr/bin/env python3
"""Near-duplicate search, one upload against 100k rows: the parent's path A (tvz_align + the device-to-host copy of its
[C, 5] rows) against B (tvz_align_topk, k = 16, + the copy of its block), at the inspector's defaults (eps 1/30,
max_offset 30 s), the query a stored row shifted by a few frames.  One process, one GPU.  Before timing, B's rows are
checked against what A's output implies.  A and B alternate; a host clock runs around work that ends in a
synchronise, device events around the kernels alone.  Also: B at Q = 64 per query, and the host side of
Inspector._near for both near_top_k settings.
   python3 profiles/align_topk.py [--reps 24] [--kernels-only]
   rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python3 profiles/align_topk.py --kernels-only
   python3 profiles/align_topk.py --summarize DIR                    (kernel times per launch shape, a run of its own)"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tvidz_amd import _lib, corpus as tc, inspector, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=24)
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--kernels-only", action="store_true", help="a few calls of each path and nothing else (for a kernel trace)")
ap.add_argument("--summarize", metavar="DIR", help="no GPU work: per kernel and grid, the durations in DIR's *kernel_trace.csv")
args = ap.parse_args()

if args.summarize:
    import csv
    import glob
    import re
    rows = {}
    for f in glob.glob(os.path.join(args.summarize, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"ts_\w+", r["Kernel_Name"])
            name = m.group(0) if m else ""
            if "align" in name or "tol_sort" in name:
                if "Grid_Size_X" in r:                      # work-items per dimension -> blocks x queries
                    key = (name, int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1), int(r["Grid_Size_Y"]))
                else:
                    key = (name, int(r["Grid_Size"]) // max(int(r["Workgroup_Size"]), 1), 0)
                rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, bx, by), us in sorted(rows.items()):
        print(f"{name:<50} blocks {bx:>5} x {by:<3} launches {len(us):>2}  us: median {np.median(us):9.1f}  min {min(us):9.1f}  max {max(us):9.1f}")
    sys.exit(0)

dev = torch.device("cuda:0")
EPS, MAX_OFFSET, K, NQ = 1.0 / 30, 30.0, 16, 200
ids, offs, keys = synth.synth_timestamp_corpus(args.rows, seed=synth.CORPUS_SEED)
dc = tc.DeviceCorpus(0)
dc.upload_csr(ids, offs, keys)
lib = _lib.load()
rng = np.random.default_rng(synth.CORPUS_SEED + 7)


def shifted_query(r, frames):
    row = keys[offs[r]:offs[r + 1]][:NQ]
    return (row + frames / 30.0).tolist()


src = rng.permutation(np.flatnonzero(np.diff(offs) >= NQ))[:64].tolist()      # rows with at least NQ cuts
queries = [shifted_query(r, 3 + i % 5) for i, r in enumerate(src)]
stream = torch.cuda.current_stream(dev)
n_rows = C.c_int64(0)
out_a = torch.empty((args.rows, 5), dtype=torch.int32, device=dev)
host_a = torch.empty((args.rows, 5), dtype=torch.int32).pin_memory()


def prep(qs):
    d_q, d_off, longest = tc.pack_queries(qs, dev)
    ws = torch.empty(tc.align_topk_workspace_bytes(len(qs), longest, d_q.numel(), K), dtype=torch.uint8, device=dev)
    out = torch.empty((len(qs), K + 1, 4), dtype=torch.int32, device=dev)
    return d_q, d_off, longest, ws, out, torch.empty((len(qs), K + 1, 4), dtype=torch.int32).pin_memory()


def enqueue_a(d_q):
    _lib.check(lib.tvz_align(dc._h, d_q.data_ptr(), d_q.numel(), EPS, MAX_OFFSET, out_a.data_ptr(), args.rows,
                             C.byref(n_rows), stream.cuda_stream))


def enqueue_b(p):
    d_q, d_off, longest, ws, out, _ = p
    _lib.check(lib.tvz_align_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), d_off.numel() - 1, longest, EPS, MAX_OFFSET,
                                  1, 0, None, K, out.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream))


def timed(enqueue, copy):
    """-> (host seconds around enqueue + copy + synchronise, device milliseconds around the kernels alone)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    enqueue()
    b.record()
    copy()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, a.elapsed_time(b)


def stats(xs):
    q1, med, q3 = np.percentile(np.asarray(xs), [25, 50, 75])
    return {"median": round(float(med), 4), "iqr": round(float(q3 - q1), 4)}


p1, p64 = prep(queries[:1]), prep(queries)
if args.kernels_only:
    for _ in range(4):
        enqueue_a(p1[0])
        enqueue_b(p1)
    enqueue_b(p64)
    torch.cuda.synchronize()
    print(json.dumps({"kernels_only": True, "calls": {"tvz_align": 4, "tvz_align_topk Q=1": 4, "tvz_align_topk Q=64": 1}}))
    sys.exit(0)

# ---- B's rows equal what A's output implies (every query of the batch, vectorised restatement of the contract)
enqueue_b(p64)
got = p64[4].cpu().numpy().astype(np.int64)
for i, q in enumerate(queries):
    A = dc.align(q, eps=EPS, max_offset=MAX_OFFSET).astype(np.int64)
    v = np.minimum(np.minimum(A[:, 3], NQ), A[:, 1])
    hit = v >= 1
    s = np.zeros(len(A), dtype=np.int64)
    s[hit] = (v[hit] << 20) // (NQ + A[hit, 1] - v[hit])
    idx = np.flatnonzero(hit)
    order = idx[np.lexsort((A[idx, 3], A[idx, 1], A[idx, 2], A[idx, 0], -s[idx]))][:K]
    exp = np.zeros((K + 1, 4), dtype=np.int64)
    exp[:, 0] = -1
    exp[:len(order)] = A[order][:, [0, 1, 2, 3]]
    exp[K, 1] = len(idx)
    assert (got[i] == exp).all(), (i, got[i].tolist(), exp.tolist())
    assert ids[src[i]] in got[i, :K, 0] and got[i, 0, 2] == -(3 + i % 5) and got[i, 0, 3] >= NQ   # the shifted source is found
print(f"checked: tvz_align_topk's {len(queries)} blocks equal what tvz_align's rows imply "
      f"({int(got[:, K, 1].min())}..{int(got[:, K, 1].max())} hits per query of {args.rows} rows)")

# ---- Q = 1: A and B alternating
for _ in range(3):                                             # warm-up
    timed(lambda: enqueue_a(p1[0]), lambda: host_a.copy_(out_a, non_blocking=True))
    timed(lambda: enqueue_b(p1), lambda: p1[5].copy_(p1[4], non_blocking=True))
ha, da, hb, db = [], [], [], []
for _ in range(args.reps):
    h, d = timed(lambda: enqueue_a(p1[0]), lambda: host_a.copy_(out_a, non_blocking=True))
    ha.append(h * 1e3)
    da.append(d)
    h, d = timed(lambda: enqueue_b(p1), lambda: p1[5].copy_(p1[4], non_blocking=True))
    hb.append(h * 1e3)
    db.append(d)
res = {"rows": args.rows, "query_len": NQ, "eps": EPS, "max_offset": MAX_OFFSET, "k": K, "reps": args.reps,
       "A_tvz_align_ms": {"host": stats(ha), "device": stats(da), "d2h_bytes": args.rows * 20},
       "B_tvz_align_topk_ms": {"host": stats(hb), "device": stats(db), "d2h_bytes": (K + 1) * 16}}
bar = res["A_tvz_align_ms"]["host"]["median"] + res["A_tvz_align_ms"]["host"]["iqr"]
res["bar_B_median_le_A_median_plus_A_iqr"] = bool(res["B_tvz_align_topk_ms"]["host"]["median"] <= bar)

# ---- B at Q = 64, per query
timed(lambda: enqueue_b(p64), lambda: p64[5].copy_(p64[4], non_blocking=True))
h64, d64 = [], []
for _ in range(max(6, args.reps // 4)):
    h, d = timed(lambda: enqueue_b(p64), lambda: p64[5].copy_(p64[4], non_blocking=True))
    h64.append(h * 1e3 / 64)
    d64.append(d / 64)
res["B_Q64_ms_per_query"] = {"host": stats(h64), "device": stats(d64)}

# ---- the host side of Inspector._near, both settings (the whole call: device work, copy and the Python filter)
store = types.SimpleNamespace(corpus=dc, get_video_by_id=lambda v: None)
near = {}
for name, top_k in (("near_top_k=None", None), ("near_top_k=16", K)):
    ins = inspector.Inspector(store, device="cuda:0", near_duplicates=True, near_top_k=top_k, max_workers=1)
    ins._near(-1, queries[0])
    ts = []
    for _ in range(max(6, args.reps // 4)):
        t0 = time.perf_counter()
        rep = ins._near(-1, queries[0])
        ts.append((time.perf_counter() - t0) * 1e3)
    near[name] = dict(stats(ts), reported=len(rep))
    ins.close()
res["inspector_near_ms"] = near
print(json.dumps(res, indent=1))
dc.close()
