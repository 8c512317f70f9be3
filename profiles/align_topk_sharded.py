#!/usr/bin/env python3
"""Near-duplicate search over a SHARDED table: service.ShardedCorpus.align_topk host to host, on the workload of
profiles/align_topk.py (100k rows, the inspector's defaults: eps 1/30, max_offset 30 s, min_score = floor(0.8 x 2^20),
k = 16, queries of 200 cuts that are stored rows shifted by a few frames) split over 8 shards on one GPU.
   python3 profiles/align_topk_sharded.py [--tree DIR] [--reps 20]     one run: medians for Q = 1 and Q = 64 as JSON
   python3 profiles/align_topk_sharded.py --merge                      the merge launch alone next to the whole call
`--tree DIR` imports tvidz_amd from DIR (a built checkout of another commit) instead of this one: the comparison of two
commits is made by alternating runs of this script, a fresh process each, and taking the median of each side's runs."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--shards", type=int, default=8)
ap.add_argument("--merge", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
from tvidz_amd import corpus as tc, service, synth  # noqa: E402

EPS, MAX_OFFSET, K, NQ = 1.0 / 30, 30.0, 16, 200
MIN_SCORE = int(0.8 * (1 << 20))
dev = torch.device("cuda:0")
ids, offs, keys = synth.synth_timestamp_corpus(args.rows, seed=synth.CORPUS_SEED)
rng = np.random.default_rng(synth.CORPUS_SEED + 7)
src = rng.permutation(np.flatnonzero(np.diff(offs) >= NQ))[:64].tolist()
queries = [(keys[offs[r]:offs[r + 1]][:NQ] + (3 + i % 5) / 30.0).tolist() for i, r in enumerate(src)]
sc = service.ShardedCorpus(0, n_shards=args.shards, k=K)
for r, s in enumerate(sc.shards):                       # video_id mod R, as ShardedCorpus.upload places them
    sel = np.flatnonzero(ids % args.shards == r)
    lens = (offs[sel + 1] - offs[sel]).astype(np.int64)
    o = np.zeros(len(sel) + 1, dtype=np.int64)
    np.cumsum(lens, out=o[1:])
    s.upload_csr(ids[sel], o, np.concatenate([keys[offs[i]:offs[i + 1]] for i in sel]))


def med(xs):
    q1, m, q3 = np.percentile(np.asarray(xs), [25, 50, 75])
    return {"median": round(float(m), 4), "iqr": round(float(q3 - q1), 4)}


def host_ms(qs, **kw):
    for _ in range(3):
        sc.align_topk(qs, eps=EPS, max_offset=MAX_OFFSET, k=K, **kw)
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows, totals = sc.align_topk(qs, eps=EPS, max_offset=MAX_OFFSET, k=K, **kw)
        ts.append((time.perf_counter() - t0) * 1e3)
    return med(ts), rows, totals


if not args.merge:
    res = {"tree": os.path.abspath(args.tree), "rows": args.rows, "shards": args.shards, "k": K, "reps": args.reps}
    for name, qs in (("Q1", queries[:1]), ("Q64", queries)):
        res[name + "_ms"], rows, totals = host_ms(qs, min_score=MIN_SCORE)
        res[name + "_min_score_0_ms"], _, _ = host_ms(qs)
        assert int(rows[0, 0, 0]) == int(ids[src[0]]) and int(totals[0]) >= 1          # the shifted source is found
        res[name + "_checksum"] = int(np.asarray(rows, dtype=np.int64).sum() + np.asarray(totals, dtype=np.int64).sum())
    print("RESULT " + json.dumps(res))
    sc.close()
    sys.exit(0)

# ---- the merge launch alone (n_lists = 8, Q = 64) next to the whole tvz_align_topk_shards call, device events
res = {"rows": args.rows, "shards": args.shards, "Q": 64}
d_q, d_off, longest = tc.pack_queries(queries, dev)
for k in (16, 64):
    ws = torch.empty(tc.align_topk_workspace_bytes(64, longest, d_q.numel(), k), dtype=torch.uint8, device=dev)
    call = lambda: tc.align_topk_shards(sc.shards, d_q, d_off, longest, eps=EPS, max_offset=MAX_OFFSET, k=k, workspace=ws)  # noqa: E731
    blocks, rows, totals = call()
    whole, merge = [], []
    for _ in range(args.reps):
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        torch.cuda.synchronize()
        a.record()
        call()
        b.record()
        r2, t2 = tc.align_topk_merge(blocks, k, d_q, d_off)
        c.record()
        torch.cuda.synchronize()
        whole.append(a.elapsed_time(b))
        merge.append(b.elapsed_time(c))
    assert torch.equal(r2, rows) and torch.equal(t2, totals)
    res[f"k{k}"] = {"shards_call_device_ms": med(whole), "merge_alone_device_ms": med(merge),
                    "merge_share": round(float(np.median(merge) / np.median(whole)), 5)}
print("RESULT " + json.dumps(res))
sc.close()
