#!/usr/bin/env python3
"""The merge of the shards' blocks at any shift (tvz_align_wide_topk_merge) next to the bounded merge
(tvz_align_topk_merge): one launch each at Q = 64, k = 16, 8 lists, on the SAME blocks - full lists of random hits with
bins inside +-2,047, sorted by the contract's order, so both merges take them and must return the same rows - and the
wide merge once more on blocks whose bins span +-2^22 and with the containment score.  Device events: a single launch,
and 200 launches back to back divided by 200 (a launch of a few microseconds is below what one pair of events
resolves); the two merges alternate.
   python3 profiles/align_wide_sharded.py [--reps 20]     -> one JSON line"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tvidz_amd import corpus as tc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--burst", type=int, default=200)
args = ap.parse_args()
Q, K, R, NQ = 64, 16, 8, 200
dev = torch.device("cuda:0")
rng = np.random.default_rng(5)
queries = [np.sort(rng.uniform(0.0, 3600.0, NQ)).tolist() for _ in range(Q)]
d_q, d_off, _ = tc.pack_queries(queries, dev)


def make_blocks(max_bin, contain):
    blocks = np.zeros((R, Q, K + 1, 4), dtype=np.int32)
    blocks[:, :, :, 0] = -1
    for r in range(R):
        for q in range(Q):
            hits = [(int(rng.integers(0, 1 << 20)), int(rng.integers(150, 260)), int(rng.integers(-max_bin, max_bin + 1)),
                     int(rng.integers(100, 200))) for _ in range(K)]
            hits.sort(key=lambda h: tc.align_wide_order_key(h, NQ, contain))
            blocks[r, q, :K] = hits
            blocks[r, q, K, 1] = 1000
    return torch.from_numpy(blocks).to(dev)


def med(xs):
    q1, m, q3 = np.percentile(np.asarray(xs), [25, 50, 75])
    return {"median_us": round(float(m) * 1e3, 3), "iqr_us": round(float(q3 - q1) * 1e3, 3)}


def timed(call, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


narrow, wide, wide_c = make_blocks(2047, False), make_blocks(tc.ALIGN_WIDE_MAX_B, False), make_blocks(tc.ALIGN_WIDE_MAX_B, True)
out = tc._topk_out(None, Q, K, 4, dev)
legs = {"bounded_merge": lambda: tc.align_topk_merge(narrow, K, d_q, d_off, out=out),
        "wide_merge_same_blocks": lambda: tc.align_wide_topk_merge(narrow, K, d_q, d_off, out=out),
        "wide_merge_bins_2p22": lambda: tc.align_wide_topk_merge(wide, K, d_q, d_off, out=out),
        "wide_merge_bins_2p22_containment": lambda: tc.align_wide_topk_merge(wide_c, K, d_q, d_off, contain=True, out=out)}
b_rows, b_totals = (t.clone() for t in legs["bounded_merge"]())
w_rows, w_totals = (t.clone() for t in legs["wide_merge_same_blocks"]())
torch.cuda.synchronize()
assert torch.equal(b_rows, w_rows) and torch.equal(b_totals, w_totals) and int(b_rows[0, 0, 0]) >= 0
for call in legs.values():                                          # every shape warm
    timed(call, 20)
single = {n: [] for n in legs}
burst = {n: [] for n in legs}
for _ in range(args.reps):                                          # alternating
    for n, call in legs.items():
        single[n].append(timed(call, 1))
        burst[n].append(timed(call, args.burst))
res = {"Q": Q, "k": K, "n_lists": R, "query_len": NQ, "bytes_read": R * Q * (K + 1) * 16 + Q * NQ * 8, "reps": args.reps,
       "burst": args.burst, "same_rows_as_bounded": True}
for n in legs:
    res[n] = {"single_launch": med(single[n]), "per_launch_in_burst": med(burst[n])}
print("RESULT " + json.dumps(res))
