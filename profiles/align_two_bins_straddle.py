#!/usr/bin/env python3
"""How many shifted copies the best SINGLE offset bin misses, and how many the best window of TWO ADJACENT bins does
(TVZ_ALIGN_TWO_BINS): a simulation with the contract's own vote expression, numpy only, nothing from the library.
   stored : 200 cuts on a 30 fps grid, gaps of 1 to 8 s
   upload : the same cuts at a random shift in +-300 s, jittered or re-timed to another frame grid, printed as %.6g
   vote   : floor((c - x) / eps + 0.5) over all pairs; v = min(votes, 200); Jaccard v / (400 - v); a miss is < 0.8
   python3 profiles/align_two_bins_straddle.py [--trials 600] [--eps-list 0.0333333,0.0666667,0.1]"""
import argparse

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--trials", type=int, default=600)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--eps-list", default="")
args = ap.parse_args()
N, JACCARD = 200, 0.8


def misses(rng, eps, jitter=0.0, grid=None, trials=args.trials):
    """-> (share of copies the best bin misses, share the best two adjacent bins miss)"""
    one = two = 0
    for _ in range(trials):
        c = np.round(np.cumsum(rng.uniform(1.0, 8.0, N)) * 30) / 30               # stored: a 30 fps grid
        x = c - rng.uniform(-300.0, 300.0)
        x = np.round(x * grid) / grid if grid else x + rng.uniform(-jitter, jitter, N)
        x = np.array([float("%.6g" % v) for v in x])
        bins, h = np.unique(np.floor((c[:, None] - x[None, :]) / eps + 0.5).astype(np.int64), return_counts=True)
        at = np.minimum(np.searchsorted(bins, bins + 1), bins.size - 1)
        j = h + np.where(bins[at] == bins + 1, h[at], 0)                           # J[b] = h[b] + h[b + 1]
        v1, v2 = min(int(h.max()), N), min(int(j.max()), N)
        one += v1 / (2 * N - v1) < JACCARD
        two += v2 / (2 * N - v2) < JACCARD
    return one / trials, two / trials


CASES = (("jittered +-0.5 ms (remux rounding)", dict(jitter=0.0005)), ("jittered +-5 ms", dict(jitter=0.005)),
         ("jittered +-10 ms", dict(jitter=0.010)), ("re-timed to a 25 fps grid", dict(grid=25.0)),
         ("re-timed to a 24 fps grid", dict(grid=24.0)), ("re-timed to 30000/1001 fps", dict(grid=30000 / 1001)))
rng = np.random.default_rng(args.seed)
print(f"eps = 1/30, Jaccard {JACCARD}, {args.trials} shifts per line: share of copies missed")
print(f"{'upload is the stored video, shifted, and ...':46s} {'best single bin':>16s} {'best two adjacent bins':>24s}")
for name, kw in CASES:
    a, b = misses(rng, 1 / 30, **kw)
    print(f"{name:46s} {100 * a:15.1f}% {100 * b:23.1f}%")
for eps in [float(e) for e in args.eps_list.split(",") if e]:
    a, b = misses(rng, eps, grid=25.0)
    print(f"{'re-timed to a 25 fps grid, eps = %g' % eps:46s} {100 * a:15.1f}% {100 * b:23.1f}%")
