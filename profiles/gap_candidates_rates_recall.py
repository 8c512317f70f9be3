#!/usr/bin/env python3
"""How well the gap codes find a stored video from a copy played at another SPEED when the upload is probed once per rate
(include/tvz_gap_rates.h), without a GPU: numpy only, the contract's own expressions - x' = x * rho on the sorted upload
(one multiplication), then profiles/gap_candidates_recall.py's query side on x'; the stored codes stay at rate 1.

    python3 profiles/gap_candidates_rates_recall.py [rows] > profiles/gap_candidates_rates_recall.txt

The tables of profiles/gap_candidates_recall.py (`rows` stored videos of 200 cuts on a 30 fps grid; gaps uniform in 1-8 s,
or skewed: 0.2-1 s for three gaps in four).  An upload is x = (stored - shift) / rho with +-0.5 ms of jitter, for rho in
24/25, 25/24, 1000/1001 and 1.25; 40 uploads per line.  The rate list is (1, 24/25, 25/24, 1000/1001, 1001/1000, 1.25);
per upload and rate: the true row's count, the best other row's count, the rows touched.  "first": the true row's best
over the list is strictly above every other row's best over the list - what the call's per-id maximum ranks by."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gap_candidates_recall import CUTS, PER_LINE, Index, jitter, table  # noqa: E402

RATES = (("1", 1.0), ("24/25", 24 / 25), ("25/24", 25 / 24), ("1000/1001", 1000 / 1001), ("1001/1000", 1001 / 1000), ("1.25", 1.25))
SPEEDS = (("24/25", 24 / 25), ("25/24", 25 / 24), ("1000/1001", 1000 / 1001), ("1.25", 1.25))


def line(ix, cuts, rho, gap_eps, rng):
    """-> per rate of the list (median true count, max best other, median rows touched), and the share ranked first"""
    true = np.zeros((PER_LINE, len(RATES)), dtype=np.int64)
    other = np.zeros_like(true)
    touched = np.zeros_like(true)
    first = 0
    for u, r in enumerate(rng.choice(cuts.shape[0], size=PER_LINE, replace=False)):
        x = np.sort(jitter((cuts[r] - 1234.5) / rho, 0.5, rng))
        best_true, best_other = 0, np.zeros(cuts.shape[0], dtype=np.int64)
        for i, (_, rate) in enumerate(RATES):
            c = ix.counts(x * np.float64(rate), gap_eps)
            true[u, i] = c[r]
            c[r] = 0
            other[u, i], touched[u, i] = c.max(), int((c > 0).sum()) + 1
            best_true = max(best_true, int(true[u, i]))
            np.maximum(best_other, c, out=best_other)
        first += best_true > int(best_other.max())
    return np.median(true, axis=0).astype(int), true.min(axis=0), other.max(axis=0), np.median(touched, axis=0).astype(int), \
        100.0 * first / PER_LINE


def main():
    n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    print(f"gap codes at a list of rates: recall by simulation, numpy only; {n_rows} rows x {CUTS} cuts on a 30 fps grid, "
          f"{PER_LINE} uploads per line, jitter +-0.5 ms; {CUTS - 3} positions per upload")
    print("rate list: " + ", ".join(n for n, _ in RATES))
    for skewed in (False, True):
        rng = np.random.default_rng(40 + skewed)
        t0 = time.time()
        cuts = table(n_rows, skewed, rng)
        print()
        print("gaps " + ("SKEWED: 0.2-1 s for three in four, 1-8 s for the rest" if skewed else "uniform in 1-8 s"))
        for gap_eps in (1 / 30, 0.1):
            ix = Index(cuts, gap_eps)
            print(f"  gap_eps {gap_eps:.4f}; per probed rate: true row's count median (min) / best other row, max / rows touched, median")
            for name, rho in SPEEDS:
                med, lo, oth, tch, pct = line(ix, cuts, rho, gap_eps, rng)
                cells = "  ".join(f"{n}: {m}({l})/{o}/{t}" for (n, _), m, l, o, t in zip(RATES, med, lo, oth, tch))
                print(f"    upload at {name:>9s}: first {pct:3.0f}%   {cells}")
        print(f"  [{time.time() - t0:.0f} s]")


if __name__ == "__main__":
    main()
