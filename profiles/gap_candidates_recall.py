#!/usr/bin/env python3
"""How well the gap codes of include/tvz_gap.h find a stored video, without a GPU: numpy only, the contract's own
expressions (d = s[i+1] - s[i], r = d / gap_eps, stored bins floor(r + 0.5), query bins floor(r) and floor(r) + 1, codes
of three consecutive bins, counts with the probes' multiplicity over each row's code SET).

    python3 profiles/gap_candidates_recall.py [rows] > profiles/gap_candidates_recall.txt

A table of `rows` (default 100,000) stored videos of 200 cuts on a 30 fps grid; 40 uploads per line, each derived from a
stored row; the true row is ranked by its count among all rows (ties broken against it: "first" means strictly more
than every other row).  Two gap distributions: uniform in 1-8 s (kind to the method: every gap is tens of bins wide and
triples are nearly unique) and a skewed one with many short gaps (0.2-1 s for three gaps in four), where triples repeat
across videos."""
import sys
import time

import numpy as np

MAX_BIN = (1 << 17) - 1
FPS = 30.0
CUTS = 200
PER_LINE = 40


def table(n_rows, skewed, rng):
    if skewed:
        short = rng.random((n_rows, CUTS - 1)) < 0.75
        frames = np.where(short, rng.integers(6, 31, size=(n_rows, CUTS - 1)), rng.integers(30, 241, size=(n_rows, CUTS - 1)))
    else:
        frames = rng.integers(30, 241, size=(n_rows, CUTS - 1))
    start = rng.integers(0, 3000, size=(n_rows, 1))
    return np.concatenate([start, start + np.cumsum(frames, axis=1)], axis=1) / FPS


def codes_of(bins):
    """[..., g] bins -> [..., g - 2] codes, -1 where a bin is invalid"""
    ok = (bins >= 0) & (bins <= MAX_BIN)
    b = np.where(ok, bins, 0).astype(np.int64)
    c = b[..., :-2] + (b[..., 1:-1] << 17) + (b[..., 2:] << 34)
    return np.where(ok[..., :-2] & ok[..., 1:-1] & ok[..., 2:], c, -1)


class Index:
    """the rows' code sets as one sorted list of (code, row) pairs"""

    def __init__(self, cuts, gap_eps):
        r = (cuts[:, 1:] - cuts[:, :-1]) / gap_eps
        c = codes_of(np.floor(r + 0.5))
        n_rows = cuts.shape[0]
        rows = np.broadcast_to(np.arange(n_rows, dtype=np.int64)[:, None], c.shape)
        keep = c >= 0
        pair = np.unique(c[keep] * n_rows + rows[keep])                # a row holds a code once
        self.code, self.row, self.n_rows = pair // n_rows, pair % n_rows, n_rows

    def counts(self, query, gap_eps):
        """count(q, r) of every row for one query (sorted cuts)"""
        a = np.floor((query[1:] - query[:-1]) / gap_eps)
        probes = []
        g = a.size - 2
        for v in range(8):
            b0 = a[:g] + (v & 1)
            b1 = a[1:g + 1] + ((v >> 1) & 1)
            b2 = a[2:g + 2] + ((v >> 2) & 1)
            ok = (b0 >= 0) & (b0 <= MAX_BIN) & (b1 >= 0) & (b1 <= MAX_BIN) & (b2 >= 0) & (b2 <= MAX_BIN)
            probes.append((b0[ok].astype(np.int64) + (b1[ok].astype(np.int64) << 17) + (b2[ok].astype(np.int64) << 34)))
        p = np.concatenate(probes)
        lo, hi = np.searchsorted(self.code, p, "left"), np.searchsorted(self.code, p, "right")
        n = hi - lo
        at = np.repeat(lo, n) + (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n))
        return np.bincount(self.row[at], minlength=self.n_rows)


def jitter(x, ms, rng):
    return x + rng.uniform(-ms / 1000.0, ms / 1000.0, size=x.shape) if ms else x


def uploads(cuts, rng):
    """-> list of (label, function(row cuts) -> upload cuts)"""
    def retime(fps):
        return lambda s: np.unique(np.round((s + 3600.0) * fps) / fps)
    foreign = lambda t0: t0 + np.cumsum(rng.uniform(2.0, 8.0, size=8))                     # noqa: E731

    def inserted(s):
        cut = CUTS // 2
        return np.concatenate([s[:cut], foreign(s[cut - 1] + 1.0)[:6], s[cut:] + 45.0])
    return [("shifted 1 h, jitter +-0.5 ms", lambda s: jitter(s + 3600.0, 0.5, rng)),
            ("shifted 1 h, jitter +-5 ms", lambda s: jitter(s + 3600.0, 5, rng)),
            ("shifted 1 h, jitter +-10 ms", lambda s: jitter(s + 3600.0, 10, rng)),
            ("re-timed to a 25 fps grid", retime(25.0)),
            ("re-timed to a 24 fps grid", retime(24.0)),
            ("a 20-cut excerpt, jitter +-5 ms", lambda s: jitter(s[90:110] + 77.0, 5, rng)),
            ("45 s inserted in the middle, jitter +-5 ms", lambda s: jitter(inserted(s), 5, rng))]


def line(ix, cuts, make, gap_eps, rng):
    true_counts, others, first, touched = [], [], 0, []
    for r in rng.choice(cuts.shape[0], size=PER_LINE, replace=False):
        q = np.sort(make(cuts[r]))
        c = ix.counts(q, gap_eps)
        t = int(c[r])
        c[r] = 0
        true_counts.append(t)
        others.append(int(c.max()))
        touched.append(int((c > 0).sum()) + 1)
        first += t > others[-1]
    return (int(np.median(true_counts)), min(true_counts), max(others), 100.0 * first / PER_LINE, int(np.median(touched)))


def main():
    n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    print(f"gap codes: recall by simulation, numpy only; {n_rows} rows x {CUTS} cuts on a {FPS:g} fps grid, {PER_LINE} uploads per line")
    for skewed in (False, True):
        rng = np.random.default_rng(20 + skewed)
        t0 = time.time()
        cuts = table(n_rows, skewed, rng)
        print()
        print("gaps " + ("SKEWED: 0.2-1 s for three in four, 1-8 s for the rest" if skewed else "uniform in 1-8 s"))
        print(f"{'upload is the stored video ...':46s} {'gap_eps':>8s} {'true row count median (min)':>28s} {'best other, max':>16s} "
              f"{'ranked first':>13s} {'rows touched':>13s}")
        for gap_eps in (1 / 30, 0.1):
            ix = Index(cuts, gap_eps)
            for label, make in uploads(cuts, rng):
                med, lo, other, pct, touched = line(ix, cuts, make, gap_eps, rng)
                print(f"{label:46s} {gap_eps:8.4f} {med:>20d} ({lo:d}) {other:>16d} {pct:>12.0f}% {touched:>13d}")
            print(f"  (index at gap_eps {gap_eps:.4f}: {ix.code.size} (code, row) pairs, {np.unique(ix.code).size} distinct codes)")
        print(f"  [{time.time() - t0:.0f} s]")


if __name__ == "__main__":
    main()
