#!/usr/bin/env python3
"""How well the SEGMENTED counts of include/tvz_gap_long.h find a long stored video, without a GPU: numpy only, the
contract's own expressions (profiles/gap_candidates_recall.py's bins, codes and probes; a probe's segment is its
position // 511; count_long = the sum over the segments of the per-segment counts that reach min_count).

    python3 profiles/gap_candidates_long_recall.py [rows] > profiles/gap_candidates_long_recall.txt

A table of `rows` (default 20,000) stored videos of 1,200 to 1,600 cuts on a 30 fps grid; 20 uploads per line, each
derived from a stored row; min_count 2, gap_eps 1/30.  Reported: the true row's count under this contract against its
whole-query count (medians), the best other row, the share of uploads whose true row is strictly first, and the rows a
SEGMENT's list holds (count >= min_count: what `cap` = 4,096 has to take), median and maximum over all segments."""
import sys
import time

import numpy as np

MAX_BIN = (1 << 17) - 1
FPS = 30.0
SEG = 511
PER_LINE = 20
MIN_COUNT = 2
CAP = 4096
GAP_EPS = 1.0 / 30


def table(n_rows, skewed, rng):
    """-> cuts [n_rows, 1600], NaN behind a row's own length (1,200..1,600)"""
    n = 1600
    if skewed:
        short = rng.random((n_rows, n - 1)) < 0.75
        frames = np.where(short, rng.integers(6, 31, size=(n_rows, n - 1)), rng.integers(30, 241, size=(n_rows, n - 1)))
    else:
        frames = rng.integers(30, 241, size=(n_rows, n - 1))
    start = rng.integers(0, 3000, size=(n_rows, 1))
    cuts = np.concatenate([start, start + np.cumsum(frames, axis=1)], axis=1) / FPS
    lens = rng.integers(1200, 1601, size=n_rows)
    cuts[np.arange(n)[None, :] >= lens[:, None]] = np.nan
    return cuts, lens


def codes_of(bins):
    ok = (bins >= 0) & (bins <= MAX_BIN)                          # NaN fails
    b = np.where(ok, bins, 0).astype(np.int64)
    c = b[..., :-2] + (b[..., 1:-1] << 17) + (b[..., 2:] << 34)
    return np.where(ok[..., :-2] & ok[..., 1:-1] & ok[..., 2:], c, -1)


class Index:
    def __init__(self, cuts):
        n_rows = cuts.shape[0]
        code, row = [], []
        for lo in range(0, n_rows, 2000):                         # in slabs: the whole table's codes at once is too much
            part = cuts[lo:lo + 2000]
            with np.errstate(invalid="ignore"):
                c = codes_of(np.floor((part[:, 1:] - part[:, :-1]) / GAP_EPS + 0.5))
            rows = np.broadcast_to(np.arange(lo, lo + part.shape[0], dtype=np.int64)[:, None], c.shape)
            keep = c >= 0
            pair = np.unique(c[keep] * n_rows + rows[keep])        # a row holds a code once
            code.append(pair // n_rows)
            row.append(pair % n_rows)
        code, row = np.concatenate(code), np.concatenate(row)
        order = np.argsort(code, kind="stable")
        self.code, self.row, self.n_rows = code[order], row[order], n_rows

    def segment_counts(self, query):
        """-> int64 [S, n_rows]: c_s(q, r) of every row for one query (sorted cuts)"""
        a = np.floor((query[1:] - query[:-1]) / GAP_EPS)
        g = a.size - 2
        S = -(-g // SEG)
        out = np.zeros((S, self.n_rows), dtype=np.int64)
        seg_of = np.arange(g) // SEG
        for v in range(8):
            b0, b1, b2 = a[:g] + (v & 1), a[1:g + 1] + ((v >> 1) & 1), a[2:g + 2] + ((v >> 2) & 1)
            ok = (b0 >= 0) & (b0 <= MAX_BIN) & (b1 >= 0) & (b1 <= MAX_BIN) & (b2 >= 0) & (b2 <= MAX_BIN)
            p = b0[ok].astype(np.int64) + (b1[ok].astype(np.int64) << 17) + (b2[ok].astype(np.int64) << 34)
            s = seg_of[ok]
            lo, hi = np.searchsorted(self.code, p, "left"), np.searchsorted(self.code, p, "right")
            n = hi - lo
            at = np.repeat(lo, n) + (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n))
            np.add.at(out, (np.repeat(s, n), self.row[at]), 1)
        return out


def jitter(x, ms, rng):
    return x + rng.uniform(-ms / 1000.0, ms / 1000.0, size=x.shape) if ms else x


def uploads(rng):
    def inserted(s):
        cut = s.size // 2
        foreign = s[cut - 1] + 1.0 + np.cumsum(rng.uniform(2.0, 8.0, size=6))
        return np.concatenate([s[:cut], foreign, s[cut:] + 45.0])
    return [("shifted 1 h, jitter +-5 ms", lambda s: jitter(s + 3600.0, 5, rng)),
            ("re-timed to a 25 fps grid", lambda s: np.unique(np.round((s + 3600.0) * 25.0) / 25.0)),
            ("a 300-cut excerpt, jitter +-5 ms", lambda s: jitter(s[400:700] + 77.0, 5, rng)),
            ("45 s inserted in the middle, jitter +-5 ms", lambda s: jitter(inserted(s), 5, rng))]


def line(ix, cuts, lens, make, rng):
    longs, wholes, others, first, per_list = [], [], [], 0, []
    for r in rng.choice(cuts.shape[0], size=PER_LINE, replace=False):
        q = np.sort(make(cuts[r, :lens[r]]))
        seg = ix.segment_counts(q)
        per_list += (seg >= MIN_COUNT).sum(axis=1).tolist()
        whole = seg.sum(axis=0)
        long_ = np.where(seg >= MIN_COUNT, seg, 0).sum(axis=0)
        longs.append(int(long_[r]))
        wholes.append(int(whole[r]))
        long_[r] = 0
        others.append(int(long_.max()))
        first += longs[-1] > others[-1]
    return int(np.median(longs)), min(longs), int(np.median(wholes)), max(others), 100.0 * first / PER_LINE, \
        int(np.median(per_list)), max(per_list)


def main():
    n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    print(f"gap codes for long uploads: recall by simulation, numpy only; {n_rows} rows x 1,200-1,600 cuts on a {FPS:g} fps grid, "
          f"{PER_LINE} uploads per line, gap_eps {GAP_EPS:.4f}, min_count {MIN_COUNT}, segments of {SEG} positions")
    for skewed in (False, True):
        rng = np.random.default_rng(40 + skewed)
        t0 = time.time()
        cuts, lens = table(n_rows, skewed, rng)
        ix = Index(cuts)
        print()
        print("gaps " + ("SKEWED: 0.2-1 s for three in four, 1-8 s for the rest" if skewed else "uniform in 1-8 s"))
        print(f"{'upload is the stored video ...':46s} {'true row: long median (min)':>28s} {'whole median':>13s} {'best other, max':>16s} "
              f"{'ranked first':>13s} {'rows per segment list, median (max)':>36s}")
        for label, make in uploads(rng):
            med, lo, whole, other, pct, lm, lmax = line(ix, cuts, lens, make, rng)
            over = "  > cap: OVERFLOWS" if lmax > CAP else ""
            print(f"{label:46s} {med:>20d} ({lo:d}) {whole:>13d} {other:>16d} {pct:>12.0f}% {lm:>28d} ({lmax:d}){over}")
        print(f"  (index: {ix.code.size} (code, row) pairs, {np.unique(ix.code).size} distinct codes)  [{time.time() - t0:.0f} s]")


if __name__ == "__main__":
    main()
