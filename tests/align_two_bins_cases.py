"""The tables of the TVZ_ALIGN_TWO_BINS tests (tests/test_align_two_bins_cpu.py, tests/test_align_two_bins_gpu.py and
tests/near_two_bins_comm_child.py): plain data, no library call.  eps = 1/64 is dyadic, so a key written as x + d * eps
votes into bin d exactly; the jittered keys land wherever the reference says."""
import os
import re

import numpy as np

E64 = 1 / 64
KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tvidz_amd", "csrc",
                       "tvz_align_kernels.h")


def kernel_constant(name):
    """constexpr int <name> = <number>; of tvz_align_kernels.h"""
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(KERNELS).read()).group(1))


def window_width(B):
    """aw_width(B) of tvz_align_kernels.h, from its constants"""
    padded = (2 * B + 2) & ~1
    return padded if padded <= kernel_constant("kAwOneWindow") else kernel_constant("kAwWidth")


# ---- the main table: every kind of row, B = 900 (one window) ------------------------------------------------------------
MAIN_B = 900
MAIN_RATES = (1.0, 0.96)


def main_table():
    """-> (rows, queries, exclude_ids).  Query 0 is the base: 40 cuts with gaps of 1 to 8 s on the 1/64 grid."""
    rng = np.random.default_rng(8)
    x = 50.0 + np.cumsum(rng.integers(64, 8 * 64 + 1, size=40)) * E64
    at = lambda d: x + np.asarray(d) * E64                                          # noqa: E731  key i in bin d[i]
    split = lambda *parts: np.concatenate([np.full(n, d) for d, n in parts])        # noqa: E731
    rows = [
        x + 5 * E64,                                            # 1 an exact copy: all votes in bin 5
        at(split((10, 20), (11, 20))),                          # 2 split across two bins
        at(split((-1, 20), (0, 20))),                           # 3 ... across (-1, 0)
        at(split((20, 10), (21, 16), (22, 14))),                # 4 three bins: b + c beats a + b
        at(split((20, 14), (21, 16), (22, 10))),                # 5 ... a + b beats b + c
        at(split((20, 12), (21, 16), (22, 12))),                # 6 ... J ties: the bin with more votes of its own
        at(split((-12, 8), (-11, 8), (-10, 8), (200, 8), (300, 8))),           # 7 J and h tie: the smaller |b|, -11
        x + 1.0e6,                                              # 8 no vote
        [],                                                     # 9 empty
        np.concatenate([x + 40 * E64, x + 40.2 * E64, x + 41 * E64]),          # 10 near-duplicate keys: votes > nv
        np.concatenate([x[:20] + 7 * E64, x[:20] + 7 * E64, [np.nan, np.inf, -np.inf]]),   # 11 duplicates, NaN, infinities
        0.96 * x + 300 * E64 + rng.integers(0, 2, size=40) * E64,               # 12 a 0.96 copy split across two bins
        x[:1] + 3 * E64,                                        # 13 one key
        at(split((MAIN_B - 1, 20), (MAIN_B, 20))),              # 14 split across (B - 1, B)
        at(split((MAIN_B, 20), (MAIN_B + 1, 20))),              # 15 half beyond B: must not count
        at(split((-MAIN_B - 1, 25), (-MAIN_B, 15))),            # 16 half below -B
        at(split((-5, 8), (-4, 8), (5, 8), (6, 8), (300, 8))),  # 17 J, h and |b| tie: the negative one, -5
    ]
    for _ in range(24):                                         # jittered copies at any shift, some of them excerpts
        n = int(rng.integers(5, 41))
        i0 = int(rng.integers(0, 41 - n))
        rows.append(x[i0:i0 + n] + rng.uniform(-12.0, 12.0) + rng.uniform(-0.7, 0.7, size=n) * E64)
    for _ in range(8):                                          # unrelated rows, up to 200 keys
        rows.append(np.sort(rng.uniform(0.0, 400.0, size=int(rng.integers(1, 201)))))
    rows = [(100 + i, np.asarray(r, dtype=np.float64).tolist()) for i, r in enumerate(rows)]
    queries = [x.tolist(),
               x.tolist() + [float("nan"), float("inf"), -float("inf")],
               x.tolist() + x[:10].tolist(),                    # duplicate values vote again
               (x[::2] - 3.0).tolist(),
               [],
               [float("nan"), float("nan")],
               (x[5:30] / 0.96).tolist()]
    return rows, queries, [101, -1, -1, 100, -1, -1, -1]


# ---- the range's edges --------------------------------------------------------------------------------------------------
def edge_table(B):
    """-> (rows, query): three query values 1,000 s (64,000 bins) apart, so only key i and value i meet inside B < 32,000"""
    q = np.array([1000.0, 2000.0, 3000.0])
    rows = [q + B * E64, q - B * E64, q + np.array([B - 1, B, B]) * E64, q + np.array([B, B + 1, B + 1]) * E64,
            q[:2] - np.array([B, B + 1]) * E64, q - (B + 1) * E64, q + np.array([B - 1, B - 1, B]) * E64,
            q + np.array([-B, -B + 1, B]) * E64]
    return [(i + 1, r.tolist()) for i, r in enumerate(rows)], q.tolist()


# ---- the seams of the window walk -----------------------------------------------------------------------------------------
def seam_B():
    """B = 3 windows' bins: beyond one window, and the seams of the grid w * width - B fall on multiples of the width,
    (-1, 0) among them"""
    W = kernel_constant("kAwWidth")
    B = 3 * W
    assert window_width(B) == W and B > 2047
    return B, W


def seam_table():
    """-> (rows, queries, B).  Query 0: eight values 1,000 s apart (no cross votes inside B * eps = 48 s), so a row's
    range covers every window; query 1: one value, so a row's range is exactly its keys' and windows go unvisited."""
    B, W = seam_B()
    rng = np.random.default_rng(15)
    q = 1000.0 * np.arange(1, 9)
    lone = 50000.0
    rows = []

    def keys(per_value, peaks, n_random):
        """per query value: `peaks` = [(bin, n)] keys inside the bin at distinct places, and n_random keys anywhere"""
        out = []
        for x in q[:per_value]:
            for b, n in peaks:
                out += [x + (b + f) * E64 for f in rng.permutation(np.arange(-24, 25))[:n] / 64.0]
            out += (x + (rng.integers(-B, B + 1, size=n_random) + 0.25) * E64).tolist()
        return out

    for S in (-W, 0, W, 2 * W):
        rows.append(keys(8, [(S - 1, 4), (S, 4), (S + 300, 6)], 2))            # a pair across the seam beats a lone bin
        rows.append(keys(8, [(S - 1, 3), (S, 5), (S + 1, 4)], 0))              # three bins at the seam: (S, S + 1) wins
        rows.append(keys(8, [(S - 2, 4), (S - 1, 5), (S, 3)], 0))              # ... (S - 2, S - 1) wins, below the seam
        rows.append(keys(8, [(S, 5)], 0))                                      # the window's lowest bin alone
        # the one-valued query: the row's range ends at the seam, the neighbouring window is never visited
        rows.append([lone + (S + f) * E64 for f in (-0.3, 0.0, 0.3)] + [lone + (S + 5) * E64, lone + (S + 5.2) * E64])
        rows.append([lone + (S - 1 + f) * E64 for f in (-0.3, 0.0, 0.3)] + [lone + (S - 3) * E64])
        rows.append([lone + (S - 1 + f) * E64 for f in (-0.2, 0.2)] + [lone + (S + f) * E64 for f in (-0.2, 0.2)])
    # three windows, the best pair on a seam; and the best pair inside a window with a smaller one on the seam
    rows.append(keys(8, [(W + 500, 3), (W - 1, 3), (W, 3), (-500, 4), (200, 2)], 0))
    rows.append(keys(8, [(W + 500, 3), (W + 501, 4), (W - 1, 3), (W, 3), (-500, 5)], 0))
    rows.append(keys(8, [(-W - 1, 3), (-W, 3), (W - 1, 3), (W, 3)], 0))        # two seams tie: the smaller |b|, W - 1
    rows.append(keys(8, [(-W, 3), (-W + 1, 3), (W - 1, 3), (W, 3)], 0))        # ... |b| = W - 1 against W: W - 1
    # 64 keys exactly, 72, and more than the resume positions cover
    rows.append(keys(8, [(W - 1, 3), (W, 3)], 2))
    rows.append(keys(8, [(W - 1, 3), (W, 4)], 2))
    assert len(rows[-2]) == 64 and len(rows[-1]) == 72
    resume = kernel_constant("kAwResume")
    rows.append(keys(8, [(-1, 20), (0, 20)], 48))
    rows.append(keys(8, [(2 * W - 1, 10), (2 * W, 30), (-W - 1, 25), (-W, 14)], 9))
    assert min(len(rows[-1]), len(rows[-2])) > resume + 64
    rows = [(i + 1, r) for i, r in enumerate(rows)]
    return rows, [q.tolist(), [lone]], B


# ---- rates ----------------------------------------------------------------------------------------------------------------
def rates_table():
    """-> (rows, query): row 1's best window at the rate 0.96 (25 votes over two bins) beats its best single bin at 1.0
    (15); row 2 has 10 votes in one bin at 1.0 and 10 over two bins at 0.96; row 3 is row 1 without the 1.0 part."""
    rng = np.random.default_rng(21)
    x = 20.0 + np.cumsum(rng.integers(64, 8 * 64 + 1, size=40)) * E64
    y = 0.96 * x
    r1 = np.concatenate([x[:15] + 5 * E64, y[15:27] + 7.1 * E64, y[27:] + 8.1 * E64])
    r2 = np.concatenate([x[:10] + 5 * E64, y[10:15] + 7.1 * E64, y[15:20] + 8.1 * E64])
    r3 = r1[15:]
    return [(1, r1.tolist()), (2, r2.tolist()), (3, r3.tolist())], x.tolist()
