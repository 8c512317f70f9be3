"""The table and the uploads of the tvz_align_parts_flags tests (tests/test_align_parts_two_bins_cpu.py asserts their
premises with the reference, tests/test_align_parts_two_bins_gpu.py runs them on the device).  Plain data, no code under
test.  The film, its grid (eps = 1/30 s: a film-to-film pair's (c - x) / eps is a whole number) and the rows of 65, 513
and 700 keys are tests/align_parts_cases.py's.

A copy whose shift lies a third of a bin above a whole bin, with every cut moved by up to 0.4 of a bin either way,
votes into two bins: (b + 1/3 +- 0.4) + 0.5 lies in (b + 0.43, b + 1.24).  `jittered` makes such an upload.

The film re-timed to a 25 fps grid: every cut rounded to the nearest 1/25 s, so stored - upload is the shift +- 0.02 s =
+- 0.6 of a bin, over two bins or three.  Two parts of at least 61 votes need 122 cuts, and a part whose best single bin
stays below 61 has at most about 100: so the stored video of that case is the film and its first 80 cuts again, 4,200 s
later (REELS, 200 cuts), and the upload is cut in two behind the 100th."""
import numpy as np

from tests import align_parts_cases as pc
from tests.align_two_bins_cases import kernel_constant, window_width

EPS = pc.EPS
NAN, INF = float("nan"), float("inf")
MAX_B = 1 << 22
THIRD = 1 / 3
FILM, LANES65, LANES513, LONG700, NINE_ROWS, SPECIAL, ABSENT = \
    pc.FILM, pc.LANES65, pc.LANES513, pc.LONG700, pc.NINE_ROWS, pc.SPECIAL, pc.ABSENT
REELS, LANES64, FLAG_BETTER, EQUAL_J, TIE0, TIE_LATER, RATE_CARRY, ONLY_B = 20, 21, 22, 23, 24, 25, 26, 27
SEAM0 = 40                                           # ids SEAM0 .. : the seam rows, in seam_rows()'s order
REEL_GAP = 4200.0
RETIME_SHIFT, RETIME_MOVE, RETIME_CUT = 123.451, 47.3, 100


def jittered(cuts, seed, third=THIRD, jitter=0.4):
    """the upload `cuts` as a copy whose shift is `third` of a bin above a whole bin: stored - upload grows by third
    -+ jitter bins"""
    rng = np.random.default_rng(seed)
    c = np.asarray(cuts, dtype=np.float64)
    return (c - (third + rng.uniform(-jitter, jitter, size=c.size)) * EPS).tolist()


def reels():
    f = np.asarray(pc.film())
    return np.concatenate([f, f[:80] + REEL_GAP]).tolist()


def retimed(cuts, to_fps=25):
    """the cuts on a `to_fps` grid, printed as a detector prints them"""
    return [float("%.9g" % x) for x in np.round(np.asarray(cuts) * to_fps) / float(to_fps)]


def seam_B():
    W = kernel_constant("kAwWidth")
    B = 3 * W
    assert window_width(B) == W and B > 2047
    return B, W


def uploads():
    """-> dict name -> the upload's cuts: the first five are tests/align_parts_cases.py's, jittered"""
    u = pc.uploads()
    r = np.asarray(reels())
    out = {"copy": jittered(u["exact"], 1), "removed": jittered(u["removed"], 2), "two_inserted": jittered(u["two_inserted"], 3),
           "swapped": jittered(u["swapped"], 4), "stranger": jittered(u["unrelated"], 5)}
    # the reels re-timed to the 25 fps grid, the second hundred later by RETIME_MOVE, foreign cuts between them
    n = RETIME_CUT
    out["retimed_inserted"] = retimed((r[:n] - RETIME_SHIFT).tolist() + (np.asarray(pc.foreign(9, r[n - 1] + 1.0, 6)) - RETIME_SHIFT).tolist()
                                      + (r[n:] - RETIME_SHIFT + RETIME_MOVE).tolist())
    # the 24 -> 25 fps copy (0.96) of the film with an insertion, on the 25 fps grid
    out["fps_inserted"] = retimed(u["fps_inserted"])
    out["special"] = [-0.0, 0.0, 5.0, 9.0, 9.0, NAN, INF, -INF, 200.0, 200.0, 207.0, 214.0, 214.0, 0.0, NAN]
    return out


def base30():
    """30 cuts with irregular gaps (the film's first 30): cross votes of two different cuts scatter"""
    return np.asarray(pc.film()[:30])


def at(x, parts, seed=0, spread=0.3):
    """keys for the values x: `parts` = [(bin, n)] takes the next n values of x into `bin`, up to `spread` of a bin off
    its middle"""
    rng = np.random.default_rng(1000 + seed)
    out, i = [], 0
    for b, n in parts:
        out += (np.asarray(x[i:i + n]) + (b + rng.uniform(-spread, spread, size=n)) * EPS).tolist()
        i += n
    return sorted(out)


SEAM_Q = (1000.0 * np.arange(1, 9)).tolist()         # 1,000 s apart: no cross votes inside 3 windows' bins
LONE_Q = [1000.0]


def seam_keys(values, peaks, seed):
    """per query value: `peaks` = [(bin, n)] keys inside the bin at distinct places"""
    rng = np.random.default_rng(2000 + seed)
    out = []
    for x in values:
        for b, n in peaks:
            out += [x + (b + f) * EPS for f in rng.permutation(np.arange(-24, 25))[:n] / 80.0]
    return sorted(out)


def seam_rows():
    """-> [(id, keys)] for B = 3 windows' bins, whose seams are the multiples of the width; SEAM_Q is their query.
    Rows 0..3: part 0's best pair of bins lies across the seam S.  Rows 4..5: part 0 takes the first four values (40
    votes in bins 40 / 41), and part 1's best pair lies across the seam among the last four values - while the first
    four values hold 8 more votes of the upper bin S, which part 0's ranges exclude: the count the walk carries over
    the seam must be the 16 allowed ones, not 24."""
    B, W = seam_B()
    rows = []
    for i, S in enumerate((-W, 0, W, 2 * W)):
        rows.append(seam_keys(SEAM_Q, [(S - 1, 4), (S, 4), (S + 300, 6)], i))
    for i, S in enumerate((-W, W)):
        rows.append(sorted(seam_keys(SEAM_Q[:4], [(40, 6), (41, 4)], 10 + i) + seam_keys(SEAM_Q[1:3], [(S, 4)], 20 + i)
                           + seam_keys(SEAM_Q[4:], [(S - 1, 3), (S, 4)], 30 + i)))
    return [(SEAM0 + i, r) for i, r in enumerate(rows)]


def table():
    """-> the rows, in table order (51 rows, at most 700 keys)"""
    B, W = seam_B()
    rng = np.random.default_rng(78)
    rows = [(1000 + i, np.sort(rng.uniform(0.0, 7200.0, size=int(n))).tolist()) for i, n in enumerate(rng.integers(5, 70, size=8))]
    rows.insert(5, (FILM, pc.film()))
    rows.append((REELS, reels()))
    rows.append((LANES64, pc.two_part_row(2, 36, 2)))
    rows.append((LANES65, pc.two_part_row(3, 36, 2)))
    rows.append((LANES513, pc.two_part_row(69, 36, 384)))
    rows.append((LONG700, pc.two_part_row(530, 100, 46)))
    x = base30()
    # two rows of one id: the first has 10 votes in one bin, the second 8 + 8 over two - better only under the flag
    rows.append((FLAG_BETTER, at(x, [(30, 10)], 1)))
    rows.append((FLAG_BETTER, at(x, [(30, 8), (31, 8)], 2)))
    # ... and two whose windows are equal: the earlier row (11 keys, not 12)
    rows.insert(2, (EQUAL_J, at(x, [(-7, 5), (-6, 4), (500, 2)], 3)))
    rows.append((EQUAL_J, at(x, [(9, 4), (10, 5), (600, 3)], 4)))
    # the tie chain in part 0: J ties between (20, 21) and (21, 22): the more votes of its own, bin 21; and between
    # (-11, -10) and (11, 12) with equal h: the smaller |b| is equal too - the negative one
    rows.append((TIE0, at(x, [(20, 4), (21, 6), (22, 4)], 5)))
    rows.append((TIE0 + 100, at(x, [(-11, 4), (-10, 4), (11, 4), (12, 4)], 6)))
    # ... and in a later part: part 0 takes the first 12 values, then (-5, -4) and (5, 6) tie in J, h and |b|
    rows.append((TIE_LATER, at(x, [(0, 7), (1, 5), (-5, 4), (-4, 4), (5, 4), (6, 4)], 7)))
    rows.append((TIE_LATER + 100, at(x, [(0, 7), (1, 5), (50, 3), (51, 5), (52, 3), (-80, 3), (-79, 3)], 8)))
    for i in range(9):
        rows.insert(4 * i + 1, (NINE_ROWS, at(pc.x24()[i:i + 4], [(i, 4)], 9)))
    rows.append((SPECIAL, sorted(at([0.0, 5.0, 9.0], [(40, 2), (41, 1)], 10) + at([200.0, 207.0, 214.0], [(-15, 1), (-14, 2)], 11)
                                 + [INF, -INF, 100.0])))
    # LONE_Q at the rates (1.0, 1.04): at 1.0 three keys vote into the lowest bin of a window (-W: the walk's last
    # window leaves 3 in its slot 0) and six lie beyond B; at 1.04 every bin is 1,200 lower, and the six vote into
    # the HIGHEST bin of the first window visited (2W - 1): a carry left over from the rate before would make it 9
    rows.append((RATE_CARRY, sorted([1000.0 + (-W + f) * EPS for f in (-0.3, 0.0, 0.3)]
                                    + [1000.0 + (2 * W - 1 + 1200 + f) * EPS for f in (-0.3, -0.2, -0.1, 0.1, 0.2, 0.3)])))
    # votes only in bin B (of the seam call): the window (B, B + 1) counts bin B alone
    rows.append((ONLY_B, seam_keys(SEAM_Q, [(B, 3), (B + 1, 4)], 40)))
    rows += seam_rows()
    return rows


NAMED = (FILM, REELS, LANES64, LANES65, LANES513, LONG700, FLAG_BETTER, EQUAL_J, TIE0, TIE0 + 100, TIE_LATER, TIE_LATER + 100,
         NINE_ROWS, SPECIAL, ABSENT, -1)
SEAM_IDS = tuple(range(SEAM0, SEAM0 + 6)) + (ONLY_B, RATE_CARRY)


def row_queries():
    """-> dict name -> upload for the named rows: the 24 cuts of the long rows and the 30 of the tie rows, jittered or not"""
    return {"parts24": jittered(pc.x24(), 11, jitter=0.3), "base30": base30().tolist(), "base30_jittered": jittered(base30(), 12, 0.0, 0.15)}
