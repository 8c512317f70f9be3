"""The table and the uploads of the tvz_align_parts tests (tests/test_align_parts_cpu.py asserts their premises with the
reference and with fractions, tests/test_align_parts_gpu.py runs them on the device).  Plain data, no code under test.

The film: 120 cuts on the 1/30 s grid (frame numbers, so every film-to-film pair's (c - x) / eps is an integer up to
rounding noise and + 0.5 puts it in the middle of its bin), a second apart at least.  Shifts are whole bins too: 47.3 s
= 1,419 bins, so the moved half votes into bin -1419.  Foreign cuts lie 0.4 of a bin off the grid."""
import numpy as np

EPS = 1 / 30
NAN, INF = float("nan"), float("inf")
FILM, LANES65, LANES513, LONG700, LATER_TIE, SECOND_BETTER, EQUAL_ROWS, NINE_ROWS, SPECIAL, ABSENT = \
    1, 2, 3, 4, 5, 6, 7, 8, 9, 999999
IDS = (FILM, LANES65, LANES513, LONG700, LATER_TIE, SECOND_BETTER, EQUAL_ROWS, NINE_ROWS, SPECIAL, ABSENT, -1)
MOVE = 47.3                                          # 1,419 bins
BIN_A, BIN_B = -100, 400                             # the two parts of the long rows: their keys do not interleave


def film():
    rng = np.random.default_rng(2024)
    frames = np.cumsum(rng.integers(30, 900, size=120)) + 3000
    return (frames / 30.0).tolist()


def foreign(n, after, seed):
    """n cuts of another video behind `after`, 0.4 of a bin off the film's grid"""
    rng = np.random.default_rng(seed)
    return ((after * 30 + np.cumsum(rng.integers(20, 120, size=n))) / 30.0 + 0.4 * EPS).tolist()


def uploads():
    """-> dict name -> the upload's cuts, as a detector would report them (ascending unless said otherwise)"""
    f = np.asarray(film())
    u = {}
    u["inserted"] = f[:60].tolist() + foreign(9, f[59] + 1.0, 1) + (f[60:] + MOVE).tolist()
    u["removed"] = f[:40].tolist() + (f[70:] - (f[70] - f[40])).tolist()
    u["two_inserted"] = (f[:40].tolist() + foreign(5, f[39] + 1.0, 2) + (f[40:80] + 20.0).tolist()
                         + foreign(6, f[79] + 21.0, 3) + (f[80:] + MOVE).tolist())
    u["swapped"] = (f[70:110] - f[70] + 10.0).tolist() + (f[10:50] - f[10] + 2000.0).tolist()
    u["exact"] = f.tolist()
    u["unrelated"] = foreign(80, 500.0, 4)
    u["fps_inserted"] = ((f[:60] - 12.0) / 0.96).tolist() + ((np.asarray(foreign(9, f[59] + 1.0, 5)) - 12.0) / 0.96).tolist() \
        + ((f[60:] + MOVE - 12.0) / 0.96).tolist()
    u["parts24"] = x24()
    u["tie30"] = x30()
    u["special"] = [-0.0, 0.0, 5.0, 9.0, 9.0, NAN, INF, -INF, 200.0, 200.0, 207.0, 214.0, 214.0, 0.0, NAN]
    return u


def x24():
    return [3000.0 + 7.0 * i for i in range(24)]


def x30():
    return [8000.0 + 11.0 * i for i in range(30)]


def _shifted(x, b):
    """the cuts x moved into bin b, a tenth of a bin inside it"""
    return (np.asarray(x) + (b + 0.1) * EPS).tolist()


def two_part_row(n_below, n_inside, n_above):
    """x24's first 12 cuts in bin BIN_A and its last 12 in bin BIN_B, with silent keys in front (n_below), between the
    voters of either part (n_inside in all) and behind (n_above): 24 + n_below + n_inside + n_above keys.  The silent
    keys lie half a second and more from every voter."""
    a, b = _shifted(x24()[:12], BIN_A), _shifted(x24()[12:], BIN_B)
    voters = sorted(a + b)
    gaps = [(lo, hi) for lo, hi in zip(voters[:-1], voters[1:]) if hi - lo > 2.0]
    inside = []
    for i in range(n_inside):
        lo, hi = gaps[i % len(gaps)]
        inside.append(lo + 0.5 + (hi - lo - 1.0) * ((i // len(gaps)) + 0.37) / (n_inside // len(gaps) + 1))
    below = [voters[0] - 2.0 - 0.83 * i for i in range(n_below)]
    above = [voters[-1] + 2.0 + 0.83 * i for i in range(n_above)]
    keys = sorted(voters + inside + below + above)
    assert len(set(keys)) == 24 + n_below + n_inside + n_above
    return keys


def table():
    """-> the rows, in table order: 30 strangers, the film, and the rows made for one case each (49 rows)"""
    rng = np.random.default_rng(77)
    rows = [(1000 + i, np.sort(rng.uniform(0.0, 7200.0, size=int(n))).tolist()) for i, n in enumerate(rng.integers(5, 70, size=30))]
    rows.insert(11, (FILM, film()))
    rows.append((LANES65, two_part_row(3, 36, 2)))              # 65 keys: a part's extremes in different lanes
    rows.append((LANES513, two_part_row(69, 36, 384)))          # 513 keys: the voters lie one lane's stride further on
    rows.append((LONG700, two_part_row(530, 100, 46)))          # 700 keys: every voter beyond the 512 resume positions
    # a later part with two bins of equal votes: 14 cuts in bin 0, then 8 in bin +50 and 8 in bin -50
    rows.append((LATER_TIE, sorted(_shifted(x30()[:14], 0) + _shifted(x30()[14:22], 50) + _shifted(x30()[22:], -50))))
    # two rows of one id: the second is better; then two that are equal in votes (the earlier one has 12 keys, not 13)
    rows.append((SECOND_BETTER, _shifted(x24()[:6], 30)))
    rows.insert(3, (EQUAL_ROWS, sorted(_shifted(x24()[4:12], -7) + [100.0, 101.0, 102.0, 103.0])))
    rows.append((SECOND_BETTER, _shifted(x24()[2:12], 30)))
    rows.append((EQUAL_ROWS, sorted(_shifted(x24()[10:18], 9) + [100.0, 101.0, 102.0, 103.0, 104.0])))
    for i in range(9):
        rows.insert(5 * i + 1, (NINE_ROWS, _shifted(x24()[i:i + 4], i)))
    rows.append((SPECIAL, sorted(_shifted([0.0, 5.0, 9.0], 40) + _shifted([200.0, 207.0, 214.0], -15) + [INF, -INF, 100.0])))
    return rows
