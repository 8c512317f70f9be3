"""The tables, uploads and rate lists of the tvz_align_candidates_rates tests (tests/test_gap_candidates_rates_cpu.py
asserts their premises with the reference, tests/test_gap_candidates_rates_gpu.py runs them on the device).  Plain data,
no code under test.

GAP_EPS = 0.0371 s is tests/gap_candidates_cases.py's: not commensurate with the film's 1/30 s grid.  A rate moves every
gap, so the premise "no gap within 1e-6 bins of an edge" is asserted for every upload at every rate it is probed at
(`scaled_edge_distance`)."""
import numpy as np

from tests import gap_candidates_cases as cs

GAP_EPS = cs.GAP_EPS
FILM = cs.FILM
TRIPLE, NTSC = 3001, 3002
SLOW, FAST, QUARTER, PULLDOWN = 24 / 25, 25 / 24, 1.25, 1000 / 1001
SPEEDS = (SLOW, FAST, QUARTER)
RATES1 = (SLOW,)
RATES2 = (1.0, PULLDOWN)                               # two close rates: one row answers at both
RATES3 = (1.0, SLOW, FAST)
RATES8 = (1.0, SLOW, FAST, PULLDOWN, 1001 / 1000, QUARTER, 0.8, 1.0)      # (the rate 1.0 twice)
RATE_LISTS = (RATES1, RATES2, RATES3, RATES8)
MIN_COUNT = 6                                          # of the speed cases: the wrong rate stays below it


def sped_up(cuts, rho, shift):
    """the upload of a stored video played so that stored ~= rho x upload + shift"""
    return ((np.asarray(cuts, dtype=np.float64) - shift) / rho).tolist()


def triple_base():
    """14 cuts with gaps of 31 to 152 bins, every triple of gaps a code of its own; 4 % of the smallest is over a bin"""
    gaps = (31.71 + 9.3 * np.arange(13)) * GAP_EPS
    return np.concatenate([[700.0], 700.0 + np.cumsum(gaps)])


def table():
    """tests/gap_candidates_cases.py's table, then three rows of ONE id that hold the base at three rates - 7, 9 and 11
    of its positions - and a row that holds the film's first 40 cuts at the 1000/1001 rate"""
    rows = cs.table()
    u = triple_base()
    rows.append((TRIPLE, (u[:10] * 1.0 + 100.0).tolist()))
    rows.insert(3, (TRIPLE, (u[:12] * SLOW + 200.0).tolist()))
    rows.append((TRIPLE, (u * FAST + 300.0).tolist()))
    rows.append((NTSC, (np.asarray(cs.film()[:40]) * PULLDOWN + 64.0).tolist()))
    return rows


def distinct_table():
    """a table of distinct ids: the first row of every id of tests/gap_candidates_cases.py's table and its counting
    table of 65 hit rows (the equivalence with tvz_align_candidates is stated for such a table)"""
    seen, rows = set(), []
    for vid, k in cs.table() + cs.counting_table(65):
        if vid not in seen:
            seen.add(vid)
            rows.append((vid, k))
    return rows


def uploads():
    """-> dict name -> the upload's cuts"""
    f = cs.film()
    u = {}
    u["slow"] = sped_up(f, SLOW, 5.0)
    u["fast"] = sped_up(f, FAST, -40.0)
    u["quarter"] = sped_up(f, QUARTER, 1000.0)
    u["plain"] = (np.asarray(f) + cs.HOUR).tolist()
    u["triple"] = triple_base().tolist()
    u["empty"] = []
    u["three"] = f[:3]
    u["four"] = sped_up(f[:4], SLOW, 9.0)
    u["q514"] = cs.long_query(514, 1)
    u["q515"] = cs.long_query(515, 2)
    u["special"] = cs.uploads()["special"]
    return u


NAMES = ("slow", "fast", "quarter", "plain", "triple", "empty", "three", "four", "q514", "q515", "special")


def queries():
    up = uploads()
    return [up[n] for n in NAMES]


def exclusions():
    """one id per query, different ones: the film for its slow copy, the triple for the base, nothing for the rest"""
    return [FILM if n == "slow" else TRIPLE if n == "triple" else 1000 + i for i, n in enumerate(NAMES)]


def scaled_edge_distance(values, rates, gap_eps=GAP_EPS):
    """the least distance, in bins, of the finite gaps of the sorted values from an integer, over the rates"""
    a = np.asarray(values, dtype=np.float64)
    a = np.sort(a[np.isfinite(a)])
    return min([cs.edge_distance((a * np.float64(r)).tolist(), gap_eps, False) for r in rates] + [float("inf")])


# ---- the fold: more entries than one chunk, ids that repeat, ties ------------------------------------------------
FOLD_ROWS, FOLD_IDS = 300, 97
FOLD_SPEEDS = (1.0, SLOW, FAST, 1.0)
FOLD_RATES = (SLOW, 1.0, PULLDOWN, 1.0, FAST, 1001 / 1000, 1.0, PULLDOWN)


def fold_table():
    """300 rows over 97 ids, three or four rows per id: row i holds the first 4 + (i % 7) cuts of the counting base played
    at the rate FOLD_SPEEDS[i % 4] and moved by a shift of its own, so the counting query finds it best at that rate -
    and, its gaps being short, with fewer positions at the others.  Behind them 5 rows that share nothing."""
    b = cs.base_cuts(cs.BASE_N)
    rows = [(5000 + (i * 31) % FOLD_IDS, (b[:4 + (i % 7)] * FOLD_SPEEDS[i % 4] + 13.0 * i).tolist()) for i in range(FOLD_ROWS)]
    return rows + cs.counting_table(0)


# ---- one rate's list over the capacity ----------------------------------------------------------------------------
def overflow_table():
    """20 rows that the counting query finds at the rate 1.0 and three rows that hold the WHOLE base at the rate 1.25: at
    (1.0, QUARTER) the first list is the longer one, the second holds the three best of the call"""
    rows = cs.counting_table(20)
    b = cs.base_cuts(cs.BASE_N)
    for j in range(3):
        rows.append((7000 + j, (b * QUARTER + 2000.0 + 50.0 * j).tolist()))
    return rows
