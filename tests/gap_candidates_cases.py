"""The tables and the uploads of the tvz_align_candidates tests (tests/test_gap_candidates_cpu.py asserts their premises
with the reference, tests/test_gap_candidates_gpu.py runs them on the device).  Plain data, no code under test.

GAP_EPS = 0.0371 s is not commensurate with the film's 1/30 s grid, so no gap of the film sits on a bin edge (the
query side's edges are the integers, the stored side's the half-integers); `edge_distance` is what the CPU test holds
against 1e-6 bins for every table row and every upload whose premise depends on it."""
import numpy as np

from tests import align_parts_cases as pc

GAP_EPS = 0.0371
GAP_EPS_2 = 0.0533                                   # the second width of the change-of-gap_eps test
NAN, INF = float("nan"), float("inf")
HOUR = 3600.0
FILM = pc.FILM
ROW0, ROW1, ROW3, ROW4, TWIN, WIDE_GAP, SPECIAL_ROW = 2000, 2001, 2003, 2004, 2005, 2006, 2007
MAX_BIN = (1 << 17) - 1


def film():
    return pc.film()


def twin_rows():
    """two rows of one id, equal in every count: the same cuts"""
    return [3.0 + 1.7 * i + 0.013 * i * i for i in range(12)]


def wide_gap_row():
    """cuts around a gap of more than 2^17 bins: the positions whose three gaps include it have no code"""
    a = [10.0 + 2.3 * i + 0.017 * i * i for i in range(8)]
    far = a[-1] + (MAX_BIN + 5.37) * GAP_EPS
    return a + [far + 2.9 * i + 0.019 * i * i for i in range(8)]


def table():
    """-> the rows, in table order: the parts tests' table (strangers, the film, rows of 65 / 513 / 700 keys, rows of one
    id, a row with +-inf) and rows of 0 / 1 / 3 / 4 keys, two equal rows of one id and a row with a gap beyond the bins"""
    rows = pc.table()
    rows.append((ROW0, []))
    rows.insert(7, (ROW1, [12.5]))
    rows.append((ROW3, [1.0, 2.5, 4.75]))
    rows.append((ROW4, [1.0, 2.5, 4.75, 8.125]))
    rows.insert(20, (TWIN, twin_rows()))
    rows.append((TWIN, twin_rows()))
    rows.append((WIDE_GAP, wide_gap_row()))
    # what the "special" upload finds: its doubled 200.0 is a gap of 0 bins there and of 0.81 bins (bin 1) here
    rows.append((SPECIAL_ROW, [-0.0, 5.0, 9.0, 200.0, 200.03, 207.03, 214.03, INF, NAN, 0.0]))
    return rows


def jittered(x, seed, amount):
    """every cut moved by less than `amount` seconds either way: every gap moves by less than 2 x amount"""
    rng = np.random.default_rng(seed)
    return (np.asarray(x) + rng.uniform(-amount, amount, size=len(x))).tolist()


def uploads():
    """-> dict name -> the upload's cuts"""
    f = np.asarray(film())
    p = pc.uploads()
    u = {}
    u["shifted"] = (f + HOUR).tolist()
    u["jitter_small"] = jittered(f + HOUR, 11, 0.0005)
    u["jitter_quarter"] = jittered(f + 17.0, 12, 0.24 * GAP_EPS)          # every gap moves by < gap_eps / 2
    u["excerpt"] = (f[50:70] + 123.0).tolist()
    u["inserted"] = p["inserted"]
    u["removed"] = p["removed"]
    u["stranger"] = p["unrelated"]
    u["special"] = [-0.0, 0.0, 5.0, 9.0, 9.0, NAN, INF, -INF, 200.0, 200.0, 207.0, 214.0, 214.0, 0.0, NAN]
    u["row4"] = [101.0, 102.5, 104.75, 108.125]                            # ROW4 shifted by 100 s
    u["twin"] = (np.asarray(twin_rows()) + 500.0).tolist()
    u["wide_gap"] = (np.asarray(wide_gap_row()) + 77.0).tolist()
    u["unsorted"] = (f[::-1] + 5.0).tolist()                               # the film backwards: the call sorts
    u["empty"] = []
    u["three"] = f[:3].tolist()
    u["four"] = (f[:4] + 9.0).tolist()
    return u


def edge_distance(values, gap_eps, stored):
    """the least distance, in bins, of the finite gaps of sorted `values` from a bin edge: the half-integers on the
    stored side (floor(r + 0.5)), the integers on the query side (floor(r)); inf where there is no finite gap"""
    a = np.asarray(values, dtype=np.float64)
    a = np.sort(a[np.isfinite(a)])
    if stored:
        a = np.unique(a)
    if a.size < 2:
        return float("inf")
    r = (a[1:] - a[:-1]) / gap_eps
    r = r[r > 0]                                     # (duplicate query values: the gap is exactly 0, on no edge's wrong side)
    if r.size == 0:
        return float("inf")
    x = r + 0.5 if stored else r
    return float(np.min(np.abs(x - np.round(x))))


# ---- the counting table: hit counts and ties by construction ------------------------------------------------------
def base_cuts(n):
    """n cuts whose gaps grow by 3.3 bins each: every triple of consecutive gaps is a code of its own"""
    gaps = (7.31 + 3.3 * np.arange(n - 1)) * GAP_EPS
    return np.concatenate([[50.0], 50.0 + np.cumsum(gaps)])


BASE_N = 12                                          # 9 positions: counts 1..9


def counting_table(n_rows, seed=5):
    """n_rows rows; row i holds the first 4 + (i % 7) cuts of the base, moved by a shift of its own, so the whole base as
    a query counts 1 + (i % 7) in it: ties in plenty, which the ids - a permutation, so that table order is not id order
    - decide.  Behind them 5 rows that share nothing with the base."""
    rng = np.random.default_rng(seed)
    ids = 5000 + rng.permutation(max(n_rows, 1))[:n_rows]
    b = base_cuts(BASE_N)
    rows = [(int(ids[i]), (b[:4 + (i % 7)] + 13.0 * i).tolist()) for i in range(n_rows)]
    for j in range(5):
        rows.append((9000 + j, (1000.0 + np.cumsum((3.77 + 1.9 * np.arange(9) + 0.27 * j) * GAP_EPS)).tolist()))
    return rows


def counting_query():
    return (base_cuts(BASE_N) + 4321.0).tolist()


HIT_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257)

# ---- the offsets scan over more queries than it has threads -------------------------------------------------------
SCAN_Q = 2049                                        # 1,024 threads take 3 probe lists each, the last 341 none
SCAN_LONG = (1023, 2048)                             # the first list of thread 341, the last list of thread 682 (and of all)
SCAN_CALL = dict(c=2, min_count=1, cap=4, max_query_len=4)


def scan_case():
    """-> (table, queries, exclude_ids): counting_table(2), whose two rows both hold the base's first position, and
    SCAN_Q tiny queries on it - that position's 4 values mostly, 3 or 0 values every seventh, and 5 values (longer than
    the call's max_query_len: refused) at SCAN_LONG - with exclusions that alternate between the two rows' ids and -1."""
    rows = counting_table(2)
    q = counting_query()
    kinds = [q[:4], q[:3], []]
    queries = [kinds[0] if i % 7 else kinds[1 + (i // 7) % 2] for i in range(SCAN_Q)]
    for i in SCAN_LONG:
        queries[i] = q[:5]
    excl = [rows[0][0] if i % 2 else rows[1][0] if i % 3 == 0 else -1 for i in range(SCAN_Q)]
    return rows, queries, excl


def scan_expected(rows, queries, excl):
    """-> (int64 [SCAN_Q, 3, 2], memo): the reference's block of every query, computed once per (length, exclusion)"""
    from tests import gap_candidates_ref as ref
    memo = {}
    exp = np.zeros((len(queries), SCAN_CALL["c"] + 1, 2), dtype=np.int64)
    for i, (query, ex) in enumerate(zip(queries, excl)):
        key = (len(query), ex)
        if key not in memo:
            memo[key] = ref.candidates(rows, [query], GAP_EPS, exclude_ids=[ex], **SCAN_CALL)[0].astype(np.int64)
        exp[i] = memo[key]
    return exp, memo


def long_query(n, seed):
    """n cuts, gaps of 20 to 400 bins: for the lengths at the probe limit (514 passes, 515 is refused)"""
    rng = np.random.default_rng(seed)
    return (100.0 + np.cumsum(rng.uniform(20.0, 400.0, size=n) * GAP_EPS)).tolist()
