"""The table and the uploads of the tvz_align_candidates_long tests (tests/test_gap_candidates_long_cpu.py asserts their
premises with the reference, tests/test_gap_candidates_long_gpu.py runs them on the device).  Plain data, no code under
test.

One MASTER upload of 4,095 cuts (4,092 positions: segments 0..7 of 511 positions and segment 8 of 4); the shorter
uploads are its prefixes, and every stored row is cut out of it and shifted, so which positions of which segment a row
answers is known by construction: the excerpt MASTER[a:b] holds the codes of the positions a .. b - 4.
GAP_EPS and `edge_distance` are tests/gap_candidates_cases.py's."""
import numpy as np

from tests import gap_candidates_cases as cs

GAP_EPS = cs.GAP_EPS
SEG = 511
LENGTHS = (514, 515, 1025, 1026, 4095)
BOUNDARY, SPLIT, ONE_SEG, TWO_SEG, ALL9, TWIN, TIE_LO, TIE_HI = 3001, 3002, 3003, 3004, 3005, 3006, 2990, 3008
STRANGERS = (3100, 3101, 3102)


def master():
    return cs.long_query(4095, 41)


def _cut(m, a, b, shift):
    return (np.asarray(m[a:b]) + shift).tolist()


def all9_row(m):
    """ten cuts out of each of the segments 0..7 (7 positions each) and the last seven cuts (the 4 positions of segment
    8), in the master's order: ascending, and the joints make codes of their own"""
    out = []
    for s in range(8):
        out += m[SEG * s + 20:SEG * s + 30]
    return (np.asarray(out + m[4088:4095]) + 777.0).tolist()


def table():
    m = master()
    rows = [
        (BOUNDARY, _cut(m, 510, 515, 11.0)),               # positions 510 | 511: one on either side of the first boundary
        (SPLIT, _cut(m, 510, 516, 23.0)),                  # positions 510 | 511, 512: min_count - 1 and min_count at 2
        (ONE_SEG, _cut(m, 100, 140, 35.0)),                # 37 positions of segment 0
        (TWO_SEG, _cut(m, 500, 530, 47.0)),                # positions 500..510 | 511..526
        (ALL9, all9_row(m)),
        (TWIN, _cut(m, 200, 220, 59.0)),                   # three rows of one id: 17 and 7 positions of segment 0 ...
        (STRANGERS[0], cs.long_query(300, 77)),
        (TWIN, _cut(m, 300, 310, 61.0)),
        (TIE_HI, _cut(m, 700, 712, 71.0)),                 # 9 positions of segment 1
        (TWIN, _cut(m, 1200, 1230, 67.0)),                 # ... and 27 of segment 2
        (TIE_LO, _cut(m, 50, 58, 83.0)),                   # 5 positions of segment 0 and ...
        (STRANGERS[1], cs.long_query(40, 78)),
        (TIE_LO, _cut(m, 1100, 1107, 89.0)),               # ... 4 of segment 2: 9 as TIE_HI, and the smaller id
        (STRANGERS[2], cs.long_query(3, 79)),
    ]
    return rows


def uploads():
    """-> dict name -> cuts: the master's prefixes at the segment thresholds, the master, the master with one cut more
    (refused: it stands beside the others), a short upload of the lookup's own size and an empty one"""
    m = master()
    u = {f"m{n}": m[:n] for n in LENGTHS}
    u["m4096"] = m + [m[-1] + 5.3]
    u["short"] = _cut(m, 95, 150, 3600.0)
    u["empty"] = []
    return u


# ---- the fold's limits: n entries of ONE segment, each a 4-key row that carries one code of the query ---------------
def limit_query():
    return cs.counting_query()[:4]


def limit_table(ids):
    """a row per id, every one the query's four cuts moved by a shift of its own: count 1 in each"""
    base = np.asarray(cs.base_cuts(cs.BASE_N)[:4])
    return [(int(v), (base + 13.0 * (i + 1)).tolist()) for i, v in enumerate(ids)]


def table_slots(n):
    """the fold's table: the next power of two at or above 2 n, at least 2"""
    s = 2
    while s < 2 * n:
        s <<= 1
    return s


def home(vid, slots):
    """the home slot of an id: the top bits of (id + 1) x 0x9E3779B1 mod 2^32"""
    return (((vid + 1) * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - (slots.bit_length() - 1))


def colliding_ids(n, slots, seed):
    """n distinct ids of which up to 100 share ONE home slot three below the table's end, so that their run wraps round
    it, as many share another, and the rest are what a seeded draw gives"""
    rng = np.random.default_rng(seed)
    k = min(n // 3, 100)
    v = np.arange(1, 1 << 21, dtype=np.uint64)
    h = (((v + np.uint64(1)) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - (slots.bit_length() - 1))
    out = []
    for target in (slots - 3, slots // 2 + 1):
        same = v[h == np.uint64(target)][:k]
        assert same.size == k
        out += [int(x) for x in same]
    seen = set(out)
    assert all(home(x, slots) in (slots - 3, slots // 2 + 1) for x in out)
    while len(out) < n:
        x = int(rng.integers(1, 1 << 30))
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out
