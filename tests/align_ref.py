"""Plain float64 restatement of tvz_align, written from its contract in include/tvz.h (not from
oracle.align_py), and the edge cases the GPU parity test (tests/test_align_gpu.py) runs.

Contract:
  * a row is a set: NaN dropped, -0.0 folded to +0.0, duplicates kept once; row_len = its size;
  * query NaNs are skipped, every other query value votes (duplicates vote again);
  * B = floor(max_offset / eps + 0.5); the pair (row key c, query value q) votes once into bin
    floor((c - q) / eps + 0.5) if that value lies in [-B, B] (so never when it is NaN or infinite);
  * best bin: most votes, then smaller |bin|, then the negative one (no votes at all: bin 0);
  * output row = (video_id, row_len, best_bin, votes in best bin, votes in bin 0).

The best bin is chosen by sorting (row, -votes, |bin|, bin) - a plain comparison of the tuple,
no bit packing.  Rows are processed in chunks of at most ~4M (key, query) pairs.
"""
import math

import numpy as np

MAX_BINS = 4096
GRID_WAVES = 2048 * 4          # the launcher's grid cap (blocks) x waves per block: one row per wave per pass


def n_bins(eps, max_offset):
    return int(math.floor(max_offset / eps + 0.5))


def row_set(ts):
    c = np.asarray(list(ts), dtype=np.float64).reshape(-1)
    c = c[~np.isnan(c)]
    c = np.where(c == 0.0, 0.0, c)          # -0.0 -> +0.0
    return np.unique(c)


def align_ref(rows, query, eps, max_offset, reciprocal=False, chunk_pairs=1 << 22):
    """-> int64 [len(rows), 5].  `reciprocal=True` computes (c - q) * (1 / eps) instead of the
    division: only used to show that a case set tells the two apart."""
    B = n_bins(eps, max_offset)
    assert 2 * B + 1 <= MAX_BINS
    nb = 2 * B + 1
    q = np.asarray(list(query), dtype=np.float64).reshape(-1)
    q = q[~np.isnan(q)]
    sets = [row_set(ts) for _, ts in rows]
    R = len(rows)
    out = np.zeros((R, 5), dtype=np.int64)
    out[:, 0] = [int(v) for v, _ in rows]
    out[:, 1] = [len(s) for s in sets]
    if R == 0 or q.size == 0:
        return out
    inv = 1.0 / eps
    r0 = 0
    while r0 < R:
        r1, pairs = r0, 0
        while r1 < R and (r1 == r0 or pairs + len(sets[r1]) * q.size <= chunk_pairs):
            pairs += len(sets[r1]) * q.size
            r1 += 1
        lens = np.array([len(s) for s in sets[r0:r1]], dtype=np.int64)
        if lens.sum():
            c = np.concatenate(sets[r0:r1])
            ri = np.repeat(np.arange(r0, r1, dtype=np.int64), lens)
            with np.errstate(invalid="ignore", over="ignore"):
                diff = c[:, None] - q[None, :]
                x = diff * inv if reciprocal else diff / eps
                b = np.floor(x + 0.5)
                ok = (b >= -B) & (b <= B)
            rr = np.broadcast_to(ri[:, None], b.shape)[ok]
            bins = b[ok].astype(np.int64)
            codes, votes = np.unique(rr * nb + (bins + B), return_counts=True)
            if codes.size == 0:
                r0 = r1
                continue
            row_u, bin_u = codes // nb, codes % nb - B
            zero = bin_u == 0
            out[row_u[zero], 4] = votes[zero]
            order = np.lexsort((bin_u, np.abs(bin_u), -votes, row_u))   # last key is the primary one
            ro = row_u[order]
            first = order[np.r_[True, ro[1:] != ro[:-1]]]
            out[row_u[first], 2] = bin_u[first]
            out[row_u[first], 3] = votes[first]
        r0 = r1
    return out


# ---------------------------------------------------------------- the edge cases (shared CPU / GPU)
# A case: (name, rows [(video_id, [keys])], [(query, eps, max_offset), ...]).  One upload per case,
# one tvz_align call per (query, eps, max_offset).

def grid_stride_case(n_rows=20_000):
    """More rows than the grid has waves: wave w takes rows w, w + GRID_WAVES, w + 2 GRID_WAVES.
    Rows of the first pass carry a strong peak, rows of the second pass have no vote at all (their
    keys are far from every query value), rows of the third pass a peak elsewhere.  A histogram not
    cleared between a wave's rows shows as votes in the second pass."""
    q = np.arange(1, 13, dtype=np.float64)
    rows = []
    for r in range(n_rows):
        n = 1 + r % 12
        if r < GRID_WAVES:
            keys = q[:n] + ((r % 7) - 3) * 0.1
        elif r < 2 * GRID_WAVES:
            keys = 1000.0 + q[:n]
        else:
            keys = q[12 - n:] + ((r % 5) - 2) * 0.1
        rows.append((r + 1, keys.tolist()))
    return "grid_stride", rows, [(q.tolist(), 0.1, 0.3)]


def long_rows_case():
    """Rows of 63, 64, 65, 128 and 1,000 keys (the lane loop runs j, j + 64, ...), duplicate keys in
    a row, duplicate values in the query; the query holds every key of the long rows, so a key the
    lane loop skipped changes the bin-0 count."""
    rng = np.random.default_rng(5)
    keys = np.round(np.arange(1000) * 0.37 + 0.05, 6)
    rows = [(1, keys[:63]), (2, keys[:64]), (3, keys[:65]), (4, keys[:128]), (5, keys[:1000]),
            (6, rng.permutation(np.concatenate([keys[:100], keys[:100], keys[40:90]]))),
            (7, keys[500:1000] + 0.2), (8, keys[::-1][:129])]
    rows = [(v, k.tolist()) for v, k in rows]
    query = rng.permutation(np.concatenate([keys[:700], keys[60:70], keys[60:62]])).tolist()
    return "long_rows", rows, [(query, 0.05, 0.5), (keys[:66].tolist(), 0.05, 0.0),
                               ((keys[:80] + 0.2).tolist(), 0.1, 1.0)]


def special_keys_case():
    """Infinities, huge and subnormal keys, signed zeros, NaN in rows and queries, the empty row,
    the empty query and a NaN-only query."""
    inf, nan = float("inf"), float("nan")
    rows = [(1, [inf, -inf, 1.0]), (2, [1e300, -1e300, 0.0]), (3, [5e-324, -5e-324, -0.0, 0.0]),
            (4, [nan, 1.0, nan]), (5, []), (6, [nan]), (7, [-0.0]), (8, [inf]), (9, [0.1, 0.2, -0.1]),
            (10, [2.0, 1.5, 1.0, 0.5, 0.0, -0.5])]
    queries = [[0.0, 5e-324, 1e300, -0.0, 1.0, nan, inf], [], [nan, nan], [-0.0], [inf, -inf],
               [0.0, 0.0, 0.0, 1.0], [5e-324], [-1e300, 1e300]]
    return "special_keys", rows, [(q, 0.1, 1.0) for q in queries] + [([0.0, 1.0], 0.5, 1.0)]


def bin_limits_case():
    """B = 0 (max_offset < eps/2), B = 2047 (4,095 bins: the largest accepted), votes landing exactly
    at +-B and at +-(B + 1), and a row whose only votes are at +B and -B (the tie goes to -B)."""
    q0 = 100.0
    e = 1 / 64                                     # dyadic: every difference below is exact
    rows = [(1, [q0 + 2047 * e]), (2, [q0 - 2047 * e]), (3, [q0 + 2048 * e]), (4, [q0 - 2048 * e]),
            (5, [q0 + 2047 * e, q0 - 2047 * e]), (6, [q0 + 2048 * e, q0 - 2048 * e, q0 + 2046 * e]),
            (7, [q0, q0 + 0.04, q0 - 0.04, q0 + 0.06, q0 - 0.06]), (8, [q0 + 0.05, q0 - 0.05]),
            (9, [q0 + 50 * 0.1, q0 - 50 * 0.1, q0 + 51 * 0.1, q0 - 51 * 0.1]), (10, [q0 + 0.5, q0 - 0.5])]
    calls = [([q0], e, 2047 * e), ([q0], e, 2047.49 * e), ([q0], 0.1, 0.04), ([q0], 0.1, 0.0),
             ([q0], 0.1, 5.0), ([q0], 1.0, 0.49), ([q0, q0 + 0.5], 1.0, 0.5)]
    return "bin_limits", rows, calls


BOUNDARY_EPS = (0.1, 1 / 30, 1 / 24, 1 / 60)


def boundary_case(k_max=80, ulps=4):
    """Keys within +-4 ulps of (k + 1/2) eps for each eps of BOUNDARY_EPS, k in [-k_max, k_max), one key
    per row, query [0.0] (so c - q = c exactly): the bin is decided by the last bits of c / eps.
    Replacing the division by a multiplication with 1/eps moves some of them (align_ref(...,
    reciprocal=True), tests/test_align_cpu.py)."""
    rows, vid = [], 1
    for eps in BOUNDARY_EPS:
        for k in range(-k_max, k_max):
            t = (k + 0.5) * eps
            v = t
            for _ in range(ulps):
                v = np.nextafter(v, -np.inf)
            for _ in range(2 * ulps + 1):
                rows.append((vid, [float(v)]))
                vid += 1
                v = np.nextafter(v, np.inf)
    return "boundary", rows, [([0.0], eps, (k_max + 1) * eps) for eps in BOUNDARY_EPS]


def ties_case():
    """+b against -b, |1| against |2|, bin 0 against a neighbour, a real majority, no votes at all."""
    rows = [(1, [2.0, -2.0]), (2, [1.0, -2.0]), (3, [-1.0, 2.0]), (4, [-1.0, 1.0]), (5, [0.0, 1.0]),
            (6, [3.0, -3.0, 4.0, 4.2]), (7, [100.0]), (8, [2.0, 12.0, -2.0, 8.0]), (9, [5.0, -5.0]),
            (10, [-3.0, 3.0, 13.0, 7.0]), (11, [])]
    return "ties", rows, [([0.0], 1.0, 5.0), ([0.0, 10.0], 1.0, 5.0), ([0.0, 10.0, 10.0], 1.0, 5.0)]


def edge_cases():
    return [grid_stride_case(), long_rows_case(), special_keys_case(), bin_limits_case(), boundary_case(),
            ties_case()]


# (eps, max_offset) pairs tvz_align must refuse, and the error each one gets (include/tvz.h)
ERR_INVALID, ERR_UNSUPPORTED = -1, -4
REFUSALS = [(1 / 64, 2048 / 64, ERR_UNSUPPORTED),            # B = 2048: 4,097 bins
            (1 / 64, 2047.5 / 64, ERR_UNSUPPORTED),          # rounds up to B = 2048
            (0.1, float("inf"), ERR_UNSUPPORTED),
            (float("inf"), float("inf"), ERR_UNSUPPORTED),   # inf / inf = NaN bins
            (0.0, 1.0, ERR_INVALID), (-0.1, 1.0, ERR_INVALID), (-0.0, 1.0, ERR_INVALID),
            (float("nan"), 1.0, ERR_INVALID), (0.1, float("nan"), ERR_INVALID), (0.1, -1.0, ERR_INVALID)]
