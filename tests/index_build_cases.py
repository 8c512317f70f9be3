"""Shapes, generators and a restatement of the sizing for the build-regime tests of the inverted index
(tests/test_index_build_cases_cpu.py checks this module without a GPU; tests/test_index_build_regimes_gpu.py runs it).

build_classic (tvidz_amd/csrc/tvz_index_build.h) builds the open-addressing directory in one of three ways that are
different code: slice by slice with slices of 32 KB, slice by slice with slices grown to 64 / 128 KB (a directory of more
than kIxMaxParts slices of 32 KB), or by the count and fill over the whole directory (more than kIxMaxParts slices of
128 KB).  The entry grows with the sub-indexes (16 + 2 bytes per sub-index, rounded up to 8), i.e. with the ROW count.
So a corpus of short rows reaches every regime: `layout` below restates where the sizing ends, SHAPES names five
corpora, `corpus` and `queries` generate them (seeded numpy, CSR, every row sorted and without repeats)."""
import functools
from collections import namedtuple

import numpy as np

# the constants the restatement assumes; the CPU test reads them from the sources
CONSTANTS = dict(kIxMaxParts=4096, kIxSliceBytes=32 * 1024, kIxSliceBytesMax=128 * 1024, kIxDirLoadPct=25,
                 kIxSliceLdsFloor=40 * 1024, TVZ_IX_SUB_LOG2=14, kIxStagePairs=8192)
SUB_ROWS = 1 << CONSTANTS["TVZ_IX_SUB_LOG2"]
LDS_PER_WORKGROUP = 160 * 1024          # gfx950
HIT_CAP = 16384                         # the GPU test's hit capacity per query: no query may have more hits
K = 16                                  # ... and its top-k

Layout = namedtuple("Layout", "entry_bytes log2 slice_log2 partitioned")


# ---- the sizing, restated -------------------------------------------------------------------------------------------
def n_sub(n_rows):
    return -(-n_rows // SUB_ROWS)


def ix_ks(subs):
    return 0 if subs <= 1 else (subs + 7) & ~7


def ix_entry_bytes(ks):
    return 16 + 2 * ks


def slice_log2_for(log2, es):
    """The slice-size loop: slices of up to kIxSliceBytes, grown up to kIxSliceBytesMax while they outnumber kIxMaxParts."""
    C = CONSTANTS
    sl = 6
    while (2 << sl) * es <= C["kIxSliceBytes"] and sl < log2:
        sl += 1
    while ((1 << log2) >> sl) > C["kIxMaxParts"] and (2 << sl) * es <= C["kIxSliceBytesMax"]:
        sl += 1
    return sl


def partitionable(log2, es):
    sl = slice_log2_for(log2, es)
    return ((1 << log2) >> sl) <= CONSTANTS["kIxMaxParts"] and (es << sl) <= CONSTANTS["kIxSliceBytesMax"]


def size_for(distinct, es):
    """log2 of the directory for `distinct` keys: load <= kIxDirLoadPct, one step down (load <= 0.5) where only the
    smaller directory can be built slice by slice."""
    lg = 10
    while float(1 << lg) * CONSTANTS["kIxDirLoadPct"] < 100.0 * distinct and lg < 30:
        lg += 1
    if not partitionable(lg, es) and partitionable(lg - 1, es) and float(1 << (lg - 1)) >= 2.0 * distinct:
        lg -= 1
    return lg


def layout(n_rows, live_keys, distinct, hint=None, guess=0, trace=None):
    """Where build_classic ends for `distinct` distinct keys among the `live_keys` keys of `n_rows` rows:
    (entry_bytes, log2, slice_log2, partitioned).  hint = (postings, distinct keys) of the directory's last build, None
    for a first build; guess > 0 = the first build of a cell directory (the key directory's distinct count).  A build is
    accepted at load <= 0.5 (no slice overflows there: a slice of 512 entries or more at that load is 16 sigma from
    full), is repeated ONCE at the size the count revealed if that is another one ("shrink once"), and doubles the
    directory while it is too crowded.  `trace`, a list, gets (log2, partitioned) of every attempt."""
    subs = n_sub(n_rows)
    es = ix_entry_bytes(ix_ks(subs))
    # (postings keep 32-bit offsets: a limit that only a corpus of more than 10^9 keys meets)
    post_cap = 2 * live_keys + CONSTANTS["kIxMaxParts"] * 7 * 64 + 64 + 512
    if hint is not None and hint[0] > 0:
        log2 = size_for(float(hint[1]) * float(live_keys) / float(hint[0]) * 1.25, es)
    elif guess > 0:
        log2 = size_for(float(guess), es)
    else:
        log2 = 10
        while (1 << log2) < live_keys // 8:
            log2 += 1
    shrunk = False
    while True:
        assert log2 <= 30
        sl = slice_log2_for(log2, es)
        part = ((1 << log2) >> sl) <= CONSTANTS["kIxMaxParts"] and post_cap < 0xfffffff0 and \
            (es << sl) <= CONSTANTS["kIxSliceBytesMax"]
        if not part:
            sl = log2
        if trace is not None:
            trace.append((log2, part))
        if distinct * 2 <= (1 << log2):
            fit = size_for(float(distinct), es)
            if not shrunk and (fit + 1 < log2 or fit > log2):
                log2, shrunk = fit, True
                continue
            return Layout(es, log2, sl, int(part))
        log2 += 1


def slice_lds_bytes(lay):
    """dynamic LDS a slice block of the partitioned build asks for"""
    return max(lay.entry_bytes << lay.slice_log2, CONSTANTS["kIxSliceLdsFloor"])


def scatter_lds_bytes(lay):
    """dynamic LDS of the scatter kernel: the staging area + three words per slice"""
    return CONSTANTS["kIxStagePairs"] * 12 + (3 * (1 << (lay.log2 - lay.slice_log2)) + 1) * 4


def delta_trigger(n_main):
    return max(512, n_main // 256)


def directory_bytes(lay):
    return lay.entry_bytes << lay.log2


def fill_cursor_bytes(lay):
    """the unpartitioned build's cursors: a 32-bit word per entry and pair of sub-indexes"""
    return 0 if lay.partitioned else (4 << lay.log2) * max((lay.entry_bytes - 16) // 4, 1)


def footprint_bytes(lay):
    """Device bytes that a handle keeps for a classic directory `lay`: the directory, the shadow generation that
    build_index pre-sizes with room to double once, the fill cursors pre-sized the same way."""
    return 3 * directory_bytes(lay) + 2 * fill_cursor_bytes(lay)


# ---- shapes ---------------------------------------------------------------------------------------------------------
# name: rows, own keys per row, alphabet of the own keys (None: all distinct), the regime it is named for:
# (entry_bytes, log2, slice_log2, partitioned) of the first build and of the hinted rebuild
Shape = namedtuple("Shape", "name rows own alphabet first rebuilt")
ROWS_2 = SUB_ROWS + 1024                 # 17,408: two sub-indexes, 32-byte entries
ROWS_57 = 56 * SUB_ROWS + 4096           # 921,600: 57 sub-indexes (the last one partial, not tiny), 144-byte entries
SHAPES = {s.name: s for s in (
    Shape("slice64k", ROWS_2, 80, None, Layout(32, 23, 11, 1), Layout(32, 23, 11, 1)),
    Shape("slice128k", ROWS_2, 140, None, Layout(32, 24, 12, 1), Layout(32, 24, 12, 1)),
    Shape("slice128k_half_load", ROWS_2, 270, None, Layout(32, 24, 12, 1), Layout(32, 24, 12, 1)),
    Shape("wide_partitioned", ROWS_57, 2, 600_000, Layout(144, 21, 9, 1), Layout(144, 21, 9, 1)),
    Shape("wide_unpartitioned", ROWS_57, 2, None, Layout(144, 23, 23, 0), Layout(144, 24, 24, 0)),
)}
TWO_SUB = ("slice64k", "slice128k", "slice128k_half_load")
MUTATED = ("slice128k_half_load", "wide_partitioned", "wide_unpartitioned")
WIDE = ("wide_partitioned", "wide_unpartitioned")

OWN_BASE, OWN_STEP = 1000.0, 0.125       # own keys: OWN_BASE + OWN_STEP * (1 + n), exact in float64
NEAR = 0.0004                            # a second own key this far above another: two keys in one 1 ms cell
POOL = 1.0 + 0.5 * np.arange(32)         # the common keys, all below OWN_BASE
P_EVERY, P_FIRST, P_LAST, P_MID, P_LONG = 0, 24, 25, 26, 27      # POOL[:24] is spread at random; the rest has roles
LONG_POSTINGS = 100                      # rows of ONE sub-index that hold POOL[P_LONG]: more than a line of postings

Corpus = namedtuple("Corpus", "ids offs keys")


def special_rows(shape):
    """rows the queries copy and the mutations replace: 0, the two sides of the first sub-index boundary, one of a
    middle sub-index, the last"""
    n = shape.rows
    return [0, SUB_ROWS - 1, SUB_ROWS, (n_sub(n) // 2) * SUB_ROWS + 4321 % (n - (n_sub(n) // 2) * SUB_ROWS), n - 1]


def long_sub(shape):
    return min(1, n_sub(shape.rows) - 1)


def _pairs_to_csr(n_rows, row, key):
    """(row, key) pairs in any order, repeats allowed -> CSR with every row sorted and without repeats"""
    order = np.lexsort((key, row))
    row, key = row[order], key[order]
    keep = np.ones(row.size, dtype=bool)
    keep[1:] = (row[1:] != row[:-1]) | (key[1:] != key[:-1])
    row, key = row[keep], key[keep]
    offs = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n_rows), out=offs[1:])
    return offs, np.ascontiguousarray(key)


@functools.lru_cache(maxsize=None)
def corpus(name):
    """The corpus of shape `name`: video ids 1..rows, offsets, keys.  Read-only (the arrays are shared)."""
    s = SHAPES[name]
    n, subs = s.rows, n_sub(s.rows)
    rng = np.random.default_rng(sorted(SHAPES).index(name) + 11)
    r = np.repeat(np.arange(n, dtype=np.int64), s.own)
    if s.alphabet is None:
        v = np.arange(n * s.own, dtype=np.int64)
    else:                                # two different letters per row
        a = rng.integers(0, s.alphabet, size=n)
        b = (a + 1 + rng.integers(0, s.alphabet - 1, size=n)) % s.alphabet
        v = np.stack([a, b], axis=1).reshape(-1)
    rows, keys = [r], [OWN_BASE + OWN_STEP * (1 + v)]
    # a few rows with a second key NEAR above their first own key
    near = np.array(special_rows(s) + [5, n // 3], dtype=np.int64)
    rows.append(near)
    keys.append(keys[0][near * s.own] + NEAR)
    # common keys: ~1 % of the rows carry one to three of POOL[:24] ...
    carriers = rng.choice(n, size=n // 100, replace=False)
    for take in (1.0, 0.6, 0.3):
        c = carriers[rng.random(carriers.size) < take]
        rows.append(c)
        keys.append(POOL[rng.integers(0, 24, size=c.size)])
    # ... POOL[0] is in every sub-index; three keys live in one sub-index only (the first, the last, a middle one);
    # one has more than a line of postings inside one sub-index; three rows hold the first eight (min_match 6)
    mid = subs // 2
    fixed = [(np.arange(subs) * SUB_ROWS + 7, P_EVERY), (np.array([10, 200, 3000]), P_FIRST),
             (np.array([n - 1, n - 50, n - 700]), P_LAST), (mid * SUB_ROWS + np.array([1, 100, 777]), P_MID),
             (long_sub(s) * SUB_ROWS + 3 * np.arange(LONG_POSTINGS), P_LONG)]
    for rr, p in fixed:
        rows.append(np.asarray(rr, dtype=np.int64))
        keys.append(np.full(len(rr), POOL[p]))
    heavy = np.array([SUB_ROWS - 1, SUB_ROWS, n - 1], dtype=np.int64)
    rows.append(np.repeat(heavy, 8))
    keys.append(np.tile(POOL[:8], heavy.size))
    offs, k = _pairs_to_csr(n, np.concatenate(rows), np.concatenate(keys))
    ids = np.arange(1, n + 1, dtype=np.int32)
    for a in (ids, offs, k):
        a.setflags(write=False)
    return Corpus(ids, offs, k)


def row_keys(c, r):
    return c.keys[c.offs[r]:c.offs[r + 1]]


@functools.lru_cache(maxsize=None)
def queries(name):
    """At most 8 queries: copies of the special rows, two rows to a query; the whole pool; one common key three times;
    keys that are in no row; a mix."""
    s, c = SHAPES[name], corpus(name)
    r0, r1, r2, rm, rl = special_rows(s)
    absent = OWN_BASE + OWN_STEP * (1 + np.arange(0, 40)) + OWN_STEP / 2        # between the own keys
    qs = [np.concatenate([row_keys(c, r0), row_keys(c, r1)]),
          np.concatenate([row_keys(c, r2), row_keys(c, rm)]),
          np.concatenate([row_keys(c, rl), row_keys(c, r0)]),
          POOL.copy(),
          np.array([POOL[P_EVERY]] * 3),
          np.concatenate([absent, [999.25, 2.25, -1.0]]),
          np.concatenate([row_keys(c, rm)[::-1], [POOL[P_LONG], POOL[P_MID]], absent[:5], row_keys(c, 5)])]
    return [np.ascontiguousarray(q, dtype=np.float64) for q in qs]


def counts(c):
    """(live keys, exact distinct keys) of a corpus"""
    return int(c.keys.size), int(np.unique(c.keys).size)


def cell_counts(c, w):
    """(postings, distinct cells) of the cell directory of width w: one posting per (cell, row); cell = floor(key / w)
    (the keys here are far inside the clamp at +-2^40 cells)"""
    cell = np.floor(c.keys / w).astype(np.int64)
    row = np.repeat(np.arange(c.ids.size), np.diff(c.offs))
    first = np.ones(cell.size, dtype=bool)
    first[1:] = (row[1:] != row[:-1]) | (cell[1:] != cell[:-1])
    return int(first.sum()), int(np.unique(cell).size)


def edit(c, replaced, appended):
    """The corpus after upserts: replaced = {row: keys} (the row keeps its id), appended = [(video_id, keys)]."""
    n = c.ids.size
    lens = np.diff(c.offs)
    row = np.repeat(np.arange(n), lens)
    keep = ~np.isin(row, np.fromiter(replaced.keys(), dtype=np.int64, count=len(replaced)))
    rows, keys = [row[keep]], [c.keys[keep]]
    for r, k in replaced.items():
        rows.append(np.full(len(k), r, dtype=np.int64))
        keys.append(np.asarray(k, dtype=np.float64))
    for i, (_, k) in enumerate(appended):
        rows.append(np.full(len(k), n + i, dtype=np.int64))
        keys.append(np.asarray(k, dtype=np.float64))
    offs, k = _pairs_to_csr(n + len(appended), np.concatenate(rows), np.concatenate(keys))
    ids = np.concatenate([c.ids, np.array([v for v, _ in appended], dtype=np.int32)])
    return Corpus(ids, offs, k)


def mutations(name):
    """Step 4's edits of shape `name`: ({row: keys} replacing ~40 indexed rows by copies of query rows or emptying
    them, [(new id, keys)] ~40 appended rows).  The replaced rows include rows of the first and of the last sub-index
    and both sides of the first sub-index boundary."""
    s, c = SHAPES[name], corpus(name)
    n = s.rows
    sp = special_rows(s)
    targets = [1, 2, 3, SUB_ROWS - 1, SUB_ROWS, SUB_ROWS + 1, n - 2, n - 3] + \
        [int(x) for x in np.linspace(50, n - 60, 30).astype(np.int64)]
    replaced = {}
    for i, t in enumerate(targets):
        replaced[t] = row_keys(c, sp[i % len(sp)]).copy()
    for t in (4, SUB_ROWS + 2, n - 4, n // 2):
        replaced[t] = np.zeros(0)
    appended = [(n + 1 + i, row_keys(c, sp[i % len(sp)]).copy()) for i in range(40)]
    return replaced, appended


def filler(i):
    """Row i of the upserts that fill the delta table: two keys that no query and no other row holds."""
    return np.array([5.0e6 + i, 5.0e6 + i + 0.5])


# ---- references -----------------------------------------------------------------------------------------------------
def tol_sorted(c):
    """every key of the corpus in numeric order with its row: what tol_expected searches (make it once per corpus)"""
    order = np.argsort(c.keys, kind="stable")
    return c.keys[order], np.repeat(np.arange(c.ids.size), np.diff(c.offs))[order]


def tol_expected(c, q, tol, mm, pre=None):
    """The tolerant match of one query, from the contract in include/tvz.h (tests/tol_ref.py), in plain float64 over the
    whole corpus at once: element i matches a row that holds a key with key == q[i] or |q[i] - key| <= tol; count =
    matching elements, kth = index of the mm-th.  -> sorted [(video_id, count, kth)]."""
    sk, row_of = pre if pre is not None else tol_sorted(c)
    per_row = {}
    for i, x in enumerate(np.asarray(q, dtype=np.float64)):
        if np.isnan(x):
            continue
        lo = np.searchsorted(sk, x - 2 * tol - 1e-9, side="left")       # a window wider than the match, then the rule
        hi = np.searchsorted(sk, x + 2 * tol + 1e-9, side="right")
        k = sk[lo:hi]
        ok = (k == x) | (np.abs(x - k) <= tol)
        for r in np.unique(row_of[lo:hi][ok]):
            per_row.setdefault(int(r), []).append(i)
    return sorted((int(c.ids[r]), len(ix), ix[mm - 1]) for r, ix in per_row.items() if len(ix) >= mm)


def tol_queries(name):
    """the queries of the tolerant calls: `queries`, and a copy of the last row moved by 0.3 ms"""
    return queries(name) + [row_keys(corpus(name), SHAPES[name].rows - 1) + 0.0003]
