"""Threshold cases of the index lookup, with a restatement of what decides a lookup's path (tests/test_lookup_cases_cpu.py
checks this module without a GPU; tests/test_lookup_edges_gpu.py runs it against the oracle).

The lookup kernels (tvidz_amd/csrc/tvz_index_kernels.h, tvz_index_wave_kernels.h) are built from fixed-size stages with
different code on either side of the size: a wave of the block kernel caches kIxPW postings and walks the rest from the
lists again; query positions come in chunks of kIxBlock; candidates in parts of kIxSlots; the fused top-k keeps
kIxTkCap entries and reads its bound from a histogram of kIxTkBins bins; the one-wave kernel holds kWqRegPost postings
in registers; an unfused lookup spreads a query over groups of sub-indexes.  Every case here is a small corpus (CSR,
every row sorted and without repeats) and a few queries built so that the sizes land ON those limits - N - 1, N, N + 1 -
and so that the hits depend on the postings on the far side.  `reaches` names the facts a case is built to reach; the
CPU test computes them again from the case's data with the restatements below.

Who owns what (restated): position i < kIxBlock of a query belongs to wave i % kIxWaves of the block kernel, whose flat
posting space holds its positions' lists in ascending position order; the one-wave kernel's flat space holds all
positions' lists in ascending position order.  The ORDER of the postings inside one list is the build's (atomics): no
case depends on it - a list that straddles a limit holds only rows for which that list's posting is the deciding one,
so whichever of them lie beyond the limit, dropping them changes the answer."""
import functools
from collections import namedtuple

import numpy as np

from tests.index_build_cases import Corpus, _pairs_to_csr, edit          # noqa: F401 (edit: used by the GPU module)

# the constants the cases assume; the CPU test reads them from the sources
CONSTANTS = dict(kIxPW=512, kIxBlock=512, kIxWaves=8, kIxSlots=512, kIxCache=4096, kIxTkCap=128, kIxTkBins=64,
                 kIxTkMaxK=64, kTop=5, kMaxQueryLen=4095, TVZ_IX_SUB_LOG2=14, kWqRegPost=4096, kWqSlots=512,
                 kWqMaxLen=512, kWqGs=4, kWqRows=16384, kLdsPerWorkgroup=160 * 1024, kIxPostPad=64 + 512)
PW, BLOCK, WAVES, SLOTS = (CONSTANTS[n] for n in ("kIxPW", "kIxBlock", "kIxWaves", "kIxSlots"))
REG = CONSTANTS["kWqRegPost"]
SUB_LOG2 = CONSTANTS["TVZ_IX_SUB_LOG2"]
SUB_ROWS = 1 << SUB_LOG2
KTH_NEVER = 2**31 - 1

# runs = ((min_match, k, cap), ..); excl = one video id per query or None; max_len = the max_query_len the batch is run
# with (None: its longest query); pad_to = empty queries appended up to this batch size (2,048 queries give every query
# ONE block over all sub-indexes: index_subs_per_block); truncated = queries that may have more hits than cap;
# forms = None (all that apply) or ("match",): the unfused lookup only
Batch = namedtuple("Batch", "queries runs excl max_len pad_to truncated forms")
# edits = ({row: keys}, [(video id, keys)]) upserted after the first round (tests.index_build_cases.edit), or None;
# again = the batches that run once more after the edits; n_sub / bucket = what the handle must report
Case = namedtuple("Case", "name corpus batches reaches edits again n_sub bucket")


def batch(queries, runs, excl=None, max_len=None, pad_to=0, truncated=(), forms=None):
    return Batch([np.ascontiguousarray(q, dtype=np.float64) for q in queries], tuple(runs), excl, max_len, pad_to,
                 frozenset(truncated), forms)


# ---- what decides the path, restated --------------------------------------------------------------------------------
def n_sub(n_rows):
    return max(1, -(-n_rows // SUB_ROWS))


def owner_wave(i):
    """the wave of the block kernel that owns position i of chunk 0 (position = lane * kIxWaves + wave)"""
    return i % WAVES


class _Index:
    """the postings of a corpus: canonical keys (-0.0 is 0.0) in numeric order, each with its rows ascending"""

    def __init__(self, c):
        row = np.repeat(np.arange(c.ids.size, dtype=np.int64), np.diff(c.offs))
        key = np.where(c.keys == 0.0, 0.0, c.keys)
        order = np.lexsort((row, key))
        self.key, self.row = key[order], row[order]

    def rows(self, x, sub=None):
        if np.isnan(x):
            return self.row[:0]
        x = 0.0 if x == 0.0 else x
        r = self.row[np.searchsorted(self.key, x, side="left"):np.searchsorted(self.key, x, side="right")]
        if sub is None:
            return r
        return r[np.searchsorted(r, sub << SUB_LOG2):np.searchsorted(r, (sub + 1) << SUB_LOG2)]


_INDEXES = {}


def index_of(c):
    e = _INDEXES.get(id(c.keys))
    if e is None or e[0] is not c.keys:
        e = _INDEXES[id(c.keys)] = (c.keys, _Index(c))
    return e[1]


def list_lens(c, q, sub=0):
    """postings of every query position in one sub-index (e_len)"""
    ix = index_of(c)
    return np.array([ix.rows(x, sub).size for x in q], dtype=np.int64)


def wave_totals(c, q, sub=0):
    """tw of the block kernel's eight waves: the postings of a wave's chunk-0 lists"""
    lens = list_lens(c, q[:BLOCK], sub)
    return [int(lens[w::WAVES].sum()) for w in range(WAVES)]


def flat_total(c, q):
    """tw of the one-wave kernel (a handle of one sub-index)"""
    return int(list_lens(c, q, 0).sum())


def list_starts(c, q, sub=0):
    """(per wave, flat): the non-empty lists as (p0, length, position) - per wave of the block kernel (chunk 0), and in
    the one-wave kernel's flat space"""
    lens = list_lens(c, q, sub)
    per_wave = []
    for w in range(WAVES):
        p0, lists = 0, []
        for i in range(w, min(len(q), BLOCK), WAVES):
            if lens[i]:
                lists.append((p0, int(lens[i]), i))
            p0 += int(lens[i])
        per_wave.append(lists)
    p0, flat = 0, []
    for i in range(len(q)):
        if lens[i]:
            flat.append((p0, int(lens[i]), i))
        p0 += int(lens[i])
    return per_wave, flat


def touches(c, q, sub=0):
    """postings per row of one sub-index (local row numbers), dead or excluded rows included: what pass A sees"""
    ix = index_of(c)
    t = np.zeros(SUB_ROWS, dtype=np.int64)
    for x in q:
        np.add.at(t, ix.rows(x, sub) - (sub << SUB_LOG2), 1)
    return t


def candidates(c, q, mm, sub=0):
    """rows with a candidate slot: seen at least once for min_match 1, at least twice otherwise"""
    return int((touches(c, q, sub) >= (1 if mm == 1 else 2)).sum())


def expected(c, q, mm, excl=None, sorted_unique=True):
    """the oracle's hits of one query: [(video_id, count, kth)] in row order"""
    from oracle import oracle
    cnt, kth = oracle.match_kth_csr(np.asarray(q, dtype=np.float64), c.offs, c.keys, mm, sorted_unique=sorted_unique)
    r = np.flatnonzero(cnt >= mm)
    if excl is not None:
        r = r[c.ids[r] != excl]
    return list(zip(c.ids[r].tolist(), cnt[r].tolist(), kth[r].tolist()))


def expected_many(c, queries, mm, excl=None):
    """`expected` of many queries (the oracle is C behind ctypes: a few threads share the work of a large batch)"""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle
    oracle.lib()
    jobs = [(q, None if excl is None else excl[i]) for i, q in enumerate(queries)]
    if len(jobs) < 64:
        return [expected(c, q, mm, x) if len(q) else [] for q, x in jobs]
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda j: expected(c, j[0], mm, j[1]) if len(j[0]) else [], jobs))


def kth_bins(hits):
    """the histogram the fused top-k keeps of a query's hits: bins 0..62 exact, bin 63 = "63 or later" """
    h = [0] * CONSTANTS["kIxTkBins"]
    for _, _, kth in hits:
        h[min(kth, CONSTANTS["kIxTkBins"] - 1)] += 1
    return h


def tk_trace(c, q, mm, k):
    """(tk_before, bound) of every part of a one-sub-index lookup with hits to keep, as ix_tk_keep decides (no dead or
    excluded rows), up to and including the first part whose keepers do not fit (tk_before + bound > kIxTkCap): what
    the reduction leaves behind it is not restated."""
    from oracle import oracle
    cnt, kth = oracle.match_kth_csr(np.asarray(q, dtype=np.float64), c.offs, c.keys, mm, sorted_unique=True)
    cand = np.flatnonzero(touches(c, q, 0)[:c.ids.size] >= (1 if mm == 1 else 2))
    bins, cap = CONSTANTS["kIxTkBins"], CONSTANTS["kIxTkCap"]
    kh, tk_n, bmax, out = [0] * bins, 0, 1 << 30, []
    for lo in range(0, cand.size, SLOTS):
        part = cand[lo:lo + SLOTS]
        offered = [int(kth[r]) for r in part if cnt[r] >= mm and kth[r] <= bmax]
        for x in offered:
            if x < bins - 1:
                kh[x] += 1
        if not offered:
            continue
        run, bfirst = 0, bins
        for b in range(bins - 1):
            run += kh[b]
            if run >= k:
                bfirst = b
                break
        bound = len(offered)
        if bfirst < bins - 1:
            bound = min(run, bound)
            bmax = min(bmax, bfirst)
        out.append((tk_n, bound))
        if tk_n + bound > cap:
            break
        tk_n += sum(1 for x in offered if x <= bmax)
    return out


def ix_lds_bytes(L, nsb, topk):
    """IxLds::each: the dynamic LDS of the block kernel for L positions and nsb sub-indexes per block"""
    L, nsb = max(L, 1), (nsb + 1) & ~1
    words = SUB_ROWS // 32
    b = words * 4 * 2 + SLOTS * 4 + SLOTS * 8 + CONSTANTS["kIxCache"] * 4 + WAVES * 64 * 8 + WAVES * (PW // 32) * 4
    if topk:
        b += CONSTANTS["kIxTkCap"] * 8 + CONSTANTS["kIxTkBins"] * 4 + 2 * 4
    b += (L + 1) * 4 + SLOTS * 2 + words * 2 + L * nsb * 2
    return b + 16


def pair_fits(max_len, subs):
    """launch_index_topk: two queries per block only if the LDS of both leaves four blocks on a CU"""
    return ix_lds_bytes(2 * max(max_len, 1), subs, True) + 256 <= CONSTANTS["kLdsPerWorkgroup"] // 4


def unfused_groups(Q, subs):
    """index_subs_per_block + launch_index: blocks per query of the unfused lookup (the LDS bound never binds for the
    lengths used here)"""
    groups = min(subs, max(1, -(-2048 // max(Q, 1))))
    spb = -(-subs // max(groups, 1))
    return -(-subs // spb)


def fused_usable(Q, subs, max_len, mm, k):
    """index_topk_usable: the lookup keeps the top-k itself"""
    return 1 <= mm <= CONSTANTS["kTop"] and 1 <= k <= CONSTANTS["kIxTkMaxK"] and Q >= 1 and \
        max_len <= CONSTANTS["kMaxQueryLen"] and unfused_groups(Q, subs) == 1


def wave_usable(c_rows, subs, bucket, max_len, mm, k):
    return subs == 1 and bucket and c_rows <= CONSTANTS["kWqRows"] and max_len <= CONSTANTS["kWqMaxLen"] and \
        1 <= mm <= CONSTANTS["kTop"] and k <= CONSTANTS["kIxTkMaxK"]


def drop_tail(c, q, form, sub=0):
    """The corpus without the postings of q's lists that lie beyond the cached range - per wave of the block kernel
    ("block": beyond kIxPW) or of the one-wave kernel's flat space ("wave": beyond kWqRegPost) - taking a list's rows
    in ascending order.  -> (corpus, postings dropped)."""
    ix = index_of(c)
    per_wave, flat = list_starts(c, q, sub)
    limit = PW if form == "block" else REG
    lists = [x for w in per_wave for x in w] if form == "block" else flat
    gone = set()
    for p0, ln, i in lists:
        first = max(0, min(limit - p0, ln))
        x = 0.0 if q[i] == 0.0 else q[i]
        for r in ix.rows(q[i], sub)[first:]:
            gone.add((int(r), float(x)))
    row = np.repeat(np.arange(c.ids.size, dtype=np.int64), np.diff(c.offs))
    keep = np.fromiter(((int(r), float(x)) not in gone for r, x in zip(row, c.keys)), dtype=bool, count=row.size)
    offs, keys = _pairs_to_csr(c.ids.size, row[keep], c.keys[keep])
    return Corpus(c.ids, offs, keys), len(gone)


# ---- building blocks --------------------------------------------------------------------------------------------------
def KEY(j):
    return 1000.0 + 0.125 * j            # exact in float64


def ABSENT(j):
    return 1000.0 + 0.125 * np.asarray(j) + 0.0625      # between the keys: in no row


OWN0 = 5.0e6                             # row r's own key OWN0 + r: in no query (no row is empty)


class _Maker:
    def __init__(self, n_rows, seed, own=True):
        self.n, self.rng, self.next = n_rows, np.random.default_rng(seed), 0
        self.rows, self.keys = [], []
        if own:
            self.rows.append(np.arange(n_rows, dtype=np.int64))
            self.keys.append(OWN0 + np.arange(n_rows, dtype=np.float64))

    def key(self, rows, value=None):
        """a new key held by `rows`"""
        if value is None:
            value = KEY(self.next)
            self.next += 1
        rows = np.asarray(rows, dtype=np.int64)
        assert rows.size == 0 or (0 <= rows.min() and rows.max() < self.n and np.unique(rows).size == rows.size)
        self.rows.append(rows)
        self.keys.append(np.full(rows.size, value, dtype=np.float64))
        return float(value)

    def sample(self, lo, hi, n):
        return np.sort(self.rng.choice(np.arange(lo, hi), size=n, replace=False))

    def corpus(self, ids=None):
        offs, keys = _pairs_to_csr(self.n, np.concatenate(self.rows), np.concatenate(self.keys))
        ids = np.arange(1, self.n + 1, dtype=np.int32) if ids is None else np.asarray(ids, dtype=np.int32)
        for a in (ids, offs, keys):
            a.setflags(write=False)
        return Corpus(ids, offs, keys)


def _query(n, at):
    """n positions of keys that are in no row, but for at = {position: key}"""
    q = ABSENT(np.arange(n, dtype=np.float64))
    for i, x in at.items():
        assert 0 <= i < n
        q[i] = x
    return q


# ---- cases 1, 2, 10: the per-wave posting cache ---------------------------------------------------------------------
# A variant = the lists of its waves in lane order, (length, decisive).  A decisive list holds rows that hold NOTHING
# else of the query but the list's min_match - 1 base keys, which sit at positions 0, 1, 2, 4 (other waves, before the
# list): every one of its postings turns a miss into a hit whose kth is the list's position.
CACHE_VARIANTS = {
    "t511": {3: [(300, 0), (200, 0), (11, 1)]},
    "t512": {3: [(300, 0), (200, 0), (12, 1)]},
    "t513": {3: [(300, 0), (200, 0), (13, 1)]},                 # straddles: twelve cached, one walked again
    "single": {3: [(520, 1)]},                                 # p0 = 0, one list longer than the cache
    "straddle": {3: [(450, 0), (100, 1)]},
    "at512": {3: [(300, 0), (212, 0), (40, 1)]},                # p0 == kIxPW: no list-start bit, first = 0
    "beyond": {3: [(300, 0), (212, 0), (30, 0), (40, 1)]},      # p0 > kIxPW
    "two_over": {3: [(500, 0), (30, 1)], 5: [(512, 0), (25, 1)]},
}
CACHE_TAILS = ("t513", "single", "straddle", "at512", "beyond", "two_over")
BASE_POS = ((0, 1, 2, 4), (6, 7, 8, 9))     # of a query's first and second decisive list
CACHE_LEN = 300                          # positions of a variant's query (two of them fit one block's LDS)


class _CacheMaker:
    """rows [row0, row0 + fill) hold the filler lists, the rows behind them the decisive ones"""

    def __init__(self, mk, row0, fill, dec):
        self.mk, self.row0, self.fill, self.dec = mk, row0, fill, dec
        self.fillers, self.variants = {}, {}

    def filler(self, n):
        if n not in self.fillers:
            self.fillers[n] = self.mk.key(self.mk.sample(self.row0, self.row0 + self.fill, n))
        return self.fillers[n]

    def make(self, names, extra=None):
        for name in names:
            used, waves = np.zeros(0, dtype=np.int64), {}
            for w, lists in CACHE_VARIANTS[name].items():
                out = []
                for n, decisive in lists:
                    if not decisive:
                        out.append((self.filler(n), None))
                        continue
                    free = np.setdiff1d(np.arange(self.row0 + self.fill, self.row0 + self.fill + self.dec), used)
                    rows = np.sort(self.mk.rng.choice(free, size=n, replace=False))
                    used = np.concatenate([used, rows])
                    out.append((self.mk.key(rows), [self.mk.key(rows) for _ in range(4)]))
                waves[w] = out
            self.variants[name] = waves
        self.small = [self.mk.key(self.mk.sample(self.row0, self.row0 + self.fill, n)) for n in (1, 2, 3, 4, 2, 1)]
        self.extra = extra or {}

    def query(self, name, mm):
        at, decisive = {}, 0
        for w, lists in sorted(self.variants[name].items()):
            for j, (key, base) in enumerate(lists):
                at[w + WAVES * (1 + j)] = key            # (lane 1 onwards: behind every base position)
                if base is not None:
                    for t in range(mm - 1):
                        at[BASE_POS[decisive][t]] = base[t]
                    decisive += 1
        for j, key in enumerate(self.small):             # short lists in the waves that stay under the cache
            at[(6, 7, 14, 15, 22, 23)[j] + WAVES * 20] = key
        assert not set(at) & set(self.extra)
        at.update(self.extra)
        return _query(CACHE_LEN, at)


@functools.lru_cache(maxsize=None)
def _cache_corpus():
    mk = _Maker(2000, 101)
    cm = _CacheMaker(mk, 0, 1400, 600)
    cm.make(list(CACHE_VARIANTS))
    return mk.corpus(), cm


def _case_wave_cache():
    c, cm = _cache_corpus()
    names = list(CACHE_VARIANTS)
    batches = [batch([cm.query(v, mm) for v in names], [(mm, 16, 2000), (mm, 64, 2000)]) for mm in (1, 2, 3, 5)]
    reaches = dict(wave_totals=[511, 512, 513], straddle=PW, p0_equal=PW, p0_beyond=PW, single_list=520, waves_over=2,
                   tails=[(b, names.index(v)) for b in range(4) for v in CACHE_TAILS], tail_form="block")
    return Case("wave_cache", c, batches, reaches, None, (), 1, True)


def _case_wave_cache_sub1():
    rows = SUB_ROWS + 2000
    mk = _Maker(rows, 102)
    cm = _CacheMaker(mk, SUB_ROWS, 1400, 600)
    edge = [mk.key([SUB_ROWS - 1, SUB_ROWS]) for _ in range(5)]          # both sides of the boundary: hits at every mm
    cm.make(["t513", "single", "at512", "two_over"],
            extra={206 + WAVES * t: edge[t] for t in range(5)})
    seen = set()
    # every list key also has three postings in sub-index 0: the waves' tables are used there, and must be left clean
    for key in list(cm.fillers.values()) + [key for v in cm.variants.values() for lists in v.values() for key, _ in lists]:
        if key not in seen:
            mk.key(mk.sample(0, SUB_ROWS - 1, 3), value=key)
            seen.add(key)
    c = mk.corpus()
    names = ["t513", "single", "at512", "two_over"]
    batches = [batch([cm.query(v, mm) for v in names], [(mm, 16, 2048)], pad_to=2048) for mm in (1, 2, 3, 5)]
    reaches = dict(sub1_over_sub0_under=True, boundary_rows_hit=True,
                   tails=[(b, q) for b in range(4) for q in range(4)], tail_form="block", tail_sub=1)
    return Case("wave_cache_sub1", c, batches, reaches, None, (), 2, False)


def _case_pair():
    c, cm = _cache_corpus()
    batches = []
    for mm in (2, 5):
        over3, over5 = cm.query("straddle", mm), _shift_wave(cm.query("at512", mm), 2)
        q300 = cm.query("t513", mm)
        nine = [cm.query("beyond", mm), np.zeros(0), over3, cm.query("t512", mm)[:7], over5, q300, cm.query("single", mm),
                np.zeros(0), cm.query("two_over", mm)]
        batches += [batch([over3, over5], [(mm, 16, 2000)]),
                    batch([q300, q300.copy(), np.zeros(0)], [(mm, 16, 2000)]),
                    batch(nine, [(mm, 16, 2000), (mm, 64, 2000)]),
                    batch([over3, over5], [(mm, 16, 2000)], max_len=PAIR_MAX_LEN),
                    batch([over3, over5], [(mm, 16, 2000)], max_len=PAIR_MAX_LEN + 1)]
    reaches = dict(pair_sizes=[2, 3, 9], sum_crosses_block=True, empty_query=True, neighbours_over=(3, 5),
                   pair_limit=PAIR_MAX_LEN)
    return Case("pair", c, batches, reaches, None, (), 1, True)


PAIR_MAX_LEN = max(n for n in range(1, 1024) if pair_fits(n, 1))


def _shift_wave(q, by):
    """the query with every position moved `by` places back (its lists change wave by `by`)"""
    return np.concatenate([ABSENT(np.arange(5000, 5000 + by, dtype=np.float64)), q])[:len(q) + by]


# ---- case 3: trips of pass A and pass B ------------------------------------------------------------------------------
# (192 and 384: the three- and six-step trips of pass A, which the other totals do not reach)
TRIP_TOTALS = (1, 63, 64, 65, 192, 255, 256, 257, 384, 448, 449, 512)


def _case_trips():
    mk = _Maker(1200, 103)
    qs = {1: [], 2: []}
    for t in TRIP_TOTALS:
        parts = [t] if t == 1 else [t // 2, t - t // 2]
        keys = [mk.key(mk.sample(0, 1200, n)) for n in parts]
        at = {2 + WAVES * (1 + j): x for j, x in enumerate(keys)}                # wave 2
        qs[1].append(_query(120, at))
        at.update({6 + WAVES * (3 + j): x for j, x in enumerate(keys)})          # the same keys again in wave 6: count 2
        qs[2].append(_query(120, at))
    batches = [batch(qs[mm], [(mm, 16, 1200)]) for mm in (1, 2)]
    return Case("trips", mk.corpus(), batches, dict(wave_totals=list(TRIP_TOTALS)), None, (), 1, True)


# ---- case 4: chunks of query positions -------------------------------------------------------------------------------
CHUNK_LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4094, 4095)


def _case_chunks():
    mk = _Maker(300, 104)
    big = 7                                                  # the row of kMaxQueryLen keys
    full = np.array([mk.key([big]) for _ in range(CONSTANTS["kMaxQueryLen"])])
    first, second, last = mk.key([20, 21, 22]), mk.key([20, 21, 40]), mk.key([20, 22, 41])

    def q(n):
        at = {}
        if n > 1:
            at[0] = first
        if n > BLOCK + 1:
            at[BLOCK] = second                               # the first position of the second chunk
        if n:
            at[n - 1] = last
        return _query(n, at)

    short = [q(n) for n in CHUNK_LENGTHS if n <= BLOCK]
    longer = [q(n) for n in CHUNK_LENGTHS if n > BLOCK]
    every = full.copy()                                      # matches at every position: count 4,095
    late = np.concatenate([ABSENT(np.arange(4091, dtype=np.float64)), full[100:104]])       # kth 4,094 at min_match 4
    over = np.concatenate([ABSENT(np.arange(4092, dtype=np.float64)), [first, second, last, full[5]]])    # 4,096
    runs = [(mm, 16, 300) for mm in (1, 2, 3, 4)]
    batches = [batch(short, runs), batch(longer + [every, late], runs), batch([over, q(9)], runs)]
    reaches = dict(lengths=list(CHUNK_LENGTHS), full_count=4095, late_kth=4094, long_query=4096)
    return Case("chunks", mk.corpus(), batches, reaches, None, (), 1, True)


# ---- case 5: parts of candidate slots ---------------------------------------------------------------------------------
PART_SIZES = (511, 512, 513, 1024, 1025)


def _case_parts():
    mk = _Maker(2000, 105)
    qs, excl, hit_rows = [], [], {}
    for n in PART_SIZES:
        cand = mk.sample(0, 2000, n)
        ranks = sorted({0, 511, 512, 1023, 1024} & set(range(n)) | set(mk.rng.choice(n, size=20, replace=False).tolist()))
        hits = cand[ranks]
        qs.append(np.array([mk.key(cand), mk.key(cand), mk.key(hits), mk.key(hits), mk.key(hits)]))
        excl.append(int(cand[512 if n > 512 else 0]) + 1)    # the id on slot 0 of part 2 (of part 1 where there is one)
        hit_rows[n] = cand
    c = mk.corpus()
    dead = int(hit_rows[1025][512])                          # slot 0 of part 2: replaced, so dead in the index
    edits = ({dead: np.array([qs[4][0], qs[4][1], OWN0 + dead])}, [])
    batches = [batch(qs, [(mm, 16, 2000) for mm in (1, 2, 3, 4, 5)] + [(2, 64, 2000)]),
               batch(qs, [(2, 16, 2000), (3, 16, 2000)], excl=excl),
               batch(qs, [(2, 16, 600)], truncated=(3, 4))]
    reaches = dict(candidates=list(PART_SIZES), part_edges_hit=True, non_hits_in_part2=True, excluded_slot0=True,
                   dead_slot0=dead)
    return Case("parts", c, batches, reaches, edits, (0,), 1, True)


# ---- cases 6, 7: the fused top-k's histogram and kept list ----------------------------------------------------------
def _kth_query(mk, pool, mm, spec, n, common):
    """rows taken from `pool` (a list, used up) whose FIRST match is at the given positions: spec = [(position, rows)]"""
    at = {0: common} if mm == 2 else {}
    for pos, cnt in spec:
        rows = [pool.pop() for _ in range(cnt)]
        at[pos] = mk.key(sorted(rows))
    return _query(n, at), at


def _case_kth_bins():
    n_rows = 1200
    mk = _Maker(n_rows, 106)
    common = mk.key(np.arange(n_rows))                       # held by every row: position 0 of the min_match 2 queries
    pool = mk.rng.permutation(n_rows).tolist()
    batches, facts = [], []
    for mm in (1, 2):
        # (the rows of a min_match 1 query are used by no min_match 2 query: `pool` hands every row out once)
        for k in (1, 16, 64):
            edge, _ = _kth_query(mk, pool, mm, [(61, 2), (62, 2), (63, 2), (64, 2), (200, 2)], 260, common)
            exact, _ = _kth_query(mk, pool, mm, ([(5, k - 1)] if k > 1 else []) + [(62, 1), (63, 3), (64, 3), (200, 3)],
                                  260, common)
            none, _ = _kth_query(mk, pool, mm, ([(10, k - 1)] if k > 1 else []) + [(63, 8), (70, 8), (200, 8)], 260, common)
            late, at = _kth_query(mk, pool, mm, [(70, 12), (63, 3), (130, 20)], 260, common)
            late[90] = mk.key(index_rows_of(mk, at[70])[::2])            # every other row of the tie at 70: count + 1
            batches.append(batch([edge, exact, none, late], [(mm, k, n_rows)]))
            facts.append((mm, k))
    ids = np.random.default_rng(7).permutation(n_rows).astype(np.int32) + 1
    reaches = dict(kth_values=[61, 62, 63, 64, 200], runs=facts)
    return Case("kth_bins", mk.corpus(ids), batches, reaches, None, (), 1, True)


def index_rows_of(mk, value):
    """the rows a maker has given key `value` so far"""
    return np.concatenate([r for r, k in zip(mk.rows, mk.keys) if k.size and k[0] == value])


KEPT_SUMS = (127, 128, 129)


def _case_kept_list():
    n_rows = 1500
    mk = _Maker(n_rows, 107)
    two_parts = []
    for total in KEPT_SUMS:                                  # 600 candidates = two parts; 100 hits in the first
        cand = mk.sample(0, n_rows, 600)
        ranks = np.concatenate([mk.rng.choice(SLOTS, size=100, replace=False),
                                SLOTS + mk.rng.choice(600 - SLOTS, size=total - 100, replace=False)])
        two_parts.append(_query(40, {0: mk.key(cand), 1: mk.key(cand), 2: mk.key(cand[np.sort(ranks)])}))
    ties = {n: _query(40, {0: mk.key(mk.sample(0, n_rows, n))}) for n in (64, 65, 127, 128, 129, 300)}
    batches = [batch(two_parts, [(3, 16, n_rows)]),
               batch([ties[n] for n in (127, 128, 129, 300)], [(1, 16, n_rows)]),
               batch([ties[n] for n in (64, 65, 129)], [(1, 64, n_rows)])]
    ids = np.random.default_rng(8).permutation(n_rows).astype(np.int32) + 1
    reaches = dict(kept_sums=list(KEPT_SUMS), tie_sets=[127, 128, 129, 300], k64_ties=[64, 65, 129])
    return Case("kept_list", mk.corpus(ids), batches, reaches, None, (), 1, True)


# ---- case 8: slot modes ---------------------------------------------------------------------------------------------
MODE_POS_LONG = (7, 14, 21, 28, 35, 42, 100, 205, 310, 515, 530, 599)       # waves 7, 6, 5, .. and a second chunk
MODE_POS_SHORT = (7, 14, 21, 28, 35, 42, 100, 113, 126, 139, 150, 199)


def _case_modes():
    mk = _Maker(300, 108)
    held = {j: [] for j in range(12)}                        # match position j -> rows
    counts = {}
    r = 0
    for cnt in range(0, 13):
        for _ in range(4):
            for j in mk.rng.choice(12, size=cnt, replace=False).tolist():
                held[j].append(r)
            counts[r] = cnt
            r += 1
    for cnt in range(6, 13):                                 # the LARGEST positions and one small one: walked last or
        take = list(range(12 - cnt + 1, 12)) + [0]           # by another wave, it displaces an entry of the five
        for j in take:
            held[j].append(r)
        counts[r] = cnt
        r += 1
    keys = [mk.key(sorted(held[j])) for j in range(12)]
    long_q = _query(600, dict(zip(MODE_POS_LONG, keys)))
    short_q = _query(200, dict(zip(MODE_POS_SHORT, keys)))
    runs = [(mm, 16, 300) for mm in range(1, 7)]
    reaches = dict(match_counts=list(range(0, 13)), min_matches=list(range(1, 7)))
    return Case("modes", mk.corpus(), [batch([long_q, short_q[:100]], runs), batch([short_q, short_q[::-1].copy()], runs)],
                reaches, None, (), 1, True)


# ---- case 9: video ids and key values -------------------------------------------------------------------------------
INT32_MAX = 2**31 - 1
TINY = 5e-324


def _case_ids_and_keys():
    n_rows = 200
    mk = _Maker(n_rows, 109)
    k1 = mk.key([0, 1, 2, 3, 4])
    k2, k3 = mk.key(np.arange(10, 60)), mk.key(np.arange(10, 60, 2))
    mk.key([0, 3], value=0.0)
    mk.key([1], value=TINY)
    mk.key([2, 5], value=np.inf)
    mk.key([3, 6], value=-np.inf)
    kd = mk.key([100, 101])                                  # after the edits: in the directory, every row dead
    k5 = mk.key([102])
    ids = np.arange(1000, 1000 + n_rows, dtype=np.int64)
    ids[0], ids[1], ids[2] = 0, 1, INT32_MAX
    ids[10:60] = 7                                           # one id owns fifty rows
    q0 = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, TINY, k1, k1, k2, np.nan, k3])
    q1 = np.array([0.0, k2, k2, k2, -0.0])                   # a repeated key: every occurrence counts
    q2 = np.array([kd, k1, kd, k5])
    runs = [(mm, 16, n_rows) for mm in (1, 2, 3)] + [(1, 64, n_rows)]
    batches = [batch([q0, q1, q2], runs), batch([q0, q1, q2], runs[:3], excl=[0, 7, INT32_MAX])]
    edits = ({100: np.array([k5, OWN0 + 100]), 101: np.array([OWN0 + 101])}, [])
    reaches = dict(ids=[0, 1, INT32_MAX], id_rows=50, dead_key=kd)
    return Case("ids_and_keys", mk.corpus(ids), batches, reaches, edits, (0, 1), 1, True)


# ---- cases 11 - 13: the one-wave kernel ---------------------------------------------------------------------------------
# (name: flat position p0 of the decisive list, its length, the length of the filler lists in front of it)
WQ_VARIANTS = {"t4095": (4084, 11, 32), "t4096": (4084, 12, 32), "t4097": (4084, 13, 32), "at4096": (4096, 40, 32),
               "first_batch": (4050, 100, 128), "t9000": (8960, 40, 32), "t256": (250, 6, 32), "t257": (250, 7, 32)}
WQ_TAILS = ("t4097", "at4096", "first_batch", "t9000")


def _case_wq_registers():
    n_rows = 2000
    mk = _Maker(n_rows, 110)
    fill = {}                                                # (length, n-th of that length) -> key

    def filler(n, j):
        if (n, j) not in fill:
            fill[(n, j)] = mk.key(mk.sample(0, 1400, n))
        return fill[(n, j)]

    dec = {}
    for name, (p0, ln, g) in WQ_VARIANTS.items():
        rows = mk.sample(1400, n_rows, ln)
        dec[name] = (mk.key(rows), [mk.key(rows) for _ in range(4)])

    def query(name, mm):
        p0, ln, g = WQ_VARIANTS[name]
        key, base = dec[name]
        lists = list(base[:mm - 1])                          # the base lists come first: positions 0 .. min_match - 2
        rest = p0 - (mm - 1) * ln
        lists += [filler(g, j) for j in range(rest // g)]
        if rest % g:
            lists.append(filler(rest % g, 0))
        lists.append(key)
        return _query(len(lists) + 3, {i: x for i, x in enumerate(lists)})

    names = list(WQ_VARIANTS)
    batches = [batch([query(v, mm) for v in names], [(mm, 16, n_rows)]) for mm in (1, 2, 3, 5)]
    reaches = dict(flat_totals=[4095, 4096, 4097, 256, 257], straddle=REG, p0_equal=REG, second_batch=64, first_batch=64,
                   about=9000, tails=[(b, names.index(v)) for b in range(4) for v in WQ_TAILS], tail_form="wave")
    return Case("wq_registers", mk.corpus(), batches, reaches, None, (), 1, True)


WQ_LENGTHS = (64, 65, 128, 129, 192, 193, 256, 257, 320, 511, 512)


def _case_wq_chunks():
    mk = _Maker(50, 111)
    last, second_round = mk.key([3, 4]), mk.key([3, 9])
    qs = [_query(n, {n - 1: last, **({256: second_round} if n > 257 else {})}) for n in WQ_LENGTHS]
    qs.append(_query(257, {256: second_round}))              # the second round's only position holds the only match
    return Case("wq_chunks", mk.corpus(), [batch(qs, [(1, 16, 50), (2, 16, 50)])],
                dict(lengths=list(WQ_LENGTHS)), None, (), 1, True)


def _case_wq_rows(n_rows):
    mk = _Maker(n_rows, 112)
    a, b = mk.key(sorted({0, n_rows - 1})), mk.key(sorted({0, n_rows - 1}))
    q = np.array([a, ABSENT(1), b, OWN0 + min(5, n_rows - 1)])
    name = "wq_rows" if n_rows > 1 else "wq_rows_one"
    return Case(name, mk.corpus(), [batch([q, q[:1]], [(1, 16, 16), (2, 16, 16)])], dict(rows=n_rows), None, (), 1, True)


# ---- case 14: groups of sub-indexes in the unfused lookup ------------------------------------------------------------
GROUP_Q = (1, 1024, 2047, 2048, 2049)
GROUP_CAP = 64


def _case_groups(subs):
    n_rows = {2: SUB_ROWS + 4000, 3: 33000}[subs]
    mk = _Maker(n_rows, 113 + subs, own=False)
    rng = mk.rng
    # rows of 1-3 keys from an alphabet of 12,000: a key has ~5 rows, spread over the sub-indexes
    lens = rng.integers(1, 4, size=n_rows)
    row = np.repeat(np.arange(n_rows, dtype=np.int64), lens)
    mk.rows.append(row)
    mk.keys.append(KEY(rng.integers(0, 12000, size=row.size)))
    c = mk.corpus()
    qs = [KEY(rng.integers(0, 12000, size=int(rng.integers(1, 4)))) for _ in range(max(GROUP_Q))]
    qs[0] = c.keys[c.offs[n_rows - 1]:c.offs[n_rows]].copy()             # the last row
    qs[1] = np.array([c.keys[c.offs[SUB_ROWS - 1]], c.keys[c.offs[SUB_ROWS]]])          # both sides of a boundary
    batches = [batch(qs[:Q], [(1, 16, GROUP_CAP), (2, 16, GROUP_CAP)], forms=("match",)) for Q in GROUP_Q]
    reaches = dict(groups=[unfused_groups(Q, subs) for Q in GROUP_Q], subs=subs)
    return Case("groups" if subs == 3 else "groups_two", c, batches, reaches, None, (), subs, False)


_MAKERS = {
    "wave_cache": _case_wave_cache, "wave_cache_sub1": _case_wave_cache_sub1, "trips": _case_trips, "chunks": _case_chunks,
    "parts": _case_parts, "kth_bins": _case_kth_bins, "kept_list": _case_kept_list, "modes": _case_modes,
    "ids_and_keys": _case_ids_and_keys, "pair": _case_pair, "wq_registers": _case_wq_registers,
    "wq_chunks": _case_wq_chunks, "wq_rows": lambda: _case_wq_rows(CONSTANTS["kWqRows"]),
    "wq_rows_one": lambda: _case_wq_rows(1), "groups": lambda: _case_groups(3), "groups_two": lambda: _case_groups(2),
}
NAMES = tuple(_MAKERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case `name`, made once (seeded: the same arrays every time).  Read-only."""
    return _MAKERS[name]()


class _Cases(dict):
    def __missing__(self, name):
        self[name] = case(name)
        return self[name]


CASES = _Cases()                          # name -> Case, made on first use (CASES[name]); NAMES lists them


def edited(cs):
    """the corpus of a case after its edits"""
    return edit(cs.corpus, cs.edits[0], cs.edits[1]) if cs.edits else cs.corpus


def padded(b):
    """the batch's queries with its empty padding"""
    return list(b.queries) + [np.zeros(0)] * max(0, b.pad_to - len(b.queries))


def batch_max_len(b):
    return b.max_len if b.max_len is not None else max([len(q) for q in b.queries] + [0])
