"""Case tables of the top-k edge tests (tests/test_topk_edges_gpu.py runs them on the GPU, tests/test_topk_cases_cpu.py
checks the tables themselves on any machine).

The tables are data: list lengths, k, cap, R, Q, the kth pattern, the value pattern and the entry order.  Every case
names the branches it is built to reach; the names come from a restatement, below, of the dispatch in tvz_match.hip
(launch_topk_local, launch_topk_lists, launch_topk_pair) and of the paths inside the kernels of tvz_topk_kernels.h
that depend on the input alone (histogram or direct sort, mid-stream reduction, the one-wave kernel's E and `fits`,
the threshold bin's place in the walk).  `mode` 0..3 here is the kernels' TopkForm: plain, shard, merge, pair.  The
thresholds assumed here are in CONSTANTS; test_topk_cases_cpu.py compares them with the sources, so a changed
threshold fails there instead of silently moving the edges away from the cases."""
import zlib

import numpy as np

from tests import topk_ref as ref

NEVER = ref.KTH_NEVER
INT32_MAX, INT32_MIN = ref.INT32_MAX, ref.INT32_MIN

CONSTANTS = {
    "kSelMin": 64,                  # lists up to this long skip the histogram
    "kSelSmallK": 256,              # k up to this: ts_topk_select_kernel<1024>, above: <kSortCap>
    "kSortCap": 2048,               # ts_topk_kernel's buffer; the larger select kernel's too
    "kSelBins": 4098,               # kth -1 .. 4095 exact, the last bin shared
    "kWsE": 16,                     # entries per lane of the one-wave kernel's largest body: 1024 per query
    "kWsK": 64,                     # the one-wave kernel's largest k
    "kTopkFallbackBlocks": 1280,    # grid of the block kernel behind the one-wave kernel
    "kBlock": 256,
    "merge_sorted_max_lists": 16,   # launch_topk_lists: the merge form && n_lists <= kMsMaxLists && k <= kMsMaxK
    "merge_sorted_max_k": 64,
}
C = CONSTANTS
WS_MAX = 64 * C["kWsE"]
LAST_BIN = C["kSelBins"] - 1
SEL_BINS_PER_THREAD = -(-C["kSelBins"] // C["kBlock"])                  # 17
WS_BINS_PER_LANE = 2 * (((C["kSelBins"] + 1) // 2 + 63) // 64)           # 66

ORDERS = ("asc", "desc", "shuffle")


# ---------------------------------------------------------------- the dispatch, restated
def sel_bin(kth):
    return min(kth + 1, LAST_BIN)


def _threshold(valid, need):
    """(B, upto): the first bin whose inclusive prefix reaches `need`, and that prefix; (LAST_BIN, all) if none does."""
    hist = {}
    for _, _, kth in valid:
        b = kth + 1 if kth < LAST_BIN - 1 else LAST_BIN      # sel_bin, inline
        hist[b] = hist.get(b, 0) + 1
    cum = 0
    for b in sorted(hist):
        cum += hist[b]
        if cum >= need:
            return b, cum
    return LAST_BIN, cum


def _wave_branches(prefix, k, mode):
    n = len(prefix)
    E = 4 if n <= 64 * 4 else 8 if n <= 64 * 8 else C["kWsE"]
    valid = [e for e in prefix if e[0] >= 0]
    base = f"wave/mode{mode}/E={E}"
    if not valid:
        return [base + "/empty"]
    B, upto = _threshold(valid, min(k, len(valid)))
    out = [base + ("/fits" if upto <= 64 else "/!fits")]
    if upto in (64, 65):
        out.append(f"wave/upto={upto}")
    out.append("wave/walk/low-half" if B % 2 == 0 else "wave/walk/high-half")
    if B % WS_BINS_PER_LANE in (0, WS_BINS_PER_LANE - 1):
        out.append("wave/walk/lane-edge")
    if B == LAST_BIN:
        out.append("wave/walk/shared-bin")
    return out


def _select_branches(prefix, k):
    selcap = 4 * C["kSelSmallK"] if k <= C["kSelSmallK"] else C["kSortCap"]
    base = f"select<{selcap}>"
    n = len(prefix)
    out = []
    limit = LAST_BIN
    if n <= C["kSelMin"]:
        out.append(base + "/direct")
    else:
        out.append(base + "/hist")
        valid = [e for e in prefix if e[0] >= 0]
        if len(valid) >= k:
            limit, _ = _threshold(valid, k)
            if limit == LAST_BIN:
                out.append("select/walk/shared-bin")
            elif limit == LAST_BIN - 1:
                out.append("select/walk/last-exact-bin")
            if limit % SEL_BINS_PER_THREAD in (0, SEL_BINS_PER_THREAD - 1):
                out.append("select/walk/thread-edge")
            if limit % (4 * SEL_BINS_PER_THREAD) in (0, 4 * SEL_BINS_PER_THREAD - 1):
                out.append("select/walk/lane-edge")
        else:
            out.append("select/walk/fewer-than-k")
    chunk, pos = selcap // 2, 0
    for j0 in range(0, n, chunk):
        pos += sum(1 for e in prefix[j0:j0 + chunk] if e[0] >= 0 and (limit == LAST_BIN or e[2] < limit))
        if pos > selcap - chunk:
            out.append(base + "/midstream-reduce")
            pos = min(pos, k)
    return out


def local_branches(prefix, k, flags, mode=1):
    """launch_topk_local for one query: `prefix` = the entries the kernels look at (the first min(max(n, 0), cap)),
    flags = the call carries a flag array (tvz_match_topk; tvz_topk and tvz_topk_shard do not)."""
    out = []
    if flags and k <= C["kWsK"]:
        if len(prefix) <= WS_MAX:
            return _wave_branches(prefix, k, mode)
        out.append("flagged")
    elif flags:
        out.append("no-wave/k>64")
    return out + _select_branches(prefix, k)


def lists_branches(per_list, k, mode, Q=1):
    """launch_topk_lists for one query: per_list = the entries looked at in every list (mode 2: the k rows of a block)."""
    R = len(per_list)
    if mode == 2 and R <= C["merge_sorted_max_lists"] and k <= C["merge_sorted_max_k"]:
        G = 1
        while G < R:
            G *= 2
        out = [f"merge_sorted<{G}>"]
        if (3 * k) % 12:
            out.append("merge_sorted/copy-tail")
        if (Q * G) % 64:
            out.append("merge_sorted/dead-groups")
        if G != R:
            out.append("merge_sorted/dead-ranks")
        return out
    if mode == 2 and k <= C["kWsK"] and R * k <= WS_MAX:
        out = _wave_branches([e for lst in per_list for e in lst], k, 2)
        if R > 64:
            out.append("wave/mode2/two-totals-per-lane")
        return out
    base = f"block/mode{mode}"
    out, pos, left = [base], 0, sum(len(lst) for lst in per_list)
    for lst in per_list:
        j = 0
        while j < len(lst):
            m = min(len(lst) - j, C["kSortCap"] - pos)
            pos, j, left = pos + m, j + m, left - m
            if pos == C["kSortCap"]:
                out.append(base + ("/midstream-reduce" if left else "/fills-on-last-entry"))
                pos = min(pos, k)
    return out


def grid_branches(Q, flagged_queries):
    """The flagged follow-up's grid: min(Q, kTopkFallbackBlocks) blocks that stride over the batch."""
    return ["flagged/grid-stride"] if any(q >= C["kTopkFallbackBlocks"] for q in flagged_queries) and \
        Q > C["kTopkFallbackBlocks"] else []


# every branch some case must reach (test_topk_cases_cpu.py checks it)
BRANCHES = (
    # a. tvz_topk_shard / b. tvz_topk on one list: the select kernels alone
    "select<1024>/direct", "select<1024>/hist", "select<1024>/midstream-reduce",
    "select<2048>/direct", "select<2048>/hist", "select<2048>/midstream-reduce",
    "select/walk/thread-edge", "select/walk/lane-edge", "select/walk/last-exact-bin", "select/walk/shared-bin",
    "select/walk/fewer-than-k",
    # b. tvz_topk on several lists
    "block/mode0", "block/mode0/midstream-reduce", "block/mode0/fills-on-last-entry",
    # c. tvz_topk_merge
    "merge_sorted<1>", "merge_sorted<2>", "merge_sorted<4>", "merge_sorted<8>", "merge_sorted<16>",
    "merge_sorted/copy-tail", "merge_sorted/dead-groups", "merge_sorted/dead-ranks",
    "wave/mode2/E=4/fits", "wave/mode2/E=8/fits", "wave/mode2/E=16/fits",
    "wave/mode2/E=4/!fits", "wave/mode2/E=8/!fits", "wave/mode2/E=16/!fits",
    "wave/mode2/E=4/empty", "wave/mode2/two-totals-per-lane",
    "block/mode2", "block/mode2/midstream-reduce",
    # d. tvz_match_topk's sweeps: the one-wave kernel in mode 1 and the flagged hand-over
    "wave/mode1/E=4/empty", "wave/mode1/E=4/fits", "wave/mode1/E=8/fits", "wave/mode1/E=16/fits",
    "wave/mode1/E=4/!fits", "wave/mode1/E=8/!fits", "wave/mode1/E=16/!fits",
    "wave/upto=64", "wave/upto=65", "wave/walk/low-half", "wave/walk/high-half", "wave/walk/lane-edge",
    "flagged", "flagged/grid-stride", "no-wave/k>64",
    # e. the pair merge behind a delta table
    "wave/mode3/E=4/fits", "wave/mode3/E=4/!fits", "mode3/sum-over-cap",
)


# ---------------------------------------------------------------- hand-made hit lists
def case_rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _kth_values(n, k, pat):
    i = np.arange(n, dtype=np.int64)
    kind = pat[0]
    if kind == "distinct":
        return i + pat[1]
    if kind == "one":
        return np.full(n, pat[1], dtype=np.int64)
    if kind == "ramp":                                       # the k-th best entry lands exactly at kth = t
        t = pat[1]
        m = 1 if k - 1 <= t else (k - 1) // t + 1            # m-fold ties where k - 1 distinct values do not fit below t
        return np.maximum(0, t + (i - (k - 1)) // m)
    if kind == "far":                                        # all in the shared bin, which must still be ordered exactly
        return np.where(i % 3 == 0, 100000, np.where(i % 3 == 1, NEVER - 1, 4096 + i))
    raise ValueError(pat)


def make_list(name, n, k, kth_pat, vals, order):
    """n entries (video_id, count, kth) as plain int tuples.  vals: "uniq" (distinct ids, 0 and 2^31 - 1 among them),
    "dup" (few ids: pairs equal in (kth, id) that differ in count, and fully identical entries), "pad" (uniq with
    padding entries scattered through the list, in every order)."""
    rng = case_rng(f"{name}/{n}/{k}/{kth_pat}/{vals}")       # not the order: the three orders hold the same entries
    kth = _kth_values(n, k, kth_pat)
    if vals == "dup":
        pool = np.concatenate([[0, INT32_MAX], rng.integers(1, INT32_MAX, size=max(1, n // 3))])
        vid = pool[rng.integers(0, pool.size, size=n)]
        cnt = np.array([1, 2, 4095, INT32_MAX])[rng.integers(0, 4, size=n)]
    else:
        vid = rng.choice(np.arange(1, 1 << 20), size=n, replace=False).astype(np.int64) * 2047
        if n >= 2:
            vid[rng.integers(0, n)] = 0
            vid[(np.flatnonzero(vid == 0)[0] + 1) % n] = INT32_MAX
        cnt = np.where(rng.random(n) < 0.5, rng.integers(1, INT32_MAX, size=n),
                       np.array([1, 4095, INT32_MAX])[rng.integers(0, 3, size=n)])
    ent = sorted(zip(vid.tolist(), cnt.tolist(), kth.tolist()), key=ref.order_key)
    pads = []
    if vals == "pad" and n >= 4:
        at = sorted(rng.choice(n, size=max(1, n // 8), replace=False).tolist())
        pads = [(p, ref.PAD if j % 2 == 0 else (-1, 9, 0)) for j, p in enumerate(at)]   # a padding entry's other words are free
        ent = ent[:n - len(pads)]
    if order == "desc":
        ent.reverse()
    elif order == "shuffle":
        ent = [ent[j] for j in case_rng(name + "/shuffle").permutation(len(ent)).tolist()]
    for p, e in pads:
        ent.insert(p, e)
    return ent


# ---- a. tvz_topk_shard: one launch per k over all of these lists
SHARD_CAP = 5003
SHARD_KS = (1, 16, 64, 255, 256, 257, 1024)
SHARD_LENGTHS = (0, 1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, SHARD_CAP)
# the k-th entry's kth: thread and lane boundaries of the select kernel's walk (17 bins per thread, 68 per lane), the
# one-wave kernel's 66 bins per lane, the last exact bins and the shared one
RAMP_TARGETS = (15, 16, 17, 33, 34, 64, 65, 66, 67, 68, 4094, 4095, 4096, 4097)


def shard_cases():
    """[(name, n_entries, kth pattern, value pattern, reported)]: reported = what hits_n says (None: n_entries)."""
    t = []
    for n in SHARD_LENGTHS:
        t.append((f"distinct/{n}", n, ("distinct", 0), "uniq", None))
        t.append((f"one/{n}", n, ("one", 7), "dup", None))
    for tgt in RAMP_TARGETS:
        for n in (513, 2049):
            t.append((f"ramp{tgt}/{n}", n, ("ramp", tgt), "dup", None))
    for tgt in (16, 17, 67, 68, 4095, 4096):
        t.append((f"ramp{tgt}/65", 65, ("ramp", tgt), "uniq", None))
    for n in (64, 65, 1025, SHARD_CAP):
        t.append((f"far/{n}", n, ("far",), "pad", None))
    for n in (65, 1024, 2049):
        t.append((f"padded/{n}", n, ("distinct", 3), "pad", None))
    t.append(("over-by-one", SHARD_CAP, ("distinct", 0), "uniq", SHARD_CAP + 1))
    t.append(("over-max", SHARD_CAP, ("one", 2), "dup", INT32_MAX))
    t.append(("refused", 100, ("distinct", 0), "uniq", INT32_MIN))
    t.append(("zero", 100, ("distinct", 0), "uniq", 0))
    t.append(("prefix", 100, ("distinct", 0), "uniq", 10))
    return t


def shard_batch(k, cases=None):
    """-> (names, lists, reported): every case in the three orders."""
    names, lists, reported = [], [], []
    for name, n, kth_pat, vals, rep in (shard_cases() if cases is None else cases):
        for order in ORDERS:
            names.append(f"{name}/{order}")
            lists.append(make_list(name, n, k, kth_pat, vals, order))
            reported.append(n if rep is None else rep)
    return names, lists, reported


# ---- b. tvz_topk (mode 0)
TOPK_ONE_LIST_KS = (16, 257)
TOPK_FULL_LENGTHS = (65, 513, 2049)                 # without lists_n: every list is `cap` entries
# (R, cap, k): 2400 entries (the buffer fills mid-stream), exactly 2048 (it fills on the last entry), 2100 with k = cap
TOPK_LISTS = ((4, 600, 16), (4, 600, 600), (2, 1024, 1024), (3, 700, 700), (3, 700, 64))


def topk_lists_batch(R, cap, k):
    """-> (names, lists[q][r], lists_n[q][r] or None per query)."""
    names, lists, ns = [], [], []
    for style, kth_pat, vals in (("distinct", ("distinct", 0), "pad"), ("one", ("one", 5), "dup"),
                                 ("ramp", ("ramp", 4095), "dup")):
        for order in ORDERS:
            flat = make_list(f"lists/{style}/{R}x{cap}", R * cap, k, kth_pat, vals, order)
            per = [flat[r * cap:(r + 1) * cap] for r in range(R)]
            names.append(f"{style}/{order}/full")
            lists.append(per)
            ns.append(None)
            names.append(f"{style}/{order}/ragged")
            lists.append(per)
            ns.append([(0, cap + 5, cap, 1, cap - 1)[(r + len(names)) % 5] for r in range(R)])
    return names, lists, ns


# ---- c. tvz_topk_merge
MERGE_SORTED_R = (1, 2, 3, 5, 7, 9, 15, 16)
MERGE_SORTED_K = (1, 2, 4, 5, 63, 64)
MERGE_SORTED_Q = (1, 63, 64, 65)
MERGE_WAVE = ((20, 12), (17, 16), (17, 60), (64, 16), (100, 10))      # E = 4, 8, 16, exactly 1024 entries, R > 64
MERGE_BLOCK = ((17, 61), (17, 64), (40, 64), (3, 700), (2, 1024))     # just past 1024, past 2048, k > 64 at small R
MERGE_Q = 37                                                          # every row style x totals style, and a part block
ROW_STYLES = ("spread", "one-kth", "same-entry", "sparse", "empty")
EDGE_KTHS = (63, 64, 65, 66, 130, 131, 4094, 4095, 4096)
TOTAL_STYLES = ("plain", "one-negative", "refused-alone", "refused-among", "saturated", "saturated-negative", "zero")


def merge_query(R, k, q):
    """The R blocks of query q, each k sorted rows + (-1, n, NEVER), and the styles they were made in."""
    s = q + 7 * R + k                                    # so a batch of one query is not always the same style
    rs, ts = ROW_STYLES[s % 5], TOTAL_STYLES[(s // 5) % 7]
    rng = case_rng(f"merge/{R}/{k}/{q}")
    blocks = []
    who = s % R
    same = None
    for r in range(R):
        m = {"spread": k, "one-kth": k, "same-entry": k, "sparse": (r + q) % 2, "empty": 0}[rs]
        if ts in ("refused-alone", "zero") or (ts == "refused-among" and r == who):
            m = 0
        if rs == "same-entry" and same is not None:
            ent = same[:m]
        else:
            if rs == "one-kth":
                kth = np.full(m, 3)
            elif rs == "sparse":                             # few entries: the threshold bin is one of these, at the edges
                kth = np.array(EDGE_KTHS)[rng.integers(0, len(EDGE_KTHS), size=m)]     # of a lane's 66 bins and a word's halves
            else:
                kth = rng.integers(0, 5000, size=m)
            vid = rng.integers(0, 40, size=m) if rs == "one-kth" else rng.integers(0, INT32_MAX, size=m, endpoint=True)
            cnt = np.array([1, 2, 4095, INT32_MAX])[rng.integers(0, 4, size=m)]
            ent = list(zip(vid.tolist(), cnt.tolist(), kth.tolist()))
            if rs == "same-entry":
                same = ent
        n = m + r % 3
        if ts == "one-negative" and r == who:
            n = -max(n, 1)
        elif ts in ("refused-alone", "refused-among") and r == who:
            n = INT32_MIN
        elif ts == "refused-alone" or ts == "zero":
            n = 0
        elif ts in ("saturated", "saturated-negative"):
            n = -INT32_MAX if ts == "saturated-negative" and r == who else INT32_MAX
        blocks.append(ref.best(ent, k) + [(-1, n, NEVER)])
    return blocks, (rs, ts)


# ---- d. tvz_match_topk's sweeps: a corpus whose hit lists have a chosen length and kth pattern
MATCH_QLEN = 48
MATCH_CAP = 2048
MATCH_KS = (1, 16, 64, 65)
# (name, [(kth, hits at it)]): "spread" lists walk over the query's positions; the ties put every hit at one position
MATCH_LISTS = (
    [(f"spread/{n}", "spread", n) for n in (0, 1, 64, 65, 256, 257, 512, 513, 1024, 1025, 1500)] +
    [(f"tie/{n}", [(9, n)], n) for n in (200, 400, 900)] +
    [("upto64", [(0, 64), (5, 30)], 94), ("upto65", [(0, 65), (5, 30)], 95),
     ("upto64-high-half", [(0, 10), (1, 54), (40, 20)], 84), ("upto65-late", [(0, 10), (46, 55)], 65)])
MATCH_BIG_Q = 1300
MATCH_BIG_LONG = {3: 1100, 1290: 1300}               # the only queries of the big batch with more than 1024 hits


def query_keys(i):
    return [(i * 64 + p) / 4.0 for p in range(MATCH_QLEN)]


def _hit_rows(i, positions, first_id):
    """One corpus row per hit of query i: the key at `positions[j]`, every other row with a later key of the same
    query behind it (count 2).  At min_match = 1 the hit's kth is that position."""
    keys, rows = query_keys(i), []
    for j, p in enumerate(positions):
        ts = [keys[p]]
        if j % 2 and p + 1 + j % 3 < MATCH_QLEN:
            ts.append(keys[p + 1 + j % 3])
        rows.append((first_id + j, ts))
    return rows


def match_corpus():
    """-> (rows, queries, intended hit counts) of MATCH_LISTS, query i = list i."""
    rows, queries, lengths = [], [], []
    for i, (name, pat, n) in enumerate(MATCH_LISTS):
        if pat == "spread":
            positions = [j % MATCH_QLEN for j in range(n)]
        else:
            positions = [kth for kth, m in pat for _ in range(m)]
        assert len(positions) == n
        rows += _hit_rows(i, positions, len(rows) + 1)
        queries.append(query_keys(i))
        lengths.append(n)
    order = case_rng("match_corpus").permutation(len(rows)).tolist()
    return [rows[j] for j in order], queries, lengths


def match_big_corpus():
    """Q = 1300 queries of which two have more than 1024 hits and every seventh a few."""
    rows, queries, lengths = [], [], []
    for i in range(MATCH_BIG_Q):
        n = MATCH_BIG_LONG.get(i, 3 if i % 7 == 0 else 0)
        rows += _hit_rows(i, [j % MATCH_QLEN for j in range(n)], len(rows) + 1)
        queries.append(query_keys(i))
        lengths.append(n)
    order = case_rng("match_big_corpus").permutation(len(rows)).tolist()
    return [rows[j] for j in order], queries, lengths


# ---- e. the pair merge (mode 3): hits from the index and from the delta table
PAIR_CASES = (
    # (name, index side [(kth, hits)], delta side, k, cap)
    ("interleaved", [(p, 3) for p in range(0, 40, 2)], [(p, 3) for p in range(1, 40, 2)], 16, 4096),
    ("interleaved-k64", [(p, 3) for p in range(0, 40, 2)], [(p, 3) for p in range(1, 40, 2)], 64, 4096),
    ("tied-both-sides", [(4, 70)], [(4, 66)], 64, 4096),
    ("index-only", [(p, 2) for p in range(30)], [], 16, 4096),
    ("delta-only", [], [(p, 2) for p in range(30)], 16, 4096),
    ("sum-over-cap", [(p, 4) for p in range(10)], [(p, 3) for p in range(10)], 16, 50),   # 40 <= cap, 30 <= cap, 70 > cap
)


def pair_corpus():
    """-> (index rows, delta rows, queries, [(index hits, delta hits)]): query i = PAIR_CASES[i]."""
    main, delta, queries, lengths = [], [], [], []
    for i, (name, ipat, dpat, k, cap) in enumerate(PAIR_CASES):
        ip = [kth for kth, m in ipat for _ in range(m)]
        dp = [kth for kth, m in dpat for _ in range(m)]
        main += _hit_rows(i, ip, 1000 * (i + 1))
        delta += _hit_rows(i, dp, 1000 * (i + 1) + 500)
        queries.append(query_keys(i))
        lengths.append((len(ip), len(dp)))
    main += [(90000 + j, [1e6 + j, 1e6 + j + 0.5]) for j in range(300)]      # rows nobody asks for
    return main, delta, queries, lengths
