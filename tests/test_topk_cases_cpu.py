"""The case tables of the top-k edge tests (tests/topk_cases.py), checked without a GPU: the thresholds they assume are
the ones in the sources (tvz_topk_kernels.h and the launchers in tvz_match.hip), every branch they name is reached by
some case, the generator is deterministic, and the reference (tests/topk_ref.py) agrees with the CPU stand-in of the
sharded service (tests/fakes.py)."""
import os
import re

import numpy as np
import torch

from oracle import oracle
from tests import topk_cases as cases, topk_ref as ref
from tests.fakes import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tvidz_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([^;]+);", text)
    assert m, name
    expr = m.group(1)
    assert re.fullmatch(r"[\d\s*+\-/()]+", expr), (name, expr)
    return int(eval(expr))                                  # digits and arithmetic only (checked above)


def test_assumed_thresholds_are_the_ones_in_the_sources():
    kern, host, common = _src("tvz_topk_kernels.h"), _src("tvz_match.hip"), _src("tvz_common.h") + _src("tvz_match_kernels.h")
    C = cases.CONSTANTS
    for name in ("kSelMin", "kSelSmallK", "kSortCap", "kSelBins", "kWsE", "kWsK"):
        assert _const(kern, name) == C[name], name
    assert _const(host, "kTopkFallbackBlocks") == C["kTopkFallbackBlocks"]
    assert _const(common, "kBlock") == C["kBlock"]
    # the sorted merge's bounds and the one-wave merge's, as launch_topk_lists states them
    assert re.search(r"form == kTopkMerge && n_lists <= kMsMaxLists && k <= kMsMaxK", host)
    assert (_const(kern, "kMsMaxLists"), _const(kern, "kMsMaxK")) == (C["merge_sorted_max_lists"], C["merge_sorted_max_k"])
    assert re.search(r"form == kTopkMerge && k <= kWsK && \(int64_t\)n_lists \* k <= kWsMax", host)
    assert re.search(r"enum TopkForm : int32_t \{ kTopkPlain = 0, kTopkShard = 1, kTopkMerge = 2, kTopkPair = 3 \};", kern)
    assert re.search(r"constexpr int kWsMax = 64 \* kWsE;", kern)
    # launch_topk_local: the one-wave kernel in front for k <= kWsK, the smaller select kernel for k <= kSelSmallK
    assert re.search(r"if \(d_flags && k <= kWsK\)", host)
    assert re.search(r"if \(k <= kSelSmallK\)\s+hipLaunchKernelGGL\(ts_topk_select_kernel<4 \* kSelSmallK>", host)
    assert re.search(r"ts_topk_select_kernel<kSortCap>", host)
    # the one-wave kernel's size classes and its `fits` bound; the select kernels' histogram bound and reduction
    assert "if (n <= 64 * 4)" in kern and "else if (n <= 64 * 8)" in kern and "if (n > kWsMax)" in kern
    assert "fits = upto <= 64u;" in kern and "if (n > kSelMin)" in kern
    assert "if (pos > kSelCap - kSelChunk)" in kern and "if (pos == kSortCap) sort_and_keep(key, cnt, pos, k);" in kern
    assert cases.SEL_BINS_PER_THREAD == 17 and cases.WS_BINS_PER_LANE == 66


def _all_lists(rows, queries, mm=1):
    ids, offs, keys = (np.array([v for v, _ in rows], dtype=np.int32),
                       np.concatenate([[0], np.cumsum([len(t) for _, t in rows])]).astype(np.int64),
                       np.array([x for _, t in rows for x in t], dtype=np.float64))
    out = []
    for q in queries:
        cnt, kth = oracle.match_kth_csr(np.asarray(q, dtype=np.float64), offs, keys, mm)
        out.append([(int(ids[c]), int(cnt[c]), int(kth[c])) for c in range(len(ids)) if cnt[c] >= mm])
    return out


def test_every_named_branch_is_reached_by_some_case():
    seen = set()
    # a. tvz_topk_shard, b. tvz_topk on one list
    for k in cases.SHARD_KS:
        _, lists, reported = cases.shard_batch(k)
        for lst, n in zip(lists, reported):
            seen.update(cases.local_branches(lst[:min(max(n, 0), cases.SHARD_CAP)], k, flags=False))
    # b. several lists
    for R, cap, k in cases.TOPK_LISTS:
        _, lists, ns = cases.topk_lists_batch(R, cap, k)
        for per, n in zip(lists, ns):
            looked = [lst[:cap if n is None else min(max(n[r], 0), cap)] for r, lst in enumerate(per)]
            seen.update(cases.lists_branches(looked, k, 0))
    # c. merges
    for R in cases.MERGE_SORTED_R:
        for k in cases.MERGE_SORTED_K:
            for Q in cases.MERGE_SORTED_Q:
                seen.update(cases.lists_branches([b[:k] for b in cases.merge_query(R, k, 0)[0]], k, 2, Q))
    styles = {fam: set() for fam in ("merge_sorted", "wave", "block")}
    for R, k in ((16, 64), (3, 5)) + cases.MERGE_WAVE + cases.MERGE_BLOCK:
        for q in range(cases.MERGE_Q if R * k > 1024 or R > 16 else max(cases.MERGE_SORTED_Q)):
            blocks, st = cases.merge_query(R, k, q)
            br = cases.lists_branches([b[:k] for b in blocks], k, 2)
            seen.update(br)
            styles[br[0].split("/")[0].split("<")[0]].add(st)
    for fam, st in styles.items():          # every row style and every totals style, in all three families
        assert {s[0] for s in st} == set(cases.ROW_STYLES) and {s[1] for s in st} == set(cases.TOTAL_STYLES), fam
    # d. the sweeps' lists (from the oracle, not from the construction)
    rows, queries, lengths = cases.match_corpus()
    lists = _all_lists(rows, queries)
    assert [len(x) for x in lists] == lengths
    for lst in lists:
        for k in cases.MATCH_KS:
            seen.update(cases.local_branches(lst, k, flags=True))
    rows, queries, lengths = cases.match_big_corpus()
    assert sorted(q for q, n in enumerate(lengths) if n > cases.WS_MAX) == sorted(cases.MATCH_BIG_LONG)
    seen.update(cases.grid_branches(len(queries), cases.MATCH_BIG_LONG))
    # e. the pair merge
    main, delta, queries, lengths = cases.pair_corpus()
    li, ld = _all_lists(main, queries), _all_lists(delta, queries)
    assert [(len(a), len(b)) for a, b in zip(li, ld)] == lengths
    for (name, _, _, k, cap), a, b in zip(cases.PAIR_CASES, li, ld):
        assert len(a) <= cap and len(b) <= cap
        seen.update(cases._wave_branches(ref.best(a, k) + ref.best(b, k), k, 3))
        if len(a) + len(b) > cap:
            seen.add("mode3/sum-over-cap")
    assert set(cases.BRANCHES) <= seen, sorted(set(cases.BRANCHES) - seen)


def test_the_generator_is_deterministic():
    for args in (("a", 513, 16, ("ramp", 33), "dup", "shuffle"), ("b", 2049, 257, ("distinct", 0), "pad", "shuffle"),
                 ("c", 65, 1, ("far",), "pad", "asc")):
        assert cases.make_list(*args) == cases.make_list(*args)
    assert cases.make_list("a", 513, 16, ("one", 7), "dup", "shuffle") != cases.make_list("b", 513, 16, ("one", 7), "dup", "shuffle")
    # the three orders hold the same entries
    a, d, s = (cases.make_list("x", 1025, 64, ("ramp", 67), "pad", o) for o in cases.ORDERS)
    assert sorted(a) == sorted(d) == sorted(s) and a != d and a != s
    assert [i for i, e in enumerate(a) if e[0] < 0] == [i for i, e in enumerate(s) if e[0] < 0]   # padding stays scattered
    assert cases.merge_query(9, 5, 11) == cases.merge_query(9, 5, 11)
    assert cases.match_corpus() == cases.match_corpus()


def test_reference_agrees_with_the_fake_backend():
    fake = OracleBackend()
    k, cap = 16, 600
    # what both express: the fake knows neither padding inside a list nor a refused query's INT32_MIN
    small = [c for c in cases.shard_cases() if c[1] <= cap and c[3] != "pad" and (c[4] is None or c[4] >= 0)]
    names, lists, reported = cases.shard_batch(k, small)
    reported[3] = cap + 9                                   # one truncated list (the fake negates its total too)
    hits = torch.zeros((len(lists), cap, 3), dtype=torch.int32)
    for q, lst in enumerate(lists):
        if lst:
            hits[q, :len(lst)] = torch.tensor(lst, dtype=torch.int64).to(torch.int32)
    got = fake.topk_shard(hits, torch.tensor(reported, dtype=torch.int32), k)
    for q, lst in enumerate(lists):
        full = lst + [(0, 0, 0)] * (cap - len(lst))
        assert [tuple(r) for r in got[q].tolist()] == ref.select(full, reported[q], cap, k, True), names[q]
    # merges, without the styles the fake does not express (saturation)
    R, k, Q = 5, 4, 35
    per_q = [cases.merge_query(R, k, q) for q in range(Q)]
    g = torch.tensor([[per_q[q][0][r] for q in range(Q)] for r in range(R)], dtype=torch.int64).to(torch.int32)
    rows, totals = fake.topk_merge(g, k)
    n = 0
    for q in range(Q):
        if per_q[q][1][1] in ("saturated", "saturated-negative", "refused-alone", "refused-among"):
            continue
        n += 1
        exp_rows, exp_total = ref.merge(per_q[q][0], k)
        assert [tuple(r) for r in rows[q].tolist()] == exp_rows and int(totals[q]) == exp_total, per_q[q][1]
    assert n >= 10
