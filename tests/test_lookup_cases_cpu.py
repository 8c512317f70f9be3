"""The threshold cases of the index lookup (tests/lookup_cases.py), checked without a GPU: the constants and the rules the
restatements assume are the ones in the sources, every case reaches what its `reaches` says - computed from the case's
data by the restatements - the verdicts that are meant to hang on postings beyond a cached range do (the oracle's answer
changes when those postings are dropped), no query has more hits than the cap it runs with, the generators are
deterministic and every row is sorted and without repeats."""
import os
import re

import numpy as np
import pytest

from tests import lookup_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tvidz_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


KERNELS, WAVE, HANDLE, MATCHK, WAVEH, MATCH = (_read(n) for n in (
    "tvz_index_kernels.h", "tvz_index_wave_kernels.h", "tvz_handle.h", "tvz_match_kernels.h", "tvz_wave.h", "tvz_match.hip"))
FLAT = {n: " ".join(s.split()) for n, s in (("kernels", KERNELS), ("wave", WAVE), ("match", MATCH))}
C = cases.CONSTANTS
PW, REG, SLOTS = cases.PW, cases.REG, cases.SLOTS


def _const(src, name):
    m = re.search(r"constexpr\s+(?:int|int64_t)\s+" + name + r"\s*=\s*([0-9* +]+);", src)
    assert m, name
    return eval(m.group(1), {"__builtins__": {}})            # digits, *, + and blanks only (the pattern)


def _define(src, name):
    m = re.search(r"#define " + name + r" (\d+)", src)
    assert m, name
    return int(m.group(1))


def test_assumed_constants_are_the_ones_in_the_sources():
    block, cache = _define(KERNELS, "TVZ_IX_BLOCK"), _define(KERNELS, "TVZ_IX_CACHE")
    slot_bits = _define(KERNELS, "TVZ_IX_SLOT_BITS")
    for line in ("constexpr int kIxBlock = TVZ_IX_BLOCK;", "constexpr int kIxWaves = kIxBlock / 64;",
                 "constexpr int kIxSlots = 1 << kIxSlotBits;", "constexpr int kIxCache = TVZ_IX_CACHE;",
                 "constexpr int kIxPW = kIxCache / kIxWaves;", "constexpr int kSubLog2 = TVZ_IX_SUB_LOG2;"):
        assert line in KERNELS, line
    assert block == C["kIxBlock"] == 512 and block // 64 == C["kIxWaves"] == 8
    assert cache == C["kIxCache"] == 4096 and cache // (block // 64) == C["kIxPW"] == 512
    assert 1 << slot_bits == C["kIxSlots"] == 512
    assert _define(KERNELS, "TVZ_IX_SUB_LOG2") == C["TVZ_IX_SUB_LOG2"] == 14
    assert _const(KERNELS, "kIxTkCap") == C["kIxTkCap"] == 128
    assert _const(KERNELS, "kIxTkBins") == C["kIxTkBins"] == 64
    assert _const(KERNELS, "kIxTkMaxK") == C["kIxTkMaxK"] == 64
    assert _const(KERNELS, "kIxPostPad") == C["kIxPostPad"] == 576
    assert _const(WAVEH, "kTop") == C["kTop"] == 5
    assert _const(MATCHK, "kMaxQueryLen") == C["kMaxQueryLen"] == 4095
    assert _const(HANDLE, "kLdsPerWorkgroup") == C["kLdsPerWorkgroup"] == 163840
    for line in ("constexpr int kWqMaxLen = kWqChunks * 64;", "constexpr int kWqRegPost = kWqSteps * 64;",
                 "constexpr int kWqGs = TVZ_WQ_GS;", "constexpr int kWqRows = 1 << kWqRowsLog2;"):
        assert line in WAVE, line
    assert _const(WAVE, "kWqChunks") * 64 == C["kWqMaxLen"] == 512
    assert _const(WAVE, "kWqSteps") * 64 == C["kWqRegPost"] == 4096
    assert _define(WAVE, "TVZ_WQ_GS") == C["kWqGs"] == 4
    assert 1 << _const(WAVE, "kWqRowsLog2") == C["kWqRows"] == 16384
    assert _const(WAVE, "kWqSlots") == C["kWqSlots"] == 512
    # the pad behind the postings covers what the dead steps of a live group read
    assert C["kIxPostPad"] >= (C["kWqGs"] - 1) * 64 + 63


def test_the_rules_are_the_ones_restated():
    """The lines that the restatements mirror, as text: a change of rule fails here first."""
    for line in (
        # the IxLds::each carve (ix_lds_bytes)
        "f(bm1, kIxWords); f(bm2, kIxWords); f(tcnt, kIxSlots); f(ttop, kIxSlots); f(cache, kIxCache);",
        "f(lst, kIxWaves * 64); f(lbits, kIxWaves * kIxLW);",
        "if (topk) { f(tkb, kIxTkCap); f(kh, kIxTkBins); f(tk_n, 2); }",
        "f(e_cur, L + 1); f(elist, kIxSlots); f(rank, kIxWords); f(e_len, L * (size_t)nsb);",
        "return lds_carve_bytes<IxLds>((size_t)(max_len > 0 ? max_len : 1), ix_nsb_padded(spb), topk) + 16;",
        "__host__ __device__ inline int ix_nsb_padded(int spb) { return (spb + 1) & ~1; }",
        "uint32_t *bm1, *bm2;", "uint32_t *tcnt;", "unsigned long long *ttop;", "uint32_t *cache;", "uint2 *lst;",
        "uint32_t *lbits;", "unsigned long long *tkb;", "uint32_t *kh;", "uint32_t *tk_n;", "uint32_t *e_cur;",
        "uint16_t *elist;", "uint16_t *rank;", "uint16_t *e_len;",
        "constexpr int kIxWords = kSubRows / 32;", "constexpr int kIxLW = kIxPW / 32;",
        # who owns a position, and where the cache ends
        "const int i = wk.lane * kIxWaves + wk.wave;",
        "ix_walk_lists(post, lane, __ballot(first < len0), off0, len0, first, (uint32_t)(lane * kIxWaves + wave), f);",
        "const uint32_t first = p0 < (uint32_t)kIxPW ? (uint32_t)kIxPW - p0 : 0u;",
        "if (wk.p0 < (uint32_t)kIxPW) atomicOr(&wk.lbits[wk.p0 >> 5], 1u << (wk.p0 & 31u));",
        "wk.c_hi = wk.tw < (uint32_t)kIxPW ? wk.tw : (uint32_t)kIxPW;",
        "wk.n_chunks = (wk.n + kIxBlock - 1) / kIxBlock;",
        "for (uint32_t lo = 0; lo < n_cand; lo += kIxSlots) {",
        "const uint32_t *cand = min_match >= 2 ? bm2 : bm1;",
        # the fused top-k's decisions (tk_trace, kth_bins)
        "const uint32_t hincl = wave_scan_incl(lane < kIxTkBins - 1 ? kh[lane] : 0u);",
        "const unsigned long long reach = __ballot(hincl >= (uint32_t)tk_k);",
        "if (tk_before + bound <= (uint32_t)kIxTkCap) {",
        "if (kth < (uint32_t)kIxTkBins - 1u) atomicAdd(&kh[kth], 1u);",
    ):
        assert line in FLAT["kernels"], line
    for line in (
        # the one-wave kernel's flat space: lists in position order, the register range
        "const int i = (c0 + c) * 64 + lane;",
        "if (p0 < (uint32_t)kWqRegPost) atomicOr(&lbits[p0 >> 5], 1u << (p0 & 31u));",
        "const uint32_t c_hi = tw < (uint32_t)kWqRegPost ? tw : (uint32_t)kWqRegPost;",
        "const bool tail = tw > (uint32_t)kWqRegPost;",
        "for (uint32_t j0 = 0; j0 < n_lists; j0 += 64u) {",
        "const uint32_t first = (uint32_t)kWqRegPost - p0c < len ? (uint32_t)kWqRegPost - p0c : len;",
        "for (int c0 = 0; c0 < nch; c0 += 4) {",
        "for (uint32_t lo = 0; lo < n_cand; lo += kWqSlots) {",
    ):
        assert line in FLAT["wave"], line
    for line in (
        # the pair condition in launch_index_topk
        "const size_t lds2 = ix_lds_bytes(2 * one, ix.n_sub, true);",
        "const bool pair = Q >= 2 && ((Q >= 2 * kIxResidentBlocks && ix.keys.nb == 0) || force_pair) && "
        "lds2 + 256 <= (size_t)kLdsPerWorkgroup / 4 && !no_pair;",
        # index_subs_per_block, and who may keep the top-k
        "int groups = hostout ? n_sub : (int)std::min<int64_t>(n_sub, std::max<int64_t>(1, tvz::ceil_div(2048, "
        "std::max(Q, 1))));",
        "int spb = (int)tvz::ceil_div(n_sub, std::max(groups, 1));",
        "const int groups = (int)tvz::ceil_div(ix.n_sub, spb);",
        "if (index_subs_per_block(Q, ix.n_sub, max_query_len, false) != ix.n_sub) return false;",
        "if (!c->ix.valid || min_match < 1 || min_match > kTop || k < 1 || k > kIxTkMaxK || Q < 1) return false;",
        # wave_usable
        "return ix.n_sub == 1 && ix.keys.nb > 0 && ix.n_main <= kWqRows && max_query_len <= kWqMaxLen && min_match >= 1 && "
        "min_match <= kTop && k <= kIxTkMaxK;",
    ):
        assert line in FLAT["match"], line
    # what the restatements give where the sources state it: 32.5 KiB + 1.3 KiB with the top-k, 20 B per position at 8 subs
    assert cases.ix_lds_bytes(1, 2, False) == 31232 + 2048 + 8 + 4 + 16
    assert cases.ix_lds_bytes(300, 8, True) - cases.ix_lds_bytes(200, 8, True) == 100 * 20
    assert cases.ix_lds_bytes(1, 1, True) - cases.ix_lds_bytes(1, 1, False) == 1024 + 256 + 8
    assert cases.pair_fits(cases.PAIR_MAX_LEN, 1) and not cases.pair_fits(cases.PAIR_MAX_LEN + 1, 1)
    assert cases.PAIR_MAX_LEN == 382
    assert [cases.unfused_groups(Q, 3) for Q in cases.GROUP_Q] == [3, 2, 2, 1, 1]
    assert [cases.unfused_groups(Q, 2) for Q in cases.GROUP_Q] == [2, 2, 2, 1, 1]
    assert [cases.owner_wave(i) for i in (0, 7, 8, 511)] == [0, 7, 0, 7]


# ---- the cases -------------------------------------------------------------------------------------------------------
_HITS = {}


def _hits(cs, c, bi, mm, phase=0):
    """the oracle's hits of every query of a batch, each distinct (query, exclusion) computed once"""
    b = cs.batches[bi]
    keys = [(cs.name, phase, mm, b.excl[qi] if b.excl else None, q.tobytes()) for qi, q in enumerate(b.queries)]
    todo = {k: qi for qi, k in enumerate(keys) if k not in _HITS}
    _HITS.update(zip(todo, cases.expected_many(c, [b.queries[qi] for qi in todo.values()], mm, [k[3] for k in todo])))
    return [_HITS[k] for k in keys]


def _all_lists(cs, form, sub=0):
    """(batch, query, wave or -1, p0, length, position) of every non-empty list of the case"""
    for bi, b in enumerate(cs.batches):
        for qi, q in enumerate(b.queries):
            per_wave, flat = cases.list_starts(cs.corpus, q, sub)
            if form == "block":
                for w, lists in enumerate(per_wave):
                    for j, (p0, ln, i) in enumerate(lists):
                        yield bi, qi, w, j, p0, ln, i
            else:
                for j, (p0, ln, i) in enumerate(flat):
                    yield bi, qi, -1, j, p0, ln, i


@pytest.mark.parametrize("name", cases.NAMES)
def test_rows_are_sorted_and_the_generators_deterministic(name):
    cs = cases.case(name)
    c = cs.corpus
    assert c.offs[0] == 0 and c.offs[-1] == c.keys.size and c.ids.size + 1 == c.offs.size and (np.diff(c.offs) > 0).all()
    inner = np.ones(c.keys.size, dtype=bool)
    inner[c.offs[1:-1]] = False                              # (the first key of a row may be below the row before)
    assert (np.diff(c.keys)[inner[1:]] > 0).all()            # sorted, no repeats, no NaN
    assert cases.n_sub(c.ids.size) == cs.n_sub and cs.bucket == (cs.n_sub == 1)
    cases.case.cache_clear()
    cases._cache_corpus.cache_clear()
    again = cases.case(name)
    assert all((a == b).all() for a, b in zip(c, again.corpus)) and len(again.batches) == len(cs.batches)
    for b, b2 in zip(cs.batches, again.batches):
        assert b.runs == b2.runs and b.excl == b2.excl and len(b.queries) == len(b2.queries)
        assert all(np.array_equal(q, q2, equal_nan=True) for q, q2 in zip(b.queries, b2.queries))
    assert len(cs.batches[0].queries) <= 12 or name.startswith("groups")


@pytest.mark.parametrize("name", cases.NAMES)
def test_no_query_has_more_hits_than_its_cap(name):
    """(from the oracle alone) - but the queries a batch marks as truncated, which have more"""
    cs = cases.case(name)
    for phase, c in ((0, cs.corpus), (1, cases.edited(cs))) if cs.edits else ((0, cs.corpus),):
        for bi, b in enumerate(cs.batches):
            if phase and bi not in cs.again:
                continue
            for mm, k, cap in b.runs:
                for qi, h in enumerate(_hits(cs, c, bi, mm, phase)):
                    assert (len(h) > cap) == (qi in b.truncated), (name, bi, mm, qi, len(h), cap)
                assert 1 <= k <= C["kIxTkMaxK"] and cases.batch_max_len(b) >= max(len(q) for q in b.queries)


@pytest.mark.parametrize("name", ["wave_cache", "wave_cache_sub1", "wq_registers"])
def test_the_verdict_hangs_on_the_postings_beyond_the_cached_range(name):
    cs = cases.case(name)
    form, sub = cs.reaches["tail_form"], cs.reaches.get("tail_sub", 0)
    limit = PW if form == "block" else REG
    assert len(cs.reaches["tails"]) >= 16
    for bi, qi in cs.reaches["tails"]:
        b = cs.batches[bi]
        (mm, _, _), q = b.runs[0], b.queries[qi]
        cut, dropped = cases.drop_tail(cs.corpus, q, form, sub)
        assert dropped > 0
        full, less = cases.expected(cs.corpus, q, mm), cases.expected(cut, q, mm)
        lost = [h for h in full if h[0] not in {x[0] for x in less}]       # hits with them, misses without
        assert lost and len(less) < len(full), (name, bi, qi)
        # a lost hit's kth is the position of a list that reaches beyond the limit: it came from a tail posting
        per_wave, flat = cases.list_starts(cs.corpus, q, sub)
        beyond = {i for lists in (per_wave if form == "block" else [flat]) for p0, ln, i in lists if p0 + ln > limit}
        assert {h[2] for h in lost} <= beyond and any(h[1] == mm for h in lost), (name, bi, qi)


def _totals(cs, sub=0):
    return {t for b in cs.batches for q in b.queries for t in cases.wave_totals(cs.corpus, q, sub)}


def test_wave_cache_reaches_its_thresholds():
    cs = cases.case("wave_cache")
    r = cs.reaches
    assert set(r["wave_totals"]) == {PW - 1, PW, PW + 1} <= _totals(cs)
    lists = list(_all_lists(cs, "block"))
    assert any(p0 < PW < p0 + ln and p0 > 0 for _, _, _, _, p0, ln, _ in lists)              # straddles
    assert any(p0 == PW for _, _, _, _, p0, ln, _ in lists) and r["p0_equal"] == PW
    assert any(p0 > PW for _, _, _, _, p0, ln, _ in lists)
    assert any(p0 == 0 and ln == r["single_list"] > PW for _, _, _, _, p0, ln, _ in lists)
    over = [sum(t > PW for t in cases.wave_totals(cs.corpus, q)) for b in cs.batches for q in b.queries]
    assert r["waves_over"] in over and 1 in over and 0 in over
    assert sorted({b.runs[0][0] for b in cs.batches}) == [1, 2, 3, 5]
    # the one-wave kernel sees the same queries (300 positions) well inside its register range
    assert max(cases.flat_total(cs.corpus, q) for b in cs.batches for q in b.queries) < REG


def test_wave_cache_sub1_overflows_in_the_second_sub_index_only():
    cs = cases.case("wave_cache_sub1")
    assert cs.n_sub == 2 and all(b.pad_to == 2048 and cases.unfused_groups(b.pad_to, 2) == 1 for b in cs.batches)
    for bi, b in enumerate(cs.batches):
        for q in b.queries:
            t0, t1 = cases.wave_totals(cs.corpus, q, 0), cases.wave_totals(cs.corpus, q, 1)
            assert max(t0) < PW < max(t1)
            assert any(0 < a and b1 > PW for a, b1 in zip(t0, t1))        # a wave used in sub-index 0 overflows in 1
        mm = b.runs[0][0]
        for h in _hits(cs, cs.corpus, bi, mm):
            assert {int(cs.corpus.ids[cases.SUB_ROWS - 1]), int(cs.corpus.ids[cases.SUB_ROWS])} <= {x[0] for x in h}
    assert any(p0 == PW for _, _, _, _, p0, ln, _ in _all_lists(cs, "block", 1))


def test_trips_reach_every_trip_length():
    cs = cases.case("trips")
    assert set(cs.reaches["wave_totals"]) == set(cases.TRIP_TOTALS) <= _totals(cs)
    assert {(t + 63) >> 6 for t in cases.TRIP_TOTALS} == set(range(1, 9))                       # ix_pass_a_trip<1..8>
    last_group = {((t - 1) % 256 + 64) >> 6 for t in cases.TRIP_TOTALS}
    assert last_group == {1, 2, 3, 4} and max(_totals(cs)) == PW                                # pass B's 1..4-step trips


def test_chunks_reach_every_length():
    cs = cases.case("chunks")
    lens = sorted(len(q) for b in cs.batches for q in b.queries)
    assert set(cases.CHUNK_LENGTHS) <= set(lens) and lens[-1] == C["kMaxQueryLen"] + 1 == cs.reaches["long_query"]
    for n in (512, 1024, 4095):
        assert {n - 1, n, n + 1} <= set(lens)
    c = cs.corpus
    for b, qs in ((cs.batches[0], cs.batches[0].queries), (cs.batches[1], cs.batches[1].queries[:-2])):
        for q in qs:
            h1 = cases.expected(c, q, 1)
            if len(q) in cases.CHUNK_LENGTHS and len(q):
                assert max(x[2] for x in h1) == len(q) - 1                     # a hit whose only match is the last position
            if len(q) in cases.CHUNK_LENGTHS and len(q) > 513:
                assert any(x[2] == 512 for x in cases.expected(c, q, 2))       # ... the first of the second chunk
    every, late = cs.batches[1].queries[-2:]
    assert (7 + 1, 4095, 0) in cases.expected(c, every, 1) and cs.reaches["full_count"] == 4095 == 0xfff
    assert cases.expected(c, late, 4) == [(7 + 1, 4, cs.reaches["late_kth"])] and cs.reaches["late_kth"] == 4094
    assert cases.batch_max_len(cs.batches[0]) == 512 and cases.batch_max_len(cs.batches[2]) == 4096


def test_parts_reach_their_candidate_counts():
    cs = cases.case("parts")
    c, b = cs.corpus, cs.batches[0]
    for n, q, ex in zip(cases.PART_SIZES, b.queries, cs.batches[1].excl):
        for mm in (1, 2, 5):
            assert cases.candidates(c, q, mm) == n
        cand = np.flatnonzero(cases.touches(c, q)[:c.ids.size] >= 2)
        hit_ids = {h[0] for h in cases.expected(c, q, 5)}
        ranks = {int(np.searchsorted(cand, v - 1)) for v in hit_ids}           # (video id = row + 1)
        assert {0, 511, 512, 1023, 1024} & set(range(n)) <= ranks              # first and last slot of every part
        assert len(hit_ids) < n - 400                                          # candidates that are no hits at 3..5
        assert ex == c.ids[cand[SLOTS if n > SLOTS else 0]]                     # the excluded id: slot 0 of the last part
        if n >= 2 * SLOTS:
            assert any(SLOTS <= r < 2 * SLOTS for r in set(range(n)) - ranks)  # candidates of part 2 that are no hits
        assert all(len(cases.expected(c, q, mm)) == len(hit_ids) for mm in (3, 4))
    dead = cs.reaches["dead_slot0"]
    q = b.queries[4]
    cand = np.flatnonzero(cases.touches(c, q)[:c.ids.size] >= 2)
    assert cand[SLOTS] == dead and list(cs.edits[0]) == [dead]
    # after the upsert the row is a candidate of the index still (its postings are stale), and no hit at 3..5 any more
    assert (dead + 1, 5, 4) in cases.expected(c, q, 5)
    assert not [h for h in cases.expected(cases.edited(cs), q, 3) if h[0] == dead + 1]
    assert cs.batches[2].truncated == {3, 4}


def test_kth_bins_reach_the_histogram_edges():
    cs = cases.case("kth_bins")
    c = cs.corpus
    assert [(b.runs[0][0], b.runs[0][1]) for b in cs.batches] == cs.reaches["runs"]
    for bi, b in enumerate(cs.batches):
        (mm, k, _), (edge, exact, none, late) = b.runs[0], b.queries
        hs = _hits(cs, c, bi, mm)
        assert set(cs.reaches["kth_values"]) == {h[2] for h in hs[0]} == {61, 62, 63, 64, 200}
        h = cases.kth_bins(hs[1])
        assert sum(h[:62]) == k - 1 and h[62] == 1 and h[63] == 9          # exactly k at or below bin 62, the k-th IN it
        h = cases.kth_bins(hs[2])
        assert sum(h[:63]) == k - 1 and h[63] == 24                        # never k hits below 63: no bound at all
        h = cases.kth_bins(hs[3])
        assert sum(h[:63]) == 0 and h[63] == 35
        tie = [x for x in hs[3] if x[2] == 70]
        assert len(tie) == 12 and len({x[0] for x in tie}) == 12 and len({x[1] for x in tie}) == 2
        assert cases.tk_trace(c, exact, mm, k) == [(0, k)] and cases.tk_trace(c, none, mm, k) == [(0, k - 1 + 24)]


def test_kept_list_reaches_the_capacity_from_both_sides():
    cs = cases.case("kept_list")
    c, cap = cs.corpus, C["kIxTkCap"]
    sums = [sum(cases.tk_trace(c, q, 3, 16)[-1]) for q in cs.batches[0].queries]
    assert sums == cs.reaches["kept_sums"] == [cap - 1, cap, cap + 1]
    assert all(len(cases.tk_trace(c, q, 3, 16)) == 2 and cases.candidates(c, q, 3) == 600 for q in cs.batches[0].queries)
    assert [cases.tk_trace(c, q, 1, 16) for q in cs.batches[1].queries] == [[(0, n)] for n in cs.reaches["tie_sets"]]
    assert [cases.tk_trace(c, q, 1, 64) for q in cs.batches[2].queries] == [[(0, n)] for n in cs.reaches["k64_ties"]]
    for bi, b in enumerate(cs.batches):
        for h in _hits(cs, c, bi, b.runs[0][0]):
            assert len({x[2] for x in h}) == 1 and len({x[0] for x in h}) == len(h)      # one kth bin, ties by video id


def test_modes_reach_every_count_around_every_min_match():
    cs = cases.case("modes")
    c = cs.corpus
    long_q, short_q = cs.batches[0].queries[0], cs.batches[1].queries[0]
    from oracle import oracle
    for q in (long_q, short_q):
        cnt, _ = oracle.match_kth_csr(q, c.offs, c.keys, 1, sorted_unique=True)
        assert set(cs.reaches["match_counts"]) <= set(cnt.tolist())
        for mm in cs.reaches["min_matches"]:
            assert {mm - 1, mm, mm + 1} <= set(cnt.tolist())
    assert [r[0] for r in cs.batches[0].runs] == [1, 2, 3, 4, 5, 6]
    # positions on waves 7, 6, 5, .. and in the second chunk; rows whose five smallest include the LAST-walked position
    assert [cases.owner_wave(p) for p in cases.MODE_POS_LONG[:6]] == [7, 6, 5, 4, 3, 2] and max(cases.MODE_POS_LONG) >= 512
    # the same query at 5 (fused) and at 6 (count + fix-up) has hits in both
    assert cases.expected(c, long_q, 5) and cases.expected(c, long_q, 6)
    assert len(cases.expected(c, long_q, 5)) > len(cases.expected(c, long_q, 6))


def test_ids_and_keys_reach_the_odd_values():
    cs = cases.case("ids_and_keys")
    c, r = cs.corpus, cs.reaches
    assert set(r["ids"]) <= set(c.ids.tolist()) and int((c.ids == 7).sum()) == r["id_rows"]
    q0, q1, q2 = cs.batches[0].queries
    assert np.isnan(q0).sum() == 2 and np.signbit(q0[1]) and q0[1] == 0 and np.isinf(q0).sum() == 2 and cases.TINY in q0
    h = {x[0]: x for x in cases.expected(c, q0, 1)}
    # (+-0.0 both count; a NaN takes a position and matches nothing)
    assert h[0][1:] == (4, 1) and h[1][1:] == (3, 5) and h[cases.INT32_MAX][1:] == (3, 3)
    assert all(x[1] == 3 for x in cases.expected(c, q1, 3) if x[0] == 7)                        # the repeated key: 3 times
    # the dead key: two hits before the edits, none of its rows after - and the key is still in the directory
    kd = r["dead_key"]
    assert len(cases.index_of(c).rows(kd)) == 2 and len(cases.index_of(cases.edited(cs)).rows(kd)) == 0
    assert len(cases.expected(c, q2, 2)) == 2 and len(cases.expected(cases.edited(cs), q2, 2)) == 0
    assert cs.batches[1].excl == [0, 7, cases.INT32_MAX]


def test_pair_reaches_both_sides_of_the_lds_limit():
    cs = cases.case("pair")
    c, r = cs.corpus, cs.reaches
    sizes = [len(b.queries) for b in cs.batches]
    assert set(r["pair_sizes"]) == set(sizes) == {2, 3, 9}
    two = cs.batches[0].queries
    t0, t1 = cases.wave_totals(c, two[0]), cases.wave_totals(c, two[1])
    assert t0[3] > PW and t1[5] > PW and r["neighbours_over"] == (3, 5)
    b = cs.batches[1]
    assert [len(q) for q in b.queries] == [300, 300, 0] and 300 < C["kIxBlock"] < 600
    assert r["sum_crosses_block"] and r["empty_query"]
    assert any(len(q) == 0 for q in cs.batches[2].queries)
    lens = [cases.batch_max_len(b) for b in cs.batches]
    assert r["pair_limit"] in lens and r["pair_limit"] + 1 in lens
    assert cases.pair_fits(r["pair_limit"], 1) and not cases.pair_fits(r["pair_limit"] + 1, 1)
    assert all(cases.pair_fits(n, 1) for n in lens if n <= r["pair_limit"])


def test_wq_registers_reach_the_register_range():
    cs = cases.case("wq_registers")
    c, r = cs.corpus, cs.reaches
    totals = {cases.flat_total(c, q) for b in cs.batches for q in b.queries}
    assert set(r["flat_totals"]) == {REG - 1, REG, REG + 1, 256, 257} <= totals and 8500 < max(totals) < 9500
    assert all(len(q) <= C["kWqMaxLen"] for b in cs.batches for q in b.queries)
    lists = list(_all_lists(cs, "wave"))
    straddle = [j for _, _, _, j, p0, ln, _ in lists if p0 < REG < p0 + ln]
    assert any(j >= r["second_batch"] for j in straddle) and any(j < r["first_batch"] for j in straddle)
    assert any(p0 == REG and j >= 64 for _, _, _, j, p0, ln, _ in lists) and r["p0_equal"] == REG
    # 256 postings: one full group of kWqGs steps; 257: a second group with three dead steps, inside the pad
    assert (256 + 63) // 64 == C["kWqGs"] and (257 + 63) // 64 == C["kWqGs"] + 1
    assert sorted({b.runs[0][0] for b in cs.batches}) == [1, 2, 3, 5]


def test_wq_chunks_and_rows_reach_their_edges():
    cs = cases.case("wq_chunks")
    c = cs.corpus
    assert [len(q) for q in cs.batches[0].queries][:-1] == list(cases.WQ_LENGTHS) == cs.reaches["lengths"]
    # nch: the instances <1>..<4> of the first round, a second round from 257 positions
    assert {(n + 63) // 64 for n in cases.WQ_LENGTHS} == {1, 2, 3, 4, 5, 8}
    for q in cs.batches[0].queries:
        h = cases.expected(c, q, 1)
        assert max(x[2] for x in h) == len(q) - 1 and (len(q) <= 257 or any(x[2] == 256 for x in h))
    for name, rows in (("wq_rows", C["kWqRows"]), ("wq_rows_one", 1)):
        cs = cases.case(name)
        assert cs.corpus.ids.size == rows == cs.reaches["rows"] and cs.n_sub == 1
        h = cases.expected(cs.corpus, cs.batches[0].queries[0], 2)
        assert {x[0] for x in h} == {1, rows}                                        # row 0 and the last bit of the bitmaps


@pytest.mark.parametrize("name,subs", [("groups", 3), ("groups_two", 2)])
def test_groups_reach_both_sides_of_one(name, subs):
    cs = cases.case(name)
    c = cs.corpus
    assert cs.n_sub == subs == cs.reaches["subs"] and [len(b.queries) for b in cs.batches] == list(cases.GROUP_Q)
    assert cs.reaches["groups"] == [cases.unfused_groups(Q, subs) for Q in cases.GROUP_Q]
    assert cs.reaches["groups"][:3] == [subs, 2, 2] and cs.reaches["groups"][3:] == [1, 1]
    assert all(1 <= len(q) <= 3 for q in cs.batches[-1].queries) and all(b.forms == ("match",) for b in cs.batches)
    # hits in every sub-index, and queries with hits in more than one (their blocks share hits_n)
    hs = _hits(cs, c, 4, 1)
    spread = 0
    for h in hs[:300]:
        spread += len({(v - 1) >> cases.SUB_LOG2 for v, _, _ in h}) > 1
    assert spread > 50 and {(v - 1) >> cases.SUB_LOG2 for h in hs for v, _, _ in h} == set(range(subs))
