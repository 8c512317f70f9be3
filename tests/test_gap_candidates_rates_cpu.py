"""tvz_align_candidates_rates without a GPU: the reference's two restatements, its equality with the plain reference at
the rate 1.0, the premises of the cases (the speed-changed copies, two close rates, three rows of one id, the fold and
the overflow tables), the new header against the fourth signature table and the library's exports, every refusal that
needs no device and their order, the Inspector switch against a fake corpus, the new code objects, and the host code
under ASan + UBSan in a stand-alone program."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from tests import gap_candidates_cases as cs, gap_candidates_rates_cases as rc, gap_candidates_rates_ref as rr, \
    gap_candidates_ref as ref
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)
from tests.test_gap_candidates_cpu import _Corpus, _Store, _kind, _prototype
from tvidz_amd import _lib, build as tbuild, corpus as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tvz_gap_rates.h")
MAIN = os.path.join(ROOT, "tests", "gap_candidates_rates_host_main.hip")
# the scan and the probes are the plain call's too (R = 1, the rate 1.0); the fold is this call's own
NEW = ("22ts_gapc_offsets_kernelE", "20ts_gapc_probe_kernelE", "19ts_gapr_fold_kernelE")
OLD = ("21ts_gapc_select_kernelE", "20ts_gapc_merge_kernelE")
GONE = ("gapr_offsets", "gapr_probe")                      # the second copies of the scan and the probes
EPS = rc.GAP_EPS
ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -4, -5
INT32_MIN = -(1 << 31)


@pytest.fixture(scope="module")
def main_matrices():
    """the count matrices of the main table for every rate list: computed once, never changed"""
    rows, queries = rc.table(), rc.queries()
    return rows, {rates: rr.count_matrix(rows, queries, EPS, rates) for rates in rc.RATE_LISTS}


# ------------------------------------------------------------------------------------------------ the reference
def test_the_two_restatements_agree():
    rows = rc.table()
    named = (rc.FILM, rc.TRIPLE, rc.NTSC, cs.TWIN, cs.SPECIAL_ROW, cs.ROW0, cs.ROW3, cs.ROW4, cs.WIDE_GAP)
    small = [(v, k[:24]) for v, k in rows if v in named or 1000 <= v < 1004]
    up = rc.uploads()
    names = ("slow", "triple", "four", "special", "three", "empty", "plain")
    queries = [up[n][:20] for n in names]
    for rates, c, min_count, excl in ((rc.RATES3, 4, 1, None), (rc.RATES2, 2, 2, [rc.FILM] * len(names)),
                                      ((1.0, rc.SLOW, 1.0, rc.PULLDOWN), 1, 6, None)):
        a = rr.candidates_rates(small, queries, EPS, rates, c, min_count=min_count, exclude_ids=excl)
        b = rr.candidates_rates_loops(small, queries, EPS, rates, c, min_count=min_count, exclude_ids=excl)
        assert (a == b).all(), (rates, c, min_count)
    # ... with a capacity that one rate's list exceeds, and a refused query
    a = rr.candidates_rates(small, queries + [cs.long_query(515, 2)], EPS, rc.RATES3, 2, min_count=1, cap=2)
    b = rr.candidates_rates_loops(small, queries + [cs.long_query(515, 2)], EPS, rc.RATES3, 2, min_count=1, cap=2)
    assert (a == b).all() and (a[:, 2, 1] < 0).any() and a[-1, 2, 1] == INT32_MIN


def test_one_rate_of_one_equals_the_plain_reference():
    rows = rc.distinct_table()
    assert len({v for v, _ in rows}) == len(rows) > 100                            # distinct ids
    up = cs.uploads()
    queries = [up[n] for n in up] + [cs.counting_query(), cs.long_query(515, 2)]
    for c, min_count, cap in ((16, 1, 4096), (1, 2, 4096), (64, 6, 4096), (4, 1, 8)):
        plain = ref.candidates(rows, queries, EPS, c, min_count=min_count, cap=cap)
        rated = rr.candidates_rates(rows, queries, EPS, (1.0,), c, min_count=min_count, cap=cap)
        assert (rated[:, :, :2] == plain).all() and (rated[:, :, 2] == 0).all()


# ---------------------------------------------------------------------------------------- premises of the cases
def test_no_gap_of_the_cases_lies_on_an_edge():
    every = tuple(sorted({r for rates in rc.RATE_LISTS for r in rates}))
    for q in rc.queries():
        assert rc.scaled_edge_distance(q, every) > 1e-6
    for table in (rc.table(), rc.fold_table(), rc.overflow_table()):
        assert min(cs.edge_distance(k, EPS, True) for _, k in table) > 1e-6
    assert rc.scaled_edge_distance(cs.counting_query(), rc.FOLD_RATES + (rc.QUARTER,)) > 1e-6


@pytest.mark.parametrize("rho", rc.SPEEDS)
def test_a_speed_changed_copy_leads_at_its_rate_and_is_lost_at_rate_one(rho):
    """stored = rho x upload + shift: with rho in the list the film leads with every position and that rate's index;
    with (1.0,) alone its count stays below min_count - every gap of the film is at least 27 bins, 4 % of which is
    more than a bin."""
    rows = rc.table()
    up = rc.sped_up(cs.film(), rho, 12.5)
    assert rc.scaled_edge_distance(up, (1.0, rho)) > 1e-6
    for rates in ((1.0, rho), (rc.PULLDOWN, 1.0, rho, rho)):
        blk = rr.candidates_rates(rows, [up], EPS, rates, 4, min_count=rc.MIN_COUNT)[0]
        assert blk[0].tolist() == [rc.FILM, 117, rates.index(rho)], rates
    alone = rr.count_matrix(rows, [up], EPS, (1.0,))[0][0]
    film_at = [i for i, (v, _) in enumerate(rows) if v == rc.FILM][0]
    assert int(alone[film_at]) < rc.MIN_COUNT
    assert int(rr.candidates_rates(rows, [up], EPS, (1.0,), 4, min_count=rc.MIN_COUNT)[0][4, 1]) == 0


def test_two_close_rates_hit_one_row_which_appears_once(main_matrices):
    rows, matrices = main_matrices
    plain = rc.NAMES.index("plain")
    m = matrices[rc.RATES2][plain]
    film_at = [i for i, (v, _) in enumerate(rows) if v == rc.FILM][0]
    ntsc_at = [i for i, (v, _) in enumerate(rows) if v == rc.NTSC][0]
    assert m[0, film_at] == 117 and 2 <= m[1, film_at] < 117                        # both rates hit the film: unequal counts
    assert 2 <= m[0, ntsc_at] < m[1, ntsc_at]                                        # ... and the second is the better one here
    blk = rr.blocks(rows, matrices[rc.RATES2], 8, min_count=2)[plain]
    assert blk[:3].tolist() == [[rc.FILM, 117, 0], [rc.NTSC, int(m[1, ntsc_at]), 1], [-1, 0, 0]]
    assert blk[8].tolist() == [-1, 4, 0]                                             # four pairs, two ids: an upper bound
    # equal counts at two indexes (the rate 1.0 stands twice in the list of 8): the smaller index
    m8 = matrices[rc.RATES8][plain]
    assert m8[0, film_at] == m8[7, film_at] == 117
    blk = rr.blocks(rows, matrices[rc.RATES8], 8, min_count=2)[plain]
    assert blk[0].tolist() == [rc.FILM, 117, 0] and [r[0] for r in blk[:8].tolist()].count(rc.FILM) == 1


def test_three_rows_of_one_id_at_three_rates_and_the_other_premises(main_matrices):
    rows, matrices = main_matrices
    at = {n: i for i, n in enumerate(rc.NAMES)}
    triple = [i for i, (v, _) in enumerate(rows) if v == rc.TRIPLE]
    m = matrices[rc.RATES3][at["triple"]]
    assert len(triple) == 3 and sorted(int(m[:, i].max()) for i in triple) == [7, 9, 11]
    assert len({int(m[:, i].argmax()) for i in triple}) == 3                          # each row at a rate of its own
    blk = rr.blocks(rows, matrices[rc.RATES3], 16, min_count=2)
    assert blk[at["triple"], 0].tolist() == [rc.TRIPLE, 11, 2] and blk[at["triple"], 16, 1] >= 3
    assert [r[0] for r in blk[at["triple"], :16].tolist()].count(rc.TRIPLE) == 1
    assert blk[at["slow"], 0].tolist() == [rc.FILM, 117, 1] and blk[at["fast"], 0].tolist() == [rc.FILM, 117, 2]
    assert blk[at["q515"], 16, 1] == INT32_MIN and (blk[at["q515"], :16] == (-1, 0, 0)).all()
    assert blk[at["empty"], 16, 1] == 0 and blk[at["three"], 16, 1] == 0
    assert rr.blocks(rows, matrices[rc.RATES8], 4, min_count=2)[at["quarter"], 0].tolist() == [rc.FILM, 117, 5]
    # the exclusions differ per query and change the answers they are meant to change
    ex = rr.blocks(rows, matrices[rc.RATES3], 16, min_count=2, exclude_ids=rc.exclusions())
    assert ex[at["slow"], 0, 0] != rc.FILM and ex[at["fast"], 0, 0] == rc.FILM and ex[at["triple"], 16, 1] == 0
    assert len(set(rc.exclusions())) == len(rc.NAMES)


def test_the_fold_and_the_overflow_tables():
    q = [cs.counting_query()]
    ft = rc.fold_table()
    m = rr.count_matrix(ft, q, EPS, rc.FOLD_RATES)[0]
    entries = int((m >= 1).sum())
    assert entries > 2048 and len(rc.FOLD_RATES) == 8                               # the fold crosses a chunk boundary
    per_id = {}
    for v, _ in ft:
        per_id[v] = per_id.get(v, 0) + 1
    assert max(per_id.values()) >= 4 and len(per_id) == rc.FOLD_IDS + 5             # ids repeat: more than R entries per id
    blk = rr.blocks(ft, [m], 64, min_count=1)[0]
    assert int(blk[64, 1]) == entries and len(set(blk[:64, 0].tolist())) == 64
    assert len(set(blk[:64, 2].tolist())) >= 3 and int(blk[0, 1]) == int(blk[1, 1]) == 7    # several rates lead; ties on count
    ot = rc.overflow_table()
    m = rr.count_matrix(ot, q, EPS, (1.0, rc.QUARTER))[0]
    n0, n1 = int((m[0] >= 1).sum()), int((m[1] >= 1).sum())
    assert n1 <= 20 < n0                                                             # cap = 20: the first list alone overflows
    blk = rr.blocks(ot, [m], 3, min_count=1, cap=20)[0]
    assert blk.tolist() == [[7000, 9, 1], [7001, 9, 1], [7002, 9, 1], [-1, -(n0 + n1), 0]]
    assert int(m[0].max()) < 9                                                       # whatever the first list lost, these three lead


# ------------------------------------------------------------------------------------------------- the C ABI
def test_the_header_the_fourth_table_and_the_exports_agree():
    text = open(HEADER).read()
    declared = set(re.findall(r"^\w[\w ]*?\b(tvz_\w+)\(", text, re.M))
    assert declared == set(_lib.GAP_RATE_SIGNATURES) and len(declared) == 2
    for name, (res, args) in _lib.GAP_RATE_SIGNATURES.items():
        assert (_kind(res), [_kind(a) for a in args]) == _prototype(text, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    defined = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", tbuild.SO], text=True).splitlines()
               if ln.strip()}
    assert declared <= defined, sorted(declared - defined)
    lib = _lib.load()
    for name in declared:                                                          # load() bound the fourth table too
        assert getattr(lib, name).argtypes == _lib.GAP_RATE_SIGNATURES[name][1]
    # the other three tables are what they were and disjoint from it; the version too
    for other, n in ((_lib.SIGNATURES, 75), (_lib.GAP_SIGNATURES, 4), (_lib.GAP_SHARD_SIGNATURES, 4)):
        assert len(other) == n and not declared & set(other)
    assert _lib.VERSION == 404 and lib.tvz_version() == 404
    assert '#include "tvz_gap.h"' in text and "upper bound" in text.lower()
    for h in ("tvz.h", "tvz_gap.h", "tvz_gap_shards.h"):
        assert "candidates_rates" not in open(os.path.join(ROOT, "include", h)).read()
    assert tc.DeviceCorpus.supports_align_candidate_rates is True


def test_the_sizing_function_and_where_it_answers_zero():
    lib = _lib.load()
    for Q, L, keys, R, cap, c in ((1, 200, 0, 1, 4096, 16), (16, 514, 0, 8, 64, 64), (70, 40, 1234, 3, 17, 1), (1, 0, 0, 2, 1, 1),
                                  (0, 10, 0, 8, 4, 4), (21845, 4, 0, 3, 1, 1)):
        total = max(keys if keys > 0 else Q * L, L)
        probe_len = min(8 * max(L - 3, 1), 4088)
        raw = Q * R * cap * 12 + 2 * Q * R * 4 + (Q * R + 1) * 8 + Q * 4 + lib.tvz_match_workspace_bytes(Q * R, probe_len, 0, 0, 1) \
            + total * (8 + 4 + 64 * R)
        got = tc.align_candidates_rates_workspace_bytes(Q, L, keys, R, cap, c)
        assert raw <= got < raw + 11 * 256, (Q, L, keys, R, cap, c, got, raw)
    for bad in ((-1, 10, 0, 1, 16, 16), (1, -1, 0, 1, 16, 16), (1, 10, -1, 1, 16, 16), (1, 10, 0, 1, 16, 0), (1, 10, 0, 1, 16, 65),
                (1, 10, 0, 1, 15, 16), (1, 4096, 0, 1, 16, 16), (1, 10, 0, 0, 16, 16), (1, 10, 0, 9, 16, 16), (8192, 10, 0, 8, 16, 16),
                (21846, 4, 0, 3, 1, 1), (65536, 4, 0, 1, 1, 1)):
        assert tc.align_candidates_rates_workspace_bytes(*bad) == 0, bad


def test_refusals_that_need_no_device_and_their_order():
    """Every parameter is refused before the handle is looked at - a NULL handle's refusal stands behind them, so the
    order shows in the message: C, cap, min_count, max_query_len (the plain call's, in its order); the rate list, in the
    words of tvz_align_rates_topk; the probe lists; then the handle."""
    lib = _lib.load()
    good = (C.c_double * 8)(1.0, 0.96, 25 / 24, 1.0, 1.25, 0.8, 1000 / 1001, 1.001)

    def call(C_=16, cap=64, min_count=2, L=4, rates=good, R=3, Q=1):
        rc_ = lib.tvz_align_candidates_rates(None, None, None, Q, L, rates, R, min_count, None, cap, C_, None, None, 0, None)
        return rc_, lib.tvz_last_error()

    for bad in (0, 65, -1):
        assert call(C_=bad) == (ERR_UNSUPPORTED, b"alignment candidates: C=%d outside 1..64" % bad)
    assert call(cap=15) == (ERR_UNSUPPORTED, b"alignment candidates: cap=15 below C=16")
    assert call(min_count=0) == (ERR_INVALID, b"alignment candidates: min_count 0 below 1")
    assert call(L=4096) == (ERR_UNSUPPORTED, b"alignment candidates: max_query_len 4096 above 4095")
    for bad in (0, 9, -2):
        assert call(R=bad) == (ERR_UNSUPPORTED, b"alignment top-k with rates: n_rates=%d outside 1..8 (TVZ_ALIGN_MAX_RATES)" % bad)
    rc_, msg = call(rates=None)
    assert rc_ == ERR_INVALID and b"h_rates is NULL" in msg
    for bad in (float("nan"), float("inf"), 0.0, -1.0, -0.0):
        rc_, msg = call(rates=(C.c_double * 3)(1.0, 0.96, bad))
        assert rc_ == ERR_INVALID and b"rate 2 is" in msg and b"every rate must be finite and > 0" in msg, bad
    for Q, R in ((8192, 8), (21846, 3), (65535, 2), (70000, 1)):
        rc_, msg = call(Q=Q, R=R)
        assert rc_ == ERR_UNSUPPORTED and msg == b"alignment candidates with rates: Q=%d x n_rates=%d is above 65535 probe lists" % (Q, R)
    # the order, one step at a time
    assert b"C=0" in call(C_=0, cap=-1, min_count=0, L=4096, R=0, Q=70000)[1]
    assert b"cap=15" in call(cap=15, min_count=0, L=4096, R=0, Q=70000)[1]
    assert b"min_count 0" in call(min_count=0, L=4096, R=0, Q=70000)[1]
    assert b"max_query_len 4096" in call(L=4096, R=0, Q=70000)[1]
    assert b"n_rates=0" in call(R=0, Q=70000)[1]
    assert b"rate 0 is" in call(rates=(C.c_double * 1)(float("nan")), R=1, Q=70000)[1]
    assert b"probe lists" in call(R=1, Q=70000)[1]
    for kw in (dict(), dict(C_=64, cap=64, min_count=1, L=4095, R=8), dict(Q=21845, R=3), dict(Q=-1)):
        rc_, msg = call(**kw)
        assert rc_ == ERR_INVALID and b"corpus is NULL" in msg, kw


# ---------------------------------------------------------------------------------------------- the inspector
class _RatesCorpus(_Corpus):
    """tests/test_gap_candidates_cpu.py's fake with the rates call: it names ids 42, 43, 44 at rate indexes 1, 0, 2; the
    parts call answers id 42 at the rate index 1 in its header, which is where the report must take it from"""

    def align_candidates_rates(self, queries, **kw):
        self.calls.append(("align_candidates_rates", dict(kw, Q=len(queries))))
        c = kw["c"]
        ids = np.full((len(queries), c), -1, dtype=np.int32)
        counts, rate_indexes = np.zeros_like(ids), np.zeros_like(ids)
        if self.refuse:
            return ids, counts, rate_indexes, np.full(len(queries), INT32_MIN, dtype=np.int32)
        ids[:, :3], counts[:, :3], rate_indexes[:, :3] = (42, 43, 44), (57, 9, 2), (2, 0, 2)    # (42: NOT the header's index)
        return ids, counts, rate_indexes, np.full(len(queries), 5, dtype=np.int32)

    def align_parts(self, queries, video_ids, **kw):
        out = super().align_parts(queries, video_ids, **kw)
        for j, vid in enumerate(video_ids[0]):
            if vid == 42:
                out[:, j, 0, 2] = 1
        return out


def test_inspector_candidate_rates_switch_calls_refusals_fallback_and_clear():
    from tvidz_amd import inspector as insp

    ok = dict(device="cuda:0", near_duplicates=True, near_top_k=8, near_any_offset=True, near_score="local", near_min_votes=8,
              near_jaccard=0.9)
    rates = (1.0, 0.96, 1.25)
    new = lambda corpus=None, **kw: insp.Inspector(_Store(corpus or _RatesCorpus()), **dict(ok, **kw))        # noqa: E731
    # switch clear: the combination raises exactly as it did
    with pytest.raises(RuntimeError, match=r"near_candidates=16 with near_rates=\(1\.0, 0\.96, 1\.25\): the gap codes are made at "
                                           "rate 1; use one of them"):
        new(near_candidates=16, near_rates=rates)
    with pytest.raises(RuntimeError, match="near_candidates=16 with near_rates"):
        new(near_candidates=16, near_rates=rates, near_candidate_rates=False)
    # switch set: what is missing is named
    with pytest.raises(RuntimeError, match="near_candidate_rates=True needs near_candidates and near_rates"):
        new(near_candidate_rates=True)
    with pytest.raises(RuntimeError, match="near_candidate_rates=True needs near_rates$"):
        new(near_candidate_rates=True, near_candidates=16)
    with pytest.raises(RuntimeError, match="near_candidate_rates=True needs near_candidates$"):
        new(near_candidate_rates=True, near_rates=rates)
    with pytest.raises(RuntimeError, match="near_candidates=16 with near_two_bins=True"):
        new(near_candidate_rates=True, near_candidates=16, near_rates=rates, near_two_bins=True)
    with pytest.raises(RuntimeError, match="has no align_candidates_rates"):
        new(_Corpus(), near_candidate_rates=True, near_candidates=16, near_rates=rates)
    flagged = _RatesCorpus()
    flagged.supports_align_candidate_rates = False
    with pytest.raises(RuntimeError, match="has no align_candidates_rates"):
        new(flagged, near_candidate_rates=True, near_candidates=16, near_rates=rates)
    cuts = [float(3 * i) for i in range(128, -1, -1)] + [float("nan")]             # unsorted, one NaN
    # set: per upload ONE rates call and ONE parts call, both with the configured list; no sweep, no plain candidates call
    corpus = _RatesCorpus()
    ins = new(corpus, near_candidates=16, near_rates=rates, near_candidate_rates=True, near_gap_eps=0.05)
    assert corpus.calls == [("set_gap_index", 0.05)]
    (near,) = ins._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates_rates", "align_parts"]
    assert corpus.calls[1][1] == dict(rates=rates, c=16, exclude_ids=[7], Q=1)
    assert corpus.calls[2][1] == dict(video_ids=[[42, 43, 44]], Q=1, eps=ins.near_eps, rates=rates, min_votes=8, max_parts=1)
    # the report: part 0 and the header, the rate from the parts header (index 1), as the rates sweep words it
    assert near["video_id"] == 42 and near["rate"] == 0.96 and near["shift_seconds"] == 0.0 and near["local"] == 1.0
    assert near["upload_span"] == [0.0, 177.0] and near["stored_span"] == [0.96 * 0.0, 0.96 * 177.0]
    sweep = _RatesCorpus()
    (swept,) = new(sweep, near_rates=rates)._near(7, cuts)                            # (the fake's sweep answers at index 0)
    assert [c[0] for c in sweep.calls] == ["align_span_topk"] and sweep.calls[0][1]["rates"] == rates
    assert {k: v for k, v in near.items() if k not in ("rate", "stored_span")} == \
        {k: v for k, v in swept.items() if k not in ("rate", "stored_span")} and swept["rate"] == 1.0
    # with near_parts the parts come from the same block at the same list; without spans the rows keep their rate
    corpus = _RatesCorpus()
    (near,) = new(corpus, near_candidates=8, near_rates=rates, near_candidate_rates=True, near_parts=3)._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates_rates", "align_parts"]
    assert corpus.calls[2][1]["max_parts"] == 3 and corpus.calls[2][1]["rates"] == rates and len(near["parts"]) == 2
    assert near["parts"][1]["stored_span"] == [0.96 * 207.0 - 1419 * ins.near_eps, 0.96 * 384.0 - 1419 * ins.near_eps]
    wide = dict(ok, near_score="jaccard", near_jaccard=0.3, near_min_votes=1)
    (near,) = insp.Inspector(_Store(_RatesCorpus()), **dict(wide, near_candidates=8, near_rates=rates,
                                                            near_candidate_rates=True))._near(7, cuts)
    assert near["rate"] == 0.96 and "upload_span" not in near
    # a refused upload takes the configured RATES sweep
    corpus = _RatesCorpus(refuse=True)
    (near,) = new(corpus, near_candidates=16, near_rates=rates, near_candidate_rates=True)._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates_rates", "align_span_topk"]
    assert corpus.calls[2][1]["rates"] == rates and near == swept
    # switch clear: untouched - the plain candidates path makes the plain call with (1.0,)
    corpus = _RatesCorpus()
    ins = new(corpus, near_candidates=16)
    assert ins.near_candidate_rates is False
    ins._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates", "align_parts"]
    assert corpus.calls[2][1]["rates"] == (1.0,)


# -------------------------------------------------------------------------------------------- the code objects
def test_the_new_kernels_exist_once_with_no_scratch_and_the_old_ones_keep_their_names(kernels):  # noqa: F811
    recorded = {}
    for name in NEW:
        found = [k for n, k in kernels.items() if name in n]
        assert len(found) == 1, (name, sorted(n for n in kernels if "gap" in n))
        (k,) = found
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (name, k)
        assert k[".wavefront_size"] == 64
        recorded[name] = (k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".max_flat_workgroup_size"])
    print("vgprs, sgprs, LDS bytes, block:", recorded)
    assert recorded[NEW[0]][3] == 1024 and recorded[NEW[1]][3] == 256 and recorded[NEW[2]][3] == 256
    # the fold's sort buffers (2,048 keys and counts), its 9 list starts and the compiler's padding between them; the
    # scan's word per wave; the probes: no LDS
    assert 2048 * 12 + 36 <= recorded[NEW[2]][2] <= 2048 * 12 + 512 and recorded[NEW[0]][2] == 64 and recorded[NEW[1]][2] == 0
    # registers, as the compiler reported them when the kernels were written (a rise is looked at, not forbidden)
    assert recorded[NEW[1]][0] <= 64 and recorded[NEW[2]][0] <= 64 and recorded[NEW[0]][0] <= 40
    for name in OLD:
        assert len([n for n in kernels if name in n]) == 1, name
    for name in GONE:
        assert not [n for n in kernels if name in n], name


# ------------------------------------------------------------------------------------ the host code, sanitized
def _program():
    sources = sorted(os.path.join(tbuild.CSRC, f) for f in os.listdir(tbuild.CSRC)) + \
        [os.path.join(tbuild.INCLUDE, h) for h in ("tvz.h", "tvz_gap.h", "tvz_gap_shards.h", "tvz_gap_rates.h")] + [MAIN]
    h = hashlib.sha1()
    for f in sources:
        h.update(open(f, "rb").read())
    cache = os.path.join(tempfile.gettempdir(), f"tvz-host-sanitizer-{os.getuid()}")
    os.makedirs(cache, exist_ok=True)
    exe = os.path.join(cache, "gapr-" + h.hexdigest()[:16])
    if not os.path.exists(exe):
        # (the device half is compiled because the translation unit registers its kernels; unoptimised: it never runs)
        subprocess.check_call([tbuild._hipcc(), f"--offload-arch={tbuild.ARCH}", "-O1", "-Xarch_device", "-O0", "-std=c++17",
                               "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                               "-Wno-unused-function", f"-I{tbuild.INCLUDE}", f"-I{tbuild.CSRC}", "-o", exe + f".{os.getpid()}.tmp",
                               MAIN, os.path.join(tbuild.CSRC, "tvz_api.hip"), "-ldl"])
        os.replace(exe + f".{os.getpid()}.tmp", exe)
    return exe


def test_host_carving_and_refusals_under_asan_and_ubsan():
    """The workspace of the rates call is carved inside its buffer at every misalignment, for n_rates 1 and 8, its regions
    disjoint and in order; the refusals that come before any device call come in the header's order."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([_program()], capture_output=True, text=True, timeout=300, env=env, stdin=subprocess.DEVNULL)
    assert out.returncode == 0 and out.stdout.strip().endswith("HOST_OK"), (out.stdout[-500:], out.stderr[-3000:])
