"""tvz_align_parts_flags without a GPU: the reference of tests/align_parts_two_bins_ref.py against tests/align_parts_ref.py
(flag clear), against tests/align_two_bins_ref.py (part 0), against a plain double loop and fractions; the premises of
tests/align_parts_two_bins_cases.py; the new header against the binding's new table and the library's exports, the old
table and version unchanged; every refusal that needs no device and their order; the Inspector's option on fakes of its
own; the gfx950 code object of the new walk kernel; and the host code under ASan + UBSan in a stand-alone program."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

from tests import align_parts_cases as pc, align_parts_ref as apr, align_parts_two_bins_cases as cs
from tests import align_parts_two_bins_ref as ref, align_two_bins_ref as tb
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)
from tests.test_gap_candidates_cpu import _kind, _prototype
from tvidz_amd import _lib, build as tbuild, corpus as tc, service

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tvz_parts_flags.h")
OLD_HEADER = os.path.join(ROOT, "include", "tvz.h")
MAIN = os.path.join(ROOT, "tests", "align_parts_two_bins_host_main.hip")
EPS, MAX_B, TWO = cs.EPS, cs.MAX_B, ref.TWO_BINS
ERR_INVALID, ERR_UNSUPPORTED = -1, -4
INT32_MIN = -(1 << 31)
NEW, SIBLING = "22ts_alignp2_walk_kernelE", "21ts_alignp_walk_kernelE"


@pytest.fixture(scope="module")
def world():
    return cs.table(), cs.uploads()


# ------------------------------------------------------------------------------------------------ 1. the reference
def test_the_reference_with_the_flag_clear_is_the_parts_reference():
    rows, uploads = pc.table(), pc.uploads()
    queries = list(uploads.values())
    ids = [list(pc.IDS)] * len(queries)
    for B, rates, min_votes, max_parts in ((900, (1.0,), 1, 4), (MAX_B, (1.0, 0.96), 8, 3), (5000, (0.96, 1.0), 1, 2)):
        a = apr.align_parts_ref(rows, queries, ids, EPS, B * EPS, rates, min_votes, max_parts)
        b = ref.align_parts_flags_ref(rows, queries, ids, EPS, B * EPS, rates, min_votes, max_parts, 0)
        assert (a == b).all(), (B, rates)


def test_part_0_is_the_two_bin_span_answer_on_every_row_of_the_cases(world):
    rows, uploads = world
    B, W = cs.seam_B()
    queries = list(uploads.values()) + list(cs.row_queries().values()) + [cs.SEAM_Q, cs.LONE_Q]
    for query in queries:
        for bins, rates in ((B, (1.0, 1.04)), (MAX_B, (0.96, 1.0))):
            span = tb.align_two_bins_ref(rows, query, EPS, bins * EPS, rates)
            for (vid, keys), want in zip(rows, span.tolist()):
                row_len, rate, votes0, parts = ref.row_parts(keys, query, EPS, bins * EPS, rates, 1, 1, TWO)
                assert (row_len, votes0) == (want[1], want[3]), (vid, bins)
                if votes0:
                    bn, J, t_first, t_last, nq, nr = parts[0]
                    assert [bn, J, rate, t_first, t_last, nr] == want[2:] and nq == t_last - t_first + 1, (vid, bins)


def test_the_reference_the_double_loop_and_fractions_agree_on_a_small_case(world):
    rows, uploads = world
    B, W = cs.seam_B()
    by_id = {v: k for v, k in rows if v not in (cs.FLAG_BETTER, cs.EQUAL_J, cs.NINE_ROWS)}
    cases = [(by_id[cs.TIE_LATER], cs.base30().tolist(), 1.0, MAX_B), (by_id[cs.TIE_LATER + 100], cs.base30().tolist(), 1.0, 900),
             (by_id[cs.SEAM0 + 4], cs.SEAM_Q, 1.0, B), (by_id[cs.SEAM0 + 5], cs.SEAM_Q, 1.0, B + 517),
             (by_id[cs.RATE_CARRY], cs.LONE_Q, 1.04, B), (by_id[cs.SPECIAL], uploads["special"], 1.0, MAX_B),
             (by_id[cs.LANES65], cs.row_queries()["parts24"], 1.0, MAX_B)]
    for keys, query, rho, bins in cases:
        for min_votes, max_parts in ((1, 4), (8, 2)):
            want = ref.row_parts(keys, query, EPS, bins * EPS, (rho,), min_votes, max_parts, TWO)[3]
            assert ref.double_loop(keys, query, EPS, bins * EPS, rho, min_votes, max_parts) == want
            # exact arithmetic agrees wherever no quotient lies near an edge (asserted for these rows below)
            assert ref.double_loop(keys, query, EPS, bins * EPS, rho, min_votes, max_parts, Fraction) == want


# ------------------------------------------------------------------------------------ 2. the premises of the cases
def test_no_vote_of_the_made_cases_lies_within_a_millionth_of_a_bin_of_an_edge(world):
    """... so exact and IEEE arithmetic agree on every bin.  The re-timed uploads are the exception by construction:
    their cuts sit on a 1/25 s grid against the film's 1/30 s grid, where quotients land on k/5 of a bin - never on .5."""
    rows, uploads = world
    by_id = dict((v, k) for v, k in rows)
    made = [(cs.TIE0, cs.base30()), (cs.TIE0 + 100, cs.base30()), (cs.TIE_LATER, cs.base30()), (cs.TIE_LATER + 100, cs.base30()),
            (cs.RATE_CARRY, cs.LONE_Q), (cs.ONLY_B, cs.SEAM_Q), (cs.LANES64, cs.row_queries()["parts24"]),
            (cs.LONG700, cs.row_queries()["parts24"]), (cs.FILM, uploads["copy"]), (cs.FILM, uploads["swapped"]),
            (cs.REELS, uploads["retimed_inserted"]), (cs.FILM, uploads["fps_inserted"])] + [(cs.SEAM0 + i, cs.SEAM_Q) for i in range(6)]
    for vid, query in made:
        c = np.asarray([x for x in by_id[vid] if np.isfinite(x)])
        for rho in (1.0, 1.04, 0.96):
            s = np.sort(np.asarray(query, dtype=np.float64)) * rho
            d = (c[:, None] - s[None, :]) / EPS + 0.5
            d = d[np.abs(d) <= 3 * 1024 + 2000]
            assert (np.abs(d - np.round(d)) > 1e-6).all(), (vid, rho)


def test_the_retimed_copy_with_an_insertion_needs_the_window(world):
    rows, uploads = world
    q, ids = [uploads["retimed_inserted"]], [[cs.REELS]]
    clear = ref.align_parts_flags_ref(rows, q, ids, EPS, MAX_B * EPS, (1.0,), 61, 4, 0)
    flag = ref.align_parts_flags_ref(rows, q, ids, EPS, MAX_B * EPS, (1.0,), 61, 4, TWO)
    assert clear[0, 0, 0].tolist() == [cs.REELS, 200, 0, 0, 1, 209] and not clear[0, 0, 1:].any()
    assert flag[0, 0].tolist()[:3] == [[cs.REELS, 200, 0, 2, 1, 209], [2284, 100, 109, 208, 100, 100], [3703, 100, 0, 99, 100, 100]]
    # single bins hold about half: 52 of each hundred
    low = ref.align_parts_flags_ref(rows, q, ids, EPS, MAX_B * EPS, (1.0,), 1, 2, 0)
    assert low[0, 0, 1:3, 1].tolist() == [52, 52]
    # the shift is the window's middle, within a bin: (2284 + 0.5) / 30 against 123.451 - 47.3
    assert abs((2284 + 0.5) * EPS - (cs.RETIME_SHIFT - cs.RETIME_MOVE)) < EPS and abs((3703 + 0.5) * EPS - cs.RETIME_SHIFT) < EPS


def test_the_copies_at_a_third_of_a_bin_keep_their_votes_only_in_the_window(world):
    rows, uploads = world
    for name, single, window in (("copy", [83], [120]), ("removed", [37, 31], [50, 40]), ("swapped", [27, 27], [40, 40]),
                                 ("two_inserted", [30, 30, 25], [41, 40, 20]), ("stranger", [], [])):
        for flags, want in ((0, single), (TWO, window)):
            out = ref.align_parts_flags_ref(rows, [uploads[name]], [[cs.FILM]], EPS, MAX_B * EPS, (1.0,), 8, 4, flags)
            assert out[0, 0, 1:1 + len(want), 1].tolist() == want and out[0, 0, 0, 3] == len(want), (name, flags)
    for rates in ((1.0, 0.96), (0.96, 1.0)):
        out = ref.align_parts_flags_ref(rows, [uploads["fps_inserted"]], [[cs.FILM]], EPS, MAX_B * EPS, rates, 8, 4, TWO)
        assert out[0, 0, 0].tolist() == [cs.FILM, 120, rates.index(0.96), 2, 1, 129]
        assert out[0, 0, 1:3, :2].tolist() == [[-1060, 59], [360, 57]]


def test_the_seam_rows_and_the_carries(world):
    rows, uploads = world
    B, W = cs.seam_B()
    out = ref.align_parts_flags_ref(rows, [cs.SEAM_Q], [list(cs.SEAM_IDS)], EPS, B * EPS, (1.0,), 1, 3, TWO)
    for i, S in enumerate((-W, 0, W, 2 * W)):
        assert S % W == 0 and out[0, i, 1].tolist() == [S - 1, 64, 0, 7, 8, 106]      # the pair (S - 1, S) across the seam
    by_id = dict(rows)
    for i, S in enumerate((-W, W)):
        assert out[0, 4 + i, 1:3].tolist() == [[40, 40, 0, 3, 4, 48], [S - 1, 28, 4, 7, 4, 28]]
        # bin S holds 24 votes over all pairs, 16 of them allowed in part 1: a carry of all votes would give 36
        c, s = np.asarray(by_id[cs.SEAM0 + 4 + i]), np.asarray(cs.SEAM_Q)
        b = np.floor((c[:, None] - s[None, :]) / EPS + 0.5)
        assert int((b == S).sum()) == 24 and int((b[:, 4:] == S).sum()) == 16 and int((b == S - 1).sum()) == 12
    assert out[0, 6, :2].tolist() == [[cs.ONLY_B, 56, 0, 1, 1, 8], [B, 24, 0, 7, 8, 52]]   # b + 1 > B: bin B alone
    # the rate that leaves 3 votes in the lowest bin of its last window (-W), in front of the better rate whose six votes
    # lie in the highest bin of its first window (2W - 1)
    out = ref.align_parts_flags_ref(rows, [cs.LONE_Q], [[cs.RATE_CARRY]], EPS, B * EPS, (1.0, 1.04), 1, 2, TWO)
    assert out[0, 0].tolist() == [[cs.RATE_CARRY, 9, 1, 1, 1, 1], [2 * W - 1, 6, 0, 0, 1, 6], [0] * 6]
    only = ref.align_parts_flags_ref(rows, [cs.LONE_Q], [[cs.RATE_CARRY]], EPS, B * EPS, (1.0,), 1, 2, TWO)
    assert only[0, 0, 1].tolist() == [-W, 3, 0, 0, 1, 3] and (2 * W - 1 + B) % W == W - 1 and (-W + B) % W == 0


def test_the_tie_chain_and_the_rows_of_one_id(world):
    rows, uploads = world
    assert len(rows) <= 51 and max(len(k) for _, k in rows) == 700
    assert sorted(len(k) for v, k in rows if v in (cs.LANES64, cs.LANES65, cs.LANES513, cs.LONG700)) == [64, 65, 513, 700]
    q, at = [cs.base30().tolist()], cs.NAMED.index
    exp = ref.align_parts_flags_ref(rows, q, [list(cs.NAMED)], EPS, MAX_B * EPS, (1.0,), 1, 4, TWO)[0]
    clear = ref.align_parts_flags_ref(rows, q, [list(cs.NAMED)], EPS, MAX_B * EPS, (1.0,), 1, 4, 0)[0]
    assert exp[at(cs.TIE0), 1].tolist() == [21, 10, 4, 13, 10, 10]
    assert exp[at(cs.TIE0 + 100), 1:3].tolist() == [[-11, 8, 0, 7, 8, 8], [11, 8, 8, 15, 8, 8]]
    assert exp[at(cs.TIE_LATER), 1:4].tolist() == [[0, 12, 0, 11, 12, 12], [-5, 8, 12, 19, 8, 8], [5, 8, 20, 27, 8, 8]]
    assert exp[at(cs.TIE_LATER + 100), 1:3].tolist() == [[0, 12, 0, 11, 12, 12], [51, 8, 15, 22, 8, 8]]
    assert clear[at(cs.FLAG_BETTER), :2].tolist() == [[cs.FLAG_BETTER, 10, 0, 1, 2, 30], [30, 10, 0, 9, 10, 10]]
    assert exp[at(cs.FLAG_BETTER), :2].tolist() == [[cs.FLAG_BETTER, 16, 0, 1, 2, 30], [30, 16, 0, 15, 16, 16]]
    assert exp[at(cs.EQUAL_J), :2].tolist() == [[cs.EQUAL_J, 11, 0, 2, 2, 30], [-7, 9, 0, 8, 9, 9]]
    assert exp[at(cs.NINE_ROWS), 0].tolist() == [cs.NINE_ROWS, 0, 0, INT32_MIN, 9, 30]


# ------------------------------------------------------------------------------------------------- 3. the C ABI
def test_the_header_the_new_table_and_the_exports_agree():
    text = open(HEADER).read()
    declared = set(re.findall(r"^\w[\w ]*?\b(tvz_\w+)\(", text, re.M))
    assert declared == set(_lib.PARTS_FLAGS_SIGNATURES) == {"tvz_align_parts_flags", "tvz_align_parts_flags_shards"}
    for name, (res, args) in _lib.PARTS_FLAGS_SIGNATURES.items():
        assert (_kind(res), [_kind(a) for a in args]) == _prototype(text, name), name
    # the old calls' lists with one uint32 behind max_parts
    for new, old, at in (("tvz_align_parts_flags", "tvz_align_parts", 15), ("tvz_align_parts_flags_shards", "tvz_align_parts_shards", 16)):
        args = list(_lib.PARTS_FLAGS_SIGNATURES[new][1])
        assert args.pop(at) is C.c_uint32 and args == _lib.SIGNATURES[old][1]
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    defined = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", tbuild.SO], text=True).splitlines()
               if ln.strip()}
    assert declared <= defined, sorted(declared - defined)
    lib = _lib.load()
    for name, (res, args) in _lib.PARTS_FLAGS_SIGNATURES.items():
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args


def test_the_old_table_the_version_and_the_old_header_are_unchanged():
    assert _lib.VERSION == 404 and _lib.load().tvz_version() == 404
    sig = repr(sorted((n, getattr(r, "__name__", repr(r)), [getattr(a, "__name__", repr(a)) for a in args])
                      for n, (r, args) in _lib.SIGNATURES.items()))
    assert len(_lib.SIGNATURES) == 75 and hashlib.sha1(sig.encode()).hexdigest() == "282938b267df1282d3482c99a5c7bf489ef006b7"
    old = open(OLD_HEADER).read()
    assert "tvz_align_parts_flags" not in old and "TVZ_VERSION 404" in old
    assert tc.DeviceCorpus.supports_align_parts_two_bins is True and service.ShardedCorpus.supports_align_parts_two_bins is True
    assert not hasattr(service.RankCorpus, "supports_align_parts_two_bins")


def _flags_call(flags, max_parts=2, eps=1 / 30, mo=1.0, k=4, min_votes=1):
    lib = _lib.load()
    rates = (C.c_double * 2)(1.0, 0.96)
    rc = lib.tvz_align_parts_flags(None, None, None, 1, 10, None, 1, 1, k, eps, mo, rates, 2, min_votes, max_parts, flags, None, None, 0,
                                   None)
    msg = lib.tvz_last_error()
    rs = lib.tvz_align_parts_flags_shards(None, 1, None, None, 1, 10, None, 1, 1, k, eps, mo, rates, 2, min_votes, max_parts, flags,
                                          None, None, None, 0, None)
    return rc, msg, rs, lib.tvz_last_error()


def test_the_flags_that_are_refused_and_where_the_check_stands():
    for flags, bits in ((4, b"0x4"), (1, b"0x1"), (8 | 1, b"0x1"), (0x80000008, b"0x80000000")):
        rc, msg, rs, msg_s = _flags_call(flags)
        assert rc == rs == ERR_INVALID and b"alignment parts: unknown flag bits " + bits in msg and msg == msg_s, (flags, msg)
    for flags in (0, 8):                                                    # accepted: the next refusal is the NULL handle's
        rc, msg, rs, msg_s = _flags_call(flags)
        assert rc == ERR_INVALID and b"flag" not in msg and rs == ERR_INVALID and b"no shards" in msg_s, (flags, msg, msg_s)
    # behind max_parts ...
    rc, msg, rs, msg_s = _flags_call(4, max_parts=5)
    assert rc == rs == ERR_UNSUPPORTED and b"max_parts=5" in msg and b"max_parts=5" in msg_s
    rc, msg, _, _ = _flags_call(4, k=65)
    assert rc == ERR_UNSUPPORTED and b"k=65" in msg
    rc, msg, _, _ = _flags_call(4, min_votes=0)
    assert rc == ERR_INVALID and b"min_votes 0" in msg
    # ... and in front of eps, max_offset and B
    for kw in (dict(eps=0.0), dict(mo=-1.0), dict(eps=1.0, mo=float((1 << 22) + 1))):
        rc, msg, rs, msg_s = _flags_call(4, **kw)
        assert rc == rs == ERR_INVALID and b"unknown flag bits 0x4" in msg and b"unknown flag bits 0x4" in msg_s, kw
    rc, msg, _, _ = _flags_call(8, eps=0.0)
    assert rc == ERR_INVALID and b"eps must be > 0" in msg
    rc, msg, _, _ = _flags_call(8, eps=1.0, mo=float((1 << 22) + 1))
    assert rc == ERR_UNSUPPORTED and b"TVZ_ALIGN_WIDE_MAX_B" in msg


# --------------------------------------------------------------------------------------------- 4. the inspector
PART0 = (2284, 100, 109, 208, 100, 100)
PART1 = (3703, 100, 0, 99, 100, 100)


class _Corpus:
    """records its calls; answers the search with one span hit of video 20 and the parts call with two parts"""
    supports_align_wide = supports_align_span = supports_align_parts = supports_align_candidates = True
    supports_align_parts_two_bins = True

    def __init__(self, refuse_candidates=False):
        self.calls, self.refuse_candidates = [], refuse_candidates

    def set_gap_index(self, gap_eps):
        self.calls.append(("set_gap_index", dict(gap_eps=gap_eps)))

    def align_topk(self, queries, **kw):
        raise AssertionError("the search of these configurations is the span call's")

    align_wide_topk = align_topk

    def align_span_topk(self, queries, **kw):
        self.calls.append(("align_span_topk", dict(kw)))
        rows = np.zeros((1, kw["k"], 8), dtype=np.int32)
        rows[:, :, 0] = -1
        rows[0, 0] = (20, 200) + PART0[:2] + (0,) + PART0[2:4] + (100,)
        return rows, np.ones(1, dtype=np.int64)

    def align_candidates(self, queries, **kw):
        self.calls.append(("align_candidates", dict(kw)))
        ids = np.full((1, kw["c"], 2), -1, dtype=np.int32)
        ids[0, 0] = (20, 50)
        return ids, np.array([INT32_MIN if self.refuse_candidates else 1], dtype=np.int64)

    def align_parts(self, queries, video_ids, **kw):
        self.calls.append(("align_parts", dict(kw)))
        P = kw["max_parts"]
        out = np.zeros((1, len(video_ids[0]), 1 + P, 6), dtype=np.int32)
        out[0, 0, 0] = (20, 200, 0, min(P, 2), 1, 209)
        out[0, 0, 1:1 + min(P, 2)] = (PART0, PART1)[:P]
        return out


class _OldCorpus(_Corpus):
    """a corpus from before the option: its parts call has no two_bins keyword, and it does not say it has one"""
    supports_align_parts_two_bins = False

    def align_parts(self, queries, video_ids, *, eps, max_offset=None, rates=(1.0,), min_votes, max_parts, max_query_len=None):
        return super().align_parts(queries, video_ids, eps=eps, rates=rates, min_votes=min_votes, max_parts=max_parts)


class _Store:
    def __init__(self, corpus):
        self.corpus = corpus

    def get_video_by_id(self, vid):
        return None


def _inspector(corpus, **kw):
    from tvidz_amd import inspector as insp
    return insp.Inspector(_Store(corpus), device="cuda:0", **kw)


BASE = dict(near_duplicates=True, near_top_k=4, near_any_offset=True, near_score="local", near_min_votes=2, near_jaccard=0.5)


def test_inspector_refusals_old_and_new():
    # the old refusals, word for word, with the option absent
    with pytest.raises(ValueError, match=r"near_two_bins=True with near_parts=2: align_parts counts single bins \(it has no flags\); "
                                         "use one of them"):
        _inspector(_Corpus(), near_parts=2, near_two_bins=True, **BASE)
    with pytest.raises(RuntimeError, match=r"near_candidates=8 with near_two_bins=True: align_parts counts single bins "
                                           r"\(it has no flags\); use one of them"):
        _inspector(_Corpus(), near_candidates=8, near_two_bins=True, **BASE)
    # the new option needs near_two_bins and one of the two parts paths
    for more in (dict(), dict(near_parts=2), dict(near_candidates=8), dict(near_two_bins=True)):
        with pytest.raises(ValueError, match="near_parts_two_bins=True needs near_two_bins=True and near_parts or near_candidates"):
            _inspector(_Corpus(), near_parts_two_bins=True, **BASE, **more)
    # ... and a corpus that says it can: the default of the attribute is False
    for corpus in (_OldCorpus(), type("Bare", (_Corpus,), {"supports_align_parts_two_bins": None})()):
        with pytest.raises(RuntimeError, match=f"near_parts_two_bins=True: the store's corpus \\({type(corpus).__name__}\\)"):
            _inspector(corpus, near_parts=2, near_two_bins=True, near_parts_two_bins=True, **BASE)
    bare = type("NoAttribute", (), {n: getattr(_Corpus, n) for n in ("align_span_topk", "align_parts", "align_candidates",
                                                                     "set_gap_index", "__init__", "align_topk", "align_wide_topk")})
    with pytest.raises(RuntimeError, match="NoAttribute"):
        _inspector(bare(), near_parts=2, near_two_bins=True, near_parts_two_bins=True, **BASE)
    from tvidz_amd import inspector as insp
    rank = service.RankCorpus.__new__(service.RankCorpus)
    with pytest.raises(RuntimeError, match="RankCorpus"):
        insp.Inspector(_Store(rank), device="cuda:0", near_candidates=8, near_two_bins=True, near_parts_two_bins=True, **BASE)


def test_inspector_unset_means_untouched():
    cuts = [float(i) for i in range(209)]
    corpus = _OldCorpus()
    ins = _inspector(corpus, near_parts=2, **BASE)
    assert ins.near_parts_two_bins is False
    (near,) = ins._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["align_span_topk", "align_parts"]
    assert all("two_bins" not in kw for _, kw in corpus.calls)
    assert [p["shift_seconds"] for p in near["parts"]] == [PART0[0] * ins.near_eps, PART1[0] * ins.near_eps]
    corpus = _OldCorpus()
    (near,) = _inspector(corpus, near_candidates=8, **BASE)._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates", "align_parts"]
    assert all("two_bins" not in kw for _, kw in corpus.calls) and near["shift_seconds"] == PART0[0] * (1 / 30)


def test_inspector_calls_under_the_new_option():
    cuts = [float(i) for i in range(209)]
    on = dict(near_two_bins=True, near_parts_two_bins=True)
    # the sweep under the flag, then the parts call with two_bins: every shift is a window's middle
    corpus = _Corpus()
    ins = _inspector(corpus, near_parts=2, **on, **BASE)
    (near,) = ins._near(7, cuts)
    (n0, k0), (n1, k1) = corpus.calls
    assert (n0, n1) == ("align_span_topk", "align_parts") and k0["two_bins"] is True and k1["two_bins"] is True
    assert k1["max_parts"] == 2 and k1["min_votes"] == 2 and k1["rates"] == (1.0,)
    assert near["shift_seconds"] == (PART0[0] + 0.5) * ins.near_eps
    assert [p["shift_seconds"] for p in near["parts"]] == [(PART0[0] + 0.5) * ins.near_eps, (PART1[0] + 0.5) * ins.near_eps]
    assert near["parts"][1]["upload_span"] == [0.0, 99.0]
    assert near["parts"][1]["stored_span"] == [0.0 + (PART1[0] + 0.5) * ins.near_eps, 99.0 + (PART1[0] + 0.5) * ins.near_eps]
    assert near["parts_score"] == 1.0
    # the candidates, then the parts call with two_bins; the report from part 0 at the window's middle
    for more, P in ((dict(), 1), (dict(near_parts=2), 2)):
        corpus = _Corpus()
        ins = _inspector(corpus, near_candidates=8, **on, **BASE, **more)
        (near,) = ins._near(7, cuts)
        assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates", "align_parts"]
        kw = corpus.calls[-1][1]
        assert kw["two_bins"] is True and kw["max_parts"] == P
        assert near["video_id"] == 20 and near["shift_seconds"] == (PART0[0] + 0.5) * ins.near_eps and near["local"] == 1.0
        assert near["upload_span"] == [109.0, 208.0]
        assert near["stored_span"] == [109.0 + near["shift_seconds"], 208.0 + near["shift_seconds"]]
        assert ("parts" in near) == (P == 2)
        if P == 2:
            assert [p["shift_seconds"] for p in near["parts"]] == [(PART0[0] + 0.5) * ins.near_eps, (PART1[0] + 0.5) * ins.near_eps]
    # with the rates of the candidates: the same, through align_candidates_rates
    corpus = type("Rated", (_Corpus,), {"supports_align_candidate_rates": True, "supports_align_rates": True,
                                        "align_rates_topk": _Corpus.align_topk, "align_candidates_rates": lambda self, q, **kw: (
        self.calls.append(("align_candidates_rates", dict(kw))) or np.array([[20, -1]]), None, None, np.array([1]))})()
    ins = _inspector(corpus, near_candidates=8, near_rates=(1.0, 0.96), near_candidate_rates=True, **on, **BASE)
    (near,) = ins._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates_rates", "align_parts"]
    assert corpus.calls[-1][1]["two_bins"] is True and corpus.calls[-1][1]["rates"] == (1.0, 0.96)
    # a refused upload falls back to the configured two-bin sweep
    corpus = _Corpus(refuse_candidates=True)
    ins = _inspector(corpus, near_candidates=8, **on, **BASE)
    (near,) = ins._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates", "align_span_topk"]
    assert corpus.calls[-1][1]["two_bins"] is True and near["shift_seconds"] == (PART0[0] + 0.5) * ins.near_eps


def test_the_corpus_calls_the_old_export_with_the_old_arguments_unless_asked(monkeypatch):
    """DeviceCorpus.align_parts_block and corpus.align_parts_shards: two_bins=False is tvz_align_parts with its 19 (21)
    arguments, True is tvz_align_parts_flags with ALIGN_TWO_BINS behind max_parts."""
    import inspect
    for fn in (tc.DeviceCorpus.align_parts, tc.DeviceCorpus.align_parts_block, tc.align_parts_shards, service.ShardedCorpus.align_parts):
        assert inspect.signature(fn).parameters["two_bins"].default is False, fn
    src = inspect.getsource(tc.DeviceCorpus.align_parts_block)
    assert "tvz_align_parts_flags(*front, ALIGN_TWO_BINS, *back)" in src and "tvz_align_parts(*front, *back)" in src
    src = inspect.getsource(tc.align_parts_shards)
    assert "tvz_align_parts_flags_shards(*front, ALIGN_TWO_BINS, *back)" in src and "tvz_align_parts_shards(*front, *back)" in src


# -------------------------------------------------------------------------------------------- 5. the code object
def test_the_new_walk_kernel_beside_its_sibling(kernels):  # noqa: F811
    """At DESIGN.md 4.14's own accounting a 200-value query's LDS allows four blocks per CU, four waves per SIMD: the
    walk may use 512 / 4 = 128 VGPRs without costing occupancy."""
    (k,) = [k for n, k in kernels.items() if NEW in n]
    (s,) = [k for n, k in kernels.items() if SIBLING in n]
    print("vgprs, sgprs:", k[".vgpr_count"], k[".sgpr_count"], "sibling:", s[".vgpr_count"], s[".sgpr_count"])
    assert k[".vgpr_count"] <= 128
    assert k[".private_segment_fixed_size"] == 0
    assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0
    assert k[".group_segment_fixed_size"] == s[".group_segment_fixed_size"]
    assert k[".max_flat_workgroup_size"] == s[".max_flat_workgroup_size"] == 256 and k[".wavefront_size"] == 64
    assert [a.get(".size") for a in k[".args"]] == [a.get(".size") for a in s[".args"]]        # one argument list


# ------------------------------------------------------------------------------------ 6. the host code, sanitized
def _program():
    sources = sorted(os.path.join(tbuild.CSRC, f) for f in os.listdir(tbuild.CSRC)) + \
        [os.path.join(tbuild.INCLUDE, h) for h in sorted(os.listdir(tbuild.INCLUDE))] + [MAIN]
    h = hashlib.sha1()
    for f in sources:
        h.update(open(f, "rb").read())
    cache = os.path.join(tempfile.gettempdir(), f"tvz-host-sanitizer-{os.getuid()}")
    os.makedirs(cache, exist_ok=True)
    exe = os.path.join(cache, "parts-flags-" + h.hexdigest()[:16])
    if not os.path.exists(exe):
        # (the device half is compiled because the translation unit registers its kernels; unoptimised: it never runs)
        subprocess.check_call([tbuild._hipcc(), f"--offload-arch={tbuild.ARCH}", "-O1", "-Xarch_device", "-O0", "-std=c++17",
                               "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                               "-Wno-unused-function", f"-I{tbuild.INCLUDE}", f"-I{tbuild.CSRC}", "-o", exe + f".{os.getpid()}.tmp",
                               MAIN, os.path.join(tbuild.CSRC, "tvz_api.hip"), "-ldl"])
        os.replace(exe + f".{os.getpid()}.tmp", exe)
    return exe


def test_the_flag_check_the_early_checks_order_and_the_carving_under_asan_and_ubsan():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([_program()], capture_output=True, text=True, timeout=300, env=env, stdin=subprocess.DEVNULL)
    assert out.returncode == 0 and out.stdout.strip() == "HOST_OK", (out.stdout, out.stderr[-3000:])
