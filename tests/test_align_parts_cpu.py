"""tvz_align_parts without a GPU: the reference of tests/align_parts_ref.py against exact rational arithmetic and against
the span reference, the premises of the cases the GPU tests run (tests/align_parts_cases.py), the binding's table
against the header, the refusals that come before anything touches a device, the inspector's argument checks and
report fields against a fake corpus, the gfx950 code objects read with the metadata readers of
tests/test_codeobj_cpu.py, and the workspace's sizing and carving in a stand-alone host program under AddressSanitizer
and UndefinedBehaviorSanitizer."""
import ctypes as C
import hashlib
import math
import os
import re
import shutil
import subprocess
import tempfile
from fractions import Fraction as F

import numpy as np
import pytest

from tests import align_parts_cases as cs, align_parts_ref as apr, align_ref as ar, align_span_ref as asr
from tests.test_align_rates_cpu import _exact_bin, _prototype
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)
from tvidz_amd import _lib, build as tbuild, corpus as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tvz.h")
MAIN = os.path.join(ROOT, "tests", "align_parts_host_main.hip")
EXPORTS = ("tvz_align_parts_workspace_bytes", "tvz_align_parts")
NEW = ("23ts_alignp_locate_kernelE", "21ts_alignp_walk_kernelE", "21ts_alignp_pick_kernelE")
EPS = cs.EPS
MAX_B = 1 << 22
INT32_MIN = -(1 << 31)


# ------------------------------------------------------------------------------------------------ the reference
_EXACT = {}


def _pairs_exact(keys, query, rho):
    """-> {(key index, t): bin} in rational arithmetic, over the pairs that vote at all (finite bins); kept per case"""
    at = (id(keys), id(query), rho)
    if at not in _EXACT:
        _EXACT[at] = _pairs_exact_once(keys, query, rho)
    return _EXACT[at]


def _pairs_exact_once(keys, query, rho):
    c, s = ar.row_set(keys), asr.sorted_query(query)
    out = {}
    for i, ci in enumerate(c.tolist()):
        for t, x in enumerate(s.tolist()):
            if math.isinf(ci) or math.isinf(x):
                continue
            out[i, t] = _exact_bin(ci, x, rho, EPS)
    return c, s, out


def _parts_exact(keys, query, rates, B, min_votes, max_parts):
    """the contract again, over the dictionary of exact bins: no matrix, no numpy"""
    def best(pairs):
        votes = {}
        for b in pairs.values():
            if -B <= b <= B:
                votes[b] = votes.get(b, 0) + 1
        return min(((-v, abs(b), b) for b, v in votes.items()), default=(0, 0, 0))
    per_rate = [_pairs_exact(keys, query, rho) for rho in rates]
    rate = min(range(len(rates)), key=lambda i: (best(per_rate[i][2])[0], i))
    c, s, pairs = per_rate[rate]
    t_out, c_out, parts = set(), set(), []
    for _ in range(max_parts):
        allowed = {(i, t): b for (i, t), b in pairs.items() if i not in c_out and t not in t_out}
        nv, _, bn = best(allowed)
        if -nv < min_votes:
            break
        at = [(i, t) for (i, t), b in allowed.items() if b == bn]
        t_range = set(range(min(t for _, t in at), max(t for _, t in at) + 1))
        i_range = set(range(min(i for i, _ in at), max(i for i, _ in at) + 1))     # the keys are sorted: an index range
        parts.append((bn, -nv, min(t_range), max(t_range), len(t_range - t_out), len(i_range - c_out)))
        t_out |= t_range
        c_out |= i_range
    return len(c), rate, parts


def test_reference_parts_equal_exact_rational_arithmetic_and_every_bin_of_the_cases_is_unambiguous():
    rows, uploads = cs.table(), cs.uploads()
    by_id = {}
    for vid, keys in rows:
        by_id.setdefault(vid, keys)                                               # the first row of an id
    cases = [("inserted", cs.FILM, (1.0,)), ("removed", cs.FILM, (1.0,)), ("two_inserted", cs.FILM, (1.0,)),
             ("swapped", cs.FILM, (1.0,)), ("exact", cs.FILM, (1.0,)), ("unrelated", cs.FILM, (1.0,)),
             ("fps_inserted", cs.FILM, (1.0, 0.96)), ("fps_inserted", cs.FILM, (0.96, 1.0)), ("special", cs.SPECIAL, (1.0,)),
             ("parts24", cs.LANES65, (1.0,)), ("tie30", cs.LATER_TIE, (1.0, 0.96))]
    for name, vid, rates in cases:
        for B, min_votes, max_parts in ((MAX_B, 1, 4), (5000, 8, 3), (900, 1, 2)):
            got = apr.row_parts(by_id[vid], uploads[name], EPS, B * EPS, rates, min_votes, max_parts)
            row_len, rate, parts = _parts_exact(by_id[vid], uploads[name], rates, B, min_votes, max_parts)
            assert (got[0], got[1], got[3]) == (row_len, rate, parts), (name, vid, rates, B)
    # the film's grid: no pair of a film key and a cut of an upload made from it lies near a bin's edge, so no rounding
    # of the device's can move a vote - (c - x) / eps + 0.5, exactly, is at least a twentieth of a bin from an integer
    # (the film's own cuts lie in the middle of their bins, the foreign ones a tenth of a bin from an edge)
    film = by_id[cs.FILM]
    for name in ("inserted", "removed", "two_inserted", "swapped", "exact"):
        for c in film[::7]:
            for x in uploads[name]:
                v = (F(c) - F(x)) / F(EPS) + F(1, 2)
                assert abs(v - round(v)) > F(1, 20), (name, c, x)


def test_part_0_is_the_span_references_and_the_premises_of_the_cases_hold():
    rows, uploads = cs.table(), cs.uploads()
    assert len(rows) == 49 and len(cs.film()) == 120
    pair = lambda name, vid, B=MAX_B, rates=(1.0,), mv=1, P=4: \
        apr.pair_ref(rows, uploads[name], vid, EPS, B * EPS, rates, mv, P).tolist()        # noqa: E731
    # part 0 against tests/align_span_ref.py, row by row, for every id the table holds once
    once = [(v, k) for v, k in rows if sum(1 for w, _ in rows if w == v) == 1]
    for name in ("inserted", "fps_inserted", "parts24", "special"):
        a = asr.align_span_ref(once, uploads[name], EPS, MAX_B * EPS, (1.0, 0.96))
        for (vid, _), hit in zip(once, a.tolist()):
            got = apr.pair_ref(rows, uploads[name], vid, EPS, MAX_B * EPS, (1.0, 0.96), 1, 1).tolist()
            if hit[3] == 0:
                assert got == [[vid, hit[1], 0, 0, 1, got[0][5]], [0] * 6]
            else:
                assert got == [[vid, hit[1], hit[4], 1, 1, got[0][5]],
                               [hit[2], hit[3], hit[5], hit[6], hit[6] - hit[5] + 1, hit[7]]], (name, vid)
    # an ad put in: the halves tie at 60 votes, part 0 is the smaller |bin|; out of the second half's reach at B = 900
    assert pair("inserted", cs.FILM)[:3] == [[cs.FILM, 120, 0, 2, 1, 129], [0, 60, 0, 59, 60, 60], [-1419, 60, 69, 128, 60, 60]]
    assert pair("inserted", cs.FILM, B=900)[1] == [0, 60, 0, 59, 60, 60] and pair("inserted", cs.FILM, B=900)[2][1] < 8
    assert pair("inserted", cs.FILM, mv=61)[0][3] == 0 and pair("inserted", cs.FILM, mv=8)[0][3] == 2
    assert pair("inserted", cs.FILM, P=1)[0][3] == 1
    # a scene taken out: the larger part first; two insertions: three parts; two clips in swapped order; the copy
    assert [p[1] for p in pair("removed", cs.FILM)[1:3]] == [50, 40] and pair("removed", cs.FILM)[2][0] == 0
    assert [p[:2] for p in pair("two_inserted", cs.FILM)[1:4]] == [[0, 40], [-600, 40], [-1419, 40]]
    sw = pair("swapped", cs.FILM)
    assert sw[0][3] == 2 and [p[1:4] for p in sw[1:3]] == [[40, 0, 39], [40, 40, 79]] and sw[1][0] > 0 > sw[2][0]
    assert pair("exact", cs.FILM)[:2] == [[cs.FILM, 120, 0, 1, 1, 120], [0, 120, 0, 119, 120, 120]]
    assert pair("unrelated", cs.FILM, mv=8)[0][3] == 0
    # 24 -> 25 fps with an insertion: found at the rate 0.96 wherever it stands in the list, chance pairs without it
    for rates, index in (((1.0, 0.96), 1), ((0.96, 1.0), 0)):
        p = pair("fps_inserted", cs.FILM, rates=rates)
        assert p[0][:4] == [cs.FILM, 120, index, 2] and [x[:2] for x in p[1:3]] == [[360, 60], [-1059, 60]]
    assert pair("fps_inserted", cs.FILM)[1][1] < 8
    # the rows of 65, 513 and 700 keys: two parts of 12; silent keys inside the key ranges (nr > votes); the voters of
    # the 700-key row lie beyond the 512 resume positions
    for vid, n in ((cs.LANES65, 65), (cs.LANES513, 513), (cs.LONG700, 700)):
        p = pair("parts24", vid)
        assert p[0] == [vid, n, 0, 2, 1, 24] and [x[:4] for x in p[1:3]] == [[cs.BIN_A, 12, 0, 11], [cs.BIN_B, 12, 12, 23]]
        assert p[1][5] > 12 and p[2][5] > 12
    keys = ar.row_set(dict((v, k) for v, k in rows)[cs.LONG700])
    assert (keys < cs.x24()[0] + cs.BIN_A * EPS).sum() > 512
    # two bins of equal votes in a later part: the negative one first
    assert pair("tie30", cs.LATER_TIE)[:4] == [[cs.LATER_TIE, 30, 0, 3, 1, 30], [0, 14, 0, 13, 14, 14], [-50, 8, 22, 29, 8, 8],
                                               [50, 8, 14, 21, 8, 8]]
    # rows sharing an id: the better second one; the earlier of two equal ones; nine are refused with their count
    assert pair("parts24", cs.SECOND_BETTER)[:2] == [[cs.SECOND_BETTER, 10, 0, 1, 2, 24], [30, 10, 2, 11, 10, 10]]
    assert pair("parts24", cs.EQUAL_ROWS, B=5000)[:2] == [[cs.EQUAL_ROWS, 12, 0, 1, 2, 24], [-7, 8, 4, 11, 8, 8]]
    assert pair("parts24", cs.NINE_ROWS) == [[cs.NINE_ROWS, 0, 0, INT32_MIN, 9, 24]] + [[0] * 6] * 4
    assert pair("parts24", cs.ABSENT)[0] == [cs.ABSENT, 0, 0, 0, 0, 24] and pair("parts24", -1)[0] == [-1, 0, 0, 0, 0, 24]
    # NaN, both infinities, both zeros, duplicates at a part's ends: m = 13, the three zeros and the two nines all vote
    assert pair("special", cs.SPECIAL)[:3] == [[cs.SPECIAL, 9, 0, 2, 1, 13], [40, 6, 1, 6, 6, 3], [-15, 5, 7, 11, 5, 3]]


def test_the_shards_merge_of_the_reference():
    a = np.zeros((3, 1, 4, 3, 6), dtype=np.int64)
    a[:, 0, :, 0, 0] = 7
    a[1, 0, 0, 0] = (7, 10, 0, 1, 1, 24)                                           # pair 0: only shard 1 holds a row
    a[1, 0, 0, 1] = (5, 9, 0, 8, 9, 9)
    a[0, 0, 1, 0], a[0, 0, 1, 1] = (7, 10, 0, 1, 2, 24), (5, 9, 0, 8, 9, 9)       # pair 1: a tie, the lower shard
    a[2, 0, 1, 0], a[2, 0, 1, 1] = (7, 11, 0, 1, 1, 24), (6, 9, 0, 8, 9, 9)
    a[0, 0, 2, 0] = (7, 10, 0, 0, 1, 24)                                           # pair 2: no part anywhere, a holder wins
    a[2, 0, 3, 0] = (7, 0, 0, INT32_MIN, 9, 24)                                    # pair 3: refused by one shard
    a[1, 0, 3, 0], a[1, 0, 3, 1] = (7, 10, 0, 1, 1, 24), (5, 9, 0, 8, 9, 9)
    exp = apr.merge_shards_ref(a)
    assert exp[0, 0].tolist() == a[1, 0, 0].tolist()
    assert exp[0, 1, 0].tolist() == [7, 10, 0, 1, 3, 24] and exp[0, 1, 1].tolist() == [5, 9, 0, 8, 9, 9]
    assert exp[0, 2, 0].tolist() == [7, 10, 0, 0, 1, 24]
    assert exp[0, 3].tolist() == [[7, 0, 0, INT32_MIN, 10, 24], [0] * 6, [0] * 6]
    assert (tc.align_parts_merge(a.astype(np.int32)) == exp).all()


# ------------------------------------------------------------------------------------------------- the C ABI
def test_both_exports_are_in_the_library_and_match_the_header():
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    defined = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", tbuild.SO], text=True).splitlines()
               if ln.strip()}
    assert set(EXPORTS) <= defined, sorted(set(EXPORTS) - defined)
    text = open(HEADER).read()
    for name in EXPORTS:
        assert _lib.SIGNATURES[name] == _prototype(text, name), name
    assert re.search(r"^#define TVZ_ALIGN_MAX_PARTS 4\b", text, re.M) and tc.ALIGN_MAX_PARTS == apr.MAX_PARTS == 4
    assert re.search(r"^#define TVZ_ALIGN_PARTS_MAX_ROWS 8\b", text, re.M) and tc.ALIGN_PARTS_MAX_ROWS == apr.MAX_ROWS == 8
    assert _lib.VERSION == 404 and _lib.load().tvz_version() == 404                # new exports only


def test_the_workspace_formula_of_the_header():
    lib = _lib.load()
    for Q, L, keys, k, P in ((1, 200, 0, 16, 4), (16, 4095, 0, 64, 1), (70, 40, 1234, 1, 2), (1, 0, 0, 1, 3), (0, 10, 0, 4, 4)):
        total = keys if keys > 0 else Q * L
        raw = lib.tvz_match_tol_workspace_bytes(Q, L, max(total, L)) + Q * k * (4 + 8 * 8 + 8 * (1 + P) * 24)
        got = tc.align_parts_workspace_bytes(Q, L, keys, k, P)
        assert raw <= got < raw + 4 * 256, (Q, L, keys, k, P, got, raw)
    for bad in ((-1, 10, 0, 1, 1), (1, -1, 0, 1, 1), (1, 10, -1, 1, 1), (1, 10, 0, 0, 1), (1, 10, 0, 1, 0), (1, 10, 0, 1, 5)):
        assert tc.align_parts_workspace_bytes(*bad) == 0, bad


def test_refusals_that_need_no_device():
    """Every parameter is refused before the handle is looked at - with a NULL handle's refusal behind them, so the order
    shows in the message - in the span call's order and words: the rate list, min_votes, k, the query limit; then
    max_parts, then the bins."""
    lib = _lib.load()
    good = (C.c_double * 2)(1.0, 0.96)

    def call(rates=good, n=2, k=16, L=4, min_votes=1, max_parts=2, eps=1 / 30, mo=1.0):
        rc = lib.tvz_align_parts(None, None, None, 1, L, None, 1, k, k, eps, mo, rates, n, min_votes, max_parts, None, None, 0, None)
        return rc, lib.tvz_last_error()

    def span(rates=good, n=2, k=16, L=4, min_votes=1, eps=1 / 30, mo=1.0):
        rc = lib.tvz_align_span_topk(None, None, None, 1, L, eps, mo, rates, n, min_votes, 0, 0, None, k, None, None, 0, None)
        return rc, lib.tvz_last_error()

    words = lambda m: m.split(b": ", 1)[1]                                         # noqa: E731  (behind the call's name)
    for kw in (dict(n=0), dict(rates=(C.c_double * 9)(*[1.0] * 9), n=9), dict(rates=None, n=1),
               dict(rates=(C.c_double * 2)(1.0, float("nan"))), dict(rates=(C.c_double * 2)(1.0, 0.0))):
        assert call(**kw) == span(**kw) and call(**kw)[0] != 0, kw                 # the rate list: the same words
    for kw in (dict(min_votes=0), dict(k=0), dict(k=65), dict(L=4096)):
        (rc, msg), (src, smsg) = call(**kw), span(**kw)
        assert rc == src != 0 and msg.startswith(b"alignment parts: ") and words(msg) == words(smsg), (kw, msg, smsg)
    for kw in (dict(eps=0.0), dict(eps=-1.0), dict(mo=-1.0), dict(mo=float("inf")), dict(mo=float("nan")),
               dict(mo=(MAX_B + 1) / 30)):
        # the span call looks at the handle before the bins: run with a handle it says the same (the GPU tests); here the
        # words are pinned
        rc, msg = call(**kw)
        assert rc in (ar.ERR_INVALID, ar.ERR_UNSUPPORTED) and (b"eps must be > 0" in msg or b"TVZ_ALIGN_WIDE_MAX_B" in msg), (kw, msg)
    for P in (0, 5, -1):
        rc, msg = call(max_parts=P)
        assert rc == ar.ERR_UNSUPPORTED and b"max_parts=%d outside 1..4 (TVZ_ALIGN_MAX_PARTS)" % P in msg
    # the order: rates, then min_votes, then k, then the query limit, then max_parts, then the bins, then the handle
    assert b"rate 1" in call(rates=(C.c_double * 2)(1.0, -1.0), min_votes=0, k=0, L=4096, max_parts=0, eps=0.0)[1]
    assert b"min_votes 0" in call(min_votes=0, k=0, L=4096, max_parts=0, eps=0.0)[1]
    assert b"k=0" in call(k=0, L=4096, max_parts=0, eps=0.0)[1]
    assert b"max_query_len 4096" in call(L=4096, max_parts=0, eps=0.0)[1]
    assert b"max_parts=0" in call(max_parts=0, eps=0.0)[1]
    assert b"eps must be > 0" in call(eps=0.0)[1]
    rc, msg = call()
    assert rc == ar.ERR_INVALID and b"corpus is NULL" in msg
    rc, msg = call(mo=MAX_B / 30, max_parts=4, k=64, L=4095)
    assert rc == ar.ERR_INVALID and b"corpus is NULL" in msg


# ---------------------------------------------------------------------------------------------- the inspector
class _PartsCorpus:
    """one hit of 60 votes over the first half of 129 cuts; align_parts answers with two parts, or refuses the pair"""

    def __init__(self, refuse=False):
        self.refuse, self.calls = refuse, []

    def align(self, timestamps, eps=0.1, max_offset=60.0):
        return np.zeros((0, 5), dtype=np.int32)

    def align_topk(self, queries, **kw):
        return np.zeros((len(queries), kw["k"], 4), dtype=np.int32), np.zeros(len(queries), dtype=np.int32)

    align_wide_topk = align_rates_topk = align_topk

    def align_span_topk(self, queries, **kw):
        rows = np.zeros((len(queries), kw["k"], 8), dtype=np.int32)
        rows[:, :, 0] = -1
        rows[:, 0] = (42, 120, 0, 60, len(kw["rates"]) - 1, 0, 59, 60)
        return rows, np.ones(len(queries), dtype=np.int64)

    def align_parts(self, queries, video_ids, **kw):
        self.calls.append(dict(kw, video_ids=video_ids, Q=len(queries)))
        P = kw["max_parts"]
        out = np.zeros((len(queries), len(video_ids[0]), 1 + P, 6), dtype=np.int32)
        out[:, :, 0] = (42, 120, len(kw["rates"]) - 1, INT32_MIN if self.refuse else 2, 1, 129)
        if not self.refuse:
            out[:, :, 1] = (0, 60, 0, 59, 60, 60)
            out[:, :, 2] = (-1419, 58, 69, 128, 60, 60)
        return out


class _Store:
    def __init__(self, corpus):
        self.corpus = corpus

    def get_video_by_id(self, vid):
        return None


def test_inspector_parts_arguments_and_report_fields():
    from tvidz_amd import inspector as insp

    ok = dict(device="cuda:0", near_duplicates=True, near_top_k=8, near_any_offset=True, near_score="local", near_min_votes=8,
              near_jaccard=0.9)
    new = lambda corpus=None, **kw: insp.Inspector(_Store(corpus or _PartsCorpus()), **dict(ok, **kw))       # noqa: E731
    for bad in (1, 5, 0):
        with pytest.raises(ValueError, match="near_parts must be None or 2..4"):
            new(near_parts=bad)
    with pytest.raises(ValueError, match="near_score='local'"):
        new(near_parts=2, near_score="jaccard")
    with pytest.raises(ValueError, match="near_score='local'"):
        new(near_parts=2, near_score="containment")
    with pytest.raises(ValueError):
        new(near_parts=2, near_top_k=None)
    with pytest.raises(ValueError):
        new(near_parts=2, near_any_offset=False)
    corpus = _PartsCorpus()
    no_parts = type("NoParts", (), {n: getattr(corpus, n) for n in ("align", "align_topk", "align_wide_topk", "align_rates_topk",
                                                                    "align_span_topk")})
    with pytest.raises(RuntimeError, match="align_parts"):
        new(no_parts(), near_parts=2)
    cuts = [float(3 * i) for i in range(128, -1, -1)] + [float("nan")]             # unsorted, one NaN
    s = sorted(x for x in cuts if x == x)
    # unset: nothing changes, and the call is never made
    ins = new(corpus)
    (plain,) = ins._near(7, cuts)
    assert ins.near_parts is None and corpus.calls == [] and "parts" not in plain and "parts_score" not in plain
    # set: one call for the reported ids, with the search's eps, rates and min_votes
    ins = new(corpus, near_parts=3, near_rates=(1.0, 0.96))
    (near,) = ins._near(7, cuts)
    (call,) = corpus.calls
    assert call == dict(video_ids=[[42]], Q=1, eps=ins.near_eps, rates=(1.0, 0.96), min_votes=8, max_parts=3)
    assert {k: v for k, v in near.items() if k not in ("parts", "parts_score", "rate", "stored_span")} == \
        {k: v for k, v in plain.items() if k != "stored_span"}
    shift = -1419 * ins.near_eps
    assert near["parts"] == [
        {"shift_seconds": 0.0, "upload_span": [s[0], s[59]], "stored_span": [0.96 * s[0] + 0.0, 0.96 * s[59] + 0.0], "votes": 60},
        {"shift_seconds": shift, "upload_span": [s[69], s[128]], "stored_span": [0.96 * s[69] + shift, 0.96 * s[128] + shift],
         "votes": 58}]
    assert near["parts_score"] == round(118 / (240 - 118), 4)
    # a refused pair leaves the entry without the fields
    (near,) = new(_PartsCorpus(refuse=True), near_parts=2)._near(7, cuts)
    assert near == plain


# -------------------------------------------------------------------------------------------- the code objects
def test_the_three_kernels_exist_once_with_no_scratch_and_no_spills(kernels):  # noqa: F811
    for name in NEW:
        found = [k for n, k in kernels.items() if name in n]
        assert len(found) == 1, (name, sorted(n for n in kernels if "alignp" in n))
        (k,) = found
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (name, k)
        assert k[".max_flat_workgroup_size"] == 256
    # the walk has no static LDS of its own: its dynamic part is the sweep's, at most 4,095 values and one window of
    # 4,096 bins per wave, inside a workgroup's 160 KiB
    (k,) = [k for n, k in kernels.items() if NEW[1] in n]
    assert k[".group_segment_fixed_size"] + 4095 * 8 + 4 * (4096 * 6 + 4) <= 160 * 1024


# ------------------------------------------------------------------------------------ the host code, sanitized
def _program():
    sources = sorted(os.path.join(tbuild.CSRC, f) for f in os.listdir(tbuild.CSRC)) + [os.path.join(tbuild.INCLUDE, "tvz.h"), MAIN]
    h = hashlib.sha1()
    for f in sources:
        h.update(open(f, "rb").read())
    cache = os.path.join(tempfile.gettempdir(), f"tvz-host-sanitizer-{os.getuid()}")
    os.makedirs(cache, exist_ok=True)
    exe = os.path.join(cache, "parts-" + h.hexdigest()[:16])
    if not os.path.exists(exe):
        # (the device half is compiled because the translation unit registers its kernels; unoptimised: it never runs)
        subprocess.check_call([tbuild._hipcc(), f"--offload-arch={tbuild.ARCH}", "-O1", "-Xarch_device", "-O0", "-std=c++17",
                               "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                               "-Wno-unused-function", f"-I{tbuild.INCLUDE}", f"-I{tbuild.CSRC}", "-o", exe + f".{os.getpid()}.tmp",
                               MAIN, os.path.join(tbuild.CSRC, "tvz_api.hip"), "-ldl"])
        os.replace(exe + f".{os.getpid()}.tmp", exe)
    return exe


def test_sizing_and_carving_under_asan_and_ubsan():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([_program()], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.strip() == "HOST_OK", (out.stdout, out.stderr[-3000:])
