"""tvz_align_candidates without a GPU: the reference's properties, the premises of the cases, the new header against the
second signature table and the library's exports, every refusal that needs no device, the Inspector option against a
fake corpus, the three new code objects, and the host code under ASan + UBSan in a stand-alone program."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from tests import gap_candidates_cases as cs, gap_candidates_ref as ref
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)
from tvidz_amd import _lib, build as tbuild, corpus as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tvz_gap.h")
MAIN = os.path.join(ROOT, "tests", "gap_candidates_host_main.hip")
NEW = ("22ts_gapc_offsets_kernelE", "20ts_gapc_probe_kernelE", "21ts_gapc_select_kernelE")
EPS = cs.GAP_EPS
ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -4, -5
INT32_MIN = -(1 << 31)


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_equals_the_plain_double_loop():
    rows = cs.table()
    named = (cs.FILM, cs.TWIN, cs.WIDE_GAP, cs.SPECIAL_ROW, cs.ROW0, cs.ROW1, cs.ROW3, cs.ROW4)
    small = [r for r in rows if r[0] in named or 1000 <= r[0] < 1006]
    up = cs.uploads()
    names = ("shifted", "special", "four", "twin", "wide_gap", "excerpt", "three", "empty")
    queries = [up[n] for n in names]
    for c, min_count, excl in ((4, 1, None), (2, 2, [cs.FILM] * len(names)), (1, 6, None)):
        a = ref.candidates(small, queries, EPS, c, min_count=min_count, exclude_ids=excl)
        b = ref.candidates_loops(small, queries, EPS, c, min_count=min_count, exclude_ids=excl)
        assert (a == b).all(), (c, min_count)
    assert int(a[0, 0, 1]) == 117                                                 # (the film, min_count 6, not excluded)


def test_shift_invariance_and_the_half_bin_guarantee():
    """A copy shifted by any amount whose every gap moved by less than gap_eps / 2 is probed at every stored position."""
    rng = np.random.default_rng(9)
    for trial in range(40):
        n = int(rng.integers(4, 60))
        eps = float(rng.choice([1 / 30, 0.0371, 0.1, 0.004]))
        s = np.cumsum(rng.uniform(0.02, 9.0, size=n)) + rng.uniform(0, 100)
        codes = ref.stored_codes(s, eps)
        shift = float(rng.choice([0.0, 3600.0, -17.25, 86400.0 * 3]))
        # every cut moves by less than eps / 4.1 either way: every gap by less than eps / 2 (and the shift's own
        # rounding, ulps of 3 days, is far inside the rest)
        moved = s + shift + rng.uniform(-eps / 4.1, eps / 4.1, size=n)
        p = [x for x in ref.probes(moved, eps) if x is not None]
        assert codes <= set(p), trial
        assert len(ref.probes(moved, eps)) == 8 * (n - 3)
        # count = one probe per stored position at least
        assert sum(1 for x in p if x in codes) >= len(codes)
    # shift invariance of the stored side, away from the edges: the same code set
    f = np.asarray(cs.film())
    assert ref.stored_codes(f, EPS) == ref.stored_codes(f + cs.HOUR, EPS) and len(ref.stored_codes(f, EPS)) == 117


def test_rows_of_0_3_and_4_keys_and_invalid_bins():
    assert ref.stored_codes([], EPS) == set() and ref.stored_codes([1.0, 2.0, 3.0], EPS) == set()
    assert ref.stored_codes([1.0, 2.0, 2.0, 3.0, float("nan")], EPS) == set()       # 3 distinct keys
    (one,) = ref.stored_codes([1.0, 2.5, 4.75, 8.125], EPS)
    b = [int(np.floor(g / EPS + 0.5)) for g in (1.5, 2.25, 3.375)]
    assert one == b[0] + (b[1] << 17) + (b[2] << 34) < 1 << 51
    assert ref.probes([1.0, 2.0, 3.0], EPS) == [] and len(ref.probes([1.0, 2.5, 4.75, 8.125], EPS)) == 8
    assert one in ref.probes([101.0, 102.5, 104.75, 108.125], EPS)
    # a gap beyond the last bin, an infinite one, inf - inf: no code, no probe
    wide = cs.wide_gap_row()
    assert len(ref.stored_codes(wide, EPS)) == 2 * 5 and ref.probes(wide, EPS).count(None) == 3 * 8
    assert ref.stored_codes([float("-inf"), 1.0, 2.0, 3.0, float("inf")], EPS) == set()
    assert all(x is None for x in ref.probes([float("-inf"), float("-inf"), 1.0, 2.0, float("inf"), float("inf")], EPS))
    # the last bin itself is valid on the stored side, and only as the lower choice on the query side
    g = cs.MAX_BIN * 0.25
    assert len(ref.stored_codes([0.0, g, g + 1.0, g + 2.0], 0.25)) == 1
    assert sum(x is not None for x in ref.probes([0.0, g, g + 1.0, g + 2.0], 0.25)) == 4
    # the refusals of the reference: 514 values pass, 515 do not; longer than max_query_len
    assert not ref.refused([0.0] * 514, 514) and ref.refused([0.0] * 515, 515) and ref.refused([0.0] * 5, 4)
    assert not ref.refused([0.0] * 514 + [float("nan")], 515)                      # (m counts: the NaN is skipped)


def test_the_premises_of_the_cases_hold():
    rows, up = cs.table(), cs.uploads()
    # no gap a premise depends on lies within 1e-6 bins of an edge, at either width
    for eps in (cs.GAP_EPS, cs.GAP_EPS_2):
        assert min(cs.edge_distance(k, eps, True) for _, k in rows) > 1e-6
        assert min(cs.edge_distance(q, eps, False) for q in up.values()) > 1e-6
    assert min(cs.edge_distance(k, EPS, True) for _, k in cs.counting_table(257)) > 1e-6
    assert cs.edge_distance(cs.counting_query(), EPS, False) > 1e-6
    assert {0, 1, 3, 4, 65, 513, 700} <= {len(ref.stored_values(k)) for _, k in rows}
    names = list(up)
    blk = ref.candidates(rows, [up[n] for n in names], EPS, 16, min_count=1)
    got = {n: b for n, b in zip(names, blk)}
    first = lambda n: tuple(int(x) for x in got[n][0])                            # noqa: E731
    total = lambda n: int(got[n][16, 1])                                           # noqa: E731
    # the copy, the jittered copies and the film backwards: every position; the excerpt: its 17; the insertion and the
    # removal lose only the positions across the edit
    for n in ("shifted", "jitter_small", "jitter_quarter", "unsorted"):
        assert first(n) == (cs.FILM, 117) and total(n) == 1, n
    assert first("excerpt") == (cs.FILM, 17) and first("inserted") == (cs.FILM, 114) and first("removed") == (cs.FILM, 85)
    assert total("stranger") == total("empty") == total("three") == 0
    assert first("row4") == (cs.ROW4, 1) and first("four") == (cs.FILM, 1)
    assert [tuple(int(x) for x in r) for r in got["twin"][:3]] == [(cs.TWIN, 16), (cs.TWIN, 16), (-1, 0)] and total("twin") == 2
    assert first("wide_gap")[0] == cs.WIDE_GAP and first("special") == (cs.SPECIAL_ROW, 2)
    # the counting table: H hits, counts 1..7 with ties that the ids decide, nothing from the rows behind them
    q = [cs.counting_query()]
    for H in cs.HIT_COUNTS:
        t = cs.counting_table(H)
        b = ref.candidates(t, q, EPS, 64, min_count=1)[0]
        assert int(b[64, 1]) == H < 4096
        want = sorted((-(1 + i % 7), vid) for i, (vid, _) in enumerate(t[:H]))[:64]
        assert [(-int(c), int(v)) for v, c in b[:len(want)]] == want
        assert len({vid for vid, _ in t}) == len(t)
        if H >= 17:
            assert int(b[0, 1]) == int(b[1, 1]) == 7 and int(b[0, 0]) < int(b[1, 0])      # a tie: id order
        six = ref.candidates(t, q, EPS, 64, min_count=6)[0]
        assert int(six[64, 1]) == sum(1 for i in range(H) if i % 7 >= 5)
    # the probe limit
    assert int(ref.candidates(rows, [cs.long_query(514, 1), cs.long_query(515, 2)], EPS, 4)[1, 4, 1]) == INT32_MIN
    # the scan case: more queries than the scan's block has threads, so that a thread has 3 lists and the last none; the
    # refused queries are a thread's first and a thread's last list; at least four different blocks, not padding alone
    t, queries, excl = cs.scan_case()
    per = -(-cs.SCAN_Q // 1024)
    assert per == 3 and cs.SCAN_LONG[0] % per == 0 and cs.SCAN_LONG[1] % per == per - 1 and cs.SCAN_LONG[1] == cs.SCAN_Q - 1
    assert {len(q) for q in queries} == {0, 3, 4, 5} and [i for i, q in enumerate(queries) if len(q) == 5] == list(cs.SCAN_LONG)
    assert set(excl) == {t[0][0], t[1][0], -1} and t[0][0] != t[1][0]
    exp, memo = cs.scan_expected(t, queries, excl)
    blocks = {tuple(v.ravel().tolist()) for v in memo.values()}
    assert len(blocks) >= 4, blocks
    both = sorted(v for v, _ in t[:2])
    assert memo[(4, -1)].tolist() == [[both[0], 1], [both[1], 1], [-1, 2]]
    assert memo[(4, both[0])].tolist() == [[both[1], 1], [-1, 0], [-1, 1]] and memo[(3, -1)].tolist() == [[-1, 0], [-1, 0], [-1, 0]]
    assert (exp[list(cs.SCAN_LONG), 2, 1] == INT32_MIN).all()


# ------------------------------------------------------------------------------------------------- the C ABI
def _kind(t):
    if t in (C.c_void_p, C.c_char_p) or isinstance(t, type) and issubclass(t, C._Pointer):
        return "pointer"
    return t


def _prototype(text, name):
    m = re.search(r"^(\w+)\s+" + name + r"\(([^;]*?)\);", text, re.M | re.S)
    assert m, name
    scalar = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "double": C.c_double,
              "size_t": C.c_size_t}

    def one(decl):
        decl = decl.strip()
        if "*" in decl or "[" in decl:
            return "pointer"
        return scalar[re.sub(r"\bconst\b", "", decl).split()[0]]
    return one(m.group(1)), [one(p) for p in m.group(2).split(",")]


def test_the_header_the_second_table_and_the_exports_agree():
    text = open(HEADER).read()
    declared = set(re.findall(r"^\w[\w ]*?\b(tvz_\w+)\(", text, re.M))
    assert declared == set(_lib.GAP_SIGNATURES) and len(declared) == 4
    for name, (res, args) in _lib.GAP_SIGNATURES.items():
        assert (_kind(res), [_kind(a) for a in args]) == _prototype(text, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    defined = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", tbuild.SO], text=True).splitlines()
               if ln.strip()}
    assert declared <= defined, sorted(declared - defined)
    lib = _lib.load()
    for name in declared:                                                          # load() bound the second table too
        assert getattr(lib, name).argtypes == _lib.GAP_SIGNATURES[name][1]
    # new exports only: the first table, its header and the version are what they were
    assert len(_lib.SIGNATURES) == 75 and not declared & set(_lib.SIGNATURES)
    assert _lib.VERSION == 404 and lib.tvz_version() == 404
    main = open(os.path.join(ROOT, "include", "tvz.h")).read()
    assert re.search(r"^#define TVZ_VERSION 404\b", main, re.M) and "tvz_gap" not in main and "tvz_align_candidates" not in main
    assert re.search(r"^#define TVZ_GAP_MAX_BIN 131071\b", text, re.M) and ref.MAX_BIN == cs.MAX_BIN == 131071
    assert re.search(r"^#define TVZ_GAP_MAX_PROBES 4095\b", text, re.M) and tc.ALIGN_CANDIDATES_MAX_PROBES == ref.MAX_PROBES == 4095
    assert re.search(r"^#define TVZ_GAP_MAX_C 64\b", text, re.M) and tc.ALIGN_CANDIDATES_MAX_C == 64
    assert tc.ALIGN_CANDIDATES_REFUSED == ref.REFUSED == INT32_MIN


def test_the_workspace_formula():
    lib = _lib.load()
    for Q, L, keys, cap, c in ((1, 200, 0, 4096, 16), (16, 514, 0, 64, 64), (70, 40, 1234, 17, 1), (1, 0, 0, 1, 1), (0, 10, 0, 4, 4)):
        total = max(keys if keys > 0 else Q * L, L)
        probe_len = min(8 * max(L - 3, 1), 4088)
        raw = Q * cap * 12 + 2 * Q * 4 + (Q + 1) * 8 + lib.tvz_match_workspace_bytes(Q, probe_len, 0, 0, 1) + total * (8 + 4 + 64)
        got = tc.align_candidates_workspace_bytes(Q, L, keys, cap, c)
        assert raw <= got < raw + 10 * 256, (Q, L, keys, cap, c, got, raw)
    for bad in ((-1, 10, 0, 16, 16), (1, -1, 0, 16, 16), (1, 10, -1, 16, 16), (1, 10, 0, 16, 0), (1, 10, 0, 16, 65),
                (1, 10, 0, 15, 16), (1, 4096, 0, 16, 16)):
        assert tc.align_candidates_workspace_bytes(*bad) == 0, bad


def test_refusals_that_need_no_device_and_their_order():
    """Every parameter is refused before the handle is looked at - a NULL handle's refusal stands behind them, so the
    order shows in the message: C, cap, min_count, max_query_len; then the handle."""
    lib = _lib.load()

    def call(C_=16, cap=64, min_count=2, L=4, ws=0):
        rc = lib.tvz_align_candidates(None, None, None, 1, L, min_count, None, cap, C_, None, None, ws, None)
        return rc, lib.tvz_last_error()

    for bad in (0, 65, -1):
        rc, msg = call(C_=bad)
        assert rc == ERR_UNSUPPORTED and msg == b"alignment candidates: C=%d outside 1..64" % bad
    rc, msg = call(cap=15)
    assert rc == ERR_UNSUPPORTED and msg == b"alignment candidates: cap=15 below C=16"
    for bad in (0, -3):
        rc, msg = call(min_count=bad)
        assert rc == ERR_INVALID and msg == b"alignment candidates: min_count %d below 1" % bad
    rc, msg = call(L=4096)
    assert rc == ERR_UNSUPPORTED and msg == b"alignment candidates: max_query_len 4096 above 4095"
    # the order, one step at a time
    assert b"C=0" in call(C_=0, cap=-1, min_count=0, L=4096)[1]
    assert b"cap=15" in call(cap=15, min_count=0, L=4096)[1]
    assert b"min_count 0" in call(min_count=0, L=4096)[1]
    assert b"max_query_len 4096" in call(L=4096)[1]
    rc, msg = call()
    assert rc == ERR_INVALID and b"corpus is NULL" in msg
    rc, msg = call(C_=64, cap=64, min_count=1, L=4095)
    assert rc == ERR_INVALID and b"corpus is NULL" in msg
    # the handle's switch and its statistics
    for bad in (-1.0, float("nan"), float("inf"), -0.001):
        assert lib.tvz_corpus_gap_index(None, bad) == ERR_INVALID
    assert lib.tvz_corpus_gap_index_stats(None, None, None) == ERR_INVALID


# ---------------------------------------------------------------------------------------------- the inspector
class _Corpus:
    """Five stored videos: the candidates call names three of them (or refuses), the parts call answers for each id it
    is asked about - id 42 aligns in two parts over 129 cuts, id 43 in one weak part, id 44 has no part; the span sweep
    reports id 42 alone."""

    def __init__(self, refuse=False):
        self.refuse, self.calls = refuse, []

    def set_gap_index(self, gap_eps):
        self.calls.append(("set_gap_index", gap_eps))

    def align(self, timestamps, eps=0.1, max_offset=60.0):
        self.calls.append(("align",))
        return np.zeros((0, 5), dtype=np.int32)

    def align_topk(self, queries, **kw):
        self.calls.append(("align_topk", kw))
        return np.zeros((len(queries), kw["k"], 4), dtype=np.int32), np.zeros(len(queries), dtype=np.int32)

    def align_wide_topk(self, queries, **kw):
        self.calls.append(("align_wide_topk", kw))
        rows = np.zeros((len(queries), kw["k"], 4), dtype=np.int32)
        rows[:, :, 0] = -1
        rows[:, 0] = (42, 120, 0, 60)
        return rows, np.ones(len(queries), dtype=np.int64)

    align_rates_topk = align_topk

    def align_span_topk(self, queries, **kw):
        self.calls.append(("align_span_topk", kw))
        rows = np.zeros((len(queries), kw["k"], 8), dtype=np.int32)
        rows[:, :, 0] = -1
        rows[:, 0] = (42, 120, 0, 60, 0, 0, 59, 60)
        return rows, np.ones(len(queries), dtype=np.int64)

    def align_candidates(self, queries, **kw):
        self.calls.append(("align_candidates", dict(kw, Q=len(queries))))
        c = kw["c"]
        rows = np.zeros((len(queries), c, 2), dtype=np.int32)
        rows[:, :, 0] = -1
        if self.refuse:
            return rows, np.full(len(queries), INT32_MIN, dtype=np.int32)
        rows[:, :3] = ((42, 57), (43, 9), (44, 2))
        return rows, np.full(len(queries), 3, dtype=np.int32)

    def align_parts(self, queries, video_ids, **kw):
        self.calls.append(("align_parts", dict(kw, video_ids=video_ids, Q=len(queries))))
        P = kw["max_parts"]
        out = np.zeros((len(queries), len(video_ids[0]), 1 + P, 6), dtype=np.int32)
        for j, vid in enumerate(video_ids[0]):
            if vid == 42:
                out[:, j, 0] = (42, 120, 0, min(P, 2), 1, 129)
                out[:, j, 1] = (0, 60, 0, 59, 60, 60)
                if P >= 2:
                    out[:, j, 2] = (-1419, 58, 69, 128, 60, 60)
            elif vid == 43:
                out[:, j, 0] = (43, 300, 0, 1, 1, 129)
                out[:, j, 1] = (7, 9, 3, 40, 38, 80)                                # local score 9 / 109
            else:
                out[:, j, 0] = (vid, 50, 0, 0, 1, 129)
        return out


class _Store:
    def __init__(self, corpus):
        self.corpus = corpus

    def get_video_by_id(self, vid):
        return None


def test_inspector_candidates_option_calls_refusals_fallback_and_unset():
    from tvidz_amd import inspector as insp

    ok = dict(device="cuda:0", near_duplicates=True, near_top_k=8, near_any_offset=True, near_score="local", near_min_votes=8,
              near_jaccard=0.9)
    new = lambda corpus=None, **kw: insp.Inspector(_Store(corpus or _Corpus()), **dict(ok, **kw))            # noqa: E731
    # every refused combination
    for bad in (7, 65, 0):
        with pytest.raises(ValueError, match=r"near_candidates must be None or near_top_k\.\.64"):
            new(near_candidates=bad)
    with pytest.raises(ValueError, match="near_candidates=16 needs"):
        new(near_candidates=16, near_any_offset=False, near_score="jaccard")
    with pytest.raises(ValueError):
        new(near_candidates=16, near_top_k=None)
    with pytest.raises(ValueError):
        insp.Inspector(_Store(_Corpus()), **dict(ok, near_duplicates=False, near_candidates=16))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="near_gap_eps"):
            new(near_candidates=16, near_gap_eps=bad)
    with pytest.raises(RuntimeError, match="near_candidates=16 with near_rates"):
        new(near_candidates=16, near_rates=(1.0, 0.96))
    with pytest.raises(RuntimeError, match="near_candidates=16 with near_two_bins=True"):
        new(near_candidates=16, near_two_bins=True)
    full = _Corpus()
    without = type("NoCandidates", (), {n: getattr(full, n) for n in ("align", "align_topk", "align_wide_topk", "align_rates_topk",
                                                                      "align_span_topk", "align_parts")})
    with pytest.raises(RuntimeError, match="has no align_candidates"):
        new(without(), near_candidates=16)
    cuts = [float(3 * i) for i in range(128, -1, -1)] + [float("nan")]             # unsorted, one NaN
    # unset: untouched - no switch, no candidates call, the sweep as before
    corpus = _Corpus()
    ins = new(corpus)
    (plain,) = ins._near(7, cuts)
    assert ins.near_candidates is None and [c[0] for c in corpus.calls] == ["align_span_topk"]
    # set: the switch once, at construction; per upload one candidates call and one parts call, no sweep
    corpus = _Corpus()
    ins = new(corpus, near_candidates=16, near_gap_eps=0.05)
    assert corpus.calls == [("set_gap_index", 0.05)]
    (near,) = ins._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates", "align_parts"]
    assert corpus.calls[1][1] == dict(c=16, exclude_ids=[7], Q=1)
    assert corpus.calls[2][1] == dict(video_ids=[[42, 43, 44]], Q=1, eps=ins.near_eps, rates=(1.0,), min_votes=8, max_parts=1)
    assert near == plain                                                           # the same entry as the sweep's
    ins._near(8, cuts)
    assert [c[0] for c in corpus.calls].count("set_gap_index") == 1
    # with near_parts: the entries' parts come from the same block, max_parts = near_parts, still one parts call
    swept = _Corpus()
    (want,) = new(swept, near_parts=3)._near(7, cuts)
    corpus = _Corpus()
    (near,) = new(corpus, near_candidates=8, near_parts=3)._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates", "align_parts"]
    assert corpus.calls[2][1]["max_parts"] == 3 and near == want and len(near["parts"]) == 2
    # a lower threshold lets the weak second candidate in, behind the first; near_top_k cuts the list
    got = new(_Corpus(), near_candidates=8, near_jaccard=0.05)._near(7, cuts)
    assert [d["video_id"] for d in got] == [42, 43] and got[1]["local"] == round(9 / 109, 4)
    got = new(_Corpus(), near_candidates=8, near_top_k=1, near_jaccard=0.05)._near(7, cuts)
    assert [d["video_id"] for d in got] == [42]
    # without spans the rows are the wide sweep's four columns: no span fields
    wide = dict(ok, near_score="jaccard", near_jaccard=0.3, near_min_votes=1)
    corpus = _Corpus()
    (near,) = insp.Inspector(_Store(corpus), **dict(wide, near_candidates=8))._near(7, cuts)
    (want,) = insp.Inspector(_Store(_Corpus()), **wide)._near(7, cuts)
    assert near == want and "upload_span" not in near
    # a refused upload takes the configured sweep
    corpus = _Corpus(refuse=True)
    (near,) = new(corpus, near_candidates=16)._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates", "align_span_topk"] and near == plain


# -------------------------------------------------------------------------------------------- the code objects
def test_the_new_kernels_exist_once_with_no_scratch_and_no_spills(kernels):  # noqa: F811
    recorded = {}
    for name in NEW:
        found = [k for n, k in kernels.items() if name in n]
        assert len(found) == 1, (name, sorted(n for n in kernels if "gapc" in n))
        (k,) = found
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (name, k)
        assert k[".wavefront_size"] == 64
        recorded[name] = (k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".max_flat_workgroup_size"])
    print("vgprs, sgprs, LDS bytes, block:", recorded)
    assert recorded[NEW[0]][3] == 1024 and recorded[NEW[1]][3] == 256 and recorded[NEW[2]][3] == 256
    # the selection's sort buffers: 2,048 keys and counts; the scan's one word per wave; the probes use no LDS
    assert recorded[NEW[2]][2] == 2048 * 12 and recorded[NEW[0]][2] == 64 and recorded[NEW[1]][2] == 0
    # registers, as the compiler reported them when the kernels were written (a rise is looked at, not forbidden); the
    # scan is the rates call's too and has its bound: it divides by the lists per query
    assert recorded[NEW[1]][0] <= 64 and recorded[NEW[2]][0] <= 64 and recorded[NEW[0]][0] <= 40
    # ... and there is ONE scan and ONE probe kernel: the rates call has no copies of its own
    for name in ("gapr_offsets", "gapr_probe"):
        assert not [n for n in kernels if name in n], name


# ------------------------------------------------------------------------------------ the host code, sanitized
def _program():
    sources = sorted(os.path.join(tbuild.CSRC, f) for f in os.listdir(tbuild.CSRC)) + \
        [os.path.join(tbuild.INCLUDE, "tvz.h"), HEADER, MAIN]
    h = hashlib.sha1()
    for f in sources:
        h.update(open(f, "rb").read())
    cache = os.path.join(tempfile.gettempdir(), f"tvz-host-sanitizer-{os.getuid()}")
    os.makedirs(cache, exist_ok=True)
    exe = os.path.join(cache, "gapc-" + h.hexdigest()[:16])
    if not os.path.exists(exe):
        # (the device half is compiled because the translation unit registers its kernels; unoptimised: it never runs)
        subprocess.check_call([tbuild._hipcc(), f"--offload-arch={tbuild.ARCH}", "-O1", "-Xarch_device", "-O0", "-std=c++17",
                               "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                               "-Wno-unused-function", f"-I{tbuild.INCLUDE}", f"-I{tbuild.CSRC}", "-o", exe + f".{os.getpid()}.tmp",
                               MAIN, os.path.join(tbuild.CSRC, "tvz_api.hip"), "-ldl"])
        os.replace(exe + f".{os.getpid()}.tmp", exe)
    return exe


def test_host_codes_and_carving_under_asan_and_ubsan():
    """The handle's code function over the edge rows - as the handle keeps them: canonical bit patterns sorted as
    integers, which puts negative values in descending order - equals the reference's code sets, and the workspace is
    carved inside its buffer at every misalignment."""
    rows = [k for _, k in cs.table()] + [
        [], [1.0], [1.0, 2.0, 3.0], [1.0, 2.5, 4.75, 8.125], [-9.0, -7.5, -3.25, -1.0, 0.0, 2.0, 7.0],
        [float("-inf"), -5.0, -2.0, 1.0, 3.0, 9.0, float("inf")], [-0.0, 0.0, 1.0, 2.0, 4.0, float("nan")],
        cs.wide_gap_row(), [0.0, cs.MAX_BIN * 0.25, cs.MAX_BIN * 0.25 + 1.0, cs.MAX_BIN * 0.25 + 2.0],
        [5e-324, 1e-310, 1.0, 2.0, 3.5], [1e300, 1.1e300, 1.3e300, 1.31e300]]
    for eps in (EPS, 0.25):
        lines = [float(eps).hex()]
        for k in rows:
            keys = np.sort(ref.stored_values(k).view(np.int64))
            lines.append(" ".join([str(keys.size)] + [str(int(x)) for x in keys]))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([_program()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0 and out.stdout.strip().endswith("HOST_OK"), (out.stdout[-500:], out.stderr[-3000:])
        got = [ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith("ROW")]
        assert len(got) == len(rows)
        for k, codes in zip(rows, got):
            assert {int(x) for x in codes} == ref.stored_codes(k, eps), k[:8]
            assert len(codes) <= max(len(ref.stored_values(k)) - 3, 0)
