"""tvz_align_candidates_long without a device: the reference's two forms against each other, the contract's two
consequences, the premises of the cases, the header against the binding's table, the refusals that need no device and
their order, the Inspector option on a fake corpus, the new kernels' code objects, and the host arithmetic in a
stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from tests import gap_candidates_cases as cs, gap_candidates_long_cases as lc, gap_candidates_long_ref as lref
from tests import gap_candidates_ref as ref
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)
from tests.test_gap_candidates_cpu import _Corpus, _Store, _kind, _prototype
from tvidz_amd import _lib, build as tbuild, corpus as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tvz_gap_long.h")
MAIN = os.path.join(ROOT, "tests", "gap_candidates_long_host_main.hip")
EPS = lc.GAP_EPS
INT32_MIN = -(1 << 31)
ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -4, -5           # include/tvz.h
NEW = ("ts_gapl_offsets_kernel", "ts_gapl_probe_kernel", "ts_gapl_fold_kernel")


@pytest.fixture(scope="module")
def world():
    return lc.table(), lc.uploads()


# ------------------------------------------------------------------------------------------------ the reference
def test_segments_at_the_thresholds():
    assert [lref.segments(m) for m in (3, 4, 514, 515, 1025, 1026, 4095)] == [0, 1, 1, 2, 2, 3, 9]
    assert [lref.lists_per_query(m) for m in (0, 3, 514, 515, 4095, 5000)] == [1, 1, 1, 2, 9, 9]


def test_reference_equals_the_plain_double_loop(world):
    rows, uploads = world
    queries = [uploads[n] for n in ("m515", "m1026", "short", "empty", "m4096")] + [cs.uploads()["special"]]
    excl = [-1, lc.ALL9, lc.TWIN, -1, -1, -1]
    for kw in (dict(c=4, min_count=1), dict(c=16, min_count=2, exclude_ids=excl), dict(c=2, min_count=3, cap=2),
               dict(c=3, min_count=1, max_query_len=1026)):
        a, b = lref.candidates(rows, queries, EPS, **kw), lref.candidates_loops(rows, queries, EPS, **kw)
        assert (a == b).all(), (kw, a.tolist(), b.tolist())
    # ... on the plain call's own table, with its NaN, infinities, doubled values and rows of one id
    rows2, u2 = cs.table(), cs.uploads()
    queries = [u2[n] for n in ("shifted", "special", "twin", "wide_gap", "four", "three")]
    a, b = lref.candidates(rows2, queries, EPS, 8, min_count=1), lref.candidates_loops(rows2, queries, EPS, 8, min_count=1)
    assert (a == b).all()


def test_one_segment_over_distinct_ids_is_the_plain_block(world):
    rows, uploads = world
    distinct = [(vid, k) for i, (vid, k) in enumerate(rows) if vid not in [v for v, _ in rows[:i]]]
    assert len({v for v, _ in distinct}) == len(distinct) < len(rows)
    queries = [uploads["m514"], uploads["short"], uploads["empty"], lc.master()[:4], lc.master()[:3]]
    for kw in (dict(min_count=1), dict(min_count=2, exclude_ids=[lc.ONE_SEG, -1, -1, -1, -1]), dict(min_count=1, cap=2)):
        for c in (1, 16):
            a, b = lref.candidates(distinct, queries, EPS, c, **kw), ref.candidates(distinct, queries, EPS, c, **kw)
            assert (a == b).all(), (kw, c)
    # with two rows of one id the plain block names the id twice and this one once, with the sum
    a, b = lref.candidates(rows, [uploads["m514"]], EPS, 16, min_count=1), ref.candidates(rows, [uploads["m514"]], EPS, 16, min_count=1)
    assert list(b[0, :16, 0]).count(lc.TWIN) == 2 and list(a[0, :16, 0]).count(lc.TWIN) == 1
    assert a[0, 16, 1] == b[0, 16, 1] - 1


def test_the_loss_against_the_whole_query_count_on_seeded_copies():
    """count_whole - S (min_count - 1) <= count_long <= count_whole, row by row (distinct ids)"""
    rng = np.random.default_rng(7)
    stored = cs.long_query(1400, 5)
    rows = [(1, stored)] + [(10 + i, cs.long_query(60, 100 + i)) for i in range(4)]
    hit_below = 0
    for trial in range(6):
        n = int(rng.integers(600, 1400))
        keep = np.sort(rng.choice(1400, size=n, replace=False))              # cuts dropped at random: short runs of hits
        q = (np.asarray(stored)[keep] + 1234.5).tolist()
        S = lref.segments(n)
        # ... and short excerpts of the upload itself, one of them across the first boundary: a few hits per segment
        starts = [507] + [int(x) for x in rng.integers(0, n - 12, size=12)]
        small = [(100 + j, (np.asarray(q[a:a + 5 + j % 6]) - 99.0).tolist()) for j, a in enumerate(starts)]
        rows = rows[:5] + small
        seg = lref.segment_counts(rows, q, EPS)
        whole = np.asarray(ref.counts(rows, q, EPS))
        assert (seg.sum(axis=0) == whole).all()
        for min_count in (1, 2, 3, 5):
            long_ = np.where(seg >= min_count, seg, 0).sum(axis=0)
            assert ((whole - S * (min_count - 1) <= long_) & (long_ <= whole)).all(), (trial, min_count)
            hit_below += int((long_ < whole).any())
    assert hit_below > 0                                                       # (the bound was exercised, not vacuous)


# ------------------------------------------------------------------------------------------------------ the cases
def test_the_premises_of_the_cases_hold(world):
    rows, uploads = world
    for _, k in rows:
        assert cs.edge_distance(k, EPS, stored=True) > 1e-6
    for q in uploads.values():
        assert cs.edge_distance(q, EPS, stored=False) > 1e-6
    m = uploads["m4095"]
    assert [lref.segments(len(uploads[f"m{n}"])) for n in lc.LENGTHS] == [1, 2, 2, 3, 9] and len(uploads["m4096"]) == 4096
    ids = [v for v, _ in rows]
    seg = lref.segment_counts(rows, m, EPS)
    by_id = lambda vid: seg[:, [i for i, v in enumerate(ids) if v == vid]]             # noqa: E731
    # the boundary row: one hit on either side
    assert by_id(lc.BOUNDARY)[:, 0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert by_id(lc.SPLIT)[:, 0].tolist() == [1, 2, 0, 0, 0, 0, 0, 0, 0]
    assert np.count_nonzero(by_id(lc.ONE_SEG)) == 1 and np.count_nonzero(by_id(lc.TWO_SEG)) == 2
    assert (by_id(lc.ALL9)[:, 0] >= 4).all()
    assert by_id(lc.TWIN).shape[1] == 3 and (by_id(lc.TWIN)[0, :2] > 0).all() and by_id(lc.TWIN)[2, 2] > 0
    assert by_id(lc.TIE_LO).sum() == by_id(lc.TIE_HI).sum() == 9 and lc.TIE_LO < lc.TIE_HI
    for s in lc.STRANGERS:
        assert by_id(s).sum() == 0
    full = {1: lref.candidates(rows, [m], EPS, 16, min_count=1)[0], 2: lref.candidates(rows, [m], EPS, 16, min_count=2)[0]}
    at = {k: {int(v): int(n) for v, n in b[:16] if v >= 0} for k, b in full.items()}
    assert at[1][lc.BOUNDARY] == 2 and lc.BOUNDARY not in at[2]
    assert at[1][lc.SPLIT] == 3 and at[2][lc.SPLIT] == 2
    assert at[1][lc.TWIN] == int(by_id(lc.TWIN).sum()) == 17 + 7 + 27
    order = [int(v) for v in full[1][:16, 0] if v >= 0]
    assert order.index(lc.TIE_LO) + 1 == order.index(lc.TIE_HI)
    assert full[1][16, 1] == 8 and full[2][16, 1] == 7
    # the lengths at the thresholds differ in what they reach
    b515 = lref.candidates(rows, [uploads["m514"], uploads["m515"], uploads["m4096"]], EPS, 16, min_count=1, max_query_len=4095)
    got = [{int(v): int(n) for v, n in b[:16] if v >= 0} for b in b515]
    assert got[0][lc.BOUNDARY] == 1 and got[1][lc.BOUNDARY] == 2 and b515[2, 16, 1] == INT32_MIN and not got[2]
    # the limit tables: every row counts 1
    q = lc.limit_query()
    t = lc.limit_table([5, 9, 77])
    assert ref.counts(t, q, EPS) == [1, 1, 1] and cs.edge_distance(q, EPS, stored=False) > 1e-6
    for n, slots in ((2048, 4096), (2049, 8192)):
        assert lc.table_slots(n) == slots
        v = lc.colliding_ids(n, slots, 3)
        assert len(set(v)) == n and [lc.home(x, slots) for x in v[:100]] == [slots - 3] * 100
    assert lc.table_slots(2047) == 4096 and lc.table_slots(1) == 2


# ------------------------------------------------------------------------------------------------- the C ABI
def test_the_header_the_table_and_the_exports_agree():
    text = open(HEADER).read()
    declared = set(re.findall(r"^\w[\w ]*?\b(tvz_\w+)\(", text, re.M))
    assert declared == set(_lib.GAP_LONG_SIGNATURES) and len(declared) == 2
    for name, (res, args) in _lib.GAP_LONG_SIGNATURES.items():
        assert (_kind(res), [_kind(a) for a in args]) == _prototype(text, name), name
    # the arguments are tvz_align_candidates'
    assert _lib.GAP_LONG_SIGNATURES["tvz_align_candidates_long"] == _lib.GAP_SIGNATURES["tvz_align_candidates"]
    assert _lib.GAP_LONG_SIGNATURES["tvz_align_candidates_long_workspace_bytes"] == \
        _lib.GAP_SIGNATURES["tvz_align_candidates_workspace_bytes"]
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    defined = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", tbuild.SO], text=True).splitlines()
               if ln.strip()}
    assert declared <= defined, sorted(declared - defined)
    lib = _lib.load()
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.GAP_LONG_SIGNATURES[name][1]
    # new exports only: the other tables, the version and the main headers are what they were
    assert (len(_lib.SIGNATURES), len(_lib.GAP_SIGNATURES), len(_lib.GAP_SHARD_SIGNATURES), len(_lib.GAP_RATE_SIGNATURES),
            len(_lib.GAP_RATE_SHARD_SIGNATURES), len(_lib.PARTS_FLAGS_SIGNATURES)) == (75, 4, 4, 2, 4, 2)
    assert _lib.VERSION == 404 and lib.tvz_version() == 404
    for h in ("tvz.h", "tvz_gap.h"):
        assert "candidates_long" not in open(os.path.join(ROOT, "include", h)).read()
    assert re.search(r"^#define TVZ_GAP_MAX_PROBES 4095\b", open(os.path.join(ROOT, "include", "tvz_gap.h")).read(), re.M)
    for name, value in (("SEG_POSITIONS", tc.ALIGN_CANDIDATES_LONG_SEG_POSITIONS), ("MAX_LEN", tc.ALIGN_CANDIDATES_LONG_MAX_LEN),
                        ("LDS_ENTRIES", tc.ALIGN_CANDIDATES_LONG_LDS_ENTRIES)):
        assert re.search(r"^#define TVZ_GAP_LONG_%s %d\b" % (name, value), text, re.M), name
    assert lref.SEG_POSITIONS == lc.SEG == tc.ALIGN_CANDIDATES_LONG_SEG_POSITIONS == 511 and lref.MAX_LEN == 4095
    assert tc.DeviceCorpus.supports_align_candidates_long is True
    from tvidz_amd import service
    assert not hasattr(service.ShardedCorpus, "supports_align_candidates_long")
    assert not hasattr(service.RankCorpus, "supports_align_candidates_long")


def test_the_workspace_formula():
    lib = _lib.load()
    E = tc.ALIGN_CANDIDATES_LONG_LDS_ENTRIES
    for Q, L, keys, cap, c in ((1, 200, 0, 4096, 16), (16, 514, 0, 64, 64), (64, 4095, 0, 4096, 16), (3, 515, 1030, 1025, 1),
                               (7, 1026, 0, 17, 1), (1, 0, 0, 1, 1), (0, 10, 0, 4, 4)):
        S = lref.lists_per_query(L)
        total = max(keys if keys > 0 else Q * L, L)
        probe_len = min(8 * max(L - 3, 1), 4088)
        table = 0 if S * cap <= E else Q * 8 * lc.table_slots(S * cap)
        raw = Q * S * cap * 12 + 2 * Q * S * 4 + (Q * S + 1) * 8 + Q * 4 + lib.tvz_match_workspace_bytes(Q * S, probe_len, 0, 0, 1) + \
            total * (8 + 4 + 64) + table
        got = tc.align_candidates_long_workspace_bytes(Q, L, keys, cap, c)
        assert raw <= got < raw + 12 * 256, (Q, L, keys, cap, c, got, raw)
    # what the issue asks the document for: Q = 64, cap = 4,096, max_query_len = 4,095
    print("workspace bytes at Q=64, cap=4096, L=4095:", tc.align_candidates_long_workspace_bytes(64, 4095, 0, 4096, 16))
    for bad in ((-1, 10, 0, 16, 16), (1, -1, 0, 16, 16), (1, 10, -1, 16, 16), (1, 10, 0, 16, 0), (1, 10, 0, 16, 65),
                (1, 10, 0, 15, 16), (1, 4096, 0, 16, 16), (65536, 10, 0, 16, 16), (32768, 515, 0, 16, 16), (7282, 4095, 0, 16, 16),
                (1, 4095, 0, 58369, 16), (1, 515, 0, 262658, 16), (1, 514, 0, 525315, 16)):
        assert tc.align_candidates_long_workspace_bytes(*bad) == 0, bad
    for good in ((65535, 514, 1, 16, 16), (32767, 515, 1, 16, 16), (7281, 4095, 1, 16, 16), (1, 4095, 0, 58368, 16),
                 (1, 515, 0, 262657, 16), (1, 514, 0, 525314, 16)):
        assert tc.align_candidates_long_workspace_bytes(*good) > 0, good


def test_refusals_that_need_no_device_and_their_order():
    """The plain call's refusals first, in its order and with its messages; then the probe lists, then the 32-bit sums;
    then the workspace; a NULL handle's refusal stands in front of all of them only where the plain call's does."""
    lib = _lib.load()

    def call(fn, Q=1, C_=16, cap=64, min_count=2, L=4, ws=0):
        rc = fn(None, None, None, Q, L, min_count, None, cap, C_, None, None, ws, None)
        return rc, lib.tvz_last_error()

    long_, plain = lib.tvz_align_candidates_long, lib.tvz_align_candidates
    for kw in (dict(C_=0), dict(C_=65), dict(C_=-1), dict(cap=15), dict(min_count=0), dict(min_count=-3), dict(L=4096),
               dict(C_=0, cap=-1, min_count=0, L=4096), dict(cap=15, min_count=0, L=4096), dict(min_count=0, L=4096), dict()):
        assert call(long_, **kw) == call(plain, **kw), kw
    assert b"max_query_len 4096 above 4095" in call(long_, L=4096)[1]
    # the 514 limit is gone, and it is the only thing that is gone: 4,095 passes to the next refusal
    rc, msg = call(long_, L=4095)
    assert rc == ERR_INVALID and b"corpus is NULL" in msg
    # the probe lists: Q x S_max
    rc, msg = call(long_, Q=32768, L=515)
    assert rc == ERR_UNSUPPORTED and msg == b"alignment candidates: Q=32768 x 2 segments is above 65535 probe lists"
    rc, msg = call(long_, Q=7282, L=4095)
    assert rc == ERR_UNSUPPORTED and b"x 9 segments" in msg
    assert b"corpus is NULL" in call(long_, Q=32767, L=515)[1] and b"corpus is NULL" in call(long_, Q=65535, L=514)[1]
    # the 32-bit sums: S_max x cap x 4,088
    rc, msg = call(long_, L=4095, cap=58369)
    assert rc == ERR_UNSUPPORTED and msg == b"alignment candidates: 9 segments x cap=58369 x 4088 probe slots is above 2147483647"
    assert b"corpus is NULL" in call(long_, L=4095, cap=58368)[1]
    # the order: the plain call's, then the lists, then the sums
    assert b"min_count 0" in call(long_, Q=70000, L=4095, cap=58369, min_count=0)[1]
    assert b"max_query_len 4096" in call(long_, Q=70000, L=4096, cap=58369)[1]
    assert b"probe lists" in call(long_, Q=70000, L=4095, cap=58369)[1]
    assert b"probe slots" in call(long_, Q=1, L=4095, cap=58369)[1]


# ---------------------------------------------------------------------------------------------- the inspector
class _LongCorpus(_Corpus):
    """tests/test_gap_candidates_cpu.py's fake corpus with the call for long uploads: it names the same three videos, and
    refuses what is longer than 4,095 values"""
    supports_align_candidates_long = True

    def align_candidates_rates(self, queries, **kw):                               # (never reached: refused at construction)
        raise AssertionError("the rates call beside the long one")

    def align_candidates_long(self, queries, **kw):
        self.calls.append(("align_candidates_long", dict(kw, Q=len(queries))))
        c = kw["c"]
        rows = np.zeros((len(queries), c, 2), dtype=np.int32)
        rows[:, :, 0] = -1
        if any(len(q) > 4095 for q in queries):
            return rows, np.full(len(queries), INT32_MIN, dtype=np.int32)
        rows[:, :3] = ((42, 57), (43, 9), (44, 2))
        return rows, np.full(len(queries), 3, dtype=np.int32)


def test_inspector_long_option_calls_refusals_fallback_and_unset():
    from tvidz_amd import inspector as insp

    ok = dict(device="cuda:0", near_duplicates=True, near_top_k=8, near_any_offset=True, near_score="local", near_min_votes=8,
              near_jaccard=0.9)
    new = lambda corpus=None, **kw: insp.Inspector(_Store(corpus or _LongCorpus()), **dict(ok, **kw))       # noqa: E731
    # every refused combination
    with pytest.raises(RuntimeError, match="near_candidates_long=True needs near_candidates"):
        new(near_candidates_long=True)
    with pytest.raises(RuntimeError, match="near_candidates_long=True with near_candidate_rates=True"):
        new(near_candidates=16, near_candidates_long=True, near_candidate_rates=True, near_rates=(1.0, 0.96))
    with pytest.raises(RuntimeError, match="has no align_candidates_long"):
        new(_Corpus(), near_candidates=16, near_candidates_long=True)
    flagged_off = _LongCorpus()
    flagged_off.supports_align_candidates_long = False
    with pytest.raises(RuntimeError, match="has no align_candidates_long"):
        new(flagged_off, near_candidates=16, near_candidates_long=True)
    with pytest.raises(ValueError):                                                # (near_candidates' own refusals stay)
        new(near_candidates=7, near_candidates_long=True)
    cuts = [float(3 * i) for i in range(128, -1, -1)] + [float("nan")]
    long_cuts = [float(3 * i) for i in range(1200)]
    too_long = [float(3 * i) for i in range(4096)]
    # unset: untouched - the plain candidates call, as before
    corpus = _LongCorpus()
    ins = new(corpus, near_candidates=16)
    assert ins.near_candidates_long is False
    (plain,) = ins._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates", "align_parts"]
    corpus = _LongCorpus()
    (swept,) = new(corpus)._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["align_span_topk"]
    # set: the ids of EVERY upload come from the long call - the short one too - and one parts call follows
    corpus = _LongCorpus()
    ins = new(corpus, near_candidates=16, near_candidates_long=True, near_gap_eps=0.05)
    assert corpus.calls == [("set_gap_index", 0.05)]
    (near,) = ins._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates_long", "align_parts"]
    assert corpus.calls[1][1] == dict(c=16, exclude_ids=[7], Q=1)
    assert corpus.calls[2][1] == dict(video_ids=[[42, 43, 44]], Q=1, eps=ins.near_eps, rates=(1.0,), min_votes=8, max_parts=1)
    assert near == plain == swept
    del corpus.calls[:]
    ins._near(8, long_cuts)
    assert [c[0] for c in corpus.calls] == ["align_candidates_long", "align_parts"]
    # above 4,095 values: the configured sweep
    del corpus.calls[:]
    ins._near(9, too_long)
    assert [c[0] for c in corpus.calls] == ["align_candidates_long", "align_span_topk"]
    # with near_parts the parts come from the same block
    corpus = _LongCorpus()
    (got,) = new(corpus, near_candidates=8, near_candidates_long=True, near_parts=3)._near(7, cuts)
    (want,) = new(_LongCorpus(), near_candidates=8, near_parts=3)._near(7, cuts)
    assert got == want and [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates_long", "align_parts"]


# -------------------------------------------------------------------------------------------- the code objects
def test_the_new_kernels_exist_once_with_no_scratch_and_no_spills(kernels):  # noqa: F811
    recorded = {}
    for name in NEW:
        found = [k for n, k in kernels.items() if name in n]
        assert len(found) == 1, (name, sorted(n for n in kernels if "gapl" in n))
        (k,) = found
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (name, k)
        assert k[".wavefront_size"] == 64
        recorded[name] = (k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".max_flat_workgroup_size"])
    print("vgprs, sgprs, LDS bytes, block:", recorded)
    assert recorded[NEW[0]][3] == 1024 and recorded[NEW[1]][3] == 256 and recorded[NEW[2]][3] == 256
    # the fold: the sort buffers (2,048 keys and counts), the table of 2 x LDS_ENTRIES 8-byte slots, the lists' starts
    lds = 2048 * 12 + 2 * tc.ALIGN_CANDIDATES_LONG_LDS_ENTRIES * 8
    assert lds <= recorded[NEW[2]][2] <= lds + 256 and recorded[NEW[2]][2] <= 64 * 1024
    assert recorded[NEW[0]][2] == 64 and recorded[NEW[1]][2] == 0
    assert recorded[NEW[0]][0] <= 40 and recorded[NEW[1]][0] <= 64 and recorded[NEW[2]][0] <= 64
    # the existing kernels of the candidates calls are all still there, once
    for name in ("ts_gapc_offsets_kernel", "ts_gapc_probe_kernel", "ts_gapc_select_kernel", "ts_gapr_fold_kernel",
                 "ts_gapc_merge_kernel", "ts_gapr_merge_kernel"):
        assert len([n for n in kernels if name in n]) == 1, name


# ------------------------------------------------------------------------------------ the host code, sanitized
def _program():
    sources = [os.path.join(tbuild.CSRC, "tvz_gap_codes.h"), MAIN]
    h = hashlib.sha1()
    for f in sources:
        h.update(open(f, "rb").read())
    cache = os.path.join(tempfile.gettempdir(), f"tvz-host-sanitizer-{os.getuid()}")
    os.makedirs(cache, exist_ok=True)
    exe = os.path.join(cache, "gapl-" + h.hexdigest()[:16])
    if not os.path.exists(exe):
        subprocess.check_call([tbuild._hipcc(), f"--offload-arch={tbuild.ARCH}", "-O1", "-std=c++17",
                               "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                               "-Wno-unused-function", f"-I{tbuild.CSRC}", "-o", exe + f".{os.getpid()}.tmp", MAIN])
        os.replace(exe + f".{os.getpid()}.tmp", exe)
    return exe


def test_host_segments_table_and_carving_under_asan_and_ubsan():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([_program()], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("HOST_OK"), (out.stdout[-500:], out.stderr[-3000:])
