"""The rates candidates call over a sharded table, without a GPU: the merge of the shards' reference blocks against the
reference over the whole table (rows split by id and by row index, so that rows of one id land in different shards), the
numpy merge against the reference merge, 20 lists as 16 + 4, the new header against the fifth signature table and the
library's exports, every refusal that needs no device and their order, the sharded sizing formula, the launcher's switch,
the Inspector over a fake sharded corpus, the new code object, and the host code under ASan + UBSan in a stand-alone
program."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from tests import gap_candidates_cases as cs, gap_candidates_rates_cases as rc, gap_candidates_rates_merge_cases as mc, \
    gap_candidates_rates_merge_ref as mref, gap_candidates_rates_ref as rr
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)
from tests.test_gap_candidates_cpu import _Store, _kind, _prototype
from tests.test_gap_candidates_rates_cpu import _RatesCorpus
from tvidz_amd import _lib, build as tbuild, corpus as tc, service, sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tvz_gap_rates_shards.h")
MAIN = os.path.join(ROOT, "tests", "gap_candidates_rates_shards_host_main.hip")
EPS = rc.GAP_EPS
ERR_INVALID, ERR_UNSUPPORTED = -1, -4
INT32_MIN = -(1 << 31)
SHARDS = (1, 2, 3, 8, 20)


# ------------------------------------------------------------------------------------------- the contract
@pytest.fixture(scope="module")
def tables():
    """the tables of tests/gap_candidates_rates_cases.py with queries and their count matrices - the fold table and the
    counting query at the fold's 8 rates, the main table and its uploads at 3 rates, the table of distinct ids at 2 -:
    computed once, never changed"""
    out = {}
    for name, rows, queries, rates in (("fold", rc.fold_table(), [cs.counting_query()], rc.FOLD_RATES),
                                       ("main", rc.table(), rc.queries(), rc.RATES3),
                                       ("distinct", rc.distinct_table(), rc.queries()[:5] + [cs.counting_query()], rc.RATES2)):
        out[name] = (rows, queries, rr.count_matrix(rows, queries, EPS, rates))
    return out


def _split_blocks(rows, matrices, R, by_row, c, **kw):
    """the reference blocks of the R shards: shard s holds the rows with video_id % R == s, or with row index % R == s"""
    out = []
    for s in range(R):
        at = [i for i, (v, _) in enumerate(rows) if (i if by_row else v) % R == s]
        out.append(rr.blocks([rows[i] for i in at], [None if m is None else m[:, at] for m in matrices], c, **kw))
    return np.stack(out)


@pytest.mark.parametrize("by_row", (False, True), ids=("by_id", "by_row_index"))
@pytest.mark.parametrize("table", ("fold", "main", "distinct"))
def test_the_merge_of_the_shards_blocks_is_the_whole_tables_answer(tables, table, by_row):
    rows, queries, matrices = tables[table]
    per_id = {}
    for i, (v, _) in enumerate(rows):
        per_id.setdefault(v, []).append(i)
    if table == "fold":
        assert max(len(r) for r in per_id.values()) >= 4                           # ids with four rows and more ...
        assert any(len({i % 3 for i in r}) >= 2 for r in per_id.values())         # ... which a split by row index parts
    if table == "main":
        assert len(per_id[rc.TRIPLE]) == 3                                         # three rows of one id: parted at R = 2, 3
    cap = 4096
    assert all(m is None or int((m[i] >= 1).sum()) <= cap for m in matrices for i in range(0 if m is None else m.shape[0]))
    for c in (1, 16, 64):
        whole = rr.blocks(rows, matrices, c, min_count=1, cap=cap)
        assert ((whole[:, c, 1] >= 0) | (whole[:, c, 1] == INT32_MIN)).all()       # no list over cap; a refused query may be there
        for R in SHARDS:
            blocks = _split_blocks(rows, matrices, R, by_row, c, min_count=1, cap=cap)
            assert (mref.merge_grouped(blocks) == whole).all(), (R, c)
            assert (sharded.merge_candidate_blocks(tc.align_candidates_rates_merge, blocks) == whole).all(), (R, c)


def test_one_shard_over_cap_at_one_rate_gives_a_negative_total():
    rows, q = rc.overflow_table(), [cs.counting_query()]
    matrices = rr.count_matrix(rows, q, EPS, (1.0, rc.QUARTER))
    blocks = _split_blocks(rows, matrices, 2, False, 3, min_count=1, cap=8)
    assert (blocks[:, 0, 3, 1] < 0).any() and not (blocks[:, 0, 3, 1] == INT32_MIN).any()
    merged = mref.merge(blocks)
    assert merged[0, 3, 1] == -int(np.abs(blocks[:, 0, 3, 1].astype(np.int64)).sum())
    assert (tc.align_candidates_rates_merge(blocks) == merged).all()


def test_the_numpy_merge_equals_the_reference_on_every_case():
    cases = mc.hand_made()
    for name, b in cases.items():
        want, got = mref.merge(b), tc.align_candidates_rates_merge(b)
        assert got.dtype == np.int32 and (got == want).all(), name
    assert cases["equal_best_smaller_rate_index"].shape[0] == 2
    assert mref.merge(cases["equal_best_smaller_rate_index"])[:, 0].tolist() == [[50, 6, 2], [50, 6, 2]]
    assert mref.merge(cases["larger_best_in_the_later_list"])[0, 0].tolist() == [50, 8, 6]
    same = mref.merge(cases["all_lists_hold_the_same_64_ids"])
    assert (same[:, :64, 0] >= 0).all() and len(set(same[0, :64, 0].tolist())) == 64
    # the generator makes ids repeat across the lists
    b = cases["mixed_R8_C16_Q5"]
    ids = [v for v in b[:, 0, :16, 0].ravel().tolist() if v >= 0]
    assert len(set(ids)) < len(ids)


def test_twenty_lists_as_sixteen_and_four_equal_the_reference_over_twenty():
    b = mc.twenty_lists()
    want = mref.merge(b)
    assert (mref.merge_grouped(b) == want).all()
    two = np.stack([tc.align_candidates_rates_merge(b[:16]), tc.align_candidates_rates_merge(b[16:])])
    assert (tc.align_candidates_rates_merge(two) == want).all()
    assert (sharded.merge_candidate_blocks(tc.align_candidates_rates_merge, b) == want).all()
    assert want[2, 16, 1] == INT32_MIN and want[1, 16, 1] < 0


# ------------------------------------------------------------------------------------------------- the C ABI
def test_the_header_the_fifth_table_and_the_exports_agree():
    text = open(HEADER).read()
    declared = set(re.findall(r"^\w[\w ]*?\b(tvz_\w+)\(", text, re.M))
    assert declared == set(_lib.GAP_RATE_SHARD_SIGNATURES) and len(declared) == 4
    for name, (res, args) in _lib.GAP_RATE_SHARD_SIGNATURES.items():
        assert (_kind(res), [_kind(a) for a in args]) == _prototype(text, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    defined = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", tbuild.SO], text=True).splitlines()
               if ln.strip()}
    assert declared <= defined, sorted(declared - defined)
    lib = _lib.load()
    for name in declared:                                                          # load() bound the fifth table too
        assert getattr(lib, name).argtypes == _lib.GAP_RATE_SHARD_SIGNATURES[name][1]
    for other, n in ((_lib.SIGNATURES, 75), (_lib.GAP_SIGNATURES, 4), (_lib.GAP_SHARD_SIGNATURES, 4), (_lib.GAP_RATE_SIGNATURES, 2)):
        assert len(other) == n and not declared & set(other)
    assert _lib.VERSION == 404 and lib.tvz_version() == 404
    assert '#include "tvz_gap_rates.h"' in text and "never run on more than one GPU" in text
    assert "#define TVZ_GAP_RATES_MERGE_MAX_LISTS 16" in text and tc.ALIGN_CANDIDATES_RATES_MERGE_MAX_LISTS == 16
    assert service.ShardedCorpus.supports_align_candidate_rates.fget(object()) is True
    assert sharded.RcclShardedMatcher.supports_align_candidate_rates is True
    assert service.ASK_CANDIDATES_RATES == 8 and service.ASK_HEADER == 5 + service.PARTS_PAR + tc.ALIGN_TOPK_MAX_K


def test_the_sharded_sizing_formula_and_its_zeros():
    al = lambda n: (n + 255) // 256 * 256                                            # noqa: E731
    for Q, L, keys, R, cap, c in ((1, 200, 0, 1, 4096, 16), (16, 514, 0, 8, 64, 64), (70, 40, 1234, 3, 17, 1), (0, 10, 0, 8, 4, 4)):
        plain = tc.align_candidates_rates_workspace_bytes(Q, L, keys, R, cap, c)
        for n in (0, 1, 3, 16, 20):
            block = Q * (c + 1) * 12
            assert tc.align_candidates_rates_sharded_workspace_bytes(Q, L, keys, R, cap, c, n) == \
                plain + al(block) + al(max(n, 1) * block) + 255, (Q, n)
    assert tc.align_candidates_rates_sharded_workspace_bytes(1, 10, 0, 1, 16, 16, -1) == 0
    for bad in ((-1, 10, 0, 1, 16, 16), (1, 10, 0, 1, 16, 0), (1, 10, 0, 1, 16, 65), (1, 10, 0, 1, 15, 16), (1, 4096, 0, 1, 16, 16),
                (1, 10, 0, 0, 16, 16), (1, 10, 0, 9, 16, 16), (8192, 10, 0, 8, 16, 16), (21846, 4, 0, 3, 1, 1)):
        assert tc.align_candidates_rates_workspace_bytes(*bad) == 0
        assert tc.align_candidates_rates_sharded_workspace_bytes(*bad, 4) == 0, bad


def test_refusals_that_need_no_device_and_their_order():
    lib = _lib.load()
    err = lib.tvz_last_error
    g, o = 0x10000, 0x80000
    merge = lib.tvz_align_candidates_rates_merge
    for n in (0, 17, -1):
        assert merge(g, n, 1, 16, o, None) == ERR_UNSUPPORTED and err() == b"alignment candidates merge: %d lists outside 1..16" % n
    for c in (0, 65):
        assert merge(g, 1, 1, c, o, None) == ERR_UNSUPPORTED and err() == b"alignment candidates merge: C=%d outside 1..64" % c
    assert merge(g, 1, -1, 16, o, None) == ERR_INVALID and b"Q=-1" in err()
    assert merge(None, 1, 1, 16, o, None) == ERR_INVALID and merge(g, 1, 1, 16, None, None) == ERR_INVALID
    for gp, op in ((g + 2, o), (g, o + 1), (g, o + 2)):
        assert merge(gp, 1, 1, 16, op, None) == ERR_INVALID and b"4-byte aligned" in err()
    assert merge(g + 4, 1, 1, 16, o + 4, None) != ERR_INVALID or b"aligned" not in err()      # 4 bytes are enough
    assert merge(g, 2, 3, 16, g + (2 * 3 * 17 * 3 - 3) * 4, None) == ERR_INVALID and b"lies inside" in err()
    assert merge(g, 2, 3, 16, g, None) == ERR_INVALID
    assert merge(None, 1, 0, 16, None, None) == 0                                   # Q = 0: no pointer is looked at
    # the order: lists, C, Q, NULL, alignment
    assert b"lists" in (merge(None, 0, -1, 0, None, None), err())[1]
    assert b"C=0" in (merge(None, 1, -1, 0, None, None), err())[1]
    assert b"Q=-1" in (merge(None, 1, -1, 16, None, None), err())[1]
    # _shards: the rates call's refusals in its order, then the shards
    ok = (C.c_double * 3)(1.0, 0.96, 1.25)
    none = (C.c_void_p * 17)()

    def shards(hs=none, n=2, Q=1, rates=ok, R=3, min_count=2, cap=16, C_=16, L=4):
        rc_ = lib.tvz_align_candidates_rates_shards(hs, n, None, None, Q, L, rates, R, min_count, None, cap, C_, g, o, None, 0, None)
        return rc_, err()

    assert b"C=0" in shards(None, 17, 70000, None, 0, 0, 1, 0, 4096)[1]
    assert b"cap=15" in shards(None, 17, 70000, None, 0, 0, 15, 16, 4096)[1]
    assert b"min_count 0" in shards(None, 17, 70000, None, 0, 0, 16, 16, 4096)[1]
    assert b"max_query_len 4096" in shards(None, 17, 70000, None, 0, 2, 16, 16, 4096)[1]
    assert b"n_rates=0" in shards(None, 17, 70000, None, 0)[1]
    assert b"h_rates is NULL" in shards(None, 17, 70000, None, 3)[1]
    assert b"rate 1 is" in shards(None, 17, 70000, (C.c_double * 2)(1.0, float("nan")), 2)[1]
    assert shards(None, 17, 70000) == (ERR_UNSUPPORTED, b"alignment candidates with rates: Q=70000 x n_rates=3 is above 65535 probe lists")
    assert shards(None, 17) == (ERR_INVALID, b"no shards")
    assert shards(none, 17)[0] == ERR_UNSUPPORTED and b"17 lists outside 1..16" in shards(none, 17)[1]
    assert shards(none, 2)[0] == ERR_INVALID and b"shard 0 is NULL" in shards(none, 2)[1]
    # _sharded: the rates call's refusals stand in front of the NULL handle and the NULL communicator

    def sharded_call(Q=1, rates=ok, R=3, min_count=2, cap=16, C_=16, L=4):
        rc_ = lib.tvz_align_candidates_rates_sharded(None, None, None, None, Q, L, rates, R, min_count, None, cap, C_, o, None, 0, None)
        return rc_, err()

    assert b"C=65" in sharded_call(C_=65, cap=70, min_count=0, R=0)[1]
    assert b"min_count 0" in sharded_call(min_count=0, R=0)[1]
    assert b"n_rates=9" in sharded_call(R=9, Q=70000)[1]
    assert b"probe lists" in sharded_call(Q=70000)[1]
    assert sharded_call()[0] == ERR_INVALID and b"corpus is NULL" in sharded_call()[1]


# ------------------------------------------------------------------------------------------------ the launcher
def test_the_launchers_switch():
    ok = dict(near_top_k=16, near_any_offset=True, near_score="local", near_min_votes=2)
    sw = service.check_near_switches
    # without the switch: the combination raises exactly the message it raised
    with pytest.raises(ValueError, match=r"^--near-candidates 32 with --near-rates: the gap codes are made at rate 1; use one of them$"):
        sw(**ok, near_candidates=32, near_rates="1.0,0.96")
    with pytest.raises(ValueError, match="--near-candidates 32 with --near-rates"):
        sw(**ok, near_candidates=32, near_rates="1.0,0.96", near_candidate_rates=False)
    # with it: what is missing is named
    with pytest.raises(ValueError, match=r"^--near-candidate-rates needs --near-candidates and --near-rates$"):
        sw(**ok, near_candidate_rates=True)
    with pytest.raises(ValueError, match=r"^--near-candidate-rates needs --near-rates$"):
        sw(**ok, near_candidates=32, near_candidate_rates=True)
    with pytest.raises(ValueError, match=r"^--near-candidate-rates needs --near-candidates$"):
        sw(**ok, near_rates="1.0,0.96", near_candidate_rates=True)
    with pytest.raises(ValueError, match="--near-candidate-rates needs --near-top-k"):
        sw(0, near_candidate_rates=True)
    with pytest.raises(ValueError, match="--near-candidates 32 with --near-two-bins"):
        sw(**ok, near_candidates=32, near_rates="1.0,0.96", near_candidate_rates=True, near_two_bins=True)
    with pytest.raises(ValueError, match="needs --near-any-offset"):
        sw(16, near_candidates=32, near_rates="1.0,0.96", near_candidate_rates=True)
    given = sw(**ok, near_candidates=32, near_rates="1.0,0.96", near_candidate_rates=True, near_gap_eps=0.05)
    assert given[-1] == "--near-candidate-rates" and given[given.index("--near-rates") + 1] == "1.0,0.96"
    assert given[given.index("--near-candidates") + 1] == "32"
    # off: the list a rank process gets is what it was
    assert "--near-candidate-rates" not in sw(**ok, near_candidates=32)
    assert sw(**ok, near_candidates=32) == sw(**ok, near_candidates=32, near_candidate_rates=False)

    class A:
        near_top_k, near_eps, near_max_offset, near_jaccard = 16, 1 / 30, 30.0, 0.8
        near_any_offset, near_score, near_min_votes, near_rates = True, "local", 2, "1.0,0.96"
        near_candidates, near_gap_eps, near_candidate_rates = 32, 0.05, True
    kw = service.near_kwargs(A)
    assert kw["near_candidate_rates"] is True and kw["near_rates"] == (1.0, 0.96) and kw["near_candidates"] == 32
    A.near_candidate_rates = False
    assert "near_candidate_rates" not in service.near_kwargs(A)


# ---------------------------------------------------------------------------------------------- the inspector
class _ShardedRatesFake(_RatesCorpus):
    """tests/test_gap_candidates_rates_cpu.py's fake as a sharded corpus: it says by its flags what it can"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.supports_align_candidates = self.supports_align_parts = self.supports_align_candidate_rates = True


def test_inspector_with_the_switch_over_a_fake_sharded_corpus():
    from tvidz_amd import inspector as insp
    ok = dict(device="cuda:0", near_duplicates=True, near_top_k=8, near_any_offset=True, near_score="local", near_min_votes=8,
              near_jaccard=0.9)
    rates = (1.0, 0.96, 1.25)
    cuts = [float(3 * i) for i in range(128, -1, -1)]
    corpus = _ShardedRatesFake()
    ins = insp.Inspector(_Store(corpus), **dict(ok, near_candidates=16, near_rates=rates, near_candidate_rates=True, near_gap_eps=0.05))
    (near,) = ins._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates_rates", "align_parts"]
    assert corpus.calls[1][1]["rates"] == rates and corpus.calls[2][1]["rates"] == rates and near["rate"] == 0.96
    flagged = _ShardedRatesFake()
    flagged.supports_align_candidate_rates = False
    with pytest.raises(RuntimeError, match="has no align_candidates_rates"):
        insp.Inspector(_Store(flagged), **dict(ok, near_candidates=16, near_rates=rates, near_candidate_rates=True))
    for cls in (service.ShardedCorpus, service.RankCorpus):
        assert hasattr(cls, "align_candidates_rates") and hasattr(cls, "supports_align_candidate_rates")


# -------------------------------------------------------------------------------------------- the code object
def test_the_new_merge_kernel_exists_once_with_no_scratch_and_the_others_keep_their_names(kernels):  # noqa: F811
    found = [k for n, k in kernels.items() if "20ts_gapr_merge_kernelE" in n]
    assert len(found) == 1, sorted(n for n in kernels if "gap" in n)
    (k,) = found
    assert k[".private_segment_fixed_size"] == 0
    assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0 and k[".wavefront_size"] == 64
    print("vgprs, sgprs, static LDS bytes, block:", k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"],
          k[".max_flat_workgroup_size"])
    # a block of 256 per query; 1,024 keys and counts and 16 totals (12,352 bytes) and 256 bytes more, as the fold has
    # over its arrays: the two kernels that call __syncthreads_count carry them, the select kernel, which does not,
    # has exactly its arrays' 24,576
    assert k[".max_flat_workgroup_size"] == 256 and 1024 * 12 + 64 <= k[".group_segment_fixed_size"] <= 1024 * 12 + 512
    assert k[".vgpr_count"] <= 64
    for name in ("19ts_gapr_fold_kernelE", "21ts_gapc_select_kernelE", "20ts_gapc_merge_kernelE"):
        assert len([n for n in kernels if name in n]) == 1, name


# ------------------------------------------------------------------------------------ the host code, sanitized
def _program():
    sources = sorted(os.path.join(tbuild.CSRC, f) for f in os.listdir(tbuild.CSRC)) + \
        [os.path.join(tbuild.INCLUDE, h) for h in ("tvz.h", "tvz_gap.h", "tvz_gap_shards.h", "tvz_gap_rates.h",
                                                   "tvz_gap_rates_shards.h")] + [MAIN]
    h = hashlib.sha1()
    for f in sources:
        h.update(open(f, "rb").read())
    cache = os.path.join(tempfile.gettempdir(), f"tvz-host-sanitizer-{os.getuid()}")
    os.makedirs(cache, exist_ok=True)
    exe = os.path.join(cache, "gapr-shards-" + h.hexdigest()[:16])
    if not os.path.exists(exe):
        # (the device half is compiled because the translation unit registers its kernels; unoptimised: it never runs)
        subprocess.check_call([tbuild._hipcc(), f"--offload-arch={tbuild.ARCH}", "-O1", "-Xarch_device", "-O0", "-std=c++17",
                               "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                               "-Wno-unused-function", f"-I{tbuild.INCLUDE}", f"-I{tbuild.CSRC}", "-o", exe + f".{os.getpid()}.tmp",
                               MAIN, os.path.join(tbuild.CSRC, "tvz_api.hip"), os.path.join(tbuild.CSRC, "tvz_comm.hip"), "-ldl"])
        os.replace(exe + f".{os.getpid()}.tmp", exe)
    return exe


def test_host_sharded_carving_and_refusals_under_asan_and_ubsan():
    """The sharded workspace of the rates call is carved inside its buffer at every misalignment, for 1 and 8 rates and 1
    and 16 ranks, the rates call's part behind the blocks; one byte less is one byte short; the early refusals make no
    invalid access."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([_program()], capture_output=True, text=True, timeout=300, env=env, stdin=subprocess.DEVNULL)
    assert out.returncode == 0 and out.stdout.strip().endswith("HOST_OK"), (out.stdout[-500:], out.stderr[-3000:])
