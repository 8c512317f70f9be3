"""The candidates call over a sharded table without a GPU: the merge of the shards' reference blocks is the reference over
the whole table (where no shard overflowed `cap`); corpus.align_candidates_merge equals the reference merge on every
hand-made case; the new header against the third signature table and the library's exports; every refusal that needs no
device; the sharded workspace formula; the launcher's switches; the tick over gloo at world sizes 2 and 3 with mixed
asks; an Inspector over a fake sharded corpus; the merge kernel's code object; the host code under ASan + UBSan in a
stand-alone program."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import gap_candidates_cases as cs, gap_candidates_merge_cases as mc, gap_candidates_merge_ref as mref
from tests import gap_candidates_ref as ref
from tests.near_fakes import free_port_run
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)
from tests.test_gap_candidates_cpu import _Corpus, _kind, _prototype, _Store
from tvidz_amd import _lib, build as tbuild, corpus as tc, service, sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tvz_gap_shards.h")
MAIN = os.path.join(ROOT, "tests", "gap_candidates_shards_host_main.hip")
EPS = cs.GAP_EPS
ERR_INVALID, ERR_UNSUPPORTED = -1, -4
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
SHARD_COUNTS = (1, 2, 3, 8, 20)


def _split(rows, R):
    return [[r for r in rows if r[0] % R == s] for s in range(R)]


def _shard_blocks(rows, queries, R, c, **kw):
    return np.stack([ref.candidates(part, queries, EPS, c, **kw) for part in _split(rows, R)])


# -------------------------------------------------------------------------------------- the merge is exact
@pytest.mark.parametrize("R", SHARD_COUNTS)
def test_merged_shard_blocks_equal_the_whole_table(R):
    up = cs.uploads()
    tables = [(cs.table(), [up[n] for n in up] + [cs.long_query(514, 1), cs.long_query(515, 2)], 1),
              (cs.counting_table(257), [cs.counting_query(), up["stranger"]], 1),
              (cs.counting_table(65), [cs.counting_query()], 6)]
    for rows, queries, min_count in tables:
        for c in (1, 16, 64):
            cap = 4096
            whole = ref.candidates(rows, queries, EPS, c, min_count=min_count, cap=cap)
            blocks = _shard_blocks(rows, queries, R, c, min_count=min_count, cap=cap)
            # the premise: no list overflowed `cap` - every total is a plain count (or a refusal, on every shard alike)
            totals = blocks[:, :, c, 1]
            assert ((totals >= 0) & (totals <= cap) | (totals == INT32_MIN)).all()
            assert ((totals == INT32_MIN).all(0) | (totals != INT32_MIN).all(0)).all()
            assert all(mref.is_sorted(b) for b in blocks)
            got = mref.merge_grouped(blocks)
            assert (got == whole).all(), (R, c, min_count)
            assert (mref.merge(blocks) == whole).all()                             # any grouping: the rule is associative
            assert (tc.align_candidates_merge(blocks) == whole).all()
            assert (sharded.merge_candidate_blocks(tc.align_candidates_merge, blocks) == whole).all()
    # every shard holds more than C candidates: 257 hits, C = 16, up to 8 shards
    if R <= 8:
        blocks = _shard_blocks(cs.counting_table(257), [cs.counting_query()], R, 16, min_count=1)
        assert (blocks[:, 0, 16, 1] > 16).all() and (blocks[:, 0, 15, 0] >= 0).all()


def test_a_shard_over_cap_gives_a_negative_total():
    rows, q = cs.counting_table(257), [cs.counting_query()]
    blocks = _shard_blocks(rows, q, 3, 16, min_count=1, cap=80)                    # 86, 86 and 85 candidates
    assert sorted(blocks[:, 0, 16, 1].tolist()) == [-86, -86, -85]
    blocks[1] = ref.candidates(_split(rows, 3)[1], q, EPS, 16, min_count=1, cap=86)
    merged = mref.merge(blocks)
    assert int(merged[0, 16, 1]) == -257 and (tc.align_candidates_merge(blocks) == merged).all()
    exact = _shard_blocks(rows, q, 3, 16, min_count=1, cap=86)
    assert int(mref.merge(exact)[0, 16, 1]) == 257


def test_the_host_merge_equals_the_reference_on_every_hand_made_case():
    cases = mc.hand_made()
    assert len(cases) >= 60
    seen = set()
    for name, blocks in cases.items():
        assert all(mref.is_sorted(b) for b in blocks), name                        # the cases keep the precondition
        want = mref.merge(blocks)
        assert mref.is_sorted(want), name                                          # ... and so does a merge's output
        got = tc.align_candidates_merge(blocks)
        assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), name
        seen.add((blocks.shape[0], blocks.shape[2] - 1))
    assert {(R, c) for R in (1, 2, 3, 8, 16) for c in (1, 16, 63, 64)} <= seen
    # what the named cases are there for
    t = mref.merge(cases["tie_straddles_C"])[0]
    assert t[:5, 1].tolist() == [9] * 5 and t[:5, 0].tolist() == [1, 3, 5, 7, 900]
    assert t[5:16, 1].tolist() == [4] * 11 and t[5:16, 0].tolist() == list(range(100, 111)) and int(t[16, 1]) == 45
    assert mref.merge(cases["equal_rows_in_two_lists"])[0, :4].tolist() == [[50, 6], [50, 6], [10, 3], [11, 3]]
    assert mref.merge(cases["equal_rows_on_the_edge"])[:, :2].tolist() == [[[50, 6], [50, 6]]] * 2
    assert mref.merge(cases["equal_rows_C1"])[0].tolist() == [[50, 6], [-1, 3]]
    assert mref.merge(cases["equal_counts_ids_ascending"])[0, :4, 0].tolist() == [5, 10, 20, 25]
    x = mref.merge(cases["extreme_ids_and_counts"])[0]
    assert x[:4].tolist() == [[0, INT32_MAX], [1, INT32_MAX], [mc.MAX_ID, INT32_MAX], [mc.MAX_ID, INT32_MAX]]
    assert x[4:8].tolist() == [[0, 2], [0, 1], [mc.MAX_ID - 1, 1], [mc.MAX_ID, 1]]
    assert mref.merge(cases["totals_plain"])[:, 4, 1].tolist() == [70005]
    assert mref.merge(cases["totals_one_negative"])[:, 4, 1].tolist() == [-4102, -1]
    assert mref.merge(cases["totals_saturate"])[:, 4, 1].tolist() == [INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX]
    assert mref.merge(cases["totals_saturate_negative"])[:, 4, 1].tolist() == [-INT32_MAX] * 3
    assert mref.merge(cases["totals_16_lists_saturate"])[:, 2, 1].tolist() == [INT32_MAX, INT32_MAX, 16 * ((1 << 27) - 1)]
    r = mref.merge(cases["refused_in_one_list"])
    assert r[:, 4, 1].tolist() == [INT32_MIN, 6, INT32_MIN, INT32_MIN] and (r[0, :4] == (-1, 0)).all() and r[1, 0, 0] == 1
    # 20 lists as 16 + 4 equal the reference over all 20
    b = mc.twenty_lists()
    assert (mref.merge_grouped(b) == mref.merge(b)).all()
    assert (sharded.merge_candidate_blocks(tc.align_candidates_merge, b) == mref.merge(b)).all()
    assert int(mref.merge(b)[1, 16, 1]) < 0 and int(mref.merge(b)[2, 16, 1]) == INT32_MIN
    # no query at all
    assert tc.align_candidates_merge(np.zeros((3, 0, 17, 2), dtype=np.int32)).shape == (0, 17, 2)


# ------------------------------------------------------------------------------------------------- the C ABI
def test_the_header_the_third_table_and_the_exports_agree():
    text = open(HEADER).read()
    declared = set(re.findall(r"^\w[\w ]*?\b(tvz_\w+)\(", text, re.M))
    assert declared == set(_lib.GAP_SHARD_SIGNATURES) and len(declared) == 4
    for name, (res, args) in _lib.GAP_SHARD_SIGNATURES.items():
        assert (_kind(res), [_kind(a) for a in args]) == _prototype(text, name), name
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    defined = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", tbuild.SO], text=True).splitlines()
               if ln.strip()}
    assert declared <= defined, sorted(declared - defined)
    lib = _lib.load()
    for name in declared:                                                          # load() bound the third table too
        assert getattr(lib, name).argtypes == _lib.GAP_SHARD_SIGNATURES[name][1]
    # new exports only: the two older tables, their headers and the version are what they were
    assert len(_lib.SIGNATURES) == 75 and len(_lib.GAP_SIGNATURES) == 4
    assert not declared & (set(_lib.SIGNATURES) | set(_lib.GAP_SIGNATURES))
    assert _lib.VERSION == 404 and lib.tvz_version() == 404
    assert '#include "tvz_gap.h"' in text
    gap = open(os.path.join(ROOT, "include", "tvz_gap.h")).read()
    assert set(re.findall(r"^\w[\w ]*?\b(tvz_\w+)\(", gap, re.M)) == set(_lib.GAP_SIGNATURES) and "shards" not in gap
    assert "tvz_gap" not in open(os.path.join(ROOT, "include", "tvz.h")).read()
    assert re.search(r"^#define TVZ_GAP_MERGE_MAX_LISTS 16\b", text, re.M) and tc.ALIGN_CANDIDATES_MERGE_MAX_LISTS == 16
    assert "never run on more than one GPU" in text and "PRECONDITION" in text
    # the tick's tables are what they were, and the new kind stands beside them
    assert service.ASK_HEADER == 5 + 16 + 64 and sorted(service.TICK_FORMS) == [2, 3, 4, 5] and service.ASK_PARTS == 6
    assert service.ASK_CANDIDATES == 7 and service.CAND_PAR <= service.NEAR_PAR


def test_the_sharded_workspace_formula():
    al = lambda x: (x + 255) & ~255                                                # noqa: E731
    for Q, L, keys, cap, c in ((1, 200, 0, 4096, 16), (16, 514, 0, 64, 64), (70, 40, 1234, 17, 1), (1, 0, 0, 1, 1)):
        plain = tc.align_candidates_workspace_bytes(Q, L, keys, cap, c)
        block = Q * (c + 1) * 8
        for n in (0, 1, 2, 8, 16, 40):
            got = tc.align_candidates_sharded_workspace_bytes(Q, L, keys, cap, c, n)
            assert got == plain + al(block) + al(max(n, 1) * block) + 255, (Q, L, keys, cap, c, n)
            assert plain + (1 + max(n, 1)) * block <= got < plain + (1 + max(n, 1)) * block + 3 * 256
        assert tc.align_candidates_sharded_workspace_bytes(Q, L, keys, cap, c, -1) == 0
    for bad in ((-1, 10, 0, 16, 16), (1, -1, 0, 16, 16), (1, 10, -1, 16, 16), (1, 10, 0, 16, 0), (1, 10, 0, 16, 65),
                (1, 10, 0, 15, 16), (1, 4096, 0, 16, 16)):
        assert tc.align_candidates_workspace_bytes(*bad) == 0 and tc.align_candidates_sharded_workspace_bytes(*bad, 2) == 0


def test_refusals_that_need_no_device_and_their_order():
    lib = _lib.load()
    G, O = 0x10000, 0x80000                                                        # never looked at: every call is refused

    def merge(n=2, Q=1, C_=16, g=G, o=O):
        return lib.tvz_align_candidates_merge(g, n, Q, C_, o, None), lib.tvz_last_error()

    for bad in (0, 17, -1):
        rc, msg = merge(n=bad)
        assert rc == ERR_UNSUPPORTED and msg == b"alignment candidates merge: %d lists outside 1..16" % bad
    for bad in (0, 65, -1):
        rc, msg = merge(C_=bad)
        assert rc == ERR_UNSUPPORTED and msg == b"alignment candidates merge: C=%d outside 1..64" % bad
    assert merge(Q=-1) == (ERR_INVALID, b"Q=-1 is negative")
    assert merge(g=None)[0] == ERR_INVALID and merge(o=None)[0] == ERR_INVALID
    for kw in (dict(g=G + 4), dict(o=O + 4)):
        rc, msg = merge(**kw)
        assert rc == ERR_INVALID and b"8-byte aligned" in msg
    block = 3 * 17 * 8
    for o in (G, G + 8, G + 2 * block - 8, G - block + 8):
        rc, msg = merge(Q=3, g=G, o=o)
        assert rc == ERR_INVALID and b"d_out lies inside the blocks" in msg, o
    # the order: the lists, C, Q, the pointers; Q = 0 looks at no pointer
    assert b"lists" in merge(n=0, C_=0, Q=-1, g=None)[1] and b"C=0" in merge(C_=0, Q=-1, g=None)[1]
    assert b"negative" in merge(Q=-1, g=None)[1]
    assert lib.tvz_align_candidates_merge(None, 1, 0, 16, None, None) == 0

    def shards(handles=(None, None), n=None, C_=16, cap=64, min_count=2, L=4):
        arr = (C.c_void_p * max(len(handles), 1))(*handles)
        rc = lib.tvz_align_candidates_shards(arr if handles is not None else None, len(handles) if n is None else n, None, None,
                                             1, L, min_count, None, cap, C_, G, O, None, 0, None)
        return rc, lib.tvz_last_error()

    # the plain call's refusals first, in its order and words ...
    assert shards(C_=0, cap=-1, min_count=0, L=4096) == (ERR_UNSUPPORTED, b"alignment candidates: C=0 outside 1..64")
    assert shards(cap=15, min_count=0, L=4096) == (ERR_UNSUPPORTED, b"alignment candidates: cap=15 below C=16")
    assert shards(min_count=0, L=4096) == (ERR_INVALID, b"alignment candidates: min_count 0 below 1")
    assert shards(L=4096, n=17) == (ERR_UNSUPPORTED, b"alignment candidates: max_query_len 4096 above 4095")
    # ... then the shards: their count, the merge's limit, a NULL handle
    assert shards(n=0) == (ERR_INVALID, b"no shards")
    rc, msg = shards(handles=(None,) * 17)
    assert rc == ERR_UNSUPPORTED and msg == b"alignment candidates merge: 17 lists outside 1..16"
    rc, msg = shards()
    assert rc == ERR_INVALID and b"shard 0 is NULL" in msg

    def sharded_call(C_=16, cap=64, min_count=2, L=4):
        rc = lib.tvz_align_candidates_sharded(None, None, None, None, 1, L, min_count, None, cap, C_, O, None, 0, None)
        return rc, lib.tvz_last_error()

    # the RCCL form: the plain call's refusals stand in front of the communicator's (a NULL one here)
    assert sharded_call(C_=65) == (ERR_UNSUPPORTED, b"alignment candidates: C=65 outside 1..64")
    assert sharded_call(cap=3) == (ERR_UNSUPPORTED, b"alignment candidates: cap=3 below C=16")
    assert sharded_call(min_count=0) == (ERR_INVALID, b"alignment candidates: min_count 0 below 1")
    assert sharded_call(L=4096) == (ERR_UNSUPPORTED, b"alignment candidates: max_query_len 4096 above 4095")
    rc, msg = sharded_call()
    assert rc == ERR_INVALID and b"corpus is NULL" in msg


def test_the_launcher_switches():
    ns = lambda **kw: type("A", (), kw)()                                          # noqa: E731
    base = dict(near_top_k=8, near_eps=0.05, near_max_offset=30.0, near_jaccard=0.8, near_any_offset=True)
    assert "near_candidates" not in service.near_kwargs(ns(**base))               # off: the driver is built as before
    assert "near_candidates" not in service.near_kwargs(ns(near_candidates=0, near_gap_eps=0.1, **base))
    kw = service.near_kwargs(ns(near_candidates=32, near_gap_eps=0.04, **base))
    assert kw["near_candidates"] == 32 and kw["near_gap_eps"] == 0.04 and kw["near_any_offset"] is True
    assert service.near_kwargs(ns(near_top_k=0, near_candidates=32)) == {}
    # the switches as a rank process takes them: behind the earlier ones, none at the defaults
    assert service.check_near_switches(8, True) == ["--near-any-offset"]
    got = service.check_near_switches(8, True, "local", 4, None, False, 0, False, 32, 0.04)
    assert got[-4:] == ["--near-candidates", "32", "--near-gap-eps", "0.04"] and got[0] == "--near-any-offset"
    assert service.check_near_switches(8, True, near_candidates=8)[-4:-2] == ["--near-candidates", "8"]
    for bad, kw in (("needs --near-top-k", dict(near_top_k=0, near_candidates=16)),
                    ("needs --near-any-offset", dict(near_top_k=8, near_candidates=16)),
                    ("must be --near-top-k..64", dict(near_top_k=8, near_any_offset=True, near_candidates=7)),
                    ("must be --near-top-k..64", dict(near_top_k=8, near_any_offset=True, near_candidates=65)),
                    ("near_candidates must be", dict(near_top_k=8, near_any_offset=True, near_candidates=-1)),
                    ("near_candidates must be", dict(near_top_k=8, near_any_offset=True, near_candidates=8.5)),
                    ("near_gap_eps", dict(near_top_k=8, near_any_offset=True, near_candidates=16, near_gap_eps=0.0)),
                    ("near_gap_eps", dict(near_top_k=8, near_any_offset=True, near_candidates=16, near_gap_eps=float("nan"))),
                    ("with --near-rates", dict(near_top_k=8, near_any_offset=True, near_candidates=16, near_rates="1.0,0.96")),
                    ("with --near-two-bins", dict(near_top_k=8, near_any_offset=True, near_candidates=16, near_two_bins=True))):
        with pytest.raises(ValueError, match=bad):
            service.check_near_switches(**kw)


# ------------------------------------------------------------------------------------------ the tick over gloo
L = 129


def _tick_table():
    up = cs.uploads()
    queries = [up[n] for n in ("shifted", "excerpt", "twin", "stranger", "three")] + [cs.long_query(515, 2)[:L]] + \
        [[float(i) for i in range(150)]]
    return cs.table(), queries                                       # the last query is over-long at max_query_len = L


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _run(target, world):
    port = free_port_run()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in procs]
    [p.join(300) for p in procs]
    assert all(not p.is_alive() for p in procs), "a rank hung"
    res = sorted(q.get(timeout=5) for _ in range(world))
    assert res == [(r, "ok") for r in range(world)], res
    assert all(p.exitcode == 0 for p in procs)


def _mixed_asks(rows, queries, rank):
    """candidates asks of three parameter sets among parts and search asks, in an order that depends on the rank"""
    from tests import align_parts_cases as pc
    qa, qb = np.asarray(queries[0]), np.asarray(queries[1])
    cand = lambda c, min_count=1, cap=4096: (EPS, 0.0, c, min_count, cap)          # noqa: E731
    r1 = service.check_near_rates((1.0,))
    parts = service.check_near(tc.FORM_SPAN, pc.EPS, None, 2, 1, 0) + r1 + (2,)
    asks = [(qa, 0, -1, service.ASK_CANDIDATES, 0.0, cand(16)),
            (qb, 0, -1, service.ASK_PARTS, 0.0, parts + (float(cs.FILM), -1.0)),
            (qb, 0, cs.FILM, service.ASK_CANDIDATES, 0.0, cand(16)),
            (qa, 0, -1, service.ASK_NEAR_WIDE, 0.0, service.check_near(tc.FORM_WIDE, pc.EPS, None, 4, 1, 0)),
            (qa, 0, -1, service.ASK_CANDIDATES, 0.0, cand(4, 6)),
            (np.asarray(rows[15][1]), 2, -1, service.ASK_TOPK, 0.0, None),
            (qa, 0, -1, service.ASK_CANDIDATES, 0.0, cand(4, 6, 64)),
            (qb, 0, -1, service.ASK_NEAR_SPAN, 0.0, service.check_near(tc.FORM_SPAN, pc.EPS, None, 4, 1, 0) + r1)]
    return asks[rank % len(asks):] + asks[:rank % len(asks)]


def _rank_worker(rank, world, port, out):
    from tests.gap_candidates_service_fakes import CandidatesBackend, GapOracleCorpus
    from tests.near_service_fakes import NearServiceBackend
    _init(rank, world, port)
    rc = None
    try:
        rows, queries = _tick_table()
        shard = GapOracleCorpus()
        g = dist.new_group(backend="gloo")                            # the tick thread's own group
        backend = CandidatesBackend(live=shard)
        rc = service.RankCorpus(shard, sharded.ShardedMatcher(backend, k=8, cap=64, group=g), group=g, xdev="cpu", tick_s=0.01)
        assert rc.supports_align_candidates and rc.supports_align_parts
        rc.upload(rows)                                               # video_id mod world
        # refused in the caller while the shard keeps no codes: nothing travels
        with pytest.raises(RuntimeError, match="keeps no gap codes"):
            rc.align_candidates(queries[:1], c=16)
        assert rc.gap_index_stats()["gap_eps"] == 0.0
        rc.set_gap_index(EPS)
        assert rc.gap_index_stats()["gap_eps"] == EPS
        dist.barrier()
        # (1) the public call, alone: the whole table's answer; the over-long query is refused without travelling, the
        #     one of 515 values (cut to L here: it travels) as the library answers it
        excl = [cs.FILM] + [-1] * (len(queries) - 1)
        for c, min_count in ((16, 1), (1, 2), (64, 1)):
            exp = ref.candidates(rows, queries, EPS, c, min_count=min_count, exclude_ids=excl, max_query_len=L)
            got_rows, got_totals = rc.align_candidates(queries, c=c, min_count=min_count, exclude_ids=excl, max_query_len=L)
            assert got_rows.dtype == np.int32 and got_rows.shape == (len(queries), c, 2) and got_totals.dtype == np.int32
            assert (got_rows == exp[:, :c]).all() and (got_totals == exp[:, c, 1]).all(), (c, min_count)
            assert got_totals[-1] == tc.ALIGN_CANDIDATES_REFUSED and (got_rows[-1] == (-1, 0)).all()
        dist.barrier()
        calls = list(backend.calls)
        dist.barrier()
        assert all(c[1] <= world * (len(queries) - 1) for c in calls)                 # the over-long query never reached a matcher
        # (2) mixed asks pending at once on every rank, in another order on each: every ask is answered as it is alone,
        #     and the matcher calls are the same, in the same order, on every rank - the candidates calls behind the parts
        asks = _mixed_asks(rows, queries, rank)
        alone = [rc._ask_all([a])[0] for a in asks]
        dist.barrier()
        together = rc._ask_all(asks)
        rc._ask(asks[0][0], 2, -1, service.ASK_TOPK)                  # one more tick: the last one has ended everywhere
        dist.barrier()
        # ... and once more from rank 0 alone, so that ONE tick holds exactly these asks: its calls can be counted
        n0 = len(backend.calls)
        dist.barrier()
        if rank == 0:
            again = rc._ask_all(asks)
            assert all((np.asarray(x[0] if a[3] != service.ASK_PARTS else x) ==
                        np.asarray(y[0] if a[3] != service.ASK_PARTS else y)).all() for a, x, y in zip(asks, together, again))
        dist.barrier()
        rc._ask(asks[0][0], 2, -1, service.ASK_TOPK)
        dist.barrier()
        for a, x, y in zip(asks, alone, together):
            if a[3] == service.ASK_PARTS:
                assert (x == y).all()
            else:
                assert (np.asarray(x[0]) == np.asarray(y[0])).all() and x[1] == y[1]
            if a[3] == service.ASK_CANDIDATES:
                _, _, c, min_count, cap = a[5]
                exp = ref.candidates(rows, [a[0].tolist()], EPS, c, min_count=min_count, cap=4096,
                                     exclude_ids=None if a[2] < 0 else [a[2]])[0]
                assert (y[0] == exp[:c]).all() and y[0].shape == (c, 2), a[5]
                assert y[1] == exp[c, 1] or (cap == 64 and abs(y[1]) == exp[c, 1])
        everyone = [None] * world
        dist.all_gather_object(everyone, list(backend.calls))
        assert all(e == everyone[0] for e in everyone)
        assert len({len(e) for e in everyone}) == 1 and n0 < len(everyone[0])
        kinds = [c[0] for c in everyone[0][n0:]]
        # ascending kind: the searches, the parts call, then the candidates calls in sorted parameters - (C, min_count, cap)
        cand = [c for c in everyone[0][n0:] if c[0] == "align_candidates"]
        assert [c[2] for c in cand] == [(EPS, 4, 6, 64), (EPS, 4, 6, 4096), (EPS, 16, 1, 4096)]
        assert [c[1] for c in cand] == [1, 1, 2]                                  # asks that agree share one call
        assert sorted(kinds) == sorted(["align_wide_topk", "align_span_topk", "align_parts"] + ["align_candidates"] * 3)
        last_parts = max(i for i, k in enumerate(kinds) if k == "align_parts")
        assert last_parts < min(i for i, k in enumerate(kinds) if k == "align_candidates")
        # (3) refused in the caller, before the tick: nothing reaches a matcher, the loop keeps running
        n1, ticks = len(backend.calls), rc.busy_ticks
        if rank == 0:
            q = [queries[1]]
            for call in (lambda: rc.align_candidates(q, c=0), lambda: rc.align_candidates(q, c=65),
                         lambda: rc.align_candidates(q, c=2.5), lambda: rc.align_candidates(q, c=16, cap=15),
                         lambda: rc.align_candidates(q, c=16, min_count=0), lambda: rc.align_candidates(q, c=16, cap=1 << 31),
                         lambda: rc.align_candidates(q, c=16, exclude_ids=[1, 2])):
                with pytest.raises(ValueError):
                    call()
            no_call = service.RankCorpus.__new__(service.RankCorpus)
            no_call.shard, no_call.matcher = shard, sharded.ShardedMatcher(NearServiceBackend(live=shard), k=8, cap=64, group=g)
            assert not no_call.supports_align_candidates
            with pytest.raises(RuntimeError, match="has no align_candidates"):
                service.RankCorpus.align_candidates(no_call, q, c=16)
            long_rows, long_totals = rc.align_candidates([[0.5] * 4096], c=4)
            assert long_totals.tolist() == [tc.ALIGN_CANDIDATES_REFUSED] and (long_rows == (-1, 0)).all()
            assert len(backend.calls) == n1 and rc.busy_ticks == ticks
        dist.barrier()
        assert rc.broken is None
        out.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        out.put((rank, repr(e)))
        raise
    finally:
        if rc is not None:
            rc.close()
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_the_tick_answers_candidates_asks_over_gloo(world):
    _run(_rank_worker, world)


# ---------------------------------------------------------------------------------------------- the inspector
class _ShardedFake(_Corpus):
    """tests/test_gap_candidates_cpu.py's fake corpus as a sharded one: it says by its flag whether it can name
    candidates (a service.RankCorpus over a matcher without the call says it cannot)."""

    def __init__(self, can=True, **kw):
        super().__init__(**kw)
        self.supports_align_candidates = can
        self.supports_align_parts = True


def test_inspector_over_a_fake_sharded_corpus():
    from tvidz_amd import inspector as insp
    ok = dict(device="cuda:0", near_duplicates=True, near_top_k=8, near_any_offset=True, near_score="local", near_min_votes=8,
              near_jaccard=0.9)
    cuts = [float(3 * i) for i in range(128, -1, -1)]
    with pytest.raises(RuntimeError, match="has no align_candidates.*ShardedCorpus"):
        insp.Inspector(_Store(_ShardedFake(can=False)), **dict(ok, near_candidates=16))
    # unset: untouched - no switch, no candidates call
    corpus = _ShardedFake()
    (plain,) = insp.Inspector(_Store(corpus), **ok)._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["align_span_topk"]
    # set: the switch once, one candidates call and one parts call per upload, the sweep's entry
    corpus = _ShardedFake()
    ins = insp.Inspector(_Store(corpus), **dict(ok, near_candidates=16, near_gap_eps=0.05))
    (near,) = ins._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["set_gap_index", "align_candidates", "align_parts"] and near == plain
    # the two product corpora say they can
    assert service.ShardedCorpus.supports_align_candidates.fget(object()) is True
    assert hasattr(service.ShardedCorpus, "set_gap_index") and hasattr(service.RankCorpus, "set_gap_index")
    assert sharded.RcclShardedMatcher.supports_align_candidates is True


# -------------------------------------------------------------------------------------------- the code object
def test_the_merge_kernel_exists_once_with_no_scratch_and_no_spills(kernels):  # noqa: F811
    found = [k for n, k in kernels.items() if "20ts_gapc_merge_kernelE" in n]
    assert len(found) == 1, sorted(n for n in kernels if "gapc" in n)
    (k,) = found
    assert k[".private_segment_fixed_size"] == 0
    assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0
    print("vgprs, sgprs, static LDS bytes, block:", k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"],
          k[".max_flat_workgroup_size"])
    # a wave per query, four per block; its LDS is dynamic (n_lists x C words per wave: 32 KiB per block at the most)
    assert k[".max_flat_workgroup_size"] == 256 and k[".group_segment_fixed_size"] == 0 and k[".vgpr_count"] <= 64


# ------------------------------------------------------------------------------------ the host code, sanitized
def _program():
    sources = sorted(os.path.join(tbuild.CSRC, f) for f in os.listdir(tbuild.CSRC)) + \
        [os.path.join(tbuild.INCLUDE, h) for h in ("tvz.h", "tvz_gap.h", "tvz_gap_shards.h")] + [MAIN]
    h = hashlib.sha1()
    for f in sources:
        h.update(open(f, "rb").read())
    cache = os.path.join(tempfile.gettempdir(), f"tvz-host-sanitizer-{os.getuid()}")
    os.makedirs(cache, exist_ok=True)
    exe = os.path.join(cache, "gapc-shards-" + h.hexdigest()[:16])
    if not os.path.exists(exe):
        # (the device half is compiled because the translation unit registers its kernels; unoptimised: it never runs)
        subprocess.check_call([tbuild._hipcc(), f"--offload-arch={tbuild.ARCH}", "-O1", "-Xarch_device", "-O0", "-std=c++17",
                               "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                               "-Wno-unused-function", f"-I{tbuild.INCLUDE}", f"-I{tbuild.CSRC}", "-o", exe + f".{os.getpid()}.tmp",
                               MAIN, os.path.join(tbuild.CSRC, "tvz_api.hip"), os.path.join(tbuild.CSRC, "tvz_comm.hip"), "-ldl"])
        os.replace(exe + f".{os.getpid()}.tmp", exe)
    return exe


def test_host_sharded_carving_and_refusals_under_asan_and_ubsan():
    """The sharded workspace is carved inside its buffer at every misalignment, the plain call's part behind the blocks,
    and the three new calls make their early refusals with no invalid access."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([_program()], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("HOST_OK"), (out.stdout[-500:], out.stderr[-3000:])
