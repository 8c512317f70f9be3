"""GPU parity of tvz_align_parts_flags (ts_alignp2_walk_kernel under TVZ_ALIGN_TWO_BINS; the existing walk with the flag
clear) against tests/align_parts_two_bins_ref.py: whole [Q, k, 1 + max_parts, 6] outputs, exact integers throughout.
The table and the uploads are tests/align_parts_two_bins_cases.py's; their premises are asserted without a device in
tests/test_align_parts_two_bins_cpu.py, and the ones a test leans on again here."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import align_parts_cases as pc, align_parts_two_bins_cases as cs, align_parts_two_bins_ref as ref
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = cs.EPS
MAX_B = cs.MAX_B
TWO = ref.TWO_BINS
SENTINEL = -0x5A5A5A5A
CANARY = 0xA5
INT32_MIN = -(1 << 31)
ERR_INVALID, ERR_UNSUPPORTED = -1, -4                               # include/tvz.h


@pytest.fixture(scope="module")
def world():
    """-> (rows, uploads, dc): the table on the device, once; no test changes it"""
    rows, uploads = cs.table(), cs.uploads()
    dc = tc.DeviceCorpus(0)
    dc.upload(rows)
    yield rows, uploads, dc
    dc.close()


def _same(got, exp, what):
    got = np.asarray(got, dtype=np.int64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere((got != exp).any(axis=(2, 3)))
    assert bad.size == 0, (what, f"{len(bad)} pairs differ", [(q, j, got[q, j].tolist(), exp[q, j].tolist()) for q, j in bad[:3].tolist()])


def _check(dc, rows, queries, ids, B, rates=(1.0,), min_votes=1, max_parts=4, max_query_len=None, two_bins=True):
    exp = ref.align_parts_flags_ref(rows, queries, ids, EPS, B * EPS, rates, min_votes, max_parts, TWO if two_bins else 0,
                                    max_query_len)
    got = dc.align_parts(queries, ids, eps=EPS, max_offset=B * EPS, rates=rates, min_votes=min_votes, max_parts=max_parts,
                         max_query_len=max_query_len, two_bins=two_bins)
    assert got.dtype == np.int32
    _same(got, exp, (B, rates, min_votes, max_parts, two_bins))
    return exp


def _raw(dc, queries, ids, k, flags, eps=EPS, mo=30.0, rates=(1.0,), min_votes=1, max_parts=2, out=None, ws_ptr=None,
         ws_bytes=None, old=False):
    """tvz_align_parts_flags (old: tvz_align_parts, without the flags) by the C ABI -> (rc, out, need)"""
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    L, Q = min(longest, 4095), len(queries)
    d_ids = torch.as_tensor(np.asarray(ids, dtype=np.int32).reshape(Q, -1)).to(DEV)
    if out is None:
        out = torch.full((Q, max(k, 1), 1 + min(max(max_parts, 1), 4), 6), SENTINEL, dtype=torch.int32, device=DEV)
    need = tc.align_parts_workspace_bytes(Q, L, d_q.numel(), min(max(k, 1), 64), min(max(max_parts, 1), 4))
    ws = None
    if ws_ptr is None:
        ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
        ws_ptr = ws.data_ptr()
    h = (C.c_double * max(len(rates), 1))(*rates)
    s = torch.cuda.current_stream(DEV)
    front = (dc._h, d_q.data_ptr(), d_off.data_ptr(), Q, int(L), d_ids.data_ptr(), 1, d_ids.shape[1], int(k), float(eps), float(mo),
             h, len(rates), int(min_votes), int(max_parts))
    back = (out.data_ptr(), ws_ptr, need if ws_bytes is None else ws_bytes, s.cuda_stream)
    lib = _lib.load()
    rc = lib.tvz_align_parts(*front, *back) if old else lib.tvz_align_parts_flags(*front, int(flags), *back)
    s.synchronize()
    return rc, out, need


# ----------------------------------------------------------------------------------------- 1. the flag clear
def test_flag_clear_is_the_old_exports_block_for_every_upload_of_the_parts_cases():
    """tests/align_parts_cases.py's table and every upload of it: flags = 0 through the new export writes what
    tvz_align_parts writes, inside an exact-size workspace in an arena of 0xA5 at three misalignments."""
    rows, uploads = pc.table(), pc.uploads()
    dc = tc.DeviceCorpus(0)
    try:
        dc.upload(rows)
        names = list(uploads)
        ids_all = list(pc.IDS)
        for lo in range(0, len(names), 8):                                     # Q <= 8
            queries = [uploads[n] for n in names[lo:lo + 8]]
            ids = [ids_all] * len(queries)
            k = len(ids_all)
            for (B, rates, max_parts, min_votes), mis in zip(((900, (1.0,), 4, 1), (MAX_B, (1.0, 0.96), 3, 8), (5000, (0.96, 1.0), 2, 1)),
                                                             (0, 8, 248)):
                kw = dict(mo=B * EPS, rates=rates, min_votes=min_votes, max_parts=max_parts)
                rc, old, need = _raw(dc, queries, ids, k, 0, old=True, **kw)
                assert rc == 0, _lib.load().tvz_last_error()
                arena = torch.full((need + 1024,), CANARY, dtype=torch.uint8, device=DEV)
                at = (-arena.data_ptr()) % 256 + 256 + mis
                rc, new, _ = _raw(dc, queries, ids, k, 0, ws_ptr=arena.data_ptr() + at, ws_bytes=need, **kw)
                assert rc == 0, _lib.load().tvz_last_error()
                assert torch.equal(old, new), (lo, B, rates)
                a = arena.cpu().numpy()
                assert (a[:at] == CANARY).all() and (a[at + need:] == CANARY).all(), mis
                exp = ref.align_parts_flags_ref(rows, queries, ids, EPS, B * EPS, rates, min_votes, max_parts, 0)
                _same(new.cpu().numpy(), exp, ("flag clear", lo, B))
    finally:
        dc.close()


def test_the_flags_refusals_leave_the_output_alone_and_sit_between_max_parts_and_the_bins(world):
    rows, uploads, dc = world
    q, ids = [uploads["copy"]], [[cs.FILM, cs.ABSENT]]
    err = lambda: _lib.load().tvz_last_error()                                  # noqa: E731
    for flags, bits in ((4, b"0x4"), (1, b"0x1"), (8 | 1, b"0x1"), (0x80000008, b"0x80000000"), (2, b"0x2")):
        rc, out, _ = _raw(dc, q, ids, 2, flags)
        assert rc == ERR_INVALID and b"alignment parts: unknown flag bits " + bits in err(), (flags, rc, err())
        assert (out.cpu().numpy() == SENTINEL).all(), flags
    rc, out, _ = _raw(dc, q, ids, 2, 4, max_parts=5)                            # max_parts in front of the flags
    assert rc == ERR_UNSUPPORTED and b"max_parts=5" in err()
    rc, out, _ = _raw(dc, q, ids, 2, 4, eps=0.0)                                # the flags in front of eps
    assert rc == ERR_INVALID and b"unknown flag bits 0x4" in err()
    rc, out, _ = _raw(dc, q, ids, 2, 4, mo=(MAX_B + 1) * EPS)                   # ... and of B
    assert rc == ERR_INVALID and b"unknown flag bits 0x4" in err()
    rc, out, _ = _raw(dc, q, ids, 2, TWO, eps=0.0)
    assert rc == ERR_INVALID and b"eps must be > 0" in err() and (out.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------------------------- 2. the film's uploads
def test_the_retimed_copy_with_an_insertion_has_no_part_in_single_bins_and_two_in_windows(world):
    rows, uploads, dc = world
    q, ids = [uploads["retimed_inserted"]], [[cs.REELS, cs.FILM]]
    for B in (cs.seam_B()[0] * 2, MAX_B):
        clear = _check(dc, rows, q, ids, B, min_votes=61, max_parts=4, two_bins=False)
        flag = _check(dc, rows, q, ids, B, min_votes=61, max_parts=4)
        assert clear[0, 0, 0].tolist() == [cs.REELS, 200, 0, 0, 1, 209] and not clear[0, 0, 1:].any()
        assert flag[0, 0, 0].tolist() == [cs.REELS, 200, 0, 2, 1, 209]
        assert flag[0, 0, 1:3].tolist() == [[2284, 100, 109, 208, 100, 100], [3703, 100, 0, 99, 100, 100]]


@pytest.mark.parametrize("B", (0, 1, 900, cs.seam_B()[0], MAX_B))
def test_the_films_uploads_at_a_third_of_a_bin_under_every_bound_and_rate_order(world, B):
    """The copy, the removal, two insertions, two clips swapped, the stranger, the re-timed and the 24 -> 25 fps copies
    with an insertion and the upload of NaN, infinities, zeros and duplicates; both orders of the rate list."""
    rows, uploads, dc = world
    queries = list(uploads.values())
    assert len(queries) == 8
    ids = [[cs.FILM, cs.REELS, cs.SPECIAL]] * len(queries)
    for rates in ((1.0,), (1.0, 0.96), (0.96, 1.0)):
        exp = _check(dc, rows, queries, ids, B, rates, 8 if B >= 900 else 1, 4)
        if B == MAX_B:
            q = list(uploads).index("fps_inserted")
            assert exp[q, 0, 0].tolist() == [cs.FILM, 120, rates.index(0.96) if 0.96 in rates else 0, 2 if 0.96 in rates else 0, 1, 129]
            if 0.96 in rates:
                assert exp[q, 0, 1:3, :2].tolist() == [[-1060, 59], [360, 57]]
            assert exp[list(uploads).index("copy"), 0, 1].tolist() == [0, 120, 0, 119, 120, 120]


def test_every_part_count_and_bar(world):
    rows, uploads, dc = world
    queries = list(uploads.values())
    ids = [[cs.FILM, cs.REELS]] * len(queries)
    for max_parts in (1, 2, 3, 4):
        for min_votes in (1, 8, 61):
            _check(dc, rows, queries, ids, MAX_B, (1.0, 0.96), min_votes, max_parts)


# ------------------------------------------------------------------------------------------------ 3. the carry
@pytest.mark.parametrize("extra", (0, 517, MAX_B))
def test_a_rate_that_leaves_its_lowest_bin_behind_in_front_of_a_better_rate(world, extra):
    rows, uploads, dc = world
    B, W = cs.seam_B()
    B = MAX_B if extra == MAX_B else B + extra
    exp = _check(dc, rows, [cs.LONE_Q], [[cs.RATE_CARRY, cs.ONLY_B]], B, (1.0, 1.04), 1, 2)
    if extra == 0:                                                              # the premise (also in the CPU test)
        assert exp[0, 0].tolist() == [[cs.RATE_CARRY, 9, 1, 1, 1, 1], [2 * W - 1, 6, 0, 0, 1, 6], [0] * 6]
    _check(dc, rows, [cs.LONE_Q], [[cs.RATE_CARRY, cs.ONLY_B]], B, (1.04, 1.0), 1, 2)


@pytest.mark.parametrize("extra", (0, 517, MAX_B))
def test_the_best_pair_of_bins_across_a_seam_in_part_0_and_in_part_1(world, extra):
    rows, uploads, dc = world
    B, W = cs.seam_B()
    Bc = MAX_B if extra == MAX_B else B + extra
    ids = [list(cs.SEAM_IDS)] * 2
    exp = _check(dc, rows, [cs.SEAM_Q, cs.LONE_Q], ids, Bc, (1.0,), 1, 3)
    for i, S in enumerate((-W, 0, W, 2 * W)):
        assert exp[0, i, 1].tolist() == [S - 1, 64, 0, 7, 8, 106], (i, S)
    for i, S in enumerate((-W, W)):
        # part 1 counts the 16 ALLOWED votes of bin S beside S - 1's 12; all 24 of bin S would make it 36
        assert exp[0, 4 + i, 1:3].tolist() == [[40, 40, 0, 3, 4, 48], [S - 1, 28, 4, 7, 4, 28]], (i, S)
    if extra == 0:                                                              # b + 1 > B: bin B alone
        assert exp[0, 6, 1].tolist() == [B, 24, 0, 7, 8, 52]
    _check(dc, rows, [cs.SEAM_Q, cs.LONE_Q], ids, Bc, (1.0,), 13, 4)
    _check(dc, rows, [cs.SEAM_Q], ids[:1], Bc, (1.0,), 1, 2, two_bins=False)


# -------------------------------------------------------------------------------------------- 4. the other rows
@pytest.mark.parametrize("B", (900, MAX_B))
def test_the_tie_chain_the_long_rows_and_the_rows_of_one_id(world, B):
    rows, uploads, dc = world
    rq = cs.row_queries()
    queries = list(rq.values())
    ids = [list(cs.NAMED)] * len(queries)
    exp = _check(dc, rows, queries, ids, B, (1.0,), 1, 4)
    clear = _check(dc, rows, queries, ids, B, (1.0,), 1, 4, two_bins=False)
    q, at = list(rq).index("base30"), cs.NAMED.index
    assert exp[q, at(cs.TIE0), 1].tolist() == [21, 10, 4, 13, 10, 10]                       # J ties: the more votes of its own
    assert exp[q, at(cs.TIE0 + 100), 1:3].tolist() == [[-11, 8, 0, 7, 8, 8], [11, 8, 8, 15, 8, 8]]        # ... the negative one
    assert exp[q, at(cs.TIE_LATER), 1:4].tolist() == [[0, 12, 0, 11, 12, 12], [-5, 8, 12, 19, 8, 8], [5, 8, 20, 27, 8, 8]]
    assert exp[q, at(cs.TIE_LATER + 100), 1:3].tolist() == [[0, 12, 0, 11, 12, 12], [51, 8, 15, 22, 8, 8]]
    # the second row is better only under the flag; equal windows keep the earlier row; nine rows are refused
    assert clear[q, at(cs.FLAG_BETTER), :2].tolist() == [[cs.FLAG_BETTER, 10, 0, 1, 2, 30], [30, 10, 0, 9, 10, 10]]
    assert exp[q, at(cs.FLAG_BETTER), :2].tolist() == [[cs.FLAG_BETTER, 16, 0, 1, 2, 30], [30, 16, 0, 15, 16, 16]]
    assert exp[q, at(cs.EQUAL_J), :2].tolist() == [[cs.EQUAL_J, 11, 0, 2, 2, 30], [-7, 9, 0, 8, 9, 9]]
    assert exp[q, at(cs.NINE_ROWS), 0].tolist() == [cs.NINE_ROWS, 0, 0, INT32_MIN, 9, 30]
    assert exp[q, at(cs.ABSENT), 0].tolist() == [cs.ABSENT, 0, 0, 0, 0, 30] and exp[q, at(-1), 0].tolist() == [-1, 0, 0, 0, 0, 30]
    q = list(rq).index("parts24")
    for vid in (cs.LANES64, cs.LANES65):
        assert exp[q, at(vid), 1:3].tolist() == [[-100, 12, 0, 11, 12, 34], [400, 12, 12, 23, 12, 24]]


def test_no_query_and_a_query_too_long_beside_a_good_one(world):
    rows, uploads, dc = world
    got = dc.align_parts([], [], eps=EPS, min_votes=1, max_parts=2, two_bins=True)
    assert got.shape[0] == 0
    long = np.linspace(0.0, 4000.0, 4096).tolist()
    queries, ids = [long, uploads["copy"]], [[cs.FILM, -1, cs.ABSENT]] * 2
    exp = _check(dc, rows, queries, ids, MAX_B, max_query_len=200)
    assert exp[0, :, 0].tolist() == [[cs.FILM, 0, 0, INT32_MIN, 1, 0], [-1, 0, 0, 0, 0, 0], [cs.ABSENT, 0, 0, INT32_MIN, 0, 0]]
    assert exp[1, 0, :2].tolist() == [[cs.FILM, 120, 0, 1, 1, 120], [0, 120, 0, 119, 120, 120]]


# ------------------------------------------------------------------------------ 5. cross-check with the search
def test_part_0_is_the_two_bin_span_searchs_hit_and_its_block_is_taken_by_strides():
    from tests import align_two_bins_cases as tb
    rows, queries, _ = tb.main_table()
    assert len({v for v, _ in rows}) == len(rows)                                # every id once: the hit's row is the pair's
    dc = tc.DeviceCorpus(0)
    try:
        dc.upload(rows)
        k, B = 16, tb.MAIN_B
        d_q, d_off, L = tc.pack_queries(queries, DEV)
        block = dc.align_span_topk_block(d_q, d_off, L, eps=tb.E64, max_offset=B * tb.E64, rates=tb.MAIN_RATES, k=k, min_votes=1,
                                         two_bins=True)
        ids = block[:, :k, 0]
        assert ids.stride() == ((k + 1) * 8, 8)
        parts = dc.align_parts_block(d_q, d_off, L, ids, eps=tb.E64, max_offset=B * tb.E64, rates=tb.MAIN_RATES, min_votes=1,
                                     max_parts=3, two_bins=True).cpu().numpy()
        hits = block.cpu().numpy()
        _same(parts, ref.align_parts_flags_ref(rows, queries, hits[:, :k, 0], tb.E64, B * tb.E64, tb.MAIN_RATES, 1, 3, TWO), "span block")
        seen = 0
        for q in range(len(queries)):
            for j in range(k):
                vid, row_len, best_bin, votes, rate, t_first, t_last, nr = hits[q, j].tolist()
                if vid < 0:
                    assert parts[q, j, 0].tolist()[:5] == [-1, 0, 0, 0, 0]
                else:
                    seen += 1
                    assert parts[q, j, 0].tolist()[:3] == [vid, row_len, rate] and parts[q, j, 0, 3] >= 1
                    assert parts[q, j, 1].tolist() == [best_bin, votes, t_first, t_last, t_last - t_first + 1, nr], (q, j)
        assert seen > 40
    finally:
        dc.close()


# ------------------------------------------------------------------------------------------------ 6. the shards
@pytest.mark.parametrize("R", (3, 20))
def test_sharded_corpus_is_one_device_corpus_with_an_ids_rows_in_different_shards(world, R):
    from tvidz_amd import service
    rows, uploads, dc = world
    sc = service.ShardedCorpus(0, n_shards=R)
    try:
        assert sc.supports_align_parts_two_bins and dc.supports_align_parts_two_bins
        shard_rows = [[] for _ in range(R)]
        seen = {}
        for vid, keys in rows:
            n = seen[vid] = seen.get(vid, -1) + 1
            shard_rows[(vid + n) % R].append((vid, keys))
        for s, part in zip(sc.shards, shard_rows):
            s.upload(part)
        queries = [cs.row_queries()["base30"], uploads["retimed_inserted"], uploads["two_inserted"]]
        ids = [[cs.FLAG_BETTER, cs.EQUAL_J, cs.NINE_ROWS, cs.FILM, cs.REELS, cs.TIE_LATER, cs.ABSENT, -1]] * 3
        for B, max_parts, min_votes in ((MAX_B, 4, 1), (5000, 2, 8)):
            got = sc.align_parts(queries, ids, eps=EPS, max_offset=B * EPS, min_votes=min_votes, max_parts=max_parts, two_bins=True)
            one = dc.align_parts(queries, ids, eps=EPS, max_offset=B * EPS, min_votes=min_votes, max_parts=max_parts, two_bins=True)
            one = np.asarray(one, dtype=np.int64)
            # nine rows of one id in ONE corpus are refused; over the shards they are answered.  Two rows with equal
            # windows in two shards: the merge keeps the lower shard's, one corpus the earlier row.  Both are compared
            # with the shards' references merged, below
            nine, equal = ids[0].index(cs.NINE_ROWS), ids[0].index(cs.EQUAL_J)
            keep = [j for j in range(len(ids[0])) if j not in (nine, equal)]
            _same(np.asarray(got)[:, keep], one[:, keep], (R, B, "against one DeviceCorpus"))
            assert (one[:, nine, 0, 3] == INT32_MIN).all() and (np.asarray(got)[:, nine, 0, 4] == 9).all()
            answers = [ref.align_parts_flags_ref(part, queries, ids, EPS, B * EPS, (1.0,), min_votes, max_parts, TWO) for part in shard_rows]
            from tests.align_parts_ref import merge_shards_ref
            _same(got, merge_shards_ref(answers), (R, B, max_parts, min_votes))
        assert one[0, 0, 0].tolist()[:2] == [cs.FLAG_BETTER, 16] and one[0, 0, 0, 4] == 2
    finally:
        sc.close()


# --------------------------------------------------------------------------------------------- 7. the inspector
def test_inspector_reports_the_retimed_copy_with_an_insertion(world):
    from tvidz_amd import inspector as insp
    rows, uploads, dc = world

    class Store:
        corpus = dc

        def get_video_by_id(self, vid):
            return None

    upload = uploads["retimed_inserted"]
    s = sorted(upload)
    kw = dict(device=DEV, near_duplicates=True, near_top_k=4, near_any_offset=True, near_score="local", near_min_votes=61,
              near_jaccard=0.9)
    try:
        # the candidate path under two bins: part 0, at the window's middle
        # (the film itself is reported too: the reels' first hundred cuts are its own)
        found = insp.Inspector(Store(), near_candidates=8, near_two_bins=True, near_parts_two_bins=True, **kw)._near(424242, upload)
        assert sorted(d["video_id"] for d in found) == [cs.FILM, cs.REELS]
        (near,) = [d for d in found if d["video_id"] == cs.REELS]
        assert near["video_id"] == cs.REELS and near["shift_seconds"] == (2284 + 0.5) * EPS and near["local"] == 1.0
        assert near["upload_span"] == [s[109], s[208]]
        # with near_parts both parts, through the sweep and through the candidates
        for more in (dict(), dict(near_candidates=8)):
            found = insp.Inspector(Store(), near_parts=2, near_two_bins=True, near_parts_two_bins=True, **kw, **more)._near(424242, upload)
            (near,) = [d for d in found if d["video_id"] == cs.REELS]
            assert [p["votes"] for p in near["parts"]] == [100, 100] and near["parts_score"] == 1.0
            assert [p["shift_seconds"] for p in near["parts"]] == [(2284 + 0.5) * EPS, (3703 + 0.5) * EPS]
            assert near["parts"][1]["upload_span"] == [s[0], s[99]]
            assert near["parts"][1]["stored_span"] == [s[0] + (3703 + 0.5) * EPS, s[99] + (3703 + 0.5) * EPS]
        # the same configuration without two bins reports nothing
        assert insp.Inspector(Store(), near_parts=2, **kw)._near(424242, upload) == []
        assert insp.Inspector(Store(), near_parts=2, near_candidates=8, **kw)._near(424242, upload) == []
    finally:
        dc.set_gap_index(0.0)
