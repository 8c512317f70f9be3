"""GPU parity of tvz_align_candidates_long (ts_gapl_offsets_kernel, ts_gapl_probe_kernel, the lookup over the handle's
code table, ts_gapl_fold_kernel) against tests/gap_candidates_long_ref.py: whole [Q, C + 1, 2] blocks, exact integers
throughout.  The table and the uploads are tests/gap_candidates_long_cases.py's; their premises are asserted without a
device in tests/test_gap_candidates_long_cpu.py.  Only the test of a list that overflows `cap` compares less than the
whole block, as the contract fixes less there."""
import numpy as np
import pytest
import torch

from tests import gap_candidates_cases as cs, gap_candidates_long_cases as lc, gap_candidates_long_ref as lref
from tests import gap_candidates_ref as ref
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = lc.GAP_EPS
SENTINEL = -0x5A5A5A5A
CANARY = 0xA5
INT32_MIN = -(1 << 31)
ERR_UNSUPPORTED, ERR_WORKSPACE = -4, -5                            # include/tvz.h
LDS_ENTRIES = tc.ALIGN_CANDIDATES_LONG_LDS_ENTRIES


@pytest.fixture(scope="module")
def world():
    """-> (rows, uploads, dc, seg): the table on the device with its gap codes, once, and the reference's per-segment
    counts of every upload, once; no test that takes it changes either"""
    rows, uploads = lc.table(), lc.uploads()
    dc = tc.DeviceCorpus(0)
    dc.upload(rows)
    dc.set_gap_index(EPS)
    sets = [ref.stored_codes(k, EPS) for _, k in rows]
    seg = {n: lref.segment_counts(rows, q, EPS, sets) for n, q in uploads.items()}
    yield rows, uploads, dc, seg
    dc.close()


@pytest.fixture(scope="module")
def scratch():
    """a handle the tests of the fold's limits fill as they like"""
    dc = tc.DeviceCorpus(0)
    yield dc
    dc.close()


def _block(dc, queries, c, **kw):
    rows, totals = dc.align_candidates_long(queries, c=c, **kw)
    assert rows.dtype == np.int32 and rows.shape == (len(queries), c, 2) and totals.shape == (len(queries),)
    out = np.zeros((len(queries), c + 1, 2), dtype=np.int64)
    out[:, :c], out[:, c, 0], out[:, c, 1] = rows, -1, totals
    return out


def _same(got, exp, what):
    bad = np.argwhere((got != exp).any(axis=(1, 2)))
    assert bad.size == 0, (what, [(int(q), got[q].tolist(), exp[q].tolist()) for q in bad[:2, 0]])


def _check(dc, rows, queries, c, what=None, **kw):
    exp = lref.candidates(rows, queries, EPS, c, **kw).astype(np.int64)
    _same(_block(dc, queries, c, **kw), exp, (what, kw))
    return exp


def _expected(rows, names, uploads, seg, c, min_count, cap=4096, excl=None, max_query_len=4095):
    ids = [i for i, _ in rows]
    out = np.zeros((len(names), c + 1, 2), dtype=np.int64)
    for i, n in enumerate(names):
        if len(uploads[n]) > max_query_len:
            out[i, :, 0], out[i, c, 1] = -1, INT32_MIN
        else:
            out[i] = lref.block_of(ids, seg[n], c, cap, min_count, -1 if excl is None else excl[i])
    return out


# ------------------------------------------------------------------------------------------ 1. the cases
@pytest.mark.parametrize("c", (1, 16, 64))
def test_every_upload_against_the_table(world, c):
    """Uploads of 514, 515, 1,025, 1,026 and 4,095 values, one of 4,096 (refused) beside them, a short and an empty one:
    the row with a hit on either side of a boundary, min_count - 1 in one segment and min_count in another, ids hit in
    1, 2 and all 9 segments, rows of one id summed, ties by id, exclusions."""
    rows, uploads, dc, seg = world
    names = list(uploads)
    queries = [uploads[n] for n in names]
    for min_count in (1, 2, 3):
        exp = _expected(rows, names, uploads, seg, c, min_count)
        _same(_block(dc, queries, c, min_count=min_count), exp, (c, min_count))
        at = {n: exp[i] for i, n in enumerate(names)}
        assert at["m4096"][c].tolist() == [-1, INT32_MIN] and (at["m4096"][:c] == (-1, 0)).all()
        assert at["empty"][c].tolist() == [-1, 0] and at["m4095"][c, 1] == {1: 8, 2: 7, 3: 6}[min_count]
        assert at["m4095"][0].tolist() == [lc.ALL9, 7 * 8 + 4] and at["short"][0].tolist() == [lc.ONE_SEG, 37]
    excl = [lc.ALL9 if n != "short" else lc.ONE_SEG for n in names]
    exp = _expected(rows, names, uploads, seg, c, 1, excl=excl)
    _same(_block(dc, queries, c, min_count=1, exclude_ids=excl), exp, (c, "exclusions"))
    assert exp[names.index("m4095"), 0, 0] == lc.TWIN and exp[names.index("short"), c, 1] == 0
    # the reference's block function is the reference: one upload through lref.candidates itself
    _check(dc, rows, [uploads["m1026"], uploads["m515"]], c, "whole reference", min_count=2)


def test_no_query_and_a_call_whose_longest_query_is_refused(world):
    rows, uploads, dc, seg = world
    rows_, totals = dc.align_candidates_long([], c=4)
    assert rows_.shape == (0, 4, 2) and totals.shape == (0,)
    # max_query_len 1,026: three lists per query; the master is longer and refused, the others are answered
    names = ["m4095", "m1026", "m515", "short"]
    exp = _expected(rows, names, uploads, seg, 8, 1, max_query_len=1026)
    _same(_block(dc, [uploads[n] for n in names], 8, min_count=1, max_query_len=1026), exp, "max_query_len 1026")
    assert exp[:, 8, 1].tolist()[0] == INT32_MIN and (exp[1:, 8, 1] > 0).all()


# ------------------------------------------------------------------------------- 2. the limits of the fold
def _limit(dc, ids, cap, c=16):
    table = lc.limit_table(ids)
    dc.upload(table)
    dc.set_gap_index(EPS)
    order = sorted(ids)
    exp = np.zeros((1, c + 1, 2), dtype=np.int64)
    exp[0, :, 0] = -1
    exp[0, :c] = [(v, 1) for v in order[:c]]
    exp[0, c, 1] = len(ids)
    return table, exp


@pytest.mark.parametrize("n", (LDS_ENTRIES - 1, LDS_ENTRIES, LDS_ENTRIES + 1))
def test_entries_at_the_lds_table_limit(scratch, n):
    """n rows that all carry the query's one code, min_count 1, cap above n: n entries of one segment, each an id of
    its own - the table in LDS up to LDS_ENTRIES, in the workspace one above."""
    ids = [7000 + 3 * i for i in range(n)]
    table, exp = _limit(scratch, ids, n + 8)
    q = [lc.limit_query()]
    _same(_block(scratch, q, 16, min_count=1, cap=n + 8), exp, n)
    if n == LDS_ENTRIES + 1:                                       # (the reference itself, once)
        assert (lref.candidates(table, q, EPS, 16, min_count=1, cap=n + 8) == exp).all()
        exp64 = _check(scratch, table, q, 64, "c = 64", min_count=1, cap=n + 8)
        assert exp64[0, 64, 1] == n


@pytest.mark.parametrize("n", (LDS_ENTRIES, LDS_ENTRIES + 1))
def test_ids_that_share_a_home_slot_and_wrap_round_the_tables_end(scratch, n):
    """The same entry counts with 100 ids on the home slot three below the table's end - their run wraps round it - and
    100 on another: the LDS table of 4,096 slots, and the workspace table of 8,192."""
    slots = lc.table_slots(n)
    ids = lc.colliding_ids(n, slots, 3)
    assert sum(1 for v in ids if lc.home(v, slots) == slots - 3) >= 100
    _, exp = _limit(scratch, ids, n + 8)
    _same(_block(scratch, [lc.limit_query()], 16, min_count=1, cap=n + 8), exp, n)
    # ... and rows of one id beside them: two rows each for the 50 smallest ids, summed to 2, lead the block
    low = sorted(ids)[:50]
    table = lc.limit_table(ids + low)
    scratch.upload(table)
    scratch.set_gap_index(EPS)
    got = _block(scratch, [lc.limit_query()], 64, min_count=1, cap=n + 64)
    assert got[0, :50].tolist() == [[v, 2] for v in low] and got[0, 64].tolist() == [-1, n]
    assert got[0, 50:64].tolist() == [[v, 1] for v in sorted(ids)[50:64]]


def test_the_exact_size_workspace_at_three_misalignments_and_the_refusals(scratch, world):
    """The workspace is exactly tvz_align_candidates_long_workspace_bytes - the fold's table region included: S x cap
    is above LDS_ENTRIES - at bases 0, 8 and 248 bytes past a 256-byte line, inside an arena of 0xA5 bytes that is
    otherwise unchanged; the output stands between guard rows.  Then the workspace refusal, with the missing bytes,
    a NULL d_out behind it, and - last - a handle without gap codes."""
    rows, uploads, dc, seg = world
    lib = _lib.load()
    names = ["m1026", "short", "m515", "empty"]
    queries = [uploads[n] for n in names]
    c, cap, Q = 16, 700, 4                                         # 3 lists x 700 entries: a table of 8,192 slots per query
    exp = _expected(rows, names, uploads, seg, c, 1, cap=cap)
    d_q, d_off, L = tc.pack_queries(queries, DEV)
    assert L == 1026
    d_ex = torch.full((Q,), -1, dtype=torch.int32, device=DEV)
    need = tc.align_candidates_long_workspace_bytes(Q, L, d_q.numel(), cap, c)
    assert need > tc.align_candidates_long_workspace_bytes(Q, L, d_q.numel(), 680, c) + Q * 4096 * 8 - 4096
    s = torch.cuda.current_stream(DEV)

    def raw(handle, out_ptr, ws_ptr, ws_bytes):
        rc = lib.tvz_align_candidates_long(handle, d_q.data_ptr(), d_off.data_ptr(), Q, int(L), 1, d_ex.data_ptr(), cap, c,
                                           out_ptr, ws_ptr, ws_bytes, s.cuda_stream)
        s.synchronize()
        return rc

    for mis in (0, 8, 248):
        arena = torch.full((need + 1024,), CANARY, dtype=torch.uint8, device=DEV)
        at = (-arena.data_ptr()) % 256 + 256 + mis
        out = torch.full((Q + 2, c + 1, 2), SENTINEL, dtype=torch.int32, device=DEV)
        assert raw(dc._h, out[1:Q + 1].data_ptr(), arena.data_ptr() + at, need) == 0, lib.tvz_last_error()
        a = arena.cpu().numpy()
        assert (a[:at] == CANARY).all() and (a[at + need:] == CANARY).all(), mis
        o = out.cpu().numpy()
        assert (o[0] == SENTINEL).all() and (o[Q + 1] == SENTINEL).all() and (o[1:Q + 1] == exp).all(), mis
    # the refusals, in their order; nothing is written
    arena = torch.full((need + 512,), CANARY, dtype=torch.uint8, device=DEV)
    at = (-arena.data_ptr()) % 256
    out = torch.full((Q, c + 1, 2), SENTINEL, dtype=torch.int32, device=DEV)
    least = tc.align_candidates_long_workspace_bytes(Q, L, L, cap, c)        # (the call takes what holds one longest query)
    assert least < need and raw(dc._h, None, arena.data_ptr() + at, least - 1) == ERR_WORKSPACE
    assert b"1 bytes missing (size it with tvz_align_candidates_long_workspace_bytes)" in lib.tvz_last_error()
    assert raw(dc._h, None, arena.data_ptr() + at, need) != 0 and b"d_out is NULL" in lib.tvz_last_error()
    bare = tc.DeviceCorpus(0)
    try:
        bare.upload(rows)
        assert raw(bare._h, out.data_ptr(), arena.data_ptr() + at, least - 1) == ERR_WORKSPACE
        assert raw(bare._h, out.data_ptr(), arena.data_ptr() + at, need) == ERR_UNSUPPORTED
        assert b"keeps no gap codes" in lib.tvz_last_error()
    finally:
        bare.close()
    assert (arena.cpu().numpy() == CANARY).all() and (out.cpu().numpy() == SENTINEL).all()


def test_one_segments_list_overflows_cap_and_the_others_do_not(world):
    """cap = 6: segment 0 of the master finds 8 rows, no other segment more than 6.  The contract fixes the last row -
    minus the segments' true hit counts summed - and that every reported id is a candidate with no more than its
    true count; this test alone compares no more than that."""
    rows, uploads, dc, seg = world
    per_list = (seg["m4095"] >= 1).sum(axis=1)
    assert per_list[0] == 8 and per_list[1:].max() <= 6 and per_list[1:].min() >= 1
    exp = lref.candidates(rows, [uploads["m4095"]], EPS, 4, min_count=1, cap=6)
    assert exp[0, 4, 1] == -int(per_list.sum())
    got = _block(dc, [uploads["m4095"]], 4, min_count=1, cap=6)
    assert got[0, 4].tolist() == [-1, -int(per_list.sum())]
    true = lref.true_sums(rows, uploads["m4095"], EPS, min_count=1)
    named = [int(v) for v in got[0, :4, 0] if v >= 0]
    assert len(named) == len(set(named)) == 4
    for vid, n in got[0, :4]:
        assert int(vid) in true and 1 <= int(n) <= true[int(vid)], (vid, n)


# ----------------------------------------------------------------------------------------- 3. differentials
def test_one_segment_over_distinct_ids_equals_the_plain_call_bit_for_bit(scratch):
    rows = []
    for vid, k in lc.table() + cs.counting_table(40):
        if vid not in [v for v, _ in rows]:
            rows.append((vid, k))
    scratch.upload(rows)
    scratch.set_gap_index(EPS)
    u = lc.uploads()
    queries = [u["m514"], u["short"], [], lc.master()[:4], lc.master()[:3], cs.counting_query(), cs.uploads()["special"],
               cs.long_query(514, 1)]
    d_q, d_off, L = tc.pack_queries(queries, DEV)
    assert L == 514
    excl = torch.tensor([-1, lc.ONE_SEG, -1, -1, -1, rows[-7][0], -1, -1], dtype=torch.int32, device=DEV)
    seen = 0
    for c, min_count, cap, ex in ((1, 1, 4096, None), (16, 2, 4096, excl), (64, 1, 64, excl), (16, 3, 4096, None), (8, 1, 8, None)):
        a = scratch.align_candidates_block(d_q, d_off, L, c=c, min_count=min_count, cap=cap, d_exclude_ids=ex)
        b = scratch.align_candidates_long_block(d_q, d_off, L, c=c, min_count=min_count, cap=cap, d_exclude_ids=ex)
        torch.cuda.synchronize()
        over = a[:, c, 1] < 0                                      # (an overflowed list: the rows may be inexact in both)
        assert torch.equal(a[:, c], b[:, c]) and torch.equal(a[~over], b[~over]), (c, min_count, cap)
        seen += int((a[:, :c, 0] >= 0).sum())
    assert seen > 100


def test_a_seeded_random_slice_against_the_reference(scratch):
    """About 200 rows cut out of three films, ids drawn from a pool so that some repeat; uploads of 4 to 1,600 values
    cut out of the same films with cuts dropped; min_count 1 to 3."""
    rng = np.random.default_rng(2024)
    films = [np.asarray(cs.long_query(1700, 300 + i)) for i in range(3)]
    rows = []
    for i in range(200):
        f = films[int(rng.integers(3))]
        a, n = int(rng.integers(0, 1600)), int(rng.integers(4, 90))
        rows.append((int(rng.integers(1, 140)), (f[a:a + n] + float(rng.integers(1, 50)) * 7.0).tolist()))
    for _, k in rows:
        assert cs.edge_distance(k, EPS, stored=True) > 1e-6
    queries = []
    for n in (4, 1600, 1100, 700) + tuple(int(x) for x in rng.integers(4, 1600, size=4)):
        f = films[int(rng.integers(3))]
        a = int(rng.integers(0, 1700 - n + 1))
        q = f[a:a + n]
        if n > 50:
            q = np.delete(q, rng.choice(n, size=n // 40, replace=False))
        assert cs.edge_distance(q, EPS, stored=False) > 1e-6
        queries.append((q + 9000.0).tolist())
    scratch.upload(rows)
    scratch.set_gap_index(EPS)
    S = [lref.segments(len(q)) for q in queries]
    assert sum(1 for s in S if s == 2) >= 1 and sum(1 for s in S if s >= 3) >= 2
    multi = 0
    ids = np.asarray([v for v, _ in rows])
    for q in queries:
        seg = lref.segment_counts(rows, q, EPS)
        for vid in set(ids.tolist()):
            multi += int(np.count_nonzero(seg[:, ids == vid].sum(axis=1)) > 1)
    assert multi > 0                                               # an id hit in more than one segment
    excl = [int(ids[i]) if i % 3 == 0 else -1 for i in range(len(queries))]
    for c, min_count, ex in ((16, 1, None), (64, 2, excl), (5, 3, None)):
        exp = _check(scratch, rows, queries, c, "random", min_count=min_count, exclude_ids=ex)
        assert (exp[:, c, 1] >= 0).all() and (exp[:, 0, 0] >= 0).sum() >= 4


# ------------------------------------------------------------------------------------------- 4. end to end
def test_a_1200_cut_upload_names_its_stored_copy_and_align_parts_aligns_it(scratch):
    """The upload is a stored row of 1,200 cuts shifted by an hour (and 11 ms: a third of an offset bin of 1/30 s
    from its middle): the true row leads the block, and part 0 of the parts call, fed the block by strides, holds all 1,200
    votes."""
    film = np.asarray(cs.long_query(1200, 900))
    rows = [(50 + i, cs.long_query(900 + 100 * i, 910 + i)) for i in range(4)] + [(77, film.tolist())] + \
        [(90 + i, (film[300 * i:300 * i + 40] + 5.0).tolist()) for i in range(3)]
    scratch.upload(rows)
    scratch.set_gap_index(EPS)
    upload = (film + cs.HOUR + 0.011).tolist()
    c = 16
    d_q, d_off, L = tc.pack_queries([upload], DEV)
    assert L == 1200
    block = scratch.align_candidates_long_block(d_q, d_off, L, c=c, min_count=2)
    ids = block[:, :c, 0]
    assert ids.stride() == ((c + 1) * 2, 2)
    parts = scratch.align_parts_block(d_q, d_off, L, ids, eps=1 / 30, min_votes=1, max_parts=1).cpu().numpy()
    h = block.cpu().numpy()
    assert (h == lref.candidates(rows, [upload], EPS, c, min_count=2)).all()
    assert h[0, 0].tolist() == [77, 1197] and h[0, c].tolist() == [-1, 4] and sorted(h[0, 1:4, 0].tolist()) == [90, 91, 92]
    assert parts[0, 0, 0].tolist()[:4] == [77, 1200, 0, 1]
    best_bin, votes, t_first, t_last, nq, nr = (int(x) for x in parts[0, 0, 1])
    assert (votes, t_first, t_last, nq, nr) == (1200, 0, 1199, 1200, 1200) and best_bin == -108000     # floor(-3600.011 x 30 + 0.5)
    # the plain call refuses the same upload
    assert dc_refuses(scratch, upload)


def dc_refuses(dc, upload):
    _, totals = dc.align_candidates([upload], c=4)
    return int(totals[0]) == INT32_MIN
