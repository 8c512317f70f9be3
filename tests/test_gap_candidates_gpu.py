"""GPU parity of tvz_align_candidates (ts_gapc_offsets_kernel, ts_gapc_probe_kernel, the lookup over the handle's code
table, ts_gapc_select_kernel) against tests/gap_candidates_ref.py: whole [Q, C + 1, 2] blocks, exact integers
throughout.  The tables and the uploads are tests/gap_candidates_cases.py's; their premises are asserted without a
device in tests/test_gap_candidates_cpu.py."""
import numpy as np
import pytest
import torch

from tests import gap_candidates_cases as cs, gap_candidates_ref as ref
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = cs.GAP_EPS
SENTINEL = -0x5A5A5A5A
CANARY = 0xA5
INT32_MIN = -(1 << 31)
ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -4, -5           # include/tvz.h


@pytest.fixture(scope="module")
def world():
    """-> (rows, uploads, dc): the table on the device with its gap codes, once; no test that takes it changes it"""
    rows, uploads = cs.table(), cs.uploads()
    dc = tc.DeviceCorpus(0)
    dc.upload(rows)
    dc.set_gap_index(EPS)
    yield rows, uploads, dc
    dc.close()


@pytest.fixture(scope="module")
def scratch():
    """a handle the tests of the index's state fill as they like"""
    dc = tc.DeviceCorpus(0)
    yield dc
    dc.close()


def _block(dc, queries, c, **kw):
    rows, totals = dc.align_candidates(queries, c=c, **kw)
    assert rows.dtype == np.int32 and rows.shape == (len(queries), c, 2) and totals.shape == (len(queries),)
    out = np.zeros((len(queries), c + 1, 2), dtype=np.int64)
    out[:, :c], out[:, c, 0], out[:, c, 1] = rows, -1, totals
    return out


def _check(dc, rows, queries, c, what=None, gap_eps=EPS, **kw):
    exp = ref.candidates(rows, queries, gap_eps, c, **kw).astype(np.int64)
    got = _block(dc, queries, c, **kw)
    bad = np.argwhere((got != exp).any(axis=(1, 2)))
    assert bad.size == 0, (what, kw, [(int(q), got[q].tolist(), exp[q].tolist()) for q in bad[:2, 0]])
    return exp


# ------------------------------------------------------------------------------------ 1. content of the uploads
@pytest.mark.parametrize("c", (1, 16, 64))
def test_every_upload_against_the_table(world, c):
    """The copy shifted by an hour, copies jittered below gap_eps / 2, the 20-cut excerpt, the insertion, the removal, a
    stranger; NaN, +-inf, +-0 and doubled values; a gap beyond the bins; lengths 0, 3 and 4; two rows of one id."""
    rows, uploads, dc = world
    names = list(uploads)
    for min_count in (1, 2, 6):
        exp = _check(dc, rows, [uploads[n] for n in names], c, min_count=min_count)
        at = {n: exp[i] for i, n in enumerate(names)}
        assert at["shifted"][0].tolist() == [cs.FILM, 117] and at["jitter_quarter"][0].tolist() == [cs.FILM, 117]
        assert at["excerpt"][0].tolist() == [cs.FILM, 17] and at["stranger"][c].tolist() == [-1, 0]
        assert at["four"][c, 1] == (1 if min_count == 1 else 0)
        if c > 1:
            assert at["twin"][:2].tolist() == [[cs.TWIN, 16], [cs.TWIN, 16]]
    # the exclusions: the film's copy without the film, the twin's without either twin
    excl = [cs.FILM if n != "twin" else cs.TWIN for n in names]
    exp = _check(dc, rows, [uploads[n] for n in names], c, min_count=1, exclude_ids=excl)
    assert exp[names.index("shifted"), 0, 0] != cs.FILM and exp[names.index("twin"), c, 1] == 0


def test_the_probe_limit_beside_a_good_query_and_no_query(world):
    rows, uploads, dc = world
    q514, q515 = cs.long_query(514, 1), cs.long_query(515, 2)
    queries = [q515, uploads["shifted"], q514, q514 + [float("nan")], uploads["excerpt"]]
    exp = _check(dc, rows, queries, 4, min_count=1)
    assert exp[0, 4, 1] == INT32_MIN and (exp[0, :4] == (-1, 0)).all()
    assert exp[1, 0].tolist() == [cs.FILM, 117] and exp[2, 4, 1] >= 0 and exp[3, 4, 1] >= 0
    # longer than the call's max_query_len, though far below the probe limit
    exp = _check(dc, rows, [uploads["shifted"], uploads["excerpt"], uploads["four"]], 4, min_count=1, max_query_len=100)
    assert exp[:, 4, 1].tolist() == [INT32_MIN, 1, 1] and exp[1, 0].tolist() == [cs.FILM, 17]
    # a long stored copy of a long query: every one of its 511 positions is found
    dc2 = tc.DeviceCorpus(0)
    try:
        dc2.set_gap_index(EPS)
        dc2.upload([(7, (np.asarray(q514) + 1e4).tolist()), (8, uploads["stranger"])])
        exp = _check(dc2, [(7, (np.asarray(q514) + 1e4).tolist()), (8, uploads["stranger"])], [q514, q515], 2, min_count=1)
        assert exp[0, 0, 0] == 7 and exp[0, 0, 1] >= 511 and exp[1, 2, 1] == INT32_MIN
    finally:
        dc2.close()
    rows_, totals = dc.align_candidates([], c=4)
    assert rows_.shape == (0, 4, 2) and totals.shape == (0,)


def test_more_queries_than_the_offsets_scan_has_threads(scratch):
    """Q = 2,049: a thread of the one-block scan takes 3 probe lists and the last threads none; refused queries on both
    sides of a thread's boundary, queries of 3 and 0 values between those of 4, exclusions that alternate between the
    table's two ids and -1.  Whole blocks, from the reference once per (length, exclusion)."""
    dc = scratch
    rows, queries, excl = cs.scan_case()
    dc.upload(rows)
    dc.set_gap_index(EPS)
    exp, memo = cs.scan_expected(rows, queries, excl)
    assert len({tuple(v.ravel().tolist()) for v in memo.values()}) >= 4                # (not padding alone)
    got = _block(dc, queries, exclude_ids=excl, **cs.SCAN_CALL)
    bad = np.argwhere((got != exp).any(axis=(1, 2)))
    assert bad.size == 0, [(int(q), got[q].tolist(), exp[q].tolist()) for q in bad[:3, 0]]
    assert exp[cs.SCAN_LONG[0], 2, 1] == exp[cs.SCAN_LONG[1], 2, 1] == INT32_MIN


# -------------------------------------------------------------------------------- 2. table and parameter edges
@pytest.mark.parametrize("H", cs.HIT_COUNTS)
def test_hit_counts_ties_and_every_c(scratch, H):
    """H rows share codes with the query, counts 1..7 with ties that the ids decide: around C = 1, 16, 64 and around
    the selection's 64- and 256-entry steps; min_count 6 is above the lookup's own 1..5 forms."""
    dc = scratch
    table = cs.counting_table(H)
    dc.upload(table)
    dc.set_gap_index(EPS)
    q = [cs.counting_query()]
    for c in (1, 16, 64):
        for min_count in (1, 2, 6):
            exp = _check(dc, table, q, c, (H, c), min_count=min_count)
        assert _check(dc, table, q, c, (H, c), min_count=1)[0, c, 1] == H
    # the capacity of the hit list: equal to the candidates, and one below (the total is negated; the rows may be inexact)
    for c in (1, 16):
        if H >= c:
            exp = _check(dc, table, q, c, (H, c, "cap"), min_count=1, cap=max(H, c))
            assert exp[0, c, 1] == H
        if H - 1 >= c:
            got = _block(dc, q, c, min_count=1, cap=H - 1)
            assert got[0, c, 1] == -H
            ids = {vid for vid, _ in table[:H]}
            assert all(int(v) in ids and 1 <= int(n) <= 7 for v, n in got[0, :c])


def test_the_exact_size_workspace_at_three_misalignments_and_the_refusals(world):
    """The workspace is exactly tvz_align_candidates_workspace_bytes at bases 0, 8 and 248 bytes past a 256-byte line,
    inside an arena of 0xA5 bytes that is otherwise unchanged; the output stands between guard rows.  Then the refusals
    that need a handle: the workspace, with the missing bytes, and - behind it - a handle without gap codes."""
    rows, uploads, dc = world
    lib = _lib.load()
    queries = [uploads["inserted"], uploads["special"], uploads["twin"], uploads["three"]]
    c, cap, Q = 16, 40, 4
    exp = ref.candidates(rows, queries, EPS, c, min_count=1, cap=cap)
    d_q, d_off, L = tc.pack_queries(queries, DEV)
    d_ex = torch.full((Q,), -1, dtype=torch.int32, device=DEV)
    need = tc.align_candidates_workspace_bytes(Q, L, d_q.numel(), cap, c)
    s = torch.cuda.current_stream(DEV)

    def raw(handle, out, ws_ptr, ws_bytes, c_=c, cap_=cap, min_count=1, L_=L):
        rc = lib.tvz_align_candidates(handle, d_q.data_ptr(), d_off.data_ptr(), Q, int(L_), min_count, d_ex.data_ptr(), cap_, c_,
                                      out.data_ptr(), ws_ptr, ws_bytes, s.cuda_stream)
        s.synchronize()
        return rc

    for mis in (0, 8, 248):
        arena = torch.full((need + 1024,), CANARY, dtype=torch.uint8, device=DEV)
        at = (-arena.data_ptr()) % 256 + 256 + mis
        out = torch.full((Q + 2, c + 1, 2), SENTINEL, dtype=torch.int32, device=DEV)
        assert raw(dc._h, out[1:Q + 1], arena.data_ptr() + at, need) == 0, lib.tvz_last_error()
        a = arena.cpu().numpy()
        assert (a[:at] == CANARY).all() and (a[at + need:] == CANARY).all(), mis
        o = out.cpu().numpy()
        assert (o[0] == SENTINEL).all() and (o[Q + 1] == SENTINEL).all() and (o[1:Q + 1] == exp).all(), mis
        # what the call insists on is room for ONE longest query behind the fixed parts: a byte less is refused
        least = tc.align_candidates_workspace_bytes(Q, L, L, cap, c)
        assert least <= need
        out.fill_(SENTINEL)
        assert raw(dc._h, out[1:Q + 1], arena.data_ptr() + at, least - 1) == ERR_WORKSPACE
        assert b" 1 bytes missing (size it with tvz_align_candidates_workspace_bytes)" in lib.tvz_last_error()
        assert (out.cpu().numpy() == SENTINEL).all()
    # with a handle: the same early refusals, the output left alone; the order ends workspace, then the gap codes
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    out = torch.full((Q, c + 1, 2), SENTINEL, dtype=torch.int32, device=DEV)
    for kw, want, word in ((dict(c_=0), ERR_UNSUPPORTED, b"C=0"), (dict(c_=65, cap_=100), ERR_UNSUPPORTED, b"C=65"),
                           (dict(cap_=15), ERR_UNSUPPORTED, b"cap=15 below C=16"), (dict(min_count=0), ERR_INVALID, b"min_count 0"),
                           (dict(L_=4096), ERR_UNSUPPORTED, b"max_query_len 4096")):
        assert raw(dc._h, out, ws.data_ptr(), ws.numel(), **kw) == want and word in lib.tvz_last_error(), kw
    plain = tc.DeviceCorpus(0)
    try:
        plain.upload(rows[:5])
        assert raw(plain._h, out, ws.data_ptr(), 100) == ERR_WORKSPACE                 # the workspace first ...
        assert raw(plain._h, out, ws.data_ptr(), ws.numel()) == ERR_UNSUPPORTED         # ... then the handle
        assert b"keeps no gap codes (tvz_corpus_gap_index)" in lib.tvz_last_error()
        with pytest.raises(RuntimeError, match="gap_eps must be 0"):
            plain.set_gap_index(-1.0)
        assert plain.gap_index_stats() == dict(gap_eps=0.0, rows=0, codes=0, indexed_rows=0, delta_rows=0, builds=0)
    finally:
        plain.close()
    assert (out.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------------------------- 3. state of the index
def test_the_index_follows_upload_upsert_clear_and_its_switch(scratch):
    dc = scratch
    rows, uploads = cs.table(), cs.uploads()
    queries = [uploads[n] for n in ("shifted", "excerpt", "twin", "special", "stranger", "row4")]
    # turned on after the upload, and before it: the same answers
    dc.set_gap_index(0.0)
    dc.upload(rows)
    dc.set_gap_index(EPS)
    after = _check(dc, rows, queries, 16, "on after the upload", min_count=1)
    st = dc.gap_index_stats()
    codes = sum(len(ref.stored_codes(k, EPS)) for _, k in rows)
    assert st["gap_eps"] == EPS and st["rows"] == len(rows) and st["codes"] == codes and st["indexed_rows"] == len(rows)
    dc.upload(rows)
    before = _check(dc, rows, queries, 16, "on before the upload", min_count=1)
    assert (after == before).all() and dc.gap_index_stats()["codes"] == codes
    # an upsert that replaces a row: the old codes are gone, the new ones are found by the next call
    stranger = uploads["stranger"]
    dc.upsert(cs.FILM, (np.asarray(stranger) + 55.0).tolist())
    rows2 = [(v, (np.asarray(stranger) + 55.0).tolist() if v == cs.FILM else k) for v, k in rows]
    exp = _check(dc, rows2, queries, 16, "after the replacing upsert", min_count=1)
    assert exp[0, 16, 1] == 0 and exp[4, 0, 0] == cs.FILM and exp[4, 0, 1] >= len(stranger) - 3
    assert dc.gap_index_stats()["delta_rows"] == 1
    # ... and a new id
    dc.upsert(31337, (np.asarray(cs.film()) + 0.5).tolist())
    rows2.append((31337, (np.asarray(cs.film()) + 0.5).tolist()))
    assert _check(dc, rows2, queries, 16, "after a new id", min_count=1)[0, 0].tolist() == [31337, 117]
    # another width rebuilds: other codes, the reference's at that width
    dc.set_gap_index(cs.GAP_EPS_2)
    assert dc.gap_index_stats()["gap_eps"] == cs.GAP_EPS_2
    _check(dc, rows2, queries, 16, "another gap_eps", gap_eps=cs.GAP_EPS_2, min_count=1)
    dc.set_gap_index(EPS)
    # clear: nothing is found, the switch stays on; rows upserted afterwards are
    dc.clear()
    assert dc.gap_index_stats()["rows"] == 0 and dc.gap_index_stats()["gap_eps"] == EPS
    assert (_block(dc, queries, 4, min_count=1)[:, 4, 1] == 0).all()
    dc.upsert(5, cs.film())
    assert _check(dc, [(5, cs.film())], queries, 4, "after clear", min_count=1)[0, 0].tolist() == [5, 117]
    # off: refused, in the library's words
    dc.set_gap_index(0.0)
    assert dc.gap_index_stats() == dict(gap_eps=0.0, rows=0, codes=0, indexed_rows=0, delta_rows=0, builds=0)
    with pytest.raises(RuntimeError, match="keeps no gap codes"):
        dc.align_candidates(queries, c=4)


def test_the_code_tables_background_rebuild_keeps_the_answers(scratch):
    """Enough upserts on a small uploaded table that the code table's delta fills and its index is rebuilt in the
    background (gap_index_stats builds); the answers still equal the reference."""
    dc = scratch
    rng = np.random.default_rng(3)
    rows = cs.table()[:20]
    dc.upload(rows)
    dc.set_gap_index(EPS)
    builds = dc.gap_index_stats()["builds"]
    film = np.asarray(cs.film())
    rows = list(rows)
    for i in range(600):
        keys = (rng.uniform(0, 5000) + np.cumsum(rng.uniform(0.7, 30.0, size=6))).tolist() if i % 100 else \
            (film[i // 100: i // 100 + 30] + 10.0 * i).tolist()
        dc.upsert(40000 + i, keys)
        rows.append((40000 + i, keys))
    st = dc.gap_index_stats()
    assert st["builds"] > builds and st["rows"] == len(rows) and st["indexed_rows"] > 20
    up = cs.uploads()
    exp = _check(dc, rows, [up["shifted"], up["excerpt"], up["stranger"]], 16, "after the rebuild", min_count=2)
    assert exp[0, 16, 1] >= 6 and (exp[0, :16, 0] == 40000).any()                    # six excerpts of the film upserted


# ------------------------------------------------------------------------ 4. calls into the alignment layer
def test_the_block_goes_to_align_parts_by_strides_and_part_0_is_the_span_searchs_hit(world):
    rows, uploads, dc = world
    eps = 1 / 30
    names = ("shifted", "inserted", "removed", "excerpt", "twin")
    queries = [uploads[n] for n in names]
    c = 16
    d_q, d_off, L = tc.pack_queries(queries, DEV)
    block = dc.align_candidates_block(d_q, d_off, L, c=c, min_count=1)
    assert block.shape == (len(queries), c + 1, 2)
    ids = block[:, :c, 0]                                                          # a view: strides (C + 1) * 2 and 2
    assert ids.stride() == ((c + 1) * 2, 2)
    parts = dc.align_parts_block(d_q, d_off, L, ids, eps=eps, min_votes=1, max_parts=1).cpu().numpy()
    span = dc.align_span_topk_block(d_q, d_off, L, eps=eps, k=64, min_votes=1, local=True).cpu().numpy()
    h = block.cpu().numpy()
    once = {v for v, _ in rows if sum(1 for w, _ in rows if w == v) == 1}
    seen = 0
    for q in range(len(queries)):
        hits = {int(r[0]): r.tolist() for r in span[q, :64] if r[0] >= 0}
        for j in range(c):
            vid = int(h[q, j, 0])
            assert int(parts[q, j, 0, 0]) == vid
            if vid in once and vid in hits:
                _, row_len, best_bin, votes, rate, t_first, t_last, nr = hits[vid]
                assert parts[q, j, 0].tolist()[:3] == [vid, row_len, rate]
                assert parts[q, j, 1].tolist() == [best_bin, votes, t_first, t_last, t_last - t_first + 1, nr], (q, j)
                seen += 1
    assert seen >= 4 and int(h[0, 0, 0]) == cs.FILM


def test_inspector_with_candidates_reports_what_the_sweep_reports(world):
    from tvidz_amd import inspector as insp
    rows, uploads, dc = world

    class Store:
        corpus = dc

        def get_video_by_id(self, vid):
            return None

    try:
        for kw in (dict(near_score="local", near_min_votes=8, near_jaccard=0.9),
                   dict(near_score="local", near_min_votes=8, near_jaccard=0.9, near_parts=2),
                   dict(near_score="containment", near_min_votes=8, near_jaccard=0.4, near_spans=True),
                   dict(near_score="jaccard", near_jaccard=0.3)):
            kw = dict(dict(device=DEV, near_duplicates=True, near_top_k=8, near_any_offset=True), **kw)
            for name in ("inserted", "shifted", "removed", "excerpt", "stranger"):
                sweep = insp.Inspector(Store(), **kw)._near(424242, uploads[name])
                cand = insp.Inspector(Store(), near_candidates=16, near_gap_eps=EPS, **kw)._near(424242, uploads[name])
                assert cand == sweep, (kw, name)
                if name == "inserted" and kw.get("near_parts"):
                    (near,) = cand
                    assert near["video_id"] == cs.FILM and [p["votes"] for p in near["parts"]] == [60, 60] and "upload_span" in near
            # a refused upload (more than 514 cuts) takes the configured sweep
            long = cs.long_query(600, 4)
            assert insp.Inspector(Store(), near_candidates=16, near_gap_eps=EPS, **kw)._near(424242, long) == \
                insp.Inspector(Store(), **kw)._near(424242, long)
    finally:
        dc.set_gap_index(EPS)                                                      # (the module's handle: as the fixture left it)
