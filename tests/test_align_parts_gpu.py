"""GPU parity of tvz_align_parts (ts_alignp_locate_kernel, ts_alignp_walk_kernel, ts_alignp_pick_kernel) against
tests/align_parts_ref.py: whole [Q, k, 1 + max_parts, 6] outputs, exact integers throughout.  The table and the uploads
are tests/align_parts_cases.py's; their premises are asserted without a device in tests/test_align_parts_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import align_parts_cases as cs, align_parts_ref as apr
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = cs.EPS
MAX_B = 1 << 22
BS = (900, 5000, MAX_B)                      # one window, a few, thousands
SENTINEL = -0x5A5A5A5A
CANARY = 0xA5
INT32_MIN = -(1 << 31)
ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -4, -5           # include/tvz.h
FILM_UPLOADS = ("inserted", "removed", "two_inserted", "swapped", "exact", "unrelated", "fps_inserted", "special")


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


def _check(dc, rows, queries, ids, B, rates=(1.0,), min_votes=1, max_parts=4, max_query_len=None):
    exp = apr.align_parts_ref(rows, queries, ids, EPS, B * EPS, rates, min_votes, max_parts, max_query_len)
    got = dc.align_parts(queries, ids, eps=EPS, max_offset=B * EPS, rates=rates, min_votes=min_votes, max_parts=max_parts,
                         max_query_len=max_query_len)
    assert got.dtype == np.int32
    _same(got, exp, (B, rates, min_votes, max_parts))
    return exp


# ------------------------------------------------------------------------------------------ 1. the film's uploads
@pytest.mark.parametrize("B", BS)
def test_the_films_uploads_under_every_bound_part_count_and_bar(world, B):
    rows, uploads, dc = world
    queries = [uploads[n] for n in FILM_UPLOADS]
    ids = [[cs.FILM, cs.SPECIAL]] * len(queries)
    for rates in ((1.0,), (1.0, 0.96), (0.96, 1.0)):
        for max_parts in (1, 2, 3, 4):
            for min_votes in (1, 8, 61):
                exp = _check(dc, rows, queries, ids, B, rates, min_votes, max_parts)
                if B >= 1419 and rates == (1.0,) and max_parts >= 2 and min_votes <= 8:
                    # the two halves tie at 60 votes: part 0 is the smaller |bin|
                    assert exp[0, 0, 0].tolist() == [cs.FILM, 120, 0, 2, 1, 129]
                    assert exp[0, 0, 1:3].tolist() == [[0, 60, 0, 59, 60, 60], [-1419, 60, 69, 128, 60, 60]]


# --------------------------------------------------------------------------------------------- 2. the other rows
@pytest.mark.parametrize("B", BS)
def test_every_upload_against_every_named_row(world, B):
    """The rows of 65, 513 and 700 keys, the later part's tie, two rows of one id (the second better; equal), nine rows
    of one id (refused, n_rows = 9), an absent id and -1 - for every upload, so most pairs are chance alignments."""
    rows, uploads, dc = world
    queries = list(uploads.values())
    ids = [list(cs.IDS)] * len(queries)
    exp = _check(dc, rows, queries, ids, B, (1.0, 0.96))
    q = list(uploads).index("parts24")
    nine, absent, none = cs.IDS.index(cs.NINE_ROWS), cs.IDS.index(cs.ABSENT), cs.IDS.index(-1)
    assert exp[q, nine, 0].tolist() == [cs.NINE_ROWS, 0, 0, INT32_MIN, 9, 24]
    assert exp[q, absent, 0].tolist() == [cs.ABSENT, 0, 0, 0, 0, 24] and exp[q, none, 0].tolist() == [-1, 0, 0, 0, 0, 24]
    assert exp[q, cs.IDS.index(cs.SECOND_BETTER), :2].tolist() == [[cs.SECOND_BETTER, 10, 0, 1, 2, 24], [30, 10, 2, 11, 10, 10]]
    assert exp[q, cs.IDS.index(cs.EQUAL_ROWS), :2].tolist() == [[cs.EQUAL_ROWS, 12, 0, 4 if B == MAX_B else 1, 2, 24], [-7, 8, 4, 11, 8, 8]]


def test_no_query_and_a_query_too_long_beside_a_good_one(world):
    rows, uploads, dc = world
    got = dc.align_parts([], [], eps=EPS, min_votes=1, max_parts=2)
    assert got.shape[0] == 0
    long = np.linspace(0.0, 4000.0, 4096).tolist()
    queries, ids = [long, uploads["inserted"], uploads["exact"]], [[cs.FILM, -1, cs.ABSENT]] * 3
    exp = _check(dc, rows, queries, ids, MAX_B, max_query_len=200)
    assert exp[0, :, 0].tolist() == [[cs.FILM, 0, 0, INT32_MIN, 1, 0], [-1, 0, 0, 0, 0, 0], [cs.ABSENT, 0, 0, INT32_MIN, 0, 0]]
    assert exp[1, 0, 0, 3] == 2 and exp[2, 0, 0, 3] == 1
    # ... and a query longer than max_query_len, though below 4,095
    exp = _check(dc, rows, queries[1:], ids[1:], MAX_B, max_query_len=125)
    assert exp[0, 0, 0].tolist() == [cs.FILM, 0, 0, INT32_MIN, 1, 0] and exp[1, 0, 0, 3] == 1


# ------------------------------------------------------------------------------ 3. cross-check with the search
def test_part_0_is_the_span_searchs_hit_and_a_span_block_is_taken_by_strides():
    from tests.test_align_span_gpu import _world_rows_and_queries
    rows, queries = _world_rows_and_queries()
    assert len(rows) >= 47                                                        # the 47-row table and the span cases' rows behind it
    once = {v for v, _ in rows if sum(1 for w, _ in rows if w == v) == 1}
    dc = tc.DeviceCorpus(0)
    try:
        dc.upload(rows)
        k, rates = 16, (1.0, 0.96)
        d_q, d_off, L = tc.pack_queries(queries, DEV)
        block = dc.align_span_topk_block(d_q, d_off, L, eps=EPS, rates=rates, k=k, min_votes=1)
        assert block.shape == (len(queries), k + 1, 8)
        ids = block[:, :k, 0]                                                    # a view: strides (k + 1) * 8 and 8
        assert ids.stride() == ((k + 1) * 8, 8)
        parts = dc.align_parts_block(d_q, d_off, L, ids, eps=EPS, rates=rates, min_votes=1, max_parts=4).cpu().numpy()
        hits = block.cpu().numpy()
        _same(parts, apr.align_parts_ref(rows, queries, hits[:, :k, 0], EPS, MAX_B * EPS, rates, 1, 4), "span block")
        seen = 0
        for q in range(len(queries)):
            for j in range(k):
                vid, row_len, best_bin, votes, rate, t_first, t_last, nr = hits[q, j].tolist()
                if vid < 0:
                    assert parts[q, j, 0].tolist()[:5] == [-1, 0, 0, 0, 0]
                elif vid in once:
                    seen += 1
                    assert parts[q, j, 0].tolist()[:3] == [vid, row_len, rate] and parts[q, j, 0, 3] >= 1
                    assert parts[q, j, 1].tolist() == [best_bin, votes, t_first, t_last, t_last - t_first + 1, nr], (q, j)
        assert seen > 100
    finally:
        dc.close()


# ----------------------------------------------------------------------------- 4. the C ABI: refusals, workspace
def _raw(dc, queries, ids, k, eps=EPS, mo=30.0, rates=(1.0,), min_votes=1, max_parts=2, L=None, out=None, ws_ptr=None,
         ws_bytes=None, null_ids=False):
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    L = min(longest, 4095) if L is None else L
    Q = len(queries)
    d_ids = torch.as_tensor(np.asarray(ids, dtype=np.int32).reshape(Q, -1)).to(DEV)
    if out is None:
        out = torch.full((Q, max(k, 1), 1 + 4, 6), SENTINEL, dtype=torch.int32, device=DEV)
    need = tc.align_parts_workspace_bytes(Q, min(max(L, 0), 4095), d_q.numel(), min(max(k, 1), 64), min(max(max_parts, 1), 4))
    ws = None
    if ws_ptr is None:
        ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
        ws_ptr = ws.data_ptr()
    h = None if rates is None else (C.c_double * max(len(rates), 1))(*rates)
    s = torch.cuda.current_stream(DEV)
    rc = _lib.load().tvz_align_parts(dc._h, d_q.data_ptr(), d_off.data_ptr(), Q, int(L), None if null_ids else d_ids.data_ptr(),
                                     1, d_ids.shape[1], int(k), float(eps), float(mo), h, 0 if rates is None else len(rates),
                                     int(min_votes), int(max_parts), out.data_ptr(), ws_ptr, need if ws_bytes is None else ws_bytes,
                                     s.cuda_stream)
    s.synchronize()
    return rc, out, need


def test_refusals_leave_the_output_alone(world):
    rows, uploads, dc = world
    q, ids = [uploads["inserted"]], [[cs.FILM, cs.ABSENT]]
    err = lambda: _lib.load().tvz_last_error()                                  # noqa: E731
    for kw, want, word in ((dict(max_parts=0), ERR_UNSUPPORTED, b"max_parts=0"), (dict(max_parts=5), ERR_UNSUPPORTED, b"max_parts=5"),
                           (dict(min_votes=0), ERR_INVALID, b"min_votes 0"), (dict(k=65), ERR_UNSUPPORTED, b"k=65"),
                           (dict(k=0), ERR_UNSUPPORTED, b"k=0"), (dict(L=4096), ERR_UNSUPPORTED, b"max_query_len 4096"),
                           (dict(rates=(1.0, -1.0)), ERR_INVALID, b"rate 1"), (dict(rates=None), ERR_UNSUPPORTED, b"n_rates=0"),
                           (dict(eps=0.0), ERR_INVALID, b"eps must be > 0"), (dict(mo=(MAX_B + 1) * EPS), ERR_UNSUPPORTED, b"TVZ_ALIGN_WIDE_MAX_B"),
                           (dict(null_ids=True), ERR_INVALID, b"NULL argument"), (dict(ws_bytes=1000), ERR_WORKSPACE, b"tvz_align_parts_workspace_bytes")):
        kw = dict(dict(k=2), **kw)
        rc, out, _ = _raw(dc, q, ids, **kw)
        assert rc == want and word in err(), (kw, rc, err())
        assert (out.cpu().numpy() == SENTINEL).all(), kw


def test_the_exact_size_workspace_at_three_misalignments(world):
    """The workspace is exactly tvz_align_parts_workspace_bytes at bases 0, 8 and 248 bytes past a 256-byte line, inside
    an arena of 0xA5 bytes that is otherwise unchanged; the output stands between guard rows."""
    rows, uploads, dc = world
    queries = [uploads["inserted"], uploads["parts24"], uploads["special"]]
    ids = [[cs.FILM, cs.LONG700, cs.NINE_ROWS, -1, cs.SPECIAL]] * 3
    exp = apr.align_parts_ref(rows, queries, ids, EPS, MAX_B * EPS, (1.0,), 1, 3)
    for mis in (0, 8, 248):
        _, _, need = _raw(dc, queries, ids, 5, mo=MAX_B * EPS, max_parts=3)
        arena = torch.full((need + 1024,), CANARY, dtype=torch.uint8, device=DEV)
        at = (-arena.data_ptr()) % 256 + 256 + mis
        out = torch.full((3 + 2, 5, 1 + 3, 6), SENTINEL, dtype=torch.int32, device=DEV)
        rc, _, _ = _raw(dc, queries, ids, 5, mo=MAX_B * EPS, max_parts=3, out=out[1:4], ws_ptr=arena.data_ptr() + at, ws_bytes=need)
        assert rc == 0, _lib.load().tvz_last_error()
        a = arena.cpu().numpy()
        assert (a[:at] == CANARY).all() and (a[at + need:] == CANARY).all(), mis
        o = out.cpu().numpy()
        assert (o[0] == SENTINEL).all() and (o[4] == SENTINEL).all()
        _same(o[1:4], exp, ("exact workspace", mis))
        # what the call insists on is room for ONE longest query behind the fixed parts: a byte less is refused
        least = tc.align_parts_workspace_bytes(3, len(queries[0]), len(queries[0]), 5, 3)
        assert least <= need
        rc, _, _ = _raw(dc, queries, ids, 5, mo=MAX_B * EPS, max_parts=3, ws_ptr=arena.data_ptr() + at, ws_bytes=least - 1)
        assert rc == ERR_WORKSPACE and b" 1 bytes missing" in _lib.load().tvz_last_error()


# ------------------------------------------------------------------------------------------------ 5. the shards
@pytest.mark.parametrize("R", (3, 20))
def test_sharded_corpus_keeps_the_best_shards_answer(world, R):
    from tvidz_amd import service
    rows, uploads, _ = world
    sc = service.ShardedCorpus(0, n_shards=R)
    try:
        # a video's rows in different shards: the two rows of one id are split, and so are the nine
        shard_rows = [[] for _ in range(R)]
        seen = {}
        for vid, keys in rows:
            n = seen[vid] = seen.get(vid, -1) + 1
            shard_rows[(vid + n) % R].append((vid, keys))
        for s, part in zip(sc.shards, shard_rows):
            s.upload(part)
        queries = [uploads["parts24"], uploads["inserted"], uploads["tie30"]]
        ids = [[cs.SECOND_BETTER, cs.EQUAL_ROWS, cs.NINE_ROWS, cs.FILM, cs.LATER_TIE, cs.ABSENT, -1]] * 3
        for B, max_parts, min_votes in ((MAX_B, 4, 1), (5000, 2, 8)):
            answers = [apr.align_parts_ref(part, queries, ids, EPS, B * EPS, (1.0,), min_votes, max_parts) for part in shard_rows]
            exp = apr.merge_shards_ref(answers)
            got = sc.align_parts(queries, ids, eps=EPS, max_offset=B * EPS, min_votes=min_votes, max_parts=max_parts)
            _same(got, exp, (R, B, max_parts, min_votes))
        # the better row and the summed count come from different shards; nine rows over several shards are no refusal
        assert exp[0, 0, 0].tolist()[:2] == [cs.SECOND_BETTER, 10] and exp[0, 0, 0, 4] == 2
        assert exp[0, 2, 0, 4] == 9 and exp[0, 2, 0, 3] >= 0
    finally:
        sc.close()


# --------------------------------------------------------------------------------------------- 6. the inspector
def test_inspector_reports_both_halves_of_the_upload_with_an_insertion(world):
    from tvidz_amd import inspector as insp
    rows, uploads, dc = world

    class Store:
        corpus = dc

        def get_video_by_id(self, vid):
            return None

    kw = dict(device=DEV, near_duplicates=True, near_top_k=8, near_any_offset=True, near_score="local", near_min_votes=8,
              near_jaccard=0.9)
    upload = uploads["inserted"]
    s = sorted(upload)
    (plain,) = insp.Inspector(Store(), **kw)._near(424242, upload)
    (near,) = insp.Inspector(Store(), near_parts=2, **kw)._near(424242, upload)
    # the local score alone: 1.0 over HALF of the upload
    assert plain["video_id"] == cs.FILM and plain["local"] == 1.0 and plain["upload_span"] == [s[0], s[59]]
    assert "parts" not in plain and {k: v for k, v in near.items() if k not in ("parts", "parts_score")} == plain
    assert near["parts_score"] == 1.0 and [p["votes"] for p in near["parts"]] == [60, 60]
    assert [p["shift_seconds"] for p in near["parts"]] == [0.0, -1419 * EPS]
    assert near["parts"][0]["upload_span"] == [s[0], s[59]] and near["parts"][1]["upload_span"] == [s[69], s[128]]
    assert near["parts"][1]["stored_span"] == [s[69] - 1419 * EPS, s[128] - 1419 * EPS]
    film = cs.film()
    assert abs(near["parts"][1]["stored_span"][0] - film[60]) < EPS and abs(near["parts"][1]["stored_span"][1] - film[119]) < EPS
