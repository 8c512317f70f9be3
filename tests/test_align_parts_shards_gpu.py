"""tvz_align_parts_shards on the GPU: the table of tests/align_parts_cases.py (and nine adjacent rows of one more id)
split into 3 and into 8 CONTIGUOUS handles - some of them empty, several ids with rows in two handles - answers as one
handle over the whole table does and as tests/align_parts_ref.py says, except where the documented difference shows: more
than eight rows of one id refuse a pair only where they lie in ONE handle.  Exact integers throughout."""
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
INT32_MIN = -(1 << 31)
SENTINEL = -0x5A5A5A5A
ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -4, -5           # include/tvz.h
NINE_TOGETHER = 10                                                  # nine rows of one id, adjacent: always in one handle
# contiguous row ranges: cs.NINE_ROWS' rows stand at 1, 6, .., 41 and split 5 + 4 at row 22; the last nine rows are
# NINE_TOGETHER's; cs.SECOND_BETTER's two rows stand at 45 and 46, cs.EQUAL_ROWS' at 4 and 47
SPLITS = {3: (0, 22, 46, 58), 8: (0, 0, 22, 22, 46, 46, 49, 49, 58)}
IDS = (cs.FILM, cs.SECOND_BETTER, cs.EQUAL_ROWS, cs.NINE_ROWS, NINE_TOGETHER, cs.LATER_TIE, cs.LONG700, cs.ABSENT, -1, cs.SPECIAL)
COMPARABLE = [j for j, v in enumerate(IDS) if v not in (cs.NINE_ROWS, NINE_TOGETHER)]      # at most 8 rows: one handle answers too


def _rows():
    rows = cs.table()
    assert len(rows) == 49 and [i for i, (v, _) in enumerate(rows) if v == cs.NINE_ROWS] == list(range(1, 42, 5))
    return rows + [(NINE_TOGETHER, (np.asarray(cs.x24()[i:i + 5]) + (3 * i + 0.1) * EPS).tolist()) for i in range(9)]


@pytest.fixture(scope="module")
def world():
    """-> (rows, queries, whole handle, {R: (row ranges, handles)}): uploaded once; no test changes them"""
    rows, uploads = _rows(), cs.uploads()
    queries = [uploads[n] for n in ("parts24", "inserted", "tie30", "special")]
    whole = tc.DeviceCorpus(0)
    whole.upload(rows)
    split = {}
    for R, b in SPLITS.items():
        parts = [rows[b[r]:b[r + 1]] for r in range(R)]
        assert sum(len(p) for p in parts) == len(rows) and (R == 3 or sum(1 for p in parts if not p) == 4)
        handles = [tc.DeviceCorpus(0) for _ in range(R)]
        for h, p in zip(handles, parts):
            h.upload(p)
        split[R] = (parts, handles)
    yield rows, queries, whole, split
    whole.close()
    for _, handles in split.values():
        for h in handles:
            h.close()


def _same(got, exp, what, pairs=None):
    got, exp = np.asarray(got, dtype=np.int64), np.asarray(exp, dtype=np.int64)
    if pairs is not None:
        got, exp = got[:, pairs], exp[:, pairs]
    bad = np.argwhere((got != exp).any(axis=(2, 3)))
    assert got.shape == exp.shape and bad.size == 0, (what, len(bad), [(q, j, got[q, j].tolist(), exp[q, j].tolist())
                                                                    for q, j in bad[:3].tolist()])


def _span_ids(Q, k):
    """the ids as the first column of a span block int32 [Q, k + 1, 8]: a view with strides (k + 1) * 8 and 8"""
    block = torch.full((Q, k + 1, 8), 12345, dtype=torch.int32, device=DEV)
    block[:, :k, 0] = torch.tensor(IDS, dtype=torch.int32, device=DEV)
    ids = block[:, :k, 0]
    assert ids.stride() == ((k + 1) * 8, 8)
    return ids


@pytest.mark.parametrize("R", (3, 8))
def test_contiguous_handles_answer_as_one_handle_and_as_the_reference(world, R):
    rows, queries, whole, split = world
    parts, handles = split[R]
    Q, k = len(queries), len(IDS)
    d_q, d_off, L = tc.pack_queries(queries, DEV)
    ids = _span_ids(Q, k)
    host_ids = [list(IDS)] * Q
    for B, rates, min_votes, P in ((MAX_B, (1.0,), 1, 4), (5000, (1.0, 0.96), 1, 2), (MAX_B, (1.0,), 8, 3)):
        kw = dict(eps=EPS, max_offset=B * EPS, rates=rates, min_votes=min_votes, max_parts=P)
        ws = torch.empty(tc.align_parts_workspace_bytes(Q, L, d_q.numel(), k, P), dtype=torch.uint8, device=DEV)
        blocks, got = tc.align_parts_shards(handles, d_q, d_off, L, ids, workspace=ws, **kw)
        torch.cuda.synchronize()
        blocks, got = blocks.cpu().numpy(), got.cpu().numpy()
        answers = [apr.align_parts_ref(p, queries, host_ids, EPS, B * EPS, rates, min_votes, P) for p in parts]
        for r in range(R):
            _same(blocks[r], answers[r], ("block", R, r, B))
        exp = apr.merge_shards_ref(answers)
        _same(got, exp, ("merged", R, B, rates, min_votes, P))
        assert (got == tc.align_parts_merge(blocks)).all()
        if min_votes == 1:
            # with every vote reported a contiguous split changes nothing: the earlier row wins a tie in one handle, the
            # lower handle here
            one = whole.align_parts_block(d_q, d_off, L, ids, **kw).cpu().numpy()
            _same(got, one, ("one handle", R, B), COMPARABLE)
            _same(got, apr.align_parts_ref(rows, queries, host_ids, EPS, B * EPS, rates, min_votes, P), ("reference", R, B), COMPARABLE)
            nine, together = IDS.index(cs.NINE_ROWS), IDS.index(NINE_TOGETHER)
            assert one[0, nine, 0].tolist() == [cs.NINE_ROWS, 0, 0, INT32_MIN, 9, 24]          # one handle refuses both
            assert got[0, nine, 0, 4] == 9 and got[0, nine, 0, 3] >= 1                         # 5 + 4: answered
            assert got[0, together, 0].tolist() == [NINE_TOGETHER, 0, 0, INT32_MIN, 9, 24]     # 9 in one handle: refused
            assert (got[0, together, 1:] == 0).all()
    # the rows of SECOND_BETTER and EQUAL_ROWS lie in two handles
    for vid in (cs.SECOND_BETTER, cs.EQUAL_ROWS):
        assert sum(1 for p in parts if any(v == vid for v, _ in p)) == 2


def _raw(handles, queries, k, P=2, n_shards=None, ws_bytes=None, null=()):
    d_q, d_off, L = tc.pack_queries(queries, DEV)
    Q, R = len(queries), len(handles)
    ids = torch.tensor([list(IDS[:k])] * Q, dtype=torch.int32, device=DEV)
    rows_of = 1 + min(max(P, 1), 4)
    blocks = torch.full((R, Q, k, rows_of, 6), SENTINEL, dtype=torch.int32, device=DEV)
    parts = torch.full((Q, k, rows_of, 6), SENTINEL, dtype=torch.int32, device=DEV)
    need = tc.align_parts_workspace_bytes(Q, L, d_q.numel(), k, rows_of - 1)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    arr = (C.c_void_p * R)(*[None if "handle" in null and r == 1 else h._h for r, h in enumerate(handles)])
    s = torch.cuda.current_stream(DEV)
    rates = (C.c_double * 1)(1.0)
    rc = _lib.load().tvz_align_parts_shards(
        arr, R if n_shards is None else n_shards, d_q.data_ptr(), d_off.data_ptr(), Q, L, None if "ids" in null else ids.data_ptr(),
        1, k, k, EPS, 30.0, rates, 1, 1, P, None if "blocks" in null else blocks.data_ptr(),
        None if "parts" in null else parts.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes, s.cuda_stream)
    msg = _lib.load().tvz_last_error()
    s.synchronize()
    return rc, msg, blocks.cpu().numpy(), parts.cpu().numpy(), (d_q, L)


def test_refusals_come_before_anything_is_written(world):
    rows, queries, whole, split = world
    _, handles = split[3]
    q = queries[:2]
    rc, msg, blocks, parts, (d_q, L) = _raw(handles, q, 3)
    assert rc == 0 and (blocks != SENTINEL).all() and (parts != SENTINEL).all()
    # a workspace one byte below the least the call takes - the fixed parts and ONE longest query - is refused by the name of
    # its sizing function, by the FIRST handle
    least = tc.align_parts_workspace_bytes(2, L, L, 3, 2)
    for kw, want, word in ((dict(ws_bytes=least - 1), ERR_WORKSPACE, b" 1 bytes missing (size it with tvz_align_parts_workspace_bytes)"),
                           (dict(n_shards=0), ERR_INVALID, b"no shards"), (dict(n_shards=17), ERR_UNSUPPORTED, b"17 lists outside 1..16"),
                           (dict(P=0), ERR_UNSUPPORTED, b"alignment parts: max_parts=0"), (dict(P=5), ERR_UNSUPPORTED, b"max_parts=5"),
                           (dict(null=("handle",)), ERR_INVALID, b"shard 1 is NULL"), (dict(null=("ids",)), ERR_INVALID, b"NULL argument"),
                           (dict(null=("blocks",)), ERR_INVALID, b"NULL argument"), (dict(null=("parts",)), ERR_INVALID, b"NULL argument")):
        rc, msg, blocks, parts, _ = _raw(handles, q, 3, **kw)
        assert rc == want and word in msg, (kw, rc, msg)
        assert (blocks == SENTINEL).all() and (parts == SENTINEL).all(), kw
    assert _raw(handles, q, 3, ws_bytes=least)[0] == 0


def test_sharded_corpus_of_20_shards_groups_and_merges_again(world):
    """service.ShardedCorpus.align_parts: one tvz_align_parts_shards per group of 16, the two answers merged by
    tvz_align_parts_merge; the rows dealt out row by row, so cs.NINE_ROWS' nine lie in nine shards of both groups."""
    from tvidz_amd import service
    rows, queries, whole, _ = world
    R = 20
    sc = service.ShardedCorpus(0, n_shards=R)
    try:
        shard_rows = [rows[r::R] for r in range(R - 1)] + [[]]
        shard_rows[0] = shard_rows[0] + rows[R - 1::R]                              # (the last shard stays empty)
        for s, part in zip(sc.shards, shard_rows):
            s.upload(part)
        ids = [list(IDS)] * len(queries)
        for B, P in ((MAX_B, 4), (900, 2)):
            answers = [apr.align_parts_ref(p, queries, ids, EPS, B * EPS, (1.0, 0.96), 1, P) for p in shard_rows]
            exp = apr.merge_shards_ref(answers)
            got = sc.align_parts(queries, ids, eps=EPS, max_offset=B * EPS, rates=(1.0, 0.96), min_votes=1, max_parts=P)
            assert got.dtype == np.int32
            _same(got, exp, (B, P))
            assert (got == tc.align_parts_merge(np.stack(answers).astype(np.int32))).all()
        nine = IDS.index(cs.NINE_ROWS)
        assert got[0, nine, 0, 4] == 9 and got[0, nine, 0, 3] >= 0
    finally:
        sc.close()
