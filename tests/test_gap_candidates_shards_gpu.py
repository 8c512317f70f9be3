"""tvz_align_candidates_shards and service.ShardedCorpus.align_candidates on the GPU: at 1, 3, 8 and 20 shards the answer
equals one DeviceCorpus over the same rows, block for block - through upserts, a clear, the index turned on before and
after the upload, exclusions and the probe limit; the refusals that need handles; the exact-size workspace in a poisoned
arena; the merged block by strides into ShardedCorpus.align_parts; Inspector(near_candidates=C) over both corpora.  The
tables and uploads are tests/gap_candidates_cases.py's (small: every call takes milliseconds)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import gap_candidates_cases as cs, gap_candidates_merge_ref as mref
from tvidz_amd import _lib, corpus as tc, service

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = cs.GAP_EPS
SENTINEL = -0x5A5A5A5A
CANARY = 0xA5
INT32_MIN = -(1 << 31)
ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -4, -5
SHARD_COUNTS = (1, 3, 8, 20)


def _queries():
    up = cs.uploads()
    names = ("shifted", "excerpt", "twin", "special", "stranger", "row4", "inserted")
    return [up[n] for n in names] + [cs.counting_query()]


@pytest.fixture(scope="module")
def whole():
    """one handle over the whole table: the answer every sharding must give; the tests leave it as they found it"""
    dc = tc.DeviceCorpus(0)
    yield dc
    dc.close()


def _same(sc, dc, queries, c, what, **kw):
    want_rows, want_totals = dc.align_candidates(queries, c=c, **kw)
    rows, totals = sc.align_candidates(queries, c=c, **kw)
    assert rows.dtype == np.int32 and rows.shape == want_rows.shape and totals.shape == want_totals.shape
    assert (rows == want_rows).all() and (totals == want_totals).all(), (what, c, kw)
    assert (np.abs(want_totals.astype(np.int64)) <= kw.get("cap", 4096)).all() or (want_totals == INT32_MIN).any()
    return want_rows, want_totals


@pytest.mark.parametrize("R", SHARD_COUNTS)
def test_sharded_corpus_equals_one_handle_through_the_tables_life(whole, R):
    dc = whole
    rows = cs.table() + cs.counting_table(65)
    queries = _queries()
    sc = service.ShardedCorpus(0, n_shards=R)
    try:
        # the index turned on after the upload ...
        dc.set_gap_index(0.0)
        dc.upload(rows)
        dc.set_gap_index(EPS)
        sc.upload(rows)
        assert sc.gap_index_stats()["gap_eps"] == 0.0
        with pytest.raises(RuntimeError, match="keeps no gap codes"):
            sc.align_candidates(queries, c=4)
        sc.set_gap_index(EPS)
        st, one = sc.gap_index_stats(), dc.gap_index_stats()
        assert st["gap_eps"] == EPS and st["rows"] == one["rows"] == len(rows) and st["codes"] == one["codes"]
        for c in (1, 16, 64):
            r, t = _same(sc, dc, queries, c, "on after the upload", min_count=1)
        assert r[0, 0].tolist() == [cs.FILM, 117] and int(t[-1]) == 65
        # ... and before it
        sc.upload(rows)
        _same(sc, dc, queries, 16, "on before the upload", min_count=1)
        _same(sc, dc, queries, 16, "min_count 6", min_count=6)
        # exclusions
        excl = [cs.FILM, cs.FILM, cs.TWIN, -1, -1, cs.ROW4, cs.FILM, 5000]
        r, _ = _same(sc, dc, queries, 16, "exclusions", min_count=1, exclude_ids=excl)
        assert r[0, 0, 0] != cs.FILM and not (r[2, :, 0] == cs.TWIN).any()
        # the 514- and 515-value queries beside a good one
        mixed = [cs.long_query(515, 2), queries[0], cs.long_query(514, 1)]
        r, t = _same(sc, dc, mixed, 4, "the probe limit", min_count=1)
        assert int(t[0]) == INT32_MIN and (r[0] == (-1, 0)).all() and r[1, 0].tolist() == [cs.FILM, 117] and int(t[2]) >= 0
        # an upsert that replaces a row, and a new id
        moved = (np.asarray(cs.uploads()["stranger"]) + 55.0).tolist()
        for corpus in (dc, sc):
            corpus.upsert(cs.FILM, moved)
        r, t = _same(sc, dc, queries, 16, "after the replacing upsert", min_count=1)
        assert int(t[0]) == 0 and r[4, 0, 0] == cs.FILM
        for corpus in (dc, sc):
            corpus.upsert(31337, (np.asarray(cs.film()) + 0.5).tolist())
        assert _same(sc, dc, queries, 16, "after a new id", min_count=1)[0][0, 0].tolist() == [31337, 117]
        # a small cap: a negative total where a shard's list overflowed, never a positive one that differs
        _, t1 = dc.align_candidates(queries[-1:], c=4, min_count=1, cap=70)
        _, tR = sc.align_candidates(queries[-1:], c=4, min_count=1, cap=70)
        assert int(t1[0]) == 65 and abs(int(tR[0])) == 65
        # clear: nothing is found, the switch stays on; rows upserted afterwards are
        for corpus in (dc, sc):
            corpus.clear()
        assert sc.gap_index_stats()["rows"] == 0 and sc.gap_index_stats()["gap_eps"] == EPS
        assert (_same(sc, dc, queries, 4, "after clear", min_count=1)[1] == 0).all()
        for corpus in (dc, sc):
            corpus.upsert(5, cs.film())
        assert _same(sc, dc, queries, 4, "an upsert after clear", min_count=1)[0][0, 0].tolist() == [5, 117]
        no_rows, no_totals = sc.align_candidates([], c=4)
        assert no_rows.shape == (0, 4, 2) and no_totals.shape == (0,)
    finally:
        sc.close()


@pytest.fixture(scope="module")
def shards(whole):
    """-> (rows, dc, eight handles with the rows by video_id % 8): for the raw library calls; not changed by the tests"""
    rows = cs.table() + cs.counting_table(65)
    dc = tc.DeviceCorpus(0)
    dc.upload(rows)
    dc.set_gap_index(EPS)
    hs = []
    for s in range(8):
        h = tc.DeviceCorpus(0)
        h.upload([r for r in rows if r[0] % 8 == s])
        h.set_gap_index(EPS)
        hs.append(h)
    yield rows, dc, hs
    for h in hs + [dc]:
        h.close()


@pytest.mark.parametrize("R", (1, 3, 8))
def test_the_library_call_block_for_block(shards, R):
    """tvz_align_candidates_shards: every handle's block is what the handle answers alone, and the merged block is one
    handle's over the same rows (R of the eight handles, and one handle over exactly their rows)."""
    rows, _, hs = shards
    queries = _queries()
    d_q, d_off, L = tc.pack_queries(queries, DEV)
    part = tc.DeviceCorpus(0)
    try:
        part.upload([r for r in rows if r[0] % 8 < R])
        part.set_gap_index(EPS)
        # (the equality is claimed where no list overflows `cap`: 65 is the largest candidate count here)
        for c, kw in ((16, dict(min_count=1)), (1, dict(min_count=2)), (64, dict(min_count=1, cap=65))):
            blocks, merged = tc.align_candidates_shards(hs[:R], d_q, d_off, L, c=c, **kw)
            assert blocks.shape == (R, len(queries), c + 1, 2) and merged.shape == (len(queries), c + 1, 2)
            alone = torch.stack([h.align_candidates_block(d_q, d_off, L, c=c, **kw) for h in hs[:R]])
            assert (blocks == alone).all()
            want = part.align_candidates_block(d_q, d_off, L, c=c, **kw)
            assert (merged == want).all(), (R, c)
            assert (merged.cpu().numpy() == mref.merge(blocks.cpu().numpy())).all()
    finally:
        part.close()


def test_the_refusals_that_need_handles_and_the_exact_size_workspace(shards):
    rows, dc, hs = shards
    lib = _lib.load()
    queries = _queries()[:4]
    Q, c, cap = 4, 16, 40
    d_q, d_off, L = tc.pack_queries(queries, DEV)
    need = tc.align_candidates_workspace_bytes(Q, L, d_q.numel(), cap, c)           # ONE handle's serves all eight
    s = torch.cuda.current_stream(DEV)
    want = dc.align_candidates_block(d_q, d_off, L, c=c, min_count=1, cap=cap).cpu().numpy()
    blocks = torch.full((8, Q, c + 1, 2), SENTINEL, dtype=torch.int32, device=DEV)
    out = torch.full((Q + 2, c + 1, 2), SENTINEL, dtype=torch.int32, device=DEV)

    def raw(handles, ws_ptr, ws_bytes, c_=c, cap_=cap, bp=None, op=None):
        arr = (C.c_void_p * len(handles))(*[h._h if h is not None else None for h in handles])
        rc = lib.tvz_align_candidates_shards(arr, len(handles), d_q.data_ptr(), d_off.data_ptr(), Q, int(L), 1, None, cap_, c_,
                                             blocks.data_ptr() if bp is None else bp, out[1:Q + 1].data_ptr() if op is None else op,
                                             ws_ptr, ws_bytes, s.cuda_stream)
        s.synchronize()
        return rc, lib.tvz_last_error()

    for mis in (0, 8, 248):
        arena = torch.full((need + 1024,), CANARY, dtype=torch.uint8, device=DEV)
        at = (-arena.data_ptr()) % 256 + 256 + mis
        blocks.fill_(SENTINEL)
        out.fill_(SENTINEL)
        rc, msg = raw(hs, arena.data_ptr() + at, need)
        assert rc == 0, msg
        a = arena.cpu().numpy()
        assert (a[:at] == CANARY).all() and (a[at + need:] == CANARY).all(), mis
        o = out.cpu().numpy()
        assert (o[0] == SENTINEL).all() and (o[Q + 1] == SENTINEL).all() and (o[1:Q + 1] == want).all(), mis
    # refused, with nothing written: in front of every launch
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    blocks.fill_(SENTINEL)
    out.fill_(SENTINEL)
    other, plain = tc.DeviceCorpus(0), tc.DeviceCorpus(0)
    try:
        other.upload(rows[:5])
        other.set_gap_index(cs.GAP_EPS_2)
        plain.upload(rows[:5])
        rc, msg = raw(hs[:3] + [other], ws.data_ptr(), ws.numel())
        assert rc == ERR_UNSUPPORTED and b"shard 3 keeps gap codes of gap_eps=" in msg
        widths = [float(x) for x in re.findall(rb"(?:gap_eps=|shard 0 of )([0-9.e+-]+)", msg)]
        assert widths == [cs.GAP_EPS_2, EPS]                                         # both widths, to the last digit
        rc, msg = raw(hs[:2] + [plain] + hs[2:4], ws.data_ptr(), ws.numel())
        assert rc == ERR_UNSUPPORTED and b"keeps no gap codes (tvz_corpus_gap_index)" in msg
        rc, msg = raw(hs[:2] + [None], ws.data_ptr(), ws.numel())
        assert rc == ERR_INVALID and b"shard 2 is NULL" in msg
        # (what a handle's call insists on is room for ONE longest query behind the fixed parts: a byte less is refused)
        rc, msg = raw(hs, ws.data_ptr(), tc.align_candidates_workspace_bytes(Q, L, L, cap, c) - 1)
        assert rc == ERR_WORKSPACE and b" 1 bytes missing" in msg
        rc, msg = raw(hs, ws.data_ptr(), ws.numel(), c_=65, cap_=100)
        assert rc == ERR_UNSUPPORTED and b"C=65" in msg
        rc, msg = raw(hs, ws.data_ptr(), ws.numel(), op=blocks.data_ptr() + 8)
        assert rc == ERR_INVALID and b"d_out lies inside the blocks" in msg
        rc, msg = raw(hs, ws.data_ptr(), ws.numel(), bp=blocks.data_ptr() + 4)
        assert rc == ERR_INVALID
        assert (blocks.cpu().numpy() == SENTINEL).all() and (out.cpu().numpy() == SENTINEL).all()
        with pytest.raises(RuntimeError, match="lists outside 1..16"):
            tc.align_candidates_shards(hs + hs + [hs[0]], d_q, d_off, L, c=c)
    finally:
        other.close()
        plain.close()


def test_the_merged_block_goes_to_align_parts_by_strides_and_the_inspector_agrees(shards):
    from tvidz_amd import inspector as insp
    rows, dc, _ = shards
    up = cs.uploads()
    names = ("shifted", "inserted", "removed", "excerpt", "twin")
    queries = [up[n] for n in names]
    eps, c = 1 / 30, 16
    sc = service.ShardedCorpus(0, n_shards=3)
    try:
        sc.upload(rows)
        sc.set_gap_index(EPS)
        block = sc.align_candidates_block(queries, c=c, min_count=1)
        ids = block[:, :c, 0]                                                      # a view: strides (C + 1) * 2 and 2
        assert ids.stride() == ((c + 1) * 2, 2)
        parts = sc.align_parts(queries, ids, eps=eps, min_votes=1, max_parts=1)
        span, _ = sc.align_span_topk(queries, eps=eps, k=64, min_votes=1, local=True)
        h = block.cpu().numpy()
        once = {v for v, _ in rows if sum(1 for w, _ in rows if w == v) == 1}
        seen = 0
        for q in range(len(queries)):
            hits = {int(r[0]): r.tolist() for r in span[q] if r[0] >= 0}
            for j in range(c):
                vid = int(h[q, j, 0])
                assert int(parts[q, j, 0, 0]) == vid
                if vid in once and vid in hits:
                    _, row_len, best_bin, votes, rate, t_first, t_last, nr = hits[vid]
                    assert parts[q, j, 0].tolist()[:3] == [vid, row_len, rate]
                    assert parts[q, j, 1].tolist() == [best_bin, votes, t_first, t_last, t_last - t_first + 1, nr], (q, j)
                    seen += 1
        assert seen >= 4 and int(h[0, 0, 0]) == cs.FILM

        # Inspector(near_candidates=C) over the sharded corpus equals the same over one handle, entry for entry
        def store(corpus):
            return type("Store", (), {"corpus": corpus, "get_video_by_id": lambda self, vid: None})()

        for kw in (dict(near_score="local", near_min_votes=8, near_jaccard=0.9, near_parts=2),
                   dict(near_score="jaccard", near_jaccard=0.3)):
            kw = dict(dict(device=DEV, near_duplicates=True, near_top_k=8, near_any_offset=True, near_candidates=16,
                           near_gap_eps=EPS), **kw)
            one, many = insp.Inspector(store(dc), **kw), insp.Inspector(store(sc), **kw)
            for name in ("inserted", "shifted", "removed", "excerpt", "stranger"):
                want = one._near(424242, up[name])
                assert many._near(424242, up[name]) == want, (kw, name)
                if name == "shifted":
                    assert want and want[0]["video_id"] == cs.FILM
            long = cs.long_query(600, 4)                                           # refused: both take the configured sweep
            assert many._near(424242, long) == one._near(424242, long)
    finally:
        sc.close()
