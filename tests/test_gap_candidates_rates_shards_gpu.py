"""GPU parity of tvz_align_candidates_rates_shards and service.ShardedCorpus.align_candidates_rates against ONE
DeviceCorpus over the same rows: whole [Q, C + 1, 3] blocks, all three columns and the totals, exact integers.  The
tables, uploads and rate lists are tests/gap_candidates_rates_cases.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gap_candidates_cases as cs, gap_candidates_rates_cases as rc
from tvidz_amd import _lib, corpus as tc, service

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = rc.GAP_EPS
INT32_MIN = -(1 << 31)
ERR_UNSUPPORTED, ERR_WORKSPACE = -4, -5


def _block(corpus, queries, rates, c, **kw):
    ids, counts, rate_indexes, totals = corpus.align_candidates_rates(queries, rates, c=c, **kw)
    Q = len(queries)
    assert ids.dtype == np.int32 and ids.shape == counts.shape == rate_indexes.shape == (Q, c) and totals.shape == (Q,)
    out = np.zeros((Q, c + 1, 3), dtype=np.int64)
    out[:, :c, 0], out[:, :c, 1], out[:, :c, 2], out[:, c, 0], out[:, c, 1] = ids, counts, rate_indexes, -1, totals
    return out


def _same(got, exp, what):
    bad = np.argwhere((np.asarray(got) != np.asarray(exp)).any(axis=(1, 2)))
    assert bad.size == 0, (what, [(int(q), got[q].tolist(), exp[q].tolist()) for q in bad[:2, 0]])


@pytest.fixture(scope="module")
def one():
    """the main table in ONE DeviceCorpus: what every sharded answer must equal"""
    dc = tc.DeviceCorpus(0)
    dc.upload(rc.table())
    dc.set_gap_index(EPS)
    yield dc
    dc.close()


@pytest.mark.parametrize("R", (1, 3, 8, 20))
def test_sharded_corpus_equals_one_device_corpus_through_upserts_and_a_clear(one, R):
    """1, 3, 8 and 20 shards (20: two library calls, 16 + 4, merged again); rates 1, 3 and 8 with a repeated rate; C 1 /
    16 / 64; exclusions that differ per query; a refused query (515 values); the index turned on before the upload for
    even R and after it for odd R; then upserts (a new id, a second and third row of a stored id - they land in one
    shard) and a clear."""
    rows, queries, excl = rc.table(), rc.queries(), rc.exclusions()
    sc = service.ShardedCorpus(0, n_shards=R)
    dc = tc.DeviceCorpus(0)
    try:
        assert sc.supports_align_candidate_rates is True
        if R % 2 == 0:
            sc.set_gap_index(EPS)
        sc.upload(rows)
        if R % 2:
            sc.set_gap_index(EPS)
        for rates in (rc.RATE_LISTS[0], rc.RATES3, rc.RATES8):
            for c, min_count in ((1, 1), (16, 2), (64, 1)):
                exp = _block(one, queries, rates, c, min_count=min_count)
                _same(_block(sc, queries, rates, c, min_count=min_count), exp, (R, rates, c))
            exp = _block(one, queries, rates, 16, min_count=1, exclude_ids=excl)
            _same(_block(sc, queries, rates, 16, min_count=1, exclude_ids=excl), exp, (R, rates, "exclusions"))
        assert (exp[:, 16, 1] == INT32_MIN).any()                                   # the refused query is among them
        assert len(rc.RATES8) == 8 and len(set(rc.RATES8)) < 8                      # a repeated rate
        # upserts and a clear, on both sides
        dc.set_gap_index(EPS)
        dc.upload(rows)
        film = next(k for v, k in rows if v == rc.FILM)
        for corpus in (sc, dc):
            corpus.upsert(990001, [t * 0.96 + 3.0 for t in film])
            corpus.upsert(rc.TRIPLE, [t + 100.0 for t in film[:40]])
        _same(_block(sc, queries, rc.RATES3, 16, min_count=1), _block(dc, queries, rc.RATES3, 16, min_count=1), (R, "upserts"))
        for corpus in (sc, dc):
            corpus.clear()
            corpus.upsert(5, film)
        got = _block(sc, queries, rc.RATES3, 4, min_count=2)
        _same(got, _block(dc, queries, rc.RATES3, 4, min_count=2), (R, "clear"))
        assert (got[:, :4, 0] >= 0).sum() >= 1 and set(got[:, :4, 0].ravel().tolist()) <= {-1, 5}
    finally:
        sc.close()
        dc.close()


def test_c_abi_rows_of_one_id_in_two_handles_refusals_and_the_exact_workspace(one):
    """Handles uploaded directly, rows split by row index % 3: rows of one id lie in two and three handles, and the
    merged block still equals one DeviceCorpus's.  Then two gap_eps (both named), a handle without codes, the exact-size
    workspace and one byte less."""
    rows, queries = rc.fold_table(), [cs.counting_query()] + rc.queries()[:4]
    per_id = {}
    for i, (v, _) in enumerate(rows):
        per_id.setdefault(v, set()).add(i % 3)
    assert max(len(s) for s in per_id.values()) >= 2                               # the premise: an id in several handles
    whole = tc.DeviceCorpus(0)
    shards = [tc.DeviceCorpus(0) for _ in range(3)]
    try:
        whole.upload(rows)
        whole.set_gap_index(EPS)
        for s, dc in enumerate(shards):
            dc.upload(rows[s::3])
            dc.set_gap_index(EPS)
        d_q, d_off, L = tc.pack_queries(queries, DEV)
        for rates, c in ((rc.FOLD_RATES, 64), (rc.RATES3, 16), ((1.0,), 1)):
            exp = whole.align_candidates_rates_block(d_q, d_off, L, rates, c=c, min_count=1).cpu().numpy()
            blocks, merged = tc.align_candidates_rates_shards(shards, d_q, d_off, L, rates, c=c, min_count=1)
            _same(merged.cpu().numpy(), exp, (rates, c))
            assert (tc.align_candidates_rates_merge(blocks.cpu().numpy()) == exp).all()    # the numpy merge agrees
            assert (exp[:, c, 1] >= 0).all()                                        # no list overflowed cap: exact
        # the exact-size workspace, and one byte less
        lib, s = _lib.load(), torch.cuda.current_stream(DEV)
        Q, c = len(queries), 16
        need = tc.align_candidates_rates_workspace_bytes(Q, L, d_q.numel(), 3, 4096, c)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        blocks = torch.empty((3, Q, c + 1, 3), dtype=torch.int32, device=DEV)
        out = torch.full((Q, c + 1, 3), -7, dtype=torch.int32, device=DEV)
        handles = (C.c_void_p * 3)(*[dc._h for dc in shards])
        h_rates = (C.c_double * 3)(*rc.RATES3)

        def call(hs=handles, n=3, bytes_=need):
            rc_ = lib.tvz_align_candidates_rates_shards(hs, n, d_q.data_ptr(), d_off.data_ptr(), Q, L, h_rates, 3, 1, None, 4096,
                                                        c, blocks.data_ptr(), out.data_ptr(), ws.data_ptr(), bytes_, s.cuda_stream)
            s.synchronize()
            return rc_, lib.tvz_last_error()

        # (the call refuses a buffer that cannot hold its fixed parts and ONE longest query: the sizing at L keys)
        floor = tc.align_candidates_rates_workspace_bytes(Q, L, L, 3, 4096, c)
        assert floor <= need
        rc_, msg = call(bytes_=floor - 1)
        assert rc_ == ERR_WORKSPACE and b"1 bytes missing" in msg and b"tvz_align_candidates_rates_workspace_bytes" in msg
        assert (out.cpu().numpy() == -7).all()
        assert call()[0] == 0
        exp = whole.align_candidates_rates_block(d_q, d_off, L, rc.RATES3, c=c, min_count=1).cpu().numpy()
        _same(out.cpu().numpy(), exp, "exact workspace")
        # two widths, both named; a handle without codes: nothing written
        out.fill_(-7)
        shards[1].set_gap_index(EPS / 2)
        rc_, msg = call()
        assert rc_ == ERR_UNSUPPORTED and b"shard 1" in msg and ("%.17g" % EPS).encode() in msg \
            and ("%.17g" % (EPS / 2)).encode() in msg, msg
        shards[1].set_gap_index(0.0)
        rc_, msg = call()
        assert rc_ == ERR_UNSUPPORTED and b"keeps no gap codes" in msg
        assert (out.cpu().numpy() == -7).all()
    finally:
        whole.close()
        for dc in shards:
            dc.close()


def test_one_rate_of_one_on_distinct_ids_equals_the_plain_shards_block_and_feeds_the_parts_call(one):
    rows = rc.distinct_table()
    up = cs.uploads()
    queries = [up[n] for n in up] + [cs.counting_query(), cs.long_query(515, 2)]
    sc = service.ShardedCorpus(0, n_shards=3)
    try:
        sc.upload(rows)
        sc.set_gap_index(EPS)
        for c in (1, 16):
            plain = sc.align_candidates_block(queries, c=c, min_count=1).cpu().numpy()
            rated = sc.align_candidates_rates_block(queries, (1.0,), c=c, min_count=1).cpu().numpy()
            assert (rated[:, :, :2] == plain).all() and (rated[:, :, 2] == 0).all()
    finally:
        sc.close()
    # the merged block goes by strides into ShardedCorpus.align_parts with the same list: the ids the parts call gets
    # are the block's column 0, and its answers equal one DeviceCorpus's for the same ids and rates (the driver on top of
    # the two calls: the Inspector test below)
    rows, queries = rc.table(), rc.queries()[:6]
    sc = service.ShardedCorpus(0, n_shards=8)
    try:
        sc.upload(rows)
        sc.set_gap_index(EPS)
        block = sc.align_candidates_rates_block(queries, rc.RATES3, c=8, min_count=2)
        ids = block[:, :8, 0]
        assert ids.stride() == (27, 3)                                              # (C + 1) * 3 and 3: tvz_gap_rates.h's strides
        kw = dict(eps=1.0 / 30, rates=rc.RATES3, min_votes=2, max_parts=2)
        got = sc.align_parts(queries, ids, **kw)
        exp = one.align_parts(queries, ids.cpu().numpy(), **kw)
        assert got.shape == exp.shape and (got == exp).all()
    finally:
        sc.close()


@pytest.mark.parametrize("n_shards", (3, 20))
def test_inspector_with_the_switch_over_a_sharded_corpus_equals_the_same_over_a_device_corpus(one, n_shards):
    """The driver end to end: ShardedCorpus.align_candidates_rates -> align_parts with the same list -> the rate from the
    parts header, entry for entry what the same Inspector reports over one DeviceCorpus; a refused upload (more than 514
    cuts) takes the configured rates sweep on both."""
    from tvidz_amd import inspector as insp
    up = rc.uploads()
    base = dict(device=DEV, near_duplicates=True, near_top_k=8, near_any_offset=True, near_candidates=16, near_gap_eps=EPS,
                near_rates=rc.RATES3, near_candidate_rates=True)
    scenarios = {f"{name} {i}": (up[name], dict(base, **kw))
                 for name in ("slow", "fast", "plain", "triple")
                 for i, kw in enumerate((dict(near_score="local", near_min_votes=8, near_jaccard=0.9),
                                         dict(near_score="local", near_min_votes=8, near_jaccard=0.9, near_parts=2),
                                         dict(near_score="jaccard", near_jaccard=0.3)))}
    scenarios["refused upload"] = (cs.long_query(600, 4), dict(base, near_score="jaccard", near_jaccard=0.3))

    def run(corpus):
        class Store:
            def get_video_by_id(self, vid):
                return None
        Store.corpus = corpus
        return {name: insp.Inspector(Store(), **kw)._near(424242, upload) for name, (upload, kw) in scenarios.items()}

    sc = service.ShardedCorpus(0, n_shards=n_shards)
    try:
        sc.upload(rc.table())
        want, got = run(one), run(sc)
        assert got == want and len(want) == 13
        (near,) = want["slow 0"]
        assert near["video_id"] == rc.FILM and near["rate"] == rc.SLOW
        assert want["fast 2"][0]["video_id"] == rc.FILM and want["fast 2"][0]["rate"] == rc.FAST
        assert want["plain 1"][0]["rate"] == 1.0 and "parts" in want["plain 1"][0]
    finally:
        sc.close()
    one.set_gap_index(EPS)                                                          # (as the module's fixture made it)
