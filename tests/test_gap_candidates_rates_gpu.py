"""GPU parity of tvz_align_candidates_rates (ts_gapc_offsets_kernel, ts_gapc_probe_kernel, ONE lookup over the handle's
code table for the Q x n_rates probe lists, ts_gapr_fold_kernel) against tests/gap_candidates_rates_ref.py: whole
[Q, C + 1, 3] blocks, exact integers throughout.  The tables, the uploads and the rate lists are
tests/gap_candidates_rates_cases.py's; their premises are asserted without a device in
tests/test_gap_candidates_rates_cpu.py."""
import numpy as np
import pytest
import torch

from tests import gap_candidates_cases as cs, gap_candidates_rates_cases as rc, gap_candidates_rates_ref as rr
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = rc.GAP_EPS
SENTINEL = -0x5A5A5A5A
CANARY = 0xA5
INT32_MIN = -(1 << 31)
ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -4, -5           # include/tvz.h


@pytest.fixture(scope="module")
def world():
    """-> (rows, queries, matrices, dc): the table on the device with its gap codes and the reference's count matrices
    for every rate list, once; no test that takes it changes either"""
    rows, queries = rc.table(), rc.queries()
    matrices = {rates: rr.count_matrix(rows, queries, EPS, rates) for rates in rc.RATE_LISTS}
    dc = tc.DeviceCorpus(0)
    dc.upload(rows)
    dc.set_gap_index(EPS)
    yield rows, queries, matrices, dc
    dc.close()


@pytest.fixture(scope="module")
def scratch():
    """a handle the tests of the tables and of the index's state fill as they like"""
    dc = tc.DeviceCorpus(0)
    yield dc
    dc.close()


def _block(dc, queries, rates, c, **kw):
    ids, counts, rate_indexes, totals = dc.align_candidates_rates(queries, rates, c=c, **kw)
    Q = len(queries)
    assert ids.dtype == np.int32 and ids.shape == counts.shape == rate_indexes.shape == (Q, c) and totals.shape == (Q,)
    out = np.zeros((Q, c + 1, 3), dtype=np.int64)
    out[:, :c, 0], out[:, :c, 1], out[:, :c, 2], out[:, c, 0], out[:, c, 1] = ids, counts, rate_indexes, -1, totals
    return out


def _same(got, exp, what):
    exp = np.asarray(exp, dtype=np.int64)
    bad = np.argwhere((got != exp).any(axis=(1, 2)))
    assert bad.size == 0, (what, [(int(q), got[q].tolist(), exp[q].tolist()) for q in bad[:2, 0]])
    return exp


def _check(dc, rows, queries, rates, c, what=None, **kw):
    exp = rr.candidates_rates(rows, queries, EPS, rates, c, **kw)
    return _same(_block(dc, queries, rates, c, **kw), exp, (what, rates, c, kw))


# ------------------------------------------------------------------------- 1. the uploads at every rate list
@pytest.mark.parametrize("rates", rc.RATE_LISTS, ids=lambda r: f"{len(r)}rates")
def test_every_upload_at_every_rate_list(world, rates):
    """Copies at 24/25, 25/24 and 1.25, the plain copy, three rows of one id at three rates, a row hit at two rates with
    equal and with unequal counts; lengths 0, 3, 4, 514 and 515; n_rates 1, 2, 3 and 8 with a repeated rate; C 1 / 16 /
    64, min_count 1 / 2 / 6; exclusions that differ per query."""
    rows, queries, matrices, dc = world
    at = {n: i for i, n in enumerate(rc.NAMES)}
    for c, min_count in ((1, 1), (16, 2), (64, 6), (16, 1)):
        exp = rr.blocks(rows, matrices[rates], c, min_count=min_count)
        _same(_block(dc, queries, rates, c, min_count=min_count), exp, (rates, c, min_count))
        assert exp[at["q515"], c, 1] == INT32_MIN and exp[at["empty"], c, 1] == 0
        if rc.SLOW in rates:
            assert exp[at["slow"], 0].tolist() == [rc.FILM, 117, rates.index(rc.SLOW)]
    if len(rates) >= 3:
        assert exp[at["triple"], 0].tolist() == [rc.TRIPLE, 11, 2] and exp[at["triple"], 16, 1] >= 3
    excl = rc.exclusions()
    exp = rr.blocks(rows, matrices[rates], 16, min_count=1, exclude_ids=excl)
    _same(_block(dc, queries, rates, 16, min_count=1, exclude_ids=excl), exp, (rates, "exclusions"))
    assert exp[at["slow"], 0, 0] != rc.FILM and exp[at["triple"], 16, 1] == 0
    # longer than the call's max_query_len, though below the probe limit: refused at every rate
    short = [m if len(q) <= 200 else None for q, m in zip(queries, matrices[rates])]
    exp = rr.blocks(rows, short, 4, min_count=2)
    _same(_block(dc, queries, rates, 4, min_count=2, max_query_len=200), exp, (rates, "max_query_len"))
    assert exp[at["q514"], 4, 1] == INT32_MIN and exp[at["plain"], 0, 0] == (rc.FILM if 1.0 in rates else -1)


def test_no_query_and_the_most_probe_lists(world):
    """Q = 0; Q x n_rates = 65,535 with tiny queries and exclusions that alternate, so that a wrong expansion of the
    exclusions to the pseudo-queries shows; 65,536 is refused."""
    rows, queries, matrices, dc = world
    ids, counts, rate_indexes, totals = dc.align_candidates_rates([], rc.RATES3, c=4)
    assert ids.shape == counts.shape == rate_indexes.shape == (0, 4) and totals.shape == (0,)
    up = rc.uploads()
    kinds = [up["four"], up["three"], up["empty"]]
    Q = 21845
    batch = [kinds[0] if q % 7 else kinds[1 + (q // 7) % 2] for q in range(Q)]
    excl = [rc.FILM if q % 2 else rc.NTSC if q % 3 == 0 else -1 for q in range(Q)]
    memo = {}
    exp = np.zeros((Q, 3, 3), dtype=np.int64)
    for q in range(Q):
        key = (len(batch[q]), excl[q])
        if key not in memo:
            memo[key] = rr.candidates_rates(rows, [batch[q]], EPS, rc.RATES3, 2, min_count=1, cap=4, exclude_ids=[excl[q]],
                                            max_query_len=4)[0]
        exp[q] = memo[key]
    assert len(memo) >= 6 and len({tuple(v.ravel().tolist()) for v in memo.values()}) >= 4
    got = _block(dc, batch, rc.RATES3, 2, min_count=1, cap=4, exclude_ids=excl, max_query_len=4)
    _same(got, exp, "65,535 probe lists")
    with pytest.raises(RuntimeError, match="Q=8192 x n_rates=8 is above 65535 probe lists"):
        dc.align_candidates_rates([kinds[0]] * 8192, rc.RATES8, c=2, cap=4)


# ---------------------------------------------------------------------------------- 2. the fold and the capacity
def test_the_fold_over_more_than_one_chunk_and_the_capacity(scratch):
    """8 lists of 225 to 300 hits, 2,325 entries in all: the fold crosses its 2,048-entry chunk; 97 ids over 300 rows, so
    an id has up to 32 entries, its best at the rate its row was made at; ties on the count throughout.  Then the
    capacity: equal to the longest list, and overflowed by one rate's list only."""
    dc = scratch
    q = [cs.counting_query()]
    table = rc.fold_table()
    dc.upload(table)
    dc.set_gap_index(EPS)
    m = rr.count_matrix(table, q, EPS, rc.FOLD_RATES)
    for c in (1, 16, 64):
        for min_count in (1, 2, 6):
            _same(_block(dc, q, rc.FOLD_RATES, c, min_count=min_count, cap=512), rr.blocks(table, m, c, min_count=min_count, cap=512),
                  ("fold", c, min_count))
    exp = _same(_block(dc, q, rc.FOLD_RATES, 64, min_count=1, cap=300), rr.blocks(table, m, 64, min_count=1, cap=300), "cap = hits")
    assert exp[0, 64, 1] > 2048 and len(set(exp[0, :64, 2].tolist())) >= 3
    # two queries side by side, the second's lists all empty: the first's fold is not disturbed
    two = q + [rc.uploads()["quarter"]]
    _same(_block(dc, two, rc.FOLD_RATES, 64, min_count=1, cap=512),
          rr.candidates_rates(table, two, EPS, rc.FOLD_RATES, 64, min_count=1, cap=512), "fold beside an empty query")
    # one list over the capacity: the total is negated, the other list is intact - its three rows lead
    table = rc.overflow_table()
    dc.upload(table)
    rates = (1.0, rc.QUARTER)
    m = rr.count_matrix(table, q, EPS, rates)
    n0, n1 = int((m[0][0] >= 1).sum()), int((m[0][1] >= 1).sum())
    exp = _same(_block(dc, q, rates, 3, min_count=1, cap=20), rr.blocks(table, m, 3, min_count=1, cap=20), "one list overflowed")
    assert n1 <= 20 < n0 and exp[0].tolist() == [[7000, 9, 1], [7001, 9, 1], [7002, 9, 1], [-1, -(n0 + n1), 0]]
    exp = _same(_block(dc, q, rates, 16, min_count=1, cap=n0), rr.blocks(table, m, 16, min_count=1, cap=n0), "cap = the longer list")
    assert exp[0, 16, 1] == n0 + n1


def test_the_exact_size_workspace_at_three_misalignments_and_the_refusals(world):
    """The workspace is exactly tvz_align_candidates_rates_workspace_bytes at bases 0, 8 and 248 bytes past a 256-byte
    line, inside an arena of 0xA5 bytes that is otherwise unchanged; the output - rows of 12 bytes, 4-byte aligned and no
    more - stands between guard rows.  Then the refusals that need a handle, which write nothing."""
    rows, queries, matrices, dc = world
    lib = _lib.load()
    rates = rc.RATES3
    sel = [rc.NAMES.index(n) for n in ("slow", "triple", "special", "three", "plain")]
    qs = [queries[i] for i in sel]
    c, cap, Q = 16, 40, len(sel)
    exp = rr.blocks(rows, [matrices[rates][i] for i in sel], c, min_count=1, cap=cap)
    d_q, d_off, L = tc.pack_queries(qs, DEV)
    d_ex = torch.full((Q,), -1, dtype=torch.int32, device=DEV)
    need = tc.align_candidates_rates_workspace_bytes(Q, L, d_q.numel(), len(rates), cap, c)
    h_rates = (_lib.C.c_double * len(rates))(*rates)
    s = torch.cuda.current_stream(DEV)

    def raw(handle, out_ptr, ws_ptr, ws_bytes, c_=c, cap_=cap, min_count=1, L_=L, R=len(rates)):
        rc_ = lib.tvz_align_candidates_rates(handle, d_q.data_ptr(), d_off.data_ptr(), Q, int(L_), h_rates, R, min_count,
                                             d_ex.data_ptr(), cap_, c_, out_ptr, ws_ptr, ws_bytes, s.cuda_stream)
        s.synchronize()
        return rc_

    for mis in (0, 8, 248):
        arena = torch.full((need + 1024,), CANARY, dtype=torch.uint8, device=DEV)
        at = (-arena.data_ptr()) % 256 + 256 + mis
        out = torch.full((Q + 2, c + 1, 3), SENTINEL, dtype=torch.int32, device=DEV)
        assert out[1:].data_ptr() % 8 == 4                                         # (17 rows of 12 bytes: 4-byte aligned)
        assert raw(dc._h, out[1:Q + 1].data_ptr(), arena.data_ptr() + at, need) == 0, lib.tvz_last_error()
        a = arena.cpu().numpy()
        assert (a[:at] == CANARY).all() and (a[at + need:] == CANARY).all(), mis
        o = out.cpu().numpy()
        assert (o[0] == SENTINEL).all() and (o[Q + 1] == SENTINEL).all() and (o[1:Q + 1] == exp).all(), mis
        # what the call insists on is room for ONE longest query behind the fixed parts: a byte less is refused
        least = tc.align_candidates_rates_workspace_bytes(Q, L, L, len(rates), cap, c)
        assert least <= need
        out.fill_(SENTINEL)
        assert raw(dc._h, out[1:Q + 1].data_ptr(), arena.data_ptr() + at, least - 1) == ERR_WORKSPACE
        assert b" 1 bytes missing (size it with tvz_align_candidates_rates_workspace_bytes)" in lib.tvz_last_error()
        assert (out.cpu().numpy() == SENTINEL).all()
    # with a handle: the early refusals, then the workspace, d_out's alignment, and last the gap codes; nothing is written
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    out = torch.full((Q, c + 1, 3), SENTINEL, dtype=torch.int32, device=DEV)
    for kw, want, word in ((dict(c_=0), ERR_UNSUPPORTED, b"C=0"), (dict(cap_=15), ERR_UNSUPPORTED, b"cap=15 below C=16"),
                           (dict(min_count=0), ERR_INVALID, b"min_count 0"), (dict(L_=4096), ERR_UNSUPPORTED, b"max_query_len 4096"),
                           (dict(R=0), ERR_UNSUPPORTED, b"n_rates=0"), (dict(R=9), ERR_UNSUPPORTED, b"n_rates=9")):
        assert raw(dc._h, out.data_ptr(), ws.data_ptr(), ws.numel(), **kw) == want and word in lib.tvz_last_error(), kw
    assert raw(dc._h, out.data_ptr() + 2, ws.data_ptr(), ws.numel()) == ERR_INVALID
    assert b"d_out is NULL or not 4-byte aligned" in lib.tvz_last_error()
    assert raw(dc._h, None, ws.data_ptr(), ws.numel()) == ERR_INVALID
    plain = tc.DeviceCorpus(0)
    try:
        plain.upload(rows[:5])
        assert raw(plain._h, out.data_ptr(), ws.data_ptr(), 100) == ERR_WORKSPACE          # the workspace first ...
        assert raw(plain._h, out.data_ptr(), ws.data_ptr(), ws.numel()) == ERR_UNSUPPORTED  # ... then the handle
        assert b"keeps no gap codes (tvz_corpus_gap_index)" in lib.tvz_last_error()
    finally:
        plain.close()
    assert (out.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------------------------- 3. state of the index
def test_the_answers_follow_an_upsert_the_background_rebuild_and_the_switch(scratch):
    dc = scratch
    rows, up = rc.table(), rc.uploads()
    queries = [up[n] for n in ("slow", "fast", "plain", "triple", "special")]
    rates = rc.RATES3
    dc.set_gap_index(0.0)
    dc.upload(rows)
    dc.set_gap_index(EPS)
    _check(dc, rows, queries, rates, 16, "uploaded", min_count=1)
    # an upsert that replaces the film, and a new id that holds the film at the fast rate
    stranger = (np.asarray(cs.uploads()["stranger"]) + 55.0).tolist()
    dc.upsert(rc.FILM, stranger)
    faster = (np.asarray(cs.film()) * rc.FAST + 0.5).tolist()
    dc.upsert(31337, faster)
    rows2 = [(v, stranger if v == rc.FILM else k) for v, k in rows] + [(31337, faster)]
    assert cs.edge_distance(faster, EPS, True) > 1e-6
    exp = _check(dc, rows2, queries, rates, 16, "after the upserts", min_count=2)
    assert exp[2, 0].tolist() == [31337, 117, 2] and rc.FILM not in exp[0, :16, 0]     # the plain copy finds it at 25/24
    assert dc.gap_index_stats()["delta_rows"] == 2
    # enough upserts that the code table's delta fills and its index is rebuilt in the background
    rng = np.random.default_rng(3)
    builds = dc.gap_index_stats()["builds"]
    film = np.asarray(cs.film())
    for i in range(600):
        keys = (rng.uniform(0, 5000) + np.cumsum(rng.uniform(0.7, 30.0, size=6))).tolist() if i % 100 else \
            (film[i // 100: i // 100 + 30] * rc.SLOW + 10.0 * i).tolist()
        dc.upsert(40000 + i, keys)
        rows2.append((40000 + i, keys))
    st = dc.gap_index_stats()
    assert st["builds"] > builds and st["rows"] == len(rows2)
    assert min(cs.edge_distance(k, EPS, True) for _, k in rows2[-600:]) > 1e-6
    exp = _check(dc, rows2, queries, rates, 16, "after the rebuild", min_count=2)
    assert (exp[2, :16, 0] >= 40000).any() and exp[2, 16, 1] >= 7                       # six slow excerpts of the film
    # off: refused, in the library's words
    dc.set_gap_index(0.0)
    with pytest.raises(RuntimeError, match="keeps no gap codes"):
        dc.align_candidates_rates(queries, rates, c=4)


# ------------------------------------------------------------------------------------------ 4. equivalences
def test_one_rate_of_one_is_the_plain_call_bit_for_bit(scratch):
    dc = scratch
    rows = rc.distinct_table()
    dc.upload(rows)
    dc.set_gap_index(EPS)
    up = cs.uploads()
    queries = [up[n] for n in up] + [cs.counting_query(), cs.long_query(514, 1), cs.long_query(515, 2)]
    d_q, d_off, L = tc.pack_queries(queries, DEV)
    d_ex = torch.tensor([rc.FILM if i % 3 == 0 else -1 for i in range(len(queries))], dtype=torch.int32, device=DEV)
    seen = 0
    for c, min_count, cap, ex in ((16, 1, 4096, None), (1, 2, 4096, d_ex), (64, 6, 4096, None), (64, 1, 65, d_ex)):
        plain = dc.align_candidates_block(d_q, d_off, L, c=c, min_count=min_count, cap=cap, d_exclude_ids=ex).cpu().numpy()
        rated = dc.align_candidates_rates_block(d_q, d_off, L, (1.0,), c=c, min_count=min_count, cap=cap,
                                                d_exclude_ids=ex).cpu().numpy()
        assert rated.shape == (len(queries), c + 1, 3) and (rated[:, :, :2] == plain).all() and (rated[:, :, 2] == 0).all()
        seen += int((plain[:, :c, 0] >= 0).sum())
    assert seen > 100 and plain[-1, 64, 1] == INT32_MIN and plain[-3, 64, 1] == 65     # (65 hits at cap = 65: exact)


def test_the_block_goes_to_align_parts_by_strides_with_the_same_rates(world):
    """block[:, :C, 0] - strides (C + 1) * 3 and 3 - is what tvz_align_parts takes; with the same rate list, part 0 and
    the header's rate_index are tvz_align_span_topk's hit for the true row."""
    rows, queries, matrices, dc = world
    eps, rates, c = 1 / 30, rc.RATES8, 16
    names = ("slow", "fast", "quarter", "plain")
    qs = [queries[rc.NAMES.index(n)] for n in names]
    d_q, d_off, L = tc.pack_queries(qs, DEV)
    block = dc.align_candidates_rates_block(d_q, d_off, L, rates, c=c, min_count=2)
    assert block.shape == (len(qs), c + 1, 3)
    ids = block[:, :c, 0]
    assert ids.stride() == ((c + 1) * 3, 3)
    parts = dc.align_parts_block(d_q, d_off, L, ids, eps=eps, rates=rates, min_votes=1, max_parts=1).cpu().numpy()
    span = dc.align_span_topk_block(d_q, d_off, L, eps=eps, rates=rates, k=64, min_votes=1, local=True).cpu().numpy()
    h = block.cpu().numpy()
    once = {v for v, _ in rows if sum(1 for w, _ in rows if w == v) == 1}
    seen = 0
    for q, name in enumerate(names):
        hits = {int(r[0]): r.tolist() for r in span[q, :64] if r[0] >= 0}
        for j in range(c):
            vid = int(h[q, j, 0])
            assert int(parts[q, j, 0, 0]) == vid
            if vid in once and vid in hits:
                _, row_len, best_bin, votes, rate, t_first, t_last, nr = hits[vid]
                assert parts[q, j, 0].tolist()[:3] == [vid, row_len, rate], (name, j)
                assert parts[q, j, 1].tolist() == [best_bin, votes, t_first, t_last, t_last - t_first + 1, nr], (name, j)
                seen += 1
        # the true row: the film leads, and the alignment finds it whole at the rate the candidates named
        want = {"slow": 1, "fast": 2, "quarter": 5, "plain": 0}[name]
        assert h[q, 0].tolist() == [rc.FILM, 117, want] and parts[q, 0, 0].tolist()[:4] == [rc.FILM, 120, want, 1]
        assert int(parts[q, 0, 1, 1]) == 120 and hits[rc.FILM][4] == want
    assert seen >= 4


def test_inspector_with_candidate_rates_reports_what_the_rates_sweep_reports(world):
    from tvidz_amd import inspector as insp
    rows, queries, matrices, dc = world
    up = rc.uploads()

    class Store:
        corpus = dc

        def get_video_by_id(self, vid):
            return None

    found = 0
    try:
        for kw in (dict(near_score="local", near_min_votes=8, near_jaccard=0.9, near_rates=rc.RATES3),
                   dict(near_score="jaccard", near_jaccard=0.5, near_rates=(1.0, rc.QUARTER, rc.SLOW, rc.FAST))):
            kw = dict(dict(device=DEV, near_duplicates=True, near_top_k=8, near_any_offset=True), **kw)
            for name in ("slow", "fast", "plain", "quarter", "special"):
                sweep = insp.Inspector(Store(), **kw)._near(424242, up[name])
                cand = insp.Inspector(Store(), near_candidates=16, near_candidate_rates=True, near_gap_eps=EPS,
                                      **kw)._near(424242, up[name])
                assert cand == sweep, (kw, name)
                if sweep:
                    found += 1
                    assert sweep[0]["video_id"] == (cs.SPECIAL_ROW if name == "special" else rc.FILM)
                    assert sweep[0]["rate"] == {"slow": rc.SLOW, "fast": rc.FAST, "quarter": rc.QUARTER}.get(name, 1.0)
            # a refused upload (more than 514 cuts) takes the configured rates sweep
            long = cs.long_query(600, 4)
            assert insp.Inspector(Store(), near_candidates=16, near_candidate_rates=True, near_gap_eps=EPS, **kw)._near(424242, long) \
                == insp.Inspector(Store(), **kw)._near(424242, long)
        assert found >= 7                                                          # (the 1.25 copy: the second list only)
    finally:
        dc.set_gap_index(EPS)                                                      # (the module's handle: as the fixture left it)
