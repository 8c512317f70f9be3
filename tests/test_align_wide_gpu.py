"""GPU parity of tvz_align_wide_topk (ts_alignw_sweep_kernel + ts_alignw_reduce_kernel): whole [Q, k + 1, 4] blocks,
bit-exact - with tvz_align_topk's own blocks wherever the bounded call is defined, with tests/align_wide_ref.py
everywhere else: every seam of the window walk, the limits of the bin range, votes one or many windows apart, far
copies under both scores, long rows and special keys, refusals, and the inspector's near_any_offset."""

import numpy as np
import pytest
import torch

from tests import align_ref as ar
from tests import align_topk_ref as atr
from tests import align_wide_ref as awr
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -0x5A5A5A5A
CANARY = 0xA5
ERR_WORKSPACE = -5
KS = (1, 16, 64)
MAX_B = 1 << 22
E64 = 1 / 64                   # dyadic: every difference of multiples of 1/64 below is exact
Q0 = 100.0


@pytest.fixture(scope="module")
def dc():
    c = tc.DeviceCorpus(0)
    yield c
    c.close()


def _args(queries, k, max_query_len, exclude_ids):
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    L = min(longest, atr.MAX_LEN) if max_query_len is None else max_query_len
    d_ex = None if exclude_ids is None else torch.as_tensor(np.asarray(exclude_ids, dtype=np.int32)).to(DEV)
    return d_q, d_off, L, d_ex


def _raw(dc, queries, eps, mo, k, min_votes=1, min_score=0, flags=0, exclude_ids=None, max_query_len=None, out=None,
         ws=None, ws_bytes=None):
    """tvz_align_wide_topk through the C ABI -> (return code, the [Q, k + 1, 4] device block)."""
    d_q, d_off, L, d_ex = _args(queries, k, max_query_len, exclude_ids)
    Q = len(queries)
    if out is None:
        out = torch.full((Q, max(k, 0) + 1, 4), SENTINEL, dtype=torch.int32, device=DEV)
    need = tc.align_wide_topk_workspace_bytes(Q, min(max(L, 0), atr.MAX_LEN), d_q.numel(), min(max(k, 1), 64))
    if ws is None:
        ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream(DEV)
    rc = _lib.load().tvz_align_wide_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), Q, int(L), float(eps), float(mo),
                                         int(min_votes), int(min_score), int(flags),
                                         d_ex.data_ptr() if d_ex is not None else None, int(k), out.data_ptr(),
                                         ws.data_ptr(), need if ws_bytes is None else ws_bytes, s.cuda_stream)
    s.synchronize()
    return rc, out


def _raw_bounded(dc, queries, eps, mo, k, min_votes=1, min_score=0, exclude_ids=None, max_query_len=None):
    """tvz_align_topk, the same way."""
    d_q, d_off, L, d_ex = _args(queries, k, max_query_len, exclude_ids)
    Q = len(queries)
    out = torch.full((Q, k + 1, 4), SENTINEL, dtype=torch.int32, device=DEV)
    need = tc.align_topk_workspace_bytes(Q, L, d_q.numel(), k)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream(DEV)
    rc = _lib.load().tvz_align_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), Q, int(L), float(eps), float(mo),
                                    int(min_votes), int(min_score), d_ex.data_ptr() if d_ex is not None else None,
                                    int(k), out.data_ptr(), ws.data_ptr(), need, s.cuda_stream)
    s.synchronize()
    return rc, out


def _expect_blocks(got, exp, what):
    got = np.asarray(got, dtype=np.int64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere((got != exp).any(axis=2))
    assert bad.size == 0, (what, f"{len(bad)} rows differ", [(q, r, got[q, r].tolist(), exp[q, r].tolist())
                                                             for q, r in bad[:4].tolist()])


def _check(dc, rows, queries, eps, mo, k, aligned=None, contain=False, **kw):
    """The library against tests/align_wide_ref.py -> the expected blocks."""
    exp = awr.topk_wide_ref(rows, queries, eps, mo, k, aligned=aligned, contain=contain, **kw)
    rc, out = _raw(dc, queries, eps, mo, k, flags=1 if contain else 0, **kw)
    assert rc == 0, _lib.load().tvz_last_error()
    _expect_blocks(out.cpu().numpy(), exp, (eps, mo, k, contain, kw))
    return exp


# ---------------------------------------------------------------------------------------------- 1. old equals new
@pytest.mark.parametrize("case", ar.edge_cases(), ids=lambda c: c[0])
def test_equals_the_bounded_call_bit_for_bit(dc, case):
    """flags = 0 and B <= 2047: tvz_align_topk's block, whatever it is - k in (1, 16, 64) and the k-th hit's own score
    as the threshold (the k-th score is read from the bounded call's reference)."""
    name, rows, calls = case
    dc.upload(rows)
    batches = {}
    for q, eps, mo in calls:
        batches.setdefault((eps, mo), []).append(list(q))
    for (eps, mo), queries in batches.items():
        aligned = [ar.align_ref(rows, q, eps, mo) for q in queries]
        for k in KS:
            thresholds = [0]
            for a, q in zip(aligned, queries):
                hits = atr.hits_of(a, atr.n_valid(q))
                if hits:
                    thresholds.append(-hits[min(k, len(hits)) - 1][0][0])
            for s_k in sorted(set(thresholds))[-3:] + [0]:
                rc_o, old = _raw_bounded(dc, queries, eps, mo, k, min_score=s_k)
                rc_n, new = _raw(dc, queries, eps, mo, k, min_score=s_k)
                assert rc_o == rc_n == 0, _lib.load().tvz_last_error()
                assert torch.equal(old, new), (name, eps, mo, k, s_k, np.argwhere((old != new).cpu().numpy())[:4].tolist())
        assert (old[:, -1, 1] >= 0).all() and (name not in ("grid_stride", "boundary") or int(old[0, -1, 1]) > 64)


# ---------------------------------------------------------------------------------- 2. every seam of any window width
@pytest.fixture(scope="module")
def seam_rows():
    """20,001 single-key rows at q0 + d / 64 and 20,001 two-key rows {c, c + eps}, d = -10000..10000, with the
    reference's rows for the queries [q0] and [q0, q0 + eps], computed once."""
    d = np.arange(-10_000, 10_001)
    one = [(i + 1, [Q0 + int(x) * E64]) for i, x in enumerate(d)]
    two = [(i + 1, [Q0 + int(x) * E64, Q0 + (int(x) + 1) * E64]) for i, x in enumerate(d)]
    q1, q2 = [Q0], [Q0, Q0 + E64]
    mo = MAX_B * E64
    return d, (one, q1, awr.align_wide_ref(one, q1, E64, mo)), (two, q2, awr.align_wide_ref(two, q2, E64, mo))


@pytest.mark.parametrize("keys", (1, 2))
def test_every_bin_of_a_20001_bin_range(dc, seam_rows, keys):
    """Whatever the window's width and origin, some d of -10000..10000 is its first bin and d - 1 its neighbour's
    last: a single-key row votes there alone, a two-key row has its peak of 2 at d and 1 vote on either side of it
    (for a seam right of the peak: a one-vote bin in the next window must not beat the two)."""
    d, one, two = seam_rows
    rows, q, aligned = one if keys == 1 else two
    assert (aligned[:, 2] == d).all() and (aligned[:, 3] == keys).all()           # the premise
    mo = MAX_B * E64
    for i0 in range(0, len(rows), 64):                                            # k = 64: every row shows in a block
        part = rows[i0:i0 + 64]
        dc.upload(part)
        exp = _check(dc, part, [q], E64, mo, 64, aligned=[aligned[i0:i0 + 64]])
        assert exp[0, 64, 1] == len(part)


# ------------------------------------------------------------------------------------------------------ 3. limits
def test_limits_of_the_bin_range(dc):
    rows = [(1, [Q0 + MAX_B * E64]), (2, [Q0 - MAX_B * E64]), (3, [Q0 + MAX_B * E64, Q0 - MAX_B * E64]),
            (4, [Q0 + (MAX_B + 1) * E64]), (5, [Q0 - (MAX_B + 1) * E64]), (6, [Q0])]
    vid = 10
    for j in range(10, 23):
        for d in (2 ** j - 1, 2 ** j + 1, -(2 ** j - 1), -(2 ** j + 1)):
            rows.append((vid, [Q0 + d * E64]))
            vid += 1
    assert len(rows) <= 64
    dc.upload(rows)
    exp = _check(dc, rows, [[Q0]], E64, MAX_B * E64, 64)
    got = {r[0]: r.tolist() for r in exp[0, :64] if r[0] >= 0}
    assert got[1] == [1, 1, MAX_B, 1] and got[2] == [2, 1, -MAX_B, 1] and got[3] == [3, 2, -MAX_B, 1]
    assert 4 not in got and 5 not in got and exp[0, 64, 1] == len(rows) - 4       # 2^22 + 1 twice more, from j = 22
    exp = _check(dc, rows, [[Q0]], E64, 0.0, 64)                                  # B = 0
    assert exp[0, :2].tolist() == [[6, 1, 0, 1], [-1, 0, 0, 0]] and exp[0, 64, 1] == 1
    for mo in ((2 ** 12 - 1) * E64, 2 ** 12 * E64, (2 ** 12 + 1) * E64, 2047 * E64, 2048 * E64):
        _check(dc, rows, [[Q0]], E64, mo, 64)


# ---------------------------------------------------------------------------------------- 4. aliasing and carry-over
def test_votes_whole_windows_apart(dc):
    """3 votes at bin d and 2 at d + w for window-sized w: a histogram that folds d + w onto d would count 5, one not
    cleared between windows would carry the 3 over."""
    q = [Q0, Q0 + 7.0, Q0 + 19.0]
    rows, d = [], 5
    for i, w in enumerate((1024, 2048, 4095, 4096, 8192)):
        for sign in (1, -1):
            rows.append((len(rows) + 1, [x + d * E64 for x in q] + [x + (d + sign * w) * E64 for x in q[:2]]))
    # votes 10^6 bins apart, equal counts: the smaller |bin|; then the negative one
    rows += [(20, [Q0 + 100 * E64, Q0 + 1_000_100 * E64]), (21, [Q0 - 1_000_100 * E64, Q0 + 100 * E64]),
             (22, [Q0 - 1_000_000 * E64, Q0 + 1_000_000 * E64])]
    dc.upload(rows)
    exp = _check(dc, rows, [q, [Q0]], E64, MAX_B * E64, 16)
    assert sorted(r.tolist() for r in exp[0, :10]) == [[v, 5, d, 3] for v in range(1, 11)]
    got = {r[0]: r.tolist() for r in exp[1, :16] if r[0] >= 0}
    assert got[20] == [20, 2, 100, 1] and got[21] == [21, 2, 100, 1] and got[22] == [22, 2, -1_000_000, 1]


def test_a_row_without_votes_between_two_rows_with_peaks(dc):
    """More rows than the grid has waves (align_ref.GRID_WAVES): wave w takes rows w, w + 8192, w + 16384.  The first
    pass peaks at bin 5000, the second has no vote at all (keys far outside +-2^22 bins), the third peaks at bin
    -70000: windows apart from the first's."""
    n = 20_000
    rows = []
    for r in range(n):
        if r < ar.GRID_WAVES:
            keys = [Q0 + 5000 * E64]
        elif r < 2 * ar.GRID_WAVES:
            keys = [Q0 + 1e6 + r]
        else:
            keys = [Q0 - 70_000 * E64, Q0 - 70_000 * E64 + 3.0]
        rows.append((r + 1, keys))
    dc.upload(rows)
    aligned = awr.align_wide_ref(rows, [Q0], E64, MAX_B * E64)
    assert (aligned[ar.GRID_WAVES:2 * ar.GRID_WAVES, 3] == 0).all()
    for k in (16, 64):
        exp = _check(dc, rows, [[Q0]], E64, MAX_B * E64, k, aligned=[aligned])
        assert exp[0, k, 1] == n - ar.GRID_WAVES
    exp = _check(dc, rows, [[Q0]], E64, MAX_B * E64, 64, aligned=[aligned], min_score=atr.ONE // 2 + 1)
    assert exp[0, 64, 1] == ar.GRID_WAVES and (exp[0, :64, 2] == 5000).all()


# ------------------------------------------------------------------------------------------------- 5. far copies
@pytest.fixture(scope="module")
def films():
    rng = np.random.default_rng(2026)
    fixed = {7: 60, 8: 60, 40: 30, 41: 30}                     # the rows the queries are made from
    rows = [(v, np.sort(rng.uniform(0.0, 7200.0, size=fixed.get(v) or int(rng.integers(1, 61)))).tolist())
            for v in range(1, 301)]
    return rows, dict(rows)


@pytest.mark.parametrize("eps", (1 / 30, 0.001, E64), ids=("30fps", "1ms", "dyadic"))
def test_far_copies(dc, films, eps):
    rows, by = films
    rng = np.random.default_rng(99)
    dc.upload(rows)
    mo = MAX_B * eps
    assert awr.n_bins(eps, mo) == MAX_B
    excerpt = by[7][24:36]
    jitter = (np.asarray(by[8]) + rng.uniform(-eps / 4, eps / 4, size=60)).tolist()
    queries = [(np.asarray(by[40]) + 3600.0).tolist(), (np.asarray(by[41]) - 3600.0).tolist(), excerpt, jitter,
               np.sort(rng.uniform(0.0, 7200.0, size=25)).tolist()]
    aligned = [awr.align_wide_ref(rows, q, eps, mo) for q in queries]
    for contain in (False, True):
        exp = _check(dc, rows, queries, eps, mo, 16, aligned=aligned, contain=contain)
        _check(dc, rows, queries, eps, mo, 16, aligned=aligned, contain=contain, exclude_ids=[40, 41, 7, 8, -1])
        if contain:                            # (a row of one cut is contained by any single vote: ask for three)
            exp = _check(dc, rows, queries, eps, mo, 64, aligned=aligned, contain=contain, min_votes=3)
        # the shifted copies: row 0 of their blocks, at the shift (key - query value = -shift)
        assert exp[0, 0].tolist() == [40, 30, round(-3600.0 / eps), 30]
        assert exp[1, 0].tolist() == [41, 30, round(3600.0 / eps), 30]
        assert exp[3, 0].tolist() == [8, 60, 0, 60]
    # the excerpt: all 12 cuts align with row 7 - contained in full, a Jaccard of 12 / 60
    hit = [h for h in awr.hits_of(aligned[2], 12, contain=True) if h[1][0] == 7][0]
    assert hit[0][0] == -atr.ONE and hit[1] == (7, 60, 0, 12)
    s_j = awr.score(12, 12, 60)[1]
    assert s_j == atr.ONE // 5
    for contain, s in ((True, atr.ONE), (False, s_j)):                               # at and just above a hit's score
        exp = _check(dc, rows, queries, eps, mo, 16, aligned=aligned, contain=contain, min_score=s)
        assert 7 in exp[2, :16, 0].tolist()
        if s < atr.ONE:
            exp = _check(dc, rows, queries, eps, mo, 16, aligned=aligned, contain=contain, min_score=s + 1)
            assert 7 not in exp[2, :16, 0].tolist()
    # the Python call: rows and totals of the same blocks; max_offset=None is the widest
    exp = awr.topk_wide_ref(rows, queries, eps, mo, 8, aligned=aligned, contain=True, min_votes=2)
    got_rows, got_totals = dc.align_wide_topk(queries, eps=eps, k=8, contain=True, min_votes=2)
    assert got_rows.dtype == got_totals.dtype == np.int32 and dc.supports_align_wide
    _expect_blocks(got_rows, exp[:, :8], "rows of the Python call")
    assert got_totals.tolist() == exp[:, 8, 1].tolist()
    live = [r for r in exp[2, :8].tolist() if r[0] >= 0]
    assert len(live) > 1 and live == sorted(live, key=lambda r: tc.align_wide_order_key(r, 12, contain=True))


# ----------------------------------------------------------------------------------- 6. long rows and special keys
def test_long_rows_shifted_by_1000_seconds(dc):
    _, rows, _ = ar.long_rows_case()
    dc.upload(rows)
    keys = np.asarray(rows[4][1])
    queries = [(keys - 1000.0).tolist(), (keys[:66] + 1000.0).tolist()]
    for eps in (0.05, E64):
        mo = MAX_B * eps
        aligned = [awr.align_wide_ref(rows, q, eps, mo) for q in queries]
        exp = _check(dc, rows, queries, eps, mo, 16, aligned=aligned)
        assert exp[0, 0, 0] == 5 and exp[0, 0, 3] >= 1000 and abs(exp[0, 0, 2] - round(1000.0 / eps)) <= 1
        _check(dc, rows, queries, eps, mo, 16, aligned=aligned, contain=True, min_votes=64)


def test_special_keys_at_the_widest_range(dc):
    _, rows, calls = ar.special_keys_case()
    dc.upload(rows)
    queries = [list(q) for q, eps, _ in calls if eps == 0.1]
    exp = _check(dc, rows, queries, 0.1, MAX_B * 0.1, 16)
    assert exp[1, 16].tolist() == exp[2, 16].tolist() == [-1, 0, 0, 0]             # the empty and the NaN-only query
    _check(dc, rows, queries, 0.1, MAX_B * 0.1, 16, contain=True)


def test_batch_edges_and_the_table_at_the_call(dc):
    # two rows of one video id whose best bins differ only in sign: ordered by the bin as a signed number
    rows = [(9, [Q0 + 5000 * E64]), (9, [Q0 - 5000 * E64]), (3, [Q0 + 3_000_000 * E64, Q0 + 7.0])]
    dc.upload(rows)
    mo = MAX_B * E64
    exp = _check(dc, rows, [[Q0]], E64, mo, 16)
    assert exp[0, :3].tolist() == [[9, 1, -5000, 1], [9, 1, 5000, 1], [3, 2, 448, 1]]
    # five queries of different lengths, one longer than max_query_len: refused alone
    queries = [[Q0], [Q0, Q0 + 1.0, Q0 + 2.0], [Q0 + i for i in range(9)], [], [Q0 - 7.0] * 8]
    exp = _check(dc, rows, queries, E64, mo, 4, max_query_len=8)
    assert exp[2].tolist() == [[-1, 0, 0, 0]] * 4 + [[-1, atr.REFUSED, 0, 0]] and exp[0, 4, 1] == 3 and exp[4, 4, 1] > 0
    # an upsert made before the call is seen
    dc.upsert(5, [Q0 + 777 * 64 * E64])
    rows.append((5, [Q0 + 777.0]))
    exp = _check(dc, rows, [[Q0]], E64, mo, 16)
    assert [5, 1, 777 * 64, 1] in exp[0, :16].tolist()
    # Q = 0: nothing to do, nothing written; an empty corpus: no hits
    out = torch.full((1, 17, 4), SENTINEL, dtype=torch.int32, device=DEV)
    assert _raw(dc, [], E64, mo, 16, out=out)[0] == 0 and (out == SENTINEL).all()
    dc.clear()
    exp = _check(dc, [], [[Q0], []], E64, mo, 16)
    assert exp[:, 16].tolist() == [[-1, 0, 0, 0]] * 2


# --------------------------------------------------------------------------------------- 7. refusals write nothing
def test_refusals_write_nothing(dc):
    rows = [(1, [Q0, Q0 + 1.0]), (2, [Q0 + 5.0])]
    dc.upload(rows)
    q = [[Q0, Q0 + 1.0]]
    out = torch.full((1, 17, 4), SENTINEL, dtype=torch.int32, device=DEV)
    need = tc.align_wide_topk_workspace_bytes(1, 2, 2, 16)
    ws = torch.full((need + 256,), CANARY, dtype=torch.uint8, device=DEV)
    invalid, unsupported = ar.ERR_INVALID, ar.ERR_UNSUPPORTED

    def call(eps=E64, mo=1.0, k=16, **kw):
        kw.setdefault("ws_bytes", need)
        return _raw(dc, q, eps, mo, k, out=out, ws=ws, **kw)[0]

    assert call(mo=(MAX_B + 1) * E64) == unsupported
    assert b"TVZ_ALIGN_WIDE_MAX_B" in _lib.load().tvz_last_error()
    assert call(mo=(MAX_B + 0.5) * E64) == unsupported                             # rounds up to 2^22 + 1
    assert call(mo=float("inf")) == unsupported
    assert call(eps=float("inf"), mo=float("inf")) == unsupported                  # a NaN quotient
    n_invalid = 0
    for eps, mo, code in ar.REFUSALS:
        if code == invalid:
            assert call(eps=eps, mo=mo) == invalid, (eps, mo)
            n_invalid += 1
    assert n_invalid == 6
    assert call(flags=2) == invalid and call(flags=0x80000001) == invalid
    assert call(k=0) == unsupported and call(k=65) == unsupported
    assert call(max_query_len=4096) == unsupported
    assert call(min_votes=0) == invalid
    assert call(min_score=-1) == invalid and call(min_score=atr.ONE + 1) == invalid
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE
    assert b"1 bytes missing" in _lib.load().tvz_last_error()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (ws == CANARY).all()
    # right next to the refused ones: the widest range, with a workspace of exactly the reported size - the bytes
    # behind it stay as they were
    assert call(mo=(MAX_B + 0.49) * E64, k=16) == 0
    torch.cuda.synchronize()
    assert (ws[need:] == CANARY).all()
    _expect_blocks(out.cpu().numpy(), awr.topk_wide_ref(rows, q, E64, MAX_B * E64, 16), "after the refusals")


# ------------------------------------------------------------------------------------------------- 8. the inspector
class _NoWideCorpus:
    def align(self, timestamps, eps=0.1, max_offset=60.0):
        return np.zeros((0, 5), dtype=np.int32)

    def align_topk(self, queries, **kw):
        return np.zeros((len(queries), kw["k"], 4), dtype=np.int32), np.zeros(len(queries), dtype=np.int32)


class _NoWideStore:
    corpus = _NoWideCorpus()


def test_inspector_near_any_offset(tmp_path):
    """A stored clip and an upload that is the same clip behind 3,000 blank frames (100 s at 30 fps: beyond the
    bounded search's +-68 s at the default near_eps): invisible to near_top_k alone, reported with near_any_offset."""
    from tests.fakes import CutReader, cut_inspector
    from tvidz_amd import db as tdb, inspector as insp

    with pytest.raises(RuntimeError, match="align_wide_topk"):
        insp.Inspector(_NoWideStore(), device=DEV, near_duplicates=True, near_top_k=8, near_any_offset=True)
    with pytest.raises(ValueError, match="near_top_k"):
        insp.Inspector(_NoWideStore(), device=DEV, near_duplicates=True, near_any_offset=True)
    with pytest.raises(ValueError, match="near_any_offset"):
        insp.Inspector(_NoWideStore(), device=DEV, near_duplicates=True, near_top_k=8, near_score="containment")

    clip = [1.0, 2.5, 4.0, 7.3, 9.9, 12.0]
    shift = 100.0
    cuts = {"a.y4m": clip, "c.y4m": [0.7, 3.3, 5.1, 8.8], "b.y4m": [x + shift for x in clip]}
    res = {}
    for any_offset in (False, True):
        store = tdb.Store(f"sqlite:///{tmp_path}/{int(any_offset)}.db", corpus=tc.DeviceCorpus(0))
        kw = dict(near_any_offset=True, near_score="containment", near_min_votes=3) if any_offset else {}
        ins = cut_inspector(store, device=DEV, near_duplicates=True, near_top_k=8, **kw,
                            frame_source=lambda bucket, key, filename, uid: (CutReader(cuts[key], frames=3600), None))
        try:
            res[any_offset] = [ins.analyze_file("videos", k) for k in ("a.y4m", "c.y4m", "b.y4m")]
        finally:
            store.close()                      # closes the corpus too
        assert all(r["status"] == "done" for r in res[any_offset]), res[any_offset]
    assert res[False][2]["near_duplicates"] == []
    (near,) = res[True][2]["near_duplicates"]
    assert near["filename"] == "a.y4m" and near["containment"] == 1.0 and near["jaccard"] == 1.0
    assert abs(near["shift_seconds"] - (-shift)) <= 1.0 / 30
    assert [r["duplicates"] for r in res[False]] == [r["duplicates"] for r in res[True]]
    assert res[False][0]["near_duplicates"] == res[True][0]["near_duplicates"] == []
