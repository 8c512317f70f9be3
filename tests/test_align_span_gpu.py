"""GPU parity of tvz_align_span_topk (ts_aligns_sweep_kernel + ts_aligns_reduce_kernel), its merge
(ts_aligns_merge_kernel) and its forms over shards: whole [Q, k + 1, 8] blocks, bit-exact, against
tests/align_span_ref.py - and against the blocks of tvz_align_rates_topk and tvz_align_wide_topk column for column."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import align_rates_ref as arr, align_ref as ar, align_span_ref as asr, align_topk_ref as atr, align_wide_ref as awr
from tests.test_align_rates_gpu import _queries as _base_queries, _table as _base_table
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -0x5A5A5A5A
POISON = 0x5A5A5A5A
CANARY = 0xA5
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -4, -5           # include/tvz.h
MAX_B = 1 << 22
EPS = 1 / 30
ONE = 1 << 20
INF, NAN = float("inf"), float("nan")
RATE_SETS = ((1.0,), (1.0, 0.96))
BS = (900, 5000, MAX_B)
KS = (1, 16, 64)
KINDS = (dict(), dict(contain=True), dict(local=True))


@pytest.fixture(scope="module")
def dc():
    c = tc.DeviceCorpus(0)
    yield c
    c.close()


def _flags(contain=False, local=False):
    return (tc.ALIGN_CONTAIN if contain else 0) | (tc.ALIGN_LOCAL if local else 0)


def _raw(dc, queries, eps, mo, rates, k, min_votes=1, min_score=0, flags=0, exclude_ids=None, max_query_len=None, out=None,
         ws=None, ws_bytes=None, n_rates=None):
    """tvz_align_span_topk through the C ABI -> (return code, the [Q, k + 1, 8] device block)."""
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    L = min(longest, atr.MAX_LEN) if max_query_len is None else max_query_len
    d_ex = None if exclude_ids is None else torch.as_tensor(np.asarray(exclude_ids, dtype=np.int32)).to(DEV)
    Q = len(queries)
    if out is None:
        out = torch.full((Q, max(k, 0) + 1, 8), SENTINEL, dtype=torch.int32, device=DEV)
    need = tc.align_span_topk_workspace_bytes(Q, min(max(L, 0), atr.MAX_LEN), d_q.numel(), min(max(k, 1), 64))
    if ws is None:
        ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    h = None if rates is None else (C.c_double * max(len(rates), 1))(*rates)
    n = (0 if rates is None else len(rates)) if n_rates is None else n_rates
    s = torch.cuda.current_stream(DEV)
    rc = _lib.load().tvz_align_span_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), Q, int(L), float(eps), float(mo), h, n,
                                         int(min_votes), int(min_score), int(flags),
                                         d_ex.data_ptr() if d_ex is not None else None, int(k), out.data_ptr(),
                                         ws.data_ptr(), need if ws_bytes is None else ws_bytes, s.cuda_stream)
    s.synchronize()
    return rc, out


def _expect_blocks(got, exp, what):
    got = np.asarray(got, dtype=np.int64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere((got != exp).any(axis=2))
    assert bad.size == 0, (what, f"{len(bad)} rows differ", [(q, r, got[q, r].tolist(), exp[q, r].tolist())
                                                             for q, r in bad[:4].tolist()])


def _check(dc, rows, queries, eps, mo, rates, k, aligned=None, contain=False, local=False, **kw):
    exp = asr.topk_span_ref(rows, queries, eps, mo, rates, k, aligned=aligned, contain=contain, local=local, **kw)
    rc, out = _raw(dc, queries, eps, mo, rates, k, flags=_flags(contain, local), **kw)
    assert rc == 0, _lib.load().tvz_last_error()
    _expect_blocks(out.cpu().numpy(), exp, (eps, mo, rates, k, contain, local, kw))
    return exp


# ------------------------------------------------------------------------------------------------ 1. the contract
SHIFT = 100 * EPS + 0.001                                                          # bin 100, well inside it
VID = dict(lanes70=201, lanes130=202, long600=203, stray=204, close=205, dups=206, special=207, zero=208, negative=209,
           tie=77)


def _voters_and_fillers(x, below, between, above, shift=SHIFT):
    """A row whose voters are x + shift (one per value of x, 7 s apart), with `below` / `above` keys beyond both ends
    and `between` keys inside, every one at least 0.9 s from a voter: none of them votes at the shift."""
    v = np.asarray(x) + shift
    n_gap = -(-between // (len(v) - 1))
    inner = [v[g] + 1.0 + (i + 0.37 * (g % 3)) * (5.0 / n_gap) for g in range(len(v) - 1) for i in range(n_gap)][:between]
    lo = [v[0] - 3.0 - 1.3 * i for i in range(below)]
    hi = [v[-1] + 3.0 + 1.3 * i for i in range(above)]
    keys = np.sort(np.concatenate([v, inner, lo, hi]))
    assert len(keys) == len(v) + below + between + above
    return keys.tolist()


def _world_rows_and_queries():
    rows = _base_table()
    queries = _base_queries(rows)
    x20 = [3000.0 + 7.0 * i for i in range(20)]
    # 6: span ends found by different lanes, by one lane's stride, and beyond the 512 resume positions; keys inside the
    # span that do not vote (nr > votes); bins positive, zero and negative
    queries.append(x20)
    rows.append((VID["lanes70"], _voters_and_fillers(x20, 3, 45, 2)))               # extremes: keys 3 and 67
    rows.append((VID["lanes130"], _voters_and_fillers(x20, 5, 45, 60)))             # keys 5 and 69: lane 5 twice
    rows.append((VID["long600"], _voters_and_fillers(x20, 100, 441, 39)))           # keys 100 and 560
    rows.append((VID["zero"], _voters_and_fillers(x20[4:16], 2, 0, 2, shift=0.0)))
    rows.append((VID["negative"], _voters_and_fillers(x20[2:9], 0, 6, 1, shift=-40.0)))
    # 7: a 20-vote cluster and one stray pair in the same bin far outside it
    x40 = [5000.0 + 7.0 * i for i in range(40)]
    queries.append(x40)
    cluster = np.asarray(x40[5:25]) + SHIFT
    filler = [cluster[-1] + 1.75 + 3.5 * i for i in range(30)]                     # between the cluster and the stray
    assert filler[-1] < x40[39] + SHIFT - 1.0 and all(0.5 < (f - cluster[0]) % 7.0 < 6.5 for f in filler)
    rows.append((VID["stray"], np.sort(np.concatenate([cluster, filler, [x40[39] + SHIFT]])).tolist()))
    # 8: two keys closer than eps voting with one query value (votes > nq), and query duplicates at both ends
    x8 = [6000.0 + 7.0 * i for i in range(8)]
    queries.append(x8)
    rows.append((VID["close"], sorted([x + SHIFT for x in x8] + [x + SHIFT + EPS / 4 for x in x8])))
    xd = [6500.0] * 3 + [6500.0 + 7.0 * i for i in range(1, 9)] + [6563.0] * 2 + [100.0, 7100.0]
    queries.append(xd)
    rows.append((VID["dups"], sorted(set(x + SHIFT for x in xd[:13]))))
    # 10: both zeros, NaNs and both infinities in the query, infinities in the row
    queries.append([-0.0, 9.0, NAN, 5.0, INF, 0.0, -INF, NAN, 0.0, -0.0])
    rows.append((VID["special"], [0.0 + SHIFT, 5.0 + SHIFT, 9.0 + SHIFT, INF, -INF, 7.0 + SHIFT + 1.0]))
    # 11: rows equal in the first six fields - one video id, row_len, bin, votes, rate - that differ in the span only
    xt = [6800.0 + 7.0 * i for i in range(12)]
    queries.append(xt)
    far = [9000.0, 9001.5]
    rows.append((VID["tie"], sorted([x + SHIFT for x in xt[2:6]] + far)))           # t 2..5, nr 4
    rows.append((VID["tie"], sorted([x + SHIFT for x in xt[0:4]] + far)))           # t 0..3, nr 4
    rows.append((VID["tie"], sorted([x + SHIFT for x in (xt[0], xt[1], xt[2], xt[4])] + [xt[3] + SHIFT + 2.0, 9000.0])))  # t 0..4, nr 5
    rows.append((VID["tie"], sorted([x + SHIFT for x in (xt[0], xt[1], xt[3], xt[4])] + far)))       # t 0..4, nr 4
    return rows, queries


@pytest.fixture(scope="module")
def world():
    rows, queries = _world_rows_and_queries()
    cache = {}

    def aligned(rates, B):
        if (rates, B) not in cache:
            cache[rates, B] = [asr.align_span_ref(rows, q, EPS, B * EPS, rates) for q in queries]
        return cache[rates, B]
    return rows, queries, aligned


def _row_of(aligned_q, rows, vid, nth=0):
    idx = [i for i, (v, _) in enumerate(rows) if v == vid][nth]
    return aligned_q[idx].tolist()


def test_the_premises_of_the_world(world):
    """What the added rows are there for, read off the reference (no device)."""
    rows, queries, aligned = world
    a = aligned((1.0,), MAX_B)
    keys = {vid: np.asarray(asr.row_set(ks)) for vid, ks in rows if vid != VID["tie"]}
    for name, first, last, nr in (("lanes70", 3, 67, 65), ("lanes130", 5, 69, 65), ("long600", 100, 560, 461)):
        r = _row_of(a[6], rows, VID[name])
        assert r[2:] == [100, 20, 0, 0, 19, nr], (name, r)
        c, ki, _ = asr.pairs_of(keys[VID[name]], queries[6], EPS, 100, 1.0)
        assert (ki.min(), ki.max()) == (first, last), name
    assert first % 64 != last % 64 and 5 % 64 == 69 % 64 and last > 512
    assert _row_of(a[6], rows, VID["zero"])[2:] == [0, 12, 0, 4, 15, 12]
    # (the query is periodic: x[2:9] - 40 is x[0:7] - 26 too, the same seven votes; the smaller |bin| wins)
    assert _row_of(a[6], rows, VID["negative"])[2:] == [-780, 7, 0, 0, 6, 13]
    r = _row_of(a[7], rows, VID["stray"])
    assert r[1:] == [51, 100, 21, 0, 5, 39, 51] and asr.score_of(r, 40, local=True) == (21, (21 << 20) // 65)
    r = _row_of(a[8], rows, VID["close"])
    assert r[1:] == [16, 100, 16, 0, 0, 7, 16] and asr.score_of(r, 8, local=True) == (8, (8 << 20) // 16)   # v clipped to nq
    r = _row_of(a[9], rows, VID["dups"])                                           # 100.0 sorts first: the triple is 1..3
    assert r[1:] == [10, 100, 13, 0, 1, 13, 10]
    r = _row_of(a[10], rows, VID["special"])                                       # sorted: -inf, four zeros, 5, 9, inf
    assert r[1:] == [6, 100, 6, 0, 1, 6, 4]                                        # (the key at 8 + shift is inside, silent)
    ties = [_row_of(a[11], rows, VID["tie"], n) for n in range(4)]
    assert all(t[:5] == [77, 6, 100, 4, 0] for t in ties) and sorted(t[5:] for t in ties) == [[0, 3, 4], [0, 4, 4], [0, 4, 5], [2, 5, 4]]
    # the rate choice: the scaled query against row 34 is found at rate index 1, and at rate 0 its span would be another
    a2 = aligned((1.0, 0.96), MAX_B)
    r = a2[0][34].tolist()
    assert r[3:] == [40, 1, 0, 39, 40]
    r1 = a[0][34].tolist()
    assert r1[3] < 10 and r1[5:] != r[5:]


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("rates", RATE_SETS, ids=("r1", "r2"))
def test_contract(dc, world, rates, B):
    rows, queries, aligned = world
    dc.upload(rows)
    mo = B * EPS
    assert awr.n_bins(EPS, mo) == B
    a = aligned(rates, B)
    excl = [rows[34][0], -1, rows[30][0], -1, -1, 9, VID["lanes70"], VID["stray"], -1, -1, VID["special"], VID["tie"]]
    assert len(excl) == len(queries)
    for kind in KINDS:
        for k in KS:
            exp = _check(dc, rows, queries, EPS, mo, rates, k, aligned=a, **kind)
            _check(dc, rows, queries, EPS, mo, rates, k, aligned=a, min_votes=8, **kind)
        cut = _check(dc, rows, queries, EPS, mo, rates, 16, aligned=a, exclude_ids=excl, min_score=ONE // 8, **kind)
        assert (cut[:, 16, 1] < exp[:, 64, 1]).any()                               # the score and the exclusions cut
        assert exp[3, 64].tolist() == exp[4, 64].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0]      # the empty and the NaN-only query
    # the ties across the k boundary: k = 1 and 2 keep the first one and two of the four rows
    for kind in KINDS[:2]:
        top = asr.topk_span_ref(rows, queries, EPS, mo, rates, 4, aligned=a, **kind)[11, :4]
        if B <= 5000:                                                              # (at any shift the periodic queries of the
                                                                                   # other rows align better somewhere)
            assert (top[:, 0] == VID["tie"]).all() and top[:, 5:].tolist() == [[0, 3, 4], [0, 4, 4], [0, 4, 5], [2, 5, 4]]
        for k in (1, 2, 3):
            _check(dc, rows, queries[11:], EPS, mo, rates, k, aligned=a[11:], **kind)
    # the Python call: rows and totals of the same blocks, in the order of the Python key
    if B == MAX_B:
        for kind in KINDS:
            exp = asr.topk_span_ref(rows, queries, EPS, mo, rates, 16, aligned=a, min_votes=2, **kind)
            got_rows, got_totals = dc.align_span_topk(queries, eps=EPS, rates=rates, k=16, min_votes=2, **kind)
            assert got_rows.dtype == got_totals.dtype == np.int32 and got_rows.shape == (len(queries), 16, 8)
            _expect_blocks(got_rows, exp[:, :16], "rows of the Python call")
            assert got_totals.tolist() == exp[:, 16, 1].tolist()
            live = [r for r in exp[6, :16].tolist() if r[0] >= 0]
            assert len(live) > 3 and live == sorted(live, key=lambda r: tc.align_span_order_key(r, 20, **kind))


def test_a_table_smaller_than_a_block(dc, world):
    rows, queries, _ = world
    few = [rows[34], rows[30], rows[7]]
    dc.upload(few)
    for B in BS:
        _check(dc, few, queries[:6], EPS, B * EPS, RATE_SETS[1], 16, local=True)
        _check(dc, few, queries[:6], EPS, B * EPS, RATE_SETS[1], 1)
    dc.clear()
    exp = _check(dc, [], queries[:6], EPS, 30.0, RATE_SETS[1], 4, local=True)
    assert (exp[:, 4, 1] == 0).all()


# ----------------------------------------------------- 2. without LOCAL: the rates call's and the wide call's columns
@pytest.mark.parametrize("case", ar.edge_cases(), ids=lambda c: c[0])
def test_columns_equal_the_rates_and_the_wide_call_bit_for_bit(dc, case):
    name, rows, calls = case
    dc.upload(rows)
    lib = _lib.load()
    batches = {}
    for q, eps, mo in calls:
        batches.setdefault((eps, mo), []).append(list(q))
    for (eps, mo), queries in batches.items():
        d_q, d_off, longest = tc.pack_queries(queries, DEV)
        Q, L = len(queries), min(longest, atr.MAX_LEN)
        for k in KS:
            for flags in (0, 1):
                wide = dc.align_wide_topk_block(d_q, d_off, L, eps=eps, max_offset=mo, k=k, contain=bool(flags))
                rc, span = _raw(dc, queries, eps, mo, (1.0,), k, flags=flags)
                assert rc == 0, lib.tvz_last_error()
                assert torch.equal(span[:, :, :4], wide), (name, eps, mo, k, flags)
                for rates in ((1.0,), (1.0, 0.96)):
                    rated = dc.align_rates_topk_block(d_q, d_off, L, eps=eps, rates=rates, max_offset=mo, k=k, contain=bool(flags))
                    rc, span = _raw(dc, queries, eps, mo, rates, k, flags=flags)
                    assert rc == 0, lib.tvz_last_error()
                    assert torch.equal(span[:, :, :5], rated), (name, eps, mo, k, flags, rates)
                    assert (span[:, :k, 5:][span[:, :k, 0] < 0] == 0).all() and (span[:, k, 2:] == 0).all()
    # the spans themselves, against the reference, where the table is small enough for it
    if name not in ("grid_stride", "boundary"):
        for (eps, mo), queries in batches.items():
            for kind in KINDS:
                _check(dc, rows, queries, eps, mo, (1.0, 0.96), 16, **kind)


# ----------------------------------------------------------------------------------- 3. the product at the span's end
def test_the_kept_rates_product_is_rounded_before_the_subtraction(dc):
    c, x, rho, eps, j = arr.no_fma_case()
    xs = [100.0, 200.0, 300.0, x]
    keys = [float(np.float64(v) * np.float64(rho)) + (j - 0.25) * eps for v in xs[:3]] + [c]
    rows = [(1, keys)]
    dc.upload(rows)
    for mo in (100.0, MAX_B * eps):                                                # one window, and the window walk
        for rates in ((rho,), (1.0, rho)):
            for kind in KINDS:
                exp = _check(dc, rows, [xs], eps, mo, rates, 4, **kind)
                assert exp[0, 0].tolist() == [1, 4, j, 4, len(rates) - 1, 0, 3, 4]  # a fused product would end the span at 2


# --------------------------------------------------------------------------------------- 4. refusals write nothing
def test_refusals_write_nothing(dc):
    rows = [(1, [100.0, 101.0]), (2, [105.0])]
    dc.upload(rows)
    q = [[100.0, 101.0]]
    need = tc.align_span_topk_workspace_bytes(1, 2, 2, 16)
    out_bytes = 17 * 8 * 4
    arena = torch.full((256 + out_bytes + 256 + need + 512,), CANARY, dtype=torch.uint8, device=DEV)
    base = arena.data_ptr()
    o0 = (-base) % 256 + 256                                                        # d_out and the workspace inside it
    out = arena[o0:o0 + out_bytes].view(torch.int32).view(1, 17, 8)
    w0 = o0 + out_bytes + 256
    ws = arena[w0:w0 + need + 256]
    good = (1.0, 0.96)
    lib = _lib.load()

    def call(eps=EPS, mo=1.0, k=16, rates=good, **kw):
        kw.setdefault("ws_bytes", need)
        return _raw(dc, q, eps, mo, rates, k, out=out, ws=ws, **kw)[0]

    assert call(flags=3) == ERR_INVALID and b"TVZ_ALIGN_CONTAIN and TVZ_ALIGN_LOCAL" in lib.tvz_last_error()
    assert call(flags=4) == ERR_INVALID and call(flags=0x80000002) == ERR_INVALID
    assert call(rates=()) == ERR_UNSUPPORTED and call(rates=(1.0,) * 9) == ERR_UNSUPPORTED
    assert call(rates=None, n_rates=1) == ERR_INVALID
    for bad in (NAN, INF, 0.0, -1.0):
        assert call(rates=(1.0, bad)) == ERR_INVALID, bad
    assert call(k=0) == ERR_UNSUPPORTED and call(k=65) == ERR_UNSUPPORTED
    assert call(max_query_len=4096) == ERR_UNSUPPORTED
    assert call(mo=(MAX_B + 1) * EPS) == ERR_UNSUPPORTED and b"TVZ_ALIGN_WIDE_MAX_B" in lib.tvz_last_error()
    assert call(mo=INF) == ERR_UNSUPPORTED
    assert call(eps=0.0) == ERR_INVALID and call(min_votes=0) == ERR_INVALID and call(min_score=-1) == ERR_INVALID
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE and b"1 bytes missing" in lib.tvz_last_error()
    assert call(ws_bytes=need - 1000, flags=2) == ERR_WORKSPACE and b"1000 bytes missing" in lib.tvz_last_error()
    torch.cuda.synchronize()
    assert (arena == CANARY).all()
    # the existing calls still refuse bit 2, with a live handle
    d_q, d_off, _ = tc.pack_queries(q, DEV)
    s = torch.cuda.current_stream(DEV).cuda_stream
    h = (C.c_double * 2)(*good)
    assert lib.tvz_align_rates_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), 1, 2, EPS, 1.0, h, 2, 1, 0, 2, None, 16,
                                    out.data_ptr(), ws.data_ptr(), need, s) == ERR_INVALID
    assert lib.tvz_align_wide_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), 1, 2, EPS, 1.0, 1, 0, 2, None, 16,
                                   out.data_ptr(), ws.data_ptr(), need, s) == ERR_INVALID
    torch.cuda.synchronize()
    assert (arena == CANARY).all()
    # right next to the refused ones: the widest range under LOCAL, with a workspace of exactly the reported size -
    # everything around the block and behind the workspace stays as it was
    assert call(mo=MAX_B * EPS, flags=2) == 0
    torch.cuda.synchronize()
    assert (arena[:o0] == CANARY).all() and (arena[o0 + out_bytes:w0] == CANARY).all() and (arena[w0 + need:] == CANARY).all()
    _expect_blocks(out.cpu().numpy(), asr.topk_span_ref(rows, q, EPS, MAX_B * EPS, good, 16, local=True), "after the refusals")


# ------------------------------------------------------------------------------------------ 5. the merge and _shards
def _merge(blocks, queries, flags=0):
    blocks = np.ascontiguousarray(blocks, dtype=np.int32)
    R, Q, k1, _ = blocks.shape
    d_b = torch.from_numpy(blocks).to(DEV)
    d_q, d_off, _ = tc.pack_queries(queries, DEV)
    rows = torch.full((Q, k1 - 1, 8), POISON, dtype=torch.int32, device=DEV)
    totals = torch.full((Q,), POISON, dtype=torch.int32, device=DEV)
    rc = _lib.load().tvz_align_span_topk_merge(d_b.data_ptr(), R, Q, k1 - 1, flags, d_q.data_ptr(), d_off.data_ptr(),
                                               rows.data_ptr(), totals.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, rows.cpu().numpy().astype(np.int64), totals.cpu().numpy().astype(np.int64)


def _check_merge(blocks, queries, contain=False, local=False):
    rc, rows, totals = _merge(blocks, queries, _flags(contain, local))
    assert rc == 0, _lib.load().tvz_last_error()
    exp_rows, exp_totals = asr.merge_ref(blocks, queries, contain, local)
    assert (totals == exp_totals).all(), (totals, exp_totals)
    assert (rows == exp_rows).all(), [(q, rows[q].tolist(), exp_rows[q].tolist()) for q in range(len(queries))
                                      if not (rows[q] == exp_rows[q]).all()][:1]
    return rows, totals


QUERIES4 = [[float(i) for i in range(10)], [float(i) if i % 2 else NAN for i in range(20)], [], [NAN] * 7]


@pytest.mark.parametrize("kind", KINDS, ids=("jaccard", "contain", "local"))
@pytest.mark.parametrize("n_lists,k", [(1, 1), (3, 5), (16, 64), (7, 16)])
def test_merge_of_hand_made_blocks(n_lists, k, kind):
    rng = np.random.default_rng(1000 * n_lists + k)
    nv = [atr.n_valid(q) for q in QUERIES4]
    lists = []
    for r in range(n_lists):
        per_q = []
        for qi in range(len(QUERIES4)):
            n = int(rng.integers(0, k + 3))
            hits = []
            for _ in range(n):
                t_first = int(rng.integers(0, 10))
                hits.append((int(rng.integers(0, 12)), int(rng.integers(1, 12)), int(rng.integers(-MAX_B, MAX_B + 1)),
                             int(rng.integers(1, 14)), int(rng.integers(0, 8)), t_first, t_first + int(rng.integers(0, 10)),
                             int(rng.integers(1, 12))))
            # rows equal in six fields and differing in the span, here and in the next list
            hits += [(0, 10, -70000, 10, 3, (r + i) % 3, 9 + (r + i) % 3, 10 + i % 2) for i in range(3)]
            per_q.append(hits)
        lists.append(per_q)
    blocks = np.stack([np.stack([asr.merge_block_of(lists[r][q], nv[q], k, **kind) for q in range(len(QUERIES4))])
                       for r in range(n_lists)])
    rows, totals = _check_merge(blocks, QUERIES4, **kind)
    if kind.get("contain"):
        assert (rows[3, :, 0] == -1).all()                                         # nv = 0: u = 0 under containment
    if kind.get("local"):
        assert (rows[2, :min(k, 3), 0] >= 0).all()                                 # the score needs no nv: an empty query's rows live
    if k >= 5 and not kind.get("local"):                                           # (nv = 10: they score 2^20, whatever the span)
        same = [r.tolist() for r in rows[0] if r[:5].tolist() == [0, 10, -70000, 10, 3]]
        assert len(same) >= 2 and [r[5:] for r in same] == sorted(r[5:] for r in same)
    # padding in the middle of a list; under LOCAL rows with nq <= 0 or nr <= 0; span indexes outside 0..4094
    if k >= 5:
        holes = blocks.copy()
        holes[:, :, 1] = (-1, 0, 0, 0, 0, 0, 0, 0)
        holes[0, 0, 3] = (-5, 9, 9, 9, 9, 1, 2, 3)
        if kind.get("local"):                                                      # (elsewhere the span only orders: a list
            holes[0, 0, 0, 5:7] = (7, 6)                                           # must stay sorted)      nq = 0
            holes[0, 1, 0, 5:7] = (9, 2)                                           # nq < 0
            holes[0, 0, 2, 7] = 0                                                  # nr = 0
            holes[0, 1, 2, 7] = -4                                                 # nr < 0
        if n_lists > 1:
            holes[1, 0, 0, 5] = 4095
            holes[1, 0, 2, 6] = -1
        _check_merge(holes, QUERIES4, **kind)


def test_a_refused_list_refuses_the_query_and_totals_saturate():
    nv = atr.n_valid(QUERIES4[0])
    for kind in KINDS:
        mk = lambda rows, n: asr.merge_block_of(rows, nv, 4, n_hits=n, **kind)       # noqa: E731
        a = [(1, 5, 100, 5, 2, 0, 4, 5), (2, 5, -100, 4, 0, 1, 5, 6)]
        blocks = np.stack([np.stack([mk(a, INT32_MAX - 1), mk(a, 2)]), np.stack([mk(a[:1], 7), mk(a, INT32_MIN)]),
                           np.stack([mk([], 0), mk(a, 1)])])
        rows, totals = _check_merge(blocks, [QUERIES4[0], QUERIES4[0]], **kind)
        assert totals.tolist() == [INT32_MAX, INT32_MIN] and (rows[1, :, 0] == -1).all() and (rows[1, :, 1:] == 0).all()
        assert rows[0, :3].tolist() == [list(a[0]), list(a[0]), list(a[1])]
    lib = _lib.load()
    d_b = torch.from_numpy(np.ascontiguousarray(blocks, dtype=np.int32)).to(DEV)
    d_q, d_off, _ = tc.pack_queries([QUERIES4[0]] * 2, DEV)
    out = torch.full((2, 4, 8), POISON, dtype=torch.int32, device=DEV)
    tot = torch.full((2,), POISON, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for n_lists, k, flags, off, want in ((0, 4, 0, 0, ERR_UNSUPPORTED), (17, 4, 0, 0, ERR_UNSUPPORTED), (3, 0, 0, 0, ERR_UNSUPPORTED),
                                         (3, 65, 0, 0, ERR_UNSUPPORTED), (3, 4, 3, 0, ERR_INVALID), (3, 4, 4, 0, ERR_INVALID),
                                         (3, 4, 0, 4, ERR_INVALID)):
        rc = lib.tvz_align_span_topk_merge(d_b.data_ptr() + off, n_lists, 2, k, flags, d_q.data_ptr(), d_off.data_ptr(),
                                           out.data_ptr(), tot.data_ptr(), s)
        assert rc == want, (n_lists, k, flags, off, lib.tvz_last_error())
    torch.cuda.synchronize()
    assert (out == POISON).all() and (tot == POISON).all()


def _upload_split(rows, R):
    shards = [tc.DeviceCorpus(0) for _ in range(R)]
    for r, s in enumerate(shards):
        s.upload(rows[r::R])
    return shards


@pytest.mark.parametrize("R", [3, 8])
def test_shards_equal_one_handle_and_the_reference(dc, world, R):
    rows, queries, aligned = world
    rates = RATE_SETS[1]
    dc.upload(rows)
    shards = _upload_split(rows, R)
    try:
        d_q, d_off, longest = tc.pack_queries(queries, DEV)
        for k, kind, B in ((1, KINDS[0], MAX_B), (16, KINDS[1], MAX_B), (16, KINDS[2], MAX_B), (64, KINDS[2], 5000)):
            mo = B * EPS
            ref = asr.topk_span_ref(rows, queries, EPS, mo, rates, k, aligned=aligned(rates, B), min_votes=2, **kind)
            one_rows, one_totals = dc.align_span_topk(queries, eps=EPS, rates=rates, max_offset=mo, k=k, min_votes=2, **kind)
            ws = torch.empty(tc.align_span_topk_workspace_bytes(len(queries), longest, d_q.numel(), k), dtype=torch.uint8,
                             device=DEV)
            blocks, got_rows, got_totals = tc.align_span_topk_shards(shards, d_q, d_off, longest, eps=EPS, rates=rates,
                                                                     max_offset=mo, k=k, workspace=ws, min_votes=2, **kind)
            torch.cuda.synchronize()
            assert blocks.shape == (R, len(queries), k + 1, 8)
            got_rows, got_totals = got_rows.cpu().numpy(), got_totals.cpu().numpy()
            assert (got_rows == one_rows).all() and (got_totals == one_totals).all(), (R, k, kind)
            assert (got_rows == ref[:, :k]).all() and (got_totals == ref[:, k, 1]).all(), (R, k, kind)
            m_rows, m_totals = tc.align_span_topk_merge(blocks, k, d_q, d_off, **kind)
            assert torch.equal(m_rows.cpu(), torch.from_numpy(got_rows)) and (m_totals.cpu().numpy() == got_totals).all()
        # a refusal of the flags comes before anything is written
        handles = (C.c_void_p * R)(*[s._h for s in shards])
        blocks = torch.full((R, len(queries), 5, 8), POISON, dtype=torch.int32, device=DEV)
        h = (C.c_double * 2)(1.0, 0.96)
        rc = _lib.load().tvz_align_span_topk_shards(handles, R, d_q.data_ptr(), d_off.data_ptr(), len(queries), longest, EPS,
                                                    30.0, h, 2, 1, 0, 3, None, 4, blocks.data_ptr(), blocks.data_ptr(),
                                                    blocks.data_ptr(), ws.data_ptr(), ws.numel(),
                                                    torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == ERR_INVALID and (blocks == POISON).all()
    finally:
        for s in shards:
            s.close()


def test_sharded_corpus_with_20_shards(world):
    from tvidz_amd import service
    rows, queries, aligned = world
    rates = RATE_SETS[1]
    sc = service.ShardedCorpus(0, n_shards=20, k=8)
    try:
        sc.upload(rows)
        excl = [rows[34][0], -1, -1, -1, -1, 9] + [-1] * (len(queries) - 6)
        for kw in ({"k": 8}, {"k": 3, "contain": True, "min_votes": 5}, {"k": 16, "local": True, "min_votes": 8},
                   {"k": 64, "local": True, "min_votes": 2, "exclude_ids": excl}):
            k = kw["k"]
            ref = asr.topk_span_ref(rows, queries, EPS, MAX_B * EPS, rates, aligned=aligned(rates, MAX_B), **kw)
            got = sc.align_span_topk(queries, eps=EPS, rates=rates, **kw)
            assert got[0].dtype == np.int32 and got[0].shape == (len(queries), k, 8)
            assert (got[0] == ref[:, :k]).all() and (got[1] == ref[:, k, 1]).all(), kw
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------- 6. the inspector
@pytest.mark.parametrize("rate", [1.0, 0.96], ids=("plain", "24to25fps"))
def test_inspector_finds_the_clip_inside_a_compilation(tmp_path, rate):
    """A stored film of 400 cuts and an upload of 400 cuts that holds 20 of the film's - played at 25 fps where the film
    has 24 for the second case: found with near_score="local", invisible to the containment at the same near_jaccard."""
    from tests.fakes import CutReader, cut_inspector
    from tvidz_amd import db as tdb

    film, upload, clip, shift = asr.compilation_case(rate=rate)
    cuts = {"film.y4m": film, "compilation.y4m": upload}
    s = sorted(upload)
    first = s.index(min(s, key=lambda x: abs(rate * x + shift - clip[0])))          # the clip's cuts: 20 neighbours
    last = first + 19
    res = {}
    for score in ("containment", "local"):
        store = tdb.Store(f"sqlite:///{tmp_path}/{score}.db", corpus=tc.DeviceCorpus(0))
        kw = dict(near_rates=(1.0, 0.96)) if rate != 1.0 else {}
        ins = cut_inspector(store, device=DEV, near_duplicates=True, near_top_k=8, near_any_offset=True, near_score=score,
                            near_min_votes=8, near_jaccard=0.5, **kw,
                            frame_source=lambda bucket, key, filename, uid: (CutReader(cuts[key], per_batch=100, frames=9000), None))
        try:
            res[score] = [ins.analyze_file("videos", k) for k in ("film.y4m", "compilation.y4m")]
        finally:
            store.close()
        assert all(r["status"] == "done" for r in res[score]), res[score]
    assert res["containment"][1]["near_duplicates"] == []
    (near,) = res["local"][1]["near_duplicates"]
    assert near["filename"] == "film.y4m" and near["local"] == 1.0 and near["jaccard"] == round(20 / 780, 4)
    sh = near["shift_seconds"]
    assert abs(sh - shift) <= EPS
    assert near["upload_span"] == [s[first], s[last]]
    assert near["stored_span"] == [rate * s[first] + sh, rate * s[last] + sh]
    assert abs(near["stored_span"][0] - clip[0]) <= EPS and abs(near["stored_span"][1] - clip[-1]) <= EPS
    assert (near.get("rate") == 0.96) if rate != 1.0 else ("rate" not in near)
    assert [r["duplicates"] for r in res["containment"]] == [r["duplicates"] for r in res["local"]]
