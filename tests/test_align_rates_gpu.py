"""GPU parity of tvz_align_rates_topk (ts_alignr_sweep_kernel + ts_alignr_reduce_kernel), its merge
(ts_alignr_merge_kernel) and its forms over shards: whole [Q, k + 1, 5] blocks, bit-exact, against
tests/align_rates_ref.py - and against tvz_align_wide_topk's own blocks at the single rate 1.0."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import align_rates_ref as arr, align_ref as ar, align_topk_ref as atr, align_wide_ref as awr
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
INF, NAN = float("inf"), float("nan")
RATE_SETS = ((1.0,), (1.0, 0.96), (0.96, 1.0, 25 / 24, 1001 / 1000, 1000 / 1001, 1.25, 0.8, 2.0))
BS = (900, 5000, MAX_B)
KS = (1, 16, 64)


@pytest.fixture(scope="module")
def dc():
    c = tc.DeviceCorpus(0)
    yield c
    c.close()


def _raw(dc, queries, eps, mo, rates, k, min_votes=1, min_score=0, flags=0, exclude_ids=None, max_query_len=None, out=None,
         ws=None, ws_bytes=None, n_rates=None):
    """tvz_align_rates_topk through the C ABI -> (return code, the [Q, k + 1, 5] device block).  rates=None: a NULL
    list."""
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    L = min(longest, atr.MAX_LEN) if max_query_len is None else max_query_len
    d_ex = None if exclude_ids is None else torch.as_tensor(np.asarray(exclude_ids, dtype=np.int32)).to(DEV)
    Q = len(queries)
    if out is None:
        out = torch.full((Q, max(k, 0) + 1, 5), SENTINEL, dtype=torch.int32, device=DEV)
    need = tc.align_rates_topk_workspace_bytes(Q, min(max(L, 0), atr.MAX_LEN), d_q.numel(), min(max(k, 1), 64))
    if ws is None:
        ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    h = None if rates is None else (C.c_double * max(len(rates), 1))(*rates)
    n = (0 if rates is None else len(rates)) if n_rates is None else n_rates
    s = torch.cuda.current_stream(DEV)
    rc = _lib.load().tvz_align_rates_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), Q, int(L), float(eps), float(mo), h, n,
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


def _check(dc, rows, queries, eps, mo, rates, k, aligned=None, contain=False, **kw):
    exp = arr.topk_rates_ref(rows, queries, eps, mo, rates, k, aligned=aligned, contain=contain, **kw)
    rc, out = _raw(dc, queries, eps, mo, rates, k, flags=1 if contain else 0, **kw)
    assert rc == 0, _lib.load().tvz_last_error()
    _expect_blocks(out.cpu().numpy(), exp, (eps, mo, rates, k, contain, kw))
    return exp


# ------------------------------------------------------------------------------------------------ 1. the contract
def _table():
    """47 rows (not a multiple of a block's 4 waves) of 0, 1, 8..40, 65, 130 and 600 keys in two hours; two rows share
    video id 9; one row has +-inf keys; rows 34 and 30 (40 and 36 keys) are the ones the queries are made from."""
    rng = np.random.default_rng(1212)
    lens = [0, 1] + list(range(8, 41)) + [65, 130, 600] + [12, 20, 25, 30, 33, 36, 40, 17, 9]
    assert len(lens) == 47 and len(lens) % 4
    rows = []
    for i, n in enumerate(lens):
        rows.append((100 + i, np.sort(rng.uniform(0.0, 7200.0, size=n)).tolist()))
    rows[5] = (9, rows[5][1])
    rows[41] = (9, rows[41][1])
    rows[7] = (rows[7][0], rows[7][1] + [INF, -INF])
    return rows


def _queries(rows):
    base, other = np.asarray(rows[34][1]), np.asarray(rows[30][1])             # 40 and 36 keys
    assert len(base) == 40 and len(other) == 36
    scaled = ((base - 12.3) / 0.96).tolist()                                   # stored = 0.96 x + 12.3
    plain = (base - 12.3).tolist()
    excerpt = ((other[10:22] + 7.7) / 0.96).tolist()                           # 12 cuts of a scaled row
    special = [INF, -INF, 50.0, 50.0, 50.0, 1234.5, 1234.5, NAN, float(base[3])]
    return [scaled, plain, excerpt, [], [NAN] * 5, special]


@pytest.fixture(scope="module")
def world():
    rows = _table()
    queries = _queries(rows)
    cache = {}

    def aligned(rates, B):
        if (rates, B) not in cache:
            cache[rates, B] = [arr.align_rates_ref(rows, q, EPS, B * EPS, rates) for q in queries]
        return cache[rates, B]
    return rows, queries, aligned


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("rates", RATE_SETS, ids=("r1", "r2", "r8"))
def test_contract(dc, world, rates, B):
    rows, queries, aligned = world
    dc.upload(rows)
    mo = B * EPS
    assert awr.n_bins(EPS, mo) == B
    a = aligned(rates, B)
    excl = [rows[34][0], -1, rows[30][0], -1, -1, 9]
    for contain in (False, True):
        for k in KS:
            exp = _check(dc, rows, queries, EPS, mo, rates, k, aligned=a, contain=contain)
            _check(dc, rows, queries, EPS, mo, rates, k, aligned=a, contain=contain, min_votes=5)
        _check(dc, rows, queries, EPS, mo, rates, 16, aligned=a, contain=contain, exclude_ids=excl, min_score=atr.ONE // 8)
        assert exp[3, 64].tolist() == exp[4, 64].tolist() == [-1, 0, 0, 0, 0]      # the empty and the NaN-only query
    # the premises: the scaled copy is found at 0.96 where the list has it, the unscaled one at 1.0
    exp = arr.topk_rates_ref(rows, queries, EPS, mo, rates, 16, aligned=a)
    shift = round(12.3 / EPS)
    if 0.96 in rates:
        assert exp[0, 0].tolist() == [rows[34][0], 40, shift, 40, rates.index(0.96)]
        contained = arr.topk_rates_ref(rows, queries, EPS, mo, rates, 16, aligned=a, contain=True, min_votes=5)
        assert contained[2, 0].tolist() == [rows[30][0], 36, round(-7.7 / EPS), 12, rates.index(0.96)]
    else:
        assert exp[0, 0, 3] < 10
    assert exp[1, 0].tolist() == [rows[34][0], 40, shift, 40, rates.index(1.0)]
    # the Python call: rows and totals of the same blocks
    if B == MAX_B:
        got_rows, got_totals = dc.align_rates_topk(queries, eps=EPS, rates=rates, k=16)
        assert got_rows.dtype == got_totals.dtype == np.int32 and got_rows.shape == (6, 16, 5)
        _expect_blocks(got_rows, exp[:, :16], "rows of the Python call")
        assert got_totals.tolist() == exp[:, 16, 1].tolist()
        live = [r for r in exp[0, :16].tolist() if r[0] >= 0]
        assert len(live) > 1 and live == sorted(live, key=lambda r: tc.align_rates_order_key(r, 40))


def test_a_table_smaller_than_a_block(dc, world):
    rows, queries, _ = world
    few = [rows[34], rows[30], rows[7]]
    dc.upload(few)
    for B in BS:
        _check(dc, few, queries, EPS, B * EPS, RATE_SETS[2], 16)
        _check(dc, few, queries, EPS, B * EPS, RATE_SETS[1], 1, contain=True)
    dc.clear()
    exp = _check(dc, [], queries, EPS, 30.0, RATE_SETS[1], 4)
    assert (exp[:, 4, 1] == 0).all()


# ---------------------------------------------------------------------------------- 2. one rate of 1.0: the wide call
@pytest.mark.parametrize("case", ar.edge_cases(), ids=lambda c: c[0])
def test_rate_one_equals_the_wide_call_bit_for_bit(dc, case):
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
                wide = torch.full((Q, k + 1, 4), SENTINEL, dtype=torch.int32, device=DEV)
                need = tc.align_wide_topk_workspace_bytes(Q, L, d_q.numel(), k)
                ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
                s = torch.cuda.current_stream(DEV)
                rc_w = lib.tvz_align_wide_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), Q, L, float(eps), float(mo), 1, 0,
                                               flags, None, k, wide.data_ptr(), ws.data_ptr(), need, s.cuda_stream)
                rc_r, rated = _raw(dc, queries, eps, mo, (1.0,), k, flags=flags)
                assert rc_w == rc_r == 0, lib.tvz_last_error()
                assert torch.equal(rated[:, :, :4], wide), (name, eps, mo, k, flags)
                assert (rated[:, :, 4] == 0).all()
    assert (rated[:, -1, 1] >= 0).all()


# -------------------------------------------------------------------------------------------------- 3. rate choice
def test_rate_choice(dc):
    eps = 1 / 64
    q = [100.0 + 3 * i for i in range(8)]
    rows = [(1, [x * 0.5 + 10.0 for x in q]),                                      # all 8 at rate 0.5
            (2, [x + 20.0 for x in q]),                                            # all 8 at rate 1.0
            (3, [q[0] + 5.0]),                                                     # one vote at any rate: a tie
            (4, [x + 20.0 for x in q[:4]] + [x * 0.5 + 10.0 for x in q[:5]])]      # 4 at rate 1.0, 5 at rate 0.5
    dc.upload(rows)
    mo = MAX_B * eps
    exp = _check(dc, rows, [q], eps, mo, (1.0, 0.5, 0.5), 16)
    got = {r[0]: r.tolist() for r in exp[0, :16] if r[0] >= 0}
    assert got[1] == [1, 8, 640, 8, 1]                                             # the repeated rate: its first index
    assert got[2] == [2, 8, 1280, 8, 0]
    assert got[3][3:] == [1, 0]                                                    # a later rate that ties: the earlier
    assert got[4][:2] + got[4][3:] == [4, 9, 5, 1]                                 # a later rate with one more vote
    exp = _check(dc, rows, [q], eps, mo, (0.5, 1.0), 16)
    got = {r[0]: r.tolist() for r in exp[0, :16] if r[0] >= 0}
    assert got[1][4] == 0 and got[2][4] == 1 and got[3][4] == 0 and got[4][3:] == [5, 0]
    exp = _check(dc, rows, [q], eps, mo, (1.0,) * 8, 16)
    assert (exp[0, :, 4] == 0).all()


# ------------------------------------------------------------------- 4. resume positions do not leak between rates
def test_resume_positions_are_one_rates(dc):
    """B = 2^22, windows of 1,024 bins.  The query lies in [4000, 4120] s, the rows in [6000, 6120] s: at rate 1.0 the
    offsets are 1,880..2,120 s = bins 56,400..63,600, at rate 0.5 they are 3,940..4,120 s = bins 118,200..123,600 -
    disjoint window ranges of several windows each, walked in both orders.  The 130-key row is inside the 512 kept
    resume positions, the 600-key row past them."""
    rng = np.random.default_rng(77)
    q = np.sort(rng.uniform(4000.0, 4120.0, size=130))
    row130 = (q + 2000.0).tolist()                                                 # the query at rate 1.0
    row600 = np.sort(np.concatenate([q * 0.5 + 4000.0, rng.uniform(6000.0, 6120.0, size=470)])).tolist()
    rows = [(1, row130), (2, row600), (3, np.sort(rng.uniform(6000.0, 6120.0, size=130)).tolist()),
            (4, np.sort(rng.uniform(6000.0, 6120.0, size=600)).tolist()), (5, row600[:513])]
    assert (max(row600) - min(row600)) / EPS >= 3 * 1024
    dc.upload(rows)
    mo = MAX_B * EPS
    for rates in ((1.0, 0.5), (0.5, 1.0), (1.0, 0.5, 1.0, 0.5)):
        aligned = [arr.align_rates_ref(rows, q.tolist(), EPS, mo, rates)]
        # (query values closer than eps / 2 vote for each other's keys too: at least 130)
        assert aligned[0][0, :3].tolist() == [1, 130, 60000] and aligned[0][0, 3] >= 130 and aligned[0][0, 4] == rates.index(1.0)
        assert aligned[0][1, 2] == 120000 and aligned[0][1, 3] >= 130 and aligned[0][1, 4] == rates.index(0.5)
        for contain in (False, True):
            _check(dc, rows, [q.tolist()], EPS, mo, rates, 16, aligned=aligned, contain=contain)


# ------------------------------------------------------------------------------------------- 5. no fused multiply
def test_the_product_is_rounded_before_the_subtraction(dc):
    c, x, rho, eps, j = arr.no_fma_case()
    rows = [(1, [c])]
    dc.upload(rows)
    for mo in (100.0, MAX_B * eps):                                                # one window, and the window walk
        exp = _check(dc, rows, [[x]], eps, mo, (rho,), 4)
        assert exp[0, 0].tolist() == [1, 1, j, 1, 0]
        exp = _check(dc, rows, [[x]], eps, mo, (rho, 1.0), 4)                      # (rate 1.0 votes once too: the tie)
        assert exp[0, 0].tolist() == [1, 1, j, 1, 0]


# --------------------------------------------------------------------------------------- 6. refusals write nothing
def test_refusals_write_nothing(dc):
    rows = [(1, [100.0, 101.0]), (2, [105.0])]
    dc.upload(rows)
    q = [[100.0, 101.0]]
    need = tc.align_rates_topk_workspace_bytes(1, 2, 2, 16)
    out_bytes = 17 * 5 * 4
    arena = torch.full((256 + out_bytes + 256 + need + 512,), CANARY, dtype=torch.uint8, device=DEV)
    base = arena.data_ptr()
    o0 = (-base) % 256 + 256                                                        # d_out and the workspace inside it
    out = arena[o0:o0 + out_bytes].view(torch.int32).view(1, 17, 5)
    w0 = o0 + out_bytes + 256
    ws = arena[w0:w0 + need + 256]
    good = (1.0, 0.96)

    def call(eps=EPS, mo=1.0, k=16, rates=good, **kw):
        kw.setdefault("ws_bytes", need)
        return _raw(dc, q, eps, mo, rates, k, out=out, ws=ws, **kw)[0]

    assert call(rates=()) == ERR_UNSUPPORTED and call(rates=(1.0,) * 9) == ERR_UNSUPPORTED
    assert b"TVZ_ALIGN_MAX_RATES" in _lib.load().tvz_last_error()
    assert call(rates=None, n_rates=1) == ERR_INVALID
    for bad in (NAN, INF, 0.0, -1.0):
        assert call(rates=(1.0, bad)) == ERR_INVALID, bad
    assert call(flags=2) == ERR_INVALID and call(flags=0x80000001) == ERR_INVALID
    assert call(k=0) == ERR_UNSUPPORTED and call(k=65) == ERR_UNSUPPORTED
    assert call(max_query_len=4096) == ERR_UNSUPPORTED
    assert call(mo=(MAX_B + 1) * EPS) == ERR_UNSUPPORTED
    assert b"TVZ_ALIGN_WIDE_MAX_B" in _lib.load().tvz_last_error()
    assert call(mo=INF) == ERR_UNSUPPORTED
    assert call(eps=0.0) == ERR_INVALID and call(min_votes=0) == ERR_INVALID and call(min_score=-1) == ERR_INVALID
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE
    assert b"1 bytes missing" in _lib.load().tvz_last_error()
    torch.cuda.synchronize()
    assert (arena == CANARY).all()
    # right next to the refused ones: the widest range and eight rates, with a workspace of exactly the reported size -
    # everything around the block and behind the workspace stays as it was
    assert call(mo=MAX_B * EPS, rates=RATE_SETS[2]) == 0
    torch.cuda.synchronize()
    assert (arena[:o0] == CANARY).all() and (arena[o0 + out_bytes:w0] == CANARY).all() and (arena[w0 + need:] == CANARY).all()
    _expect_blocks(out.cpu().numpy(), arr.topk_rates_ref(rows, q, EPS, MAX_B * EPS, RATE_SETS[2], 16), "after the refusals")


# ------------------------------------------------------------------------------------------ 7. the merge and _shards
def _merge(blocks, queries, flags=0):
    blocks = np.ascontiguousarray(blocks, dtype=np.int32)
    R, Q, k1, _ = blocks.shape
    d_b = torch.from_numpy(blocks).to(DEV)
    d_q, d_off, _ = tc.pack_queries(queries, DEV)
    rows = torch.full((Q, k1 - 1, 5), POISON, dtype=torch.int32, device=DEV)
    totals = torch.full((Q,), POISON, dtype=torch.int32, device=DEV)
    rc = _lib.load().tvz_align_rates_topk_merge(d_b.data_ptr(), R, Q, k1 - 1, flags, d_q.data_ptr(), d_off.data_ptr(),
                                                rows.data_ptr(), totals.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, rows.cpu().numpy().astype(np.int64), totals.cpu().numpy().astype(np.int64)


def _check_merge(blocks, queries, contain=False):
    rc, rows, totals = _merge(blocks, queries, tc.ALIGN_CONTAIN if contain else 0)
    assert rc == 0, _lib.load().tvz_last_error()
    exp_rows, exp_totals = arr.merge_ref(blocks, queries, contain)
    assert (totals == exp_totals).all(), (totals, exp_totals)
    assert (rows == exp_rows).all(), [(q, rows[q].tolist(), exp_rows[q].tolist()) for q in range(len(queries))
                                      if not (rows[q] == exp_rows[q]).all()][:1]
    return rows, totals


QUERIES4 = [[float(i) for i in range(10)], [float(i) if i % 2 else NAN for i in range(20)], [], [NAN] * 7]


@pytest.mark.parametrize("contain", [False, True])
@pytest.mark.parametrize("n_lists,k", [(1, 1), (3, 5), (16, 64), (7, 16)])
def test_merge_of_hand_made_blocks(n_lists, k, contain):
    rng = np.random.default_rng(1000 * n_lists + k)
    nv = [atr.n_valid(q) for q in QUERIES4]
    lists = []
    for r in range(n_lists):
        per_q = []
        for qi in range(len(QUERIES4)):
            n = int(rng.integers(0, k + 3))
            hits = [(int(rng.integers(0, 12)), int(rng.integers(1, 12)), int(rng.integers(-MAX_B, MAX_B + 1)),
                     int(rng.integers(1, 14)), int(rng.integers(0, 8))) for _ in range(n)]
            # rows equal in five fields and differing in the rate, here and in the next list
            hits += [(0, 10, -70000, 10, (r + i) % 8) for i in range(3)]
            per_q.append(hits)
        lists.append(per_q)
    blocks = np.stack([np.stack([arr.merge_block_of(lists[r][q], nv[q], k, contain) for q in range(len(QUERIES4))])
                       for r in range(n_lists)])
    rows, totals = _check_merge(blocks, QUERIES4, contain)
    if contain:
        assert (rows[3, :, 0] == -1).all()                                         # nv = 0: u = 0 under containment
    if k >= 5:                                                                     # (nv = 10: they score 2^20)
        same = [r.tolist() for r in rows[0] if r[:4].tolist() == [0, 10, -70000, 10]]
        assert len(same) >= 2 and [r[4] for r in same] == sorted(r[4] for r in same)
    # padding in the middle of a list: a row with video_id < 0 is padding wherever it stands
    if k >= 5:
        holes = blocks.copy()
        holes[:, :, 1] = (-1, 0, 0, 0, 0)
        holes[0, 0, 3] = (-5, 9, 9, 9, 9)
        _check_merge(holes, QUERIES4, contain)


def test_a_refused_list_refuses_the_query_and_totals_saturate():
    nv = atr.n_valid(QUERIES4[0])
    mk = lambda rows, n: arr.merge_block_of(rows, nv, 4, n_hits=n)                   # noqa: E731
    a = [(1, 5, 100, 5, 2), (2, 5, -100, 4, 0)]
    blocks = np.stack([np.stack([mk(a, INT32_MAX - 1), mk(a, 2)]), np.stack([mk(a[:1], 7), mk(a, INT32_MIN)]),
                       np.stack([mk([], 0), mk(a, 1)])])
    rows, totals = _check_merge(blocks, [QUERIES4[0], QUERIES4[0]])
    assert totals.tolist() == [INT32_MAX, INT32_MIN] and (rows[1, :, 0] == -1).all() and (rows[1, :, 1:] == 0).all()
    assert rows[0, :3].tolist() == [[1, 5, 100, 5, 2], [1, 5, 100, 5, 2], [2, 5, -100, 4, 0]]
    # limits: as the wide merge
    lib = _lib.load()
    d_b = torch.from_numpy(np.ascontiguousarray(blocks, dtype=np.int32)).to(DEV)
    d_q, d_off, _ = tc.pack_queries([QUERIES4[0]] * 2, DEV)
    out = torch.full((2, 4, 5), POISON, dtype=torch.int32, device=DEV)
    tot = torch.full((2,), POISON, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for n_lists, k, flags, off, want in ((0, 4, 0, 0, ERR_UNSUPPORTED), (17, 4, 0, 0, ERR_UNSUPPORTED), (3, 0, 0, 0, ERR_UNSUPPORTED),
                                         (3, 65, 0, 0, ERR_UNSUPPORTED), (3, 4, 2, 0, ERR_INVALID), (3, 4, 0, 4, ERR_INVALID)):
        rc = lib.tvz_align_rates_topk_merge(d_b.data_ptr() + off, n_lists, 2, k, flags, d_q.data_ptr(), d_off.data_ptr(),
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
    rates = RATE_SETS[2]
    dc.upload(rows)
    shards = _upload_split(rows, R)
    try:
        d_q, d_off, longest = tc.pack_queries(queries, DEV)
        for k, contain, B in ((1, False, MAX_B), (16, True, MAX_B), (64, False, 5000)):
            mo = B * EPS
            ref = arr.topk_rates_ref(rows, queries, EPS, mo, rates, k, aligned=aligned(rates, B), contain=contain)
            one_rows, one_totals = dc.align_rates_topk(queries, eps=EPS, rates=rates, max_offset=mo, k=k, contain=contain)
            ws = torch.empty(tc.align_rates_topk_workspace_bytes(len(queries), longest, d_q.numel(), k), dtype=torch.uint8,
                             device=DEV)
            blocks, got_rows, got_totals = tc.align_rates_topk_shards(shards, d_q, d_off, longest, eps=EPS, rates=rates,
                                                                      max_offset=mo, k=k, workspace=ws, contain=contain)
            torch.cuda.synchronize()
            assert blocks.shape == (R, len(queries), k + 1, 5)
            got_rows, got_totals = got_rows.cpu().numpy(), got_totals.cpu().numpy()
            assert (got_rows == one_rows).all() and (got_totals == one_totals).all(), (R, k)
            assert (got_rows == ref[:, :k]).all() and (got_totals == ref[:, k, 1]).all(), (R, k)
            # the merge on its own, through the Python wrapper, over the blocks the call left
            m_rows, m_totals = tc.align_rates_topk_merge(blocks, k, d_q, d_off, contain=contain)
            assert torch.equal(m_rows.cpu(), torch.from_numpy(got_rows)) and (m_totals.cpu().numpy() == got_totals).all()
        # a refusal of the rate list comes before anything is written
        handles = (C.c_void_p * R)(*[s._h for s in shards])
        blocks = torch.full((R, len(queries), 5, 5), POISON, dtype=torch.int32, device=DEV)
        h = (C.c_double * 2)(1.0, -2.0)
        rc = _lib.load().tvz_align_rates_topk_shards(handles, R, d_q.data_ptr(), d_off.data_ptr(), len(queries), longest, EPS,
                                                     30.0, h, 2, 1, 0, 0, None, 4, blocks.data_ptr(), blocks.data_ptr(),
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
        for kw in ({"k": 8}, {"k": 3, "contain": True, "min_votes": 5}, {"k": 64, "exclude_ids": [rows[34][0], -1, -1, -1, -1, 9]}):
            k = kw["k"]
            ref = arr.topk_rates_ref(rows, queries, EPS, MAX_B * EPS, rates, aligned=aligned(rates, MAX_B), **kw)
            got = sc.align_rates_topk(queries, eps=EPS, rates=rates, **kw)
            assert got[0].dtype == np.int32 and got[0].shape == (len(queries), k, 5)
            assert (got[0] == ref[:, :k]).all() and (got[1] == ref[:, k, 1]).all(), kw
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------- 8. the inspector
def test_inspector_near_rates(tmp_path):
    """A stored 40-cut video on a 24 fps grid, an upload that is the same film at 25 fps behind 12.3 s of something
    else - its cuts are the stored ones x 25/24 + 12.3, so stored = 0.96 x upload - 11.808 - and an unscaled copy
    50.01 s later."""
    from tests.fakes import CutReader, cut_inspector
    from tvidz_amd import db as tdb

    rng = np.random.default_rng(24)
    stored = (np.sort(rng.choice(np.arange(24, 24 * 300), size=40, replace=False)) / 24.0).tolist()
    cuts = {"a.y4m": stored, "fast.y4m": [x * 25 / 24 + 12.3 for x in stored], "late.y4m": [x + 50.01 for x in stored]}
    res = {}
    for rated in (False, True):
        store = tdb.Store(f"sqlite:///{tmp_path}/{int(rated)}.db", corpus=tc.DeviceCorpus(0))
        kw = dict(near_rates=(1.0, 0.96)) if rated else {}
        ins = cut_inspector(store, device=DEV, near_duplicates=True, near_top_k=8, near_any_offset=True, **kw,
                            frame_source=lambda bucket, key, filename, uid: (CutReader(cuts[key], frames=9000), None))
        try:
            res[rated] = [ins.analyze_file("videos", k) for k in ("a.y4m", "fast.y4m", "late.y4m")]
        finally:
            store.close()
        assert all(r["status"] == "done" for r in res[rated]), res[rated]
    assert res[False][1]["near_duplicates"] == []                                   # invisible at one speed
    (near,) = res[True][1]["near_duplicates"]
    assert near["filename"] == "a.y4m" and near["rate"] == 0.96 and near["jaccard"] >= 0.95
    assert abs(near["shift_seconds"] - (-12.3 * 0.96)) <= EPS
    (late,) = res[True][2]["near_duplicates"]
    assert late["filename"] == "a.y4m" and late["rate"] == 1.0 and late["jaccard"] == 1.0
    assert abs(late["shift_seconds"] - (-50.01)) <= EPS
    (plain,) = res[False][2]["near_duplicates"]
    assert "rate" not in plain and {k: v for k, v in late.items() if k != "rate"} == plain
    assert [r["duplicates"] for r in res[False]] == [r["duplicates"] for r in res[True]]
