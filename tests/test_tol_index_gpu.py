"""GPU parity of the tolerant match through cell postings (tvz_corpus_tol_index): every result of tvz_match_tol,
tvz_match_tol_topk and tvz_match_tol_sharded on a handle WITH cell postings equals the result of the same call on a
twin handle with the same corpus and none - top-k blocks as they are (they are ordered), hit lists as sorted triples
with equal counts (their order is unspecified) - over min_match 1, 2, 3, 5, tol in {0, cell / 4, cell} and one above
the cell (the fallback), k in {1, 16, 64}, with and without exclude ids; a sample also against the restatement of the
contract (tests/tol_ref.py); tol = 0 against tvz_match bit for bit.  Then the handle's life: upserts after the build,
a background rebuild crossed mid-test, clear, postings off and on, a handle grown by upserts past its first build."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import tol_ref
from tvidz_amd import corpus as tc, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN = int(np.iinfo(np.int32).min)
CELL = 0.001


class Twins:
    """Two handles with the same rows: `cells` carries cell postings of width `cell`, `plain` never hears of them."""

    def __init__(self, cell=CELL):
        self.plain, self.cells = tc.DeviceCorpus(0), tc.DeviceCorpus(0)
        self.cell = cell
        self.cells.set_tol_index(cell)

    def both(self, fn):
        for h in (self.plain, self.cells):
            fn(h)

    def close(self):
        self.both(lambda h: h.close())


@pytest.fixture()
def twins():
    t = Twins()
    yield t
    t.close()


def _pack(qs, excl):
    d_q, d_off, ml = tc.pack_queries(qs, DEV)
    d_ex = torch.tensor(excl, dtype=torch.int32, device=DEV) if excl is not None else None
    return d_q, d_off, ml, d_ex


def _lists(h, packed, tol, mm, cap):
    """tvz_match_tol -> per query (hits_n, sorted (video_id, count, kth) triples)."""
    d_q, d_off, ml, d_ex = packed
    hits, n = h.match_tol(d_q, d_off, ml, tol, mm, cap, d_exclude_ids=d_ex)
    torch.cuda.synchronize()
    hits, n = hits.cpu().numpy(), n.cpu().numpy()
    return [(int(n[q]), sorted(map(tuple, hits[q, :min(int(n[q]), cap)].tolist()))) for q in range(len(n))]


def _blocks(h, packed, tol, mm, k):
    d_q, d_off, ml, d_ex = packed
    out = h.match_tol_topk(d_q, d_off, ml, tol, mm, k, d_exclude_ids=d_ex)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_same(t, qs, excl, cap, tols, mms=(1, 2, 3, 5), ks=(1, 16, 64), what=""):
    """Both forms, every (tol, min_match, k, exclude) of the issue, identical between the twins.  Returns the cells
    handle's lists at the last tol for further checks."""
    last = None
    for ex in (None, excl):
        packed = _pack(qs, ex)
        for tol in tols:
            for mm in mms:
                a, b = _lists(t.plain, packed, tol, mm, cap), _lists(t.cells, packed, tol, mm, cap)
                assert all(n <= cap for n, _ in a), "cap too small for a complete comparison"
                assert a == b, (what, "list", tol, mm, ex is not None, [i for i in range(len(a)) if a[i] != b[i]][:4])
                last = b
                for k in ks:
                    x, y = _blocks(t.plain, packed, tol, mm, k), _blocks(t.cells, packed, tol, mm, k)
                    assert np.array_equal(x, y), (what, "topk", tol, mm, k, ex is not None)
                    # the block agrees with the list: the k best by (kth, video_id, count), the true total
                    for q in range(len(qs)):
                        n, trip = b[q]
                        best = sorted(trip, key=lambda e: (e[2], e[0], e[1]))[:k]
                        assert [tuple(r) for r in y[q, :len(best)].tolist()] == best and int(y[q, k, 1]) == n, (what, tol, mm, k, q)
    return last


def _special_rows():
    """Cells holding several keys of one row, negative keys, +-inf, keys at and far beyond +-2^40 cells."""
    inf = float("inf")
    far = 2.0 ** 40 * CELL
    return [
        (1, [5.0001, 5.0002, 5.0003, 5.00035, 9.0]),                 # four keys in one 1 ms cell
        (2, [-5.0001, -5.0002, -3.0, -0.0004, 0.0, 0.0004]),         # negative keys, a window straddling 0
        (3, [inf, 1.0, 2.0]), (4, [-inf, inf]), (5, [inf, far, far * 4, 1e300]),
        (6, [-far, -far * 3, -1e300, -inf]), (7, [far - CELL, far, far + CELL]),
        (8, [100.0, 100.0005, 100.001, 100.0015, 100.002]),          # a run across three cells
        (9, [5.0002, 9.0004, 100.0011]), (10, []), (11, [float("nan"), 7.0]),
        (12, [0.999, 1.0, 1.001, 1.9995, 2.0005]),
    ]


def _special_queries():
    inf = float("inf")
    far = 2.0 ** 40 * CELL
    return [
        [5.0002, 9.0003, 100.001], [-5.00015, -3.0005, -0.0002, 0.0002], [inf, 1.0004, 2.0], [-inf, inf, inf],
        [far, far * 4, 1e300, inf], [-far, -far * 3, -1e300], [far - CELL / 2, far + CELL / 2], [100.0007, 100.0007, 100.0018],
        [float("nan"), 7.0004, 5.00025], [], [1.0005, 1.9999, 0.9985], [5.0001, 5.0002, 5.0003, 5.00035, 9.0],
    ]


def test_special_rows_twins_and_the_restatement(twins):
    rows = _special_rows()
    twins.both(lambda h: h.upload(rows))
    assert twins.cells.tol_index_stats()["cell"] == CELL and twins.plain.tol_index_stats()["cell"] == 0.0
    qs = _special_queries()
    excl = [(i % 4) + 1 if i % 2 else -1 for i in range(len(qs))]
    tols = (0.0, CELL / 4, CELL, 2.5 * CELL)
    _assert_same(twins, qs, excl, cap=64, tols=tols, what="special")
    packed = _pack(qs, excl)
    for tol in tols:
        for mm in (1, 2, 3, 5):
            got = _lists(twins.cells, packed, tol, mm, 64)
            for q in range(len(qs)):
                exp = tol_ref.find_duplicates_tol(rows, qs[q], tol, mm, excl[q], form="brute")
                assert got[q] == (len(exp), exp), (tol, mm, q, got[q], exp)


def _corpus_queries(C_, mean_len, seed, Q):
    ids, offs, keys = synth.synth_timestamp_corpus(C_, seed=seed, mean_len=mean_len, dup_frac=0.02, frag_frac=0.02)
    rng = np.random.default_rng(seed + 1)
    qs, excl = [], []
    for t in range(Q):
        r = int(rng.integers(0, C_))
        q = keys[offs[r]:offs[r + 1]] + (0.0, 0.0004, -0.0003, 0.00025)[t % 4]
        if t % 5 == 4:
            q = np.concatenate([q[: max(2, len(q) // 3)], rng.choice(keys, size=25) + 0.0002])
        if t % 7 == 6:
            q = np.concatenate([q, q[:5]])                                 # repeated elements: multiplicity counts
        qs.append(q.tolist())
        excl.append(int(ids[r]) if t % 2 else -1)
    return ids, offs, keys, qs, excl


def test_small_corpus_every_form(twins):
    ids, offs, keys, qs, excl = _corpus_queries(3000, 60, 3, 24)
    twins.both(lambda h: h.upload_csr(ids, offs, keys))
    st = twins.cells.tol_index_stats()
    assert st["cells"] > 0 and 0 < st["postings"] <= len(keys) and st["builds"] >= 1 and st["delta_rows"] == 0
    assert twins.plain.tol_index_stats() == dict(cell=0.0, cells=0, postings=0, builds=0, delta_rows=0)
    got = _assert_same(twins, qs, excl, cap=3000, tols=(0.0, CELL / 4, CELL, 3 * CELL), what="small")
    assert sum(n for n, _ in got) > 0
    # a sample against the restatement, at tol = cell
    packed = _pack(qs, excl)
    for mm in (1, 2, 5):
        got = _lists(twins.cells, packed, CELL, mm, 3000)
        for q in (0, 1, 2, 3, 4, 6, 13):
            exp = tol_ref.find_duplicates_tol_csr(ids, offs, keys, qs[q], CELL, mm, excl[q])
            assert got[q] == (len(exp), exp), (mm, q)
    # tol = 0 equals tvz_match bit for bit (as sorted lists: either order is unspecified)
    d_q, d_off, ml, d_ex = packed
    for mm in (1, 2, 3, 5):
        hits, n = twins.cells.match(d_q, d_off, ml, mm, 3000, d_exclude_ids=d_ex)
        torch.cuda.synchronize()
        hits, n = hits.cpu().numpy(), n.cpu().numpy()
        exact = [(int(n[q]), sorted(map(tuple, hits[q, :int(n[q])].tolist()))) for q in range(len(qs))]
        assert _lists(twins.cells, packed, 0.0, mm, 3000) == exact, mm


def test_config3_size_twins_and_a_sample_of_the_restatement():
    C_ = 100_000
    ids, offs, keys, qs, excl = _corpus_queries(C_, 200, 3, 16)
    t = Twins()
    try:
        t.both(lambda h: h.upload_csr(ids, offs, keys))
        assert t.cells.index_stats()["indexed_rows"] == C_ and t.cells.tol_index_stats()["postings"] > 0
        got = _assert_same(t, qs, excl, cap=C_, tols=(0.0, CELL / 4, CELL, 3 * CELL), mms=(1, 2, 3, 5), ks=(1, 16, 64), what="config3")
        assert got is not None
        packed = _pack(qs, excl)
        for mm in (2, 5):
            lists = _lists(t.cells, packed, CELL, mm, C_)
            for q in (0, 1, 5):
                exp = tol_ref.find_duplicates_tol_csr(ids, offs, keys, qs[q], CELL, mm, excl[q])
                assert lists[q] == (len(exp), exp), (mm, q)
        d_q, d_off, ml, d_ex = packed
        for mm in (1, 2, 5):
            hits, n = t.cells.match(d_q, d_off, ml, mm, C_, d_exclude_ids=d_ex)
            torch.cuda.synchronize()
            hits, n = hits.cpu().numpy(), n.cpu().numpy()
            exact = [(int(n[q]), sorted(map(tuple, hits[q, :int(n[q])].tolist()))) for q in range(len(qs))]
            assert _lists(t.cells, packed, 0.0, mm, C_) == exact, mm
    finally:
        t.close()


# ---- blocks that walk several sub-indexes ------------------------------------------------------------------------------
# The launch gives a query about 1,024 / Q blocks.  On a handle of three sub-indexes (40,000 rows) that is, for
#   Q = 1,100: ONE block per query that walks all three sub-indexes, its candidates not split (the large ticks' shape);
#   Q =   512: two blocks per query, the first walks two sub-indexes, the second one;
#   Q =    24: three blocks per sub-index, each one sub-index (the shape of the other tests).
# What a block carries from one sub-index to the next - the cleared bitmaps, the ranks, the kept directory slots, the
# staged hits of the list form (more than the 256 the stage holds: the long queries), the waves' kept lists and
# thresholds of the top-k form - is only exercised by the first two.
@pytest.fixture(scope="module")
def three_subs():
    C_ = 40_000
    ids, offs, keys = synth.synth_timestamp_corpus(C_, seed=17, mean_len=30, dup_frac=0.02, frag_frac=0.02)
    t = Twins()
    t.both(lambda h: h.upload_csr(ids, offs, keys))
    assert t.cells.index_stats()["indexed_rows"] == C_ and (C_ + 16383) // 16384 == 3
    rng = np.random.default_rng(18)
    qs, excl = [], []
    for i in range(1100):
        r = int(rng.integers(0, C_))
        row = keys[offs[r]:offs[r + 1]]
        if i % 64 == 5:                                     # long: hundreds of hits at min_match 1, past one block's stage
            q = np.concatenate([row, rng.choice(keys, size=600)]) + 0.0002
        elif i % 3 == 0:
            q = row[:12] + (0.0004 if i % 2 else -0.0003)
        else:
            q = np.concatenate([row[:6], rng.choice(keys, size=6) + 0.0002])
        qs.append(q.tolist())
        excl.append(int(ids[r]) if i % 2 else -1)
    for h in (t.plain, t.cells):                            # and rows only the delta table knows
        h.upsert(int(ids[3]), qs[0][:9])
        h.upsert(910001, qs[5][:40])
    yield t, ids, offs, keys, qs, excl
    t.close()


@pytest.mark.parametrize("Q", [1100, 512])
def test_blocks_that_walk_several_sub_indexes(three_subs, Q):
    t, ids, offs, keys, qs, excl = three_subs
    qs, excl = qs[:Q], excl[:Q]
    cap = 4096
    packed = _pack(qs, excl)
    rows_now = {int(ids[c]): keys[offs[c]:offs[c + 1]] for c in range(len(ids))}
    rows_now[int(ids[3])] = qs[0][:9]
    rows_now[910001] = qs[5][:40]
    rows_now = list(rows_now.items())
    for tol in (CELL / 4, CELL):
        for mm in (1, 2, 5):
            a, b = _lists(t.plain, packed, tol, mm, cap), _lists(t.cells, packed, tol, mm, cap)
            assert all(n <= cap for n, _ in a)
            assert a == b, ("list", Q, tol, mm, [i for i in range(Q) if a[i] != b[i]][:4])
            if mm == 1:
                assert max(n for n, _ in b) > 256                          # a block's stage overflowed across sub-indexes
            for k in (16, 64):
                x, y = _blocks(t.plain, packed, tol, mm, k), _blocks(t.cells, packed, tol, mm, k)
                assert np.array_equal(x, y), ("topk", Q, tol, mm, k)
                for q in range(0, Q, 37):
                    n, trip = b[q]
                    best = sorted(trip, key=lambda e: (e[2], e[0], e[1]))[:k]
                    assert [tuple(r) for r in y[q, :len(best)].tolist()] == best and int(y[q, k, 1]) == n, (Q, tol, mm, k, q)
            if tol == CELL:
                for q in (0, 5, 69, Q - 1):                                # 5 and 69 are long queries
                    exp = tol_ref.find_duplicates_tol(rows_now, qs[q], tol, mm, excl[q], form="sorted")
                    assert b[q] == (len(exp), exp), (Q, mm, q)
    # without exclude ids, and tol = 0 against the exact match
    packed = _pack(qs, None)
    for mm in (1, 2):
        assert _lists(t.plain, packed, CELL, mm, cap) == _lists(t.cells, packed, CELL, mm, cap), (Q, mm)
        d_q, d_off, ml, _ = packed
        hits, n = t.cells.match(d_q, d_off, ml, mm, cap)
        torch.cuda.synchronize()
        hits, n = hits.cpu().numpy(), n.cpu().numpy()
        exact = [(int(n[q]), sorted(map(tuple, hits[q, :int(n[q])].tolist()))) for q in range(Q)]
        assert _lists(t.cells, packed, 0.0, mm, cap) == exact, (Q, mm)


def test_long_queries_and_refusals_fall_back_or_flag_alike(twins):
    ids, offs, keys, qs, excl = _corpus_queries(2000, 40, 8, 6)
    twins.both(lambda h: h.upload_csr(ids, offs, keys))
    rng = np.random.default_rng(2)
    long_q = (rng.choice(keys, size=5000) + 0.0003).tolist()               # beyond the top-k form, inside the list form's LDS
    packed = _pack(qs + [long_q], None)
    for mm in (1, 2, 7):                                                   # 7: the list form's fix-up path (sweep on both)
        assert _lists(twins.plain, packed, CELL, mm, 2000) == _lists(twins.cells, packed, CELL, mm, 2000), mm
    # max_query_len that is no upper bound: the affected query is flagged on both, the others answered alike
    d_q, d_off, ml, _ = _pack(qs, None)
    short = max(2, min(len(q) for q in qs))
    for h_tol in (CELL, 0.0):
        res = []
        for h in (twins.plain, twins.cells):
            hits, n = h.match_tol(d_q, d_off, short, h_tol, 2, 2000)
            blk = h.match_tol_topk(d_q, d_off, short, h_tol, 2, 16)
            torch.cuda.synchronize()
            n = n.cpu().numpy()
            res.append((n.tolist(), [sorted(map(tuple, hits[q, :max(int(n[q]), 0)].cpu().tolist())) for q in range(len(qs))],
                        blk.cpu().tolist()))
        assert res[0] == res[1] and INT32_MIN in res[1][0]


def _rng_row(rng, keys, n):
    return (rng.choice(keys, size=n) + rng.choice([0.0, 0.0003, -0.0002], size=n)).tolist()


def test_life_cycle_against_the_twin():
    ids, offs, keys, qs, excl = _corpus_queries(6000, 50, 11, 20)
    t = Twins()
    try:
        t.both(lambda h: h.upload_csr(ids, offs, keys))
        tols, cap = (CELL / 4, CELL), 8000
        builds0 = t.cells.tol_index_stats()["builds"]
        # upserts after the build: replaced indexed rows show their NEW content once (from the delta), new rows appear
        rng = np.random.default_rng(12)
        new_rows = {}
        for i in range(40):
            vid = int(ids[int(rng.integers(0, 6000))]) if i % 2 else 700000 + i
            new_rows[vid] = qs[i % len(qs)][: 12 + i % 9] if i % 3 else _rng_row(rng, keys, 30)
            t.both(lambda h: h.upsert(vid, new_rows[vid]))
        st = t.cells.tol_index_stats()
        assert st["delta_rows"] == len(new_rows) and st["builds"] == builds0
        got = _assert_same(t, qs, excl, cap, tols, ks=(16,), what="upserts")
        rows_now = {int(ids[c]): keys[offs[c]:offs[c + 1]] for c in range(len(ids))}
        rows_now.update(new_rows)
        packed = _pack(qs, excl)
        lists = _lists(t.cells, packed, CELL, 2, cap)
        for q in (0, 3, 7):
            exp = tol_ref.find_duplicates_tol(list(rows_now.items()), qs[q], CELL, 2, excl[q], form="sorted")
            assert lists[q] == (len(exp), exp), q                          # each replaced row once, with its new content
            assert len({v for v, _, _ in lists[q][1]}) == len(lists[q][1])
        # a background rebuild crossed mid-test: the delta trigger is max(512, indexed / 256) rows
        n = 0
        while t.cells.tol_index_stats()["builds"] == builds0:
            vid = 800000 + n
            row = _rng_row(rng, keys, 20)
            new_rows[vid] = row
            t.both(lambda h: h.upsert(vid, row))
            n += 1
            assert n <= 2000, "no background rebuild within 2000 upserts"
        st = t.cells.tol_index_stats()
        assert st["builds"] == builds0 + 1 and st["cell"] == CELL and st["delta_rows"] < 100
        assert t.cells.index_stats()["indexed_rows"] > 6000
        _assert_same(t, qs, excl, cap, tols, ks=(1, 64), what="rebuilt")
        for i in range(5):                                                 # and upserts on top of the rebuilt generation
            t.both(lambda h: h.upsert(int(ids[i]), qs[i][:15]))
        _assert_same(t, qs, excl, cap, tols, mms=(2, 5), ks=(16,), what="rebuilt + upserts")
        # postings off: the next build drops them (same results, now by the sweep); on again: built at once
        t.cells.set_tol_index(0.0)
        assert t.cells.tol_index_stats()["cell"] == CELL                   # until the next build
        t.both(lambda h: h.build_index())
        st = t.cells.tol_index_stats()
        assert (st["cell"], st["cells"], st["postings"]) == (0.0, 0, 0) and st["builds"] == builds0 + 1
        _assert_same(t, qs, excl, cap, (CELL,), mms=(2,), ks=(16,), what="off")
        t.cells.set_tol_index(2 * CELL)
        st = t.cells.tol_index_stats()
        assert st["cell"] == 2 * CELL and st["builds"] == builds0 + 2 and st["postings"] > 0
        _assert_same(t, qs, excl, cap, (CELL, 2 * CELL, 3 * CELL), mms=(1, 3), ks=(16,), what="on again, wider")
        for bad in (float("nan"), float("inf"), -0.001, 2.0 ** -21, 1e-9):
            with pytest.raises(RuntimeError, match="cell must be"):
                t.cells.set_tol_index(bad)
        assert t.cells.tol_index_stats()["cell"] == 2 * CELL               # a refusal changes nothing
        # clear: nothing left on either, the stats say so; rows upserted afterwards are swept
        t.both(lambda h: h.clear())
        assert t.cells.tol_index_stats()["cells"] == 0
        packed = _pack(qs[:4], excl[:4])
        assert _lists(t.cells, packed, CELL, 1, 16) == [(0, [])] * 4
        t.both(lambda h: h.upsert(5, qs[0][:20]))
        _assert_same(t, qs[:4], excl[:4], 16, (CELL,), mms=(1, 2), ks=(16,), what="cleared")
    finally:
        t.close()


def test_a_handle_grown_by_upserts_past_its_first_index_build():
    t = Twins()
    try:
        rng = np.random.default_rng(31)
        grid = np.round(np.arange(1, 90000) / 30.0, 6)
        rows = []
        for v in range(4400):                                              # the first build comes at 4,096 rows
            row = rng.choice(grid, size=int(rng.integers(5, 30)), replace=False).tolist()
            rows.append((v + 1, row))
            t.both(lambda h: h.upsert(v + 1, row))
        st = t.cells.tol_index_stats()
        assert st["cell"] == CELL and st["builds"] >= 1 and st["postings"] > 0
        assert t.cells.index_stats()["indexed_rows"] >= 4096
        qs = [(np.asarray(rows[int(v)][1]) + 0.0004).tolist() for v in rng.integers(0, len(rows), 12)]
        excl = [rows[i][0] if i % 2 else -1 for i in range(12)]
        got = _assert_same(t, qs, excl, 4400, (0.0, CELL / 4, CELL), mms=(1, 2, 5), ks=(16,), what="grown")
        for q in (0, 1, 2):
            exp = tol_ref.find_duplicates_tol(rows, qs[q], CELL, 5, excl[q], form="sorted")
            assert got[q] == (len(exp), exp), q
    finally:
        t.close()


# ---- sharded -------------------------------------------------------------------------------------------------------
def test_match_tol_sharded_world_size_1_equals_the_twin_without_postings():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tol_index_comm_child.py")], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["stats"]["cell"] == CELL and res["stats"]["postings"] > 0 and res["stats"]["delta_rows"] == 2
    assert res["plain_stats"]["cell"] == 0.0
    assert len(res["equal"]) == 24 and all(res["equal"].values()), res["equal"]
    assert sum(res["hits"].values()) > 0


def test_one_tolerant_ask_through_a_rank_corpus_tick_with_cell_postings():
    from tvidz_amd import service, sharded
    ids, offs, keys = synth.synth_timestamp_corpus(5000, seed=41, mean_len=50)
    rows = [(int(ids[c]), keys[offs[c]:offs[c + 1]].tolist()) for c in range(len(ids))]
    shard = tc.DeviceCorpus(0)
    comm = sharded.make_comm(0)
    matcher = sharded.RcclShardedMatcher(shard, comm, k=64, cap=2048)
    rc = service.RankCorpus(shard, matcher, xdev="cuda:0", tick_s=0.001, tol_index_cell=CELL)   # --match-tol-index
    try:
        rc.upload(rows)
        st = shard.tol_index_stats()
        assert st["cell"] == CELL and st["postings"] > 0
        q = (np.asarray(rows[17][1]) + 0.0004).tolist()
        exp = tol_ref.find_duplicates_tol(rows, q, CELL, 2, -1, form="sorted")
        assert (rows[17][0], len(q), 1) in exp
        got = rc.find_duplicates(q, 2, with_kth=True, tolerance=CELL)
        assert got == exp
        assert rc.find_duplicates(q, 2, exclude_id=rows[17][0], with_kth=True, tolerance=CELL) == [e for e in exp if e[0] != rows[17][0]]
        assert rc.broken is None
    finally:
        rc.close()
        comm.close()
