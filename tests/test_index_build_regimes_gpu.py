"""The build regimes of the inverted index that no other test reaches (tests/index_build_cases.py): directory slices of
64 and 128 KB, the step down to load <= 0.5, entries of 144 bytes (57 sub-indexes) in slices of 73,728 bytes, and the
unpartitioned build - count, offsets and fill over the whole directory - for keys and for cell postings.  Every test
first asserts the layout the build made (tvz_corpus_index_layout) against the restated sizing, so a run that took
another path fails there; answers are compared bit for bit with the oracle's restatement of db.find_duplicates
(inspector/db.py:76-94), tolerant answers with the contract restated in numpy, and the sweep with the index.

Device memory.  One handle at a time (the fixture closes it).  A classic directory keeps a shadow generation with room
to double once, an unpartitioned build also 4 bytes of fill cursors per entry and pair of sub-indexes, pre-sized to
double as well:
  slice64k 0.8 GB, slice128k / slice128k_half_load 1.6 GB, wide_partitioned 0.9 GB (directory + shadow);
  wide_unpartitioned, first build: 1.2 GB directory (2^23 x 144 B) + 2.4 GB shadow + 2.1 GB cursors = 5.8 GB;
  wide_unpartitioned, rebuilt at 2^24: 2.4 GB + 4.8 GB shadow + 4.3 GB cursors = 11.5 GB, and 15.1 GB in the test of
  the cell postings, whose unpartitioned cell directory of 2^23 entries adds 1.2 GB + 2.4 GB."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import index_build_cases as cases
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP, K = cases.HIT_CAP, cases.K
NEVER = tc.KTH_NEVER
NAMES = list(cases.SHAPES)
_EXPECTED = {}                         # (corpus state, query, min_match) -> the oracle's sorted triples


@pytest.fixture()
def dc():
    c = tc.DeviceCorpus(0)
    yield c
    c.close()


def _expected(state, c, qs, mm):
    """sorted (video_id, count, kth) per query; `state` names the corpus `c` (a shape, or a shape after its edits)"""
    out = []
    for qi, q in enumerate(qs):
        key = (state, qi, mm)
        if key not in _EXPECTED:
            cnt, kth = oracle.match_kth_csr(q, c.offs, c.keys, mm, sorted_unique=True)
            r = np.flatnonzero(cnt >= mm)
            _EXPECTED[key] = sorted(zip(c.ids[r].tolist(), cnt[r].tolist(), kth[r].tolist()))
        out.append(_EXPECTED[key])
    return out


def _layout(dc, cells=False):
    lay = dc.index_layout()
    pre = "cell_" if cells else ""
    return cases.Layout(*(lay[pre + f] for f in cases.Layout._fields))


def _check(dc, state, c, qs, mms, single=(), what=""):
    """tvz_match through the index and through the sweep, tvz_match_topk and (for the queries `single`)
    tvz_find_duplicates against the oracle, for every min_match of `mms`."""
    d_q, d_off, max_len = tc.pack_queries(qs, DEV)
    for mm in mms:
        exp = _expected(state, c, qs, mm)
        assert max(len(e) for e in exp) <= CAP
        for algo in (_lib.ALGO_INDEX, _lib.ALGO_TILE):
            hits, n = dc.match(d_q, d_off, max_len, mm, CAP, algo=algo)
            torch.cuda.synchronize()
            hits, n = hits.cpu().numpy(), n.cpu().numpy()
            for qi in range(len(qs)):
                assert int(n[qi]) == len(exp[qi]), (what, mm, algo, qi, int(n[qi]), len(exp[qi]))
                got = sorted(map(tuple, hits[qi, :int(n[qi])].tolist()))
                assert got == exp[qi], (what, mm, algo, qi)
        out = dc.match_topk(d_q, d_off, max_len, mm, CAP, K, algo=_lib.ALGO_INDEX)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        for qi in range(len(qs)):
            best = sorted(exp[qi], key=lambda h: (h[2], h[0], h[1]))[:K]
            best += [(-1, 0, NEVER)] * (K - len(best))
            assert list(map(tuple, out[qi, :K].tolist())) == best, (what, "topk", mm, qi)
            assert tuple(out[qi, K].tolist()) == (-1, len(exp[qi]), NEVER), (what, "topk total", mm, qi)
        if mm == 2:
            for qi in single:
                assert dc.find_duplicates(qs[qi], 2, with_kth=True) == exp[qi], (what, "single", qi)


def _assert_stats(dc, c, builds=None):
    live, distinct = cases.counts(c)
    st = dc.index_stats()
    assert st["indexed_rows"] == c.ids.size and st["delta_rows"] == 0, st
    assert st["postings"] == live and st["distinct_keys"] == distinct, (st, live, distinct)
    if builds is not None:
        assert st["builds"] == builds, st


def test_layout_query_on_small_handles(dc):
    """Zeros without an index and for the bucket directory of a one-sub-index handle; a small classic directory:
    slices of 32 KB, fewer than the partition kernels hold - the regime of the other index tests."""
    zeros = dict.fromkeys(dc.index_layout(), 0)
    assert len(zeros) == 8 and dc.index_layout() == zeros
    c = cases.corpus("slice64k")
    dc.upload_csr(c.ids[:300], c.offs[:301], c.keys[:c.offs[300]])
    assert dc.bucket_stats()["buckets"] > 0 and dc.index_layout() == zeros
    dc.set_tol_index(0.001)
    assert dc.tol_index_stats()["cells"] > 0 and dc.index_layout() == zeros       # as the header says: all of it
    dc.set_tol_index(0.0)
    n = cases.SUB_ROWS + 5
    ids, offs = c.ids[:n], np.arange(n + 1, dtype=np.int64) * 2
    keys = np.repeat(cases.OWN_BASE + np.arange(n) % 5000, 2) + np.tile([0.0, 0.5], n)
    dc.upload_csr(ids, offs, keys)
    want = cases.layout(n, 2 * n, 10000)
    assert want == cases.Layout(32, 16, 10, 1) and _layout(dc) == want and _layout(dc, cells=True) == (0, 0, 0, 0)
    dc.clear()
    assert dc.index_layout() == zeros


@pytest.mark.parametrize("name", NAMES)
def test_build_regime(dc, name):
    s, c, qs = cases.SHAPES[name], cases.corpus(name), cases.queries(name)
    live, distinct = cases.counts(c)
    # 1. first build: sized from the key count, doubled while crowded, once more at the size the count revealed
    dc.upload_csr(c.ids, c.offs, c.keys)
    first = cases.layout(s.rows, live, distinct)
    print(name, "first build:", dc.index_layout())
    assert first == s.first and _layout(dc) == first, (dc.index_layout(), first)
    assert _layout(dc, cells=True) == (0, 0, 0, 0)
    _assert_stats(dc, c, builds=1)
    # 2. parity: the M2 mode (min_match 1, 2), the five-position mode (3), the count-only mode with the kth fix-up (6)
    mms = (1, 2, 3, 6) if name in cases.TWO_SUB else (1, 2, 6)
    _check(dc, name, c, qs, mms, single=(0, 3), what="first build")
    # 3. the rebuild sized from the last build's counts
    dc.build_index()
    rebuilt = cases.layout(s.rows, live, distinct, hint=(live, distinct))
    print(name, "hinted rebuild:", dc.index_layout())
    assert rebuilt == s.rebuilt and _layout(dc) == rebuilt, (dc.index_layout(), rebuilt)
    _assert_stats(dc, c, builds=2)
    _check(dc, name, c, qs, (2,), single=(1,), what="hinted rebuild")
    if name not in cases.MUTATED:
        return
    # 4. mutations: stale postings in the directory's entries + the delta sweep ...
    replaced, appended = cases.mutations(name)
    for r, k in replaced.items():
        dc.upsert(int(c.ids[r]), k)
    for vid, k in appended:
        dc.upsert(vid, k)
    e = cases.edit(c, replaced, appended)
    st = dc.index_stats()
    assert st["delta_rows"] == len(replaced) + len(appended) and st["builds"] == 2 and st["indexed_rows"] == s.rows, st
    _check(dc, name + "+edits", e, qs, (2,), single=(0,), what="edited")
    # ... then the background rebuild (from the snapshot table, on the build stream) that the delta table triggers
    trigger = cases.delta_trigger(s.rows)
    fill = []
    while dc.index_stats()["builds"] == 2 and len(fill) <= trigger:
        fill.append((s.rows + 100 + len(fill), cases.filler(len(fill))))
        dc.upsert(*fill[-1])
    f = cases.edit(e, {}, fill)
    st = dc.index_stats()
    assert st["builds"] == 3 and st["delta_rows"] < trigger <= len(replaced) + len(appended) + len(fill), (st, len(fill))
    live_f, distinct_f = cases.counts(f)
    again = cases.layout(f.ids.size, live_f, distinct_f, hint=(live, distinct))
    print(name, "background rebuild after", len(fill), "fillers:", dc.index_layout(), st)
    assert again == s.rebuilt and _layout(dc) == again, (dc.index_layout(), again)
    _assert_stats(dc, f, builds=3)
    _check(dc, name + "+edits+fill", f, qs, (2,), single=(2,), what="background rebuild")


def _tol_lists(dc, packed, tol, mm):
    d_q, d_off, max_len = packed
    hits, n = dc.match_tol(d_q, d_off, max_len, tol, mm, CAP)
    torch.cuda.synchronize()
    hits, n = hits.cpu().numpy(), n.cpu().numpy()
    assert int(n.max()) <= CAP
    return [sorted(map(tuple, hits[q, :int(n[q])].tolist())) for q in range(len(n))]


def _tol_blocks(dc, packed, tol, mm):
    d_q, d_off, max_len = packed
    out = dc.match_tol_topk(d_q, d_off, max_len, tol, mm, K)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", cases.WIDE)
def test_cell_postings_through_the_same_kernels(dc, name):
    """5. build_classic with cellw > 0: the cell directory of a 1 ms cell is guessed from the key directory's distinct
    count, so it is built in the same regime.  The tolerant calls through it, the sweep and the restated contract give
    the same lists; the top-k blocks are the k best of those lists."""
    s, c, qs = cases.SHAPES[name], cases.corpus(name), cases.tol_queries(name)
    live, distinct = cases.counts(c)
    tol, cell = 0.0005, 0.001
    pre = cases.tol_sorted(c)
    exp = {mm: [cases.tol_expected(c, q, tol, mm, pre) for q in qs] for mm in (1, 2)}
    assert all(len(e) <= CAP for mm in exp for e in exp[mm]) and len(exp[2][-1]) >= 1
    packed = tc.pack_queries(qs, DEV)
    dc.upload_csr(c.ids, c.offs, c.keys)
    assert _layout(dc) == s.first and dc.tol_index_stats()["cells"] == 0

    def answers(what):
        blocks = {}
        for mm in (1, 2):
            got = _tol_lists(dc, packed, tol, mm)
            for qi in range(len(qs)):
                assert got[qi] == exp[mm][qi], (what, mm, qi, len(got[qi]), len(exp[mm][qi]))
            blocks[mm] = _tol_blocks(dc, packed, tol, mm)
            for qi in range(len(qs)):
                best = sorted(exp[mm][qi], key=lambda h: (h[2], h[0], h[1]))[:K]
                assert list(map(tuple, blocks[mm][qi, :len(best)].tolist())) == best, (what, "topk", mm, qi)
                assert int(blocks[mm][qi, K, 1]) == len(exp[mm][qi]), (what, "topk total", mm, qi)
        return blocks

    swept = answers("sweep")
    dc.set_tol_index(cell)                                  # rebuilds: the keys from their hint, the cells from a guess
    posts, cells = cases.cell_counts(c, cell)
    print(name, "with cell postings:", dc.index_layout(), dc.tol_index_stats())
    assert _layout(dc) == s.rebuilt, dc.index_layout()
    want = cases.layout(s.rows, live, cells, guess=distinct)
    assert want == s.first and _layout(dc, cells=True) == want, (dc.index_layout(), want)
    st = dc.tol_index_stats()
    assert st["cell"] == cell and st["cells"] == cells and st["postings"] == posts and st["builds"] == 1, st
    _assert_stats(dc, c, builds=2)
    indexed = answers("cell postings")
    for mm in (1, 2):
        assert np.array_equal(swept[mm], indexed[mm]), mm
