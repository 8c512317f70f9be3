"""The top-k family of tvz_topk_kernels.h - ts_topk_select_kernel<1024 / 2048>, ts_topk_kernel, ts_topk_wave_kernel
(E = 4/8/16; the shard, merge and pair forms: modes 1, 2, 3 in the case tables), ts_topk_merge_sorted_kernel<1..16> -
at every size class, tie path and totals rule the dispatch in tvz_match.hip has, against tests/topk_ref.py (a Python sorted() and a sum).  The inputs are the hand-made
lists of tests/topk_cases.py, each in ascending, descending and shuffled order; every comparison is exact equality of
int32 rows and totals."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import topk_cases as cases, topk_ref as ref
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEVER = tc.KTH_NEVER
INT32_MAX, INT32_MIN = ref.INT32_MAX, ref.INT32_MIN


def _rows(a):
    """int32 [.., 3] -> list of int tuples."""
    return [tuple(r) for r in a.tolist()]


def _pack(lists, cap):
    """Lists of entries -> int32 [Q, cap, 3]; what lies behind a list is junk that looks like good hits."""
    out = np.empty((len(lists), cap, 3), dtype=np.int32)
    out[:] = (5, 1, 0)
    for q, lst in enumerate(lists):
        if lst:
            out[q, :len(lst)] = np.array(lst, dtype=np.int64).astype(np.int32)
    return out


# ---------------------------------------------------------------- a. tvz_topk_shard: the select kernels alone
@pytest.mark.parametrize("k", cases.SHARD_KS)
def test_topk_shard_on_hand_made_lists(k):
    cap = cases.SHARD_CAP
    names, lists, reported = cases.shard_batch(k)
    hits = torch.from_numpy(_pack(lists, cap)).to(DEV)
    n = torch.tensor(reported, dtype=torch.int64).to(torch.int32).to(DEV)
    got = tc.topk_shard(hits, n, k).cpu().numpy()
    by_case = {}
    for q, name in enumerate(names):
        full = lists[q] + [(5, 1, 0)] * (cap - len(lists[q]))
        exp = ref.select(full, reported[q], cap, k, True)
        assert _rows(got[q]) == exp, (k, name, cases.local_branches(full[:min(max(reported[q], 0), cap)], k, False))
        if not 0 < reported[q] < len(lists[q]):      # (a list cut short by its count holds other entries in every order)
            by_case.setdefault(name.rsplit("/", 1)[0], []).append(got[q])
    for name, outs in by_case.items():              # the answer does not depend on the order of the entries
        assert len(outs) == 3 and (outs[0] == outs[1]).all() and (outs[0] == outs[2]).all(), (k, name)


# ---------------------------------------------------------------- b. tvz_topk (mode 0)
@pytest.mark.parametrize("k", cases.TOPK_ONE_LIST_KS)
def test_topk_of_one_list_with_and_without_counts(k):
    cap = cases.SHARD_CAP
    names, lists, reported = cases.shard_batch(k)
    hits = torch.from_numpy(_pack(lists, cap)).to(DEV)
    n = torch.tensor(reported, dtype=torch.int64).to(torch.int32).to(DEV)
    got = tc.topk(hits, n, k).cpu().numpy()
    for q, name in enumerate(names):
        full = lists[q] + [(5, 1, 0)] * (cap - len(lists[q]))
        assert _rows(got[q]) == ref.select(full, reported[q], cap, k, False), (k, name)
    # lists_n = NULL: all `cap` entries count, padding among them
    for cap in cases.TOPK_FULL_LENGTHS:
        full_cases = [(f"full-distinct/{cap}", cap, ("distinct", 0), "pad", None), (f"full-one/{cap}", cap, ("one", 7), "dup", None),
                      (f"full-ramp/{cap}", cap, ("ramp", 4096), "pad", None)]
        names, lists, _ = cases.shard_batch(k, full_cases)
        got = tc.topk(torch.from_numpy(_pack(lists, cap)).to(DEV), None, k).cpu().numpy()
        for q, name in enumerate(names):
            assert _rows(got[q]) == ref.select(lists[q], None, cap, k, False), (k, name)


@pytest.mark.parametrize("R,cap,k", cases.TOPK_LISTS)
def test_topk_over_several_lists_fills_the_block_kernels_buffer(R, cap, k):
    names, lists, ns = cases.topk_lists_batch(R, cap, k)
    Q = len(names)
    packed = np.stack([_pack([lists[q][r] for q in range(Q)], cap) for r in range(R)])       # [R, Q, cap, 3]
    d_lists = torch.from_numpy(packed).to(DEV)
    # every list full (lists_n = NULL) for the queries made that way, explicit counts for all of them
    got_full = tc.topk(d_lists, None, k).cpu().numpy()
    counts = np.array([[cap if ns[q] is None else ns[q][r] for q in range(Q)] for r in range(R)], dtype=np.int32)
    got = tc.topk(d_lists, torch.from_numpy(counts).to(DEV), k).cpu().numpy()
    for q, name in enumerate(names):
        assert _rows(got[q]) == ref.select_lists(lists[q], ns[q], cap, k), (name, "counts")
        assert _rows(got_full[q]) == ref.select_lists(lists[q], None, cap, k), (name, "NULL")


# ---------------------------------------------------------------- c. tvz_topk_merge
def _merge_batch(R, k, Q):
    per_q = [cases.merge_query(R, k, q) for q in range(Q)]
    g = np.array([[per_q[q][0][r] for q in range(Q)] for r in range(R)], dtype=np.int64).astype(np.int32)
    return g, [ref.merge(b, k) for b, _ in per_q], [st for _, st in per_q]


def _check_merge(g, exp, styles, k, Q):
    merged, totals = tc.topk_merge(torch.from_numpy(np.ascontiguousarray(g[:, :Q])).to(DEV), k)
    merged, totals = merged.cpu().numpy(), totals.cpu().numpy()
    for q in range(Q):
        assert int(totals[q]) == exp[q][1], (g.shape[0], k, Q, q, styles[q])
        assert _rows(merged[q]) == exp[q][0], (g.shape[0], k, Q, q, styles[q])


@pytest.mark.parametrize("R", cases.MERGE_SORTED_R)
def test_sorted_merge_every_group_size_and_part_wave(R):
    for k in cases.MERGE_SORTED_K:
        g, exp, styles = _merge_batch(R, k, max(cases.MERGE_SORTED_Q))     # one reference, shared by the batch sizes
        assert cases.lists_branches([b[:k] for b in g[:, 0].tolist()], k, 2)[0].startswith("merge_sorted<")
        for Q in cases.MERGE_SORTED_Q:
            _check_merge(g, exp, styles, k, Q)


@pytest.mark.parametrize("R,k", cases.MERGE_WAVE + cases.MERGE_BLOCK)
def test_unsorted_merges_one_wave_and_block_kernel(R, k):
    g, exp, styles = _merge_batch(R, k, cases.MERGE_Q)
    family = "wave/mode2" if (R, k) in cases.MERGE_WAVE else "block/mode2"
    assert cases.lists_branches([b[:k] for b in g[:, 0].tolist()], k, 2)[0].startswith(family)
    _check_merge(g, exp, styles, k, cases.MERGE_Q)


def test_the_three_merge_families_apply_one_totals_rule():
    """The same totals - plain, a negative rank, INT32_MIN alone and among others, saturation - through the sorted
    merge (R = 16), the one-wave kernel (R = 17) and the block kernel (R = 33, k = 64): a rank of n = 0 more or less
    changes no sum, so the three answers are the reference's and each other's."""
    cols = {"plain": [5, 0, 7], "one-negative": [5, -3, 7], "refused-alone": [INT32_MIN], "refused-among": [4, INT32_MIN, 9],
            "saturated": [INT32_MAX] * 16, "saturated-negative": [INT32_MAX] * 15 + [-INT32_MAX], "zero": [0],
            "max-alone": [INT32_MAX], "just-saturated": [INT32_MAX - 1, 1, 1], "just-not": [INT32_MAX - 1, 1]}
    names = list(cols)
    answers = []
    for R, k in ((16, 4), (17, 4), (33, 64)):
        g = np.empty((R, len(names), k + 1, 3), dtype=np.int32)
        g[:] = (-1, 0, NEVER)
        for q, name in enumerate(names):
            for r, n in enumerate(cols[name]):
                g[(r * 5 + q) % R if len(cols[name]) < 16 else r, q, k, 1] = n
        _, totals = tc.topk_merge(torch.from_numpy(g).to(DEV), k)
        answers.append(totals.cpu().tolist())
        exp = [ref.merge([[ref.PAD] * k + [(-1, n, NEVER)] for n in cols[name]], k)[1] for name in names]
        assert answers[-1] == exp, (R, k, names)
    assert answers[0] == answers[1] == answers[2]
    assert dict(zip(names, answers[0]))["refused-alone"] == -INT32_MAX          # the header's rule, spelled out


# ---------------------------------------------------------------- d. the one-wave kernel in mode 1, the flagged hand-over
def _oracle_lists(rows, queries, mm=1):
    ids, offs, keys = tc.rows_to_csr(rows)
    out = []
    for q in queries:
        cnt, kth = oracle.match_kth_csr(np.asarray(q, dtype=np.float64), offs, keys, mm)
        out.append([(int(ids[c]), int(cnt[c]), int(kth[c])) for c in range(len(ids)) if cnt[c] >= mm])
    return out


@pytest.fixture(scope="module")
def match_case():
    rows, queries, lengths = cases.match_corpus()
    lists = _oracle_lists(rows, queries)
    assert [len(x) for x in lists] == lengths                # on the CPU, before anything runs: the lists intended
    dc = tc.DeviceCorpus(0)
    dc.upload(rows)
    yield dc, queries, lists
    dc.close()


@pytest.mark.parametrize("algo", [_lib.ALGO_TILE, _lib.ALGO_JOIN, _lib.ALGO_Q1], ids=["tile", "join", "q1"])
def test_match_topk_lists_of_chosen_length_and_ties(match_case, algo):
    dc, queries, lists = match_case
    cap = cases.MATCH_CAP
    d_q, d_off, max_len = tc.pack_queries(queries, DEV)
    hits, n = dc.match(d_q, d_off, max_len, 1, cap, algo=algo)
    assert n.cpu().tolist() == [len(x) for x in lists]
    for k in cases.MATCH_KS:
        got = dc.match_topk(d_q, d_off, max_len, 1, cap, k, algo=algo).cpu().numpy()
        unfused = tc.topk_shard(hits, n, k).cpu().numpy()                  # the select kernel, no wave kernel in front
        for q, lst in enumerate(lists):
            what = (k, cases.MATCH_LISTS[q][0], cases.local_branches(lst, k, True))
            assert _rows(got[q]) == ref.select(lst, len(lst), cap, k, True), what
            assert (unfused[q] == got[q]).all(), what


def test_match_topk_at_the_largest_k_and_past_it():
    """k = 1024, the largest the library takes: 1,024 rows per query, all but the few hits padding, and the totals
    row.  k = 1025 is refused."""
    Q, cap = 3, 1024
    rows = cases._hit_rows(0, list(range(25)), 1) + cases._hit_rows(1, [7] * 15, 26)         # 40 rows; query 2 hits none
    queries = [cases.query_keys(i) for i in range(Q)]
    lists = _oracle_lists(rows, queries)
    assert len(rows) == 40 and [len(x) for x in lists] == [25, 15, 0]
    dc = tc.DeviceCorpus(0)
    try:
        dc.upload(rows)
        d_q, d_off, max_len = tc.pack_queries(queries, DEV)
        with pytest.raises(RuntimeError, match=r"k=1025 out of range \[1, 1024\]"):
            dc.match_topk(d_q, d_off, max_len, 1, cap, 1025)
        got = dc.match_topk(d_q, d_off, max_len, 1, cap, 1024).cpu().numpy()
    finally:
        dc.close()
    assert got.shape == (Q, 1025, 3)
    for q, lst in enumerate(lists):
        assert _rows(got[q]) == ref.select(lst, len(lst), cap, 1024, True), q


@pytest.fixture(scope="module")
def big_case():
    rows, queries, lengths = cases.match_big_corpus()
    lists = _oracle_lists(rows, queries)
    assert [len(x) for x in lists] == lengths
    return rows, queries, lists


@pytest.mark.parametrize("algo", [_lib.ALGO_TILE, _lib.ALGO_JOIN, _lib.ALGO_Q1], ids=["tile", "join", "q1"])
def test_flagged_queries_past_the_follow_up_grid(big_case, algo):
    """Q = 1300 > kTopkFallbackBlocks: the block kernel behind the one-wave kernel has 1280 blocks that stride over
    the batch; the only flagged queries are 3 and 1290, the second of them in the stride's second round."""
    rows, queries, lists = big_case
    Q, cap, k = len(queries), cases.MATCH_CAP, 16
    lengths = [len(x) for x in lists]
    assert Q > cases.CONSTANTS["kTopkFallbackBlocks"] and max(cases.MATCH_BIG_LONG) >= cases.CONSTANTS["kTopkFallbackBlocks"]
    assert [q for q in range(Q) if lengths[q] > cases.WS_MAX] == sorted(cases.MATCH_BIG_LONG)
    dc = tc.DeviceCorpus(0)
    try:
        dc.upload(rows)
        d_q, d_off, max_len = tc.pack_queries(queries, DEV)
        got = dc.match_topk(d_q, d_off, max_len, 1, cap, k, algo=algo).cpu().numpy()
        hits, n = dc.match(d_q, d_off, max_len, 1, cap, algo=algo)
        assert n.cpu().tolist() == lengths
        unfused = tc.topk_shard(hits, n, k).cpu().numpy()
    finally:
        dc.close()
    for q in range(Q):
        assert _rows(got[q]) == ref.select(lists[q], lengths[q], cap, k, True), q
    assert (unfused == got).all()


# ---------------------------------------------------------------- e. mode 3: the pair merge behind a delta table
def test_pair_merge_of_index_and_delta_blocks():
    main, delta, queries, lengths = cases.pair_corpus()
    assert len(delta) < 300
    dc = tc.DeviceCorpus(0)
    try:
        dc.upload(main)
        for vid, ts in delta:
            dc.upsert(vid, ts)
        st = dc.index_stats()
        assert st["delta_rows"] > 0 and st["builds"] == 1            # the upserts stayed in the delta table
        li, ld = _oracle_lists(main, queries), _oracle_lists(delta, queries)
        assert [(len(a), len(b)) for a, b in zip(li, ld)] == lengths
        d_q, d_off, max_len = tc.pack_queries(queries, DEV)
        for q, (name, _, _, k, cap) in enumerate(cases.PAIR_CASES):
            got = dc.match_topk(d_q, d_off, max_len, 1, cap, k).cpu().numpy()       # the default algo: lookup + delta sweep
            a, b = li[q], ld[q]
            assert len(a) <= cap and len(b) <= cap          # neither side truncated: the rows are the exact k best
            rows, total = ref.merge([ref.select(a, len(a), cap, k, True), ref.select(b, len(b), cap, k, True)], k, pair_cap=cap)
            assert _rows(got[q]) == rows + [(-1, total, NEVER)], (name, k, cap)
            assert total == (-(len(a) + len(b)) if len(a) + len(b) > cap else len(a) + len(b))
            assert rows == ref.best(a + b, k)
        assert dc.index_stats()["builds"] == 1 and dc.index_stats()["delta_rows"] > 0      # still a delta table at the end
    finally:
        dc.close()
