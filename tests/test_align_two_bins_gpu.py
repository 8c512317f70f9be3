"""GPU parity of TVZ_ALIGN_TWO_BINS on tvz_align_wide_topk, tvz_align_rates_topk and tvz_align_span_topk
(ts_alignw2_sweep_kernel, ts_alignr2_sweep_kernel, ts_aligns2_sweep_kernel): whole [Q, k + 1, cols] blocks, bit for bit
against tests/align_two_bins_ref.py - every kind of row under every score, the edges of the bin range, the seams of the
window walk (where the count of a window's lowest bin is carried into the window below), the rates, the flag clear
against the three forms' own references, the re-timed copy, and the sharded forms."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import align_rates_ref as arr, align_span_ref as asr, align_two_bins_cases as cs, align_two_bins_ref as tb
from tests import align_wide_ref as awr
from tvidz_amd import corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E64 = cs.E64
ONE = 1 << 20
KS = (1, 16, 64)
SCORES = {"wide": ({}, dict(contain=True)), "rates": ({}, dict(contain=True)),
          "span": ({}, dict(contain=True), dict(local=True, min_votes=2))}


@pytest.fixture(scope="module")
def dc():
    c = tc.DeviceCorpus(0)
    yield c
    c.close()


def _block(dc, form, queries, eps, mo, k, rates=(1.0,), exclude_ids=None, **kw):
    """a form's block call -> int64 [Q, k + 1, cols]"""
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    d_ex = None if exclude_ids is None else torch.as_tensor(np.asarray(exclude_ids, dtype=np.int32)).to(DEV)
    args = dict(eps=eps, max_offset=mo, k=k, d_exclude_ids=d_ex, **kw)
    if form == "wide":
        out = dc.align_wide_topk_block(d_q, d_off, longest, **args)
    elif form == "rates":
        out = dc.align_rates_topk_block(d_q, d_off, longest, rates=rates, **args)
    else:
        out = dc.align_span_topk_block(d_q, d_off, longest, rates=rates, **args)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def _same(got, exp, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere((got != exp).any(axis=2))
    assert bad.size == 0, (what, f"{len(bad)} rows differ",
                           [(q, r, got[q, r].tolist(), exp[q, r].tolist()) for q, r in bad[:4].tolist()])


def _rates_of(form, rates):
    return (1.0,) if form == "wide" else tuple(rates)


# ------------------------------------------------------------------------------------- 1. every kind of row, all forms
@pytest.fixture(scope="module")
def main_world():
    rows, queries, excl = cs.main_table()
    mo = cs.MAIN_B * E64
    aligned = {r: [tb.align_two_bins_ref(rows, q, E64, mo, r) for q in queries] for r in ((1.0,), cs.MAIN_RATES)}
    return rows, queries, excl, mo, aligned


def test_the_main_tables_premises(main_world):
    rows, queries, excl, mo, aligned = main_world
    a = aligned[(1.0,)][0]
    one = awr.align_wide_ref(rows, queries[0], E64, mo)
    assert a[:7, 2:4].tolist() == [[5, 40], [10, 40], [-1, 40], [21, 30], [20, 30], [21, 28], [-11, 16]]
    assert one[1, 3] == 20 and one[3, 2:4].tolist() == [21, 16]                    # the single bin holds half
    assert a[7, 3] == 0 and a[8, 1] == 0 and a[9, 3] > 40                          # no vote, empty, votes above nv
    assert a[13, 2:4].tolist() == [cs.MAIN_B - 1, 40] and a[14, 2:4].tolist() == [cs.MAIN_B, 20]
    assert a[15, 2:4].tolist() == [-cs.MAIN_B, 15] and a[16, 2] == -5
    assert aligned[cs.MAIN_RATES][0][11, 4] == 1 and aligned[cs.MAIN_RATES][0][11, 3] == 40   # the 0.96 copy, both bins


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("form", tb.FORMS)
def test_all_rows_all_scores(dc, main_world, form, k):
    rows, queries, excl, mo, aligned = main_world
    dc.upload(rows)
    rates = _rates_of(form, cs.MAIN_RATES)
    for kw in SCORES[form]:
        for more in ({}, dict(exclude_ids=excl, min_score=ONE // 4)):
            args = dict(kw, **more)
            args.setdefault("min_votes", 1)
            exp = tb.topk_two_bins_ref(form, rows, queries, E64, mo, k, rates=rates, aligned=aligned[rates], **args)
            got = _block(dc, form, queries, E64, mo, k, rates=rates, two_bins=True, **args)
            _same(got, exp, (form, k, args))
    assert exp[0, k, 1] >= 1


# ---------------------------------------------------------------------------------------------- 2. the range's edges
@pytest.mark.parametrize("B", (0, 1, 5, 2047, 2048, 5000))
def test_the_edges_of_the_bin_range(dc, B):
    rows, q = cs.edge_table(B)
    dc.upload(rows)
    mo = B * E64
    a = tb.align_two_bins_ref(rows, q, E64, mo)
    assert a[:, 1:4].tolist() == [list(r[1:4]) for r in tb.brute_force(rows, q, E64, mo)]
    if B >= 2:                                                                     # the premises, row by row
        assert a[:, 2:4].tolist() == [[B, 3], [-B, 3], [B - 1, 3], [B, 1], [-B, 1], [0, 0], [B - 1, 3], [-B, 2]]
    for form in tb.FORMS:
        exp = tb.topk_two_bins_ref(form, rows, [q], E64, mo, 16, aligned=[a])
        _same(_block(dc, form, [q], E64, mo, 16, two_bins=True), exp, (form, B))
    if B == 0:                                                                     # the flag changes nothing
        _same(_block(dc, "wide", [q], E64, mo, 16, two_bins=True), _block(dc, "wide", [q], E64, mo, 16), "B = 0")
        assert (a[:, :4] == awr.align_wide_ref(rows, q, E64, mo)).all()


# ---------------------------------------------------------------------------------- 3. the seams of the window walk
@pytest.fixture(scope="module")
def seam_world():
    rows, queries, B = cs.seam_table()
    mo = B * E64
    return rows, queries, B, mo, [tb.align_two_bins_ref(rows, q, E64, mo) for q in queries]


def test_the_seam_tables_premises(seam_world):
    rows, queries, B, mo, aligned = seam_world
    W = cs.kernel_constant("kAwWidth")
    assert cs.window_width(B) == W and (2 * B + W) // W > 3                        # windows, more than three of them
    seams = {w * W - B for w in range(1, (2 * B + W) // W)}
    assert {-W, 0, W, 2 * W} <= seams                                              # a negative one, (-1, 0), positive ones
    wide = aligned[0]
    on_seam = [r for r in wide.tolist() if r[2] + 1 in seams]                     # the best window straddles a seam
    assert {r[2] + 1 for r in on_seam} >= {-W, 0, W, 2 * W} and len(on_seam) >= 10
    lone = aligned[1]
    assert sorted(set(lone[lone[:, 3] > 0, 2].tolist())) == sorted({S - d for S in (-W, 0, W, 2 * W) for d in (0, 1)})
    lens = [r[1] for r in wide.tolist()]
    assert 64 in [len(k) for _, k in rows] and max(lens) > cs.kernel_constant("kAwResume") + 64


@pytest.mark.parametrize("form", tb.FORMS)
def test_window_seams_and_the_carried_count(dc, seam_world, form):
    rows, queries, B, mo, aligned = seam_world
    dc.upload(rows)
    for k in (64, 5):
        exp = tb.topk_two_bins_ref(form, rows, queries, E64, mo, k, aligned=aligned)
        _same(_block(dc, form, queries, E64, mo, k, two_bins=True), exp, (form, k))
    assert exp[0, 5, 1] == sum(1 for r in aligned[0].tolist() if r[3]) and exp[1, 5, 1] == 12
    # wider ranges, the widest among them: the seams of other window grids fall elsewhere in the same table
    for wider in (B + 517, tc.ALIGN_WIDE_MAX_B):
        if form == "wide" or wider != tc.ALIGN_WIDE_MAX_B:
            a = [tb.align_two_bins_ref(rows, q, E64, wider * E64) for q in queries]
            exp = tb.topk_two_bins_ref(form, rows, queries, E64, wider * E64, 64, aligned=a)
            _same(_block(dc, form, queries, E64, wider * E64, 64, two_bins=True), exp, (form, wider))


# ------------------------------------------------------------------------------------------------------- 4. rates
def test_rates_keep_the_best_window(dc):
    rows, q = cs.rates_table()
    dc.upload(rows)
    mo = 20.0
    both = tb.align_two_bins_ref(rows, q, E64, mo, (1.0, 0.96))
    assert both[0, 2:5].tolist() == [7, 25, 1]                                     # the window at 0.96 ...
    assert arr.align_rates_ref(rows, q, E64, mo, (1.0, 0.96))[0, 2:5].tolist() == [5, 15, 0]   # ... the single bin at 1.0
    assert both[1, 2:5].tolist() == [5, 10, 0]                                     # equal J: the smaller index
    assert tb.align_two_bins_ref(rows, q, E64, mo, (0.96,))[1, 3] == 10
    for rates in ((1.0, 0.96), (0.96, 1.0), (1.0, 1.0), (1.0,)):
        a = [tb.align_two_bins_ref(rows, q, E64, mo, rates)]
        for form in ("rates", "span"):
            exp = tb.topk_two_bins_ref(form, rows, [q], E64, mo, 4, rates=rates, aligned=a)
            _same(_block(dc, form, [q], E64, mo, 4, rates=rates, two_bins=True), exp, (form, rates))
    wide = _block(dc, "wide", [q], E64, mo, 4, two_bins=True)
    rated = _block(dc, "rates", [q], E64, mo, 4, rates=(1.0,), two_bins=True)
    assert (rated[:, :, :4] == wide).all() and (rated[:, :4, 4] == 0).all()


# -------------------------------------------------------------------------------------------------- 5. the flag clear
@pytest.mark.parametrize("form", tb.FORMS)
def test_flag_clear_is_the_single_bin(dc, main_world, form):
    rows, queries, excl, mo, _ = main_world
    dc.upload(rows)
    rates = _rates_of(form, cs.MAIN_RATES)
    for kw in SCORES[form]:
        if form == "wide":
            exp = awr.topk_wide_ref(rows, queries, E64, mo, 16, exclude_ids=excl, **kw)
        elif form == "rates":
            exp = arr.topk_rates_ref(rows, queries, E64, mo, rates, 16, exclude_ids=excl, **kw)
        else:
            exp = asr.topk_span_ref(rows, queries, E64, mo, rates, 16, exclude_ids=excl, **kw)
        _same(_block(dc, form, queries, E64, mo, 16, rates=rates, exclude_ids=excl, **kw), exp, (form, kw))
        _same(_block(dc, form, queries, E64, mo, 16, rates=rates, exclude_ids=excl, two_bins=False, **kw), exp, (form, kw))


# ---------------------------------------------------------------------------------------------- 6. the re-timed copy
def test_the_retimed_copy_is_found_with_the_flag_only(dc):
    stored, upload = tb.retimed_case()
    dc.upload([(7, stored), (8, [s + 0.011 for s in stored[:50]])])
    kw = dict(eps=1 / 30, max_offset=300.0, k=4, min_score=int(0.8 * ONE))
    rows, totals = dc.align_wide_topk([upload], **kw)
    assert totals.tolist() == [0] and (rows[:, :, 0] == -1).all()
    rows, totals = dc.align_wide_topk([upload], two_bins=True, **kw)
    exp = tb.align_two_bins_ref([(7, stored)], upload, 1 / 30, 300.0)[0]
    assert totals.tolist() == [1] and rows[0, 0].tolist() == exp[:4].tolist() and exp[3] == 200
    assert abs((rows[0, 0, 2] + 0.5) / 30 - 123.4567) <= 1 / 30                    # the shift at the window's middle


# ------------------------------------------------------------------------------------------------------ 7. sharded
SHARDS = {"wide": tc.align_wide_topk_shards, "rates": tc.align_rates_topk_shards, "span": tc.align_span_topk_shards}
MERGES = {"wide": tc.align_wide_topk_merge, "rates": tc.align_rates_topk_merge, "span": tc.align_span_topk_merge}
SIZERS = {"wide": tc.align_wide_topk_workspace_bytes, "rates": tc.align_rates_topk_workspace_bytes,
          "span": tc.align_span_topk_workspace_bytes}


@pytest.fixture(scope="module")
def three_shards(main_world):
    rows = main_world[0]
    shards = [tc.DeviceCorpus(0) for _ in range(3)]
    for r, s in enumerate(shards):
        s.upload(rows[r::3])
    yield shards
    for s in shards:
        s.close()


@pytest.mark.parametrize("form", tb.FORMS)
def test_three_shards_equal_one_handle_and_merges_ignore_the_bit(dc, main_world, three_shards, form):
    rows, queries, excl, mo, aligned = main_world
    dc.upload(rows)
    rates = _rates_of(form, cs.MAIN_RATES)
    more = {} if form == "wide" else dict(rates=rates)
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    d_ex = torch.as_tensor(np.asarray(excl, dtype=np.int32)).to(DEV)
    for k in (5, 64):
        for kw in SCORES[form]:
            one = _block(dc, form, queries, E64, mo, k, rates=rates, exclude_ids=excl, two_bins=True, **kw)
            ws = torch.empty(SIZERS[form](len(queries), longest, d_q.numel(), k), dtype=torch.uint8, device=DEV)
            blocks, got, totals = SHARDS[form](three_shards, d_q, d_off, longest, eps=E64, max_offset=mo, k=k, workspace=ws,
                                               d_exclude_ids=d_ex, two_bins=True, **more, **kw)
            torch.cuda.synchronize()
            assert (got.cpu().numpy() == one[:, :k]).all() and (totals.cpu().numpy() == one[:, k, 1]).all(), (form, k, kw)
            exp = tb.topk_two_bins_ref(form, rows, queries, E64, mo, k, rates=rates, aligned=aligned[rates],
                                       exclude_ids=excl, **dict(dict(min_votes=1), **kw))
            _same(one, exp, (form, k, kw))
            # the merge of the same lists with and without the bit: identical
            score = {n: v for n, v in kw.items() if n in ("contain", "local")}
            with_bit = MERGES[form](blocks, k, d_q, d_off, two_bins=True, **score)
            without = MERGES[form](blocks, k, d_q, d_off, **score)
            torch.cuda.synchronize()
            assert torch.equal(with_bit[0], without[0]) and torch.equal(with_bit[1], without[1])
            assert torch.equal(with_bit[0], got) and torch.equal(with_bit[1], totals)


def test_sharded_through_rccl_world_size_1(tmp_path):
    """tvz_align_{wide,rates,span}_topk_sharded in a child process of its own (the communicator comes before the first
    GPU call): the one-handle call's rows and totals under the flag, which differ from the flag-clear ones."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "near_two_bins_comm_child.py")], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for form in tb.FORMS:
        r = res[form]
        assert r["rows"] == r["one_rows"] and r["totals"] == r["one_totals"], form
        assert r["rows"] != r["clear_rows"], form
    assert res["unknown_flag"][0] == -1 and "unknown flag bits 0x4" in res["unknown_flag"][1]


# ------------------------------------------------------------------------------- 8. the service's corpus, the inspector
@pytest.mark.parametrize("n_shards", [3, 20])
def test_sharded_corpus_carries_the_flag(main_world, n_shards):
    """service.ShardedCorpus: one tvz_<stem>_shards call per group of 16 shards (20: two groups, merged again)"""
    from tvidz_amd import service
    rows, queries, excl, mo, aligned = main_world
    sc = service.ShardedCorpus(0, n_shards=n_shards, k=8)
    try:
        sc.upload(rows)
        for form, call, kw in (("wide", sc.align_wide_topk, dict(contain=True)), ("rates", sc.align_rates_topk, dict()),
                               ("span", sc.align_span_topk, dict(local=True, min_votes=2))):
            rates = _rates_of(form, cs.MAIN_RATES)
            exp = tb.topk_two_bins_ref(form, rows, queries, E64, mo, 5, rates=rates, aligned=aligned[rates], exclude_ids=excl,
                                       **dict(dict(min_votes=1), **kw))
            more = {} if form == "wide" else dict(rates=rates)
            got_rows, got_totals = call(queries, eps=E64, max_offset=mo, k=5, exclude_ids=excl, two_bins=True, **more, **kw)
            assert (got_rows == exp[:, :5]).all() and (got_totals == exp[:, 5, 1]).all(), form
    finally:
        sc.close()


@pytest.mark.parametrize("shift,any_offset", [(12.3456, False), (123.4567, True)])
def test_inspector_reports_the_retimed_copy_with_the_option_only(tmp_path, shift, any_offset):
    """the bounded configuration (routed to align_wide_topk over near_max_offset) and the search at any shift"""
    from tests.fakes import CutReader, cut_inspector
    from tvidz_amd import db as tdb
    stored, upload = tb.retimed_case(shift=shift)
    cuts = {"stored.y4m": stored, "copy.y4m": upload}
    more = dict(near_any_offset=True) if any_offset else dict()
    for two in (False, True):
        store = tdb.Store(f"sqlite:///{tmp_path}/{int(two)}.db", corpus=tc.DeviceCorpus(0))
        ins = cut_inspector(store, device=DEV, near_duplicates=True, near_top_k=4, near_two_bins=two,
                            frame_source=lambda bucket, key, filename, uid: (CutReader(cuts[key], per_batch=50,
                                                                                       frames=12000), None), **more)
        try:
            res = [ins.analyze_file("videos", k) for k in ("stored.y4m", "copy.y4m")]
            assert all(r["status"] == "done" and r["duplicates"] == [] for r in res), res
            assert res[0]["near_duplicates"] == []
            if not two:
                assert res[1]["near_duplicates"] == []
                continue
            (near,) = res[1]["near_duplicates"]
            assert near["filename"] == "stored.y4m" and near["jaccard"] == 1.0
            assert abs(near["shift_seconds"] - shift) <= 1 / 30 and round(near["shift_seconds"] * 30 - 0.5, 6) % 1 == 0
        finally:
            store.close()                      # closes the corpus too
