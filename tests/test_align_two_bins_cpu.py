"""TVZ_ALIGN_TWO_BINS without a GPU: the flag checks that come before anything touches a device, the reference of
tests/align_two_bins_ref.py against a plain-Python double loop and against its own properties, the re-timed copy that
only the window of two bins finds, the Inspector's and the service's option on fakes of their own
(tests/near_two_bins_fakes.py), the binding's table and version unchanged, and the gfx950 code objects of the three new
sweep kernels read with the metadata readers of tests/test_codeobj_cpu.py."""
import argparse
import ctypes as C
import hashlib
import re
import subprocess

import numpy as np
import pytest

from tests import align_rates_ref as arr, align_ref as ar, align_span_ref as asr, align_two_bins_cases as cs
from tests import align_two_bins_ref as tb, align_wide_ref as awr
from tests.near_two_bins_fakes import HIT, OldCorpus, Store, TwoBinsCorpus
from tests.test_align_span_cpu import HEADER
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)
from tvidz_amd import _lib, corpus as tc, service

E64 = cs.E64
ONE = 1 << 20
TWO = tc.ALIGN_TWO_BINS
NEW = ("23ts_alignw2_sweep_kernelE", "23ts_alignr2_sweep_kernelE", "23ts_aligns2_sweep_kernelE")
SIBLINGS = ("22ts_alignw_sweep_kernelE", "22ts_alignr_sweep_kernelE", "22ts_aligns_sweep_kernelE")


# ------------------------------------------------------------------------------------------------ 1. the flag checks
def _calls():
    """the three forms' calls, their _shards and their merges on NULL handles and pointers: flags -> return code"""
    lib = _lib.load()
    rates = (C.c_double * 2)(1.0, 0.96)

    def wide(flags):
        rc = lib.tvz_align_wide_topk(None, None, None, 1, 4, 1 / 30, 1.0, 1, 0, flags, None, 16, None, None, 0, None)
        rs = lib.tvz_align_wide_topk_shards(None, 1, None, None, 1, 4, 1 / 30, 1.0, 1, 0, flags, None, 16, None, None, None,
                                            None, 0, None)
        return rc, rs

    def rated(flags):
        rc = lib.tvz_align_rates_topk(None, None, None, 1, 4, 1 / 30, 1.0, rates, 2, 1, 0, flags, None, 16, None, None, 0, None)
        rs = lib.tvz_align_rates_topk_shards(None, 1, None, None, 1, 4, 1 / 30, 1.0, rates, 2, 1, 0, flags, None, 16, None,
                                             None, None, None, 0, None)
        return rc, rs

    def span(flags):
        rc = lib.tvz_align_span_topk(None, None, None, 1, 4, 1 / 30, 1.0, rates, 2, 1, 0, flags, None, 16, None, None, 0, None)
        rs = lib.tvz_align_span_topk_shards(None, 1, None, None, 1, 4, 1 / 30, 1.0, rates, 2, 1, 0, flags, None, 16, None,
                                            None, None, None, 0, None)
        return rc, rs

    def merge(stem):
        return lambda flags: getattr(lib, f"tvz_align_{stem}_topk_merge")(None, 3, 0, 4, flags, None, None, None, None, None)

    return lib, wide, rated, span, merge


def test_the_flags_value_and_the_header():
    text = open(HEADER).read()
    assert re.search(r"^#define TVZ_ALIGN_TWO_BINS 8u\b", text, re.M) and TWO == tb.TWO_BINS == 8
    assert "bit 4 is no flag" in text                                              # 4 stays refused, and the header says so
    assert tc.FORM_WIDE.two_bins and tc.FORM_RATES.two_bins and tc.FORM_SPAN.two_bins and not tc.FORM_BOUNDED.two_bins
    assert tc._span_flags(True, False, True) == 9 and tc._span_flags(False, True, True) == 10
    assert tc._align_flags(tc.FORM_WIDE, two_bins=True) == [8] and tc._align_flags(tc.FORM_WIDE) == [0]
    with pytest.raises(ValueError, match="TVZ_ALIGN_TWO_BINS"):
        tc._align_flags(tc.FORM_BOUNDED, two_bins=True)


def test_the_span_form_takes_the_flag_before_the_handle_is_looked_at():
    lib, wide, rated, span, merge = _calls()
    for flags in (TWO, TWO | 1, TWO | 2):                                          # good: refused for the NULL handle
        assert span(flags) == (ar.ERR_INVALID, ar.ERR_INVALID)
        msg = lib.tvz_last_error()
        assert b"flag" not in msg and b"rate" not in msg and b"TVZ_ALIGN" not in msg, (flags, msg)
    for flags, word in ((TWO | 3, b"TVZ_ALIGN_CONTAIN and TVZ_ALIGN_LOCAL are two score kinds"), (3, b"two score kinds"),
                        (4, b"unknown flag bits 0x4"), (TWO | 4, b"unknown flag bits 0x4"),
                        (0x80000008, b"unknown flag bits 0x80000000"), (16, b"unknown flag bits 0x10")):
        assert span(flags) == (ar.ERR_INVALID, ar.ERR_INVALID)
        assert word in lib.tvz_last_error(), (flags, lib.tvz_last_error())


def test_the_wide_and_rates_forms_and_every_merge():
    lib, wide, rated, span, merge = _calls()
    # (these two look at the handle first: a NULL one is what every call below is refused for, as before; their flag
    # rule shows in their merges, which take no handle and check the same table entry)
    for call in (wide, rated):
        for flags in (TWO, TWO | 1, TWO | 3, 4, TWO | 4, 0x80000008, 2, TWO | 2):
            assert call(flags) == (ar.ERR_INVALID, ar.ERR_INVALID), flags
    for stem in ("wide", "rates"):
        for flags in (0, 1, TWO, TWO | 1):
            assert merge(stem)(flags) == 0, (stem, flags)
        for flags, bits in ((2, b"0x2"), (TWO | 2, b"0x2"), (3, b"0x2"), (4, b"0x4"), (TWO | 4, b"0x4"),
                            (0x80000008, b"0x80000000"), (TWO | 3, b"0x2")):
            assert merge(stem)(flags) == ar.ERR_INVALID and b"merge: unknown flag bits " + bits in lib.tvz_last_error(), (stem, flags)
    for flags in (0, 1, 2, TWO, TWO | 1, TWO | 2):
        assert merge("span")(flags) == 0, flags
    for flags in (3, TWO | 3, 4, TWO | 4, 0x80000008):
        assert merge("span")(flags) == ar.ERR_INVALID, flags
    # what the merges refused they still refuse, with the bit set too
    for n_lists, k in ((0, 4), (17, 4), (3, 0), (3, 65)):
        for stem in ("wide", "rates", "span"):
            assert getattr(lib, f"tvz_align_{stem}_topk_merge")(None, n_lists, 0, k, TWO, None, None, None, None,
                                                                None) == ar.ERR_UNSUPPORTED


def test_signatures_and_version_are_unchanged():
    assert _lib.VERSION == 404 and _lib.load().tvz_version() == 404
    # the binding's table as it stood before the flag: 75 exports, every result and argument type (a digest of their names)
    sig = repr(sorted((n, getattr(r, "__name__", repr(r)), [getattr(a, "__name__", repr(a)) for a in args])
                      for n, (r, args) in _lib.SIGNATURES.items()))
    assert len(_lib.SIGNATURES) == 75 and hashlib.sha1(sig.encode()).hexdigest() == "282938b267df1282d3482c99a5c7bf489ef006b7"
    for stem in ("wide", "rates", "span"):                                         # flags: the uint32 it was
        for suffix in ("", "_merge", "_shards", "_sharded"):
            assert C.c_uint32 in _lib.SIGNATURES[f"tvz_align_{stem}_topk{suffix}"][1]
    assert not [n for n in _lib.SIGNATURES if "two_bins" in n]                     # no new export


# ------------------------------------------------------------------------------- 2. the reference and its properties
def test_reference_equals_the_double_loop():
    checked = 0
    for rows, queries, mo, rates in ((cs.main_table()[0], cs.main_table()[1][:4], cs.MAIN_B * E64, (1.0,)),
                                     (cs.main_table()[0][:14], [cs.main_table()[1][6]], cs.MAIN_B * E64, (0.96,)),
                                     (cs.seam_table()[0], cs.seam_table()[1], cs.seam_table()[2] * E64, (1.0,)),
                                     (cs.edge_table(5)[0], [cs.edge_table(5)[1]], 5 * E64, (1.0,)),
                                     (cs.edge_table(1)[0], [cs.edge_table(1)[1]], 1 * E64, (1.0,)),
                                     (cs.rates_table()[0], [cs.rates_table()[1]], 20.0, (0.96,))):
        for q in queries:
            a = tb.align_two_bins_ref(rows, q, E64, mo, rates)
            brute = tb.brute_force(rows, q, E64, mo, rates[0])
            assert [tuple(r[:4]) + tuple(r[5:]) for r in a.tolist()] == brute
            checked += sum(1 for r in brute if r[3])
    assert checked > 150


def test_b_zero_is_the_single_bin_reference():
    rows, queries, _ = cs.main_table()
    for q in queries[:3]:
        for mo in (0.0, 0.4 * E64):
            assert (tb.align_two_bins_ref(rows, q, E64, mo)[:, :4] == awr.align_wide_ref(rows, q, E64, mo)).all()
            span = asr.align_span_ref(rows, q, E64, mo, (1.0, 0.96))
            assert (tb.align_two_bins_ref(rows, q, E64, mo, (1.0, 0.96)) == span).all()


def test_votes_in_one_bin_only_report_that_bin():
    q = [10.0, 20.0, 30.0]
    for d in (-7, 0, 7):
        (row,) = tb.align_two_bins_ref([(1, [x + d * E64 for x in q])], q, E64, 1.0).tolist()
        assert row[2:4] == [d, 3] and row[2:4] == awr.align_wide_ref([(1, [x + d * E64 for x in q])], q, E64, 1.0)[0, 2:4].tolist()


def test_h_3_0_2_2_and_the_tie_chain():
    q = [100.0 * i for i in range(1, 8)]                                           # 6,400 bins apart: no cross votes

    def row(bins):
        return [(1, [x + b * E64 for x, b in zip(q, bins)])]

    rows = row([0, 0, 0, 2, 2, 3, 3])                                              # h = (3, 0, 2, 2) on bins 0..3
    assert awr.align_wide_ref(rows, q, E64, 10.0)[0, 2:4].tolist() == [0, 3]
    assert tb.align_two_bins_ref(rows, q, E64, 10.0)[0, 2:4].tolist() == [2, 4]
    assert tb.best_window(np.array([0, 0, 0, 2, 2, 3, 3])) == (2, 4, 2)
    # J ties: the most h[b] ...
    assert tb.best_window(np.array([5, 6, 6, 7])) == (6, 3, 2)                     # J[5] = J[6] = 3; h = 1 against 2
    # ... then the smaller |b| ...
    assert tb.best_window(np.array([5, 6, 7])) == (5, 2, 1) and tb.best_window(np.array([-7, -6, -5])) == (-6, 2, 1)
    # ... then the negative one
    assert tb.best_window(np.array([-5, -4, 5, 6])) == (-5, 2, 1)
    assert tb.best_window(np.array([], dtype=np.int64)) == (0, 0, 0)
    # a window whose lower bin is empty never wins: every reported bin has votes of its own
    rows, queries, _ = cs.main_table()
    a = tb.align_two_bins_ref(rows, queries[0], E64, cs.MAIN_B * E64)
    one = {r[0]: r for r in a.tolist()}
    for (vid, keys) in rows:
        if one[vid][3]:
            _, b, ok = tb.bins_of(keys, asr.sorted_query(queries[0]), E64, cs.MAIN_B)
            assert (b[ok] == one[vid][2]).sum() >= 1


def test_the_retimed_copy_is_found_by_the_window_of_two_bins_only():
    stored, upload = tb.retimed_case()
    assert len(stored) == len(upload) == 200
    rows = [(7, stored)]
    need = int(np.floor(0.8 * ONE))
    single = awr.align_wide_ref(rows, upload, 1 / 30, 300.0)[0]
    double = tb.align_two_bins_ref(rows, upload, 1 / 30, 300.0)[0]
    print("single bin:", single.tolist(), awr.score(single[3], 200, 200), "two bins:", double.tolist(),
          awr.score(double[3], 200, 200), "needed:", need)
    assert awr.score(single[3], 200, 200)[1] < need <= awr.score(double[3], 200, 200)[1]
    assert double[2] in (single[2], single[2] - 1) and double[3] > single[3]
    for kw, found in ((dict(), False), (dict(two=True), True)):
        block = (tb.topk_two_bins_ref("wide", rows, [upload], 1 / 30, 300.0, 4, min_score=need) if kw else
                 awr.topk_wide_ref(rows, [upload], 1 / 30, 300.0, 4, min_score=need))
        assert (block[0, 4, 1] == 1) == found and (block[0, 0, 0] == 7) == found


def test_rates_keep_the_most_j():
    rows, q = cs.rates_table()
    both = tb.align_two_bins_ref(rows, q, E64, 20.0, (1.0, 0.96))
    assert both[0, 2:5].tolist() == [7, 25, 1] and arr.align_rates_ref(rows, q, E64, 20.0, (1.0, 0.96))[0, 2:5].tolist() == [5, 15, 0]
    assert both[1, 2:5].tolist() == [5, 10, 0] and tb.align_two_bins_ref(rows, q, E64, 20.0, (0.96, 1.0))[1, 2:5].tolist() == [7, 10, 0]


# ------------------------------------------------------------------------------------- 3. the inspector, the service
def _inspector(corpus, **kw):
    from tvidz_amd import inspector as insp
    return insp.Inspector(Store(corpus), device="cuda:0", **kw)


def test_inspector_refusals():
    with pytest.raises(ValueError, match="near_two_bins=True needs near_duplicates=True and near_top_k"):
        _inspector(TwoBinsCorpus(), near_duplicates=True, near_two_bins=True)
    with pytest.raises(ValueError, match="near_two_bins=True needs near_duplicates=True and near_top_k"):
        _inspector(TwoBinsCorpus(), near_top_k=8, near_two_bins=True)
    with pytest.raises(ValueError, match="near_parts=2"):
        _inspector(TwoBinsCorpus(), near_duplicates=True, near_top_k=8, near_any_offset=True, near_score="local",
                   near_min_votes=2, near_parts=2, near_two_bins=True)
    bounded_only = type("BoundedOnly", (), {"align": TwoBinsCorpus.align, "align_topk": TwoBinsCorpus.align_topk})
    with pytest.raises(RuntimeError, match="align_wide_topk"):
        _inspector(bounded_only(), near_duplicates=True, near_top_k=8, near_two_bins=True)


def test_inspector_passes_the_keyword_only_when_set_and_reports_the_windows_middle():
    cuts = [100.0 - i for i in range(40)] + [float("nan")]
    s = sorted(x for x in cuts if x == x)
    ok = dict(near_duplicates=True, near_top_k=8, near_jaccard=0.01)
    # off: no corpus method hears of it, whatever the other options - an old corpus keeps working
    old = OldCorpus()
    (near,) = _inspector(old, **ok)._near(7, cuts)
    assert old.calls == ["align_topk"] and near["shift_seconds"] == HIT[2] * (1 / 30)
    (near,) = _inspector(old, near_any_offset=True, **ok)._near(7, cuts)
    assert old.calls[-1] == "align_wide_topk" and near["shift_seconds"] == HIT[2] * (1 / 30)
    for more in (dict(), dict(near_any_offset=True), dict(near_any_offset=True, near_rates=(1.0, 0.96)),
                 dict(near_any_offset=True, near_spans=True)):
        corpus = TwoBinsCorpus()
        ins = _inspector(corpus, **ok, **more)
        assert ins.near_two_bins is False and ins._near(7, cuts)
        assert all("two_bins" not in kw for _, kw in corpus.calls)
    # on, the bounded configuration: the call that takes flags, over near_max_offset
    corpus = TwoBinsCorpus()
    ins = _inspector(corpus, near_two_bins=True, near_max_offset=12.5, **ok)
    (near,) = ins._near(7, cuts)
    (name, kw), = corpus.calls
    assert name == "align_wide_topk" and kw["two_bins"] is True and kw["max_offset"] == 12.5 and "min_votes" not in kw
    assert "contain" not in kw and kw["exclude_ids"] == [7] and kw["k"] == 8
    assert near["shift_seconds"] == (HIT[2] + 0.5) * ins.near_eps and near["video_id"] == 42
    ins = _inspector(corpus, near_two_bins=True, near_min_votes=3, **ok)
    ins._near(7, cuts)
    assert corpus.calls[-1][0] == "align_wide_topk" and corpus.calls[-1][1]["min_votes"] == 3
    # on, at any shift: each form's own call with the keyword; the stored span starts from the same shift
    for more, name in ((dict(), "align_wide_topk"), (dict(near_rates=(1.0, 0.96)), "align_rates_topk"),
                       (dict(near_spans=True), "align_span_topk"),
                       (dict(near_score="local", near_min_votes=2), "align_span_topk")):
        corpus = TwoBinsCorpus()
        ins = _inspector(corpus, near_two_bins=True, near_any_offset=True, **dict(ok, **more))
        (near,) = ins._near(7, cuts)
        assert [c[0] for c in corpus.calls] == [name] and corpus.calls[0][1]["two_bins"] is True
        assert corpus.calls[0][1]["max_offset"] is None
        shift = (HIT[2] + 0.5) * ins.near_eps
        assert near["shift_seconds"] == shift
        if name == "align_span_topk":
            assert near["upload_span"] == [s[3], s[22]] and near["stored_span"] == [s[3] + shift, s[22] + shift]
    # a refused query falls back to the walk, whose bins are single: no half bin
    corpus = TwoBinsCorpus(refuse=True)
    (near,) = _inspector(corpus, near_two_bins=True, **ok)._near(7, cuts)
    assert [c[0] for c in corpus.calls] == ["align_wide_topk", "align"] and near["shift_seconds"] == HIT[2] * (1 / 30)


def test_the_service_carries_the_flag():
    # an ask's flags
    six = service.check_near(tc.FORM_WIDE, 1 / 30, None, 4, 1, 0, two_bins=True)
    assert six[5] == TWO and service.check_near(tc.FORM_WIDE, 1 / 30, None, 4, 1, 0)[5] == 0
    assert service.check_near(tc.FORM_SPAN, 1 / 30, None, 4, 2, 0, local=True, two_bins=True)[5] == TWO | tc.ALIGN_LOCAL
    assert service.check_near(tc.FORM_RATES, 1 / 30, None, 4, 1, 0, contain=True, two_bins=True)[5] == TWO | tc.ALIGN_CONTAIN
    with pytest.raises(ValueError, match="two bins"):
        service.check_near(tc.FORM_BOUNDED, 1 / 30, 3.0, 4, 1, 0, two_bins=True)
    # the switch
    assert service.check_near_switches(4, near_two_bins=True) == ["--near-two-bins"]
    assert service.check_near_switches(4) == [] and service.check_near_switches(0) == []
    assert service.check_near_switches(4, True, "local", 8, (1.0, 0.96), True, 0, True)[-2:] == ["--near-spans", "--near-two-bins"]
    with pytest.raises(ValueError, match="--near-two-bins needs --near-top-k"):
        service.check_near_switches(0, near_two_bins=True)
    with pytest.raises(ValueError, match="--near-two-bins with --near-parts 2"):
        service.check_near_switches(4, True, "local", 2, None, False, 2, True)
    assert service.near_kwargs(argparse.Namespace(near_top_k=4, near_eps=1 / 30, near_max_offset=30.0, near_jaccard=0.8,
                                                  near_two_bins=True))["near_two_bins"] is True
    assert "near_two_bins" not in service.near_kwargs(argparse.Namespace(near_top_k=4, near_eps=1 / 30, near_max_offset=30.0,
                                                                         near_jaccard=0.8, near_two_bins=False))
    assert "near_two_bins" not in service.near_kwargs(argparse.Namespace(near_top_k=4, near_eps=1 / 30, near_max_offset=30.0,
                                                                         near_jaccard=0.8))


def test_the_launcher_hands_the_switch_to_every_rank(monkeypatch, tmp_path):
    started = []

    class FakePopen:
        def __init__(self, cmd, env=None):
            self.args = cmd
            started.append(cmd)

        def poll(self):
            return 0

    monkeypatch.setattr(subprocess, "Popen", FakePopen)
    monkeypatch.setattr(service.RankService, "_wait_ready", lambda self, timeout: None)
    url = f"sqlite:///{tmp_path}/t.db"
    kw = dict(base_port=5900, backend="gloo", parts="m:f", k=4, cap=64, workers=8, tick_s=0.002)
    with pytest.raises(ValueError, match="--near-two-bins needs --near-top-k"):
        service.RankService(2, url, near_two_bins=True, **kw)
    with pytest.raises(ValueError, match="--near-two-bins needs --near-top-k"):
        service.main(["--ranks", "2", "--db", url, "--near-two-bins"])
    assert started == []
    off = service.RankService(2, url, near_top_k=4, **kw)
    assert len(off.procs) == 2 and all("--near-two-bins" not in p.args for p in off.procs)
    on = service.RankService(2, url, near_top_k=4, near_two_bins=True, **kw)
    assert len(on.procs) == 2 and all(p.args[-1] == "--near-two-bins" for p in on.procs)
    seen = {}
    monkeypatch.setattr(service, "_child_main", lambda a: seen.update(vars(a)) or 0)
    assert service.main(["--child"] + on.procs[0].args[on.procs[0].args.index("--near-top-k"):]) == 0
    assert seen["near_two_bins"] is True and service.near_kwargs(argparse.Namespace(**seen))["near_two_bins"] is True


# -------------------------------------------------------------------------------------------- 4. the code objects
def _one(kernels, name):  # noqa: F811
    (k,) = [k for n, k in kernels.items() if name in n]
    return k


def test_the_new_sweeps_exist_once_beside_their_siblings(kernels):  # noqa: F811
    for name in NEW + SIBLINGS:
        assert len([n for n in kernels if name in n]) == 1, (name, sorted(n for n in kernels if "align" in n))
    for name in NEW:                                                               # names of their own
        assert not any(s in n for s in SIBLINGS for n in kernels if name in n)


def test_the_new_sweeps_have_no_scratch_no_spills_and_256_threads(kernels):  # noqa: F811
    for name in NEW:
        k = _one(kernels, name)
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (name, k)
        assert k[".max_flat_workgroup_size"] == 256


def test_the_new_sweeps_lds_and_registers(kernels):  # noqa: F811
    """Static LDS: the sibling's, byte for byte (the block-end merge's 4 x 64 kept hits + the hit counter); the largest
    dynamic part (4,095 query values, one window of 4,096 bins) still inside a workgroup's 160 KiB.  Registers, as the
    compiler reports them: 76 / 78 / 84 against the siblings' 70 / 78 / 82 - the lane's best window is three words
    (J, and h with the bin's order) where the best bin is two, and the scan of the touched list holds two counts and
    the carried one.  The hardware allocates in granules of 8: the wide sweep goes from the sibling's 72 (its test's
    cap) to 80, seven waves per SIMD to six, where the LDS already limits every call of more than ~600 bins to three
    or four blocks per CU (tests/test_align_wide_codeobj_cpu.py); the sweep with rates stays inside its sibling's cap
    of 80; the span sweep stays inside the granule its sibling (82 -> 88) occupies."""
    for name, sibling, hit_bytes, cap in zip(NEW, SIBLINGS, (20, 24, 32), (72 + 8, 80, 88)):
        k, s = _one(kernels, name), _one(kernels, sibling)
        assert k[".group_segment_fixed_size"] == s[".group_segment_fixed_size"], name
        assert 4 * 64 * hit_bytes <= k[".group_segment_fixed_size"] <= 4 * 64 * hit_bytes + 64, k[".group_segment_fixed_size"]
        assert k[".group_segment_fixed_size"] + 4095 * 8 + 4 * (4096 * 6 + 4) <= 160 * 1024
        assert k[".vgpr_count"] <= cap, (name, k[".vgpr_count"])
        assert (s[".vgpr_count"] + 7) // 8 * 8 <= cap                              # (the sibling fits the same cap)


# ------------------------------------------------------------------------------ 5. through the tick, two ranks on gloo
def _rank_worker(rank, world, port, out):
    import os

    import torch.distributed as dist

    from tests.fakes import OracleCorpus
    from tests.near_two_bins_fakes import two_bins_backend
    from tvidz_amd import sharded
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rc = None
    try:
        rows, queries, excl = cs.main_table()
        queries, excl = queries[:4], excl[:4]
        mo = cs.MAIN_B * E64
        shard = OracleCorpus()
        g = dist.new_group(backend="gloo")
        backend = two_bins_backend(live=shard)
        rc = service.RankCorpus(shard, sharded.ShardedMatcher(backend, k=8, cap=64, group=g), group=g, xdev="cpu", tick_s=0.01)
        rc.upload(rows)                                               # video_id mod world
        dist.barrier()
        k = 5
        # the flag clear: no backend hears the keyword
        exp = awr.topk_wide_ref(rows, queries, E64, mo, k, exclude_ids=excl)
        got_rows, got_totals = rc.align_wide_topk(queries, eps=E64, max_offset=mo, k=k, exclude_ids=excl)
        assert (got_rows == exp[:, :k]).all() and (got_totals == exp[:, k, 1]).all()
        dist.barrier()
        # the flag set, on the three forms: the whole table's answer under the flag
        for form, call, kw in (("wide", rc.align_wide_topk, dict(contain=True)),
                               ("rates", rc.align_rates_topk, dict(rates=cs.MAIN_RATES)),
                               ("span", rc.align_span_topk, dict(rates=cs.MAIN_RATES, local=True, min_votes=2))):
            exp = tb.topk_two_bins_ref(form, rows, queries, E64, mo, k, exclude_ids=excl, **dict(dict(min_votes=1), **kw))
            got_rows, got_totals = call(queries, eps=E64, max_offset=mo, k=k, exclude_ids=excl, two_bins=True, **kw)
            assert (got_rows == exp[:, :k]).all() and (got_totals == exp[:, k, 1]).all(), form
            dist.barrier()
        assert (exp[:, :k] != asr.topk_span_ref(rows, queries, E64, mo, cs.MAIN_RATES, k, min_votes=2, local=True,
                                                exclude_ids=excl)[:, :k]).any()
        with pytest.raises(ValueError, match="two bins"):             # refused in the caller, before the tick
            rc._near(tc.FORM_BOUNDED, queries, None, None, E64, 3.0, k, 1, 0, two_bins=True)
        # (a rank's own asks may be answered before the tick's last calls are made: one more tick, which starts when that
        # one has ended everywhere, before what the backend heard is read)
        rc._ask(np.asarray(queries[0]), 2, -1, service.ASK_TOPK)
        dist.barrier()
        # the keyword came with every local call of a search under the flag and with none of the flag-clear one
        assert set(backend.heard) == {("align_wide_topk", False), ("align_wide_topk", True), ("align_rates_topk", True),
                                      ("align_span_topk", True)}, backend.heard
        assert rc.broken is None
        out.put((rank, "ok"))
    except BaseException as e:  # noqa: BLE001
        out.put((rank, repr(e)))
        raise
    finally:
        if rc is not None:
            rc.close()
        dist.destroy_process_group()


def test_the_rank_service_carries_the_flag_through_the_tick():
    import torch.multiprocessing as mp

    from tests.near_fakes import free_port_run
    world, port = 2, free_port_run()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in procs]
    [p.join(300) for p in procs]
    assert all(not p.is_alive() for p in procs), "a rank hung"
    res = sorted(q.get(timeout=5) for _ in range(world))
    assert res == [(r, "ok") for r in range(world)], res
