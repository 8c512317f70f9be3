"""The case tables of the scene edge tests (tests/scene_cases.py), checked without a GPU: the oracle agrees with a plain
numpy reference on every case, every case has the property it is named for (per the oracle), the restated host decisions
assume the constants and the flat_ok expression that tvz_scene.hip holds, and the generators are deterministic."""
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import scene_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tvidz_amd", "csrc", "tvz_scene.hip")) as _f:
    SRC = _f.read()

CASES = {c.name: c for c in cases.table_cases()}


def _const(name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", SRC)
    assert m, name
    return int(m.group(1))


def test_assumed_constants_are_the_ones_in_the_source():
    C = cases.CONSTANTS
    assert _const("kTailBlock") == C["kTailBlock"] == 1024
    assert _const("kFinT") == C["kFinT"] == 64
    assert _const("kWave") == cases.WAVE
    # the tail kernel's ownership rule and its 16-wave base, as tail_spans restates them
    assert "const int64_t c = (T + kTailBlock - 1) / kTailBlock;" in SRC
    assert "const int64_t t0 = (int64_t)threadIdx.x * c;" in SRC
    assert "if (w < wave) base += v;" in SRC
    # the refusal of a grid beyond 65,535 time chunks, and how the chunks are counted
    m = re.search(r"if \(grid\.y > (\d+)u\)", SRC)
    assert m and int(m.group(1)) == C["max_time_chunks"]
    assert "(unsigned)tvz::ceil_div(T, p.tc)" in SRC and "time chunks" in SRC
    # the allowed shapes
    m = re.search(r"TVZ_REQUIRE\(tn\.tc == 0((?: \|\| tn\.tc == \d+)*) \|\| tn\.tc % (\d+) == 0,", SRC)
    assert m, "decode_shape's tc rule"
    assert tuple(int(x) for x in re.findall(r"== (\d+)", m.group(1))) == C["tc_small"]
    assert int(m.group(2)) == C["tc_multiple"]
    m = re.search(r"TVZ_REQUIRE\(tn\.U == 0((?: \|\| tn\.U == \d+)*),", SRC)
    assert m and tuple(int(x) for x in re.findall(r"== (\d+)", m.group(1))) == C["U"]
    for _, tc, _ in cases.SHAPE_MATRIX:
        assert cases.tc_allowed(tc)
    assert not cases.tc_allowed(100) and cases.tc_allowed(192) and 192 & 191


def test_flat_ok_is_restated_from_the_source_text():
    m = re.search(r"bool flat_ok\(const void \*p, int64_t fs, int64_t rs, int32_t H, int32_t W, int bps\) \{(.*?)\n\}",
                  SRC, re.S)
    assert m, "flat_ok's signature"
    assert " ".join(m.group(1).split()) == cases.FLAT_OK_TEXT
    # the restatement, term by term
    ok = dict(ptr=4096, fs=3840, rs=80, H=48, W=80, bps=1)
    assert cases.flat_ok(**ok)
    for change in (dict(rs=88), dict(H=47, W=81, rs=81), dict(fs=3848), dict(ptr=4104), dict(ptr=4098)):
        assert not cases.flat_ok(**dict(ok, **change)), change
    assert cases.flat_ok(**dict(ok, fs=4160, ptr=4096 + 160))          # padded frames, a 16-byte base: still flat


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_the_plain_reference(name):
    case = CASES[name]
    T, H, W = case.frames.shape
    assert case.frames.dtype == (np.uint8 if case.bitdepth == 8 else np.uint16)
    assert int(case.frames.max()) < (1 << case.bitdepth)
    exp = cases.expected(case)
    assert exp["sad"].dtype == np.uint64 and (exp["sad"] == cases.sad_ref(case.frames)).all()
    if T <= 4096:
        sel, score, mafd = cases.select_ref(exp["sad"], H, W, case.threshold, case.bitdepth)
        assert (sel == exp["sel"]).all()
        assert (score.view(np.uint64) == exp["score"].view(np.uint64)).all()
        assert (mafd.view(np.uint64) == exp["mafd"].view(np.uint64)).all()
        if T > 3:      # continuing a stream: the tail scored behind its predecessor's mafd
            sel2, score2, _ = cases.select_ref(exp["sad"][3:], H, W, case.threshold, case.bitdepth, prev_mafd=exp["mafd"][2])
            assert (sel2 == exp["sel"][3:]).all() and (score2 == exp["score"][3:]).all()
            o = oracle.scene_select(exp["sad"][3:], H, W, case.threshold, case.bitdepth, float(exp["mafd"][2]), True)
            assert (o[0] == sel2).all() and (o[1] == score2).all()


def test_select_ref_is_scene_select_py_with_a_threshold_and_a_predecessor():
    sad = [0, 5000, 123456, 3, 99999, 99999, 0, 70000]
    for bd in (8, 10):
        a_sel, a_score = oracle.scene_select_py(sad, 16, 32, 0.3, bd)
        b_sel, b_score, _ = cases.select_ref(sad, 16, 32, 0.3, bd)
        assert (a_sel == b_sel).all() and (a_score == b_score).all()


@pytest.mark.parametrize("name", list(CASES))
def test_the_case_has_the_property_it_is_named_for(name):
    case = CASES[name]
    how, exp = case.how, cases.expected(case)
    T, H, W = case.frames.shape
    bps = case.frames.itemsize
    kind = how["kind"]
    assert (case.frames == cases.window(how["big"], how["window"])).all()
    # which kernel the view takes (a device allocation is aligned to at least 256 bytes)
    assert cases.flat_ok_window(how["big"].shape, how["window"], bps) == how["flat"]
    if "expect_sel" in how:
        assert exp["sel"].tolist() == how["expect_sel"]
    if "expect_sad" in how:
        assert exp["sad"].tolist() == how["expect_sad"]
    if kind == "wide":
        assert int(exp["sad"].max()) >= 1 << 32
        if case.bitdepth == 16:
            assert H * W >= 65538 and [t for t in range(T) if exp["sad"][t] >= 1 << 32] == [1, 2, 4]
    elif kind == "dense":
        assert exp["cuts"] == list(range(2, T, 2))
        for lo, hi in cases.tail_spans(T):
            if hi > 2:
                assert exp["sel"][lo:hi].any(), (lo, hi)
        if T >= 2048:
            assert len([s for s in cases.tail_spans(T) if s[1] > 2]) >= 10 and cases.tail_frames_per_thread(T) >= 2
        if "t_ok" in how:
            t_ok, (U, tc) = how["t_ok"], how["shape"]
            assert cases.time_chunks(t_ok, tc) == cases.CONSTANTS["max_time_chunks"]
            assert cases.time_chunks(T, tc) == cases.CONSTANTS["max_time_chunks"] + 1 and T == t_ok + 1
            assert cases.tail_frames_per_thread(t_ok) == 512 and len(cases.tail_spans(t_ok)) == 16
            assert int(exp["sel"][:t_ok].sum()) == how["n_cuts_ok"]
    elif kind == "cap":
        n = len(exp["cuts"])
        assert n == how["n_cuts"]
        caps = cases.caps_for(n)
        assert caps == (0, 1, 7, n - 1, n) and sum(n > cap for cap in caps) == 4
        # the cap falls into a later wave's span as well as into the first one's
        spans = cases.tail_spans(T)
        assert exp["cuts"][7] < spans[0][1] and exp["cuts"][n - 1] >= spans[-1][0]
    elif kind == "threshold":
        assert bool((exp["score"] == case.threshold).any()) == how["equal"]
        if how["equal"] and case.threshold > 0:
            t = int(np.flatnonzero(exp["score"] == case.threshold)[0])
            assert exp["sel"][t] == 0
            above = oracle.scene_select(exp["sad"], H, W, float(np.nextafter(case.threshold, 0.0)), case.bitdepth)[0]
            assert above[t] == 1
    elif kind == "flat-stride":
        oh = how["window"][0]
        fs = how["big"].shape[1] * how["big"].shape[2] * bps
        assert fs > H * W * bps and fs % 16 == 0
        assert (oh * W * bps) % 16 == 0 and (oh == 0 or (oh * W * bps) % 256 != 0)
        assert len(exp["cuts"]) >= 1
        assert any(n % 8 for n in how["runs"][1])
    elif kind == "mixed":
        plan = how["plan"]
        assert sum(n for _, n in plan) == T
        seq = [cases.LAYOUTS[k][1] for k, _ in plan]
        assert (True, False) in zip(seq, seq[1:]) and (False, True) in zip(seq, seq[1:])
        assert {(k, n == 1) for k, n in plan} >= {("contig", True), ("rowpad", True), ("contig", False),
                                                  ("rowpad", False), ("framepad", False)}
        for k, n in plan:
            (ph, pw, oh, ow), flat = cases.LAYOUTS[k]
            assert cases.flat_ok_window((n, H + ph, W + pw), (oh, ow, H, W), bps) == flat
        assert len(exp["cuts"]) >= 1
    elif kind == "shapes":
        assert sum(how["split"]) == T and len(exp["cuts"]) >= 2
        assert any(c >= how["split"][0] for c in exp["cuts"]) and any(c < how["split"][0] for c in exp["cuts"])
        assert {tc for _, tc, _ in how["matrix"]} == {8, 64, 192, 1024} and max(tc for _, tc, _ in how["matrix"]) > T
    elif kind == "buffers":
        assert how["flat"] == how["want_flat"]
        for Tb in cases.BUFFER_T:           # but for the one-frame batch, more cuts than the list holds
            assert int(exp["sel"][:Tb].sum()) > cases.BUFFER_CAP or Tb == 1
    else:
        raise AssertionError(kind)


def test_added_fuzz_trials_take_the_flat_kernel_with_a_stride():
    trials = cases.fuzz_flat_trials()
    assert trials == cases.fuzz_flat_trials() and len(trials) >= 12
    strided = 0
    for t in trials:
        bps = 1 if t["bitdepth"] == 8 else 2
        big = (t["T"], t["H"] + t["pad_h"], t["W"])
        assert cases.flat_ok_window(big, (t["off_h"], 0, t["H"], t["W"]), bps), t
        strided += t["pad_h"] > 0 and t["T"] > 1
    assert 4 * strided >= len(trials)
    assert any(t["bitdepth"] > 8 and t["pad_h"] > 0 for t in trials)


def test_the_first_40_fuzz_trials_hold_no_flat_view():
    """Why the trials above were added: a replay of test_fuzz_shapes_strides_chunking's generator (the draws that decide
    the layout) finds no view that the flat kernel would take."""
    rng = np.random.default_rng(424242)
    flat = 0
    for trial in range(40):
        H, W, T = int(rng.integers(1, 97)), int(rng.integers(1, 130)), int(rng.integers(1, 200))
        if trial % 5 == 0:
            H, W = int(rng.integers(1, 40)) * 2, int(rng.integers(1, 40)) * 8
        s16 = trial % 3 == 2
        bd = int(rng.choice([10, 12, 16])) if s16 else 8
        pad_h, pad_w, off_h, off_w = (int(x) for x in rng.integers(0, 5, 4))
        rng.integers(0, 1 << bd, size=(T, H + pad_h + off_h, W + pad_w + off_w))
        rng.integers(1, T + 1)
        flat += cases.flat_ok_window((T, H + pad_h + off_h, W + pad_w + off_w), (off_h, off_w, H, W), 2 if s16 else 1)
    assert flat == 0


def test_the_generators_are_deterministic():
    a = {c.name: c for c in cases.flat_stride_cases()}
    b = {c.name: c for c in cases.flat_stride_cases()}
    assert list(a) == list(b) and all((a[n].how["big"] == b[n].how["big"]).all() for n in a)
    assert (cases.dense_frames("x", 100, 4, 16) == cases.dense_frames("x", 100, 4, 16)).all()
    assert (cases.dense_frames("x", 100, 4, 16) != cases.dense_frames("y", 100, 4, 16)).any()
    assert len(CASES) == len(list(cases.table_cases()))                 # names are unique
