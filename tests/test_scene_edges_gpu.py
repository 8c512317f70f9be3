"""The scene kernels of tvz_scene.hip at the edges their inputs decide: frame sums beyond 2^32, a cut list with cuts in
every wave of the tail kernel, several frames per tail thread and more cuts than the list holds, scores equal to the
threshold, the flat kernel with a frame stride larger than the plane, one stream that changes kernel between batches,
every kernel shape at both sample sizes, the largest accepted grid and the refusal behind it, and every buffer a call is
given placed inside one arena of 0xA5.  The inputs are the tables of tests/scene_cases.py (checked on the CPU by
tests/test_scene_cases_cpu.py); the expected values are the CPU oracle's.  Every comparison is exact: integers, the bit
patterns of doubles, and lists."""
import numpy as np
import pytest
import torch

from tests import scene_cases as cases
from tvidz_amd import _lib, scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
FILL32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])


def _t(a):
    """numpy frames -> device tensor (uint16 samples travel as the bit patterns of int16)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def _dev_window(big, win):
    oh, ow, H, W = win
    return _t(big)[:, oh:oh + H, ow:ow + W]


def _dev_view(case):
    view = _dev_window(case.how["big"], case.how["window"])
    assert cases.flat_ok_tensor(view) == case.how["flat"], case.name
    return view


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _split(view, sizes):
    parts, at = [], 0
    for n in sizes:
        parts.append(view[at:at + n])
        at += n
    assert at == view.shape[0]
    return parts


def _stream(sc, parts, shape=_lib.SHAPE_AUTO, carry=True):
    """Feed the parts to one scorer; -> the concatenated outputs and the cut list in stream positions."""
    out = {"sad": [], "mafd": [], "score": [], "sel": []}
    cuts, at = [], 0
    for part in parts:
        sad, mafd, score, sel = sc.score_batch(part, carry=carry, shape=shape)
        cuts += [at + i for i in sc.fetch_cuts()]
        out["sad"].append(sad.cpu().numpy().view(np.uint64).copy())
        out["mafd"].append(mafd.cpu().numpy().copy())
        out["score"].append(score.cpu().numpy().copy())
        out["sel"].append(sel.cpu().numpy().copy())
        at += int(part.shape[0])
    got = {k: np.concatenate(v) for k, v in out.items()}
    got["cuts"] = cuts
    return got


def _assert_same(got, exp, lo=0, hi=None, what=None):
    hi = len(exp["sad"]) if hi is None else hi
    assert (got["sad"] == exp["sad"][lo:hi]).all(), what
    assert (_bits(got["mafd"]) == _bits(exp["mafd"][lo:hi])).all(), what
    assert (_bits(got["score"]) == _bits(exp["score"][lo:hi])).all(), what
    assert (got["sel"] == exp["sel"][lo:hi]).all(), what
    assert got["cuts"] == [c - lo for c in exp["cuts"] if lo <= c < hi], what
    assert got["cuts"] == np.flatnonzero(got["sel"]).tolist(), what


def _run(case, run, view=None):
    view = _dev_view(case) if view is None else view
    T, H, W = view.shape
    sizes = [T] if run == "whole" else list(run)
    sc = scene.SceneScorer(H, W, max(sizes), DEV, case.threshold, bitdepth=case.bitdepth)
    return _stream(sc, _split(view, sizes))


def _ids(gen):
    return [c.name for c in gen()]


# ---------------------------------------------------------------- wide sums
@pytest.mark.parametrize("name", _ids(cases.wide_cases))
def test_frame_sums_beyond_32_bits(name):
    case = {c.name: c for c in cases.wide_cases()}[name]
    exp = cases.expected(case)
    assert int(exp["sad"].max()) >= 1 << 32
    view = _dev_view(case)
    for run in case.how["runs"]:
        _assert_same(_run(case, run, view), exp, what=(name, run))


# ---------------------------------------------------------------- the cut list
@pytest.mark.parametrize("name", _ids(cases.dense_cases))
def test_dense_cuts_reach_the_list_in_order(name):
    case = {c.name: c for c in cases.dense_cases()}[name]
    exp = cases.expected(case)
    got = _run(case, "whole")
    _assert_same(got, exp, what=name)
    assert got["cuts"] == list(range(2, case.frames.shape[0], 2))


def test_more_cuts_than_the_list_holds():
    case = next(cases.cap_cases())
    exp = cases.expected(case)
    n = len(exp["cuts"])
    view = _dev_view(case)
    T, H, W = view.shape
    for cap in cases.caps_for(n):
        sc = scene.SceneScorer(H, W, T, DEV, case.threshold, cuts_cap=cap)
        arena = torch.full((64 + 1 + cap + 64,), FILL32, dtype=torch.int32, device=DEV)
        sc.cuts = arena[64:64 + 1 + cap]                     # the list, with guard words on both sides
        _, _, _, sel = sc.score_batch(view)
        torch.cuda.synchronize()
        raw = arena.cpu().numpy()
        assert (sel.cpu().numpy() == exp["sel"]).all()
        assert int(raw[64]) == n, cap                        # the true total, whatever the cap
        kept = min(n, cap)
        assert raw[65:65 + kept].tolist() == exp["cuts"][:kept], cap
        assert (raw[:64] == FILL32).all() and (raw[65 + kept:] == FILL32).all(), cap
        if n > cap:
            with pytest.raises(RuntimeError, match="exceed cuts_cap"):
                sc.fetch_cuts()
        else:
            assert sc.fetch_cuts() == exp["cuts"]


def test_largest_grid_and_the_refusal_behind_it():
    case = next(cases.long_cases())
    exp = cases.expected(case)
    t_ok, (U, tc) = case.how["t_ok"], case.how["shape"]
    view = _dev_view(case)
    T, H, W = view.shape
    sc = scene.SceneScorer(H, W, T, DEV, case.threshold)
    got = _stream(sc, [view[:t_ok]], shape=_lib.shape(U, tc))          # 65,535 time chunks, 512 frames per tail thread
    _assert_same(got, exp, 0, t_ok, "largest grid")
    assert len(got["cuts"]) == case.how["n_cuts_ok"]
    # one frame more at that shape: refused before anything is launched
    sc.reset()
    for buf in (sc.sad, sc.mafd, sc.score):
        buf.view(torch.uint8).fill_(FILL)
    sc.selected.fill_(FILL)
    sc.cuts.fill_(FILL32)
    state = sc.state.clone()
    with pytest.raises(RuntimeError, match="time chunks"):
        sc.score_batch(view, shape=_lib.shape(U, tc))
    torch.cuda.synchronize()
    for buf in (sc.sad, sc.mafd, sc.score):
        assert bool((buf.view(torch.uint8) == FILL).all())
    assert bool((sc.selected == FILL).all()) and bool((sc.cuts == FILL32).all())
    assert bool((sc.state == state).all())
    # the same batch with the automatic shape
    _assert_same(_stream(sc, [view]), exp, what="automatic shape")


# ---------------------------------------------------------------- the threshold
@pytest.mark.parametrize("name", _ids(cases.threshold_cases))
def test_a_score_equal_to_the_threshold_is_not_selected(name):
    case = {c.name: c for c in cases.threshold_cases()}[name]
    exp = cases.expected(case)
    T, H, W = case.frames.shape
    got = _run(case, "whole")
    _assert_same(got, exp, what=name)
    assert got["sel"].tolist() == case.how["expect_sel"]
    assert bool((got["score"] == case.threshold).any()) == case.how["equal"]
    # the standalone epilogue
    sad = torch.from_numpy(exp["sad"].view(np.int64).copy()).to(DEV)
    sel, score, mafd = scene.scene_select(sad, H, W, case.threshold, bitdepth=case.bitdepth)
    torch.cuda.synchronize()
    assert sel.cpu().numpy().tolist() == case.how["expect_sel"]
    assert (_bits(score.cpu().numpy()) == _bits(exp["score"])).all()
    assert (_bits(mafd.cpu().numpy()) == _bits(exp["mafd"])).all()
    if T > 2:      # and continuing a stream: the last frames behind their predecessor's mafd, read from the device
        prev = torch.from_numpy(exp["mafd"][1:2].copy()).to(DEV)
        sel2, score2, _ = scene.scene_select(sad[2:].contiguous(), H, W, case.threshold, bitdepth=case.bitdepth,
                                             prev_mafd=prev)
        torch.cuda.synchronize()
        assert sel2.cpu().numpy().tolist() == case.how["expect_sel"][2:]
        assert (_bits(score2.cpu().numpy()) == _bits(exp["score"][2:])).all()


# ---------------------------------------------------------------- the flat kernel with a stride
@pytest.mark.parametrize("name", _ids(cases.flat_stride_cases))
def test_flat_kernel_with_padding_between_frames(name):
    case = {c.name: c for c in cases.flat_stride_cases()}[name]
    exp = cases.expected(case)
    view = _dev_view(case)
    T, H, W = view.shape
    es = view.element_size()
    assert cases.flat_ok_tensor(view) and view.stride(0) * es > H * W * es and view.stride(1) == W
    assert len(exp["cuts"]) >= 1
    for run in case.how["runs"]:
        _assert_same(_run(case, run, view), exp, what=(name, "whole" if run == "whole" else run[0]))


# ---------------------------------------------------------------- one stream, both kernels
@pytest.mark.parametrize("name", _ids(cases.mixed_cases))
def test_one_stream_alternates_between_the_flat_and_the_generic_kernel(name):
    case = {c.name: c for c in cases.mixed_cases()}[name]
    exp = cases.expected(case)
    T, H, W = case.frames.shape
    parts, at = [], 0
    for kind, n in case.how["plan"]:
        spec, flat = cases.LAYOUTS[kind]
        big, win = cases.embed(case.frames[at:at + n], *spec)
        part = _dev_window(big, win)
        assert cases.flat_ok_tensor(part) == flat, (kind, n)
        parts.append(part)
        at += n
    sc = scene.SceneScorer(H, W, max(n for _, n in case.how["plan"]), DEV, case.threshold, bitdepth=case.bitdepth)
    _assert_same(_stream(sc, parts), exp, what=name)


# ---------------------------------------------------------------- kernel shapes
@pytest.mark.parametrize("name", _ids(cases.shape_cases))
def test_every_shape_at_both_sample_sizes(name):
    case = {c.name: c for c in cases.shape_cases()}[name]
    exp = cases.expected(case)
    view = _dev_view(case)
    T, H, W = view.shape
    sc = scene.SceneScorer(H, W, T, DEV, case.threshold, bitdepth=case.bitdepth)
    for U, tc, nt in case.how["matrix"]:
        shape = _lib.shape(U, tc, nt)
        _assert_same(_stream(sc, [view], shape=shape, carry=False), exp, what=(U, tc, nt, "whole"))
        sc.reset()
        _assert_same(_stream(sc, _split(view, case.how["split"]), shape=shape), exp, what=(U, tc, nt, "split"))


# ---------------------------------------------------------------- buffers
class Arena:
    """One device buffer of 0xA5 that holds every buffer of a call: each slice starts on a 256-byte boundary (plus
    `extra` bytes) and has 256 guard bytes or more on both sides."""

    def __init__(self, sizes, extra=None):
        self.off, at = {}, 512
        for name, n in sizes.items():
            self.off[name] = (at + (extra or {}).get(name, 0), int(n))
            at = (at + 256 + int(n) + 255) // 256 * 256 + 256
        self.buf = torch.full((at + 512,), FILL, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 256 == 0

    def ptr(self, name):
        return self.buf.data_ptr() + self.off[name][0]

    def read(self):
        torch.cuda.synchronize()
        self.host = self.buf.cpu().numpy()
        return self

    def get(self, name, dtype, count):
        lo, n = self.off[name]
        assert count * np.dtype(dtype).itemsize <= n
        return self.host[lo:lo + n].view(dtype)[:count].copy()

    def outside_untouched(self, written=None):
        """Every byte outside the slices is 0xA5, and so is every slice not named in `written`."""
        mask = np.ones(self.host.shape[0], dtype=bool)
        for name, (lo, n) in self.off.items():
            if written is None or name in written:
                mask[lo:lo + n] = False
        return bool((self.host[mask] == FILL).all())


def _abi_call(lib, bitdepth, part, H, W, threshold, ptrs, cap, ws_bytes, shape):
    es = part.element_size()
    fn = lib.tvz_scene_scores_u8 if bitdepth == 8 else lib.tvz_scene_scores_u16
    return fn(part.data_ptr(), int(part.shape[0]), H, W, part.stride(0) * es, part.stride(1) * es, ptrs.get("state"),
              bitdepth, threshold, ptrs.get("sad"), ptrs.get("mafd"), ptrs.get("score"), ptrs.get("sel"),
              ptrs.get("cuts"), cap, ptrs["ws"], ws_bytes, shape, torch.cuda.current_stream().cuda_stream)


def _check_batch(ar, exp, lo, hi, cap, what, before=None):
    """The outputs of the batch [lo, hi) of the stream; behind the cuts written, the list holds what it held `before`
    (0xA5 if it was never written).  -> the raw list."""
    n = hi - lo
    assert (ar.get("sad", np.uint64, n) == exp["sad"][lo:hi]).all(), what
    assert (ar.get("mafd", np.uint64, n) == _bits(exp["mafd"][lo:hi])).all(), what
    assert (ar.get("score", np.uint64, n) == _bits(exp["score"][lo:hi])).all(), what
    assert (ar.get("sel", np.uint8, n) == exp["sel"][lo:hi]).all(), what
    cuts = [c - lo for c in exp["cuts"] if lo <= c < hi]
    raw = ar.get("cuts", np.int32, 1 + cap)
    kept = min(len(cuts), cap)
    assert int(raw[0]) == len(cuts) and raw[1:1 + kept].tolist() == cuts[:kept], what
    assert (raw[1 + kept:] == (FILL32 if before is None else before[1 + kept:])).all(), what
    return raw


@pytest.mark.parametrize("name", _ids(cases.buffer_cases))
def test_the_scene_calls_stay_inside_their_buffers(name):
    case = {c.name: c for c in cases.buffer_cases()}[name]
    exp = cases.expected(case)
    lib = _lib.load()
    view = _dev_view(case)
    _, H, W = view.shape
    bps = view.element_size()
    cap, more = cases.BUFFER_CAP, cases.BUFFER_MORE
    shape = _lib.shape(case.how["U"], 0) if case.how["U"] else _lib.SHAPE_AUTO
    stream = torch.cuda.current_stream().cuda_stream
    for T in cases.BUFFER_T:
        ws_bytes = int(lib.tvz_scene_workspace_bytes(T, H, W))
        st_bytes = int(lib.tvz_scene_state_bytes(H, W, bps))
        assert ws_bytes > 0 and st_bytes > 0
        for extra in cases.BUFFER_WS_OFFSETS:
            what = (name, T, extra)
            ar = Arena({"ws": ws_bytes, "state": st_bytes, "sad": 8 * T, "mafd": 8 * T, "score": 8 * T, "sel": T,
                        "cuts": 4 * (1 + cap)}, extra={"ws": extra})
            ptrs = {k: ar.ptr(k) for k in ar.off}
            _lib.check(lib.tvz_scene_state_reset(ptrs["state"], stream))
            part = view[:T]
            assert cases.flat_ok_tensor(part) == case.how["want_flat"], what
            _lib.check(_abi_call(lib, case.bitdepth, part, H, W, case.threshold, ptrs, cap, ws_bytes, shape))
            assert ar.read().outside_untouched(), what
            first = _check_batch(ar, exp, 0, T, cap, what)
            # a second batch through the state (no longer than the first: the outputs hold T elements): the other
            # frame buffer is written, the predecessor is read back
            T2 = min(more, T)
            _lib.check(_abi_call(lib, case.bitdepth, view[T:T + T2], H, W, case.threshold, ptrs, cap, ws_bytes, shape))
            assert ar.read().outside_untouched(), what
            _check_batch(ar, exp, T, T + T2, cap, what, before=first)


@pytest.mark.parametrize("name", ["buffers-flat-U8-bd8", "buffers-generic-odd-bd16"])
def test_a_workspace_too_small_is_refused_and_nothing_is_written(name):
    case = {c.name: c for c in cases.buffer_cases()}[name]
    lib = _lib.load()
    view = _dev_view(case)
    _, H, W = view.shape
    T, cap = 65, cases.BUFFER_CAP
    ar = Arena({"ws": 256, "state": int(lib.tvz_scene_state_bytes(H, W, view.element_size())), "sad": 8 * T,
                "mafd": 8 * T, "score": 8 * T, "sel": T, "cuts": 4 * (1 + cap)})
    ptrs = {k: ar.ptr(k) for k in ar.off}
    rc = _abi_call(lib, case.bitdepth, view[:T], H, W, case.threshold, ptrs, cap, 256, _lib.SHAPE_AUTO)
    assert rc == -5 and b"workspace" in lib.tvz_last_error()           # TVZ_ERR_WORKSPACE
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.check(rc)
    assert ar.read().outside_untouched(written=())


@pytest.mark.parametrize("name", ["buffers-flat-U8-bd8", "buffers-generic-odd-bd16"])
def test_null_output_combinations_equal_the_full_call(name):
    case = {c.name: c for c in cases.buffer_cases()}[name]
    exp = cases.expected(case)
    lib = _lib.load()
    view = _dev_view(case)
    _, H, W = view.shape
    bps = view.element_size()
    T, more, cap = 65, cases.BUFFER_MORE, 100
    ws_bytes = int(lib.tvz_scene_workspace_bytes(T, H, W))
    sizes = {"ws": ws_bytes, "state": int(lib.tvz_scene_state_bytes(H, W, bps)), "sad": 8 * T, "mafd": 8 * T,
             "score": 8 * T, "sel": T, "cuts": 4 * (1 + cap)}
    stream = torch.cuda.current_stream().cuda_stream

    def call(part, outputs):
        ar = Arena(sizes)
        ptrs = {k: ar.ptr(k) for k in ("ws",) + tuple(outputs)}
        if "state" in outputs:
            _lib.check(lib.tvz_scene_state_reset(ptrs["state"], stream))
        _lib.check(_abi_call(lib, case.bitdepth, part, H, W, case.threshold, ptrs, cap, ws_bytes, _lib.SHAPE_AUTO))
        assert ar.read().outside_untouched(written=("ws",) + tuple(outputs)), outputs
        return ar, ptrs

    ar, _ = call(view[:T], ("sad",))
    assert (ar.get("sad", np.uint64, T) == exp["sad"][:T]).all()
    ar, _ = call(view[:T], ("sel",))
    assert (ar.get("sel", np.uint8, T) == exp["sel"][:T]).all()
    ar, _ = call(view[:T], ("mafd",))
    assert (ar.get("mafd", np.uint64, T) == _bits(exp["mafd"][:T])).all()
    # state only: nothing comes back, and the next batch continues the stream
    ar, ptrs = call(view[:T], ("state",))
    ptrs.update({k: ar.ptr(k) for k in ("sad", "mafd", "score", "sel", "cuts")})
    _lib.check(_abi_call(lib, case.bitdepth, view[T:T + more], H, W, case.threshold, ptrs, cap, ws_bytes, _lib.SHAPE_AUTO))
    assert ar.read().outside_untouched()
    _check_batch(ar, exp, T, T + more, cap, "behind a state-only batch")
    # the scorer without a score buffer (what Inspector uses)
    sc = scene.SceneScorer(H, W, T, DEV, case.threshold, keep_scores=False, bitdepth=case.bitdepth)
    assert sc.score is None
    cuts, at = [], 0
    for part in (view[:T], view[T:T + more]):
        sad, mafd, score, sel = sc.score_batch(part)
        assert score is None
        cuts += [at + i for i in sc.fetch_cuts()]
        lo, hi = at, at + int(part.shape[0])
        assert (sad.cpu().numpy().view(np.uint64) == exp["sad"][lo:hi]).all()
        assert (_bits(mafd.cpu().numpy()) == _bits(exp["mafd"][lo:hi])).all()
        assert (sel.cpu().numpy() == exp["sel"][lo:hi]).all()
        at = hi
    assert cuts == [c for c in exp["cuts"] if c < T + more]
