"""Case tables of the scene edge tests (tests/test_scene_edges_gpu.py runs them on the GPU, tests/test_scene_cases_cpu.py
checks the tables themselves on any machine).

A case is (name, frames ndarray, bitdepth, threshold, how): `how` is a dict that says how the frames are laid out in
memory (`big` and `window`: the frames are the window big[:, oh:oh+H, ow:ow+W] of a larger array, so a view with padded
rows, padded frames or an offset base is the same view on the device) and how they are fed (`runs`: "whole" or a list of
batch sizes through the carried state), plus what the case is built for (`kind` and its parameters).  Every generator is
deterministic: the noise comes from a generator seeded with the case's name.

Next to the tables: a plain numpy reference of the two halves (sad_ref: |a - b| summed in int64; select_ref: the
get_scene_score epilogue in Python floats and np.float32, oracle.scene_select_py extended with a predecessor's mafd and
the threshold) and restatements of what the host code of tvz_scene.hip decides from its arguments alone (flat_ok: which
SAD kernel a view takes; tail_spans: which frames a wave of scene_tail_kernel owns; time_chunks: the launch's grid.y).
The constants assumed are in CONSTANTS; test_scene_cases_cpu.py compares them with the source."""
import zlib
from collections import namedtuple

import numpy as np

from oracle import oracle

Case = namedtuple("Case", "name frames bitdepth threshold how")

CONSTANTS = {
    "kTailBlock": 1024,             # threads of the one-block tail kernel; thread i owns ceil(T/1024) frames
    "kFinT": 64,                    # frames per finalize block
    "max_time_chunks": 65535,       # launch_sad refuses a larger grid.y
    "tc_small": (8, 16, 32),        # decode_shape: tc is one of these or a multiple of ...
    "tc_multiple": 64,
    "U": (1, 2, 4, 8),
}
# the body of flat_ok() in tvz_scene.hip, whitespace collapsed
FLAT_OK_TEXT = ("return rs == (int64_t)W * bps && ((int64_t)H * W * bps) % 16 == 0 && fs % 16 == 0 && "
                "(reinterpret_cast<uintptr_t>(p) % 16) == 0;")
WAVE = 64


# ---------------------------------------------------------------- restatements of the host code
def flat_ok(ptr, fs, rs, H, W, bps):
    """flat_ok() of tvz_scene.hip: tight rows, a plane and a frame stride of whole 16-byte chunks, a 16-byte base."""
    return rs == W * bps and (H * W * bps) % 16 == 0 and fs % 16 == 0 and ptr % 16 == 0


def flat_ok_window(big_shape, window, bps, base=0):
    """flat_ok of the window (oh, ow, H, W) of a contiguous array of big_shape whose first byte is at `base`."""
    _, Hb, Wb = big_shape
    oh, ow, H, W = window
    return flat_ok(base + (oh * Wb + ow) * bps, Hb * Wb * bps, Wb * bps, H, W, bps)


def flat_ok_tensor(x):
    """flat_ok of a [T, H, W] torch tensor or numpy array as SceneScorer.score_batch passes it."""
    if isinstance(x, np.ndarray):
        es, ptr, s0, s1 = x.itemsize, x.ctypes.data, x.strides[0], x.strides[1]
    else:
        es, ptr, s0, s1 = x.element_size(), x.data_ptr(), x.stride(0) * x.element_size(), x.stride(1) * x.element_size()
    return flat_ok(ptr, s0, s1, int(x.shape[1]), int(x.shape[2]), es)


def tail_spans(T):
    """Frame ranges [lo, hi) owned by the 16 waves of scene_tail_kernel (empty ones left out)."""
    c = -(-T // CONSTANTS["kTailBlock"])
    out = []
    for w in range(CONSTANTS["kTailBlock"] // WAVE):
        lo, hi = min(w * WAVE * c, T), min((w + 1) * WAVE * c, T)
        if lo < hi:
            out.append((lo, hi))
    return out


def tail_frames_per_thread(T):
    return -(-T // CONSTANTS["kTailBlock"])


def time_chunks(T, tc):
    return -(-T // tc)


def tc_allowed(tc):
    return tc == 0 or tc in CONSTANTS["tc_small"] or tc % CONSTANTS["tc_multiple"] == 0


# ---------------------------------------------------------------- the plain reference
def sad_ref(frames):
    """uint64[T]: sum over the plane of |cur - prev| in int64, 0 for frame 0.  Plain numpy, a few frames at a time."""
    T = frames.shape[0]
    out = np.zeros(T, dtype=np.uint64)
    plane = max(1, frames.shape[1] * frames.shape[2])
    step = max(1, (1 << 22) // plane)
    for lo in range(1, T, step):
        hi = min(T, lo + step)
        a = frames[lo - 1:hi - 1].astype(np.int64)
        b = frames[lo:hi].astype(np.int64)
        out[lo:hi] = np.abs(a - b).sum(axis=(1, 2)).astype(np.uint64)
    return out


def select_ref(sad, H, W, threshold, bitdepth=8, prev_mafd=None):
    """get_scene_score's epilogue in Python floats (IEEE doubles) and np.float32 -> (selected u8, score f64, mafd f64).
    prev_mafd None: sad[0] belongs to a stream's first frame (score 0).  Else sad[0] is a real SAD and prev_mafd the
    mafd of the frame before it."""
    prev = 0.0 if prev_mafd is None else float(prev_mafd)
    sel, score, mafd = [], [], []
    for t, s in enumerate(sad):
        if t == 0 and prev_mafd is None:
            sel.append(0); score.append(0.0); mafd.append(0.0)
            continue
        m = float(int(s)) / float(W * H) / float(1 << (bitdepth - 8))
        diff = abs(m - prev)
        low = diff if m > diff else m                              # FFMIN
        f = np.float32(low / 100.0)
        f = np.float32(0.0) if f < 0 else (np.float32(1.0) if f > 1 else f)
        prev = m
        mafd.append(m); score.append(float(f)); sel.append(1 if float(f) > threshold else 0)
    return np.array(sel, dtype=np.uint8), np.array(score, dtype=np.float64), np.array(mafd, dtype=np.float64)


_EXPECTED = {}


def expected(case):
    """The oracle's answer for the case's whole stream, computed once: dict of sad, sel, score, mafd, cuts."""
    if case.name not in _EXPECTED:
        T, H, W = case.frames.shape
        sad = oracle.luma_sad(case.frames)
        sel, score, mafd, _ = oracle.scene_select(sad, H, W, case.threshold, bitdepth=case.bitdepth)
        for a in (sad, sel, score, mafd):
            a.setflags(write=False)
        _EXPECTED[case.name] = {"sad": sad, "sel": sel, "score": score, "mafd": mafd,
                                "cuts": np.flatnonzero(sel).tolist()}
    return _EXPECTED[case.name]


# ---------------------------------------------------------------- building blocks
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _dtype(bitdepth):
    return np.uint8 if bitdepth == 8 else np.uint16


def embed(frames, pad_h=0, pad_w=0, off_h=0, off_w=0):
    """-> (big, window): the frames copied into a larger array of pad_h more rows and pad_w more columns, at row off_h
    and column off_w; what surrounds them is junk over the whole sample range."""
    T, H, W = frames.shape
    assert off_h <= pad_h and off_w <= pad_w
    top = int(np.iinfo(frames.dtype).max) + 1
    big = _rng(f"pad/{T}/{H}/{W}/{pad_h}/{pad_w}").integers(0, top, size=(T, H + pad_h, W + pad_w)).astype(frames.dtype)
    big[:, off_h:off_h + H, off_w:off_w + W] = frames
    return big, (off_h, off_w, H, W)


def window(big, win):
    oh, ow, H, W = win
    return big[:, oh:oh + H, ow:ow + W]


def batches(T, n):
    return [min(n, T - s) for s in range(0, T, n)]


def _case(name, big, win, bitdepth, threshold, **how):
    how = dict(how, big=big, window=win)
    how.setdefault("runs", ("whole",))
    return Case(name, window(big, win), bitdepth, threshold, how)


def _whole(name, frames, bitdepth, threshold, **how):
    T, H, W = frames.shape
    return _case(name, frames, (0, 0, H, W), bitdepth, threshold, **how)


def dense_frames(name, T, H, W, bitdepth=8):
    """Levels 0, 0, 100, 100, 0, 0, ... (times 2^(bitdepth-8)) plus noise in [0, 8): every second frame is a cut."""
    mul = 1 << (bitdepth - 8)
    level = (100 * ((np.arange(T) // 2) % 2) * mul).astype(np.int64)
    noise = _rng(name).integers(0, 8, size=(T, H, W))
    return (level[:, None, None] + noise).astype(_dtype(bitdepth))


def random_frames(name, T, H, W, bitdepth):
    """Full-range noise with a level change in the middle (real cuts), as the suite's fuzz makes it."""
    f = _rng(name).integers(0, 1 << bitdepth, size=(T, H, W)).astype(_dtype(bitdepth))
    f[T // 2:] = f[T // 2:] // 3
    return f


def level_frames(levels, H, W, bitdepth):
    out = np.empty((len(levels), H, W), dtype=_dtype(bitdepth))
    for t, v in enumerate(levels):
        out[t] = v
    return out


# ---------------------------------------------------------------- the tables
def wide_cases():
    """A frame's SAD reaches 2^32: the strip partials are u32, their sum is not."""
    base = _rng("wide16").integers(0, 64, size=(6, 264, 256)).astype(np.uint16)
    for t in (1, 4, 5):
        base[t] = 65535 - base[t]
    yield _whole("wide16", base, 16, 0.3, kind="wide", flat=True, runs=("whole", batches(6, 2)),
                 expect_sel=[0, 1, 0, 0, 1, 0])
    yield _case("wide16-generic", base, (0, 0, 264, 255), 16, 0.3, kind="wide", flat=False,
                runs=("whole", batches(6, 2)), expect_sel=[0, 1, 0, 0, 1, 0])
    big8 = np.zeros((3, 4100, 4112), dtype=np.uint8)
    big8[1] = 255
    yield _whole("wide8-4k", big8, 8, 0.3, kind="wide", flat=True, expect_sad=[0, 4299096000, 4299096000])


DENSE_T = (1, 1023, 1024, 1025, 2049, 2500)


def dense_cases():
    """Cuts in every wave of the tail kernel, one and several frames per thread."""
    for T in DENSE_T:
        yield _whole(f"dense-{T}", dense_frames(f"dense-{T}", T, 4, 16), 8, 0.3, kind="dense", flat=True)


def caps_for(n):
    return (0, 1, 7, n - 1, n)


def cap_cases():
    """More cuts than the list holds: the count stays true, the list stops at the cap."""
    yield _whole("cap-2500", dense_frames("dense-2500", 2500, 4, 16), 8, 0.3, kind="cap", flat=True, n_cuts=1249)


LONG_T = 524280          # 65,535 time chunks of 8 frames; one frame more is refused at that shape


def long_cases():
    yield _whole("long-524281", dense_frames("long", LONG_T + 1, 1, 16), 8, 0.3, kind="dense", flat=True,
                 t_ok=LONG_T, shape=(8, 8), n_cuts_ok=262139)


def _down(x):
    return float(np.nextafter(x, 0.0))


THRESHOLD_LEVELS = (0, 25, 25, 75)          # scores 0, 0.25, 0, 0.5
CLIP_LEVELS = (0, 255, 0)                   # scores 0, 1.0 (clipped from 2.55), 0


def threshold_cases():
    """(threshold, a score equals it, expected selection): `>` and not `>=`, and the clip next to 1.0."""
    table = [(THRESHOLD_LEVELS, 8, 0.25, True, [0, 0, 0, 1]), (THRESHOLD_LEVELS, 8, 0.5, True, [0, 0, 0, 0]),
             (THRESHOLD_LEVELS, 8, _down(0.25), False, [0, 1, 0, 1]), (THRESHOLD_LEVELS, 8, _down(0.5), False, [0, 0, 0, 1]),
             (THRESHOLD_LEVELS, 8, 0.0, True, [0, 1, 0, 1]), (THRESHOLD_LEVELS, 8, 1.0, False, [0, 0, 0, 0]),
             (CLIP_LEVELS, 8, 1.0, True, [0, 0, 0]), (CLIP_LEVELS, 8, _down(1.0), False, [0, 1, 0]),
             (tuple(4 * v for v in THRESHOLD_LEVELS), 10, 0.25, True, [0, 0, 0, 1]),
             (tuple(4 * v for v in THRESHOLD_LEVELS), 10, _down(0.25), False, [0, 1, 0, 1])]
    for levels, bd, thr, equal, sel in table:
        name = f"threshold-{'-'.join(map(str, levels))}-bd{bd}-{thr!r}"
        yield _whole(name, level_frames(levels, 8, 16, bd), bd, thr, kind="threshold", flat=True, equal=equal,
                     expect_sel=sel)


FLAT_STRIDE = (((130, 48, 80), 8, 4), ((70, 24, 40), 10, 2))


def flat_stride_cases():
    """The flat kernel with a frame stride larger than the plane: tight rows, padding between frames, and a base that
    is 16-byte but not 256-byte aligned."""
    for (T, H, W), bd, pad in FLAT_STRIDE:
        frames = random_frames(f"stride-{T}-{bd}", T, H, W, bd)
        for off in (0, 2):
            big, win = embed(frames, pad_h=pad, off_h=off)
            yield _case(f"flat-stride-bd{bd}-row{off}", big, win, bd, 0.3, kind="flat-stride", flat=True,
                        runs=("whole", batches(T, 50), batches(T, 1)))


# layouts a batch of the mixed stream is given in: (pad_h, pad_w, off_h, off_w) and the kernel it takes
LAYOUTS = {"contig": ((0, 0, 0, 0), True), "rowpad": ((0, 8, 0, 3), False), "framepad": ((4, 0, 2, 0), True)}
MIXED_CYCLE = (("contig", 17), ("rowpad", 23), ("framepad", 9), ("contig", 1),
               ("framepad", 11), ("rowpad", 1), ("contig", 14), ("rowpad", 8))


def mixed_cases():
    """One stream whose batches change kernel: the carried frame is written by one and read by the other."""
    T, H, W = 120, 48, 80
    plan, at, i = [], 0, 0
    while at < T:
        kind, n = MIXED_CYCLE[i % len(MIXED_CYCLE)]
        n = min(n, T - at)
        plan.append((kind, n))
        at += n
        i += 1
    for bd in (8, 10):
        yield _whole(f"mixed-bd{bd}", random_frames(f"mixed-{bd}", T, H, W, bd), bd, 0.3, kind="mixed", flat=True,
                     plan=tuple(plan))


SHAPE_MATRIX = tuple((U, tc, nt) for U in (1, 2, 4, 8) for tc in (8, 64, 192, 1024) for nt in (True, False))
SHAPE_SPLIT = (61, 89)


def shape_cases():
    for (T, H, W), bd in (((150, 66, 96), 10), ((150, 64, 96), 8)):
        f = random_frames(f"shapes-{bd}", T, H, W, bd)
        f[70:] = f[70:] // 2                                    # a second level change, inside the second part
        yield _whole(f"shapes-bd{bd}", f, bd, 0.3, kind="shapes", flat=True, matrix=SHAPE_MATRIX, split=SHAPE_SPLIT)


# the buffer test's combinations: (name, (H, W), layout, U or 0)
BUFFER_KERNELS = (("flat-U1", (16, 72), "contig", 1), ("flat-U8", (16, 72), "contig", 8),
                  ("generic-rowpad", (16, 72), "rowpad", 0), ("generic-odd", (17, 53), "contig", 0))
BUFFER_T = (1, 63, 65, 130)
BUFFER_WS_OFFSETS = (0, 8, 248)
BUFFER_CAP = 3
BUFFER_MORE = 2          # frames of a second batch, so both of the state's frame buffers get written


def buffer_cases():
    for kname, (H, W), layout, U in BUFFER_KERNELS:
        for bd in (8, 16):
            T = max(BUFFER_T) + BUFFER_MORE
            frames = dense_frames(f"buffers-{kname}-{bd}", T, H, W, bd)
            (ph, pw, oh, ow), _ = LAYOUTS[layout]
            big, win = embed(frames, ph, pw, oh, ow)
            bps = 1 if bd == 8 else 2
            yield _case(f"buffers-{kname}-bd{bd}", big, win, bd, 0.3, kind="buffers",
                        flat=flat_ok_window(big.shape, win, bps), want_flat=kname.startswith("flat"), U=U)


def fuzz_flat_trials(n=16, seed=20240607):
    """The trials added behind the 40 of test_fuzz_shapes_strides_chunking: views that the flat kernel takes (tight
    rows of whole 16-byte chunks, row offsets and frame padding in whole rows), most with a frame stride larger than
    the plane.  -> dicts of H, W, T, bitdepth, pad_h, off_h, step, seed."""
    rng = np.random.default_rng(seed)
    out = []
    for trial in range(n):
        s16 = trial % 3 == 2
        bd = int(rng.choice([10, 12, 16])) if s16 else 8
        W = int(rng.integers(1, 9)) * (8 if s16 else 16)
        H, T = int(rng.integers(1, 60)), int(rng.integers(1, 200))
        off_h = int(rng.integers(0, 4))
        pad_h = off_h + int(rng.integers(0, 4))
        out.append({"H": H, "W": W, "T": T, "bitdepth": bd, "pad_h": pad_h, "off_h": off_h,
                    "step": int(rng.integers(1, T + 1)), "seed": int(rng.integers(1 << 30))})
    return out


def table_cases():
    """Every case that is one stream of frames with one expected answer."""
    for gen in (wide_cases, dense_cases, cap_cases, long_cases, threshold_cases, flat_stride_cases, mixed_cases,
                shape_cases, buffer_cases):
        yield from gen()
