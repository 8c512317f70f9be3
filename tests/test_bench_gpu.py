"""bench.py on the GPU: a plain run times exactly --steps steps of the headline (scene) leg and nothing else, and
--dump-outputs writes what the last step handed its caller - checked bit-exactly against the CPU oracle on the same
seeded frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from tvidz_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, W = 96, 1080, 1920


def test_plain_run_and_dumped_outputs(tmp_path):
    out_dir = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--frames", str(T), "--dump-outputs", str(out_dir)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u8" and d["ms_per_step"] > 0
    assert abs(d["value"] - T * 3 / (d["ms_per_step"] * 1e-3 * 3)) / d["value"] < 1e-6
    for leg in ("match", "config0", "h2d", "e2e"):            # the secondary legs run only with --full
        assert leg not in d, leg
    assert d["cpu_baseline"] is None

    got = {n: np.load(out_dir / f"{n}.npy") for n in ("sad", "mafd", "score", "selected", "cuts")}
    for n, a in got.items():
        assert a.dtype == np.float64, n
    frames, _ = synth.synth_luma(T, H, W, device="cuda:0", seed=synth.FRAME_SEED)
    sad = oracle.luma_sad(frames.cpu().numpy())
    sel, score, mafd, _ = oracle.scene_select(sad, H, W, 0.3)
    assert np.array_equal(got["sad"], sad.astype(np.float64))
    assert np.array_equal(got["mafd"], mafd) and np.array_equal(got["score"], score)
    assert np.array_equal(got["selected"], sel.astype(np.float64))
    assert np.array_equal(got["cuts"], np.flatnonzero(sel).astype(np.float64))
    assert d["cuts_detected_per_step"] == len(got["cuts"])
