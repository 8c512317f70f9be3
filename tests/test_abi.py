"""CPU tests: libtvz.so loads without a GPU and exports every symbol include/tvz.h declares."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "tvz.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(tvz_[a-z0-9_]+)\s*\(", src)))


def _header_version():
    """TVZ_VERSION as include/tvz.h defines it: the number the library, the binding and every C consumer
    must agree on (an ABI change bumps it in the header, and these tests follow without an edit)."""
    m = re.search(r"^#define TVZ_VERSION (\d+)\b", open(os.path.join(ROOT, "include", "tvz.h")).read(), flags=re.M)
    assert m, "include/tvz.h defines no TVZ_VERSION"
    return int(m.group(1))


def test_header_declares_the_path():
    names = _declared()
    for must in ("tvz_luma_sad_u8", "tvz_scene_select", "tvz_scene_scores_u8", "tvz_corpus_create",
                 "tvz_corpus_upload", "tvz_corpus_upsert", "tvz_match", "tvz_find_duplicates",
                 "tvz_topk", "tvz_last_error", "tvz_version", "tvz_scene_state_bytes",
                 "tvz_scene_state_reset", "tvz_match_topk", "tvz_match_workspace_bytes",
                 "tvz_corpus_reserve", "tvz_comm_unique_id", "tvz_comm_init", "tvz_match_sharded"):
        assert must in names


def test_library_builds_loads_exports_every_symbol_at_the_header_version():
    from tvidz_amd import _lib, build
    build.build()
    lib = _lib.load()
    for name in _declared():
        assert hasattr(lib, name), f"{name} declared in tvz.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert lib.tvz_version() == _lib.VERSION == _header_version() > 0
    assert lib.tvz_scene_workspace_bytes(10000, 1080, 1920) > 0
    assert lib.tvz_scene_workspace_bytes(-1, 1080, 1920) == 0
    assert lib.tvz_scene_state_bytes(1080, 1920, 1) >= 2 * 1080 * 1920
    assert lib.tvz_scene_state_bytes(1080, 1920, 3) == 0
    # workspace sizes are pure arithmetic: hash-join tables only (k = 0) < with hit lists + top-k
    a = lib.tvz_match_workspace_bytes(1024, 260, 0, 0, 1)
    b = lib.tvz_match_workspace_bytes(1024, 260, 16384, 16, 8)
    assert 0 < a < b and b - a >= 1024 * 16384 * 12


def test_no_process_global_tuning_knobs():
    """Kernel-shape / algorithm choices are per-call arguments: the library exports
    no *_set_tuning entry point and no mutable global."""
    import subprocess
    from tvidz_amd import _lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH], text=True)
    names = [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert not [n for n in names if "set_tuning" in n or n.startswith("g_")], names
    assert all(n.startswith("tvz_") for n in names if not n.startswith("_")), names


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from tvidz_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SO_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "tvidz_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f
                assert "libtvz_oracle" not in txt, f


def test_bench_refuses_to_run_without_a_gpu():
    """No CPU fallback anywhere: on a GPU-less host bench.py exits with a clear message."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode != 0 and "needs a GPU" in (out.stderr + out.stdout)


def test_entry_points_fail_gracefully_without_a_gpu():
    """On a GPU-less host the library must return an error code + message, never crash and never
    fall back to a CPU path (argument validation and the device probe run before any launch)."""
    import ctypes as C
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from tvidz_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.tvz_corpus_create(C.byref(h), 0)
    assert rc != 0 and h.value is None and len(lib.tvz_last_error()) > 0
    with pytest.raises(RuntimeError, match="libtvz error"):
        _lib.check(rc)
    # pure argument validation (no HIP call is reached)
    assert lib.tvz_luma_sad_u8(None, 4, 32, 32, 1024, 32, None, None, 0, None) != 0
    assert lib.tvz_scene_select(None, 4, 32, 32, 8, 0.3, None, None, None, None, None) != 0
    assert lib.tvz_scene_scores_u8(None, 4, 32, 32, 1024, 32, None, 8, 0.3, None, None, None, None,
                                   None, 0, None, 0, 0, None) != 0
    assert lib.tvz_scene_state_reset(None, None) != 0
    assert lib.tvz_topk(None, None, 1, 4, 8, 0, None, None) != 0          # k out of range
    assert lib.tvz_match(None, None, None, 1, 1, 1, None, 1, None, None, None, 0, 0, None) != 0
    assert lib.tvz_match_topk(None, None, None, 1, 1, 1, None, 1, 4, None, None, 0, 0, None) != 0
    assert lib.tvz_match_sharded(None, None, None, None, 1, 1, 1, None, 1, 4, None, None, None, 0, 0, None) != 0
    assert lib.tvz_corpus_reserve(None, 1, 1) != 0
    n_rows = C.c_int64(-7)
    assert lib.tvz_align(None, None, 0, 0.1, 1.0, None, 0, C.byref(n_rows), None) != 0
    assert n_rows.value == -7                                              # a refusal reports no row count
    from tvidz_amd import scene
    with pytest.raises(RuntimeError):
        scene.SceneScorer(32, 32, 4, "cpu")


def test_topk_entry_points_refuse_k_out_of_range_with_one_message():
    """tvz_topk, tvz_topk_shard and tvz_topk_merge check k against [1, 1024] in front of every pointer check and HIP
    call (so with or without a GPU), and say so in the same words."""
    from tvidz_amd import _lib
    lib = _lib.load()
    for k in (0, 1025):
        calls = (lambda: lib.tvz_topk(None, None, 1, 4, 8, k, None, None),
                 lambda: lib.tvz_topk_shard(None, None, 4, 8, k, None, None),
                 lambda: lib.tvz_topk_merge(None, 2, 4, k, None, None, None))
        msgs = []
        for call in calls:
            assert call() != 0
            msgs.append(lib.tvz_last_error().decode())
        assert f"k={k} " in msgs[0] and "range [1, 1024]" in msgs[0], msgs
        assert msgs[0] == msgs[1] == msgs[2], msgs


def test_diagnostic_builds_report_the_negated_header_version_and_are_quarantined(tmp_path):
    """A library compiled with one of the TVZ_IX_* diagnostic defines (profiles/variant_build.sh: some return WRONG
    results on purpose) reports a negated version, and the product binding refuses to load it; build.build()
    ignores TVZ_CXXFLAGS unless TVZ_DIAGNOSTIC=1 says the build is meant to be one."""
    import subprocess
    import sys
    from tvidz_amd import build as b
    so = str(tmp_path / "libtvz_diag.so")
    # tvz_api.hip alone carries tvz_version(): compile it with the define the kernels' wrong-result path uses
    subprocess.check_call([b._hipcc(), f"--offload-arch={b.ARCH}", "-O1", "-std=c++17", "-fPIC", "-shared",
                           f"-I{b.INCLUDE}", f"-I{b.CSRC}", "-DTVZ_IX_FAKEPOST", "-o", so,
                           os.path.join(b.CSRC, "tvz_api.hip"), "-ldl"])
    code = ("import ctypes, os, sys\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "from tvidz_amd import _lib\n"
            "print(ctypes.CDLL(os.environ['TVZ_LIB']).tvz_version())\n"
            "try:\n    _lib.load()\n    print('LOADED')\nexcept RuntimeError as e:\n    print('REFUSED', 'DIAGNOSTIC' in str(e))\n")
    env = dict(os.environ, TVZ_LIB=so)
    env.pop("TVZ_ALLOW_DIAGNOSTIC", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.stdout.split() == [str(-_header_version()), "REFUSED", "True"], (out.stdout, out.stderr)
    # the product build does not take flags from a stray environment variable
    src = open(os.path.join(ROOT, "tvidz_amd", "build.py")).read()
    assert 'os.environ.get("TVZ_DIAGNOSTIC") == "1"' in src and "TVZ_CXXFLAGS ignored" in src
