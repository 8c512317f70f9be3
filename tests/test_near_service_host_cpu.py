"""The host code that sizes and carves the workspaces of tvz_align_rates_topk_sharded, tvz_align_span_topk_sharded and
tvz_align_parts_sharded, under AddressSanitizer and UndefinedBehaviorSanitizer, without a GPU: a stand-alone program with
its own main (tests/near_service_host_main.hip includes the library's translation unit, so the code under test is the
product's own) is built for the host with -fsanitize=address,undefined and run directly; nothing loaded into Python is
sanitized."""
import hashlib
import os
import subprocess
import tempfile

from tvidz_amd import build as tbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "near_service_host_main.hip")


def _program():
    sources = sorted(os.path.join(tbuild.CSRC, f) for f in os.listdir(tbuild.CSRC)) + [os.path.join(tbuild.INCLUDE, "tvz.h"), MAIN]
    h = hashlib.sha1()
    for f in sources:
        h.update(open(f, "rb").read())
    cache = os.path.join(tempfile.gettempdir(), f"tvz-host-sanitizer-{os.getuid()}")
    os.makedirs(cache, exist_ok=True)
    exe = os.path.join(cache, "near-service-" + h.hexdigest()[:16])
    if not os.path.exists(exe):
        # (the device half is compiled because the translation unit registers its kernels; unoptimised: it never runs)
        subprocess.check_call([tbuild._hipcc(), f"--offload-arch={tbuild.ARCH}", "-O1", "-Xarch_device", "-O0", "-std=c++17",
                               "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                               "-Wno-unused-function", f"-I{tbuild.INCLUDE}", f"-I{tbuild.CSRC}", "-o", exe + f".{os.getpid()}.tmp",
                               MAIN, os.path.join(tbuild.CSRC, "tvz_api.hip"), "-ldl"])
        os.replace(exe + f".{os.getpid()}.tmp", exe)
    return exe


def test_sizing_and_carving_of_the_sharded_workspaces_under_asan_and_ubsan():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([_program()], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.strip() == "HOST_OK", (out.stdout, out.stderr[-3000:])
