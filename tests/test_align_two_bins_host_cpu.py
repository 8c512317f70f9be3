"""The host code TVZ_ALIGN_TWO_BINS touched - the permitted-flags column of the form table, the flag check, the refusals
of the three calls and their merges that return before any HIP call - under AddressSanitizer and
UndefinedBehaviorSanitizer, in a stand-alone program with its own main (tests/align_two_bins_host_main.hip includes the
library's translation unit, so the code under test is the product's own).  Only the host half is instrumented
(-Xarch_host); the program never touches a GPU and nothing sanitized is loaded into Python.  Built as
tests/test_align_topk_sharded_host_cpu.py builds its program: kept, named by a hash of its sources, in the system's
temporary directory."""
import hashlib
import os
import subprocess
import tempfile

from tvidz_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "align_two_bins_host_main.hip")


def _program():
    sources = sorted(os.path.join(b.CSRC, f) for f in os.listdir(b.CSRC)) + [os.path.join(b.INCLUDE, "tvz.h"), MAIN]
    h = hashlib.sha1()
    for f in sources:
        h.update(open(f, "rb").read())
    cache = os.path.join(tempfile.gettempdir(), f"tvz-host-sanitizer-{os.getuid()}")
    os.makedirs(cache, exist_ok=True)
    exe = os.path.join(cache, "two-bins-" + h.hexdigest()[:16])
    if not os.path.exists(exe):
        # (the device half is compiled because the translation unit registers its kernels; unoptimised: it never runs)
        subprocess.check_call([b._hipcc(), f"--offload-arch={b.ARCH}", "-O1", "-Xarch_device", "-O0", "-std=c++17",
                               "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                               "-Wno-unused-function", f"-I{b.INCLUDE}", f"-I{b.CSRC}", "-o", exe + f".{os.getpid()}.tmp",
                               MAIN, os.path.join(b.CSRC, "tvz_api.hip"), "-ldl"])
        os.replace(exe + f".{os.getpid()}.tmp", exe)
    return exe


def test_the_flag_table_and_the_refusals_under_asan_and_ubsan():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([_program()], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.strip() == "HOST_OK", (out.stdout, out.stderr[-3000:])
