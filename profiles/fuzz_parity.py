#!/usr/bin/env python3
"""Randomised differential soak: HIP path vs the oracle / the plain references for N seconds (default 60).
   python profiles/fuzz_parity.py [seconds] [seed] [--family match|near]
`--family match` (the default): the matcher, top-k and scene cases of tests/fuzz_cases.py against the oracle (a seeded
slice of them runs inside `pytest -m gpu`: tests/test_fuzz_gpu.py).  `--family near`: the near-duplicate search - every
alignment and candidate call, their sharded forms and merges - against the references under tests/, with larger tables
than the suite's slice (tests/near_fuzz_cases.py, tests/test_near_fuzz_gpu.py).  Prints a summary line; exits non-zero
at the first mismatch."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

argv = sys.argv[1:]
FAMILY = "match"
if "--family" in argv:
    i = argv.index("--family")
    FAMILY = argv[i + 1]
    del argv[i:i + 2]
if FAMILY not in ("match", "near"):
    sys.exit(f"--family must be match or near, got {FAMILY!r}")
SECONDS = float(argv[0]) if len(argv) > 0 else 60.0
SEED = int(argv[1]) if len(argv) > 1 else 12345
try:
    if FAMILY == "near":
        from tests import near_fuzz_cases  # noqa: E402
        stats = near_fuzz_cases.run(SEED, 1 << 30, big=True, seconds=SECONDS, progress=True)
    else:
        from tests import fuzz_cases  # noqa: E402
        stats = fuzz_cases.run(SECONDS, SEED, progress=True)
except AssertionError as e:
    print(e.args[0] if e.args else e)
    sys.exit(1)
print(json.dumps({"family": FAMILY, "seconds": SECONDS, "seed": SEED, **stats, "result": "no mismatch"}))
