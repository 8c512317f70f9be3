"""Test-only rank parts for tests/test_gap_candidates_rates_launch_gpu.py (`--parts
tests.gap_candidates_rates_launch_parts:rank_parts`): the PRODUCT's rank - DeviceCorpus, the RCCL matcher behind the C
ABI, the real driver with the HIP scene kernels and the launcher's --near-* switches through service.near_kwargs - over
tests/fakes.py's procedural clips, made long enough for eight cuts."""
from tests.fakes import KeyedClipReader


class LongClipReader(KeyedClipReader):
    T = 400


def rank_parts(rank, world, group, a):
    from tvidz_amd import service
    from tvidz_amd.inspector import Inspector
    parts = service._hip_parts(rank, world, group, a)
    parts["inspector"] = lambda store: Inspector(store, device=f"cuda:{a.device}", max_workers=a.workers, batch=32,
                                                 frame_source=lambda b, key, f, u: (LongClipReader(key), None),
                                                 **service.near_kwargs(a))
    return parts
