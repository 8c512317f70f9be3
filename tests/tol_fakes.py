"""Test-only stand-ins that CAN match tolerantly (never imported by the product): tests/fakes.py's oracle shard
and matcher backend, with the tolerant verdicts taken from the restatement of the contract (tests/tol_ref.py).
At tolerance 0 they are their parents, call for call."""
import torch

from tests import tol_ref
from tests.fakes import NEVER, CutReader, OracleBackend, OracleCorpus, cut_inspector


class TolCorpus(OracleCorpus):
    """fakes.OracleCorpus + DeviceCorpus.find_duplicates' `tolerance` keyword."""
    supports_tolerance = True

    def find_duplicates(self, new_timestamps, min_match=5, exclude_id=-1, with_kth=False, tolerance=0.0):
        if not tolerance:
            return super().find_duplicates(new_timestamps, min_match, exclude_id=exclude_id, with_kth=with_kth)
        with self.lock:
            rows = list(self.rows)
        out = tol_ref.find_duplicates_tol(rows, list(new_timestamps), float(tolerance), int(min_match), int(exclude_id))
        return out if with_kth else [(a, b) for a, b, _ in out]


class TolBackend(OracleBackend):
    """fakes.OracleBackend + sharded.HipBackend.local_topk's `tolerance` keyword: the tolerant block is exact and
    has no cap (tvz_match_tol_topk), the exact one is the parent's match + topk_shard."""
    supports_tolerance = True

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.tolerant_calls = []            # (Q, min_match, tolerance) of every tolerant batch

    def local_topk(self, d_q, d_off, max_len, min_match, cap, k, d_excl, tolerance=0.0):
        if not tolerance:
            hits, n = self.match(d_q, d_off, max_len, min_match, cap, d_excl)
            return self.topk_shard(hits, n, k)
        q_all, off = d_q.numpy(), d_off.numpy()
        Q = len(off) - 1
        self.tolerant_calls.append((Q, int(min_match), float(tolerance)))
        ids, offs, keys = self._csr()
        rows = [(int(ids[c]), keys[offs[c]:offs[c + 1]]) for c in range(len(ids))]
        out = torch.empty((Q, k + 1, 3), dtype=torch.int32)
        for qi in range(Q):
            hits = tol_ref.find_duplicates_tol(rows, q_all[off[qi]:off[qi + 1]], float(tolerance), int(min_match),
                                               int(d_excl[qi]) if d_excl is not None else -1)
            out[qi] = torch.tensor(self._best(hits, k) + [(-1, len(hits), NEVER)], dtype=torch.int32)
        return out


def tol_rank_parts(rank, world, group, a):
    """service.py `--parts tests.tol_fakes:tol_rank_parts`: fakes.cpu_rank_parts with the tolerant stand-ins, and
    the launcher's --match-tolerance handed to the driver as service._hip_parts does."""
    from tvidz_amd import sharded
    shard = TolCorpus()
    matcher = sharded.ShardedMatcher(TolBackend(live=shard), k=a.k, cap=max(a.cap, a.k), group=group)
    return dict(shard=shard, matcher=matcher, xdev="cpu",
                inspector=lambda store: cut_inspector(
                    store, device="cuda:0", max_workers=a.workers, match_tolerance=a.match_tolerance,
                    frame_source=lambda bucket, key, filename, uid: (CutReader(micro_cuts_of_key(key)), None)))


def micro_cuts_of_key(key: str):
    """As fakes.cuts_of_key, with the cut list in MICROSECONDS (`...__<c0>_<c1>_...`): fine enough to tell a
    millisecond remux (1.133) from its original (1.133333)."""
    body = key.split("/")[-1].rsplit(".", 1)[0].split("__", 1)[1]
    return [int(x) / 1e6 for x in body.split("_")]


# ---- the N-rank service on the GPU at world size 1 (tests/test_tol_topk_gpu.py) ------------------------------------
def gpu_tol_rank_parts(rank, world, group, a):
    """service.py `--parts tests.tol_fakes:gpu_tol_rank_parts`: the PRODUCT's rank as fakes.gpu_rank_parts builds it,
    with the launcher's --match-tolerance handed to the driver as service._hip_parts does; a key whose name holds
    `remux` is read as a container with time base 1/1000 would deliver it (pts = round(frame * 1000 / 30))."""
    from tests.fakes import KeyedClipReader
    from tvidz_amd import service
    from tvidz_amd.inspector import Inspector

    class RemuxClipReader(KeyedClipReader):
        def __init__(self, key):
            super().__init__(key)
            self.time_base = (1, 1000)

        def pts_of(self, n):
            return round((self.pts0 + n) * 1000 / 30)

    def source(bucket, key, filename, uid):
        return ((RemuxClipReader if "remux" in key else KeyedClipReader)(key), None)

    parts = service._hip_parts(rank, world, group, a)
    parts["inspector"] = lambda store: Inspector(store, device=f"cuda:{a.device}", max_workers=a.workers, batch=32,
                                                 frame_source=source, match_tolerance=a.match_tolerance)
    return parts
