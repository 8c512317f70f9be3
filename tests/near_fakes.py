"""Test-only stand-ins for the near-duplicate search over a sharded table (never imported by the product):
tests/fakes.py's oracle shard and matcher backend, with sharded.HipBackend's two alignment methods answered by the
plain-Python restatements (tests/align_topk_ref.py for a rank's block, tests/align_topk_shard_ref.py for the merge)."""
import numpy as np
import torch

from tests import align_topk_ref as atr, align_topk_shard_ref as asr
from tests.fakes import CutReader, OracleBackend, OracleCorpus, cut_inspector, cuts_of_key


class NearBackend(OracleBackend):
    """fakes.OracleBackend + local_align_topk / align_topk_merge on CPU tensors."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.near_calls = []                # (Q, eps, max_offset, k, min_votes, min_score) of every batch

    def local_align_topk(self, d_q, d_off, max_len, eps, max_offset, k, min_votes, min_score, d_excl):
        q_all, off = d_q.numpy(), d_off.numpy()
        Q = len(off) - 1
        self.near_calls.append((Q, float(eps), float(max_offset), int(k), int(min_votes), int(min_score)))
        ids, offs, keys = self._csr()
        rows = [(int(ids[c]), keys[offs[c]:offs[c + 1]].tolist()) for c in range(len(ids))]
        queries = [q_all[off[i]:off[i + 1]].tolist() for i in range(Q)]
        excl = None if d_excl is None else [int(e) for e in d_excl]
        block = atr.topk_ref(rows, queries, eps, max_offset, k, min_votes, min_score, excl, max_query_len=max_len)
        return torch.from_numpy(block.astype(np.int32))

    def align_topk_merge(self, gathered, k, d_q, d_off):
        q_all, off = d_q.numpy(), d_off.numpy()
        queries = [q_all[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
        rows, totals = asr.merge_ref(gathered.numpy(), queries)
        return torch.from_numpy(rows.astype(np.int32)), torch.from_numpy(totals.astype(np.int32))


def near_rank_parts(rank, world, group, a):
    """service.py `--parts tests.near_fakes:near_rank_parts`: fakes.cpu_rank_parts with the alignment stand-ins, and
    the launcher's --near-* switches handed to the driver as service._hip_parts does."""
    from tvidz_amd import service, sharded
    shard = OracleCorpus()
    matcher = sharded.ShardedMatcher(NearBackend(live=shard), k=a.k, cap=max(a.cap, a.k), group=group)
    return dict(shard=shard, matcher=matcher, xdev="cpu",
                inspector=lambda store: cut_inspector(
                    store, device="cuda:0", max_workers=a.workers, **service.near_kwargs(a),
                    frame_source=lambda bucket, key, filename, uid: (CutReader(cuts_of_key(key)), None)))


# ---- what the launch test needs: free ports, and the front's surface as tests/test_service_launch_cpu.py drives it ----
def free_port_run(n=1):
    """The first of n consecutive TCP ports on 127.0.0.1 that are free right now (all n bound at once to find out)."""
    import random
    import socket
    for _ in range(200):
        base = random.randint(20000, 60000)
        socks = []
        try:
            for i in range(n):
                s = socket.socket()
                socks.append(s)
                s.bind(("127.0.0.1", base + i))
            return base
        except OSError:
            continue
        finally:
            for s in socks:
                s.close()
    raise RuntimeError(f"no run of {n} free ports found")


def upload_key(name, cuts, stamp=1700000000):
    """An S3 key that carries its cut list in tenths of seconds (fakes.cuts_of_key reads it back)."""
    return f"videos/{stamp}-{name}__{'_'.join(str(int(round(c * 10))) for c in cuts)}.mp4"


def notify(base, key):
    import requests
    r = requests.post(f"{base}/notify", json={"Records": [{"s3": {"bucket": {"name": "videos"}, "object": {"key": key}}}]},
                      timeout=30)
    assert r.status_code == 200 and r.json() == {"status": "Analysis started", "file": key}


def wait_done(base, filename, timeout=60):
    import time

    import requests
    deadline = time.time() + timeout
    while time.time() < deadline:
        rec = requests.get(f"{base}/status/{filename}", timeout=30).json()
        if rec.get("status") in ("done", "error"):
            return rec
        time.sleep(0.05)
    raise AssertionError(f"{filename} never finished")
