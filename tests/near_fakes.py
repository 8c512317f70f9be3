"""Test-only stand-ins for the near-duplicate search over a sharded table (never imported by the product):
tests/fakes.py's oracle shard and matcher backend, with sharded.HipBackend's local_align / align_merge answered by the
plain-Python restatements: tests/align_topk_ref.py and tests/align_wide_ref.py for a rank's block of the bounded and
of the wide form, tests/align_topk_shard_ref.py and tests/align_wide_shard_ref.py for their merges."""
import numpy as np
import torch

from tests import align_topk_ref as atr, align_topk_shard_ref as asr, align_wide_ref as awr, align_wide_shard_ref as wsr
from tests.fakes import CutReader, OracleBackend, OracleCorpus, cut_inspector, cuts_of_key
from tvidz_amd.corpus import FORM_BOUNDED, FORM_WIDE


def _queries(d_q, d_off):
    q_all, off = d_q.numpy(), d_off.numpy()
    return [q_all[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


class NearBackend(OracleBackend):
    """fakes.OracleBackend + local_align / align_merge on CPU tensors, for the forms named in `align_forms` (both it
    knows unless told: `align_forms=(FORM_BOUNDED,)` is a backend with the bounded pair only)."""

    def __init__(self, *a, align_forms=(FORM_BOUNDED, FORM_WIDE), **kw):
        super().__init__(*a, **kw)
        self.align_forms = tuple(align_forms)
        self.near_calls = []                # (Q, eps, max_offset, k, min_votes, min_score) of every bounded batch
        self.wide_calls = []                # (Q, eps, max_offset, k, min_votes, min_score, contain) of every wide batch

    def local_align(self, form, d_q, d_off, max_len, k, d_excl, *, eps, max_offset, min_votes, min_score, contain=False):
        queries = _queries(d_q, d_off)
        ids, offs, keys = self._csr()
        rows = [(int(ids[c]), keys[offs[c]:offs[c + 1]].tolist()) for c in range(len(ids))]
        excl = None if d_excl is None else [int(e) for e in d_excl]
        if form == FORM_BOUNDED:
            self.near_calls.append((len(queries), float(eps), float(max_offset), int(k), int(min_votes), int(min_score)))
            block = atr.topk_ref(rows, queries, eps, max_offset, k, min_votes, min_score, excl, max_query_len=max_len)
        else:
            max_offset = awr.MAX_B * float(eps) if max_offset is None else float(max_offset)
            self.wide_calls.append((len(queries), float(eps), max_offset, int(k), int(min_votes), int(min_score),
                                    bool(contain)))
            block = awr.topk_wide_ref(rows, queries, eps, max_offset, k, min_votes, min_score, contain, excl,
                                      max_query_len=max_len)
        return torch.from_numpy(block.astype(np.int32))

    def align_merge(self, form, gathered, k, d_q, d_off, **flags):
        ref = asr.merge_ref if form == FORM_BOUNDED else wsr.merge_ref
        rows, totals = ref(gathered.numpy(), _queries(d_q, d_off), *(flags[n] for n in form.flags))
        return torch.from_numpy(rows.astype(np.int32)), torch.from_numpy(totals.astype(np.int32))


def near_rank_parts(rank, world, group, a):
    """service.py `--parts tests.near_fakes:near_rank_parts`: fakes.cpu_rank_parts with the alignment stand-ins of both
    forms, and the launcher's --near-* switches handed to the driver as service._hip_parts does."""
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
