#!/usr/bin/env python3
"""What the near-duplicate search costs through the rank service, recorded in profiles/near_service.txt (no pass criterion):
  1. tvz_align_parts_merge for 1, 2, 4 and 8 lists at Q = 16, k = 16, max_parts = 4: device events around bursts of launches,
     next to corpus.align_parts_merge (numpy) on the same blocks on the host clock; the outputs are compared first;
  2. a span ask and a parts ask through the tick of a one-rank service.RankCorpus over sharded.RcclShardedMatcher, host to
     host, next to the direct DeviceCorpus calls on the same table (100k rows of ~40 cuts unless --rows says otherwise) and
     upload; the answers are compared first.
   python3 profiles/near_service.py [--rows N] [--repeat R]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tvidz_amd import corpus as tc, service, sharded, synth  # noqa: E402


def med_iqr(xs):
    q = statistics.quantiles(xs, n=4)
    return f"median {statistics.median(xs):9.1f} us  (IQR {q[0]:.1f}..{q[2]:.1f}, n={len(xs)})"


def blocks(rng, R, Q, k, P):
    a = np.zeros((R, Q, k, 1 + P, 6), dtype=np.int32)
    a[:, :, :, 0, 0] = rng.integers(0, 100000, size=(Q, k))[None]
    n_rows = rng.integers(0, 3, size=(R, Q, k))
    a[:, :, :, 0, 4] = n_rows
    a[:, :, :, 0, 3] = np.where(n_rows > 0, P, 0)
    a[:, :, :, 1:, :] = np.where((n_rows > 0)[..., None, None], rng.integers(1, 400, size=(R, Q, k, P, 6)), 0)
    return a


def merge_leg(dev, repeat):
    rng = np.random.default_rng(7)
    Q = k = 16
    P = 4
    print(f"1. the parts merge, Q = {Q}, k = {k}, max_parts = {P}: one launch (device events over bursts of 200) | numpy on the host")
    for R in (1, 2, 4, 8):
        a = blocks(rng, R, Q, k, P)
        d = torch.from_numpy(a).to(dev)
        out = torch.empty((Q, k, 1 + P, 6), dtype=torch.int32, device=dev)
        assert (tc.align_parts_merge_device(d, out=out).cpu().numpy() == tc.align_parts_merge(a)).all()
        dev_us, host_us = [], []
        for _ in range(repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                tc.align_parts_merge_device(d, out=out)
            e1.record()
            e1.synchronize()
            dev_us.append(e0.elapsed_time(e1) * 1000.0 / 200)
            t0 = time.perf_counter()
            for _ in range(20):
                tc.align_parts_merge(a)
            host_us.append((time.perf_counter() - t0) * 1e6 / 20)
        print(f"   lists={R}: device {med_iqr(dev_us)} | numpy {med_iqr(host_us)}")


def tick_leg(dev, n_rows, repeat):
    comm = sharded.make_comm(0)               # (first: the communicator before this process's other GPU work)
    ids, offs, keys = synth.synth_timestamp_corpus(n_rows, seed=1, mean_len=40)
    c = int(np.flatnonzero(np.diff(offs) >= 40)[0])           # a stored video of 40 cuts or more
    stored = keys[offs[c]:offs[c + 1]]
    upload = np.concatenate([stored[:len(stored) // 2], stored[len(stored) // 2:] + 47.3]).tolist()      # a part put in
    kw = dict(eps=1 / 30, rates=(1.0, 0.96), k=16, min_votes=4, local=True)
    pkw = dict(eps=1 / 30, rates=(1.0, 0.96), min_votes=4, max_parts=2)
    plain = tc.DeviceCorpus(0)
    plain.upload_csr(ids, offs, keys)
    shard = tc.DeviceCorpus(0)
    shard.upload_csr(ids, offs, keys)
    rc = service.RankCorpus(shard, sharded.RcclShardedMatcher(shard, comm, k=16, cap=1024, priority=-1), xdev="cpu")
    try:
        rows, totals = plain.align_span_topk([upload], **kw)
        hit_ids = [rows[0, :, 0].tolist()]
        r2, t2 = rc.align_span_topk([upload], **kw)
        assert (r2 == rows).all() and (t2 == totals).all()
        parts = plain.align_parts([upload], hit_ids, **pkw)
        assert (rc.align_parts([upload], hit_ids, **pkw) == parts).all()
        at = hit_ids[0].index(int(ids[c])) if int(ids[c]) in hit_ids[0] else -1
        print(f"   (the search reports {int(totals[0])} rows, the source video at place {at}"
              + (f" with {int(parts[0, at, 0, 3])} parts" if at >= 0 else "") + "; both routes agree)")
        legs = {"span ask, direct DeviceCorpus": lambda: plain.align_span_topk([upload], **kw),
                "span ask, through the tick": lambda: rc.align_span_topk([upload], **kw),
                "parts ask, direct DeviceCorpus": lambda: plain.align_parts([upload], hit_ids, **pkw),
                "parts ask, through the tick": lambda: rc.align_parts([upload], hit_ids, **pkw)}
        print(f"2. one upload of {len(upload)} cuts against {n_rows} rows, host to host (the call returns numpy arrays), k = 16, "
              f"rates (1.0, 0.96), world size 1:")
        times = {n: [] for n in legs}
        for _ in range(repeat):                                   # alternating, so that drift lands on every leg alike
            for n, f in legs.items():
                for _ in range(3):
                    f()
                t0 = time.perf_counter()
                for _ in range(10):
                    f()
                times[n].append((time.perf_counter() - t0) * 1e6 / 10)
        for n, xs in times.items():
            print(f"   {n:32s} {med_iqr(xs)}")
        print(f"   ticks {rc.ticks}, busy {rc.busy_ticks}, broken {rc.broken!r}")
    finally:
        rc.close()
        plain.close()
        comm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--repeat", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("near_service.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    tick_leg(dev, a.rows, a.repeat)
    merge_leg(dev, a.repeat)


if __name__ == "__main__":
    main()
