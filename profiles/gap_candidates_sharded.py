#!/usr/bin/env python3
"""Candidate ids from the gap index over a sharded table, on the table and queries of profiles/gap_candidates.py (100k
rows x ~200 cuts, synth_timestamp_corpus; queries = stored rows of 200 cuts shifted by an hour; eps 1/30):
  1. tvz_align_candidates_merge at n_lists 1, 2, 4, 8, 16, Q = 64 and 4,096, C = 16 and 64, beside tvz_topk_merge at
     the same n_lists, Q and k = C (the same number of rows, 12 bytes each against 8) and the numpy merge on the host
     (corpus.align_candidates_merge); the device merge is held against the host one before anything is timed; a sample
     is 10 calls enqueued back to back between two device events, divided by 10; medians of 20 samples with the IQR;
  2. the candidates call and candidates + parts through service.ShardedCorpus at 8 shards and through a one-rank
     service.RankCorpus (the tick, RcclShardedMatcher), host in / host out, beside align_span_topk (TVZ_ALIGN_LOCAL,
     k = 16) on the SAME corpus object, Q = 1, 16, 64: wall time of the call, the device idle before and after it
     (these paths begin and end on the host); medians with the IQR; the blocks of both are held against one
     DeviceCorpus's first;
  3. gap_index_stats and the device memory of the gap index per shard at 8 shards.
One process, one GPU; the communicator is created before the first GPU call:
   timeout -k 10 900 python3 profiles/gap_candidates_sharded.py > gap_candidates_sharded.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--sweep-reps", type=int, default=3)
ap.add_argument("--shards", type=int, default=8)
args = ap.parse_args()

import torch  # noqa: E402

from tvidz_amd import corpus as tc, service, sharded, synth  # noqa: E402

comm = tc.Comm(tc.Comm.unique_id(), 1, 0, 0)           # ncclCommInitRank: the first GPU call of this process
dev = torch.device("cuda:0")
EPS, GAP_EPS, K, NQ, SHIFT, MIN_VOTES = 1.0 / 30, 1.0 / 30, 16, 200, 3600.0, 8
print(f"gap candidates over shards: {torch.cuda.get_device_name(0)}")


def stats(xs):
    q1, med, q3 = np.percentile(np.asarray(xs), [25, 50, 75])
    return f"{med:9.4f} ({q3 - q1:.4f})"


def device_ms(fn, reps, per=10):
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(per):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / per)
    return out


def wall_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


# ---- 1. the merge ------------------------------------------------------------------------------------------------------
def candidate_blocks(rng, R, Q, c):
    """R sorted lists per query, all full: counts 1..40 (ties in plenty), ids below 2^20"""
    cnt = -np.sort(-rng.integers(1, 41, size=(R, Q, c)), axis=2)
    vid = rng.integers(0, 1 << 20, size=(R, Q, c))
    order = np.lexsort((vid, -cnt), axis=2)
    b = np.zeros((R, Q, c + 1, 2), dtype=np.int32)
    b[:, :, :c, 0], b[:, :, :c, 1] = np.take_along_axis(vid, order, 2), np.take_along_axis(cnt, order, 2)
    b[:, :, c] = (-1, c + 5)
    return b


def topk_blocks(rng, R, Q, k):
    """the same number of rows as tvz_topk_merge takes them: (video_id, count, kth) sorted by (kth, video_id), then the total"""
    kth = np.sort(rng.integers(0, 40, size=(R, Q, k)), axis=2)
    vid = rng.integers(0, 1 << 20, size=(R, Q, k))
    order = np.lexsort((vid, kth), axis=2)
    b = np.zeros((R, Q, k + 1, 3), dtype=np.int32)
    b[:, :, :k, 0], b[:, :, :k, 2] = np.take_along_axis(vid, order, 2), np.take_along_axis(kth, order, 2)
    b[:, :, :k, 1] = 5
    b[:, :, k] = (-1, k + 5, tc.KTH_NEVER if hasattr(tc, "KTH_NEVER") else 0x7FFFFFFF)
    return b


print()
print("1. the merge: us per call, median (IQR); 10 calls between two device events")
print(f"{'Q':>5s} {'C':>3s} {'lists':>5s} {'candidates merge':>22s} {'tvz_topk_merge k=C':>22s} {'numpy on the host':>22s}")
rng = np.random.default_rng(11)
for Q in (64, 4096):
    for c in (16, 64):
        for R in (1, 2, 4, 8, 16):
            h = candidate_blocks(rng, R, Q, c)
            g = torch.from_numpy(h).to(dev)
            out = torch.empty((Q, c + 1, 2), dtype=torch.int32, device=dev)
            host = tc.align_candidates_merge(h)
            assert (tc.align_candidates_merge_device(g, out=out).cpu().numpy() == host).all(), (Q, c, R)
            t_new = device_ms(lambda: tc.align_candidates_merge_device(g, out=out), args.reps)
            g3 = torch.from_numpy(topk_blocks(rng, R, Q, c)).to(dev)
            t_old = device_ms(lambda: tc.topk_merge(g3, c), args.reps)
            t0 = time.perf_counter()
            n_host = 3 if Q > 64 else 10
            for _ in range(n_host):
                tc.align_candidates_merge(h)
            t_host = (time.perf_counter() - t0) / n_host * 1e6
            print(f"{Q:5d} {c:3d} {R:5d} {stats(np.asarray(t_new) * 1e3):>22s} {stats(np.asarray(t_old) * 1e3):>22s} {t_host:>18.0f}")

# ---- 2. and 3. the table, one handle, the shards of one process, one rank ----------------------------------------------------
ids, offs, keys = synth.synth_timestamp_corpus(args.rows, seed=synth.CORPUS_SEED)
rng = np.random.default_rng(synth.CORPUS_SEED + 7)
src = rng.permutation(np.flatnonzero(np.diff(offs) >= NQ))[:64].tolist()          # rows with at least NQ cuts
queries = [(keys[offs[r]:offs[r + 1]][:NQ] + SHIFT).tolist() for r in src]
print()
print(f"the table: {args.rows} rows, {int(offs[-1])} keys, queries of {NQ} cuts shifted by {SHIFT:g} s, eps {EPS:.4f}, gap_eps {GAP_EPS:.4f}")


def csr_of(rows_idx):
    lens = (offs[rows_idx + 1] - offs[rows_idx]).astype(np.int64)
    o = np.zeros(rows_idx.size + 1, dtype=np.int64)
    np.cumsum(lens, out=o[1:])
    k = np.concatenate([keys[offs[r]:offs[r + 1]] for r in rows_idx]) if rows_idx.size else np.zeros(0)
    return ids[rows_idx], o, k


def mib():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0] / 2**20


R = args.shards
sc = service.ShardedCorpus(0, n_shards=R)
free0 = mib()
for s in range(R):
    sc.shards[s].upload_csr(*csr_of(np.flatnonzero(ids % R == s)))                 # a row lives in shard video_id % R
free1 = mib()
t0 = time.perf_counter()
sc.set_gap_index(GAP_EPS)
t_ix = time.perf_counter() - t0
free2 = mib()
st = sc.gap_index_stats()
print(f"3. {R} shards: the rows and their indexes {free0 - free1:.1f} MiB; set_gap_index on all of them {t_ix * 1e3:.1f} ms, "
      f"{free1 - free2:.1f} MiB of device memory = {(free1 - free2) / R:.1f} MiB per shard (one handle over the table: 18,554 MiB)")
print(f"   gap_index_stats summed: {st}")
print(f"   per shard: {[(x['rows'], x['codes']) for x in (s.gap_index_stats() for s in sc.shards)]}")
dc = tc.DeviceCorpus(0)
dc.upload_csr(ids, offs, keys)
f0 = mib()
dc.set_gap_index(GAP_EPS)
print(f"   one handle over the table, this run: {f0 - mib():.1f} MiB")
shard = tc.DeviceCorpus(0)
rc = service.RankCorpus(shard, sharded.RcclShardedMatcher(shard, comm, k=16, cap=4096), xdev="cpu")
shard.upload_csr(ids, offs, keys)
rc.set_gap_index(GAP_EPS)

print()
print("2. ms per call, host in / host out, wall time, median (IQR); the blocks equal one DeviceCorpus's")
print(f"{'corpus':>14s} {'Q':>3s} {'C':>3s} {'cand':>20s} {'cand+parts':>20s} {'align_span_topk k=16':>22s}")
for name, corpus in (("DeviceCorpus", dc), (f"Sharded x{R}", sc), ("RankCorpus x1", rc)):
    for Q in (1, 16, 64):
        qs = queries[:Q]
        t_sweep = wall_ms(lambda: corpus.align_span_topk(qs, eps=EPS, k=K, min_votes=MIN_VOTES, local=True), args.sweep_reps)
        for C in (16, 64):
            want = dc.align_candidates(qs, c=C, min_count=2, cap=4096)
            got = corpus.align_candidates(qs, c=C, min_count=2, cap=4096)
            assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), (name, Q, C)

            def both():
                rows, _ = corpus.align_candidates(qs, c=C, min_count=2, cap=4096)
                return corpus.align_parts(qs, np.ascontiguousarray(rows[:, :, 0]), eps=EPS, min_votes=MIN_VOTES, max_parts=1)
            if not (both() == dc.align_parts(qs, np.ascontiguousarray(want[0][:, :, 0]), eps=EPS, min_votes=MIN_VOTES,
                                             max_parts=1)).all():
                print(f"   PARTS DIFFER from one DeviceCorpus's: {name} Q={Q} C={C}")
            t_c = wall_ms(lambda: corpus.align_candidates(qs, c=C, min_count=2, cap=4096), args.reps)
            t_b = wall_ms(both, args.reps)
            print(f"{name:>14s} {Q:3d} {C:3d} {stats(t_c):>20s} {stats(t_b):>20s} {stats(t_sweep):>22s}")
print(f"   the tick: {rc.busy_ticks} busy ticks, {rc.tick_host_s / max(rc.busy_ticks, 1) * 1e3:.3f} ms of host time per busy tick")
rc.close()
sc.close()
dc.close()
comm.close()
