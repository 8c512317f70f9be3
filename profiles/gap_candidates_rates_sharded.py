#!/usr/bin/env python3
"""Candidate ids at a list of rates over a sharded table, on one GPU in ONE process:
  1. tvz_align_candidates_rates_merge (ts_gapr_merge_kernel, a block per query) at n_lists 1, 2, 4, 8, 16, Q = 64 and
     4,096, C = 16 and 64, beside tvz_align_candidates_merge (the wave-per-query kernel, unchanged) and tvz_topk_merge
     at the same n_lists, Q and k = C, in the same run; the new merge is held against the numpy one before it is timed; a
     sample is 10 calls enqueued back to back between two device events, divided by 10; medians of 20 with the IQR.
     Per cell from 8 lists on: is the new merge no slower than the plain one by more than the larger IQR?
  2. on the table and queries of profiles/gap_candidates_rates.py (100k rows x ~200 cuts; stored rows of 200 cuts played
     at 25/24 and shifted): align_candidates_rates alone and followed by align_parts on the same list, host in / host out,
     wall time, through one DeviceCorpus, service.ShardedCorpus at 8 shards and a one-rank service.RankCorpus (the tick,
     RcclShardedMatcher), Q = 1, 16, 64 at 1, 3 and 8 rates, C = 16; medians with the IQR; beside them ONE timed call of
     the same object's align_span_topk sweep (TVZ_ALIGN_LOCAL, k = 16) with that list.  Every block is first held
     against one DeviceCorpus's.
The communicator is created before the first GPU call:
   timeout -k 10 1100 python3 profiles/gap_candidates_rates_sharded.py > gap_candidates_rates_sharded.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--shards", type=int, default=8)
ap.add_argument("--no-sweep", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

from tvidz_amd import corpus as tc, service, sharded, synth  # noqa: E402

comm = tc.Comm(tc.Comm.unique_id(), 1, 0, 0)           # ncclCommInitRank: the first GPU call of this process
dev = torch.device("cuda:0")
EPS, GAP_EPS, K, C, NQ, SHIFT, MIN_VOTES, SPEED = 1.0 / 30, 1.0 / 30, 16, 16, 200, 3600.0, 8, 25 / 24
RATE_LISTS = ((SPEED,), (1.0, 24 / 25, SPEED), (1.0, 24 / 25, SPEED, 1000 / 1001, 1001 / 1000, 1.25, 0.8, 1.1))
print(f"gap candidates at a list of rates over shards: {torch.cuda.get_device_name(0)}", flush=True)


def quart(xs):
    q1, med, q3 = np.percentile(np.asarray(xs), [25, 50, 75])
    return med, q3 - q1


def stats(xs):
    med, iqr = quart(xs)
    return f"{med:9.4f} ({iqr:.4f})"


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


def wall_ms(fn, reps, warm=True):
    if warm:
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
def rated_blocks(rng, R, Q, c):
    """R sorted lists per query, all full: bests 1..40 (ties in plenty), ids below 2^20 - distinct ids, as shards give"""
    best = rng.integers(1, 41, size=(R, Q, c))
    vid = rng.integers(0, 1 << 20, size=(R, Q, c))
    order = np.lexsort((vid, -best), axis=2)
    b = np.zeros((R, Q, c + 1, 3), dtype=np.int32)
    b[:, :, :c, 0], b[:, :, :c, 1] = np.take_along_axis(vid, order, 2), np.take_along_axis(best, order, 2)
    b[:, :, :c, 2] = rng.integers(0, 8, size=(R, Q, c))
    b[:, :, c] = (-1, c + 5, 0)
    return b


def topk_blocks(rng, R, Q, k):
    kth = np.sort(rng.integers(0, 40, size=(R, Q, k)), axis=2)
    vid = rng.integers(0, 1 << 20, size=(R, Q, k))
    order = np.lexsort((vid, kth), axis=2)
    b = np.zeros((R, Q, k + 1, 3), dtype=np.int32)
    b[:, :, :k, 0], b[:, :, :k, 2] = np.take_along_axis(vid, order, 2), np.take_along_axis(kth, order, 2)
    b[:, :, :k, 1] = 5
    b[:, :, k] = (-1, k + 5, 0x7FFFFFFF)
    return b


print()
print("1. the merge: us per call, median (IQR); 10 calls between two device events")
print(f"{'Q':>5s} {'C':>3s} {'lists':>5s} {'rates merge (block)':>22s} {'plain merge (wave)':>22s} {'tvz_topk_merge k=C':>22s}  no slower than plain")
rng = np.random.default_rng(11)
for Q in (64, 4096):
    for c in (16, 64):
        for R in (1, 2, 4, 8, 16):
            h = rated_blocks(rng, R, Q, c)
            g = torch.from_numpy(h).to(dev)
            out = torch.empty((Q, c + 1, 3), dtype=torch.int32, device=dev)
            assert (tc.align_candidates_rates_merge_device(g, out=out).cpu().numpy() == tc.align_candidates_rates_merge(h)).all(), (Q, c, R)
            g2 = torch.from_numpy(np.ascontiguousarray(h[:, :, :, :2])).to(dev)      # the same rows without the rate column
            out2 = torch.empty((Q, c + 1, 2), dtype=torch.int32, device=dev)
            g3 = torch.from_numpy(topk_blocks(rng, R, Q, c)).to(dev)
            t_new = np.asarray(device_ms(lambda: tc.align_candidates_rates_merge_device(g, out=out), args.reps)) * 1e3
            t_old = np.asarray(device_ms(lambda: tc.align_candidates_merge_device(g2, out=out2), args.reps)) * 1e3
            t_top = np.asarray(device_ms(lambda: tc.topk_merge(g3, c), args.reps)) * 1e3
            (m_new, i_new), (m_old, i_old) = quart(t_new), quart(t_old)
            verdict = "" if R < 8 else ("holds" if m_new <= m_old + max(i_new, i_old) else f"FAILS ({m_new / m_old:.2f}x)")
            print(f"{Q:5d} {c:3d} {R:5d} {stats(t_new):>22s} {stats(t_old):>22s} {stats(t_top):>22s}  {verdict}", flush=True)

# ---- 2. the compositions -----------------------------------------------------------------------------------------------
ids, offs, keys = synth.synth_timestamp_corpus(args.rows, seed=synth.CORPUS_SEED)
rng = np.random.default_rng(synth.CORPUS_SEED + 7)
src = rng.permutation(np.flatnonzero(np.diff(offs) >= NQ))[:64].tolist()          # rows with at least NQ cuts
queries = [((keys[offs[r]:offs[r + 1]][:NQ] - SHIFT) / SPEED).tolist() for r in src]
print()
print(f"the table: {args.rows} rows, {int(offs[-1])} keys, queries of {NQ} cuts played at 25/24 and moved by {SHIFT:g} s, "
      f"eps {EPS:.4f}, gap_eps {GAP_EPS:.4f}, C = K = {C}")


def csr_of(rows_idx):
    lens = (offs[rows_idx + 1] - offs[rows_idx]).astype(np.int64)
    o = np.zeros(rows_idx.size + 1, dtype=np.int64)
    np.cumsum(lens, out=o[1:])
    k = np.concatenate([keys[offs[r]:offs[r + 1]] for r in rows_idx]) if rows_idx.size else np.zeros(0)
    return ids[rows_idx], o, k


R = args.shards
sc = service.ShardedCorpus(0, n_shards=R)
for s in range(R):
    sc.shards[s].upload_csr(*csr_of(np.flatnonzero(ids % R == s)))                 # a row lives in shard video_id % R
sc.set_gap_index(GAP_EPS)
dc = tc.DeviceCorpus(0)
dc.upload_csr(ids, offs, keys)
dc.set_gap_index(GAP_EPS)
shard = tc.DeviceCorpus(0)
rk = service.RankCorpus(shard, sharded.RcclShardedMatcher(shard, comm, k=16, cap=4096), xdev="cpu")
shard.upload_csr(ids, offs, keys)
rk.set_gap_index(GAP_EPS)

print()
print("2. ms per call, host in / host out, wall time, median (IQR); the sweep: ONE timed call; the blocks equal one DeviceCorpus's")
print(f"{'corpus':>14s} {'Q':>3s} {'R':>2s} {'cand R':>20s} {'cand+parts':>20s} {'align_span_topk k=16':>22s} {'true row first':>15s}")
for name, corpus in (("DeviceCorpus", dc), (f"Sharded x{R}", sc), ("RankCorpus x1", rk)):
    for Q in (1, 16, 64):
        qs = queries[:Q]
        for rates in RATE_LISTS:
            want = dc.align_candidates_rates(qs, rates, c=C, min_count=2, cap=4096)
            got = corpus.align_candidates_rates(qs, rates, c=C, min_count=2, cap=4096)
            assert all((a == b).all() for a, b in zip(got, want)), (name, Q, len(rates))

            def both():
                block_ids = corpus.align_candidates_rates(qs, rates, c=C, min_count=2, cap=4096)[0]
                return corpus.align_parts(qs, block_ids, eps=EPS, rates=rates, min_votes=MIN_VOTES, max_parts=1)
            if not (both() == dc.align_parts(qs, want[0], eps=EPS, rates=rates, min_votes=MIN_VOTES, max_parts=1)).all():
                print(f"   PARTS DIFFER from one DeviceCorpus's: {name} Q={Q} R={len(rates)}")
            t_c = wall_ms(lambda: corpus.align_candidates_rates(qs, rates, c=C, min_count=2, cap=4096), args.reps)
            t_b = wall_ms(both, args.reps)
            t_s = "-" if args.no_sweep else "%9.1f" % wall_ms(
                lambda: corpus.align_span_topk(qs, eps=EPS, rates=rates, k=K, min_votes=MIN_VOTES, local=True), 1, warm=False)[0]
            first = sum(int(got[0][q, 0]) == int(ids[src[q]]) and int(got[2][q, 0]) == rates.index(SPEED) for q in range(Q))
            print(f"{name:>14s} {Q:3d} {len(rates):2d} {stats(t_c):>20s} {stats(t_b):>20s} {t_s:>22s} {first:>11d}/{Q:<3d}", flush=True)
print(f"   the tick: {rk.busy_ticks} busy ticks, {rk.tick_host_s / max(rk.busy_ticks, 1) * 1e3:.3f} ms of host time per busy tick")
rk.close()
sc.close()
dc.close()
comm.close()
