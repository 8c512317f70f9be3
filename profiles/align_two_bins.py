#!/usr/bin/env python3
"""TVZ_ALIGN_TWO_BINS against the flag clear, tvz_align_wide_topk on 100k rows x ~200 cuts (the table of
profiles/align_topk.py), a 200-cut query, eps 1/30, k = 16, Q in (1, 64):
   b900        B = 900   (max_offset 30 s: one window of all bins), flags = 0
   b900two     B = 900, flags = TVZ_ALIGN_TWO_BINS
   wide        B = 2^22  (+-38.8 h: windows of 1,024 bins, every (key, value) pair of a row votes), flags = 0
   widetwo     B = 2^22, flags = TVZ_ALIGN_TWO_BINS
Device events around the enqueued call, medians.  The queries are stored rows shifted by an hour and a third of a bin,
each cut jittered by +-0.6 bins (the legs at B = 900 do not see the copy; the wide ones must report it, and only the
flag sees all of its votes).  One process, one GPU, ONE leg per run - each leg under a time limit of its own, the
same build, the legs alternating, three rounds:
   for r in 1 2 3; do for leg in b900 b900two wide widetwo; do
       timeout -k 10 300 python3 profiles/align_two_bins.py --leg $leg > DIR/$leg.$r.json || break 2; done; done
   python3 profiles/align_two_bins.py --report DIR     (no GPU work: the median of the rounds' medians, spread, ratios)"""
import argparse
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = ("b900", "b900two", "wide", "widetwo")
ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=LEGS)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--report", metavar="DIR")
args = ap.parse_args()

if args.report:
    runs = {}
    for f in sorted(glob.glob(os.path.join(args.report, "*.json"))):
        for line in open(f):
            if line.startswith("{"):
                r = json.loads(line)
                for q, s in r["ms_per_call"].items():
                    runs.setdefault((r["leg"], q), []).append(s["median"])
    for q in ("Q=1", "Q=64"):
        for clear, two, what in (("b900", "b900two", "B=900 "), ("wide", "widetwo", "B=2^22")):
            a, b = sorted(runs[(clear, q)]), sorted(runs[(two, q)])
            ma, mb = float(np.median(a)), float(np.median(b))
            print(f"{what} {q:5s} flag clear {ma:9.4f} ms (rounds {a[0]:.4f} .. {a[-1]:.4f})   two bins {mb:9.4f} ms "
                  f"(rounds {b[0]:.4f} .. {b[-1]:.4f})   ratio {mb / ma:.3f}")
    sys.exit(0)

import torch  # noqa: E402

from tvidz_amd import _lib, corpus as tc, synth  # noqa: E402

dev = torch.device("cuda:0")
EPS, K, NQ, SHIFT = 1.0 / 30, 16, 200, 3600.0 + 1.0 / 90
two = args.leg.endswith("two")
mo = 30.0 if args.leg.startswith("b900") else tc.ALIGN_WIDE_MAX_B * EPS
flags = tc.ALIGN_TWO_BINS if two else 0
ids, offs, keys = synth.synth_timestamp_corpus(args.rows, seed=synth.CORPUS_SEED)
dc = tc.DeviceCorpus(0)
dc.upload_csr(ids, offs, keys)
lib = _lib.load()
rng = np.random.default_rng(synth.CORPUS_SEED + 7)
src = rng.permutation(np.flatnonzero(np.diff(offs) >= NQ))[:64].tolist()      # rows with at least NQ cuts
queries = [(keys[offs[r]:offs[r + 1]][:NQ] + SHIFT + rng.uniform(-0.6, 0.6, size=NQ) * EPS).tolist() for r in src]
stream = torch.cuda.current_stream(dev)


def prep(qs):
    d_q, d_off, longest = tc.pack_queries(qs, dev)
    ws = torch.empty(tc.align_wide_topk_workspace_bytes(len(qs), longest, d_q.numel(), K), dtype=torch.uint8, device=dev)
    return d_q, d_off, longest, ws, torch.empty((len(qs), K + 1, 4), dtype=torch.int32, device=dev)


def enqueue(p):
    d_q, d_off, longest, ws, out = p
    _lib.check(lib.tvz_align_wide_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), d_off.numel() - 1, longest, EPS, mo,
                                       1, 0, flags, None, K, out.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream))


def timed(p):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    enqueue(p)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(xs):
    q1, med, q3 = np.percentile(np.asarray(xs), [25, 50, 75])
    return {"median": round(float(med), 4), "iqr": round(float(q3 - q1), 4)}


res = {"leg": args.leg, "rows": args.rows, "query_len": NQ, "eps": EPS, "max_offset": mo, "k": K, "flags": flags,
       "reps": args.reps, "ms_per_call": {}}
for nq in (1, 64):
    p = prep(queries[:nq])
    reps = args.reps if mo == 30.0 else max(3, args.reps // 4)
    timed(p)                                   # warm-up
    res["ms_per_call"][f"Q={nq}"] = stats([timed(p) for _ in range(reps)])
    if mo != 30.0:                             # the copy an hour away leads its block; its votes: all under the flag
        got = p[4].cpu().numpy()
        votes = []
        for i in range(nq):
            top = got[i, 0].tolist()
            assert top[0] == ids[src[i]] and abs(top[2] + (0.5 if two else 0.0) + SHIFT / EPS) <= 1.0, (i, top)
            votes.append(top[3])
        assert not two or min(votes) >= NQ, votes
        res["checked"] = f"the row shifted by an hour leads every block; its votes {min(votes)}..{max(votes)} of {NQ}"
print(json.dumps(res))
dc.close()
