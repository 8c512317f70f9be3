#!/usr/bin/env python3
"""Near-duplicate search with rates, queries against 100k rows x ~200 cuts (the table and queries of
profiles/align_wide_topk.py: stored rows of 200 cuts shifted by an hour, eps 1/30, k = 16):
   wide   tvz_align_wide_topk                                           (the yardstick)
   r1     tvz_align_rates_topk, rates (1.0,)                            (must be the wide call's work)
   r2     ... rates (1.0, 0.96)
   r5     ... rates (1.0, 0.96, 25/24, 1000/1001, 1001/1000)
each at B = 900 and B = 2^22, Q in (1, 16); device events around the enqueued call - whole calls: sort + sweep +
selection -, medians with IQR.  Before timing, r1's blocks are checked against the wide call's bit for bit (columns
0..3; column 4 is 0), and r2 / r5 must report the row shifted by an hour at rate index 0.  One process, one GPU, ONE
leg per run - each leg under a time limit of its own:
   for leg in wide r1 r2 r5; do timeout -k 10 300 python3 profiles/align_rates.py --leg $leg || break; done
   python3 profiles/align_rates.py --report DIR     (no GPU work: the legs' JSON lines in DIR -> the table)"""
import argparse
import ctypes as C
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RATES = {"r1": (1.0,), "r2": (1.0, 0.96), "r5": (1.0, 0.96, 25 / 24, 1000 / 1001, 1001 / 1000)}
ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=("wide",) + tuple(RATES))
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--report", metavar="DIR")
args = ap.parse_args()

if args.report:
    legs = {}
    for f in sorted(glob.glob(os.path.join(args.report, "*.json"))):
        for line in open(f):
            if line.startswith("{"):
                r = json.loads(line)
                legs[r["leg"]] = r
    print("ms per call, median (IQR); xN = against the wide call")
    for case in ("B=900 Q=1", "B=900 Q=16", "B=2^22 Q=1", "B=2^22 Q=16"):
        w = legs["wide"]["ms_per_call"][case]["median"]
        cells = []
        for n in ("wide", "r1", "r2", "r5"):
            s = legs[n]["ms_per_call"][case]
            cells.append(f"{n} {s['median']:.4f} ({s['iqr']:.4f}) x{s['median'] / w:.2f}")
        print(f"{case:12s} " + "   ".join(cells))
    sys.exit(0)

import torch  # noqa: E402

from tvidz_amd import _lib, corpus as tc, synth  # noqa: E402

dev = torch.device("cuda:0")
EPS, K, NQ, SHIFT = 1.0 / 30, 16, 200, 3600.0
BS = {"B=900": 30.0, "B=2^22": tc.ALIGN_WIDE_MAX_B * EPS}
ids, offs, keys = synth.synth_timestamp_corpus(args.rows, seed=synth.CORPUS_SEED)
dc = tc.DeviceCorpus(0)
dc.upload_csr(ids, offs, keys)
lib = _lib.load()
rng = np.random.default_rng(synth.CORPUS_SEED + 7)
src = rng.permutation(np.flatnonzero(np.diff(offs) >= NQ))[:16].tolist()      # rows with at least NQ cuts
queries = [(keys[offs[r]:offs[r + 1]][:NQ] + SHIFT).tolist() for r in src]
stream = torch.cuda.current_stream(dev)


def prep(qs, rates):
    d_q, d_off, longest = tc.pack_queries(qs, dev)
    size = tc.align_rates_topk_workspace_bytes if rates else tc.align_wide_topk_workspace_bytes
    ws = torch.empty(size(len(qs), longest, d_q.numel(), K), dtype=torch.uint8, device=dev)
    return d_q, d_off, longest, ws, torch.empty((len(qs), K + 1, 5 if rates else 4), dtype=torch.int32, device=dev)


def enqueue(p, rates, mo):
    d_q, d_off, longest, ws, out = p
    if rates:
        h = (C.c_double * len(rates))(*rates)
        _lib.check(lib.tvz_align_rates_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), d_off.numel() - 1, longest, EPS, mo, h,
                                            len(rates), 1, 0, 0, None, K, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                            stream.cuda_stream))
    else:
        _lib.check(lib.tvz_align_wide_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), d_off.numel() - 1, longest, EPS, mo,
                                           1, 0, 0, None, K, out.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream))


def timed(p, rates, mo):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    enqueue(p, rates, mo)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(xs):
    q1, med, q3 = np.percentile(np.asarray(xs), [25, 50, 75])
    return {"median": round(float(med), 4), "iqr": round(float(q3 - q1), 4)}


rates = RATES.get(args.leg)
res = {"leg": args.leg, "rows": args.rows, "query_len": NQ, "eps": EPS, "k": K, "reps": args.reps, "rates": rates,
       "ms_per_call": {}}
for bname, mo in BS.items():
    full = bname == "B=2^22"
    if args.leg == "r1":                       # the wide call's blocks, bit for bit
        pr, pw = prep(queries, rates), prep(queries, None)
        enqueue(pr, rates, mo)
        enqueue(pw, None, mo)
        torch.cuda.synchronize()
        assert torch.equal(pr[4][:, :, :4], pw[4]) and bool((pr[4][:, :, 4] == 0).all())
        res["checked"] = "16 blocks equal tvz_align_wide_topk's at both widths"
    for nq in (1, 16):
        p = prep(queries[:nq], rates)
        reps = max(3, args.reps // 4) if full else args.reps
        timed(p, rates, mo)                    # warm-up
        res["ms_per_call"][f"{bname} Q={nq}"] = stats([timed(p, rates, mo) for _ in range(reps)])
        if full:                               # the copy an hour away is in every block, at rate 1.0 where there are rates
            got = p[4].cpu().numpy()
            for i in range(nq):
                hit = [r for r in got[i, :K].tolist() if r[0] == ids[src[i]]]
                assert hit and hit[0][2] == -round(SHIFT / EPS) and hit[0][3] >= NQ and (not rates or hit[0][4] == 0), \
                    (i, got[i].tolist())
print(json.dumps(res))
dc.close()
