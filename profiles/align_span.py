#!/usr/bin/env python3
"""Near-duplicate search with spans, queries against 100k rows x ~200 cuts (the table and queries of
profiles/align_rates.py: stored rows of 200 cuts shifted by an hour, eps 1/30, k = 16):
   rates  tvz_align_rates_topk at min_votes 1 and 8                      (the yardstick, per min_votes)
   s1     tvz_align_span_topk, flags 0, min_votes 1                      (nearly every row takes the span pass)
   s8     ... flags 0, min_votes 8
   l8     ... TVZ_ALIGN_LOCAL, min_votes 8
each with the rate lists (1.0,) and (1.0, 0.96), at B = 900 and B = 2^22, Q in (1, 16); device events around the
enqueued call - whole calls: sort + sweep + selection -, medians with IQR.  Before timing, every span leg's blocks are
checked against the rates call's on the same handle, queries and rates: columns 0..4 bit for bit without LOCAL; with
it the order is another one, so at B = 2^22 the row shifted by an hour must lead its block with all its votes and the
whole query as its span.  One process, one GPU, ONE leg per run - each leg under a time limit of its own:
   for leg in rates s1 s8 l8; do timeout -k 10 300 python3 profiles/align_span.py --leg $leg || break; done
   python3 profiles/align_span.py --report DIR     (no GPU work: the legs' JSON lines in DIR -> the table)"""
import argparse
import ctypes as C
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = {"rates": None, "s1": (0, 1), "s8": (0, 8), "l8": (2, 8)}              # (flags, min_votes)
RATES = {"R=1": (1.0,), "R=2": (1.0, 0.96)}
ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=tuple(LEGS))
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
    print("ms per call, median (IQR); xN = against tvz_align_rates_topk with the same rates and min_votes")
    for case in sorted(legs["s1"]["ms_per_call"], key=lambda c: (len(c), c)):
        cells = []
        for n in ("s1", "s8", "l8"):
            mv = LEGS[n][1]
            base = legs["rates"]["ms_per_call"][f"{case} mv={mv}"]
            s = legs[n]["ms_per_call"][case]
            cells.append(f"rates/mv{mv} {base['median']:.4f} ({base['iqr']:.4f})  {n} {s['median']:.4f} ({s['iqr']:.4f}) "
                         f"x{s['median'] / base['median']:.3f}")
        print(f"{case:16s} " + "   ".join(cells))
    for n in ("s1", "s8", "l8"):
        print(f"# {n}: rows that took the span pass, per query (hits counted by the call at min_score 0):", legs[n]["span_rows"])
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


def prep(qs, span):
    d_q, d_off, longest = tc.pack_queries(qs, dev)
    size = tc.align_span_topk_workspace_bytes if span else tc.align_rates_topk_workspace_bytes
    ws = torch.empty(size(len(qs), longest, d_q.numel(), K), dtype=torch.uint8, device=dev)
    return d_q, d_off, longest, ws, torch.empty((len(qs), K + 1, 8 if span else 5), dtype=torch.int32, device=dev)


def enqueue(p, span, rates, mo, flags, min_votes):
    d_q, d_off, longest, ws, out = p
    h = (C.c_double * len(rates))(*rates)
    call = lib.tvz_align_span_topk if span else lib.tvz_align_rates_topk
    _lib.check(call(dc._h, d_q.data_ptr(), d_off.data_ptr(), d_off.numel() - 1, longest, EPS, mo, h, len(rates), min_votes, 0,
                    flags, None, K, out.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream))


def timed(*a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    enqueue(*a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(xs):
    q1, med, q3 = np.percentile(np.asarray(xs), [25, 50, 75])
    return {"median": round(float(med), 4), "iqr": round(float(q3 - q1), 4)}


span = args.leg != "rates"
res = {"leg": args.leg, "rows": args.rows, "query_len": NQ, "eps": EPS, "k": K, "reps": args.reps, "ms_per_call": {},
       "span_rows": {}}
for bname, mo in BS.items():
    full = bname == "B=2^22"
    for rname, rates in RATES.items():
        if span:                                # the rates call's blocks on the same handle, queries and rates first
            flags, mv = LEGS[args.leg]
            ps, pr = prep(queries, True), prep(queries, False)
            enqueue(ps, True, rates, mo, flags, mv)
            enqueue(pr, False, rates, mo, 0, mv)
            torch.cuda.synchronize()
            got = ps[4].cpu().numpy()
            if flags == 0:
                assert torch.equal(ps[4][:, :, :5], pr[4])
                res["checked"] = "16 blocks equal tvz_align_rates_topk's in columns 0..4 at both widths and rate lists"
            elif full:
                for i in range(len(queries)):   # the copy leads: all its votes, the whole query as its span
                    assert got[i, 0, 0] == ids[src[i]] and got[i, 0, 3] >= NQ and got[i, 0, 5:7].tolist() == [0, NQ - 1], got[i, 0]
                res["checked"] = "at B = 2^22 the shifted row leads all 16 blocks with the span 0..199"
            # how many rows took the pass: with min_score 0 every row that passes min_votes does, and the call counts them
            res["span_rows"][f"{bname} {rname}"] = [int(x) for x in got[:, K, 1]]
        for nq in (1, 16):
            variants = [(LEGS[args.leg][0], LEGS[args.leg][1], "")] if span else [(0, 1, " mv=1"), (0, 8, " mv=8")]
            for flags, mv, tag in variants:
                p = prep(queries[:nq], span)
                reps = max(3, args.reps // 4) if full else args.reps
                timed(p, span, rates, mo, flags, mv)                    # warm-up
                res["ms_per_call"][f"{bname} Q={nq} {rname}{tag}"] = stats([timed(p, span, rates, mo, flags, mv) for _ in range(reps)])
print(json.dumps(res))
dc.close()
