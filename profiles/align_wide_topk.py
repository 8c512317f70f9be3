#!/usr/bin/env python3
"""Near-duplicate search at any shift, queries against 100k rows x ~200 cuts (the table of profiles/align_topk.py):
   bounded   tvz_align_topk       at B = 900   (eps 1/30, max_offset 30 s: the parent's code, the yardstick)
   wide900   tvz_align_wide_topk  at B = 900   (one window: the same work through the new sweep)
   wide      tvz_align_wide_topk  at B = 2^22  (eps 1/30: +-38.8 h, every (key, value) pair of a row votes)
Q in (1, 16), k = 16, device events around the enqueued call, medians.  The query is a stored row shifted by an hour
(the legs at B = 900 do not see it; `wide` must report it).  Before timing, wide900's blocks are checked
against bounded's bit for bit.  One process, one GPU, ONE leg per run - each leg under a time limit of its own:
   for leg in bounded wide900 wide; do timeout -k 10 300 python3 profiles/align_wide_topk.py --leg $leg || break; done
   python3 profiles/align_wide_topk.py --report DIR     (no GPU work: the legs' JSON lines in DIR -> times and ratios)"""
import argparse
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=("bounded", "wide900", "wide"))
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
    for q in ("Q=1", "Q=16"):
        b, w9, w = (legs[n]["ms_per_call"][q]["median"] for n in ("bounded", "wide900", "wide"))
        print(f"{q}: bounded B=900 {b:.4f} ms   wide B=900 {w9:.4f} ms ({w9 / b:.2f}x)   wide B=2^22 {w:.3f} ms ({w / b:.1f}x)"
              f"   per query at full width {w / int(q[2:]):.3f} ms")
    sys.exit(0)

import torch  # noqa: E402

from tvidz_amd import _lib, corpus as tc, synth  # noqa: E402

dev = torch.device("cuda:0")
EPS, K, NQ, SHIFT = 1.0 / 30, 16, 200, 3600.0
B900 = 30.0
WIDE = tc.ALIGN_WIDE_MAX_B * EPS
ids, offs, keys = synth.synth_timestamp_corpus(args.rows, seed=synth.CORPUS_SEED)
dc = tc.DeviceCorpus(0)
dc.upload_csr(ids, offs, keys)
lib = _lib.load()
rng = np.random.default_rng(synth.CORPUS_SEED + 7)
src = rng.permutation(np.flatnonzero(np.diff(offs) >= NQ))[:16].tolist()      # rows with at least NQ cuts
queries = [(keys[offs[r]:offs[r + 1]][:NQ] + SHIFT).tolist() for r in src]
stream = torch.cuda.current_stream(dev)


def prep(qs, wide):
    d_q, d_off, longest = tc.pack_queries(qs, dev)
    size = tc.align_wide_topk_workspace_bytes if wide else tc.align_topk_workspace_bytes
    ws = torch.empty(size(len(qs), longest, d_q.numel(), K), dtype=torch.uint8, device=dev)
    return d_q, d_off, longest, ws, torch.empty((len(qs), K + 1, 4), dtype=torch.int32, device=dev)


def enqueue(p, wide, mo):
    d_q, d_off, longest, ws, out = p
    if wide:
        _lib.check(lib.tvz_align_wide_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), d_off.numel() - 1, longest, EPS, mo,
                                           1, 0, 0, None, K, out.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream))
    else:
        _lib.check(lib.tvz_align_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), d_off.numel() - 1, longest, EPS, mo,
                                      1, 0, None, K, out.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream))


def timed(p, wide, mo):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    enqueue(p, wide, mo)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(xs):
    q1, med, q3 = np.percentile(np.asarray(xs), [25, 50, 75])
    return {"median": round(float(med), 4), "iqr": round(float(q3 - q1), 4)}


wide = args.leg != "bounded"
mo = WIDE if args.leg == "wide" else B900
res = {"leg": args.leg, "rows": args.rows, "query_len": NQ, "eps": EPS, "max_offset": mo, "k": K, "reps": args.reps,
       "ms_per_call": {}}
if args.leg == "wide900":                      # the same blocks as the bounded call, bit for bit
    pw, pb = prep(queries, True), prep(queries, False)
    enqueue(pw, True, B900)
    enqueue(pb, False, B900)
    torch.cuda.synchronize()
    assert torch.equal(pw[4], pb[4])
    res["checked"] = "16 blocks equal tvz_align_topk's"
for nq in (1, 16):
    p = prep(queries[:nq], wide)
    reps = args.reps if args.leg != "wide" else max(3, args.reps // 4)
    timed(p, wide, mo)                         # warm-up
    res["ms_per_call"][f"Q={nq}"] = stats([timed(p, wide, mo) for _ in range(reps)])
    if args.leg == "wide":                     # the copy an hour away is row 0 of every block
        got = p[4].cpu().numpy()
        for i in range(nq):
            hit = [r for r in got[i, :K].tolist() if r[0] == ids[src[i]]]
            assert hit and hit[0][2] == -round(SHIFT / EPS) and hit[0][3] >= NQ, (i, got[i].tolist())
        res["checked"] = "the row shifted by 3,600 s is in its block at bin -108000 with all its votes"
print(json.dumps(res))
dc.close()
