"""Child process of tests/test_tol_index_gpu.py: creates the libtvz RCCL communicator BEFORE its first GPU call, then
runs tvz_match_tol_sharded at world size 1 on two handles with the same corpus - one with cell postings, one without -
and prints whether every merged block and total is identical, as JSON."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (import only: no GPU call yet)

from tvidz_amd import corpus as tc, synth  # noqa: E402

uid = tc.Comm.unique_id()
comm = tc.Comm(uid, 1, 0, 0)                   # the first GPU call of this process
dev = torch.device("cuda:0")
CELL = 0.001
ids, offs, keys = synth.synth_timestamp_corpus(20000, seed=21, mean_len=60)
plain, cells = tc.DeviceCorpus(0), tc.DeviceCorpus(0)
plain.upload_csr(ids, offs, keys)
cells.upload_csr(ids, offs, keys)
cells.set_tol_index(CELL)
rng = np.random.default_rng(4)
qs, excl = [], []
for t in range(40):
    r = int(rng.integers(0, len(ids)))
    qs.append((keys[offs[r]:offs[r + 1]] + (0.0, 0.0004, -0.0003)[t % 3]).tolist())
    excl.append(int(ids[r]) if t % 2 else -1)
for h in (plain, cells):                       # rows only the delta table knows
    h.upsert(int(ids[5]), [t + 0.0002 for t in qs[0][:10]])
    h.upsert(900001, qs[1][:7])
d_q, d_off, ml = tc.pack_queries(qs, dev)
d_ex = torch.tensor(excl, dtype=torch.int32, device=dev)
out = {"stats": cells.tol_index_stats(), "plain_stats": plain.tol_index_stats(), "equal": {}, "hits": {}}
for tol in (0.0, 0.00025, 0.001, 0.002):       # the last one is above the cell: the sweep on both
    for mm in (1, 2, 5):
        for k in (1, 16):
            a = comm.match_tol_sharded(plain, d_q, d_off, ml, tol, mm, k, d_exclude_ids=d_ex)
            a = (a[0].clone(), a[1].clone())
            b = comm.match_tol_sharded(cells, d_q, d_off, ml, tol, mm, k, d_exclude_ids=d_ex)
            torch.cuda.synchronize()
            out["equal"][f"{tol}/{mm}/{k}"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
            out["hits"][f"{tol}/{mm}/{k}"] = int(b[1].sum())
comm.close()
plain.close()
cells.close()
print("RESULT " + json.dumps(out))
