"""Child process of tests/test_align_two_bins_gpu.py: creates the libtvz RCCL communicator BEFORE its first GPU call (as
tests/near_wide_comm_child.py does), then runs tvz_align_{wide,rates,span}_topk_sharded at world size 1 with
TVZ_ALIGN_TWO_BINS against the one-handle calls on the same table, and prints the results as JSON."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (import only: no GPU call yet)

from tests import align_two_bins_cases as cs  # noqa: E402
from tvidz_amd import _lib, corpus as tc  # noqa: E402

comm = tc.Comm(tc.Comm.unique_id(), 1, 0, 0)           # ncclCommInitRank: the first GPU call of this process
dev = torch.device("cuda:0")
rows, queries, excl = cs.main_table()
mo = cs.MAIN_B * cs.E64
dc = tc.DeviceCorpus(0)
dc.upload(rows)
d_q, d_off, longest = tc.pack_queries(queries, dev)
d_ex = torch.tensor(excl, dtype=torch.int32, device=dev)
k = 16
out = {}
for form, one, sharded, kw in (
        ("wide", dc.align_wide_topk, comm.align_wide_topk_sharded, dict(contain=True)),
        ("rates", dc.align_rates_topk, comm.align_rates_topk_sharded, dict(rates=cs.MAIN_RATES)),
        ("span", dc.align_span_topk, comm.align_span_topk_sharded, dict(rates=cs.MAIN_RATES, local=True, min_votes=2))):
    one_rows, one_totals = one(queries, eps=cs.E64, max_offset=mo, k=k, exclude_ids=excl, two_bins=True, **kw)
    clear_rows, _ = one(queries, eps=cs.E64, max_offset=mo, k=k, exclude_ids=excl, **kw)
    r, t = sharded(dc, d_q, d_off, longest, eps=cs.E64, max_offset=mo, k=k, d_exclude_ids=d_ex, two_bins=True, **kw)
    torch.cuda.synchronize()
    out[form] = {"rows": r.cpu().tolist(), "totals": t.cpu().tolist(), "one_rows": one_rows.tolist(),
                 "one_totals": one_totals.tolist(), "clear_rows": clear_rows.tolist()}
# bit 4 stays no flag, with or without the new one
ws = torch.empty(tc.align_wide_topk_sharded_workspace_bytes(len(queries), longest, d_q.numel(), k, 1), dtype=torch.uint8,
                 device=dev)
r4, t4 = torch.empty((len(queries), k, 4), dtype=torch.int32, device=dev), torch.empty(len(queries), dtype=torch.int32, device=dev)
rc = comm.lib.tvz_align_wide_topk_sharded(dc._h, comm._h, d_q.data_ptr(), d_off.data_ptr(), len(queries), longest, cs.E64, mo,
                                          1, 0, tc.ALIGN_TWO_BINS | 4, None, k, r4.data_ptr(), t4.data_ptr(), ws.data_ptr(),
                                          ws.numel(), torch.cuda.current_stream().cuda_stream)
out["unknown_flag"] = [int(rc), (_lib.load().tvz_last_error() or b"").decode()]
torch.cuda.synchronize()
dc.close()
comm.close()
print("RESULT " + json.dumps(out))
