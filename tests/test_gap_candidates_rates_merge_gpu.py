"""GPU parity of tvz_align_candidates_rates_merge (ts_gapr_merge_kernel) against
tests/gap_candidates_rates_merge_ref.py on the lists of tests/gap_candidates_rates_merge_cases.py: whole [Q, C + 1, 3]
blocks, exact integers throughout.  The reference's own answers on the named cases are asserted without a device in
tests/test_gap_candidates_rates_shards_cpu.py."""
import numpy as np
import pytest
import torch

from tests import gap_candidates_rates_merge_cases as mc, gap_candidates_rates_merge_ref as mref
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -0x5A5A5A5A
CANARY = 0xA5
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
ERR_INVALID, ERR_UNSUPPORTED = -1, -4                                  # include/tvz.h


@pytest.fixture(scope="module")
def cases():
    """-> {name: (blocks, the reference's merge)}: computed once, no test changes them"""
    return {name: (b, mref.merge(b)) for name, b in mc.hand_made().items()}


def _merge(blocks):
    return tc.align_candidates_rates_merge_device(torch.from_numpy(np.ascontiguousarray(blocks)).to(DEV)).cpu().numpy()


def test_every_hand_made_case(cases):
    """n_lists 1, 2, 3, 8, 16 x C 1, 16, 63, 64 x Q 1, 5; all lists full of distinct ids (1,024 rows); all 16 lists
    holding the same 64 ids (64 rows out); equal best at rate indexes 5 and 2 (2 comes out); the larger best in the later
    list; a tie group across rank C; all empty; shorter than C; unsorted lists; ids 0 and 2^31 - 1, best 0 and 4,095,
    rate index 7; every rule of the totals."""
    for name, (blocks, want) in cases.items():
        got = _merge(blocks)
        assert got.dtype == np.int32 and got.shape == want.shape
        bad = np.argwhere((got != want).any(axis=(1, 2)))
        assert bad.size == 0, (name, [(int(q), got[q].tolist(), want[q].tolist()) for q in bad[:1, 0]])
    # what the named cases are there to show, said of the reference's answers
    assert cases["all_full_distinct_1024_rows"][0].shape[0] * 64 == 1024
    same = cases["all_lists_hold_the_same_64_ids"][1]
    assert (same[:, :64, 0] >= 0).all() and len(set(same[0, :64, 0].tolist())) == 64 and (same[1, :64, 2] == 0).all()
    assert cases["equal_best_smaller_rate_index"][1][:, 0].tolist() == [[50, 6, 2], [50, 6, 2]]
    assert cases["larger_best_in_the_later_list"][1][0, 0].tolist() == [50, 8, 6]
    assert int(cases["totals_saturate_negative"][1][0, 4, 1]) == -INT32_MAX
    assert int(cases["totals_saturate"][1][0, 4, 1]) == INT32_MAX
    assert int(cases["refused_in_one_list"][1][0, 4, 1]) == INT32_MIN


def test_many_queries_and_none():
    """A block per query and no grid cap: Q = 4,097 and 70,001 at small C, the same 64 queries tiled; Q = 0 launches
    nothing."""
    for seed, (R, Q, c) in enumerate(((3, 7, 16), (16, 4097, 1), (2, 70001, 3))):
        blocks = mc.random_case(50 + seed, R, min(Q, 64), c)
        if Q > 64:                                                                  # the same 64 queries, over and over
            blocks = np.ascontiguousarray(np.tile(blocks, (1, -(-Q // 64), 1, 1))[:, :Q])
        want = mref.merge(blocks[:, :64])
        got = _merge(blocks)
        assert got.shape == (Q, c + 1, 3)
        for q0 in range(0, Q, 64):
            n = min(64, Q - q0)
            assert (got[q0:q0 + n] == want[:n]).all(), (R, Q, c, q0)
    out = tc.align_candidates_rates_merge_device(torch.zeros((5, 0, 17, 3), dtype=torch.int32, device=DEV))
    assert out.shape == (0, 17, 3)


def test_the_output_stands_in_an_untouched_arena_and_every_refusal_writes_nothing(cases):
    lib = _lib.load()
    blocks, want = cases["mixed_R8_C63_Q5"]
    R, Q, c1, _ = blocks.shape
    nbytes = Q * c1 * 12
    # the input 4-byte aligned and no more, too
    g_arena = torch.zeros((R * nbytes + 512,), dtype=torch.uint8, device=DEV)
    g_at = (-g_arena.data_ptr()) % 256 + 4
    g = g_arena[g_at:g_at + R * nbytes].view(torch.int32).view(R, Q, c1, 3)
    g.copy_(torch.from_numpy(blocks))
    before = g.clone()
    s = torch.cuda.current_stream(DEV)
    arena = torch.full((4096 + nbytes,), CANARY, dtype=torch.uint8, device=DEV)
    at = (-arena.data_ptr()) % 256 + 256 + 4                                       # 4-byte aligned, no more
    assert lib.tvz_align_candidates_rates_merge(g.data_ptr(), R, Q, c1 - 1, arena.data_ptr() + at, s.cuda_stream) == 0
    s.synchronize()
    a = arena.cpu().numpy()
    assert (a[:at] == CANARY).all() and (a[at + nbytes:] == CANARY).all()
    assert (a[at:at + nbytes].view(np.int32).reshape(Q, c1, 3) == want).all()
    assert (g == before).all()                                                     # the lists are read only
    # every refusal, with nothing written
    out = torch.full((Q, c1, 3), SENTINEL, dtype=torch.int32, device=DEV)

    def raw(gp=g.data_ptr(), n=R, Q_=Q, C_=c1 - 1, op=out.data_ptr()):
        rc = lib.tvz_align_candidates_rates_merge(gp, n, Q_, C_, op, s.cuda_stream)
        s.synchronize()
        return rc

    for kw, rc in ((dict(n=0), ERR_UNSUPPORTED), (dict(n=17), ERR_UNSUPPORTED), (dict(C_=0), ERR_UNSUPPORTED),
                   (dict(C_=65), ERR_UNSUPPORTED), (dict(Q_=-1), ERR_INVALID), (dict(gp=None), ERR_INVALID),
                   (dict(op=None), ERR_INVALID), (dict(gp=g.data_ptr() + 2), ERR_INVALID),
                   (dict(op=out.data_ptr() + 2), ERR_INVALID), (dict(op=out.data_ptr() + 1), ERR_INVALID),
                   (dict(op=g.data_ptr()), ERR_INVALID), (dict(op=g.data_ptr() + (R - 1) * nbytes), ERR_INVALID),
                   (dict(op=g.data_ptr() + R * nbytes - 12), ERR_INVALID)):
        assert raw(**kw) == rc, kw
        assert (out.cpu().numpy() == SENTINEL).all() and (g == before).all(), kw
    assert raw(Q_=0, gp=None, op=None) == 0
    with pytest.raises(RuntimeError, match="contiguous int32 CUDA tensor"):
        tc.align_candidates_rates_merge_device(g[:, :, :, :2])
    with pytest.raises(RuntimeError, match="lists outside 1..16"):
        tc.align_candidates_rates_merge_device(torch.zeros((17, 1, 5, 3), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="C=65 outside"):
        tc.align_candidates_rates_merge_device(torch.zeros((2, 1, 66, 3), dtype=torch.int32, device=DEV))


def test_twenty_lists_as_sixteen_and_four_equal_the_reference_over_all_twenty():
    from tvidz_amd import sharded
    b = mc.twenty_lists()
    want = mref.merge(b)
    got = _merge(np.stack([_merge(b[:16]), _merge(b[16:])]))
    assert (got == want).all()
    d = torch.from_numpy(b).to(DEV)
    assert (sharded.merge_candidate_blocks(tc.align_candidates_rates_merge_device, d).cpu().numpy() == want).all()
    # any other grouping gives the same: 7 + 7 + 6
    parts = np.stack([_merge(b[0:7]), _merge(b[7:14]), _merge(b[14:20])])
    assert (_merge(parts) == want).all()
