"""GPU parity of tvz_align_candidates_merge (ts_gapc_merge_kernel) against tests/gap_candidates_merge_ref.py on the
hand-made lists of tests/gap_candidates_merge_cases.py: whole [Q, C + 1, 2] blocks, exact integers throughout.  The
reference's own answers on the named cases are asserted without a device in tests/test_gap_candidates_shards_cpu.py."""
import numpy as np
import pytest
import torch

from tests import gap_candidates_cases as cs, gap_candidates_merge_cases as mc, gap_candidates_merge_ref as mref
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
    return tc.align_candidates_merge_device(torch.from_numpy(np.ascontiguousarray(blocks)).to(DEV)).cpu().numpy()


def test_every_hand_made_case(cases):
    """n_lists 1, 2, 3, 8, 16 x C 1, 16, 63, 64 x Q 1, 5; every list full (1,024 rows), all empty, one full and the rest
    empty, shorter than C; a tie group across rank C; equal rows in two lists; equal counts across lists; ids 0 and
    2^31 - 1 and count 2^31 - 1; every rule of the totals."""
    for name, (blocks, want) in cases.items():
        got = _merge(blocks)
        assert got.dtype == np.int32 and got.shape == want.shape
        bad = np.argwhere((got != want).any(axis=(1, 2)))
        assert bad.size == 0, (name, [(int(q), got[q].tolist(), want[q].tolist()) for q in bad[:1, 0]])
    assert cases["all_full_1024_rows"][0].shape[0] * 64 == 1024
    assert int(cases["totals_saturate_negative"][1][0, 4, 1]) == -INT32_MAX and int(cases["refused_in_one_list"][1][0, 4, 1]) == INT32_MIN


def test_many_queries_and_none():
    """More queries than one block's four waves, a count that is no multiple of four, and enough of them that the grid
    has thousands of blocks (the launch has no grid cap: a block per four queries); Q = 0 launches nothing."""
    for seed, (R, Q, c) in enumerate(((3, 7, 16), (16, 4097, 1), (2, 70001, 3), (8, 1025, 64))):
        blocks = mc.random_case(50 + seed, R, min(Q, 64), c)
        if Q > 64:                                                                  # the same 64 queries, over and over
            blocks = np.ascontiguousarray(np.tile(blocks, (1, -(-Q // 64), 1, 1))[:, :Q])
        want = mref.merge(blocks[:, :64])
        got = _merge(blocks)
        assert got.shape == (Q, c + 1, 2)
        for q0 in range(0, Q, 64):
            n = min(64, Q - q0)
            assert (got[q0:q0 + n] == want[:n]).all(), (R, Q, c, q0)
    out = tc.align_candidates_merge_device(torch.zeros((5, 0, 17, 2), dtype=torch.int32, device=DEV))
    assert out.shape == (0, 17, 2)


def test_the_output_stands_in_an_untouched_arena_and_every_refusal_writes_nothing(cases):
    lib = _lib.load()
    blocks, want = cases["mixed_R8_C63_Q5"]
    R, Q, c1, _ = blocks.shape
    g = torch.from_numpy(blocks).to(DEV)
    before = g.clone()
    s = torch.cuda.current_stream(DEV)
    arena = torch.full((4096 + Q * c1 * 8,), CANARY, dtype=torch.uint8, device=DEV)
    at = (-arena.data_ptr()) % 256 + 256 + 8                                       # 8-byte aligned, no more
    assert lib.tvz_align_candidates_merge(g.data_ptr(), R, Q, c1 - 1, arena.data_ptr() + at, s.cuda_stream) == 0
    s.synchronize()
    a = arena.cpu().numpy()
    assert (a[:at] == CANARY).all() and (a[at + Q * c1 * 8:] == CANARY).all()
    assert (a[at:at + Q * c1 * 8].view(np.int32).reshape(Q, c1, 2) == want).all()
    assert (g == before).all()                                                     # the lists are read only
    # every refusal, with nothing written
    out = torch.full((Q, c1, 2), SENTINEL, dtype=torch.int32, device=DEV)

    def raw(gp=g.data_ptr(), n=R, Q_=Q, C_=c1 - 1, op=out.data_ptr()):
        rc = lib.tvz_align_candidates_merge(gp, n, Q_, C_, op, s.cuda_stream)
        s.synchronize()
        return rc

    for kw, rc in ((dict(n=0), ERR_UNSUPPORTED), (dict(n=17), ERR_UNSUPPORTED), (dict(C_=0), ERR_UNSUPPORTED),
                   (dict(C_=65), ERR_UNSUPPORTED), (dict(Q_=-1), ERR_INVALID), (dict(gp=None), ERR_INVALID),
                   (dict(op=None), ERR_INVALID), (dict(gp=g.data_ptr() + 4), ERR_INVALID),
                   (dict(op=out.data_ptr() + 4), ERR_INVALID), (dict(op=g.data_ptr()), ERR_INVALID),
                   (dict(op=g.data_ptr() + (R - 1) * Q * c1 * 8), ERR_INVALID),
                   (dict(op=g.data_ptr() + R * Q * c1 * 8 - 8), ERR_INVALID)):
        assert raw(**kw) == rc, kw
        assert (out.cpu().numpy() == SENTINEL).all() and (g == before).all(), kw
    assert raw(Q_=0, gp=None, op=None) == 0
    with pytest.raises(RuntimeError, match="contiguous int32 CUDA tensor"):
        tc.align_candidates_merge_device(g[:, :, :, :1])
    with pytest.raises(RuntimeError, match="lists outside 1..16"):
        tc.align_candidates_merge_device(torch.zeros((17, 1, 5, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="C=65 outside"):
        tc.align_candidates_merge_device(torch.zeros((2, 1, 66, 2), dtype=torch.int32, device=DEV))


def test_twenty_lists_as_sixteen_and_four_equal_the_reference_over_all_twenty():
    from tvidz_amd import sharded
    b = mc.twenty_lists()
    want = mref.merge(b)
    first, second = _merge(b[:16]), _merge(b[16:])
    assert mref.is_sorted(first) and mref.is_sorted(second)                        # the merge keeps its own precondition
    got = _merge(np.stack([first, second]))
    assert (got == want).all()
    d = torch.from_numpy(b).to(DEV)
    assert (sharded.merge_candidate_blocks(tc.align_candidates_merge_device, d).cpu().numpy() == want).all()
    # any other grouping gives the same: 7 + 7 + 6
    parts = np.stack([_merge(b[0:7]), _merge(b[7:14]), _merge(b[14:20])])
    assert (_merge(parts) == want).all()


def test_both_producers_keep_the_precondition():
    """Each list as the local call wrote it (ts_gapc_select_kernel) is sorted by the contract's order with the padding
    last, and so is the merge's own output: what the kernel's binary searches rely on."""
    rows, uploads = cs.table() + cs.counting_table(257), cs.uploads()
    queries = [cs.counting_query()] + [uploads[n] for n in ("shifted", "twin", "stranger", "excerpt", "special")] + \
        [cs.long_query(515, 2)]
    shards = []
    try:
        for s in range(3):
            dc = tc.DeviceCorpus(0)
            dc.upload([r for r in rows if r[0] % 3 == s])
            dc.set_gap_index(cs.GAP_EPS)
            shards.append(dc)
        d_q, d_off, L = tc.pack_queries(queries, DEV)
        for c in (1, 16, 64):
            blocks = torch.stack([dc.align_candidates_block(d_q, d_off, L, c=c, min_count=1) for dc in shards])
            h = blocks.cpu().numpy()
            assert all(mref.is_sorted(b) for b in h), c
            assert (h[:, 0, c, 1] > c).all() or c == 64                            # every shard holds more than C candidates
            merged = tc.align_candidates_merge_device(blocks).cpu().numpy()
            assert mref.is_sorted(merged) and (merged == mref.merge(h)).all(), c
            assert int(merged[-1, c, 1]) == INT32_MIN and int(merged[0, c, 1]) >= 257
    finally:
        for dc in shards:
            dc.close()
