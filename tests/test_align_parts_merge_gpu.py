"""GPU parity of tvz_align_parts_merge (ts_alignp_merge_kernel) on hand-made blocks against corpus.align_parts_merge, the
numpy merge service.ShardedCorpus used before the device had one: whole [Q, k, 1 + max_parts, 6] outputs, exact
integers.  Every input and output sits 4 bytes past a 16-byte line (a pair's block is (1 + max_parts) x 24 bytes: nothing
may assume more than int32 alignment) inside an arena of 0xA5 bytes that is otherwise unchanged."""
import numpy as np
import pytest
import torch

from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
ERR_INVALID, ERR_UNSUPPORTED = -1, -4                                 # include/tvz.h


def _blocks(rng, R, Q, k, P):
    """R lists of plausible answers: few distinct vote counts (ties are common), lists without a row, now and then a
    refusal, ids of either sign; zeros behind n_parts as the call writes them."""
    a = np.zeros((R, Q, k, 1 + P, 6), dtype=np.int32)
    a[:, :, :, 0, 0] = rng.integers(-3, 1000, size=(Q, k))[None]      # one call: the same ids in every list
    a[:, :, :, 0, 5] = rng.integers(0, 200, size=(Q,))[None, :, None]
    n_rows = rng.choice([0, 0, 1, 2, 8], size=(R, Q, k))
    holds = n_rows > 0
    a[:, :, :, 0, 4] = n_rows
    a[:, :, :, 0, 1] = np.where(holds, rng.integers(1, 500, size=(R, Q, k)), 0)
    a[:, :, :, 0, 2] = np.where(holds, rng.integers(0, 8, size=(R, Q, k)), 0)
    n_parts = np.where(holds, rng.integers(0, P + 1, size=(R, Q, k)), 0)
    a[:, :, :, 0, 3] = n_parts
    parts = rng.integers(-4000, 4000, size=(R, Q, k, P, 6))
    parts[..., 1] = rng.integers(1, 4, size=(R, Q, k, P))             # votes 1..3: the lists tie often
    a[:, :, :, 1:] = np.where((np.arange(P)[None, None, None, :] < n_parts[..., None])[..., None], parts, 0)
    refused = holds & (rng.random((R, Q, k)) < 0.08)
    a[refused, 1:] = 0
    a[refused, 0, 1:4] = (0, 0, INT32_MIN)
    a[refused, 0, 4] = 9
    return a


def _merge_in_arena(a):
    """tvz_align_parts_merge with gathered and d_parts at 4 bytes past a 256-byte line inside poisoned arenas -> the
    output, after checking that nothing else changed"""
    R, Q, k, rows, _ = a.shape
    n_in, n_out = a.size * 4, Q * k * rows * 24
    src = torch.full((256 + 4 + n_in + 256,), CANARY, dtype=torch.uint8, device=DEV)
    dst = torch.full((256 + 4 + n_out + 256,), CANARY, dtype=torch.uint8, device=DEV)
    at_in, at_out = (-src.data_ptr()) % 256 + 4, (-dst.data_ptr()) % 256 + 4
    src[at_in:at_in + n_in] = torch.from_numpy(a.reshape(-1).view(np.uint8)).to(DEV)
    s = torch.cuda.current_stream(DEV)
    rc = _lib.load().tvz_align_parts_merge(src.data_ptr() + at_in, R, Q, k, rows - 1, dst.data_ptr() + at_out, s.cuda_stream)
    s.synchronize()
    assert rc == 0, _lib.load().tvz_last_error()
    d = dst.cpu().numpy()
    assert (d[:at_out] == CANARY).all() and (d[at_out + n_out:] == CANARY).all()
    after = src.cpu().numpy()
    assert (after[:at_in] == CANARY).all() and (after[at_in + n_in:] == CANARY).all()
    assert (after[at_in:at_in + n_in] == a.reshape(-1).view(np.uint8)).all()
    return d[at_out:at_out + n_out].copy().view(np.int32).reshape(Q, k, rows, 6)


def _same(got, exp, what):
    bad = np.argwhere((got != exp).any(axis=(2, 3)))
    assert got.shape == exp.shape and bad.size == 0, (what, len(bad), [(q, j, got[q, j].tolist(), exp[q, j].tolist())
                                                                    for q, j in bad[:2].tolist()])


@pytest.mark.parametrize("P", (1, 4))
@pytest.mark.parametrize("R", (1, 2, 3, 16))
def test_random_blocks_of_every_shape(R, P):
    rng = np.random.default_rng(1000 * R + P)
    for Q in (1, 5):
        for k in (1, 3, 64):
            a = _blocks(rng, R, Q, k, P)
            _same(_merge_in_arena(a), tc.align_parts_merge(a), (R, Q, k, P))
            # the wrapper: the same launch on ordinary tensors
            got = tc.align_parts_merge_device(torch.from_numpy(a).to(DEV)).cpu().numpy()
            _same(got, tc.align_parts_merge(a), ("wrapper", R, Q, k, P))


def _answer(vid, row_len, votes, n_rows, n_parts=1, m=24, P=2):
    b = np.zeros((1 + P, 6), dtype=np.int32)
    b[0] = (vid, row_len, 0, n_parts, n_rows, m)
    if n_parts > 0:
        b[1] = (5, votes, 0, 8, 9, 9)
    if n_parts > 1:
        b[2] = (-40, 2, 10, 12, 3, 3)
    return b


@pytest.mark.parametrize("R", (2, 3, 16))
def test_the_named_cases(R):
    """One pair per case, in one call: the rule as include/tvz.h words it."""
    P, last = 2, R - 1
    absent = lambda vid: _answer(vid, 0, 0, 0, n_parts=0)                          # noqa: E731  (no row of the id)
    refused = np.zeros((3, 6), dtype=np.int32)
    refused[0] = (7, 0, 0, INT32_MIN, 9, 24)
    cases = {
        "a vote tie: the lower list": {0: _answer(7, 10, 5, 1), last: _answer(7, 11, 5, 2)},
        "rows but no votes against lists without rows": {last: _answer(7, 10, 0, 1, n_parts=0)},
        "no list with rows: list 0's block": {},
        "a negative id": {0: _answer(-1, 0, 0, 0, n_parts=0), last: _answer(-1, 0, 0, 0, n_parts=0)},
        "one refused list among good ones": {0: _answer(7, 10, 5, 1, n_parts=2), last: refused},
        "n_rows past INT32_MAX": {0: _answer(7, 10, 3, INT32_MAX - 1), last: _answer(7, 12, 4, 5)},
        "the winner in the last list": {0: _answer(7, 10, 3, 1), last: _answer(7, 12, 4, 1, n_parts=2)},
        "refused, and n_rows past INT32_MAX": {0: _answer(7, 10, 3, INT32_MAX), last: refused},
    }
    a = np.zeros((R, 1, len(cases), 1 + P, 6), dtype=np.int32)
    for j, lists in enumerate(cases.values()):
        for r in range(R):
            a[r, 0, j] = lists.get(r, absent(-1 if j == 3 else 7))
        if j == 2:
            a[0, 0, j, 0, 5] = 99                                                   # tell list 0's block from the others'
    got, exp = _merge_in_arena(a), tc.align_parts_merge(a)
    _same(got, exp, R)
    g = {name: got[0, j].tolist() for j, name in enumerate(cases)}
    assert g["a vote tie: the lower list"][0] == [7, 10, 0, 1, 3, 24]
    assert g["rows but no votes against lists without rows"][0] == [7, 10, 0, 0, 1, 24]
    assert g["no list with rows: list 0's block"][0] == [7, 0, 0, 0, 0, 99]
    assert g["a negative id"][0] == [-1, 0, 0, 0, 0, 24]
    assert g["one refused list among good ones"] == [[7, 0, 0, INT32_MIN, 10, 24], [0] * 6, [0] * 6]
    assert g["n_rows past INT32_MAX"][0] == [7, 12, 0, 1, INT32_MAX, 24]
    assert g["the winner in the last list"] == [[7, 12, 0, 2, 2, 24], [5, 4, 0, 8, 9, 9], [-40, 2, 10, 12, 3, 3]]
    assert g["refused, and n_rows past INT32_MAX"][0] == [7, 0, 0, INT32_MIN, INT32_MAX, 24]


def test_regrouping_gives_the_same_answer():
    """20 lists merged in groups of 16 and 4 and the two answers merged again, as ShardedCorpus does beyond 16 shards"""
    rng = np.random.default_rng(20)
    a = _blocks(rng, 20, 5, 3, 4)
    d = torch.from_numpy(a).to(DEV)
    groups = torch.stack([tc.align_parts_merge_device(d[:16].contiguous()), tc.align_parts_merge_device(d[16:].contiguous())])
    _same(tc.align_parts_merge_device(groups).cpu().numpy(), tc.align_parts_merge(a), "20 lists")


def test_refusals_write_nothing():
    lib = _lib.load()
    src = torch.zeros((2, 1, 4, 3, 6), dtype=torch.int32, device=DEV)
    out = torch.full((1, 4, 3, 6), -0x5A5A5A5A, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream(DEV)

    def call(n_lists=2, Q=1, k=4, P=2, gathered=src.data_ptr(), parts=out.data_ptr()):
        rc = lib.tvz_align_parts_merge(gathered, n_lists, Q, k, P, parts, s.cuda_stream)
        return rc, lib.tvz_last_error()

    for kw, want, word in ((dict(n_lists=0), ERR_UNSUPPORTED, b"0 lists outside 1..16"), (dict(n_lists=17), ERR_UNSUPPORTED, b"17 lists"),
                           (dict(k=0), ERR_UNSUPPORTED, b"k=0 outside 1..64"), (dict(k=65), ERR_UNSUPPORTED, b"k=65"),
                           (dict(P=0), ERR_UNSUPPORTED, b"max_parts=0 outside 1..4"), (dict(P=5), ERR_UNSUPPORTED, b"max_parts=5"),
                           (dict(gathered=None), ERR_INVALID, b"NULL argument"), (dict(parts=None), ERR_INVALID, b"NULL argument"),
                           (dict(Q=-1), ERR_INVALID, b"Q=-1 is negative")):
        rc, msg = call(**kw)
        assert rc == want and word in msg, (kw, rc, msg)
    s.synchronize()
    assert (out.cpu().numpy() == -0x5A5A5A5A).all()
    assert call(Q=0, gathered=None, parts=None)[0] == 0                            # no query: nothing to do
