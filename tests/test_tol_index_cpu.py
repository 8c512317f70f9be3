"""The tolerant lookup through cell postings (tvz_corpus_tol_index), without a GPU: the two new entry points are
declared, exported, bound and refuse a NULL handle at the unchanged version; the probe range of every query value
covers the cell of every key it matches (tests/tol_index_ref.py against tests/tol_ref.py's predicate, random and
adversarial values) in at most four cells; the new kernels' code objects have no scratch and no spills; the service's
--match-tol-index reaches every shard handle, is refused below --match-tolerance before any rank starts, and is
never named without the flag."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import tol_index_ref as tir
from tests import tol_ref
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)
from tests.tol_fakes import TolBackend, TolCorpus
from tvidz_amd import service, sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tvz_corpus_tol_index", "tvz_corpus_tol_index_stats")


# ---- binding ---------------------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_declared_exported_bound_and_refuse_null():
    from tvidz_amd import _lib, build
    build.build()
    header = open(os.path.join(ROOT, "include", "tvz.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.tvz_corpus_tol_index(None, 0.001) == -1                       # TVZ_ERR_INVALID
    assert b"NULL" in lib.tvz_last_error()
    cell, out = C.c_double(7.0), (C.c_int64 * 4)(1, 2, 3, 4)
    assert lib.tvz_corpus_tol_index_stats(None, C.byref(cell), out) == -1
    assert cell.value == 7.0 and list(out) == [1, 2, 3, 4]                   # nothing written
    # new exports only: the version every layer pins stays
    assert re.search(r"#define TVZ_VERSION 404\b", header) and "new exports only" in header
    assert lib.tvz_version() == _lib.VERSION == 404
    assert float(re.search(r"#define TVZ_TOL_CELL_MIN (\S+)", header).group(1)) == tir.CELL_MIN


# ---- the probe range is a superset -----------------------------------------------------------------------------------
def _ulps(x, n):
    """x moved n ulps (n may be negative)."""
    x = np.asarray(x, dtype=np.float64).copy()
    with np.errstate(over="ignore"):
        for _ in range(abs(n)):
            x = np.nextafter(x, np.inf if n > 0 else -np.inf)
    return x


def _check(q, key, tol, w, what):
    """Every matching (q, key) pair has cell_of(key) inside q's probe range; the range is at most four cells."""
    q, key = np.broadcast_arrays(np.asarray(q, dtype=np.float64), np.asarray(key, dtype=np.float64))
    assert tol <= w, what
    lo, hi = tir.probe_range(q, tol, w)
    assert np.all(lo <= hi), what
    assert np.all(hi - lo + 1 <= tir.MAX_CELLS), (what, int((hi - lo).max()))
    m = tir.matches(q, key, tol)
    ck = tir.cell_of(key, w)
    bad = m & ~((lo <= ck) & (ck <= hi))
    assert not bad.any(), (what, q[bad][:3], key[bad][:3], tol, w)
    return int(m.sum())


def test_the_restated_predicate_is_tol_refs():
    rng = np.random.default_rng(5)
    q = rng.uniform(-5, 5, 300)
    row = tol_ref.row_set(rng.uniform(-5, 5, 40))
    for tol in (0.0, 1e-3, 0.1):
        assert np.array_equal(tir.matches(q[:, None], row[None, :], tol).any(axis=1), tol_ref.match_mask_brute(q, row, tol))


def test_cell_of_is_monotone_and_clamped():
    rng = np.random.default_rng(6)
    for w in (tir.CELL_MIN, 1e-3, 0.1, 3.0, 1e6):
        x = np.sort(np.concatenate([rng.uniform(-1e4, 1e4, 5000), rng.uniform(-1, 1, 500) * tir.CELL_LIMIT * w * 4,
                                    [-np.inf, np.inf, 0.0, -1e308, 1e308, tir.CELL_LIMIT * w, -tir.CELL_LIMIT * w]]))
        c = tir.cell_of(x, w)
        assert np.all(np.diff(c) >= 0), w
        assert c[0] == -int(tir.CELL_LIMIT) and c[-1] == int(tir.CELL_LIMIT)
        assert np.all(c[x < 0] <= -1) and np.all(c[x >= 0] >= 0)            # negative keys never share a cell with the others


@pytest.mark.parametrize("w", [tir.CELL_MIN, 1e-3, 0.0333, 0.1, 1.0, 4096.0])
def test_probe_range_covers_every_match_random(w):
    rng = np.random.default_rng(int(w * 1e9) % 1000 + 1)
    total = 0
    for tol in (0.0, w / 4, w / 2, np.nextafter(w, 0.0), w):
        for scale in (1.0, 1e3, 7200.0, 1e6):
            q = rng.uniform(-scale, scale, 20000)
            # keys near q: inside, at and just outside the window
            key = q + rng.uniform(-1.5, 1.5, q.size) * (tol if tol else w) * rng.choice([1.0, 1.0, 1e-3], q.size)
            total += _check(q, key, tol, w, ("random", tol, scale))
            total += _check(q, q.copy(), tol, w, ("equal", tol, scale))
    assert total > 0


@pytest.mark.parametrize("w", [tir.CELL_MIN, 1e-3, 0.1, 1.0])
def test_probe_range_covers_every_match_adversarial(w):
    inf = np.inf
    Lw = tir.CELL_LIMIT * w
    n_match = 0
    for tol in (0.0, 5e-324, w / 4, np.nextafter(w, 0.0), w):
        if tol > w:
            continue
        base = [0.0, tol, -tol, 2 * tol, w, -w, w / 2, 3 * w, -3 * w, 10.0, -10.0, 1234.5678, -7199.999, 1e-300, -1e-300,
                5e-324, -5e-324, 1e6 * w, -1e6 * w,
                # at and beyond +-L w (the clamp), and far beyond
                Lw, -Lw, Lw - w, -Lw + w, Lw + w, -Lw - w, Lw * 1.5, -Lw * 1.5, 2 * Lw, -2 * Lw, 2 * Lw + w, 4 * Lw, -4 * Lw,
                Lw * 1e3, -Lw * 1e3, 1e300, -1e300, 1.7976931348623157e308, -1.7976931348623157e308, inf, -inf]
        # cell edges: multiples of w and their neighbours
        base += [k * w for k in (-3, -2, -1, 1, 2, 3, 1000, -1000, 2 ** 30, -(2 ** 30))]
        q0 = np.array(base, dtype=np.float64)
        qs = np.concatenate([_ulps(q0, d) for d in (-2, -1, 0, 1, 2)])
        with np.errstate(over="ignore", invalid="ignore"):
            for sign in (-1.0, 1.0):
                edge = qs + sign * tol                                       # q -+ tol, and one / two ulps either side
                keys = [_ulps(edge, d) for d in (-2, -1, 0, 1, 2)] + [qs]
                # ... and the keys one ulp around where a SUBTRACTION of exactly tol lands: k with fl(q - k) == tol
                keys += [_ulps(qs - sign * tol, d) for d in (-1, 0, 1)]
                for k in keys:
                    k = np.where(np.isnan(k), qs, k)                         # (inf - inf: keep the pair q == key)
                    n_match += _check(qs, k, tol, w, ("adversarial", tol, sign))
        # every adversarial value against every other one
        n_match += _check(qs[:, None], qs[None, :], tol, w, ("cross", tol))
    assert n_match > 0


def test_infinities_match_only_themselves_and_sit_in_the_end_cells():
    w, tol = 1e-3, 1e-3
    for q in (np.inf, -np.inf):
        lo, hi = tir.probe_range(q, tol, w)
        assert lo == hi == tir.cell_of(q, w) == int(np.sign(q) * tir.CELL_LIMIT)
        assert tir.matches(q, q, tol) and not tir.matches(q, 1e308 * np.sign(q), tol)


# ---- code object -----------------------------------------------------------------------------------------------------
LOOKUP = "ts_tol_index_kernel"


def _named(kernels, name):  # noqa: F811
    return {n: k for n, k in kernels.items() if name in n}


def test_the_lookup_kernels_have_no_scratch_and_no_spills(kernels):  # noqa: F811
    ks = _named(kernels, LOOKUP)
    # kModeM2 / kModeTop5 x list form / top-k form
    assert len(ks) == 4, sorted(ks)
    for n, k in ks.items():
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (n, k)
        assert k[".max_flat_workgroup_size"] == 256
        # Recorded: the compiler reports 74 / 77 VGPRs for the list form, 71 / 74 for the top-k form (the sweep's row
        # walk + the arguments read back from LDS): <= 80 keeps six waves per SIMD, and 256-thread blocks put one
        # wave on each.
        assert k[".vgpr_count"] <= 80, (n, k[".vgpr_count"])
        # static LDS: two bitmaps of a sub-index (4 KiB), the ranks (1 KiB), the parked arguments, the hit stage
        # (3 KiB) or the four waves' lists and stages (4 KiB): within kTolIxStaticLds, the bound the launch adds the
        # sorted query to before it checks the sum against a workgroup's 160 KiB
        assert 5 * 1024 <= k[".group_segment_fixed_size"] <= 512 * 10 + 256 + 4 * 1024, (n, k[".group_segment_fixed_size"])


def _mode_of(mangled, kernel):
    """The kernel's first template argument (MODE: 0 = kModeM2, 1 = kModeTop5), read from the name itself: the Itanium
    encoding puts an int template argument N right behind the name as `ILi<N>E`, which demangles to `kernel<N>`."""
    m = re.search(re.escape(kernel) + r"ILi(\d+)E", mangled)
    assert m, mangled
    return int(m.group(1))


def test_the_sweeps_keep_their_registers_next_to_the_new_list_arguments(kernels):  # noqa: F811
    # ts_tol_topk_kernel gained two scalar arguments (where its lists start among the query's): no VGPR more
    by_mode = {_mode_of(n, "ts_tol_topk_kernel"): k for n, k in _named(kernels, "ts_tol_topk_kernel").items()}
    assert sorted(by_mode) == [0, 1]
    m2, top5 = by_mode[0], by_mode[1]
    assert m2[".vgpr_count"] <= 64 and top5[".vgpr_count"] <= 72
    for k in (m2, top5):
        assert k[".private_segment_fixed_size"] == 0


# ---- service ---------------------------------------------------------------------------------------------------------
class CellCorpus(TolCorpus):
    """tol_fakes.TolCorpus that records DeviceCorpus.set_tol_index."""

    def __init__(self):
        super().__init__()
        self.cells = []

    def set_tol_index(self, cell):
        self.cells.append(float(cell))


def test_rank_corpus_sets_the_cell_on_its_shard_only_when_asked():
    for cell, exp in ((0.0, []), (0.002, [0.002])):
        shard = CellCorpus()
        rc = service.RankCorpus(shard, sharded.ShardedMatcher(TolBackend(live=shard), k=4, cap=64), xdev="cpu",
                                tol_index_cell=cell)
        try:
            assert shard.cells == exp
        finally:
            rc.close()
    shard = CellCorpus()
    rc = service.RankCorpus(shard, sharded.ShardedMatcher(TolBackend(live=shard), k=4, cap=64), xdev="cpu")
    rc.close()
    assert shard.cells == []                                                 # the default never names it
    plain = TolCorpus()                                                      # a shard without cell postings refuses the flag
    with pytest.raises(RuntimeError, match="cell postings"):
        service.RankCorpus(plain, sharded.ShardedMatcher(TolBackend(live=plain), k=4, cap=64), xdev="cpu",
                           tol_index_cell=0.002)
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="match_tol_index"):
            service.RankCorpus(CellCorpus(), None, tol_index_cell=bad)


def test_sharded_corpus_sets_the_cell_on_every_shard_handle(monkeypatch):
    made = []

    class Handle(CellCorpus):
        def __init__(self, device=0):
            super().__init__()
            made.append(self)

    from tvidz_amd import corpus as tc
    monkeypatch.setattr(tc, "DeviceCorpus", Handle)
    monkeypatch.setattr(service.torch.cuda, "Stream", lambda *a, **kw: None)
    monkeypatch.setattr(service, "_Stage", lambda dev: None)
    sc = service.ShardedCorpus(device=0, n_shards=3, tol_index_cell=0.004)
    assert len(made) == 3 and [h.cells for h in made] == [[0.004]] * 3
    sc.batcher.close() if hasattr(sc.batcher, "close") else None
    del made[:]
    sc = service.ShardedCorpus(device=0, n_shards=3)
    assert len(made) == 3 and [h.cells for h in made] == [[]] * 3
    sc.batcher.close() if hasattr(sc.batcher, "close") else None


def test_the_launcher_passes_the_cell_to_every_rank_and_refuses_one_below_the_tolerance(monkeypatch, tmp_path):
    started = []

    class FakePopen:
        def __init__(self, cmd, env=None):
            self.args = cmd
            started.append(cmd)

        def poll(self):
            return 0

    monkeypatch.setattr(subprocess, "Popen", FakePopen)
    monkeypatch.setattr(service.RankService, "_wait_ready", lambda self, timeout: None)
    url = f"sqlite:///{tmp_path}/t.db"
    kw = dict(base_port=5900, backend="gloo", parts="m:f", k=4, cap=64, workers=8, tick_s=0.002)
    # without the flag no child hears of it, with or without a tolerance
    for s in (service.RankService(2, url, **kw), service.RankService(2, url, match_tolerance=0.001, **kw)):
        assert all("--match-tol-index" not in p.args for p in s.procs)
    before = [list(p.args) for p in service.RankService(2, url, match_tolerance=0.001, **kw).procs]
    s = service.RankService(2, url, match_tolerance=0.001, match_tol_index=0.002, **kw)
    for r, p in enumerate(s.procs):
        mp_old = before[r][before[r].index("--master-port") + 1]
        mp_new = p.args[p.args.index("--master-port") + 1]
        assert p.args == [mp_new if x == mp_old else x for x in before[r]] + ["--match-tol-index", "0.002"]
    assert service.RankService(2, url, match_tolerance=0.002, match_tol_index=0.002, **kw).procs   # equal is fine
    assert service.RankService(2, url, match_tol_index=0.002, **kw).procs                           # its own switch
    n = len(started)
    with pytest.raises(ValueError, match="below match_tolerance"):           # before any rank starts
        service.RankService(2, url, match_tolerance=0.01, match_tol_index=0.002, **kw)
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="match_tol_index"):
            service.RankService(2, url, match_tol_index=bad, **kw)
    assert len(started) == n


def test_the_command_line_has_the_flag_off_by_default_and_refuses_a_small_cell(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "tvidz_amd.service", "--help"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0 and "--match-tol-index CELL" in r.stdout
    r = subprocess.run([sys.executable, "-m", "tvidz_amd.service", "--ranks", "1", "--db", f"sqlite:///{tmp_path}/t.db",
                        "--match-tolerance", "0.01", "--match-tol-index", "0.001"], capture_output=True, text=True,
                       env=env, cwd=ROOT, timeout=120)
    assert r.returncode != 0 and "below match_tolerance" in r.stderr
