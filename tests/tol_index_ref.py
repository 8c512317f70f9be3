"""Plain float64 restatement of the cell function and the probe range of the tolerant lookup through cell postings
(tvz_corpus_tol_index; tvidz_amd/csrc/tvz_index_kernels.h `tol_cell_of`, tvz_tol_index_kernels.h `tol_probe_range`),
next to tests/tol_ref.py, which restates the match itself.  numpy float64 arithmetic is IEEE, operation by operation,
as the kernels' is."""
import numpy as np

CELL_LIMIT = 2.0 ** 40          # L: cell ids are clamped to [-L, +L]
CELL_MIN = 2.0 ** -20           # TVZ_TOL_CELL_MIN, seconds
MAX_CELLS = 4                   # cells an element probes at most (tol <= w)


def cell_of(x, w):
    """clamp(floor(x / w), -L, +L) in double, then int64.  Monotone in x; +-inf land in the end cells."""
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.floor(np.asarray(x, dtype=np.float64) / np.float64(w))
    return np.clip(c, -CELL_LIMIT, CELL_LIMIT).astype(np.int64)


def probe_range(q, tol, w):
    """(first cell, last cell) probed for query value q: cell_of of fl(fl(q -+ tol) -+ w / 1024)."""
    q = np.asarray(q, dtype=np.float64)
    m = np.float64(w) * np.float64(2.0 ** -10)
    with np.errstate(over="ignore", invalid="ignore"):
        a = (q - np.float64(tol)) - m
        b = (q + np.float64(tol)) + m
    return cell_of(a, w), cell_of(b, w)


def matches(q, key, tol):
    """tests/tol_ref.py's predicate for arrays of pairs."""
    q = np.asarray(q, dtype=np.float64)
    key = np.asarray(key, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (q == key) | (np.abs(q - key) <= tol)
