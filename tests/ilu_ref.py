"""CPU restatement of ILU(0) (include/spal.h) and the matrices its tests use.

The contract is `ilu0_loop`: F starts as a copy of A's values on A's structure, which never changes (no fill); for rows
i ascending and every stored (i, k) with k < i in ascending k: w = F[i,k] / F[k,k], F[i,k] = w, and for every stored
(k, j) with j > k in ascending j for which (i, j) is stored: F[i,j] = F[i,j] - (w * F[k,j]), the product and the
difference rounded separately in the matrix dtype.  `ilu0_rows` is the same arithmetic with the updates of one (i, k)
taken together as numpy vectors (they touch distinct entries, so their order among themselves does not matter);
tests/test_ilu_host.py proves the two bit-equal, and the larger device tests use the faster one.
"""
import numpy as np

from . import trsv_ref as tr

full, fill, assert_same_bits = tr.full, tr.fill, tr.assert_same_bits


def diag_positions(n, rowptr, colind):
    """Position of the stored (i, i) entry of every row (every row must store one)."""
    rp = rowptr.astype(np.int64)
    ci = colind.astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    pos = np.flatnonzero(rows == ci)
    assert pos.size == n and np.array_equal(rows[pos], np.arange(n)), "a row stores no diagonal"
    return pos


def ilu0_loop(n, rowptr, colind, values):
    """THE definition, in numpy scalars of the matrix dtype."""
    dt = values.dtype.type
    f = values.copy()
    rp = [int(p) for p in rowptr]
    ci = [int(c) for c in colind]
    dg = [int(d) for d in diag_positions(n, rowptr, colind)]
    with np.errstate(all="ignore"):
        for i in range(n):
            where = {ci[q]: q for q in range(rp[i], rp[i + 1])}
            for p in range(rp[i], dg[i]):
                k = ci[p]
                w = dt(f[p] / f[dg[k]])
                f[p] = w
                for pu in range(dg[k] + 1, rp[k + 1]):
                    q = where.get(ci[pu])
                    if q is not None:
                        f[q] = dt(f[q] - dt(w * f[pu]))
    return f


def ilu0_rows(n, rowptr, colind, values):
    """ilu0_loop's arithmetic; the updates of one (i, k) in one numpy operation each (elementwise multiply, then
    elementwise subtract: two roundings, as in the loop)."""
    f = values.copy()
    rp = rowptr.astype(np.int64)
    ci = colind.astype(np.int64)
    dg = diag_positions(n, rowptr, colind)
    with np.errstate(all="ignore"):
        for i in range(n):
            e = int(rp[i + 1])
            for p in range(int(rp[i]), int(dg[i])):
                k = int(ci[p])
                w = f[p] / f[dg[k]]
                f[p] = w
                u0, u1 = int(dg[k]) + 1, int(rp[k + 1])
                if u0 == u1 or p + 1 == e:
                    continue
                tail = ci[p + 1:e]                       # row i past (i, k): ascending
                at = np.searchsorted(tail, ci[u0:u1])
                hit = at < tail.size
                hit[hit] = tail[at[hit]] == ci[u0:u1][hit]
                q = p + 1 + at[hit]
                f[q] = f[q] - w * f[u0:u1][hit]
    return f


# ---- patterns ----------------------------------------------------------------------------------------------------

def sym(pattern):
    """The union of a pattern and its transpose: a lower pattern with its diagonal becomes a structurally symmetric
    matrix whose lower triangle is the pattern, so the factorisation's levels are the pattern's."""
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    cols = colind.astype(np.int64)
    return tr.from_coo(n, np.concatenate([rows, cols]), np.concatenate([cols, rows]))


def fan(n):
    """The diagonal, a full last row and a full last column: one row of n entries, every other row of two."""
    i = np.arange(n - 1, dtype=np.int64)
    last = np.full(n - 1, n - 1, dtype=np.int64)
    d = np.arange(n, dtype=np.int64)
    return tr.from_coo(n, np.concatenate([d, last, i]), np.concatenate([d, i, last]))


def rows_with_lower_entries(pattern):
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    return int(np.unique(rows[colind.astype(np.int64) < rows]).size)


def to_csc(pattern, values):
    """(colptr, rowind, values by columns, the permutation that takes CSR positions to CSC positions)."""
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    order = np.lexsort((rows, colind.astype(np.int64)))
    colptr = np.concatenate([[0], np.cumsum(np.bincount(colind.astype(np.int64), minlength=n))]).astype(np.uint64)
    return colptr, rows[order].astype(np.uint64), values[order], order


# ---- the hand examples (tests/test_ilu_host.py checks the loop on them, tests/test_gpu_ilu.py the device) ----------

HAND_A = np.array([[2, 1, 0, 0], [4, 1, 3, 0], [0, 3, -4, -2], [0, 0, 20, -5]], dtype=np.float64)
HAND_F = np.array([[2, 1, 0, 0], [2, -1, 3, 0], [0, -3, 5, -2], [0, 0, 4, 3]], dtype=np.float64)
# rows {0,1,2}, {0,1}, {0,2}: the update of (1, 2) and of (2, 1) falls on an entry that is not stored and is dropped
DROP_A = np.array([[2, 1, 1], [4, 5, 0], [6, 0, 7]], dtype=np.float64)
DROP_F = np.array([[2, 1, 1], [2, 3, 0], [3, 0, 4]], dtype=np.float64)


def dense_to_csr(a, dtype):
    """The non-zeros of a dense array as (n, rowptr, colind), values."""
    r, c = np.nonzero(a)
    n, rowptr, colind = tr.from_coo(a.shape[0], r, c)
    return (n, rowptr, colind), a[r, c].astype(dtype)
