"""CPU restatement of the sparse triangular solve (include/spal.h) and the matrices its tests use.

The contract is `solve_loop`: rows ascending (lower) or descending (upper); s = b[i]; for every stored entry (i, j, v) of
the chosen triangle off the diagonal, in ascending column, s = s - (v * x[j]) with the product and the difference rounded
separately in the matrix dtype; x[i] = s / d, or s with a unit diagonal.  `solve_by_levels` is the same arithmetic taken
one level at a time with numpy vectors (for the one large case); tests/test_trsv_host.py proves the two bit-equal.
"""
import numpy as np


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_same_bits(x, ref):
    """Raw bits equal, NaN compared by position (any NaN payload matches any other)."""
    x, ref = np.asarray(x), np.asarray(ref)
    assert x.dtype == ref.dtype and x.shape == ref.shape
    nx, nr = np.isnan(x), np.isnan(ref)
    assert np.array_equal(nx, nr), f"NaN positions differ at {np.flatnonzero(nx != nr)[:8]}"
    bad = np.flatnonzero((_bits(x) != _bits(ref)) & ~nr)
    assert bad.size == 0, f"{bad.size} elements differ, first at {bad[:8]}: {x[bad[:8]]} vs {ref[bad[:8]]}"


def _used(i, cols, lower):
    """Slice of a row's (ascending) columns that the solve reads off the diagonal, and the diagonal's position or -1."""
    lo = int(np.searchsorted(cols, i, side="left"))
    has = lo < cols.size and int(cols[lo]) == i
    return (slice(0, lo) if lower else slice(lo + (1 if has else 0), cols.size)), (lo if has else -1)


def solve_loop(n, rowptr, colind, values, b, lower=True, unit=False):
    """THE definition, in numpy scalars of the matrix dtype."""
    dt = values.dtype.type
    x = np.zeros(n, dtype=values.dtype)
    rp = [int(p) for p in rowptr]
    with np.errstate(all="ignore"):
        for i in (range(n) if lower else range(n - 1, -1, -1)):
            cols = colind[rp[i]:rp[i + 1]]
            vals = values[rp[i]:rp[i + 1]]
            sl, d = _used(i, cols, lower)
            s = dt(b[i])
            for j, v in zip(cols[sl].tolist(), vals[sl]):
                s = dt(s - dt(v * x[j]))
            if unit:
                x[i] = s
            else:
                assert d >= 0, f"row {i} stores no diagonal"
                x[i] = dt(s / vals[d])
    return x


def levels(n, rowptr, colind, lower=True):
    """level_of (uint64, n) and the number of levels: 0 for a row that reads no other row of the triangle, else one more
    than the deepest row it reads."""
    level_of = np.zeros(n, dtype=np.uint64)
    rp = [int(p) for p in rowptr]
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        cols = colind[rp[i]:rp[i + 1]]
        sl, _ = _used(i, cols, lower)
        used = cols[sl]
        if used.size:
            level_of[i] = level_of[used.astype(np.int64)].max() + 1
    return level_of, (int(level_of.max()) + 1 if n else 0)


def level_widths(level_of, nlevels):
    return np.bincount(level_of.astype(np.int64), minlength=nlevels).tolist()


def solve_by_levels(n, rowptr, colind, values, b, lower=True, unit=False):
    """solve_loop's arithmetic, a level at a time: the k-th used entry of every row of the level in one numpy
    operation (elementwise multiply, then elementwise subtract: two roundings, as in the loop)."""
    level_of, nl = levels(n, rowptr, colind, lower)
    rp = rowptr.astype(np.int64)
    ci = colind.astype(np.int64)
    erow = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    # first entry with column >= row, per row, and whether it is the diagonal
    dlo = rp[:-1] + np.bincount(erow[ci < erow], minlength=n)
    has = np.zeros(n, dtype=bool)
    inside = dlo < rp[1:]
    has[inside] = ci[dlo[inside]] == np.flatnonzero(inside)
    p0 = rp[:-1] if lower else dlo + has
    p1 = dlo if lower else rp[1:]
    order = np.argsort(level_of, kind="stable")
    cuts = np.concatenate([[0], np.cumsum(np.bincount(level_of.astype(np.int64), minlength=nl))])
    x = np.zeros(n, dtype=values.dtype)
    with np.errstate(all="ignore"):
        for l in range(nl):
            rows = order[cuts[l]:cuts[l + 1]]
            s = b[rows].astype(values.dtype)
            cnt = p1[rows] - p0[rows]
            for k in range(int(cnt.max()) if rows.size else 0):
                m = cnt > k
                p = p0[rows[m]] + k
                s[m] = s[m] - values[p] * x[ci[p]]
            if unit:
                x[rows] = s
            else:
                assert has[rows].all(), "a row stores no diagonal"
                x[rows] = s / values[dlo[rows]]
    return x


# ---- patterns: (n, rowptr, colind) with uint64 indices, columns strictly ascending inside a row ----------------------

def from_coo(n, rows, cols):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    key = np.unique(rows * n + cols)
    rows, cols = key // n, key % n
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.uint64)
    return n, rowptr, cols.astype(np.uint64)


def mirror(pattern):
    """(i, j) -> (n-1-i, n-1-j): a lower pattern becomes an upper one with the same dependency graph, hence the same
    level widths."""
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    return from_coo(n, n - 1 - rows, n - 1 - colind.astype(np.int64))


def _with_diag(n, rows, cols):
    d = np.arange(n, dtype=np.int64)
    return from_coo(n, np.concatenate([np.asarray(rows, dtype=np.int64), d]),
                    np.concatenate([np.asarray(cols, dtype=np.int64), d]))


def diagonal(n):
    return _with_diag(n, [], [])


def bidiagonal(n):
    i = np.arange(1, n, dtype=np.int64)
    return _with_diag(n, i, i - 1)


def dense_triangle(n):
    r, c = np.tril_indices(n, -1)
    return _with_diag(n, r, c)


def banded(n, off, window, rng):
    """`off` off-diagonal entries per row at random inside [i - window, i), plus the diagonal."""
    i = np.repeat(np.arange(1, n, dtype=np.int64), off)
    back = rng.integers(1, window + 1, size=i.size)
    j = np.maximum(i - back, 0)
    return _with_diag(n, i, j)


def arrow(n):
    """Dense last row and dense first column: one very long row, and one level of n - 2 rows."""
    i = np.arange(1, n, dtype=np.int64)
    j = np.arange(0, n - 1, dtype=np.int64)
    return _with_diag(n, np.concatenate([i, np.full(n - 1, n - 1)]), np.concatenate([np.zeros(n - 1, np.int64), j]))


def chains(lengths):
    """Independent chains laid out level by level: level l holds one row of every chain longer than l, so the levels
    narrow from len(lengths) rows to one."""
    lengths = np.sort(np.asarray(lengths, dtype=np.int64))[::-1]
    rows, cols, prev, n = [], [], None, 0
    for l in range(int(lengths[0])):
        w = int((lengths > l).sum())
        cur = np.arange(n, n + w, dtype=np.int64)
        if prev is not None:
            rows.append(cur)
            cols.append(prev[:w])
        prev, n = cur, n + w
    return _with_diag(n, np.concatenate(rows) if rows else [], np.concatenate(cols) if cols else [])


PRESCRIBED_WIDTHS = (1, 1023, 1024, 1025, 1, 2049, 3, 1)


def prescribed(widths, rng):
    """Rows in level order with exactly these level widths: every row of level l > 0 reads 1-3 rows of level l - 1."""
    rows, cols, n, prev0 = [], [], 0, 0
    for l, w in enumerate(widths):
        if l:
            pw = widths[l - 1]
            for k in range(w):
                deps = rng.choice(pw, size=min(pw, int(rng.integers(1, 4))), replace=False)
                rows += [n + k] * deps.size
                cols += (prev0 + deps).tolist()
        prev0, n = n, n + w
    return _with_diag(n, rows, cols)


def full(n, per_row, rng):
    """Both triangles stored: per_row random off-diagonal entries per row, plus the diagonal."""
    i = np.repeat(np.arange(n, dtype=np.int64), per_row)
    j = rng.integers(0, n, size=i.size)
    keep = i != j
    return _with_diag(n, i[keep], j[keep])


def drop_diagonal(pattern, row):
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    keep = ~((rows == row) & (colind.astype(np.int64) == row))
    return from_coo(n, rows[keep], colind.astype(np.int64)[keep])


def fill(pattern, dtype, rng):
    """Values and a right-hand side in (-1, 1); d_i = 1 + the sum of |off-diagonal| of row i (both triangles' entries
    counted, so either triangle of the matrix gives |x| <= max |b| by induction: nothing overflows)."""
    n, rowptr, colind = pattern
    values = rng.uniform(-1, 1, size=colind.size).astype(dtype)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    isd = rows == colind.astype(np.int64)
    off = np.bincount(rows[~isd], weights=np.abs(values[~isd]).astype(np.float64), minlength=n)
    values[isd] = (1.0 + off[rows[isd]]).astype(dtype)
    b = rng.uniform(-1, 1, size=n).astype(dtype)
    return values, b
