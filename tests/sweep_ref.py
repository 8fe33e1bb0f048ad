"""CPU restatement of the Jacobi sweeps on a triangle (include/spal.h).

The contract is `sweep_loop`: x0[i] = b[i] / d[i] (b[i] with a unit diagonal); for t = 1 .. s every row on its own:
acc = b[i]; for every stored entry (i, j, v) of the chosen triangle off the diagonal, in ascending column,
acc = acc - (v * x(t-1)[j]) with the product and the difference rounded separately in the matrix dtype;
xt[i] = acc / d[i] (acc with a unit diagonal).  `sweep_vec` is the same arithmetic with the k-th used entry of every row
taken in one numpy operation (elementwise multiply, then elementwise subtract: two roundings, as in the loop);
tests/test_sweep_host.py proves the two bit-equal, and the larger device tests use the faster one.
"""
import numpy as np

from . import trsv_ref as tr

assert_same_bits = tr.assert_same_bits


def sweep_loop(n, rowptr, colind, values, b, sweeps, lower=True, unit=False):
    """THE definition, in numpy scalars of the matrix dtype."""
    dt = values.dtype.type
    rp = [int(p) for p in rowptr]
    used = []
    for i in range(n):
        cols = colind[rp[i]:rp[i + 1]]
        sl, d = tr._used(i, cols, lower)
        if not unit:
            assert d >= 0, f"row {i} stores no diagonal"
        used.append((cols[sl].tolist(), values[rp[i]:rp[i + 1]][sl], None if unit else values[rp[i] + d]))
    with np.errstate(all="ignore"):
        x = np.array([dt(b[i]) if unit else dt(dt(b[i]) / used[i][2]) for i in range(n)], dtype=values.dtype)
        for _ in range(sweeps):
            nxt = np.empty_like(x)
            for i in range(n):
                cols, vals, d = used[i]
                acc = dt(b[i])
                for j, v in zip(cols, vals):
                    acc = dt(acc - dt(v * x[j]))
                nxt[i] = acc if unit else dt(acc / d)
            x = nxt
    return x


def triangle_ranges(n, rowptr, colind, lower):
    """Per row: the positions [p0, p1) of its entries of the triangle off the diagonal, the position of its first entry
    with column >= row, and whether that entry is the diagonal."""
    rp = rowptr.astype(np.int64)
    ci = colind.astype(np.int64)
    erow = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    dlo = rp[:-1] + np.bincount(erow[ci < erow], minlength=n)
    has = np.zeros(n, dtype=bool)
    inside = dlo < rp[1:]
    has[inside] = ci[dlo[inside]] == np.flatnonzero(inside)
    return (rp[:-1], dlo, dlo, has) if lower else (dlo + has, rp[1:], dlo, has)


def sweep_vec(n, rowptr, colind, values, b, sweeps, lower=True, unit=False):
    """sweep_loop's arithmetic, the k-th used entry of every row at once."""
    p0, p1, dlo, has = triangle_ranges(n, rowptr, colind, lower)
    ci = colind.astype(np.int64)
    cnt = p1 - p0
    order = np.argsort(-cnt, kind="stable")          # rows by falling count: those with a k-th entry are a prefix
    sorted_cnt = cnt[order]
    bb = np.asarray(b).astype(values.dtype)
    with np.errstate(all="ignore"):
        if unit:
            x = bb.copy()
        else:
            assert has.all(), "a row stores no diagonal"
            d = values[dlo]
            x = bb / d
        for _ in range(sweeps):
            acc = bb.copy()
            for k in range(int(cnt.max()) if n else 0):
                rows = order[:int(np.searchsorted(-sorted_cnt, -k, side="left"))]     # rows with cnt > k
                p = p0[rows] + k
                acc[rows] = acc[rows] - values[p] * x[ci[p]]
            x = acc if unit else acc / d
    return x


def preconditioner(pattern, factor_values, sweeps):
    """v -> M^-1 v as spal_*_krylov_* applies a factor whose "trsv_sweeps" is `sweeps`: the lower triangle with its unit
    diagonal, then the upper one with the stored diagonal."""
    def apply(v):
        y = sweep_vec(*pattern, factor_values, v, sweeps, lower=True, unit=True)
        return sweep_vec(*pattern, factor_values, y, sweeps, lower=False, unit=False)
    return apply


def poisson2d(m):
    """The 5-point Laplacian on an m x m grid: (pattern, float64 values), 4 on the diagonal and -1 beside it."""
    idx = np.arange(m * m, dtype=np.int64).reshape(m, m)
    rows = [idx.ravel(), idx[:, 1:].ravel(), idx[:, :-1].ravel(), idx[1:, :].ravel(), idx[:-1, :].ravel()]
    cols = [idx.ravel(), idx[:, :-1].ravel(), idx[:, 1:].ravel(), idx[:-1, :].ravel(), idx[1:, :].ravel()]
    pattern = tr.from_coo(m * m, np.concatenate(rows), np.concatenate(cols))
    n, rowptr, colind = pattern
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    values = np.where(r == colind.astype(np.int64), 4.0, -1.0)
    return pattern, values
