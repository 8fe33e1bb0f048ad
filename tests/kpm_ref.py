"""CPU restatement of the KPM moments (include/spal.h): the sequential text.  Built on cheb_ref's rowsum and
gershgorin, krylov_ref's dot and near_ref's interval; only the probe hash, the recurrence with its doubling identities and
the direct moments (for the host tests) are new.  Matrix builders of the tests are at the end.
"""
import numpy as np

from tests import cheb_ref as C
from tests import near_ref as N
from tests.krylov_ref import TILE, dot

MAX_DEGREE = 4096
MAX_PROBES = 256


def mix32(x):
    """the text's hash of one 32-bit word, a scalar loop"""
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def probes_scalar(n, k, seed, dtype):
    """z[i, j] of the text, entry by entry"""
    z = np.empty((n, k), dtype=dtype)
    for i in range(n):
        h = mix32((i + seed) % 2**32)
        for j in range(k):
            z[i, j] = -1 if mix32((h + j) % 2**32) >> 31 else 1
    return z


def scalars(lo, hi, dtype):
    """(a1, a2, cT) in the dtype; host doubles until the one conversion"""
    dt = np.dtype(dtype).type
    lo, hi = np.float64(lo), np.float64(hi)
    c = (lo + hi) / np.float64(2)
    e = (hi - lo) / np.float64(2)
    return dt(np.float64(1) / e), dt(np.float64(2) / e), dt(c)


def auto_interval(rowptr, colind, values):
    glo, ghi = C.gershgorin(rowptr, colind, values)
    return N.auto_interval(glo, ghi)


def moments_column(rowptr, colind, values, z, degree, lo, hi):
    """mu_0 .. mu_d of one column in the values' dtype: the text"""
    assert 1 <= degree <= MAX_DEGREE
    dt = values.dtype.type
    a1, a2, cT = scalars(lo, hi, values.dtype)
    m = (degree + 1) // 2
    mu = np.zeros(degree + 1, dtype=values.dtype)
    with np.errstate(all="ignore"):
        t0 = np.ascontiguousarray(z, dtype=values.dtype)
        t1 = a1 * (C.rowsum(rowptr, colind, values, t0) - (cT * t0))
        mu[0] = dot(t0, t0)
        mu[1] = dot(t1, t0)
        tp, ti = t0, t1                      # t_{i-1}, t_i
        for i in range(1, m + 1):
            if i >= 2:
                tn = (a2 * (C.rowsum(rowptr, colind, values, ti) - (cT * ti))) - tp
                tp, ti = ti, tn
                mu[2 * i - 1] = (dt(2) * dot(ti, tp)) - mu[1]
            if 2 * i <= degree:
                mu[2 * i] = (dt(2) * dot(ti, ti)) - mu[0]
    return mu


def rowsum_block(rowptr, colind, values, Y):
    """cheb_ref.rowsum on every column of Y at once: the same additions in the same order per element"""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colind = np.asarray(colind, dtype=np.int64)
    n = rowptr.size - 1
    dt = values.dtype
    acc = np.zeros((n, Y.shape[1]), dtype=dt)   # +0.0, and it is added
    length = np.diff(rowptr)
    short = np.where(length <= C.LONG, length, 0)
    with np.errstate(all="ignore"):
        for t in range(int(short.max()) if n else 0):
            rows = np.nonzero(short > t)[0]
            p = rowptr[rows] + t
            acc[rows] = acc[rows] + values[p][:, None] * Y[colind[p]]
        for r in np.nonzero(length > C.LONG)[0]:
            p = slice(rowptr[r], rowptr[r + 1])
            prods = values[p][:, None] * Y[colind[p]]
            acc[r] = np.cumsum(np.concatenate([np.zeros((1, Y.shape[1]), dt), prods]), axis=0, dtype=dt)[-1]
    return acc


def reduce_columns(V):
    """krylov_ref.reduce on every column of V (m, k) at once: the same tree per column"""
    m, k = V.shape
    c = max(1, -(-m // TILE))
    e = np.zeros((TILE * c, k), dtype=V.dtype)   # +0.0, and it is added
    e[:m] = V
    e = e.reshape(c, TILE, k)
    h = TILE // 2
    with np.errstate(all="ignore"):
        while h >= 1:
            e = e[:, :h] + e[:, h:2 * h]
            h //= 2
    sums = np.ascontiguousarray(e[:, 0, :])
    return sums[0] if c == 1 else reduce_columns(sums)


def dots(A, B):
    """dot of every column pair"""
    with np.errstate(all="ignore"):
        return reduce_columns(A * B)


def moments(csr, Z, degree, interval=None):
    """out[i, j] = double(mu_i of column j); csr = (rowptr, colind, values), Z an (n, k) block of the values' dtype.  The
    text of moments_column on all columns at once (the columns are independent)."""
    rowptr, colind, values = csr
    lo, hi = auto_interval(rowptr, colind, values) if interval is None else interval
    assert 1 <= degree <= MAX_DEGREE
    dt = values.dtype.type
    a1, a2, cT = scalars(lo, hi, values.dtype)
    m = (degree + 1) // 2
    T0 = np.ascontiguousarray(Z, dtype=values.dtype)
    mu = np.zeros((degree + 1, T0.shape[1]), dtype=values.dtype)
    with np.errstate(all="ignore"):
        T1 = a1 * (rowsum_block(rowptr, colind, values, T0) - (cT * T0))
        mu[0] = dots(T0, T0)
        mu[1] = dots(T1, T0)
        Tp, Ti = T0, T1
        for i in range(1, m + 1):
            if i >= 2:
                Tn = (a2 * (rowsum_block(rowptr, colind, values, Ti) - (cT * Ti))) - Tp
                Tp, Ti = Ti, Tn
                mu[2 * i - 1] = (dt(2) * dots(Ti, Tp)) - mu[1]
            if 2 * i <= degree:
                mu[2 * i] = (dt(2) * dots(Ti, Ti)) - mu[0]
    return mu.astype(np.float64)


def moments_direct(csr, z, degree, lo, hi):
    """mu_i = dot(z, t_i) for i = 0 .. d with the full recurrence: what the doubling identities replace"""
    rowptr, colind, values = csr
    a1, a2, cT = scalars(lo, hi, values.dtype)
    with np.errstate(all="ignore"):
        z0 = t0 = np.ascontiguousarray(z, dtype=values.dtype)
        t1 = a1 * (C.rowsum(rowptr, colind, values, t0) - (cT * t0))
        mu = [dot(z0, t0), dot(z0, t1)]
        for _ in range(2, degree + 1):
            t2 = (a2 * (C.rowsum(rowptr, colind, values, t1) - (cT * t1))) - t0
            mu.append(dot(z0, t2))
            t0, t1 = t1, t2
    return np.array(mu[:degree + 1], dtype=np.float64)


# ---- matrices ------------------------------------------------------------------------------------------------------
def from_dense(a, dtype):
    a = np.asarray(a)
    n = a.shape[0]
    rowptr, colind, values = [0], [], []
    for r in range(n):
        for c in np.nonzero(a[r])[0]:
            colind.append(int(c))
            values.append(a[r, c])
        rowptr.append(len(colind))
    return np.array(rowptr, dtype=np.uint64), np.array(colind, dtype=np.uint64), np.array(values, dtype=dtype)


def laplace1d(n, dtype):
    """tridiag(-1, 2, -1)"""
    rows = np.arange(n)
    r = np.concatenate([rows[1:], rows, rows[:-1]])
    c = np.concatenate([rows[1:] - 1, rows, rows[:-1] + 1])
    v = np.concatenate([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)])
    return from_triplets(n, r, c, v, dtype)


def poisson2d(m, dtype):
    """the 5-point Laplacian on an m x m grid: 4 on the diagonal, -1 to the four neighbours"""
    idx = np.arange(m * m).reshape(m, m)
    r = [idx.ravel()]
    c = [idx.ravel()]
    v = [4 * np.ones(m * m)]
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        r += [a.ravel(), b.ravel()]
        c += [b.ravel(), a.ravel()]
        v += [-np.ones(a.size), -np.ones(a.size)]
    return from_triplets(m * m, np.concatenate(r), np.concatenate(c), np.concatenate(v), dtype)


def from_triplets(n, r, c, v, dtype):
    """CSR with ascending columns inside a row; (r, c) pairs are distinct"""
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    order = np.lexsort((c, r))
    rowptr = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    return rowptr, c[order].astype(np.uint64), np.asarray(v)[order].astype(dtype)


def to_dense(csr):
    rowptr, colind, values = csr
    n = len(rowptr) - 1
    a = np.zeros((n, n), dtype=np.float64)
    for r in range(n):
        for p in range(int(rowptr[r]), int(rowptr[r + 1])):
            a[r, int(colind[p])] += float(values[p])
    return a


def csr_to_csc(csr):
    """(colptr, rowind, values) of the same matrix: a stable sort of the entries by column"""
    rowptr, colind, values = csr
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(rowptr, dtype=np.int64)))
    ci = np.asarray(colind, dtype=np.int64)
    order = np.argsort(ci, kind="stable")
    colptr = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.bincount(ci, minlength=n), out=colptr[1:])
    return colptr, rows[order].astype(np.uint64), np.asarray(values)[order]
