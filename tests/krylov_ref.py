"""CPU restatement of the dot product, CG and BiCGStab (include/spal.h) and the matrices their tests use.

`reduce` / `dot` are THE definition: products rounded, padded with +0.0 to whole tiles of 1024, every tile halved
(h = 512 .. 1: e[t] = e[t] + e[t + h]), the tile sums reduced the same way.  `cg` and `bicgstab` are the loops of the
header with every scalar in the vectors' dtype and every product rounded before the sum it enters.  They take the product
and the preconditioner as callables, so the same text runs on pure host operations (oracle.csr_spmv,
trsv_ref.solve_by_levels) or on the device's own spmv / solve_triangular.
"""
import numpy as np

TILE = 1024


def reduce(v):
    v = np.asarray(v)
    c = max(1, -(-v.size // TILE))
    e = np.zeros(TILE * c, dtype=v.dtype)       # +0.0, and it is added
    e[:v.size] = v
    e = e.reshape(c, TILE)
    h = TILE // 2
    with np.errstate(all="ignore"):
        while h >= 1:
            e = e[:, :h] + e[:, h:2 * h]
            h //= 2
    sums = np.ascontiguousarray(e[:, 0])
    return sums[0] if c == 1 else reduce(sums)


def dot(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.ndim == 1
    with np.errstate(all="ignore"):
        return reduce(a * b)


def sequential_sum(v):
    """e[0] + e[1] + ... left to right, in the vector's dtype: an order the definition is NOT."""
    return np.cumsum(v, dtype=v.dtype)[-1]


def _stop(rr, thr, it, maxit):
    """The test: the reason, or None to go on."""
    if rr <= thr:
        return 0
    if not np.isfinite(rr):
        return 2
    if it == maxit:
        return 1
    return None


def _result(x, it, reason, rr, bb):
    return x, dict(iterations=it, reason=reason, residual_sq=float(rr), rhs_sq=float(bb))


def cg(mul, prec, b, x0, tol, maxit):
    """prec = None: M^-1 v is v itself."""
    dt = b.dtype.type
    with np.errstate(all="ignore"):
        x = x0.astype(b.dtype, copy=True)
        bb = dot(b, b)
        thr = dt(dt(tol * tol) * bb)
        r = b - mul(x)
        rr = dot(r, r)
        it = 0
        reason = _stop(rr, thr, it, maxit)
        if reason is not None:
            return _result(x, it, reason, rr, bb)
        z = r if prec is None else prec(r)
        p = z.copy()
        rz = dot(r, z)
        while True:
            q = mul(p)
            alpha = dt(rz / dot(p, q))
            x = x + alpha * p
            r = r - alpha * q
            it += 1
            rr = dot(r, r)
            reason = _stop(rr, thr, it, maxit)
            if reason is not None:
                return _result(x, it, reason, rr, bb)
            z = r if prec is None else prec(r)
            rz1 = dot(r, z)
            beta = dt(rz1 / rz)
            rz = rz1
            p = z + beta * p


def bicgstab(mul, prec, b, x0, tol, maxit):
    dt = b.dtype.type
    with np.errstate(all="ignore"):
        x = x0.astype(b.dtype, copy=True)
        bb = dot(b, b)
        thr = dt(dt(tol * tol) * bb)
        r = b - mul(x)
        rhat = r.copy()
        rho = alpha = omega = dt(1)
        v = np.zeros_like(b)
        p = np.zeros_like(b)
        rr = dot(r, r)
        it = 0
        reason = _stop(rr, thr, it, maxit)
        if reason is not None:
            return _result(x, it, reason, rr, bb)
        while True:
            rho1 = dot(rhat, r)
            beta = dt(dt(rho1 / rho) * dt(alpha / omega))
            rho = rho1
            p = r + beta * (p - omega * v)
            ph = p if prec is None else prec(p)
            v = mul(ph)
            alpha = dt(rho / dot(rhat, v))
            s = r - alpha * v
            it += 1
            ss = dot(s, s)
            if ss <= thr or not np.isfinite(ss):                  # the half-step exit
                return _result(x + alpha * ph, it, 0 if ss <= thr else 2, ss, bb)
            sh = s if prec is None else prec(s)
            t = mul(sh)
            omega = dt(dot(t, s) / dot(t, t))
            x = (x + alpha * ph) + omega * sh
            r = s - omega * t
            rr = dot(r, r)
            reason = _stop(rr, thr, it, maxit)
            if reason is not None:
                return _result(x, it, reason, rr, bb)


METHODS = {"cg": cg, "bicgstab": bicgstab}


def spd_fill(pattern, dtype, rng):
    """Symmetric, diagonally dominant values on a structurally symmetric pattern (d_i = 1 + the sum of |off-diagonal| of
    row i): the matrix is symmetric positive definite.  Returns (values, b)."""
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    cols = colind.astype(np.int64)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    key = lo * n + hi
    uniq, inverse = np.unique(key, return_inverse=True)
    values = rng.uniform(-1, 1, size=uniq.size)[inverse].astype(dtype)      # (i, j) and (j, i) share one value
    isd = rows == cols
    pair = np.bincount(inverse[~isd], minlength=uniq.size)
    assert np.all(pair[np.unique(inverse[~isd])] == 2), "the pattern is not structurally symmetric"
    off = np.bincount(rows[~isd], weights=np.abs(values[~isd]).astype(np.float64), minlength=n)
    values[isd] = (1.0 + off[rows[isd]]).astype(dtype)
    b = rng.uniform(-1, 1, size=n).astype(dtype)
    return values, b


def true_relative_residual(pattern, values, x, b):
    """||b - A x|| / ||b|| in float64 on the host."""
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    ax = np.bincount(rows, weights=values.astype(np.float64) * x.astype(np.float64)[colind.astype(np.int64)], minlength=n)
    return float(np.linalg.norm(b.astype(np.float64) - ax) / np.linalg.norm(b.astype(np.float64)))
