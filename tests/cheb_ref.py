"""CPU restatement of the Chebyshev filter and of filtered eigsh (include/spal.h): the sequential text.
`rowsum` is the filter's own product order -- the stored entries of a row of the CSR form, in storage order, added left
to right onto +0.0, every product rounded --, `coefficients` the host doubles of the three-term recurrence, `cheb_apply`
the recurrence, `gershgorin` the enclosure in double, and `eigsh_filtered` the text of eigsh (tests/eigsh_ref.py) with
its five changes.  Built on eigsh_ref and krylov_ref: the Gram-Schmidt passes, the dot, the Jacobi text and the rotation
are theirs.
"""
import numpy as np

from tests import eigsh_ref as E
from tests.krylov_ref import dot

LA, SA = E.LA, E.SA
MAX_DEGREE = 256


LONG = 64      # rows above this many entries are summed one by one (numpy's cumsum is the same left-to-right chain)


def rowsum(rowptr, colind, values, y):
    """q[r] = (..((+0.0 + (a[p]*y[col[p]])) + (a[p+1]*y[col[p+1]])) ..) over row r's entries in storage order.  Column by
    column of the rows' entries, so the loop runs at most LONG times; a longer row is one cumsum that starts at +0.0: the
    same additions in the same order either way."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colind = np.asarray(colind, dtype=np.int64)
    n = rowptr.size - 1
    dt = values.dtype
    acc = np.zeros(n, dtype=dt)                 # +0.0, and it is added
    length = np.diff(rowptr)
    short = np.where(length <= LONG, length, 0)
    with np.errstate(all="ignore"):
        for t in range(int(short.max()) if n else 0):
            rows = np.nonzero(short > t)[0]
            p = rowptr[rows] + t
            acc[rows] = acc[rows] + values[p] * y[colind[p]]
        for r in np.nonzero(length > LONG)[0]:
            p = slice(rowptr[r], rowptr[r + 1])
            acc[r] = np.cumsum(np.concatenate([np.zeros(1, dt), values[p] * y[colind[p]]]), dtype=dt)[-1]
    return acc


def csc_to_csr(nrows, colptr, rowind, values):
    """the CSR twin of a CSC matrix: a stable sort of the entries by row, so a row's entries come in column order"""
    colptr = np.asarray(colptr, dtype=np.int64)
    cols = np.repeat(np.arange(colptr.size - 1, dtype=np.int64), np.diff(colptr))
    order = np.argsort(np.asarray(rowind, dtype=np.int64), kind="stable")
    rowptr = np.zeros(nrows + 1, dtype=np.int64)
    np.cumsum(np.bincount(np.asarray(rowind, dtype=np.int64), minlength=nrows), out=rowptr[1:])
    return rowptr, cols[order], np.asarray(values)[order]


def check_interval(degree, lo, hi, a0):
    """the refusals of the text, in its order; None when the arguments are fine"""
    if not 1 <= degree <= MAX_DEGREE:
        return "degree"
    if not (np.isfinite(lo) and np.isfinite(hi) and np.isfinite(a0)):
        return "not finite"
    if not lo < hi:
        return "lo >= hi"
    if lo <= a0 <= hi:
        return "a0 inside"
    return None


def coefficients(degree, lo, hi, a0, dtype):
    """(alpha[1..d], beta[1..d], cT) as arrays of the dtype, index 0 = step 1; host doubles until the last conversion"""
    dt = np.dtype(dtype).type
    lo, hi, a0 = np.float64(lo), np.float64(hi), np.float64(a0)
    c = (lo + hi) / np.float64(2)
    e = (hi - lo) / np.float64(2)
    s1 = e / (a0 - c)
    alpha, beta = [dt(s1 / e)], [dt(0)]
    s_prev = s1
    for _ in range(2, degree + 1):
        s = np.float64(1) / (np.float64(2) / s1 - s_prev)
        alpha.append(dt((np.float64(2) * s) / e))
        beta.append(dt(s_prev * s))
        s_prev = s
    return np.array(alpha, dtype=dt), np.array(beta, dtype=dt), dt(c)


def cheb_apply(rowptr, colind, values, x, degree, lo, hi, a0):
    """t_d of the text; x and the values share one dtype"""
    assert check_interval(degree, lo, hi, a0) is None
    alpha, beta, cT = coefficients(degree, lo, hi, a0, values.dtype)
    with np.errstate(all="ignore"):
        t0 = np.asarray(x, dtype=values.dtype)
        t1 = alpha[0] * (rowsum(rowptr, colind, values, t0) - (cT * t0))
        for i in range(1, degree):
            t2 = (alpha[i] * (rowsum(rowptr, colind, values, t1) - (cT * t1))) - (beta[i] * t0)
            t0, t1 = t1, t2
    return t1


def gershgorin(rowptr, colind, values):
    """(glo, ghi) in double: per row d = the stored diagonal entry (0 without one; the last one stored if the row holds
    several), s = the |off-diagonal entries| added in storage order onto +0.0; glo = min(d - s), ghi = max(d + s).  A row
    value that is not finite makes both NaN."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = rowptr.size - 1
    lo, hi = np.empty(n), np.empty(n)
    with np.errstate(all="ignore"):
        for r in range(n):
            d = s = np.float64(0)
            for p in range(rowptr[r], rowptr[r + 1]):
                v = np.float64(values[p])
                if int(colind[p]) == r:
                    d = v
                else:
                    s = s + abs(v)
            lo[r], hi[r] = d - s, d + s
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        return np.float64(np.nan), np.float64(np.nan)
    return lo.min(), hi.max()


def default_tol(dtype):
    return 256.0 * float(np.finfo(dtype).eps)


def eigsh_filtered(csr, dtype, k, which, ncv, tol, maxit, degree, interval=None, warmup=5, v0=None, seed=0, jacobi_fn=None,
                   mul_plain=None):
    """csr = (rowptr, colind, values) of the CSR form.  dict(theta, resid, X, restarts, products, converged, reason,
    pairs, warm_restarts, warm_products, lo, hi, a0, degree).  interval = None: automatic.  mul_plain: the product of
    the warm-up, which is eigsh's text unchanged and so the handle's product on the device (None: rowsum)."""
    rowptr, colind, values = csr
    dt = np.dtype(dtype).type
    values = np.asarray(values, dtype=dt)
    which = E.WHICH.get(which, which)
    n, m = len(rowptr) - 1, int(ncv)
    assert 0 < k < m <= n and 1 <= degree <= MAX_DEGREE
    if tol == 0:
        tol = default_tol(dt)

    def mul(v):
        return rowsum(rowptr, colind, values, v)

    glo, ghi = gershgorin(rowptr, colind, values)
    a0 = ghi if which == LA else glo
    extra = dict(warm_restarts=0, warm_products=0, lo=0.0, hi=0.0, a0=float(a0), degree=degree)
    if not (np.isfinite(glo) and np.isfinite(ghi)):
        return dict(theta=np.zeros(0, dt), resid=np.zeros(0, dt), X=np.zeros((n, 0), dt), restarts=0, products=0, converged=0,
                    reason=2, pairs=0, **extra)
    scale = max(abs(glo), abs(ghi))
    if interval is None:
        warm = E.eigsh(mul_plain or mul, n, dt, k, which, m, tol, min(warmup, maxit), v0=v0, seed=seed, jacobi_fn=jacobi_fn)
        extra.update(warm_restarts=warm["restarts"], warm_products=warm["products"])
        if warm["reason"] != 1:
            return dict(warm, **extra)
        cut = np.float64(warm["theta"][k - 1])
        if not glo < cut < ghi:
            return dict(warm, **extra)
        lo, hi = (glo, cut) if which == LA else (cut, ghi)
    else:
        lo, hi = np.float64(interval[0]), np.float64(interval[1])
        assert check_interval(degree, lo, hi, a0) is None and (a0 > hi if which == LA else a0 < lo)
    extra.update(lo=float(lo), hi=float(hi))

    with np.errstate(all="ignore"):
        v0 = E.default_start(n, seed, dt) if v0 is None else np.asarray(v0, dtype=dt)
        V = [v0 / np.sqrt(dot(v0, v0))]
        S = np.zeros((m, m), dtype=np.float64)
        keep = restarts = products = 0
        none = dict(theta=np.zeros(0, dt), resid=np.zeros(0, dt), X=np.zeros((n, 0), dt), converged=0, reason=2, pairs=0)

        while True:
            exhausted = False
            jj = keep
            for j in range(keep, m):
                w = cheb_apply(rowptr, colind, values, V[j], degree, lo, hi, a0)
                h, w = E._project(V[:j + 1], w, dt)
                c, w = E._project(V[:j + 1], w, dt)
                h = [dt(hk + ck) for hk, ck in zip(h, c)]
                hn = np.sqrt(dot(w, w))
                V.append(w / hn)
                products += degree
                S[:j + 1, j] = S[j, :j + 1] = np.array(h, dtype=np.float64)
                jj = j + 1
                if not np.isfinite(hn):
                    return dict(none, restarts=restarts, products=products, **extra)
                if hn == 0:
                    exhausted = True
                    break
            r = E.ritz(S[:jj, :jj], hn, LA, jacobi_fn)      # descending in p for both sides
            if r is None:
                return dict(none, restarts=restarts, products=products, **extra)
            mu, Y, _ = r
            nk = min(k, jj)
            kc = min(E.keep_of(k, m), jj)
            # rotate first: the columns are the restart's
            Vn = E.rotate(V[:jj], Y, kc, dt)
            th, res = [], []
            for c in range(nk):
                q = mul(Vn[c])
                products += 1
                t = dot(Vn[c], q)
                rc = q - (t * Vn[c])
                th.append(t)
                res.append(np.sqrt(dot(rc, rc)))
            th, res = np.array(th, dtype=dt), np.array(res, dtype=dt)
            if not (np.all(np.isfinite(th)) and np.all(np.isfinite(res))):
                return dict(none, restarts=restarts, products=products, **extra)
            conv = 0
            while conv < nk and np.float64(res[conv]) <= np.float64(tol) * scale:
                conv += 1
            reason = None
            if exhausted:
                reason = 0 if jj >= k else 3
                if reason == 3:
                    conv = nk
            elif conv == k:
                reason = 0
            elif restarts == maxit:
                reason = 1
            if reason is not None:
                return dict(theta=th, resid=res, X=np.stack(Vn[:nk], axis=1), restarts=restarts, products=products,
                            converged=conv, reason=reason, pairs=nk, **extra)
            keep = kc
            V = Vn + [V[m]]
            S = np.zeros((m, m), dtype=np.float64)
            S[np.arange(keep), np.arange(keep)] = mu[:keep]
            restarts += 1


# ---- the matrices of the tests -----------------------------------------------------------------------------------------

def laplace_1d_csr(n, dtype):
    """the 1-D Laplacian tridiag(-1, 2, -1) as (rowptr, colind, values)"""
    rows, cols, vals = [], [], []
    for i in range(n):
        for j, v in ((i - 1, -1.0), (i, 2.0), (i + 1, -1.0)):
            if 0 <= j < n:
                rows.append(i)
                cols.append(j)
                vals.append(v)
    rowptr = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr, np.array(cols, dtype=np.uint64), np.array(vals, dtype=dtype)
