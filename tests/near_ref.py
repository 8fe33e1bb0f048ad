"""CPU restatement of the Chebyshev series, the delta filter's coefficients and eigsh near sigma (include/spal.h,
DESIGN 3.28): the sequential texts.  Built on cheb_ref (rowsum, gershgorin, default_tol) and eigsh_ref (the Gram-Schmidt
passes, the projected problem, the rotation) and krylov_ref's dot; only the series, the coefficients and the interval
are new, and the phase loop is the filtered text's with the series as the step's product and no warm-up.
"""
import numpy as np

from tests import cheb_ref as C
from tests import eigsh_ref as E
from tests.krylov_ref import dot

MAX_DEGREE = 4096


def delta_coefficients(degree, gamma):
    """coef[0..d] of the Fejer-damped delta function at gamma in host doubles, only + - * /; None when refused"""
    if not 1 <= degree <= MAX_DEGREE:
        return None
    gamma = np.float64(gamma)
    if not -1.0 < gamma < 1.0:
        return None
    d1 = np.float64(degree + 1)
    g2 = np.float64(2) * gamma
    m = [np.float64(1), gamma]
    for i in range(2, degree + 1):
        m.append((g2 * m[i - 1]) - m[i - 2])
    u = [(d1 / d1) * m[0]] + [(np.float64(degree + 1 - i) / d1) * (np.float64(2) * m[i]) for i in range(1, degree + 1)]
    nrm = np.float64(0)
    with np.errstate(all="ignore"):
        for i in range(degree + 1):
            nrm = nrm + u[i] * m[i]
        if not np.isfinite(nrm) or nrm == 0:
            return None
        return np.array([ui / nrm for ui in u], dtype=np.float64)


def series_scalars(lo, hi, coef, dtype):
    """(a1, a2, cT, k[0..d]) in the dtype; host doubles until the one conversion"""
    dt = np.dtype(dtype).type
    lo, hi = np.float64(lo), np.float64(hi)
    c = (lo + hi) / np.float64(2)
    e = (hi - lo) / np.float64(2)
    return dt(np.float64(1) / e), dt(np.float64(2) / e), dt(c), np.asarray(coef, dtype=np.float64).astype(dt)


def cheb_series(rowptr, colind, values, x, lo, hi, coef, keep_t=False):
    """s of the text (and t_d with keep_t); x and the values share one dtype"""
    a1, a2, cT, k = series_scalars(lo, hi, coef, values.dtype)
    d = len(k) - 1
    assert 1 <= d <= MAX_DEGREE
    with np.errstate(all="ignore"):
        t0 = np.asarray(x, dtype=values.dtype)
        s = k[0] * t0
        t1 = a1 * (C.rowsum(rowptr, colind, values, t0) - (cT * t0))
        s = s + (k[1] * t1)
        for i in range(2, d + 1):
            t2 = (a2 * (C.rowsum(rowptr, colind, values, t1) - (cT * t1))) - t0
            s = s + (k[i] * t2)
            t0, t1 = t1, t2
    return (s, t1) if keep_t else s


def auto_interval(glo, ghi):
    m = (np.float64(ghi) - np.float64(glo)) / np.float64(1024)
    return np.float64(glo) - m, np.float64(ghi) + m


def near_filter(degree, sigma, lo, hi):
    """(gamma, coef), or None when the text refuses: sigma not strictly inside, or the coefficients refused"""
    lo, hi, sigma = np.float64(lo), np.float64(hi), np.float64(sigma)
    if not lo < sigma < hi:
        return None
    c = (lo + hi) / np.float64(2)
    e = (hi - lo) / np.float64(2)
    gamma = (sigma - c) / e
    coef = delta_coefficients(degree, gamma)
    return None if coef is None else (gamma, coef)


def eigsh_near(csr, dtype, k, sigma, ncv, tol, maxit, degree, interval=None, v0=None, seed=0, jacobi_fn=None):
    """csr = (rowptr, colind, values) of the CSR form.  dict(theta, resid, X, restarts, products, converged, reason, pairs,
    lo, hi, sigma, gamma, degree); "refused" in place of a dict where the text refuses the call after Gershgorin."""
    rowptr, colind, values = csr
    dt = np.dtype(dtype).type
    values = np.asarray(values, dtype=dt)
    n, m = len(rowptr) - 1, int(ncv)
    assert 0 < k < m <= n and 2 <= degree <= MAX_DEGREE
    if tol == 0:
        tol = C.default_tol(dt)

    def mul(v):
        return C.rowsum(rowptr, colind, values, v)

    glo, ghi = C.gershgorin(rowptr, colind, values)
    extra = dict(lo=0.0, hi=0.0, sigma=float(sigma), gamma=0.0, degree=degree)
    none = dict(theta=np.zeros(0, dt), resid=np.zeros(0, dt), X=np.zeros((n, 0), dt), converged=0, reason=2, pairs=0)
    if not (np.isfinite(glo) and np.isfinite(ghi)):
        return dict(none, restarts=0, products=0, **extra)
    scale = max(abs(glo), abs(ghi))
    lo, hi = auto_interval(glo, ghi) if interval is None else (np.float64(interval[0]), np.float64(interval[1]))
    f = near_filter(degree, sigma, lo, hi)
    if f is None:
        return "refused"
    gamma, coef = f
    extra.update(lo=float(lo), hi=float(hi), gamma=float(gamma))

    with np.errstate(all="ignore"):
        v0 = E.default_start(n, seed, dt) if v0 is None else np.asarray(v0, dtype=dt)
        V = [v0 / np.sqrt(dot(v0, v0))]
        S = np.zeros((m, m), dtype=np.float64)
        keep = restarts = products = 0

        while True:
            exhausted = False
            jj = keep
            for j in range(keep, m):
                w = cheb_series(rowptr, colind, values, V[j], lo, hi, coef)
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
            r = E.ritz(S[:jj, :jj], hn, E.LA, jacobi_fn)      # descending: rho is largest nearest sigma
            if r is None:
                return dict(none, restarts=restarts, products=products, **extra)
            mu, Y, _ = r
            nk = min(k, jj)
            kc = min(E.keep_of(k, m), jj)
            Vn = E.rotate(V[:jj], Y, kc, dt)                  # rotate first: the columns are the restart's
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
