"""CPU restatement of MINRES on (A - shift I) x = b (include/spal.h) and the indefinite matrices its tests use.

`minres` is the text of the header with every scalar in the vectors' dtype and every product rounded before the sum it
enters; `dot` and the test are krylov_ref's.  It takes the product and the preconditioner as callables, so the same text
runs on pure host operations or on the device's own spmv / solve_triangular.
"""
import numpy as np

from tests.krylov_ref import _result, _stop, dot, spd_fill


def minres(mul, prec, b, x0, shift, tol, maxit):
    """prec = None: M^-1 v is v itself.  `mul` is A alone: the shift is applied here, as the text has it."""
    dt = b.dtype.type
    with np.errstate(all="ignore"):
        sg = dt(shift)
        x = x0.astype(b.dtype, copy=True)
        zb = b if prec is None else prec(b)
        bb = dot(b, zb)
        thr = dt(dt(tol * tol) * bb)
        q = mul(x)
        r2 = b - (q - sg * x)
        y = r2 if prec is None else prec(r2)
        beta = dt(np.sqrt(dot(r2, y)))
        phibar = beta
        pp = dt(phibar * phibar)
        it = 0
        reason = _stop(pp, thr, it, maxit)
        if reason is not None:
            return _result(x, it, reason, pp, bb)
        oldb = dbar = epsln = dt(0)
        cs, sn = dt(-1), dt(0)
        r1 = np.zeros_like(b)
        w = np.zeros_like(b)
        w2 = np.zeros_like(b)
        s = dt(dt(1) / beta)
        v = y * s
        while True:
            q = mul(v)
            c1 = dt(0) if it == 0 else dt(beta / oldb)
            t = (q - sg * v) - c1 * r1
            alfa = dot(v, t)
            c2 = dt(alfa / beta)
            t = t - c2 * r2
            r1, r2 = r2, t
            y = r2 if prec is None else prec(r2)
            oldb = beta
            beta = dt(np.sqrt(dot(r2, y)))
            it += 1
            oldeps = epsln
            delta = dt(dt(cs * dbar) + dt(sn * alfa))
            gbar = dt(dt(sn * dbar) - dt(cs * alfa))
            epsln = dt(sn * beta)
            dbar = dt(-dt(cs * beta))
            gamma = dt(np.sqrt(dt(dt(gbar * gbar) + dt(beta * beta))))
            cs = dt(gbar / gamma)
            sn = dt(beta / gamma)
            phi = dt(cs * phibar)
            phibar = dt(sn * phibar)
            denom = dt(dt(1) / gamma)
            w1, w2 = w2, w
            w = ((v - oldeps * w1) - delta * w2) * denom
            x = x + phi * w
            pp = dt(phibar * phibar)
            reason = _stop(pp, thr, it, maxit)
            if reason is not None:
                return _result(x, it, reason, pp, bb)
            s = dt(dt(1) / beta)
            v = y * s


def indefinite_fill(pattern, dtype, rng):
    """krylov_ref.spd_fill's values with the sign of the diagonal flipped on odd rows: symmetric, and by Gershgorin every
    eigenvalue has |lambda| >= 1, in both signs from n = 2 on; with |shift| <= 0.25 the shifted matrix keeps
    |lambda| >= 0.75.  Returns (values, b)."""
    n, rowptr, colind = pattern
    values, b = spd_fill(pattern, dtype, rng)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    flip = (rows == colind.astype(np.int64)) & (rows % 2 == 1)
    values[flip] = -values[flip]
    return values, b


def true_relative_residual(pattern, values, shift, x, b):
    """||b - (A - shift I) x|| / ||b|| in float64 on the host."""
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    x64, b64 = x.astype(np.float64), b.astype(np.float64)
    ax = np.bincount(rows, weights=values.astype(np.float64) * x64[colind.astype(np.int64)], minlength=n)
    return float(np.linalg.norm(b64 - (ax - float(shift) * x64)) / np.linalg.norm(b64))
