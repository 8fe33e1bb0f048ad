"""CPU restatement of restarted GMRES (include/spal.h): the sequential text, right-preconditioned, two
passes of classical Gram-Schmidt, Givens rotations, a column-form back substitution.  Every scalar has the vectors' dtype,
every product is rounded before the sum or difference it enters, every dot is tests/krylov_ref.dot.  `mul` and `prec` are
callables, as in krylov_ref, so the same text runs on pure host operations or on the device's own spmv /
solve_triangular; prec = None: M^-1 v is v itself.
"""
import numpy as np

from tests.krylov_ref import _result, _stop, dot


def _project(V, w, dt):
    """f[k] = dot(v_k, w) for every k from the SAME w, then w - f[0] v_0 - f[1] v_1 - ..., left to right."""
    f = [dot(v, w) for v in V]
    for fk, v in zip(f, V):
        w = w - fk * v
    return f, w


def gmres(mul, prec, b, x0, restart, tol, maxit):
    dt = b.dtype.type
    m = int(restart)
    assert m >= 1
    apply_m = (lambda v: v) if prec is None else prec
    with np.errstate(all="ignore"):
        x = x0.astype(b.dtype, copy=True)
        bb = dot(b, b)
        thr = dt(dt(tol * tol) * bb)
        it = 0
        while True:
            r = b - mul(x)
            rr = dot(r, r)
            reason = _stop(rr, thr, it, maxit)
            if reason is not None:
                return _result(x, it, reason, rr, bb)
            beta = np.sqrt(rr)
            V = [r / beta]
            g = np.zeros(m + 1, dtype=b.dtype)
            g[0] = beta
            H = np.zeros((m + 1, m), dtype=b.dtype)
            cs = np.zeros(m, dtype=b.dtype)
            sn = np.zeros(m, dtype=b.dtype)
            jj = 0
            while True:
                j = jj
                w = mul(apply_m(V[j]))
                h, w = _project(V, w, dt)
                c, w = _project(V, w, dt)
                h = [dt(hk + ck) for hk, ck in zip(h, c)]
                hn = np.sqrt(dot(w, w))
                V.append(w / hn)
                it += 1
                h.append(hn)
                for k in range(j):
                    t = dt(dt(cs[k] * h[k]) + dt(sn[k] * h[k + 1]))
                    h[k + 1] = dt(dt(cs[k] * h[k + 1]) - dt(sn[k] * h[k]))
                    h[k] = t
                d = np.sqrt(dt(dt(h[j] * h[j]) + dt(hn * hn)))
                cs[j] = dt(h[j] / d)
                sn[j] = dt(hn / d)
                h[j] = d
                g[j + 1] = -dt(sn[j] * g[j])
                g[j] = dt(cs[j] * g[j])
                H[:j + 1, j] = h[:j + 1]
                est = dt(g[j + 1] * g[j + 1])
                jj = j + 1
                if not np.isfinite(est):
                    return _result(x, it, 2, est, bb)        # x is what it was at the start of this cycle
                if est <= thr or it == maxit or jj == m:
                    break
            y = np.zeros(jj, dtype=b.dtype)
            for k in range(jj - 1, -1, -1):                  # column form
                y[k] = dt(g[k] / H[k, k])
                g[:k] = g[:k] - H[:k, k] * y[k]
            u = y[0] * V[0]
            for k in range(1, jj):
                u = u + y[k] * V[k]
            x = x + apply_m(u)


def cyclic_shift(n, dtype):
    """(mul, b, exact x) of the n x n cyclic shift (A e_i = e_{i+1 mod n}) with b = e0: BiCGStab breaks down on it after
    one iteration, GMRES needs exactly n steps."""
    b = np.zeros(n, dtype=dtype)
    b[0] = 1
    x = np.zeros(n, dtype=dtype)
    x[n - 1] = 1
    return (lambda v: np.roll(v, 1)), b, x
