"""CPU restatement of eigsh (include/spal.h): thick-restart Lanczos with full orthogonalisation, the
sequential text.  The vectors and a step's scalars have the vectors' dtype, every product is rounded before the sum or
difference it enters, every dot is tests/krylov_ref.dot, the Gram-Schmidt pass is tests/gmres_ref._project (restated here
on one 2-D array, the same tree per row and so the same bits: tests/test_eigsh_host.py compares the two); the projected
problem is solved in float64 by `jacobi`, the cyclic Jacobi of the text (only + - * / sqrt on doubles, so numpy gives the
library's bits).  `mul` is a callable, as in krylov_ref, so the same text runs on pure host operations or on the device's
own spmv.
"""
import numpy as np

from tests.colour_ref import mix32
from tests.krylov_ref import TILE, dot, reduce

LA, SA = 0, 1
WHICH = {"LA": LA, "SA": SA}
JACOBI_SWEEPS = 64


def dots(V, w):
    """[dot(v, w) for v in V]: krylov_ref.reduce's tree applied to every row of one 2-D array"""
    P = np.stack(V) * w
    k, n = P.shape
    c = max(1, -(-n // TILE))
    e = np.zeros((k, TILE * c), dtype=P.dtype)      # +0.0, and it is added
    e[:, :n] = P
    e = e.reshape(k, c, TILE)
    h = TILE // 2
    while h >= 1:
        e = e[..., :h] + e[..., h:2 * h]
        h //= 2
    sums = np.ascontiguousarray(e[..., 0])
    return [row[0] if c == 1 else reduce(row) for row in sums]


def _project(V, w, dt):
    """f[k] = dot(v_k, w) for every k from the SAME w, then w - f[0] v_0 - f[1] v_1 - ..., left to right."""
    f = dots(V, w)
    for fk, v in zip(f, V):
        w = w - fk * v
    return f, w


def jacobi(S):
    """(theta, Y, sweeps) of a symmetric float64 matrix: theta[i] = S[i, i] after the rotations, its vector Y[:, i].  Not
    ordered."""
    S = np.array(S, dtype=np.float64)
    m = S.shape[0]
    Y = np.eye(m, dtype=np.float64)
    sweep = 0
    with np.errstate(all="ignore"):
        while sweep < JACOBI_SWEEPS:
            rotated = False
            for p in range(m - 1):
                for q in range(p + 1, m):
                    a = S[p, q]
                    if a == 0.0:
                        continue
                    app, aqq, g = S[p, p], S[q, q], abs(a)
                    if abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
                        S[p, q] = S[q, p] = 0.0
                        continue
                    rotated = True
                    th = (0.5 * (aqq - app)) / a
                    t = 1.0 / (abs(th) + np.sqrt((th * th) + 1.0))
                    if th < 0.0:
                        t = -t
                    c = 1.0 / np.sqrt((t * t) + 1.0)
                    s = t * c
                    x, y = S[:, p].copy(), S[:, q].copy()
                    xp = (c * x) - (s * y)
                    xq = (s * x) + (c * y)
                    S[:, p] = S[p, :] = xp
                    S[:, q] = S[q, :] = xq
                    S[p, p] = app - (t * a)
                    S[q, q] = aqq + (t * a)
                    S[p, q] = S[q, p] = 0.0
                    x, y = Y[:, p].copy(), Y[:, q].copy()
                    Y[:, p] = (c * x) - (s * y)
                    Y[:, q] = (s * x) + (c * y)
            if not rotated:
                break
            sweep += 1
    return np.diag(S).copy(), Y, sweep


def ritz(S, hn, which, jacobi_fn=None):
    """(theta, Y, res) ordered, or None when S holds a value that is not finite."""
    if not np.all(np.isfinite(S)):
        return None
    theta, Y, _ = (jacobi_fn or jacobi)(S)
    order = np.argsort(-theta if which == LA else theta, kind="stable")
    theta, Y = theta[order], Y[:, order]
    with np.errstate(all="ignore"):
        res = np.abs(np.float64(hn) * Y[-1, :])
    return theta, Y, res


def default_start(n, seed, dtype):
    i = (np.arange(n, dtype=np.uint64) + np.uint64(seed & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    return ((mix32(i) >> np.uint64(8)) + np.uint64(1)).astype(dtype) / dtype(2 ** 24)


def rotate(V, Y, nc, dtype):
    """column c: (..((Y[0,c] * v_0) + (Y[1,c] * v_1)) ..) + (Y[jj-1,c] * v_{jj-1}), Y rounded to the dtype first"""
    Yt = Y.astype(dtype)
    out = []
    with np.errstate(all="ignore"):
        for c in range(nc):
            u = Yt[0, c] * V[0]
            for t in range(1, Y.shape[0]):
                u = u + Yt[t, c] * V[t]
            out.append(u)
    return out


def keep_of(k, ncv):
    return min(k + (ncv - k) // 2, ncv - 1)


def eigsh(mul, n, dtype, k, which, ncv, tol, maxit, v0=None, seed=0, jacobi_fn=None):
    """dict(theta, resid, X, restarts, products, converged, reason, pairs): theta, resid and the columns of X (n x pairs)
    hold the `pairs` = min(k, jj) values the text writes; reason 2 writes none.  jacobi_fn: another implementation of
    `jacobi` with the same bits (the library's spal_eigsh_jacobi, where numpy's loop would take too long)."""
    dt = np.dtype(dtype).type
    which = WHICH.get(which, which)
    m = int(ncv)
    assert 0 < k < m <= n
    with np.errstate(all="ignore"):
        v0 = default_start(n, seed, dt) if v0 is None else np.asarray(v0, dtype=dt)
        V = [v0 / np.sqrt(dot(v0, v0))]
        S = np.zeros((m, m), dtype=np.float64)
        keep = restarts = products = 0

        def result(reason, conv=0, theta=None, Y=None, res=None, jj=0):
            nk = 0 if reason == 2 else min(k, jj)
            X = np.stack(rotate(V[:jj], Y, nk, dt), axis=1) if nk else np.zeros((n, 0), dtype=dt)
            return dict(theta=np.zeros(0, dt) if not nk else theta[:nk].astype(dt), resid=np.zeros(0, dt) if not nk else res[:nk].astype(dt),
                        X=X, restarts=restarts, products=products, converged=0 if reason == 2 else conv, reason=reason, pairs=nk)

        while True:
            exhausted = False
            jj = keep
            for j in range(keep, m):
                w = mul(V[j])
                h, w = _project(V[:j + 1], w, dt)
                c, w = _project(V[:j + 1], w, dt)
                h = [dt(hk + ck) for hk, ck in zip(h, c)]
                hn = np.sqrt(dot(w, w))
                V.append(w / hn)
                products += 1
                S[:j + 1, j] = S[j, :j + 1] = np.array(h, dtype=np.float64)
                jj = j + 1
                if not np.isfinite(hn):
                    return result(2)
                if hn == 0:
                    exhausted = True
                    break
            r = ritz(S[:jj, :jj], hn, which, jacobi_fn)
            if r is None:
                return result(2)
            theta, Y, res = r
            nk = min(k, jj)
            scale = np.max(np.abs(theta))
            conv = 0
            while conv < nk and res[conv] <= tol * scale:
                conv += 1
            if exhausted:
                return result(0 if jj >= k else 3, conv, theta, Y, res, jj)
            if conv == k:
                return result(0, conv, theta, Y, res, jj)
            if restarts == maxit:
                return result(1, conv, theta, Y, res, jj)
            keep = keep_of(k, m)
            V = rotate(V[:m], Y, keep, dt) + [V[m]]
            S = np.zeros((m, m), dtype=np.float64)
            S[np.arange(keep), np.arange(keep)] = theta[:keep]
            restarts += 1


# ---- the matrices of the tests -----------------------------------------------------------------------------------------

def laplace_1d_plus(n=200):
    """A1: the 1-D Laplacian plus diag(linspace(0, 3, n)^2), dense float64"""
    a = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    return a + np.diag(np.linspace(0.0, 3.0, n) ** 2)


def laplace_2d(g=13):
    """the g x g five-point Laplacian, dense float64"""
    t = 2.0 * np.eye(g) - np.eye(g, k=1) - np.eye(g, k=-1)
    return np.kron(np.eye(g), t) + np.kron(t, np.eye(g))


def laplace_2d_plus(g=13):
    """A2: the g x g five-point Laplacian plus diag(arange(g^2) / g^2)"""
    n = g * g
    return laplace_2d(g) + np.diag(np.arange(n) / n)


def dense_to_csr(a, dtype):
    n = a.shape[0]
    rows, cols = np.nonzero(a)
    rowptr = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return n, rowptr, cols.astype(np.uint64), a[rows, cols].astype(dtype)
