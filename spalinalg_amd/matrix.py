"""Host-side mirror of the reference's matrix types over the C ABI.

Names, argument meaning and error behaviour follow the reference
(lokyhark/spalinalg; paths relative to its root):

* ``CsrMatrix(nrows, ncols, rowptr, colind, values)``  == ``CsrMatrix::new``
  (src/csr.rs:137-164) incl. its panics (-> :class:`Panic`),
  ``nrows()/ncols()/rowptr()/colind()/values()/nnz()`` (src/csr.rs:200-289).
* ``a * x`` / ``a @ x`` with a dense vector: the product the reference only
  reaches through ``&a * &x_as_matrix`` (src/csr/ops/mul.rs:5-59); what a Rust
  binding adds as ``impl Mul<&[T]> for &CsrMatrix<T>``.
* ``a * b`` / ``a @ b`` with a matrix of the same format: the reference's own
  ``impl Mul for &CsrMatrix<T>`` / ``&CscMatrix<T>``, on the device, bit-identical.
* ``a + b``, ``a - b`` and ``-a``: ``impl Add / Sub / Neg`` of the same types
  (src/csr/ops/{add,sub,neg}.rs, src/csc/ops/...), on the device, bit-identical.
* ``CsrMatrix.from_coo(coo)`` == ``CsrMatrix::from(&coo)``
  (src/csr/conv/coo.rs:3-116), assembled on the device.
* ``CscMatrix`` / ``CooMatrix`` likewise (src/csc.rs, src/coo.rs).

Host arrays stay numpy (``uint64`` indices like ``usize``, ``float64`` /
``float32`` values like the two ``Scalar`` impls); a device copy is created
on first use and owned by the :class:`DeviceCsr` / :class:`DeviceCsc` handle.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

from . import _ffi
from ._ffi import Panic, check, f32p, f64p, u64, u64p, vp


def _scalar_dtype(values) -> np.dtype:
    dt = np.asarray(values).dtype
    if dt == np.float32:
        return np.dtype(np.float32)
    if dt == np.float64 or dt.kind in "iub":
        return np.dtype(np.float64)
    raise TypeError("Scalar is implemented for f32 and f64 only (src/scalar.rs:56-57)")


def _sfx(dt: np.dtype) -> str:
    return "f64" if dt == np.float64 else "f32"


def _idx(a) -> np.ndarray:
    arr = np.asarray(a)
    if arr.size and arr.dtype.kind not in "iu":
        raise TypeError("indices must be integers (usize)")
    if arr.size and arr.dtype.kind == "i" and (arr < 0).any():
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "negative index (usize cannot be negative)")
    return np.ascontiguousarray(arr, dtype=np.uint64)


def _p(a: np.ndarray):
    return a.ctypes.data_as({np.dtype(np.uint64): u64p, np.dtype(np.float64): f64p,
                             np.dtype(np.float32): f32p}[a.dtype])


def _stream_ptr(stream) -> vp:
    if stream is None:
        return vp(0)
    if isinstance(stream, int):
        return vp(stream)
    return vp(int(stream.cuda_stream))  # torch.cuda.Stream


# --------------------------------------------------------------------------
# the dot product and the Krylov solvers' result (include/spal.h)
# --------------------------------------------------------------------------
class _KrylovInfoC(C.Structure):
    """spal_krylov_info"""
    _fields_ = [("iterations", C.c_uint64), ("reason", C.c_int), ("residual_sq", C.c_double),
                ("rhs_sq", C.c_double), ("solve_ms", C.c_double)]


class KrylovInfo(dict):
    """What a solve reports: iterations, reason (0 converged, 1 maxit, 2 breakdown / not finite), residual_sq = the
    recurrence's dot(r, r) and rhs_sq = dot(b, b) (exact conversions of the element type's values), solve_ms."""
    __getattr__ = dict.__getitem__


_KRYLOV_METHODS = {"cg": 0, "bicgstab": 1}


def _krylov_method(method) -> int:
    if isinstance(method, str):
        if method.lower() not in _KRYLOV_METHODS:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"method {method!r} must be 'cg' or 'bicgstab'")
        return _KRYLOV_METHODS[method.lower()]
    return int(method)


def _eigsh_info(c, resid) -> "EigshInfo":
    return EigshInfo(restarts=int(c.restarts), products=int(c.products), converged=int(c.converged), reason=int(c.reason),
                     resid=np.array(resid, copy=True), solve_ms=float(c.solve_ms))


def _krylov_info(c: _KrylovInfoC) -> KrylovInfo:
    return KrylovInfo(iterations=int(c.iterations), reason=int(c.reason), residual_sq=float(c.residual_sq),
                      rhs_sq=float(c.rhs_sq), solve_ms=float(c.solve_ms))


class _EigshInfoC(C.Structure):
    """spal_eigsh_info"""
    _fields_ = [("restarts", C.c_uint64), ("products", C.c_uint64), ("converged", C.c_uint64), ("reason", C.c_int),
                ("solve_ms", C.c_double)]


class EigshInfo(dict):
    """What eigsh() reports: restarts, products (with A), converged (leading pairs whose estimate met tol), reason (0
    converged or the space exhausted with at least k pairs, 1 maxit restarts, 2 not finite, 3 exhausted with fewer than
    k pairs), resid (the estimates |hn * Y[m-1, i]| of the pairs returned), solve_ms."""
    __getattr__ = dict.__getitem__


class _EigshFilterInfoC(C.Structure):
    """spal_eigsh_filter_info"""
    _fields_ = [("restarts", C.c_uint64), ("products", C.c_uint64), ("converged", C.c_uint64), ("reason", C.c_int),
                ("solve_ms", C.c_double), ("warm_restarts", C.c_uint64), ("warm_products", C.c_uint64), ("lo", C.c_double),
                ("hi", C.c_double), ("a0", C.c_double), ("degree", C.c_uint64)]


def _eigsh_filter_info(c, resid) -> "EigshInfo":
    out = _eigsh_info(c, resid)
    out.update(warm_restarts=int(c.warm_restarts), warm_products=int(c.warm_products), lo=float(c.lo), hi=float(c.hi),
               a0=float(c.a0), degree=int(c.degree))
    return out


def _filter_args(filter_degree, filter_interval, filter_warmup):
    """(degree, automatic, lo, hi, warmup) of a filtered eigsh call, refused as the library does"""
    degree = int(filter_degree)
    if not 1 <= degree <= 256:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: filter_degree = {degree} must be 0 (no filter) or 1 .. 256")
    warmup = int(filter_warmup)
    if warmup < 0:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: filter_warmup = {warmup} must be >= 0")
    if filter_interval is None:
        return degree, 1, 0.0, 0.0, warmup
    lo, hi = (float(v) for v in filter_interval)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: filter_interval = [{lo}, {hi}] must be finite with lo < hi")
    return degree, 0, lo, hi, warmup


class _EigshNearInfoC(C.Structure):
    """spal_eigsh_near_info"""
    _fields_ = [("restarts", C.c_uint64), ("products", C.c_uint64), ("converged", C.c_uint64), ("reason", C.c_int),
                ("solve_ms", C.c_double), ("lo", C.c_double), ("hi", C.c_double), ("sigma", C.c_double), ("gamma", C.c_double),
                ("degree", C.c_uint64)]


def _eigsh_near_info(c, resid) -> "EigshInfo":
    out = _eigsh_info(c, resid)
    out.update(lo=float(c.lo), hi=float(c.hi), sigma=float(c.sigma), gamma=float(c.gamma), degree=int(c.degree))
    return out


def _near_args(sigma, which, filter_degree, filter_interval):
    """(sigma, degree, automatic, lo, hi) of an eigsh(sigma=...) call.  What scipy would answer with shift-invert is a
    ValueError here; the rest is refused as the library does."""
    if _eigsh_which(which) != 0 or int(filter_degree) < 2:
        raise ValueError("eigsh: sigma is served by a Chebyshev delta filter, there is no shift-invert: it needs "
                         "filter_degree >= 2 (the degree sets the resolution) and takes no which='SA'")
    sigma, degree = float(sigma), int(filter_degree)
    if degree > 4096:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: filter_degree = {degree} must be 2 .. 4096 with sigma")
    if not np.isfinite(sigma):
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: sigma = {sigma} must be finite")
    if filter_interval is None:
        return sigma, degree, 1, 0.0, 0.0
    lo, hi = (float(v) for v in filter_interval)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: filter_interval = [{lo}, {hi}] must be finite with lo < hi")
    if not lo < sigma < hi:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: sigma = {sigma} must lie strictly inside filter_interval = [{lo}, {hi}]")
    return sigma, degree, 0, lo, hi


def _series_args(coef, lo, hi):
    """(coef as contiguous doubles, degree, lo, hi) of a cheb_series call, refused as the library does"""
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    lo, hi = float(lo), float(hi)
    if coef.ndim != 1 or not 2 <= coef.size <= 4097:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"cheb_series: coef has shape {coef.shape}: degree + 1 values, degree 1 .. 4096")
    if not (np.isfinite(lo) and np.isfinite(hi)) or not np.all(np.isfinite(coef)):
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "cheb_series: lo, hi and every coefficient must be finite")
    if not lo < hi:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"cheb_series: lo = {lo} must be less than hi = {hi}")
    return coef, coef.size - 1, lo, hi


def cheb_delta_coefficients(degree: int, gamma: float) -> np.ndarray:
    """The degree + 1 Chebyshev coefficients of the Fejer-damped delta function at gamma in (-1, 1), scaled so that the
    series is 1 at gamma (spal_cheb_delta_coefficients): host only, only + - * / on doubles.  With
    gamma = (sigma - (lo+hi)/2) / ((hi-lo)/2) they are the filter of eigsh(sigma=...); pass them to cheb_series()."""
    degree = int(degree)
    coef = np.empty(max(degree, 0) + 1, dtype=np.float64)
    check(_ffi.lib().spal_cheb_delta_coefficients(u64(max(degree, 0)), C.c_double(gamma), _p(coef), u64(coef.size)))
    return coef


# --------------------------------------------------------------------------
# KPM moments, the spectral density and eigenvalue counts (include/spal.h)
# --------------------------------------------------------------------------
class _KpmInfoC(C.Structure):
    """spal_kpm_info"""
    _fields_ = [("products", C.c_uint64), ("lo", C.c_double), ("hi", C.c_double), ("glo", C.c_double), ("ghi", C.c_double),
                ("degree", C.c_uint64), ("probes", C.c_uint64), ("solve_ms", C.c_double)]


class KpmInfo(dict):
    """What a kpm_moments call reports: products (per column), lo, hi, glo, ghi (0, 0 with a given interval), degree,
    probes, solve_ms."""
    __getattr__ = dict.__getitem__


def _kpm_info(c: _KpmInfoC) -> KpmInfo:
    return KpmInfo(products=int(c.products), lo=float(c.lo), hi=float(c.hi), glo=float(c.glo), ghi=float(c.ghi),
                   degree=int(c.degree), probes=int(c.probes), solve_ms=float(c.solve_ms))


def _mix32(x: np.ndarray) -> np.ndarray:
    """mix32 of include/spal.h on an array of uint32 words"""
    x = x.astype(np.uint32, copy=True)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def kpm_probes(n: int, k: int, seed: int = 0, dtype=np.float64) -> np.ndarray:
    """The hashed Rademacher probes of kpm_moments, an (n, k) block of +-1 (include/spal.h): on the host, exact.
    z[i, j] = -1 where the top bit of mix32(mix32(i + seed) + j) is set; only seed mod 2^32 enters."""
    n, k = int(n), int(k)
    with np.errstate(over="ignore"):
        h = _mix32((np.arange(n, dtype=np.uint64) + np.uint64(int(seed) % 2**32)).astype(np.uint32))
        w = _mix32(h[:, None] + np.arange(k, dtype=np.uint32)[None, :])
    return np.where(w >> np.uint32(31), -1.0, 1.0).astype(np.dtype(dtype))


def _kpm_args(what, degree, k, interval):
    """(degree, k, automatic, lo, hi) of a kpm_moments call, refused as the library does"""
    degree, k = int(degree), int(k)
    if not 1 <= degree <= 4096:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"{what}: degree = {degree} must be 1 .. 4096")
    if not 1 <= k <= 256:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"{what}: probes = {k} must be 1 .. 256")
    if interval is None:
        return degree, k, 1, 0.0, 0.0
    lo, hi = (float(v) for v in interval)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"{what}: interval = [{lo}, {hi}] must be finite with lo < hi")
    return degree, k, 0, lo, hi


def kpm_damping(degree: int, kind: str = "jackson") -> np.ndarray:
    """g[0 .. degree], the damping factors of a truncated Chebyshev series: "jackson" (the usual choice: a nonnegative
    kernel of width ~ pi/degree) or "fejer" (g_i = (d+1-i)/(d+1)), or "none".  Host doubles with cos: not bit-pinned."""
    d = int(degree)
    i = np.arange(d + 1, dtype=np.float64)
    if kind == "jackson":
        q = np.pi / (d + 2)
        return ((d + 2 - i) * np.cos(i * q) + np.sin(i * q) / np.tan(q)) / (d + 2)
    if kind == "fejer":
        return (d + 1 - i) / (d + 1)
    if kind in (None, "none"):
        return np.ones(d + 1)
    raise ValueError(f"kpm_damping: kind = {kind!r} must be 'jackson', 'fejer' or 'none'")


def _kpm_damped(mu, damping):
    mu = np.asarray(mu, dtype=np.float64)
    if mu.ndim == 1:
        mu = mu[:, None]
    if mu.ndim != 2 or mu.shape[0] < 2:
        raise ValueError(f"mu has shape {mu.shape}: (degree + 1, probes) moments, degree >= 1")
    g = kpm_damping(mu.shape[0] - 1, damping) if isinstance(damping, str) or damping is None else np.asarray(damping, float)
    return mu * g[:, None]


def kpm_density(mu, lo: float, hi: float, points, damping="jackson") -> np.ndarray:
    """The spectral density at `points` from the moments of kpm_moments on [lo, hi], averaged over the probes and
    normalised to integrate to n (mu[0] is n for +-1 probes):
        rho(x) = (g_0 mu_0 + 2 sum_i g_i mu_i T_i(t)) / (pi e sqrt(1 - t^2)),   t = (x - c)/e.
    Points outside (lo, hi) give 0.  Host double arithmetic: not bit-pinned."""
    m = _kpm_damped(mu, damping).mean(axis=1)
    c, e = (lo + hi) / 2.0, (hi - lo) / 2.0
    t = (np.asarray(points, dtype=np.float64) - c) / e
    inside = np.abs(t) < 1.0
    th = np.arccos(np.where(inside, t, 0.0))
    i = np.arange(m.size, dtype=np.float64)
    w = m * np.where(i == 0, 1.0, 2.0)
    series = np.cos(th[..., None] * i) @ w
    return np.where(inside, series / (np.pi * e * np.sin(th)), 0.0)


def kpm_count(mu, lo: float, hi: float, a: float, b: float, damping="jackson"):
    """(estimate, standard_error) of the number of eigenvalues in [a, b] from the moments of kpm_moments on [lo, hi]:
    the damped series integrated in closed form,
        count = (g_0 mu_0 (th_a - th_b) + 2 sum_i g_i mu_i (sin(i th_a) - sin(i th_b))/i) / pi,   th = arccos((x - c)/e),
    a and b clipped to [lo, hi].  The estimate is the probes' mean; the standard error is the spread of the per-probe
    estimates over sqrt(probes) (0 for one probe).  Host double arithmetic: not bit-pinned."""
    m = _kpm_damped(mu, damping)
    c, e = (lo + hi) / 2.0, (hi - lo) / 2.0
    ta, tb = (float(np.clip((v - c) / e, -1.0, 1.0)) for v in (a, b))
    tha, thb = np.arccos(ta), np.arccos(tb)
    i = np.arange(1, m.shape[0], dtype=np.float64)
    w = np.concatenate([[tha - thb], 2.0 * (np.sin(i * tha) - np.sin(i * thb)) / i]) / np.pi
    per_probe = w @ m
    k = per_probe.size
    err = float(per_probe.std(ddof=1) / np.sqrt(k)) if k > 1 else 0.0
    return float(per_probe.mean()), err


_EIGSH_WHICH = {"LA": 0, "SA": 1}


def _eigsh_which(which) -> int:
    if isinstance(which, str):
        if which.upper() not in _EIGSH_WHICH:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: which = {which!r} must be 'LA' or 'SA'")
        return _EIGSH_WHICH[which.upper()]
    return int(which)


def _eigsh_args(n: int, ncols: int, k, ncv, tol, dtype):
    """(k, ncv, tol) resolved and refused as the library does, before anything touches a device."""
    k = int(k)
    if n != ncols:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: the matrix is not square ({n} x {ncols})")
    ncv = min(n, max(2 * k + 1, 20)) if ncv is None else int(ncv)
    if k < 1:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "eigsh: k = 0 (at least one eigenpair)")
    if ncv <= k:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: ncv = {ncv} must be greater than k = {k} (a matrix of {n} rows)")
    if ncv > 256 or ncv > n:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: ncv = {ncv} must be at most 256 and at most the matrix's {n} rows")
    tol = float(tol)
    if not (tol >= 0.0) or not np.isfinite(tol):
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: tol = {tol} must be finite and >= 0")
    return k, ncv, tol if tol > 0.0 else float(np.finfo(dtype).eps)


def dot(a, b):
    """dot(a, b) by the library's definition (include/spal.h): products rounded, then the fixed tree over tiles of
    1024 -- on the host, no device needed (spal_dot_*).  A numpy scalar of the vectors' dtype (float32 / float64)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.dtype not in (np.float32, np.float64) or a.ndim != 1 or a.shape != b.shape:
        raise TypeError("dot() takes two 1-D vectors of one length and dtype, float32 or float64")
    out = np.empty(1, dtype=a.dtype)
    check(getattr(_ffi.lib(), f"spal_dot_{_sfx(a.dtype)}")(_p(a), _p(b), u64(a.size), _p(out)))
    return out[0]


def dot_dev(dtype, a_ptr: int, b_ptr: int, n: int, out_ptr: int, device: int = 0, stream=None) -> None:
    """The same dot for device vectors (spal_dot_dev_*): the one result is written to out_ptr; enqueued on `stream`,
    not synchronised."""
    check(getattr(_ffi.lib(), f"spal_dot_dev_{_sfx(np.dtype(dtype))}")(C.c_int(device), vp(a_ptr), vp(b_ptr), u64(n),
                                                                     vp(out_ptr), _stream_ptr(stream)))


# --------------------------------------------------------------------------
# aggregation AMG (include/spal.h)
# --------------------------------------------------------------------------
class _AmgParamsC(C.Structure):
    """spal_amg_params"""
    _fields_ = [("seed", C.c_uint64), ("max_levels", C.c_uint64), ("coarse_rows", C.c_uint64), ("nu", C.c_uint64),
                ("coarse_sweeps", C.c_uint64), ("gamma", C.c_uint64), ("omega", C.c_double), ("alpha", C.c_double)]


def _amg_params(seed, max_levels, coarse_rows, nu, coarse_sweeps, cycle, omega, alpha) -> _AmgParamsC:
    if not isinstance(cycle, str) or cycle.lower() not in ("v", "w"):
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"amg: cycle {cycle!r} must be 'v' or 'w'")
    for name, v in (("seed", seed), ("max_levels", max_levels), ("coarse_rows", coarse_rows), ("nu", nu),
                    ("coarse_sweeps", coarse_sweeps)):
        if int(v) < 0:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"amg: {name} = {int(v)} is negative")
    return _AmgParamsC(int(seed), int(max_levels), int(coarse_rows), int(nu), int(coarse_sweeps),
                       1 if cycle.lower() == "v" else 2, float(omega), float(alpha))


def amg_aggregate(rowptr, colind, seed: int = 0):
    """(agg, nagg): the aggregation text of include/spal.h on the pattern (rowptr, colind) of a square matrix, on the
    host (spal_amg_aggregate): no device needed."""
    rowptr, colind = _idx(rowptr), _idx(colind)
    if rowptr.size < 1:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "amg_aggregate: rowptr is empty")
    n = rowptr.size - 1
    agg = np.empty(n, dtype=np.uint64)
    nagg = u64()
    check(_ffi.lib().spal_amg_aggregate(u64(n), _p(rowptr), _p(colind), u64(seed), _p(agg), C.byref(nagg)))
    return agg, nagg.value


class Amg:
    """An aggregation multigrid hierarchy on the device (spal_*_amg_setup): apply(b) is one cycle, bit for bit the text
    of include/spal.h; `a.solve(b, M=g)` preconditions CG / BiCGStab with it.  It holds its own copy of the matrix and
    outlives the matrix it was built from."""

    def __init__(self, handle, dtype, device: int, nrows: int):
        self._h = handle
        self.dtype = np.dtype(dtype)
        self.device = device
        self._nrows = int(nrows)

    def close(self):
        if self._h is not None:
            _ffi.lib().spal_amg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def nrows(self) -> int:
        return self._nrows

    def describe(self) -> dict:
        buf = C.create_string_buffer(16384)
        check(_ffi.lib().spal_amg_describe(self._h, buf, C.c_size_t(len(buf))))
        return json.loads(buf.value.decode())

    def set_option(self, key: str, value: int) -> None:
        check(_ffi.lib().spal_amg_set_option(self._h, key.encode(), C.c_int64(value)))

    def apply(self, b) -> np.ndarray:
        """x = cycle(0, b) for a host vector of the hierarchy's dtype."""
        b = np.ascontiguousarray(b)
        if b.dtype not in (np.float32, np.float64):
            b = b.astype(self.dtype)
        if b.ndim != 1:
            raise TypeError("apply() takes one 1-D vector")
        x = np.empty_like(b)
        check(getattr(_ffi.lib(), f"spal_amg_apply_{_sfx(b.dtype)}")(self._h, _p(b), u64(b.size), _p(x), u64(x.size)))
        return x

    def apply_dev(self, b_ptr: int, x_ptr: int, stream=None, dtype=None) -> None:
        """Device pointers (x != b): enqueued on `stream`, not synchronised."""
        dt = self.dtype if dtype is None else np.dtype(dtype)
        check(getattr(_ffi.lib(), f"spal_amg_apply_dev_{_sfx(dt)}")(self._h, vp(b_ptr), vp(x_ptr), _stream_ptr(stream)))

    def level(self, l: int) -> "CsrMatrix":
        """A_l as a CsrMatrix (an independent copy, downloaded; it keeps its device handle)."""
        out = vp()
        check(_ffi.lib().spal_amg_level_csr(self._h, u64(l), C.byref(out)))
        dev = DeviceCsr(out, self.dtype, self.device)
        n = dev.shape()[0]
        ptr, ind, val = dev.download()
        m = CsrMatrix._trusted(n, n, ptr, ind, val)
        m._dev[self.device] = dev
        return m

    def aggregates(self, l: int) -> np.ndarray:
        """agg[] of level l, which must have a coarser level."""
        rows = self.describe()["rows"]
        if not 0 <= int(l) < len(rows):
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"aggregates: level = {l} but the hierarchy has {len(rows)}")
        agg = np.empty(rows[int(l)], dtype=np.uint64)
        check(_ffi.lib().spal_amg_aggregates(self._h, u64(l), _p(agg), u64(agg.size)))
        return agg


# --------------------------------------------------------------------------
# FSAI (include/spal.h)
# --------------------------------------------------------------------------
def fsai_row(B_lower, dtype=None):
    """(g, rejected): the text's Cholesky and back-substitution of include/spal.h on ONE local system, on the host
    (spal_fsai_row_*): no device needed.  `B_lower` is the lower triangle of B packed by rows (m (m + 1) / 2 values) or
    a square 2-D array, whose lower triangle is taken."""
    b = np.asarray(B_lower)
    dt = np.dtype(dtype) if dtype is not None else (b.dtype if b.dtype in (np.float32, np.float64) else np.dtype(np.float64))
    if b.ndim == 2:
        if b.shape[0] != b.shape[1]:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"fsai_row: B has shape {b.shape}")
        b = b[np.tril_indices(b.shape[0])]
    b = np.ascontiguousarray(b, dtype=dt)
    m = int((np.sqrt(8.0 * b.size + 1.0) - 1.0) / 2.0 + 0.5)
    if b.ndim != 1 or m * (m + 1) // 2 != b.size:
        raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"fsai_row: {b.size} values are no packed lower triangle")
    g = np.empty(m, dtype=dt)
    rejected = C.c_int(0)
    check(getattr(_ffi.lib(), f"spal_fsai_row_{_sfx(dt)}")(u64(m), _p(b), _p(g), C.byref(rejected)))
    return g, rejected.value


class Fsai:
    """A factorised sparse approximate inverse on the device (spal_*_fsai_setup): G ~ L^-1 on a prescribed pattern, bit
    for bit the text of include/spal.h; apply(b) = Gt (G b), two SpMVs on planned handles; `a.solve(b, M=f)` and
    `a.minres(b, M=f)` precondition CG / BiCGStab / MINRES with it.  It holds its own matrices and outlives the matrix
    it was built from."""

    def __init__(self, handle, dtype, device: int, nrows: int):
        self._h = handle
        self.dtype = np.dtype(dtype)
        self.device = device
        self._nrows = int(nrows)
        self._factors = {}

    def close(self):
        if self._h is not None:
            _ffi.lib().spal_fsai_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def nrows(self) -> int:
        return self._nrows

    def describe(self) -> dict:
        buf = C.create_string_buffer(4096)
        check(_ffi.lib().spal_fsai_describe(self._h, buf, C.c_size_t(len(buf))))
        return json.loads(buf.value.decode())

    @property
    def rejected(self) -> int:
        return int(self.describe()["rejected"])

    def _factor(self, transposed: int) -> "CsrMatrix":
        if transposed not in self._factors:
            out = vp()
            check(_ffi.lib().spal_fsai_factor_csr(self._h, C.c_int(transposed), C.byref(out)))
            dev = DeviceCsr(out, self.dtype, self.device)
            n = dev.shape()[0]
            ptr, ind, val = dev.download()
            m = CsrMatrix._trusted(n, n, ptr, ind, val)
            m._dev[self.device] = dev
            self._factors[transposed] = m
        return self._factors[transposed]

    @property
    def G(self) -> "CsrMatrix":
        """G as a CsrMatrix (an independent copy, downloaded; it keeps its device handle)."""
        return self._factor(0)

    @property
    def Gt(self) -> "CsrMatrix":
        """The transpose of G, likewise."""
        return self._factor(1)

    def apply(self, b) -> np.ndarray:
        """x = Gt (G b) for a host vector of the factor's dtype."""
        b = np.ascontiguousarray(b)
        if b.dtype not in (np.float32, np.float64):
            b = b.astype(self.dtype)
        if b.ndim != 1:
            raise TypeError("apply() takes one 1-D vector")
        x = np.empty_like(b)
        check(getattr(_ffi.lib(), f"spal_fsai_apply_{_sfx(b.dtype)}")(self._h, _p(b), u64(b.size), _p(x), u64(x.size)))
        return x

    def apply_dev(self, b_ptr: int, x_ptr: int, stream=None, dtype=None) -> None:
        """Device pointers (x != b): two products enqueued on `stream`, not synchronised."""
        dt = self.dtype if dtype is None else np.dtype(dtype)
        check(getattr(_ffi.lib(), f"spal_fsai_apply_dev_{_sfx(dt)}")(self._h, vp(b_ptr), vp(x_ptr), _stream_ptr(stream)))


def _refuse_amg(M, what: str) -> None:
    if isinstance(M, Amg):
        raise TypeError(f"{what} takes an ILU(0) factor as M, not an Amg: an AMG hierarchy preconditions solve() "
                        "(method 'cg' or 'bicgstab') only")
    if isinstance(M, Fsai) and what != "minres()":   # (solve() dispatches on an Fsai before it asks here)
        raise TypeError(f"{what} takes an ILU(0) factor as M, not an Fsai: an FSAI factor preconditions solve() "
                        "(method 'cg' or 'bicgstab') and minres() only")


# --------------------------------------------------------------------------
# device handles
# --------------------------------------------------------------------------
class _DeviceMatrix:
    _kind = ""  # "csr" | "csc"

    def __init__(self, handle, dtype: np.dtype, device: int):
        self._h = handle
        self.dtype = np.dtype(dtype)
        self.device = device

    def _fn(self, name):
        return getattr(_ffi.lib(), f"spal_{self._kind}_{name}")

    def close(self):
        if self._h is not None:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shape(self):
        nr, nc, nz, es = u64(), u64(), u64(), C.c_int()
        check(self._fn("shape")(self._h, C.byref(nr), C.byref(nc), C.byref(nz), C.byref(es)))
        return nr.value, nc.value, nz.value

    def set_option(self, key: str, value: int) -> None:
        check(self._fn("set_option")(self._h, key.encode(), C.c_int64(value)))
        if key == "fsai_max_row":
            self._fsai_max_row = int(value)   # (what fsai(max_row=...) restores)

    def describe(self) -> dict:
        buf = C.create_string_buffer(16384)
        check(self._fn("describe")(self._h, buf, C.c_size_t(len(buf))))
        return json.loads(buf.value.decode())

    def spmv(self, x) -> np.ndarray:
        """Host vectors in, host vector out (H2D x, kernel, D2H y)."""
        x = np.ascontiguousarray(x, dtype=self.dtype)
        nrows = self.shape()[0]
        y = np.empty(nrows, dtype=self.dtype)
        check(self._fn(f"spmv_{_sfx(self.dtype)}")(self._h, _p(x), u64(x.size), _p(y), u64(y.size)))
        return y

    def spmv_dev(self, x_ptr: int, y_ptr: int, stream=None) -> None:
        """Device pointers; enqueued on `stream`, not synchronised."""
        check(self._fn(f"spmv_dev_{_sfx(self.dtype)}")(self._h, vp(x_ptr), vp(y_ptr), _stream_ptr(stream)))

    def spmm(self, X) -> np.ndarray:
        """Y = A * X for a host 2-D array X of shape (ncols, k): host (nrows, k) array out (H2D, one pass over the
        matrix for all k columns, D2H).  Bit for bit the reference's `&A * &X` for a fully stored X, whatever k is.
        With one or two vectors spmv() is the faster call; from about four on this one is."""
        X = np.ascontiguousarray(X, dtype=self.dtype)
        if X.ndim != 2:
            raise TypeError("spmm() takes a 2-D block of vectors, shape (ncols, k)")
        nrows = self.shape()[0]
        k = X.shape[1]
        Y = np.empty((nrows, k), dtype=self.dtype)
        check(self._fn(f"spmm_{_sfx(self.dtype)}")(self._h, u64(k), _p(X), u64(k), u64(X.shape[0]),
                                                   _p(Y), u64(k), u64(nrows)))
        return Y

    def spmm_dev(self, k: int, x_ptr: int, ldx: int, y_ptr: int, ldy: int, stream=None) -> None:
        """Device pointers of row-major blocks (element (i, j) at i * ld + j); enqueued on `stream`, not synchronised."""
        check(self._fn(f"spmm_dev_{_sfx(self.dtype)}")(self._h, u64(k), vp(x_ptr), u64(ldx), vp(y_ptr), u64(ldy),
                                                       _stream_ptr(stream)))

    def spmm_torch(self, X, out=None):
        """X: (ncols, k) torch tensor on this handle's device with unit stride in its last dimension -- stride(0) is
        passed as the leading dimension, so a column slice X[:, 2:6] of a wider tensor needs no copy; the same holds
        for `out` (nrows, k).  Runs on torch's current stream."""
        import torch
        nrows, ncols, _ = self.shape()
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32

        def rows_ok(t, rows):   # 2-D, unit stride inside a row, rows ld >= k apart
            return (t.dim() == 2 and t.shape[0] == rows and t.shape[1] >= 1 and t.stride(1) == 1
                    and (t.stride(0) >= t.shape[1] or t.shape[0] <= 1))

        def span(t):            # [first byte, one past the last byte) the kernel may touch
            n = (t.shape[0] - 1) * t.stride(0) + t.shape[1] if t.shape[0] else 0
            return t.data_ptr(), t.data_ptr() + n * t.element_size()

        if X.dtype != tdt or not X.is_cuda or X.dim() != 2:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"X must be a 2-D {tdt} device tensor of shape (ncols = {ncols}, k)")
        if X.shape[0] != ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"assertion failed: ncols == rhs.nrows (left: {ncols}, right: {X.shape[0]})")
        if not rows_ok(X, ncols):
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "X needs k >= 1 columns, unit stride in its last dimension and "
                                                        "stride(0) >= k")
        if X.device.index != self.device:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"X lives on cuda:{X.device.index} but the matrix on cuda:{self.device}")
        k = X.shape[1]
        if out is None:
            out = torch.empty((nrows, k), dtype=tdt, device=X.device)
        elif out.dtype != tdt or not out.is_cuda or not rows_ok(out, nrows) or out.shape[1] != k:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"out must be a {tdt} device tensor of shape (nrows = {nrows}, k = {k}) with unit stride in its "
                        "last dimension")
        elif out.device != X.device:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "out and X live on different devices")
        else:
            (x0, x1), (y0, y1) = span(X), span(out)
            if y0 < x1 and x0 < y1:
                # the spans meet: fine only for disjoint column ranges of one wider row-major buffer (same leading dimension)
                ld, shift = X.stride(0), abs(y0 - x0) // X.element_size() % max(X.stride(0), 1)
                if not (out.stride(0) == ld and k <= shift <= ld - k):
                    raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "out overlaps X (Y = A*X is not computed in place)")
        self.spmm_dev(k, X.data_ptr(), max(X.stride(0), k), out.data_ptr(), max(out.stride(0), k),
                      torch.cuda.current_stream(X.device))
        return out

    def trsv_analyse(self, lower: bool = True, unit_diagonal: bool = False, stream=None) -> dict:
        """Builds the solve plan of one triangle now (spal_*_trsv_analyse: levels on the host, setup time; synchronises
        `stream`) instead of with the first trsv(); returns describe()["trsv"]."""
        check(self._fn("trsv_analyse")(self._h, C.c_int(0 if lower else 1), C.c_int(1 if unit_diagonal else 0),
                                       _stream_ptr(stream)))
        return self.describe()["trsv"]

    def trsv(self, b, lower: bool = True, unit_diagonal: bool = False) -> np.ndarray:
        """Solves L x = b (lower) or U x = b with the chosen triangle of this square matrix; entries of the other
        triangle are ignored.  Host vector in, host vector out.  Bit for bit the sequential substitution.
        A float32 / float64 `b` is passed as it is: a dtype other than the handle's is refused by the library."""
        b = np.ascontiguousarray(b)
        if b.dtype not in (np.float32, np.float64):
            b = b.astype(self.dtype)
        if b.ndim != 1:
            raise TypeError("trsv() takes one right-hand side, a 1-D vector")
        x = np.empty_like(b)
        check(self._fn(f"trsv_{_sfx(b.dtype)}")(self._h, C.c_int(0 if lower else 1), C.c_int(1 if unit_diagonal else 0),
                                                _p(b), u64(b.size), _p(x), u64(x.size)))
        return x

    def trsv_dev(self, b_ptr: int, x_ptr: int, lower: bool = True, unit_diagonal: bool = False, stream=None) -> None:
        """Device pointers (x_ptr == b_ptr solves in place); enqueued on `stream`, not synchronised once the triangle
        has its plan (the first solve of a triangle builds it, which synchronises)."""
        check(self._fn(f"trsv_dev_{_sfx(self.dtype)}")(self._h, C.c_int(0 if lower else 1),
                                                       C.c_int(1 if unit_diagonal else 0), vp(b_ptr), vp(x_ptr),
                                                       _stream_ptr(stream)))

    def trsv_sweep(self, b, sweeps: int, lower: bool = True, unit_diagonal: bool = False) -> np.ndarray:
        """`sweeps` Jacobi passes x <- D^-1 (b - N x) on the chosen triangle instead of the substitution
        (spal_*_trsv_sweep_*): x0 = b / d, every pass one launch of independent rows; bit for bit the
        sequential text in include/spal.h, and trsv()'s result from sweeps = levels - 1 on.  No host analysis.  Host
        vector in, host vector out; a dtype other than the handle's is refused by the library."""
        b = np.ascontiguousarray(b)
        if b.dtype not in (np.float32, np.float64):
            b = b.astype(self.dtype)
        if b.ndim != 1:
            raise TypeError("trsv_sweep() takes one right-hand side, a 1-D vector")
        x = np.empty_like(b)
        check(self._fn(f"trsv_sweep_{_sfx(b.dtype)}")(self._h, C.c_int(0 if lower else 1),
                                                      C.c_int(1 if unit_diagonal else 0), u64(sweeps), _p(b), u64(b.size),
                                                      _p(x), u64(x.size)))
        return x

    def trsv_sweep_dev(self, b_ptr: int, x_ptr: int, sweeps: int, lower: bool = True, unit_diagonal: bool = False,
                       stream=None) -> None:
        """Device pointers (x_ptr == b_ptr is allowed); enqueued on `stream`, not synchronised once the handle is
        prepared (its first sweep call prepares it, which synchronises).  The passes' scratch is taken and returned in
        stream order."""
        check(self._fn(f"trsv_sweep_dev_{_sfx(self.dtype)}")(self._h, C.c_int(0 if lower else 1),
                                                             C.c_int(1 if unit_diagonal else 0), u64(sweeps), vp(b_ptr),
                                                             vp(x_ptr), _stream_ptr(stream)))

    def _block(self, B, who):
        B = np.asarray(B)
        if B.dtype not in (np.float32, np.float64):
            B = B.astype(self.dtype)
        if B.ndim != 2:
            raise TypeError(f"{who}() takes a 2-D block of right-hand sides, shape (nrows, k)")
        return np.ascontiguousarray(B)

    def trsm(self, B, lower: bool = True, unit_diagonal: bool = False) -> np.ndarray:
        """Solves L X = B (lower) or U X = B for a host block B of shape (n, k): every column is, bit for bit, what
        trsv() returns for it, and all k ride on the launches of one vector solve (spal_*_trsm_*).  Host
        block in, host block out; a dtype other than the handle's is refused by the library."""
        B = self._block(B, "trsm")
        n, k = B.shape
        X = np.empty_like(B)
        check(self._fn(f"trsm_{_sfx(B.dtype)}")(self._h, C.c_int(0 if lower else 1), C.c_int(1 if unit_diagonal else 0),
                                                u64(k), _p(B), u64(k), u64(n), _p(X), u64(k), u64(n)))
        return X

    def trsm_dev(self, k: int, b_ptr: int, ldb: int, x_ptr: int, ldx: int, lower: bool = True,
                 unit_diagonal: bool = False, stream=None) -> None:
        """Device pointers of row-major blocks (element (i, j) at i * ld + j; x_ptr == b_ptr with ldx == ldb solves in
        place); enqueued on `stream`, not synchronised once the triangle has its plan -- the one trsv() uses."""
        check(self._fn(f"trsm_dev_{_sfx(self.dtype)}")(self._h, C.c_int(0 if lower else 1),
                                                       C.c_int(1 if unit_diagonal else 0), u64(k), vp(b_ptr), u64(ldb),
                                                       vp(x_ptr), u64(ldx), _stream_ptr(stream)))

    def trsm_sweep(self, B, sweeps: int, lower: bool = True, unit_diagonal: bool = False) -> np.ndarray:
        """`sweeps` Jacobi passes on the chosen triangle for a host block B of shape (n, k): every column is, bit for
        bit, what trsv_sweep() returns for it; a pass stages the matrix once for all k columns (spal_*_trsm_sweep_*,
        DESIGN 3.20).  Host block in, host block out."""
        B = self._block(B, "trsm_sweep")
        n, k = B.shape
        X = np.empty_like(B)
        check(self._fn(f"trsm_sweep_{_sfx(B.dtype)}")(self._h, C.c_int(0 if lower else 1),
                                                      C.c_int(1 if unit_diagonal else 0), u64(sweeps), u64(k), _p(B),
                                                      u64(k), u64(n), _p(X), u64(k), u64(n)))
        return X

    def trsm_sweep_dev(self, k: int, b_ptr: int, ldb: int, x_ptr: int, ldx: int, sweeps: int, lower: bool = True,
                       unit_diagonal: bool = False, stream=None) -> None:
        """Device pointers of row-major blocks (x_ptr == b_ptr with ldx == ldb is allowed); enqueued on `stream`, not
        synchronised once the handle is prepared.  The passes' scratch is taken and returned in stream order."""
        check(self._fn(f"trsm_sweep_dev_{_sfx(self.dtype)}")(self._h, C.c_int(0 if lower else 1),
                                                             C.c_int(1 if unit_diagonal else 0), u64(sweeps), u64(k),
                                                             vp(b_ptr), u64(ldb), vp(x_ptr), u64(ldx),
                                                             _stream_ptr(stream)))

    def trsm_torch(self, B, out=None, lower: bool = True, unit_diagonal: bool = False, sweeps=None):
        """B: (n, k) torch tensor on this handle's device with unit stride in its last dimension -- stride(0) is passed
        as the leading dimension, so a column slice B[:, 2:6] of a wider tensor needs no copy; the same holds for `out`.
        `out is B` solves in place; `sweeps` = None is the exact solve, an integer that many Jacobi passes.  Runs on
        torch's current stream."""
        import torch
        n = self.shape()[0]
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32

        def rows_ok(t):   # 2-D, unit stride inside a row, rows ld >= k apart
            return (t.dim() == 2 and t.shape[0] == n and t.shape[1] >= 1 and t.stride(1) == 1
                    and (t.stride(0) >= t.shape[1] or t.shape[0] <= 1))

        def span(t):      # [first byte, one past the last byte) the kernels may touch
            m = (t.shape[0] - 1) * t.stride(0) + t.shape[1] if t.shape[0] else 0
            return t.data_ptr(), t.data_ptr() + m * t.element_size()

        if B.dtype != tdt or not B.is_cuda or B.dim() != 2:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"B must be a 2-D {tdt} device tensor of shape (n = {n}, k)")
        if B.shape[0] != n:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"B has {B.shape[0]} rows but the matrix has {n} rows")
        if not rows_ok(B):
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "B needs k >= 1 columns, unit stride in its last dimension and "
                                                        "stride(0) >= k")
        if B.device.index != self.device:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"B lives on cuda:{B.device.index} but the matrix on cuda:{self.device}")
        k = B.shape[1]
        if out is None:
            out = torch.empty((n, k), dtype=tdt, device=B.device)
        elif out is not B:
            if out.dtype != tdt or not out.is_cuda or not rows_ok(out) or out.shape[1] != k:
                raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                            f"out must be a {tdt} device tensor of shape (n = {n}, k = {k}) with unit stride in its last "
                            "dimension")
            if out.device != B.device:
                raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "out and B live on different devices")
            (b0, b1), (x0, x1) = span(B), span(out)
            same = x0 == b0 and out.stride(0) == B.stride(0)            # the same block: in place
            if x0 < b1 and b0 < x1 and not same:
                # the spans meet: fine only for disjoint column ranges of one wider row-major buffer (same leading dimension)
                ld, shift = B.stride(0), abs(x0 - b0) // B.element_size() % max(B.stride(0), 1)
                if not (out.stride(0) == ld and k <= shift <= ld - k):
                    raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "out overlaps B (in place needs out is B)")
        ldb, ldx = max(B.stride(0), k), max(out.stride(0), k)
        if out is B:
            ldx = ldb
        st = torch.cuda.current_stream(B.device)
        if sweeps is None:
            self.trsm_dev(k, B.data_ptr(), ldb, out.data_ptr(), ldx, lower, unit_diagonal, st)
        else:
            self.trsm_sweep_dev(k, B.data_ptr(), ldb, out.data_ptr(), ldx, int(sweeps), lower, unit_diagonal, st)
        return out

    def krylov(self, b, method="cg", M=None, x0=None, tol: float = 1e-8, maxit: int = 1000):
        """Solves A x = b by CG ("cg") or BiCGStab ("bicgstab") on the device (spal_*_krylov_*), optionally
        preconditioned by `M`, an ILU(0) factor handle of this class (M^-1 v = two solves on it, or, when M's option
        "trsv_sweeps" is s >= 0, s Jacobi sweeps per triangle).  Host vectors; returns
        (x, KrylovInfo).  Bit for bit the loops written out in include/spal.h, whatever "krylov_check_every" is."""
        b = np.ascontiguousarray(b)
        if b.dtype not in (np.float32, np.float64):
            b = b.astype(self.dtype)
        if b.ndim != 1:
            raise TypeError("krylov() takes one right-hand side, a 1-D vector")
        x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=b.dtype, order="C", copy=True)
        info = _KrylovInfoC()
        if isinstance(M, Amg):   # the same loops with M^-1 v = one multigrid cycle (spal_*_krylov_amg_*)
            check(self._fn(f"krylov_amg_{_sfx(b.dtype)}")(self._h, C.c_int(_krylov_method(method)), M._h, _p(b),
                                                          u64(b.size), _p(x), u64(x.size), C.c_double(tol), u64(maxit),
                                                          C.byref(info)))
            return x, _krylov_info(info)
        if isinstance(M, Fsai):   # ... with M^-1 v = Gt (G v) (spal_*_krylov_fsai_*)
            check(self._fn(f"krylov_fsai_{_sfx(b.dtype)}")(self._h, C.c_int(_krylov_method(method)), M._h, _p(b),
                                                           u64(b.size), _p(x), u64(x.size), C.c_double(tol), u64(maxit),
                                                           C.byref(info)))
            return x, _krylov_info(info)
        if M is not None and type(M) is not type(self):
            raise TypeError(f"M must be a {type(self).__name__} (the factor of a matrix of the same format)")
        check(self._fn(f"krylov_{_sfx(b.dtype)}")(self._h, C.c_int(_krylov_method(method)), M._h if M is not None else None,
                                                  _p(b), u64(b.size), _p(x), u64(x.size), C.c_double(tol), u64(maxit),
                                                  C.byref(info)))
        return x, _krylov_info(info)

    def krylov_dev(self, b_ptr: int, x_ptr: int, method="cg", M=None, tol: float = 1e-8, maxit: int = 1000,
                   stream=None) -> KrylovInfo:
        """Device pointers: x holds x0 on entry and the result on exit; the call polls, so it synchronises `stream`."""
        info = _KrylovInfoC()
        if isinstance(M, Amg):
            check(self._fn(f"krylov_amg_dev_{_sfx(self.dtype)}")(self._h, C.c_int(_krylov_method(method)), M._h,
                                                                 vp(b_ptr), vp(x_ptr), C.c_double(tol), u64(maxit),
                                                                 _stream_ptr(stream), C.byref(info)))
            return _krylov_info(info)
        if isinstance(M, Fsai):
            check(self._fn(f"krylov_fsai_dev_{_sfx(self.dtype)}")(self._h, C.c_int(_krylov_method(method)), M._h,
                                                                  vp(b_ptr), vp(x_ptr), C.c_double(tol), u64(maxit),
                                                                  _stream_ptr(stream), C.byref(info)))
            return _krylov_info(info)
        check(self._fn(f"krylov_dev_{_sfx(self.dtype)}")(self._h, C.c_int(_krylov_method(method)),
                                                         M._h if M is not None else None, vp(b_ptr), vp(x_ptr),
                                                         C.c_double(tol), u64(maxit), _stream_ptr(stream), C.byref(info)))
        return _krylov_info(info)

    def krylov_block(self, B, method="cg", M=None, X0=None, tol: float = 1e-8, maxit: int = 1000):
        """Solves A X = B for a host block B of shape (n, k) by CG or BiCGStab: k independent iterations in lockstep on
        shared launches (spal_*_krylov_block_*).  Column j is, bit for bit, the loop of include/spal.h on
        B[:, j] with SpMM's products and the block solves as M^-1; a column that has stopped is frozen while the others
        run on.  Returns (X, [KrylovInfo] * k)."""
        _refuse_amg(M, "krylov_block()")
        B = self._block(B, "krylov_block")
        n, k = B.shape
        X = np.zeros_like(B) if X0 is None else np.array(X0, dtype=B.dtype, order="C", copy=True)
        if X.shape != B.shape:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"krylov_block: X0 has shape {X.shape} but B {B.shape}")
        if M is not None and type(M) is not type(self):
            raise TypeError(f"M must be a {type(self).__name__} (the factor of a matrix of the same format)")
        infos = (_KrylovInfoC * max(k, 1))()
        check(self._fn(f"krylov_block_{_sfx(B.dtype)}")(self._h, C.c_int(_krylov_method(method)),
                                                        M._h if M is not None else None, u64(k), _p(B), u64(k), u64(n),
                                                        _p(X), u64(k), u64(n), C.c_double(tol), u64(maxit), infos))
        return X, [_krylov_info(c) for c in infos[:k]]

    def krylov_block_dev(self, k: int, b_ptr: int, ldb: int, x_ptr: int, ldx: int, method="cg", M=None,
                         tol: float = 1e-8, maxit: int = 1000, stream=None):
        """Device pointers of row-major blocks (element (i, j) at i * ld + j): X holds X0 on entry and the result on
        exit; the call polls, so it synchronises `stream`.  Returns the k KrylovInfo records."""
        infos = (_KrylovInfoC * max(int(k), 1))()
        check(self._fn(f"krylov_block_dev_{_sfx(self.dtype)}")(self._h, C.c_int(_krylov_method(method)),
                                                               M._h if M is not None else None, u64(k), vp(b_ptr),
                                                               u64(ldb), vp(x_ptr), u64(ldx), C.c_double(tol), u64(maxit),
                                                               _stream_ptr(stream), infos))
        return [_krylov_info(c) for c in infos[:int(k)]]

    def minres(self, b, M=None, shift: float = 0.0, x0=None, tol: float = 1e-8, maxit: int = 1000):
        """Solves (A - shift I) x = b by MINRES on the device (spal_*_minres_*): A symmetric, possibly
        indefinite; `M`, a factor handle of this class, symmetric positive definite and applied as krylov() applies it.
        Host vectors; returns (x, KrylovInfo).  Bit for bit the text written out in include/spal.h, whatever
        "krylov_check_every" is."""
        _refuse_amg(M, "minres()")
        b = np.ascontiguousarray(b)
        if b.dtype not in (np.float32, np.float64):
            b = b.astype(self.dtype)
        if b.ndim != 1:
            raise TypeError("minres() takes one right-hand side, a 1-D vector")
        x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=b.dtype, order="C", copy=True)
        info = _KrylovInfoC()
        if isinstance(M, Fsai):   # M^-1 v = Gt (G v), symmetric positive definite by construction (spal_*_minres_fsai_*)
            check(self._fn(f"minres_fsai_{_sfx(b.dtype)}")(self._h, M._h, C.c_double(shift), _p(b), u64(b.size), _p(x),
                                                           u64(x.size), C.c_double(tol), u64(maxit), C.byref(info)))
            return x, _krylov_info(info)
        if M is not None and type(M) is not type(self):
            raise TypeError(f"M must be a {type(self).__name__} (the factor of a matrix of the same format)")
        check(self._fn(f"minres_{_sfx(b.dtype)}")(self._h, M._h if M is not None else None, C.c_double(shift), _p(b),
                                                  u64(b.size), _p(x), u64(x.size), C.c_double(tol), u64(maxit),
                                                  C.byref(info)))
        return x, _krylov_info(info)

    def minres_dev(self, b_ptr: int, x_ptr: int, M=None, shift: float = 0.0, tol: float = 1e-8, maxit: int = 1000,
                   stream=None) -> KrylovInfo:
        """Device pointers: x holds x0 on entry and the result on exit; the call polls, so it synchronises `stream`."""
        info = _KrylovInfoC()
        if isinstance(M, Fsai):
            check(self._fn(f"minres_fsai_dev_{_sfx(self.dtype)}")(self._h, M._h, C.c_double(shift), vp(b_ptr), vp(x_ptr),
                                                                  C.c_double(tol), u64(maxit), _stream_ptr(stream),
                                                                  C.byref(info)))
            return _krylov_info(info)
        check(self._fn(f"minres_dev_{_sfx(self.dtype)}")(self._h, M._h if M is not None else None, C.c_double(shift),
                                                         vp(b_ptr), vp(x_ptr), C.c_double(tol), u64(maxit),
                                                         _stream_ptr(stream), C.byref(info)))
        return _krylov_info(info)

    def minres_block(self, B, M=None, shift: float = 0.0, X0=None, tol: float = 1e-8, maxit: int = 1000):
        """Solves (A - shift I) X = B for a host block B of shape (n, k) by MINRES: k independent iterations in lockstep
        on shared launches (spal_*_minres_block_*).  Column j is, bit for bit, the text of include/spal.h
        on B[:, j] with SpMM's products and the block solves as M^-1; a column that has stopped is frozen while the
        others run on.  Returns (X, [KrylovInfo] * k)."""
        _refuse_amg(M, "minres_block()")
        B = self._block(B, "minres_block")
        n, k = B.shape
        X = np.zeros_like(B) if X0 is None else np.array(X0, dtype=B.dtype, order="C", copy=True)
        if X.shape != B.shape:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"minres_block: X0 has shape {X.shape} but B {B.shape}")
        if M is not None and type(M) is not type(self):
            raise TypeError(f"M must be a {type(self).__name__} (the factor of a matrix of the same format)")
        infos = (_KrylovInfoC * max(k, 1))()
        check(self._fn(f"minres_block_{_sfx(B.dtype)}")(self._h, M._h if M is not None else None, C.c_double(shift),
                                                        u64(k), _p(B), u64(k), u64(n), _p(X), u64(k), u64(n),
                                                        C.c_double(tol), u64(maxit), infos))
        return X, [_krylov_info(c) for c in infos[:k]]

    def minres_block_dev(self, k: int, b_ptr: int, ldb: int, x_ptr: int, ldx: int, M=None, shift: float = 0.0,
                         tol: float = 1e-8, maxit: int = 1000, stream=None):
        """Device pointers of row-major blocks (element (i, j) at i * ld + j): X holds X0 on entry and the result on
        exit; the call polls, so it synchronises `stream`.  Returns the k KrylovInfo records."""
        infos = (_KrylovInfoC * max(int(k), 1))()
        check(self._fn(f"minres_block_dev_{_sfx(self.dtype)}")(self._h, M._h if M is not None else None,
                                                               C.c_double(shift), u64(k), vp(b_ptr), u64(ldb), vp(x_ptr),
                                                               u64(ldx), C.c_double(tol), u64(maxit),
                                                               _stream_ptr(stream), infos))
        return [_krylov_info(c) for c in infos[:int(k)]]

    def gmres(self, b, M=None, x0=None, restart: int = 30, tol: float = 1e-8, maxit: int = 1000):
        """Solves A x = b by restarted GMRES(restart) on the device (spal_*_gmres_*), right-preconditioned
        by `M` as krylov() is (an ILU(0) factor handle of this class: two solves, or "trsv_sweeps" sweeps per triangle).
        Host vectors; returns (x, KrylovInfo).  Bit for bit the text written out in include/spal.h, whatever
        "krylov_check_every" is."""
        _refuse_amg(M, "gmres()")
        b = np.ascontiguousarray(b)
        if b.dtype not in (np.float32, np.float64):
            b = b.astype(self.dtype)
        if b.ndim != 1:
            raise TypeError("gmres() takes one right-hand side, a 1-D vector")
        x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=b.dtype, order="C", copy=True)
        if M is not None and type(M) is not type(self):
            raise TypeError(f"M must be a {type(self).__name__} (the factor of a matrix of the same format)")
        info = _KrylovInfoC()
        check(self._fn(f"gmres_{_sfx(b.dtype)}")(self._h, M._h if M is not None else None, _p(b), u64(b.size), _p(x),
                                                 u64(x.size), u64(restart), C.c_double(tol), u64(maxit), C.byref(info)))
        return x, _krylov_info(info)

    def gmres_dev(self, b_ptr: int, x_ptr: int, M=None, restart: int = 30, tol: float = 1e-8, maxit: int = 1000,
                  stream=None) -> KrylovInfo:
        """Device pointers: x holds x0 on entry and the result on exit; the call polls, so it synchronises `stream`."""
        info = _KrylovInfoC()
        check(self._fn(f"gmres_dev_{_sfx(self.dtype)}")(self._h, M._h if M is not None else None, vp(b_ptr), vp(x_ptr),
                                                        u64(restart), C.c_double(tol), u64(maxit), _stream_ptr(stream),
                                                        C.byref(info)))
        return _krylov_info(info)

    def gmres_block(self, B, M=None, X0=None, restart: int = 30, tol: float = 1e-8, maxit: int = 1000):
        """Solves A X = B for a host block B of shape (n, k) by restarted GMRES(restart): k independent iterations in
        lockstep on shared launches, with cycles common to the block (spal_*_gmres_block_*).  Column j is,
        bit for bit, the GMRES text of include/spal.h on B[:, j] with SpMM's products and the block solves as M^-1; a
        column whose cycle has ended idles until the others' have, one that has stopped is frozen.  Returns
        (X, [KrylovInfo] * k)."""
        _refuse_amg(M, "gmres_block()")
        B = self._block(B, "gmres_block")
        n, k = B.shape
        X = np.zeros_like(B) if X0 is None else np.array(X0, dtype=B.dtype, order="C", copy=True)
        if X.shape != B.shape:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"gmres_block: X0 has shape {X.shape} but B {B.shape}")
        if M is not None and type(M) is not type(self):
            raise TypeError(f"M must be a {type(self).__name__} (the factor of a matrix of the same format)")
        infos = (_KrylovInfoC * max(k, 1))()
        check(self._fn(f"gmres_block_{_sfx(B.dtype)}")(self._h, M._h if M is not None else None, u64(k), _p(B), u64(k),
                                                       u64(n), _p(X), u64(k), u64(n), u64(restart), C.c_double(tol),
                                                       u64(maxit), infos))
        return X, [_krylov_info(c) for c in infos[:k]]

    def gmres_block_dev(self, k: int, b_ptr: int, ldb: int, x_ptr: int, ldx: int, M=None, restart: int = 30,
                        tol: float = 1e-8, maxit: int = 1000, stream=None):
        """Device pointers of row-major blocks (element (i, j) at i * ld + j): X holds X0 on entry and the result on
        exit; the call polls, so it synchronises `stream`.  Returns the k KrylovInfo records."""
        infos = (_KrylovInfoC * max(int(k), 1))()
        check(self._fn(f"gmres_block_dev_{_sfx(self.dtype)}")(self._h, M._h if M is not None else None, u64(k),
                                                              vp(b_ptr), u64(ldb), vp(x_ptr), u64(ldx), u64(restart),
                                                              C.c_double(tol), u64(maxit), _stream_ptr(stream), infos))
        return [_krylov_info(c) for c in infos[:int(k)]]

    def cheb_apply(self, x, degree: int, lo: float, hi: float, a0: float) -> np.ndarray:
        """t_d = p(A) x for the Chebyshev polynomial of `degree` on [lo, hi] scaled to p(a0) = 1 (spal_*_cheb_apply_*,
        DESIGN 3.26): host vector in, host vector out.  a0 lies outside [lo, hi]; p is small on the interval and grows
        monotonically towards a0.  Bit for bit the text of include/spal.h, whatever the handle's plan is."""
        x = np.ascontiguousarray(x, dtype=self.dtype)
        out = np.empty(self.shape()[0], dtype=self.dtype)
        check(self._fn(f"cheb_apply_{_sfx(self.dtype)}")(self._h, _p(x), u64(x.size), _p(out), u64(out.size), u64(degree),
                                                         C.c_double(lo), C.c_double(hi), C.c_double(a0)))
        return out

    def cheb_apply_dev(self, x_ptr: int, out_ptr: int, degree: int, lo: float, hi: float, a0: float, stream=None) -> None:
        """Device pointers (out must not overlap x); `degree` launches enqueued on `stream`, not synchronised."""
        check(self._fn(f"cheb_apply_dev_{_sfx(self.dtype)}")(self._h, vp(x_ptr or None), vp(out_ptr or None), u64(degree),
                                                             C.c_double(lo), C.c_double(hi), C.c_double(a0), _stream_ptr(stream)))

    def cheb_series(self, x, coef, lo: float, hi: float) -> np.ndarray:
        """s = sum_i coef[i] T_i(B) x, B = A mapped from [lo, hi] onto [-1, 1], T_i the unscaled Chebyshev polynomials
        (spal_*_cheb_series_*): host vector in, host vector out, coef = degree + 1 doubles.  The building
        block of matrix functions and spectral densities.  [lo, hi] must enclose the spectrum, else the T_i grow.  Bit
        for bit the text of include/spal.h, whatever the handle's plan is."""
        x = np.ascontiguousarray(x, dtype=self.dtype)
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        out = np.empty(self.shape()[0], dtype=self.dtype)
        check(self._fn(f"cheb_series_{_sfx(self.dtype)}")(self._h, _p(x), u64(x.size), _p(out), u64(out.size),
                                                          u64(max(coef.size, 1) - 1), C.c_double(lo), C.c_double(hi), _p(coef),
                                                          u64(coef.size)))
        return out

    def cheb_series_dev(self, x_ptr: int, out_ptr: int, coef, lo: float, hi: float, stream=None) -> None:
        """Device pointers (out must not overlap x, which is only read); degree launches enqueued on `stream`, not
        synchronised.  coef is read before the call returns."""
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        check(self._fn(f"cheb_series_dev_{_sfx(self.dtype)}")(self._h, vp(x_ptr or None), vp(out_ptr or None),
                                                              u64(max(coef.size, 1) - 1), C.c_double(lo), C.c_double(hi), _p(coef),
                                                              u64(coef.size), _stream_ptr(stream)))

    def kpm_moments(self, degree: int, probes: int = 8, seed: int = 0, interval=None, Z=None):
        """(mu, info): the Chebyshev moments mu[i, j] = z_j^T T_i(B) z_j, i = 0 .. degree, of `probes` probe columns, B =
        this symmetric matrix mapped from the interval onto [-1, 1] (spal_*_kpm_moments_*).  mu is float64
        of shape (degree + 1, probes): bit for bit the text of include/spal.h.  Z = None: hashed +-1 probes from `seed`
        (kpm_probes gives the same block); else an (n, probes) block of this matrix's dtype.  interval = None:
        Gershgorin's bounds with the margin of eigsh(sigma=...); else (lo, hi), which must enclose the spectrum."""
        n = self.shape()[0]
        if Z is not None:
            Z = np.asarray(Z, dtype=self.dtype)
            if Z.ndim != 2 or Z.shape[0] != n:
                raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"kpm_moments: Z has shape {Z.shape} but the matrix has {n} rows")
            if Z.strides[1] != Z.itemsize or Z.strides[0] % Z.itemsize or Z.strides[0] < Z.shape[1] * Z.itemsize:
                Z = np.ascontiguousarray(Z)
            probes = Z.shape[1]
        degree, k, automatic, lo, hi = _kpm_args("kpm_moments", degree, probes, interval)
        mu = np.empty((degree + 1, k), dtype=np.float64)
        info = _KpmInfoC()
        ldz = k if Z is None else Z.strides[0] // Z.itemsize
        check(self._fn(f"kpm_moments_{_sfx(self.dtype)}")(
            self._h, u64(degree), u64(k), u64(int(seed) % 2**64), C.c_int(automatic), C.c_double(lo), C.c_double(hi),
            None if Z is None else Z.ctypes.data_as(vp), u64(n), u64(ldz), _p(mu), u64(mu.size), C.byref(info)))
        return mu, _kpm_info(info)

    def kpm_moments_dev(self, degree: int, probes: int, seed: int = 0, interval=None, z_ptr: int = 0, ldz: int = 0, stream=None):
        """(mu, info) as kpm_moments, with the probes in device memory at z_ptr (leading dimension ldz >= probes; 0 =
        hashed probes) and everything enqueued on `stream`; the call synchronises the stream once, at its end."""
        degree, k, automatic, lo, hi = _kpm_args("kpm_moments_dev", degree, probes, interval)
        mu = np.empty((degree + 1, k), dtype=np.float64)
        info = _KpmInfoC()
        check(self._fn(f"kpm_moments_dev_{_sfx(self.dtype)}")(
            self._h, u64(degree), u64(k), u64(int(seed) % 2**64), C.c_int(automatic), C.c_double(lo), C.c_double(hi),
            vp(z_ptr or None), u64(ldz if z_ptr else k), _p(mu), u64(mu.size), _stream_ptr(stream), C.byref(info)))
        return mu, _kpm_info(info)

    def gershgorin(self):
        """(glo, ghi): Gershgorin's enclosure of this square matrix's spectrum, in double (spal_*_gershgorin)."""
        lo, hi = C.c_double(), C.c_double()
        check(self._fn("gershgorin")(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def _eigsh_filtered(self, k, w, ncv, v0, seed, tol, maxit, return_eigenvectors, degree, automatic, lo, hi, warmup):
        n = self.shape()[0]
        theta = np.zeros(k, dtype=self.dtype)
        resid = np.zeros(k, dtype=self.dtype)
        X = np.zeros((n, k), dtype=self.dtype) if return_eigenvectors else None
        info = _EigshFilterInfoC()
        check(self._fn(f"eigsh_filtered_{_sfx(self.dtype)}")(
            self._h, u64(k), C.c_int(w), u64(ncv), None if v0 is None else _p(v0), u64(0 if v0 is None else n), u64(seed),
            C.c_double(tol), u64(maxit), u64(degree), C.c_int(automatic), C.c_double(lo), C.c_double(hi), u64(warmup), _p(theta),
            u64(k), _p(resid), u64(k), None if X is None else _p(X), u64(k), u64(n), C.byref(info)))
        pairs = 0 if info.reason == 2 else int(info.converged) if info.reason == 3 else k
        return theta[:pairs], (None if X is None else X[:, :pairs]), _eigsh_filter_info(info, resid[:pairs])

    def _eigsh_near(self, k, ncv, v0, seed, tol, maxit, return_eigenvectors, sigma, degree, automatic, lo, hi):
        n = self.shape()[0]
        theta = np.zeros(k, dtype=self.dtype)
        resid = np.zeros(k, dtype=self.dtype)
        X = np.zeros((n, k), dtype=self.dtype) if return_eigenvectors else None
        info = _EigshNearInfoC()
        check(self._fn(f"eigsh_near_{_sfx(self.dtype)}")(
            self._h, u64(k), C.c_double(sigma), u64(ncv), None if v0 is None else _p(v0), u64(0 if v0 is None else n), u64(seed),
            C.c_double(tol), u64(maxit), u64(degree), C.c_int(automatic), C.c_double(lo), C.c_double(hi), _p(theta), u64(k),
            _p(resid), u64(k), None if X is None else _p(X), u64(k), u64(n), C.byref(info)))
        pairs = 0 if info.reason == 2 else int(info.converged) if info.reason == 3 else k
        return theta[:pairs], (None if X is None else X[:, :pairs]), _eigsh_near_info(info, resid[:pairs])

    def eigsh(self, k: int = 6, which="LA", ncv=None, v0=None, seed: int = 0, tol: float = 0, maxit: int = 1000,
              return_eigenvectors: bool = True, filter_degree: int = 0, filter_interval=None, filter_warmup: int = 5,
              sigma=None):
        """The k largest (which="LA") or smallest ("SA") eigenvalues of this symmetric matrix and their vectors, by
        thick-restart Lanczos with full orthogonalisation on the device (spal_*_eigsh_*); symmetry is not
        checked.  Returns (theta, X, info): theta in the order of `which` (LA descending, SA ascending), X of shape
        (n, pairs) or None, info an EigshInfo.  ncv=None is min(n, max(2k + 1, 20)); tol=0 is the dtype's machine
        epsilon; a pair counts as converged when its estimate is <= tol * max|theta|.  v0=None is the text's start
        vector from `seed`.  Bit for bit the text of include/spal.h.  An eigenvalue of multiplicity > 1 is returned
        ONCE: a single-vector Lanczos iteration sees one direction of its eigenspace.  pairs = k unless the space was
        exhausted earlier (reason 3) or a value was not finite (reason 2: no pair).
        filter_degree > 0 runs Lanczos on a Chebyshev polynomial of A of that degree instead (spal_*_eigsh_filtered_*,
        DESIGN 3.26), the remedy for CLUSTERED extreme eigenvalues: filter_interval=None takes the interval to damp from
        `filter_warmup` restarts of the plain iteration, (lo, hi) gives it; convergence is then decided on true
        residuals, <= tol * max(|glo|, |ghi|) of Gershgorin's bounds, tol=0 is 256 machine epsilons, info.resid holds
        them and info gains warm_restarts, warm_products, lo, hi, a0, degree.  filter_degree=0 is the plain call.
        sigma=s returns the k eigenvalues NEAREST s, inside the spectrum too (spal_*_eigsh_near_*): Lanczos
        on a Chebyshev delta filter of degree filter_degree >= 2 at s -- there is no shift-invert, so a degree is
        required, and which="SA" is a ValueError.  filter_interval=None is Gershgorin's interval with a margin, (lo, hi)
        must enclose the spectrum; s lies strictly inside.  filter_warmup is ignored.  The pairs come in DESCENDING ORDER
        OF THE FILTER VALUE, which near s is ascending distance from s; convergence is on true residuals as above and
        info gains lo, hi, sigma, gamma, degree.  TWO-TO-ONE: eigenvalues at the same filter value -- mirror images in a
        spectrum symmetric about s -- are not separated; the call then ends with reason 1.  Move s off the centre."""
        n, ncols, _ = self.shape()
        tol_given = float(tol)
        near = None if sigma is None else _near_args(sigma, which, filter_degree, filter_interval)
        k, ncv, tol = _eigsh_args(n, ncols, k, ncv, tol, self.dtype)
        w = _eigsh_which(which)
        if v0 is not None:
            v0 = np.ascontiguousarray(v0, dtype=self.dtype)
            if v0.shape != (n,):
                raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: v0 has shape {v0.shape} but the matrix has {n} rows")
        if near is not None:
            return self._eigsh_near(k, ncv, v0, seed, tol_given, maxit, return_eigenvectors, *near)
        if filter_degree:
            return self._eigsh_filtered(k, w, ncv, v0, seed, tol_given, maxit, return_eigenvectors,
                                        *_filter_args(filter_degree, filter_interval, filter_warmup))
        theta = np.zeros(k, dtype=self.dtype)
        resid = np.zeros(k, dtype=self.dtype)
        X = np.zeros((n, k), dtype=self.dtype) if return_eigenvectors else None
        info = _EigshInfoC()
        check(self._fn(f"eigsh_{_sfx(self.dtype)}")(self._h, u64(k), C.c_int(w), u64(ncv), None if v0 is None else _p(v0),
                                                    u64(0 if v0 is None else n), u64(seed), C.c_double(tol), u64(maxit),
                                                    _p(theta), u64(k), _p(resid), u64(k), None if X is None else _p(X),
                                                    u64(k), u64(n), C.byref(info)))
        pairs = 0 if info.reason == 2 else int(info.converged) if info.reason == 3 else k
        out = _eigsh_info(info, resid[:pairs])
        return theta[:pairs], (None if X is None else X[:, :pairs]), out

    def eigsh_dev(self, k: int, theta, resid, x_ptr: int, ldx: int, which="LA", ncv=None, v0_ptr: int = 0, seed: int = 0,
                  tol: float = 0, maxit: int = 1000, stream=None, filter_degree: int = 0, filter_interval=None,
                  filter_warmup: int = 5, sigma=None):
        """Device pointers: v0_ptr (0: the text's start vector) and x_ptr (0: values only; else n x k row-major with
        leading dimension ldx); theta and resid are host arrays of k values of the handle's dtype, written in place.
        The call polls, so it synchronises `stream`.  Returns the EigshInfo.  filter_degree > 0: the filtered call, as
        in eigsh(); sigma: the k pairs nearest sigma, as in eigsh()."""
        n, ncols, _ = self.shape()
        tol_given = float(tol)
        near = None if sigma is None else _near_args(sigma, which, filter_degree, filter_interval)
        k, ncv, tol = _eigsh_args(n, ncols, k, ncv, tol, self.dtype)
        for a in (theta, resid):
            if not isinstance(a, np.ndarray) or a.dtype != self.dtype or a.shape != (k,) or not a.flags.c_contiguous:
                raise TypeError(f"theta and resid must be contiguous arrays of {k} {self.dtype} values")
        if near is not None:
            sg, degree, automatic, lo, hi = near
            ninfo = _EigshNearInfoC()
            check(self._fn(f"eigsh_near_dev_{_sfx(self.dtype)}")(
                self._h, u64(k), C.c_double(sg), u64(ncv), vp(v0_ptr or None), u64(seed), C.c_double(tol_given), u64(maxit),
                u64(degree), C.c_int(automatic), C.c_double(lo), C.c_double(hi), _p(theta), _p(resid), vp(x_ptr or None), u64(ldx),
                _stream_ptr(stream), C.byref(ninfo)))
            pairs = 0 if ninfo.reason == 2 else int(ninfo.converged) if ninfo.reason == 3 else k
            return _eigsh_near_info(ninfo, resid[:pairs])
        if filter_degree:
            degree, automatic, lo, hi, warmup = _filter_args(filter_degree, filter_interval, filter_warmup)
            finfo = _EigshFilterInfoC()
            check(self._fn(f"eigsh_filtered_dev_{_sfx(self.dtype)}")(
                self._h, u64(k), C.c_int(_eigsh_which(which)), u64(ncv), vp(v0_ptr or None), u64(seed), C.c_double(tol_given),
                u64(maxit), u64(degree), C.c_int(automatic), C.c_double(lo), C.c_double(hi), u64(warmup), _p(theta), _p(resid),
                vp(x_ptr or None), u64(ldx), _stream_ptr(stream), C.byref(finfo)))
            pairs = 0 if finfo.reason == 2 else int(finfo.converged) if finfo.reason == 3 else k
            return _eigsh_filter_info(finfo, resid[:pairs])
        info = _EigshInfoC()
        check(self._fn(f"eigsh_dev_{_sfx(self.dtype)}")(self._h, u64(k), C.c_int(_eigsh_which(which)), u64(ncv), vp(v0_ptr or None),
                                                        u64(seed), C.c_double(tol), u64(maxit), _p(theta), _p(resid),
                                                        vp(x_ptr or None), u64(ldx), _stream_ptr(stream), C.byref(info)))
        pairs = 0 if info.reason == 2 else int(info.converged) if info.reason == 3 else k
        return _eigsh_info(info, resid[:pairs])

    def amg(self, seed: int = 0, max_levels: int = 16, coarse_rows: int = 64, nu: int = 2, coarse_sweeps: int = 16,
            cycle: str = "v", omega: float = 2.0 / 3.0, alpha: float = 1.0, stream=None) -> Amg:
        """The aggregation AMG hierarchy of this square matrix (spal_*_amg_setup): an Amg, built on the
        device level after level; synchronises `stream`."""
        params = _amg_params(seed, max_levels, coarse_rows, nu, coarse_sweeps, cycle, omega, alpha)
        out = vp()
        check(self._fn("amg_setup")(self._h, C.byref(params), _stream_ptr(stream), C.byref(out)))
        return Amg(out, self.dtype, self.device, self.shape()[0])

    def fsai(self, pattern=None, max_row=None, stream=None) -> Fsai:
        """The FSAI factor of this square matrix on the pattern of `pattern`, a handle of this class (None: this
        matrix's own), an Fsai (spal_*_fsai_setup).  `max_row` sets the option "fsai_max_row" (1 .. 64,
        default 32) for this call and restores it afterwards; synchronises `stream`."""
        if pattern is not None and type(pattern) is not type(self):
            raise TypeError(f"pattern must be a {type(self).__name__} (a matrix of the same format)")
        keep = getattr(self, "_fsai_max_row", 32)
        out = vp()
        if max_row is not None:
            self.set_option("fsai_max_row", int(max_row))
        try:
            check(self._fn("fsai_setup")(self._h, pattern._h if pattern is not None else None, _stream_ptr(stream),
                                         C.byref(out)))
        finally:
            if max_row is not None:
                self.set_option("fsai_max_row", keep)
        return Fsai(out, self.dtype, self.device, self.shape()[0])

    def colour(self, seed: int = 0, stream=None):
        """The greedy colouring of this square matrix's graph by hashed priority (spal_*_colour): exactly
        the sequential text of include/spal.h, by Jones-Plassmann rounds on the device.  Returns (colours as a uint64
        array, ncolours, rounds); synchronises `stream`."""
        n = self.shape()[0]
        colours = np.empty(n, dtype=np.uint64)
        nc, rounds = u64(), u64()
        check(self._fn("colour")(self._h, u64(seed), _stream_ptr(stream), _p(colours), C.byref(nc), C.byref(rounds)))
        return colours, nc.value, rounds.value

    def permute(self, perm, stream=None):
        """B = P A P^T as a new handle of this class, B[i'][j'] = A[perm[i']][perm[j']] for any permutation `perm`
        (new -> old); values are moved, never recomputed.  The result keeps `perm` (ordering(), permute_vec())."""
        perm = _idx(perm)
        out = vp()
        check(self._fn("permute")(self._h, _p(perm), u64(perm.size), _stream_ptr(stream), C.byref(out)))
        return type(self)(out, self.dtype, self.device)

    def multicolour(self, seed: int = 0, stream=None):
        """colour -> order by (colour, row) -> permute, on the device (spal_*_multicolour): a new handle of this class
        whose two triangles have at most ncolours levels each; ordering() returns its perm and ncolours."""
        out, nc = vp(), u64()
        check(self._fn("multicolour")(self._h, u64(seed), _stream_ptr(stream), C.byref(out), C.byref(nc)))
        return type(self)(out, self.dtype, self.device)

    def ordering(self):
        """(perm, ncolours) of a handle made by permute() (ncolours = 0) or multicolour(); any other handle is refused."""
        perm = np.empty(self.shape()[0], dtype=np.uint64)
        nc = u64()
        check(self._fn("ordering")(self._h, _p(perm), C.byref(nc)))
        return perm, nc.value

    def permute_vec(self, x, back: bool = False) -> np.ndarray:
        """Host vectors: x[perm] (into this handle's order), or with `back` the inverse, y[perm] = x."""
        x = np.ascontiguousarray(x)
        if x.dtype not in (np.float32, np.float64):
            x = x.astype(self.dtype)
        y = np.empty_like(x)
        check(self._fn(f"permute_vec_{_sfx(x.dtype)}")(self._h, _p(x), u64(x.size), _p(y), u64(y.size),
                                                       C.c_int(1 if back else 0)))
        return y

    def permute_vec_dev(self, x_ptr: int, y_ptr: int, back: bool = False, stream=None) -> None:
        """Device pointers, x_ptr != y_ptr; enqueued on `stream`, not synchronised."""
        check(self._fn(f"permute_vec_dev_{_sfx(self.dtype)}")(self._h, vp(x_ptr), vp(y_ptr), C.c_int(1 if back else 0),
                                                           _stream_ptr(stream)))

    def alloc_vectors(self, stream=None):
        """Device pointers (x, y) of vectors owned by this handle and placed so that the stores of y do not collide
        with the matrix stream (spal_csr_alloc_vectors: a walk over the device's memory, setup time).  CSR handles."""
        if self._kind != "csr":   # the entry point reads a spal_csr: never hand it another handle type
            raise TypeError("alloc_vectors() exists for CSR handles only (spal_csr_alloc_vectors)")
        x, y = vp(), vp()
        check(_ffi.lib().spal_csr_alloc_vectors(self._h, C.byref(x), C.byref(y), _stream_ptr(stream)))
        return x.value, y.value

    def vectors_torch(self):
        """alloc_vectors() as torch tensors (zero-copy views of the handle's block; they keep the handle alive)."""
        import torch
        nrows, ncols, _ = self.shape()
        xp, yp = self.alloc_vectors(torch.cuda.current_stream(self.device))

        class _View:
            def __init__(self, owner, ptr, n, dtype):
                self._owner = owner
                self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": np.dtype(dtype).str, "data": (int(ptr), False),
                                                 "version": 2, "strides": None}
        dev = torch.device("cuda", self.device)
        return (torch.as_tensor(_View(self, xp, ncols, self.dtype), device=dev),
                torch.as_tensor(_View(self, yp, nrows, self.dtype), device=dev))

    def _binary(self, op: str, other, stream):
        """spal_<kind>_add / _sub: a new handle of this class (both operands of one format, as in the reference)."""
        if type(other) is not type(self):
            raise TypeError(f"{type(self).__name__}.{op} needs a {type(self).__name__} (the reference has no mixed operands)")
        out = vp()
        check(self._fn(op)(self._h, other._h, _stream_ptr(stream), C.byref(out)))
        return type(self)(out, self.dtype, self.device)

    def autotune(self, x, y, iters: int = 30) -> dict:
        """Times the plan's kernel variants on torch device vectors x, y and keeps
        the fastest (setup-time; synchronises the current stream)."""
        import torch
        st = torch.cuda.current_stream(x.device)
        check(self._fn(f"autotune_{_sfx(self.dtype)}")(self._h, vp(x.data_ptr()), vp(y.data_ptr()),
                                                       _stream_ptr(st), C.c_int(iters)))
        return self.describe()

    def spmv_torch(self, x, out=None):
        """x, out: torch tensors on this handle's device; runs on torch's
        current stream (so torch.cuda.Event brackets it)."""
        import torch
        nrows, ncols, _ = self.shape()
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        if x.dtype != tdt or not x.is_cuda or not x.is_contiguous() or x.numel() != ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"x must be a contiguous {tdt} device vector of length ncols = {ncols}")
        if x.device.index != self.device:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"x lives on cuda:{x.device.index} but the matrix on cuda:{self.device}")
        if out is None:
            out = torch.empty(nrows, dtype=tdt, device=x.device)
        elif out.dtype != tdt or not out.is_cuda or not out.is_contiguous() or out.numel() != nrows:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"out must be a contiguous {tdt} device vector of length nrows = {nrows}")
        elif out.device != x.device:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "out and x live on different devices")
        else:
            # the kernels read x and write y through __restrict__ pointers: the two must not overlap
            es = x.element_size()
            if out.data_ptr() < x.data_ptr() + ncols * es and x.data_ptr() < out.data_ptr() + nrows * es:
                raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "out overlaps x (y = A*x is not computed in place)")
        self.spmv_dev(x.data_ptr(), out.data_ptr(), torch.cuda.current_stream(x.device))
        return out


def _sweep_count(sweeps) -> int:
    """ilu0(sweeps=...): an integer >= 0 (bool is not one), at most what the ABI's uint64_t holds."""
    if isinstance(sweeps, bool) or not isinstance(sweeps, (int, np.integer)):
        raise TypeError(f"sweeps must be None or an integer >= 0, not {type(sweeps).__name__}")
    if sweeps < 0:
        raise ValueError(f"sweeps must be >= 0, not {sweeps}")
    return min(int(sweeps), 2 ** 64 - 1)


class DeviceCsr(_DeviceMatrix):
    _kind = "csr"

    def plan(self) -> None:
        """spal_csr_plan: builds the product kernels' plan of a device-assembled handle now (otherwise its first product,
        set_option, autotune, alloc_vectors or describe does).  No-op on handles created from host arrays."""
        check(_ffi.lib().spal_csr_plan(self._h))

    def download(self):
        nrows, _, nnz = self.shape()
        rp = np.empty(nrows + 1, dtype=np.uint64)
        ci = np.empty(nnz, dtype=np.uint64)
        va = np.empty(nnz, dtype=self.dtype)
        check(self._fn(f"download_{_sfx(self.dtype)}")(self._h, _p(rp), _p(ci), _p(va)))
        return rp, ci, va

    def to_csc(self) -> "DeviceCsc":
        """device CSR -> CSC (stable sort by column; src/csc/conv/csr.rs:4-52)"""
        out = vp()
        check(_ffi.lib().spal_csr_to_csc(self._h, C.byref(out)))
        return DeviceCsc(out, self.dtype, self.device)

    def mul(self, other: "DeviceCsr", stream=None) -> "DeviceCsr":
        """C = self * other on the device (spal_csr_mul: `impl Mul for &CsrMatrix<T>`, src/csr/ops/mul.rs:5-59,
        bit-identical); synchronises `stream`.  Options "spgemm_route" / "spgemm_lds_cap" are read from self."""
        if not isinstance(other, DeviceCsr):
            raise TypeError("DeviceCsr.mul needs a DeviceCsr (the reference has no mixed CSR x CSC Mul)")
        out = vp()
        check(_ffi.lib().spal_csr_mul(self._h, other._h, _stream_ptr(stream), C.byref(out)))
        return DeviceCsr(out, self.dtype, self.device)

    def add(self, other: "DeviceCsr", stream=None) -> "DeviceCsr":
        """C = self + other on the device (spal_csr_add: `impl Add for &CsrMatrix<T>`, src/csr/ops/add.rs:5-75,
        bit-identical); synchronises `stream`.  Option "spadd_tile" is read from self."""
        return self._binary("add", other, stream)

    def sub(self, other: "DeviceCsr", stream=None) -> "DeviceCsr":
        """C = self - other (spal_csr_sub: `impl Sub for &CsrMatrix<T>`, src/csr/ops/sub.rs:5-75)."""
        return self._binary("sub", other, stream)

    def neg(self, stream=None) -> "DeviceCsr":
        """C = -self (spal_csr_neg: `impl Neg for &CsrMatrix<T>`, src/csr/ops/neg.rs:5-17)."""
        out = vp()
        check(_ffi.lib().spal_csr_neg(self._h, _stream_ptr(stream), C.byref(out)))
        return DeviceCsr(out, self.dtype, self.device)

    def ilu0(self, stream=None, sweeps=None) -> "DeviceCsr":
        """The ILU(0) factor of this square matrix as a new handle of the same structure (spal_csr_ilu0):
        L strictly below the diagonal, its unit diagonal implied, U on and above it; bit for bit the sequential loop.
        Synchronises `stream`.  Applying the preconditioner is two solves on the result::

            f = a.ilu0()
            z = f.trsv(f.trsv(r, lower=True, unit_diagonal=True), lower=False)      # z = U^-1 L^-1 r

        The result already has its lower solve plan (a copy of self's); options "ilu_wide_work" and
        "trsv_chain_rows" are read from self.

        `sweeps` = None is that exact call; an integer s >= 0 builds the factor by s row sweeps instead
        (spal_csr_ilu0_sweep): every pass factorises every row on its own against the previous pass's
        factor -- no analysis, no solve plan, one SpMV-shaped launch per pass, bit for bit its sequential text and the
        exact factor's bits from s = levels - 1 on.  Apply it by sweeps as well (trsv_sweep, `precond_sweeps`)."""
        out = vp()
        if sweeps is None:
            check(_ffi.lib().spal_csr_ilu0(self._h, _stream_ptr(stream), C.byref(out)))
        else:
            check(_ffi.lib().spal_csr_ilu0_sweep(self._h, u64(_sweep_count(sweeps)), _stream_ptr(stream), C.byref(out)))
        return DeviceCsr(out, self.dtype, self.device)


class DeviceCsc(_DeviceMatrix):
    _kind = "csc"

    def download(self):
        _, ncols, nnz = self.shape()
        cp = np.empty(ncols + 1, dtype=np.uint64)
        ri = np.empty(nnz, dtype=np.uint64)
        va = np.empty(nnz, dtype=self.dtype)
        check(self._fn(f"download_{_sfx(self.dtype)}")(self._h, _p(cp), _p(ri), _p(va)))
        return cp, ri, va

    def invalid_products(self) -> int:
        """spal_csc_status: device-pointer products of this handle whose hand-off hit its spin bound (their y was not
        valid); call after synchronising the stream."""
        n = C.c_int(-1)
        check(_ffi.lib().spal_csc_status(self._h, C.byref(n)))
        return n.value

    def to_csr(self) -> DeviceCsr:
        """device CSC -> CSR (stable sort by row; src/csr/conv/csc.rs:4-52)"""
        out = vp()
        check(_ffi.lib().spal_csc_to_csr(self._h, C.byref(out)))
        return DeviceCsr(out, self.dtype, self.device)

    def mul(self, other: "DeviceCsc", stream=None) -> "DeviceCsc":
        """C = self * other on the device (spal_csc_mul: `impl Mul for &CscMatrix<T>`, src/csc/ops/mul.rs:5-60,
        bit-identical); synchronises `stream`.  Options "spgemm_route" / "spgemm_lds_cap" are read from self."""
        if not isinstance(other, DeviceCsc):
            raise TypeError("DeviceCsc.mul needs a DeviceCsc (the reference has no mixed CSR x CSC Mul)")
        out = vp()
        check(_ffi.lib().spal_csc_mul(self._h, other._h, _stream_ptr(stream), C.byref(out)))
        return DeviceCsc(out, self.dtype, self.device)

    def add(self, other: "DeviceCsc", stream=None) -> "DeviceCsc":
        """C = self + other on the device (spal_csc_add: `impl Add for &CscMatrix<T>`, src/csc/ops/add.rs:5-70)."""
        return self._binary("add", other, stream)

    def sub(self, other: "DeviceCsc", stream=None) -> "DeviceCsc":
        """C = self - other (spal_csc_sub: `impl Sub for &CscMatrix<T>`, src/csc/ops/sub.rs:5-70)."""
        return self._binary("sub", other, stream)

    def neg(self, stream=None) -> "DeviceCsc":
        """C = -self (spal_csc_neg: `impl Neg for &CscMatrix<T>`, src/csc/ops/neg.rs:5-17)."""
        out = vp()
        check(_ffi.lib().spal_csc_neg(self._h, _stream_ptr(stream), C.byref(out)))
        return DeviceCsc(out, self.dtype, self.device)

    def ilu0(self, stream=None, sweeps=None) -> "DeviceCsc":
        """The ILU(0) factor as a new CSC handle (spal_csc_ilu0, or spal_csc_ilu0_sweep when `sweeps` is given: the CSR
        twin is factorised, the factor returned by columns); see DeviceCsr.ilu0 for the contract and the application."""
        out = vp()
        if sweeps is None:
            check(_ffi.lib().spal_csc_ilu0(self._h, _stream_ptr(stream), C.byref(out)))
        else:
            check(_ffi.lib().spal_csc_ilu0_sweep(self._h, u64(_sweep_count(sweeps)), _stream_ptr(stream), C.byref(out)))
        return DeviceCsc(out, self.dtype, self.device)


class DeviceCoo:
    """Device-resident COO triplets (SoA, 32-bit indices): the input of the
    timed assembly path."""

    def __init__(self, handle, dtype, device, nrows, ncols, length):
        self._h, self.dtype, self.device = handle, np.dtype(dtype), device
        self.nrows, self.ncols, self.length = nrows, ncols, length

    def assemble_csr(self, stream=None) -> DeviceCsr:
        """COO -> CSR on the device (one host sync for the output size)."""
        out = vp()
        check(_ffi.lib().spal_coo_assemble_csr(self._h, _stream_ptr(stream), C.byref(out)))
        return DeviceCsr(out, self.dtype, self.device)

    def assemble_csc(self, stream=None) -> DeviceCsc:
        """COO -> CSC on the device (src/csc/conv/coo.rs:4-115)."""
        out = vp()
        check(_ffi.lib().spal_coo_assemble_csc(self._h, _stream_ptr(stream), C.byref(out)))
        return DeviceCsc(out, self.dtype, self.device)

    def describe(self) -> dict:
        """The handle and the route its last assembly took (tile geometry of the local sort)."""
        buf = C.create_string_buffer(1024)
        check(_ffi.lib().spal_coo_describe(self._h, buf, C.c_size_t(len(buf))))
        return json.loads(buf.value.decode())

    def close(self):
        if self._h is not None:
            _ffi.lib().spal_coo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiGpuCsr:
    """A CsrMatrix partitioned by rows over `ngpus` GPUs of this node, driven
    from this one process (C ABI spal_mg_*): every GPU reads
    only its window of x (scatter_x; broadcast_x sends all of it), local
    kernels, y slices gathered on GPU 0 (gather_y) or all-gathered
    (spmv_resident), per-step halo exchange for iterative use (spmv_halo).

    transport: "rccl" (grouped ncclSend/ncclRecv over xGMI), "copy" (peer
    copies ordered by events; also takes a device list with repeats, i.e.
    several shards on one GPU) or None = rccl unless `devices` repeats."""

    PHASES = ("x_distribution", "compute", "halo", "y_collection")

    def __init__(self, csr: "CsrMatrix", ngpus: int, devices=None, transport=None):
        self.dtype = csr.dtype
        self._ctx, self._h = vp(), vp()
        dev = (C.c_int * ngpus)(*devices) if devices is not None else None
        tr = {None: -1, "rccl": 0, "copy": 1}[transport]
        check(_ffi.lib().spal_mg_create_transport(C.c_int(ngpus), dev, C.c_int(tr), C.byref(self._ctx)))
        try:
            check(getattr(_ffi.lib(), f"spal_mg_csr_create_{_sfx(self.dtype)}")(
                self._ctx, u64(csr.nrows()), u64(csr.ncols()), _p(csr.rowptr()), u64(csr.rowptr().size),
                _p(csr.colind()), u64(csr.colind().size), _p(csr.values()), u64(csr.values().size),
                C.byref(self._h)))
        except Exception:
            _ffi.lib().spal_mg_destroy(self._ctx)
            self._ctx = None
            raise
        self.nrows, self.ncols, self.ngpus = csr.nrows(), csr.ncols(), ngpus
        t = C.c_int(0)
        check(_ffi.lib().spal_mg_transport(self._ctx, C.byref(t)))
        self.transport = "rccl" if t.value == 0 else "copy"
        self.root_device = devices[0] if devices is not None else 0
        self.devices = list(devices) if devices is not None else list(range(ngpus))

    def partition(self) -> np.ndarray:
        b = np.empty(self.ngpus + 1, dtype=np.uint64)
        check(_ffi.lib().spal_mg_csr_partition(self._h, _p(b)))
        return b

    def windows(self):
        """per GPU: its rows store columns in [need_lo[g], need_hi[g]) only"""
        lo, hi = np.empty(self.ngpus, dtype=np.uint64), np.empty(self.ngpus, dtype=np.uint64)
        check(_ffi.lib().spal_mg_csr_windows(self._h, _p(lo), _p(hi)))
        return lo, hi

    def exchange_bytes(self) -> dict:
        x, y, h = u64(), u64(), u64()
        check(_ffi.lib().spal_mg_csr_exchange_bytes(self._h, C.byref(x), C.byref(y), C.byref(h)))
        return {"x_scatter": x.value, "y_gather": y.value, "halo": h.value}

    def spmv(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=self.dtype)
        y = np.empty(self.nrows, dtype=self.dtype)
        check(getattr(_ffi.lib(), f"spal_mg_csr_spmv_{_sfx(self.dtype)}")(self._h, _p(x), u64(x.size), _p(y), u64(y.size)))
        return y

    # ---- resident path (asynchronous on the context's streams until synchronize) ----
    def _call(self, name):
        check(getattr(_ffi.lib(), f"spal_mg_csr_{name}")(self._h))

    def set_x(self, x) -> None:
        """host vector -> GPU 0's x buffer (synchronous copy)"""
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if x.size != self.ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"assertion failed: ncols == x.len() (left: {self.ncols}, right: {x.size})")
        ptr = vp()
        self.synchronize()
        check(_ffi.lib().spal_mg_csr_x_root(self._h, C.byref(ptr)))
        check(_ffi.lib().spal_memcpy_h2d(C.c_int(self.root_device), ptr, _p(x), C.c_size_t(x.nbytes)))

    def broadcast_x(self): self._call("broadcast_x")
    def scatter_x(self): self._call("scatter_x")
    def spmv_local(self): self._call("spmv_local")
    def gather_y(self): self._call("gather_y")
    def spmv_halo(self): self._call("spmv_halo")
    def spmv_resident(self): self._call("spmv_resident")
    def synchronize(self): self._call("synchronize")

    def y_gathered(self) -> np.ndarray:
        """GPU 0's y after gather_y (synchronises)"""
        self.synchronize()
        ptr = vp()
        check(_ffi.lib().spal_mg_csr_y_gathered(self._h, C.byref(ptr)))
        y = np.empty(self.nrows, dtype=self.dtype)
        check(_ffi.lib().spal_memcpy_d2h(C.c_int(self.root_device), _p(y), ptr, C.c_size_t(y.nbytes)))
        return y

    def y_allgathered(self) -> np.ndarray:
        """GPU 0's copy of the all-gathered y after spmv_resident (synchronises)"""
        self.synchronize()
        ptr, stride = vp(), u64()
        check(_ffi.lib().spal_mg_csr_y_root(self._h, C.byref(ptr), C.byref(stride)))
        pad = np.empty(self.ngpus * stride.value, dtype=self.dtype)
        check(_ffi.lib().spal_memcpy_d2h(C.c_int(self.root_device), _p(pad), ptr, C.c_size_t(pad.nbytes)))
        b = self.partition().astype(np.int64)
        return np.concatenate([pad[g * stride.value: g * stride.value + (b[g + 1] - b[g])] for g in range(self.ngpus)])

    def timing(self) -> dict:
        """HIP-event durations (ms, longest over the GPUs) of the last x distribution, local kernels,
        halo exchange and y collection; None for a phase that has not run.  Synchronises."""
        ms = (C.c_double * 4)()
        check(_ffi.lib().spal_mg_csr_timing(self._h, ms))
        return {k: (None if ms[i] < 0 else ms[i]) for i, k in enumerate(self.PHASES)}

    def close(self):
        if getattr(self, "_h", None):
            _ffi.lib().spal_mg_csr_destroy(self._h)
            self._h = None
        if getattr(self, "_ctx", None):
            _ffi.lib().spal_mg_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------
# CsrMatrix / CscMatrix
# --------------------------------------------------------------------------
class _Compressed:
    _kind = ""
    _dev_cls = _DeviceMatrix

    def __init__(self, nrows, ncols, ptr, ind, values):
        dt = _scalar_dtype(values)
        self._nrows, self._ncols = int(nrows), int(ncols)
        if self._nrows < 0 or self._ncols < 0:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "negative dimension")
        self._ptr, self._ind = _idx(ptr), _idx(ind)
        self._values = np.ascontiguousarray(values, dtype=dt)
        # the constructor's assertions, checked by the library's host code
        reason = C.c_int(0)
        check(getattr(_ffi.lib(), f"spal_{self._kind}_validate")(
            u64(self._nrows), u64(self._ncols), _p(self._ptr), u64(self._ptr.size),
            _p(self._ind), u64(self._ind.size), u64(self._values.size), C.byref(reason)))
        self._dev = {}

    @classmethod
    def _trusted(cls, nrows, ncols, ptr, ind, values):
        """struct-literal construction (what the reference's conversions do,
        e.g. src/csr/conv/coo.rs:108-114): no validation."""
        self = cls.__new__(cls)
        self._nrows, self._ncols = int(nrows), int(ncols)
        self._ptr, self._ind, self._values = ptr, ind, values
        self._dev = {}
        return self

    # accessors (src/csr.rs:200-289)
    def nrows(self) -> int:
        return self._nrows

    def ncols(self) -> int:
        return self._ncols

    def values(self) -> np.ndarray:
        return self._values

    def nnz(self) -> int:
        return int(self._ptr[-1])

    @property
    def dtype(self) -> np.dtype:
        return self._values.dtype

    def device(self, device: int = 0):
        """The device-resident copy (created on first use)."""
        h = self._dev.get(device)
        if h is None or h._h is None:
            out = vp()
            check(getattr(_ffi.lib(), f"spal_{self._kind}_create_{_sfx(self.dtype)}")(
                C.c_int(device), u64(self._nrows), u64(self._ncols), _p(self._ptr),
                u64(self._ptr.size), _p(self._ind), u64(self._ind.size), _p(self._values),
                u64(self._values.size), C.byref(out)))
            h = self._dev_cls(out, self.dtype, device)
            self._dev[device] = h
        return h

    def device_copy(self, device: int = 0):
        """ANOTHER device-resident copy with arrays of its own, not cached on the matrix (benchmarks rotate their
        launches over several, so that a matrix smaller than the 256 MB Infinity Cache is not served from it)."""
        out = vp()
        check(getattr(_ffi.lib(), f"spal_{self._kind}_create_{_sfx(self.dtype)}")(
            C.c_int(device), u64(self._nrows), u64(self._ncols), _p(self._ptr),
            u64(self._ptr.size), _p(self._ind), u64(self._ind.size), _p(self._values),
            u64(self._values.size), C.byref(out)))
        return self._dev_cls(out, self.dtype, device)

    def _mul_vec(self, x):
        x = np.asarray(x)
        if x.ndim == 2:
            return self._mul_block(x)
        if x.ndim != 1:
            raise TypeError("right-hand side must be a dense vector or a 2-D block of vectors")
        if x.shape[0] != self._ncols:
            # assert_eq!(self.ncols(), rhs.nrows())  src/csr/ops/mul.rs:9
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"assertion failed: ncols == x.len() (left: {self._ncols}, right: {x.shape[0]})")
        return self.device().spmv(x.astype(self.dtype, copy=False))

    def _mul_block(self, X):
        """`&self * &X` for a dense block X of shape (ncols, k): a (nrows, k) ndarray (SpMM, one pass over the matrix)."""
        if X.shape[0] != self._ncols:
            # assert_eq!(self.ncols(), rhs.nrows())  mul.rs:9 -- before any device copy is made
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"assertion failed: ncols == rhs.nrows (left: {self._ncols}, right: {X.shape[0]})")
        return self.device().spmm(X.astype(self.dtype, copy=False))

    def solve_triangular(self, b, lower: bool = True, unit_diagonal: bool = False, device: int = 0,
                         sweeps=None) -> np.ndarray:
        """x with L x = b (the lower triangle of self, `lower`) or U x = b; entries of the other triangle are ignored
        and `unit_diagonal` takes the diagonal as ones.  Forward / backward substitution on the device, bit for bit
        the sequential loop (spal_*_trsv_*).  The reference has no solve; a Rust binding adds it as a
        method of the matrix types.
        `sweeps` = None is that exact solve; an integer s >= 0 asks for s Jacobi passes on the triangle instead
        (spal_*_trsv_sweep_*): approximate, every pass one launch, exact from s = levels - 1 on.
        A block of right-hand sides goes to solve_triangular_block."""
        b = np.asarray(b)
        if self._nrows != self._ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"solve_triangular: the matrix is not square ({self._nrows} x {self._ncols})")
        if b.ndim != 1 or b.shape[0] != self._nrows:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"solve_triangular: b has shape {b.shape} but the matrix has {self._nrows} rows")
        if sweeps is not None:
            return self.device(device).trsv_sweep(b, int(sweeps), lower, unit_diagonal)
        return self.device(device).trsv(b, lower, unit_diagonal)

    def solve_triangular_block(self, B, lower: bool = True, unit_diagonal: bool = False, device: int = 0,
                               sweeps=None) -> np.ndarray:
        """X with L X = B / U X = B for a block of right-hand sides B of shape (n, k): column j of the result is bit for
        bit solve_triangular's result for B[:, j], and the k columns share one solve's launches (spal_*_trsm_*,
        DESIGN 3.20).  `sweeps` = None is the exact solve, an integer s >= 0 that many Jacobi passes per column
        (spal_*_trsm_sweep_*).  solve_triangular itself keeps taking one 1-D right-hand side and refusing everything
        else.  A matrix that is not square, a B that is not 2-D or has another first dimension than n is refused before
        any device copy is made."""
        B = np.asarray(B)
        if self._nrows != self._ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"solve_triangular_block: the matrix is not square ({self._nrows} x {self._ncols})")
        if B.ndim != 2 or B.shape[0] != self._nrows:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"solve_triangular_block: B has shape {B.shape} but the matrix has {self._nrows} rows")
        if sweeps is not None:
            return self.device(device).trsm_sweep(B, int(sweeps), lower, unit_diagonal)
        return self.device(device).trsm(B, lower, unit_diagonal)

    def solve(self, b, method="cg", M=None, x0=None, tol: float = 1e-8, maxit: int = 1000, device: int = 0,
              precond_sweeps=None):
        """x with A x = b by CG (`method="cg"`: A symmetric positive definite) or BiCGStab ("bicgstab") on the device,
        optionally preconditioned by `M = a.ilu0()`; returns (x, info) with info.iterations, info.reason (0 converged to
        dot(r, r) <= tol^2 dot(b, b), 1 maxit reached, 2 breakdown), info.residual_sq, info.rhs_sq, info.solve_ms.
        Bit for bit the loops of include/spal.h.  The reference has no solver; a Rust binding adds it as a
        method of the matrix types.
        `precond_sweeps`, when given, SETS M's option "trsv_sweeps" before the call, and the option stays set on M's
        device handle: s >= 0 applies M by s Jacobi sweeps per triangle instead of two exact solves (3 is a good
        start; `M=self, precond_sweeps=0` is the Jacobi preconditioner), -1 restores the exact solves."""
        b = np.asarray(b)
        if self._nrows != self._ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"solve: the matrix is not square ({self._nrows} x {self._ncols})")
        if b.ndim != 1 or b.shape[0] != self._nrows:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"solve: b has shape {b.shape} but the matrix has {self._nrows} rows")
        if x0 is not None and np.shape(x0) != b.shape:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"solve: x0 has shape {np.shape(x0)} but b {b.shape}")
        if isinstance(M, Amg):   # M^-1 v = one multigrid cycle: `M = a.amg()`
            if precond_sweeps is not None:
                raise TypeError("precond_sweeps is an option of an ILU(0) factor: an Amg has no triangular sweeps")
            return self.device(device).krylov(b, method, M, x0, tol, maxit)
        if isinstance(M, Fsai):   # M^-1 v = Gt (G v), two SpMVs: `M = a.fsai()`
            if precond_sweeps is not None:
                raise TypeError("precond_sweeps is an option of an ILU(0) factor: an Fsai has no triangular sweeps")
            return self.device(device).krylov(b, method, M, x0, tol, maxit)
        if M is not None and type(M) is not type(self):
            raise TypeError(f"M must be a {type(self).__name__}, e.g. self.ilu0()")
        if precond_sweeps is not None:
            if M is None:
                raise TypeError("precond_sweeps needs M, the factor it is an option of")
            M.device(device).set_option("trsv_sweeps", int(precond_sweeps))
        return self.device(device).krylov(b, method, None if M is None else M.device(device), x0, tol, maxit)

    def solve_block(self, B, method="cg", M=None, X0=None, tol: float = 1e-8, maxit: int = 1000, device: int = 0,
                    precond_sweeps=None):
        """X with A X = B for a block of right-hand sides B of shape (n, k): k independent CG / BiCGStab iterations run
        in lockstep, one pass over the matrix per product and one walk of M's launches per solve for all k columns
        (spal_*_krylov_block_*).  Returns (X, infos), infos a list of k records as solve() returns one;
        column j of X and infos[j] are bit for bit the loop of include/spal.h on B[:, j], whatever k, the other
        columns or the options are.  `M` and `precond_sweeps` as in solve(), which keeps taking one 1-D right-hand
        side.  A matrix that is not square, a B that is not 2-D or has another first dimension than n and an X0 of
        another shape than B are refused before any device copy is made."""
        _refuse_amg(M, "solve_block()")
        B = np.asarray(B)
        if self._nrows != self._ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"solve_block: the matrix is not square ({self._nrows} x {self._ncols})")
        if B.ndim != 2 or B.shape[0] != self._nrows:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"solve_block: B has shape {B.shape} but the matrix has {self._nrows} rows")
        if X0 is not None and np.shape(X0) != B.shape:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"solve_block: X0 has shape {np.shape(X0)} but B {B.shape}")
        if M is not None and type(M) is not type(self):
            raise TypeError(f"M must be a {type(self).__name__}, e.g. self.ilu0()")
        if precond_sweeps is not None:
            if M is None:
                raise TypeError("precond_sweeps needs M, the factor it is an option of")
            M.device(device).set_option("trsv_sweeps", int(precond_sweeps))
        return self.device(device).krylov_block(B, method, None if M is None else M.device(device), X0, tol, maxit)

    def _minres_args(self, who, M, shift, precond_sweeps, device):
        """What minres() and minres_block() refuse alike before any device copy is made; returns M's device handle."""
        _refuse_amg(M, f"{who}()")
        if self._nrows != self._ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"{who}: the matrix is not square ({self._nrows} x {self._ncols})")
        if not np.isfinite(float(shift)):
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"{who}: shift = {float(shift)} must be finite")
        if isinstance(M, Fsai):   # (minres() only: minres_block() has refused it above)
            if precond_sweeps is not None:
                raise TypeError("precond_sweeps is an option of an ILU(0) factor: an Fsai has no triangular sweeps")
            return M
        if M is not None and type(M) is not type(self):
            raise TypeError(f"M must be a {type(self).__name__}, e.g. self.ilu0()")
        if precond_sweeps is not None:
            if M is None:
                raise TypeError("precond_sweeps needs M, the factor it is an option of")
            M.device(device).set_option("trsv_sweeps", int(precond_sweeps))
        return None if M is None else M.device(device)

    def minres(self, b, M=None, shift: float = 0.0, x0=None, tol: float = 1e-8, maxit: int = 1000, device: int = 0,
               precond_sweeps=None):
        """x with (A - shift I) x = b by MINRES on the device, for a SYMMETRIC matrix that may be indefinite (a saddle
        point, or A - shift I with the shift inside the spectrum), where CG does not apply; symmetry is not checked.
        `M`, when given, must be symmetric positive definite; `precond_sweeps` as in solve() (`M=D, precond_sweeps=0`
        with D a diagonal matrix of |a_ii| is the Jacobi preconditioner).  Returns (x, info) as solve() does, with
        info.residual_sq the recurrence's estimate of the squared residual norm, which never grows: reason 1 at maxit
        still returns the best iterate.  Bit for bit the text of include/spal.h."""
        b = np.asarray(b)
        m = self._minres_args("minres", M, shift, precond_sweeps, device)
        if b.ndim != 1 or b.shape[0] != self._nrows:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"minres: b has shape {b.shape} but the matrix has {self._nrows} rows")
        if x0 is not None and np.shape(x0) != b.shape:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"minres: x0 has shape {np.shape(x0)} but b {b.shape}")
        return self.device(device).minres(b, m, float(shift), x0, tol, maxit)

    def minres_block(self, B, M=None, shift: float = 0.0, X0=None, tol: float = 1e-8, maxit: int = 1000, device: int = 0,
                     precond_sweeps=None):
        """X with (A - shift I) X = B for a block of right-hand sides B of shape (n, k): k independent MINRES iterations
        in lockstep, one pass over the matrix per product for all k columns (spal_*_minres_block_*).
        Returns (X, infos) like solve_block(); column j of X and infos[j] are bit for bit the text of include/spal.h on
        B[:, j], whatever k, the other columns or the options are.  `M`, `shift` and `precond_sweeps` as in minres()."""
        B = np.asarray(B)
        m = self._minres_args("minres_block", M, shift, precond_sweeps, device)
        if B.ndim != 2 or B.shape[0] != self._nrows:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"minres_block: B has shape {B.shape} but the matrix has {self._nrows} rows")
        if X0 is not None and np.shape(X0) != B.shape:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"minres_block: X0 has shape {np.shape(X0)} but B {B.shape}")
        return self.device(device).minres_block(B, m, float(shift), X0, tol, maxit)

    def gmres(self, b, M=None, x0=None, restart: int = 30, tol: float = 1e-8, maxit: int = 1000, device: int = 0,
              precond_sweeps=None):
        """x with A x = b by restarted GMRES(restart) on the device, for matrices that are not symmetric (BiCGStab, the
        other solver for them, can break down); right-preconditioned by `M = a.ilu0()`, with `precond_sweeps` as in
        solve().  Returns (x, info) as solve() does: reasons 0 and 1 are decided on the true residual, recomputed at
        the head of every cycle.  restart is 1 .. 256; the call holds restart + 1 basis vectors on the device.  Bit for
        bit the text of include/spal.h."""
        _refuse_amg(M, "gmres()")
        b = np.asarray(b)
        if self._nrows != self._ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"gmres: the matrix is not square ({self._nrows} x {self._ncols})")
        if b.ndim != 1 or b.shape[0] != self._nrows:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"gmres: b has shape {b.shape} but the matrix has {self._nrows} rows")
        if x0 is not None and np.shape(x0) != b.shape:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"gmres: x0 has shape {np.shape(x0)} but b {b.shape}")
        if not 1 <= int(restart) <= 256:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"gmres: restart = {int(restart)} must be 1 .. 256 (one Hessenberg "
                        "column element per thread of the scalar workgroup)")
        if M is not None and type(M) is not type(self):
            raise TypeError(f"M must be a {type(self).__name__}, e.g. self.ilu0()")
        if precond_sweeps is not None:
            if M is None:
                raise TypeError("precond_sweeps needs M, the factor it is an option of")
            M.device(device).set_option("trsv_sweeps", int(precond_sweeps))
        return self.device(device).gmres(b, None if M is None else M.device(device), x0, int(restart), tol, maxit)

    def cheb_apply(self, x, degree: int, lo: float, hi: float, a0: float, device: int = 0) -> np.ndarray:
        """p(A) x for the Chebyshev polynomial of `degree` that is small on [lo, hi] and 1 at a0, which lies outside the
        interval: the text of include/spal.h bit for bit.  Refused before anything is copied to a device:
        a degree outside 1 .. 256, values that are not finite, lo >= hi, a0 inside [lo, hi], a matrix that is not
        square, an x of another length."""
        degree, lo, hi, a0 = int(degree), float(lo), float(hi), float(a0)
        if not 1 <= degree <= 256:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"cheb_apply: degree = {degree} must be 1 .. 256")
        if not (np.isfinite(lo) and np.isfinite(hi) and np.isfinite(a0)):
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, "cheb_apply: lo, hi and a0 must be finite")
        if not lo < hi:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"cheb_apply: lo = {lo} must be less than hi = {hi}")
        if lo <= a0 <= hi:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"cheb_apply: a0 = {a0} must lie outside [{lo}, {hi}]")
        if self._nrows != self._ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"cheb_apply: the matrix is not square ({self._nrows} x {self._ncols})")
        if np.shape(x) != (self._nrows,):
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"cheb_apply: x has shape {np.shape(x)} but the matrix has {self._nrows} rows")
        return self.device(device).cheb_apply(x, degree, lo, hi, a0)

    def cheb_series(self, x, coef, lo: float, hi: float, device: int = 0) -> np.ndarray:
        """sum_i coef[i] T_i(B) x with B = A mapped from [lo, hi] onto [-1, 1] and T_i the unscaled Chebyshev polynomials
        (DESIGN 3.28): the text of include/spal.h bit for bit.  coef holds degree + 1 doubles, degree 1 .. 4096
        (cheb_delta_coefficients() gives the delta filter's); [lo, hi] must enclose the spectrum.  Refused before
        anything is copied to a device: a bad degree, values that are not finite, lo >= hi, a matrix that is not square,
        an x of another length."""
        coef, _, lo, hi = _series_args(coef, lo, hi)
        if self._nrows != self._ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"cheb_series: the matrix is not square ({self._nrows} x {self._ncols})")
        if np.shape(x) != (self._nrows,):
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"cheb_series: x has shape {np.shape(x)} but the matrix has {self._nrows} rows")
        return self.device(device).cheb_series(x, coef, lo, hi)

    def kpm_moments(self, degree: int, probes: int = 8, seed: int = 0, interval=None, Z=None, device: int = 0):
        """(mu, info): the Chebyshev moments of `probes` probe columns, mu of shape (degree + 1, probes) in float64
        (DESIGN 3.29): the text of include/spal.h bit for bit.  The matrix must be symmetric (not checked).  Z = None:
        hashed +-1 probes from `seed` (kpm_probes); interval = None: Gershgorin's bounds with a margin, else (lo, hi)
        enclosing the spectrum.  kpm_density and kpm_count turn the moments into the spectral density and into the
        number of eigenvalues in an interval.  Refused before anything is copied to a device: a degree outside
        1 .. 4096, probes outside 1 .. 256, an interval that is not finite or is empty, a matrix that is not square,
        a Z of another shape."""
        k = probes if Z is None else (np.shape(Z)[1] if np.ndim(Z) == 2 else -1)
        if Z is not None and (np.ndim(Z) != 2 or np.shape(Z)[0] != self._nrows):
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"kpm_moments: Z has shape {np.shape(Z)} but the matrix has {self._nrows} rows")
        _kpm_args("kpm_moments", degree, k, interval)
        if self._nrows != self._ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"kpm_moments: the matrix is not square ({self._nrows} x {self._ncols})")
        return self.device(device).kpm_moments(degree, probes, seed, interval, Z)

    def eig_count(self, a: float, b: float, degree: int = 128, probes: int = 32, seed: int = 0, interval=None,
                  damping="jackson", device: int = 0):
        """(estimate, standard_error) of the number of eigenvalues of this symmetric matrix in [a, b]: kpm_count of
        kpm_moments(degree, probes, seed, interval).  The resolution is about pi (hi - lo) / (2 degree)."""
        mu, info = self.kpm_moments(degree, probes, seed, interval, device=device)
        return kpm_count(mu, info.lo, info.hi, a, b, damping)

    def spectral_density(self, points, degree: int = 128, probes: int = 32, seed: int = 0, interval=None,
                         damping="jackson", device: int = 0) -> np.ndarray:
        """The spectral density at `points`, normalised to integrate to n: kpm_density of kpm_moments(...)."""
        mu, info = self.kpm_moments(degree, probes, seed, interval, device=device)
        return kpm_density(mu, info.lo, info.hi, points, damping)

    def gershgorin(self, device: int = 0):
        """(glo, ghi): Gershgorin's enclosure of the spectrum, in double, computed on the device."""
        if self._nrows != self._ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"gershgorin: the matrix is not square ({self._nrows} x {self._ncols})")
        return self.device(device).gershgorin()

    def eigsh(self, k: int = 6, which="LA", ncv=None, v0=None, seed: int = 0, tol: float = 0, maxit: int = 1000,
              return_eigenvectors: bool = True, device: int = 0, filter_degree: int = 0, filter_interval=None,
              filter_warmup: int = 5, sigma=None):
        """theta, X, info = a.eigsh(k): the k largest (which="LA") or smallest ("SA") eigenvalues of this SYMMETRIC
        matrix and their vectors, by thick-restart Lanczos with full orthogonalisation on the device;
        symmetry is not checked, as with CG.  theta comes in the order of `which`, X has shape (n, k) (None with
        return_eigenvectors=False), info is an EigshInfo (restarts, products, converged, reason, resid, solve_ms).
        ncv=None means min(n, max(2k + 1, 20)) basis vectors, at most 256; tol=0 means the dtype's machine epsilon, as
        scipy does; maxit bounds the restarts.  An eigenvalue of multiplicity > 1 is returned ONCE (a single-vector
        Lanczos iteration sees one direction of its eigenspace).  Refused on a matrix that is not square or has fewer
        than ncv rows before anything is copied to a device.  Bit for bit the text of include/spal.h.
        CLUSTERED extreme eigenvalues: filter_degree > 0 runs the iteration on a Chebyshev polynomial of A of that degree
        (DESIGN 3.26), which needs many times fewer restarts; filter_interval=None finds the interval to damp with
        filter_warmup plain restarts, (lo, hi) gives it.  Convergence is then decided on true residuals against
        tol * max(|glo|, |ghi|) of Gershgorin's bounds, and tol=0 means 256 machine epsilons.
        INTERIOR eigenvalues: sigma=s returns the k eigenvalues nearest s by Lanczos on a Chebyshev delta filter at s
        (DESIGN 3.28).  There is no shift-invert: filter_degree >= 2 is required (it sets the resolution: the filter
        separates eigenvalues about (hi - lo) / degree apart) and which="SA" raises ValueError.  filter_interval=None is
        Gershgorin's interval with a margin; a given (lo, hi) must enclose the spectrum and hold s strictly inside;
        filter_warmup is ignored.  The pairs come in DESCENDING ORDER OF THE FILTER VALUE -- near s that is ascending
        distance from s -- and are not re-sorted; convergence is on true residuals.  THE TWO-TO-ONE LIMITATION: two
        eigenvalues with the same filter value (mirror images in a spectrum symmetric about s, such as the 1-D
        Laplacian's about 2) cannot be separated by a single-vector iteration; the call ends with reason 1 and
        residuals that do not fall.  Move s off the centre of symmetry."""
        if sigma is not None:
            _near_args(sigma, which, filter_degree, filter_interval)
        _eigsh_args(self._nrows, self._ncols, k, ncv, tol, self.dtype)
        _eigsh_which(which)
        if v0 is not None and np.shape(v0) != (self._nrows,):
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"eigsh: v0 has shape {np.shape(v0)} but the matrix has {self._nrows} rows")
        if filter_degree and sigma is None:
            _filter_args(filter_degree, filter_interval, filter_warmup)
        return self.device(device).eigsh(k, which, ncv, v0, seed, tol, maxit, return_eigenvectors, filter_degree,
                                         filter_interval, filter_warmup, sigma)

    def gmres_block(self, B, M=None, X0=None, restart: int = 30, tol: float = 1e-8, maxit: int = 1000, device: int = 0,
                    precond_sweeps=None):
        """X with A X = B for a block of right-hand sides B of shape (n, k) by restarted GMRES(restart): k independent
        iterations in lockstep, one pass over the matrix per product and one walk of M's launches per solve for all k
        columns; cycles are common to the block (spal_*_gmres_block_*).  Returns (X, infos) like
        solve_block(); column j of X and infos[j] are bit for bit the GMRES text of include/spal.h on B[:, j], whatever
        k, the other columns or the options are.  `M`, `restart` and `precond_sweeps` as in gmres().  A matrix that is
        not square, a B that is not 2-D or has another first dimension than n, an X0 of another shape than B and a
        restart outside 1 .. 256 are refused before any device copy is made."""
        _refuse_amg(M, "gmres_block()")
        B = np.asarray(B)
        if self._nrows != self._ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"gmres_block: the matrix is not square ({self._nrows} x {self._ncols})")
        if B.ndim != 2 or B.shape[0] != self._nrows:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"gmres_block: B has shape {B.shape} but the matrix has {self._nrows} rows")
        if X0 is not None and np.shape(X0) != B.shape:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"gmres_block: X0 has shape {np.shape(X0)} but B {B.shape}")
        if not 1 <= int(restart) <= 256:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"gmres_block: restart = {int(restart)} must be 1 .. 256 (one "
                        "Hessenberg column element per thread of the scalar workgroup)")
        if M is not None and type(M) is not type(self):
            raise TypeError(f"M must be a {type(self).__name__}, e.g. self.ilu0()")
        if precond_sweeps is not None:
            if M is None:
                raise TypeError("precond_sweeps needs M, the factor it is an option of")
            M.device(device).set_option("trsv_sweeps", int(precond_sweeps))
        return self.device(device).gmres_block(B, None if M is None else M.device(device), X0, int(restart), tol, maxit)

    def _mul_mat(self, other, device: int = 0):
        """`&self * &other` (src/csr/ops/mul.rs:5-59 / src/csc/ops/mul.rs:5-60) on the device; the result is downloaded
        and keeps its device handle, as from_coo does."""
        if type(other) is not type(self):
            raise TypeError(f"{type(self).__name__} * {type(other).__name__}: the reference has no mixed Mul")
        if self._ncols != other._nrows:
            # assert_eq!(self.ncols(), rhs.nrows())  mul.rs:9
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"assertion failed: ncols == rhs.nrows (left: {self._ncols}, right: {other._nrows})")
        dev = self.device(device).mul(other.device(device))
        ptr, ind, val = dev.download()
        out = type(self)._trusted(self._nrows, other._ncols, ptr, ind, val)
        out._dev[device] = dev
        return out

    def __mul__(self, x):
        if isinstance(x, _Compressed):
            return self._mul_mat(x)
        return self._mul_vec(x)

    __matmul__ = __mul__

    def _add_sub(self, op: str, other, device: int = 0):
        """`&self + &other` / `&self - &other` (src/csr/ops/{add,sub}.rs:5-75, src/csc/ops/...) on the device; the result
        is downloaded and keeps its device handle, as `_mul_mat`'s does."""
        if not isinstance(other, _Compressed):
            return NotImplemented
        sign = "+" if op == "add" else "-"
        if type(other) is not type(self):
            raise TypeError(f"{type(self).__name__} {sign} {type(other).__name__}: the reference has no mixed {op.title()}")
        # assert_eq!(self.nrows(), rhs.nrows()); assert_eq!(self.ncols(), rhs.ncols())  add.rs:9-10, sub.rs:9-10
        if self._nrows != other._nrows:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"assertion failed: nrows == rhs.nrows (left: {self._nrows}, right: {other._nrows})")
        if self._ncols != other._ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT,
                        f"assertion failed: ncols == rhs.ncols (left: {self._ncols}, right: {other._ncols})")
        dev = getattr(self.device(device), op)(other.device(device))
        return self._adopt_result(dev, device)

    def _adopt_result(self, dev, device: int):
        ptr, ind, val = dev.download()
        out = type(self)._trusted(self._nrows, self._ncols, ptr, ind, val)
        out._dev[device] = dev
        return out

    def __add__(self, other):
        return self._add_sub("add", other)

    def __sub__(self, other):
        return self._add_sub("sub", other)

    def __neg__(self):
        """`-&self` (src/csr/ops/neg.rs:5-17 / src/csc/ops/neg.rs:5-17) on the device."""
        return self._adopt_result(self.device().neg(), 0)

    def ilu0(self, device: int = 0, sweeps=None):
        """The ILU(0) factor of this square matrix, a matrix of the same class and structure (spal_*_ilu0, DESIGN
        3.12): L strictly below the diagonal with its unit diagonal implied, U on and above it, bit for bit the
        sequential loop without fill.  Every row must store its diagonal.  The result is downloaded and keeps its
        device handle, which already has its lower solve plan.  Applying the preconditioner is two solves::

            f = a.ilu0()
            y = f.solve_triangular(r, lower=True, unit_diagonal=True)      # L y = r
            z = f.solve_triangular(y, lower=False)                         # U z = y

        `sweeps` = None is that exact factorisation, which analyses the matrix and walks its levels; an integer
        s >= 0 builds the factor by s row sweeps instead (spal_*_ilu0_sweep): no analysis, one
        SpMV-shaped launch per pass, the exact factor's bits from s = levels - 1 on and a preconditioner well before.
        Such a factor has no solve plan and is meant to be applied by sweeps, SpMV-shaped from start to finish::

            f = a.ilu0(sweeps=3)
            x, info = a.solve(b, M=f, precond_sweeps=3)
        """
        if sweeps is not None:
            sweeps = _sweep_count(sweeps)              # refused before anything is uploaded
        return self._adopt_result(self.device(device).ilu0(sweeps=sweeps), device)

    def amg(self, seed: int = 0, max_levels: int = 16, coarse_rows: int = 64, nu: int = 2, coarse_sweeps: int = 16,
            cycle: str = "v", omega: float = 2.0 / 3.0, alpha: float = 1.0, device: int = 0) -> Amg:
        """The aggregation AMG hierarchy of this square matrix, an :class:`Amg` (spal_*_amg_setup):
        unsmoothed aggregation by hashed priority with the degree first, Galerkin coarse matrices through the COO
        assembly, a V (`cycle="v"`) or W cycle with `nu` damped Jacobi sweeps (weight `omega`) before and after,
        `coarse_sweeps` on the coarsest level, the coarse correction scaled by `alpha`.  Every row must store its
        diagonal.  Its iteration counts grow slowly with the problem size where ILU(0)'s and Jacobi's do not::

            g = a.amg(cycle="w", alpha=1.5)
            x, info = a.solve(b, M=g)
        """
        self._square("amg")
        _amg_params(seed, max_levels, coarse_rows, nu, coarse_sweeps, cycle, omega, alpha)   # refused before any upload
        return self.device(device).amg(seed, max_levels, coarse_rows, nu, coarse_sweeps, cycle, omega, alpha)

    def fsai(self, pattern=None, max_row=None, device: int = 0) -> Fsai:
        """The factorised sparse approximate inverse of this square, symmetric positive definite matrix, an
        :class:`Fsai` (spal_*_fsai_setup): G ~ L^-1 on the lower triangle of `pattern`'s structure (a
        matrix of this class and shape, None: this matrix's own), M^-1 = Gt G, symmetric positive definite by
        construction and applied by two SpMVs.  Every row of the pattern must store its diagonal; `max_row` (1 .. 64,
        default 32) caps a row's local system.  A denser pattern buys iterations with the library's own product::

            f = a.fsai(pattern=a @ a)
            x, info = a.solve(b, M=f)
            x, info = a.minres(b, M=f, shift=0.5)
        """
        self._square("fsai")
        if pattern is not None and type(pattern) is not type(self):
            raise TypeError(f"pattern must be a {type(self).__name__} (a matrix of the same format)")
        if pattern is not None and (pattern._nrows, pattern._ncols) != (self._nrows, self._ncols):
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"fsai: the pattern is {pattern._nrows} x {pattern._ncols} but the "
                                                        f"matrix {self._nrows} x {self._ncols}")
        if max_row is not None and not 1 <= int(max_row) <= 64:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"fsai: max_row = {int(max_row)} must be 1 .. 64")
        return self.device(device).fsai(None if pattern is None else pattern.device(device), max_row)

    def _square(self, what: str) -> None:
        if self._nrows != self._ncols:
            raise Panic(_ffi.SPAL_ERR_INVALID_ARGUMENT, f"{what}: the matrix is not square ({self._nrows} x {self._ncols})")

    def colour(self, seed: int = 0, device: int = 0):
        """(colours, ncolours): the greedy colouring of the graph of A + A^T by hashed priority, as written out in
        include/spal.h, computed on the device (spal_*_colour)."""
        self._square("colour")
        colours, ncolours, _ = self.device(device).colour(seed)
        return colours, ncolours

    def _adopt_ordered(self, dev, device: int):
        out = self._adopt_result(dev, device)
        out.perm, out.ncolours = dev.ordering()
        return out

    def permute(self, perm, device: int = 0):
        """P A P^T for any permutation `perm` (new -> old): a matrix of the same class, its values A's bits.  The result
        keeps its device handle and has `perm`, `ncolours` = 0, to_order() and from_order()."""
        self._square("permute")
        return self._adopt_ordered(self.device(device).permute(perm), device)

    def multicolour(self, seed: int = 0, device: int = 0):
        """The matrix in multicolour order: rows numbered colour by colour, so that both triangles -- and those of its
        ILU(0) factor -- have at most `ncolours` levels and an exact triangular solve is a few wide launches.  A matrix
        of the same class that keeps its device handle, with `perm` (new -> old), `ncolours`, to_order(), from_order()::

            p = a.multicolour(); f = p.ilu0()
            xp, info = p.solve(p.to_order(b), method="bicgstab", M=f); x = p.from_order(xp)

        ILU(0) in this order is usually a weaker preconditioner than in the natural one (more iterations), and the
        permuted matrix has lost its band."""
        self._square("multicolour")
        return self._adopt_ordered(self.device(device).multicolour(seed), device)

    def _perm(self) -> np.ndarray:
        perm = getattr(self, "perm", None)
        if perm is None:
            raise TypeError("this matrix has no ordering: it is no result of permute() or multicolour()")
        return perm.astype(np.int64)

    def to_order(self, v) -> np.ndarray:
        """v[perm]: a vector of the original numbering in this matrix's order."""
        return np.asarray(v)[self._perm()]

    def from_order(self, vp_) -> np.ndarray:
        """The inverse of to_order()."""
        vp_ = np.asarray(vp_)
        out = np.empty_like(vp_)
        out[self._perm()] = vp_
        return out


class CsrMatrix(_Compressed):
    """Compressed sparse row matrix (reference src/csr.rs:66-72)."""
    _kind = "csr"
    _dev_cls = DeviceCsr

    @classmethod
    def new(cls, nrows, ncols, rowptr, colind, values):
        return cls(nrows, ncols, rowptr, colind, values)

    @classmethod
    def eye(cls, size: int, dtype=np.float64):
        """src/csr.rs:179-189"""
        if not size > 0:
            raise Panic(_ffi.SPAL_ERR_INVARIANT, "assertion failed: size > 0")
        idx = np.arange(size + 1, dtype=np.uint64)
        return cls._trusted(size, size, idx, idx[:-1].copy(), np.ones(size, dtype=dtype))

    def rowptr(self) -> np.ndarray:
        return self._ptr

    def colind(self) -> np.ndarray:
        return self._ind

    def row_slice(self, row_begin: int, row_end: int) -> "CsrMatrix":
        """Rows [row_begin, row_end) as a CsrMatrix of their own (a row range of
        a valid CSR matrix is a valid CSR matrix after rebasing rowptr):
        the per-GPU shard of the row-partitioned product."""
        a0, a1 = int(self._ptr[row_begin]), int(self._ptr[row_end])
        return CsrMatrix._trusted(row_end - row_begin, self._ncols,
                                  self._ptr[row_begin:row_end + 1] - np.uint64(a0),
                                  self._ind[a0:a1], self._values[a0:a1])

    @classmethod
    def from_coo(cls, coo: "CooMatrix", device: int = 0) -> "CsrMatrix":
        """`CsrMatrix::from(&coo)` (src/csr/conv/coo.rs:3-116) on the device."""
        dev = coo.assemble_csr(device)
        rp, ci, va = dev.download()
        out = cls._trusted(coo.nrows(), coo.ncols(), rp, ci, va)
        out._dev[device] = dev
        return out

    @classmethod
    def from_csc(cls, csc: "CscMatrix", device: int = 0) -> "CsrMatrix":
        """`CsrMatrix::from(&csc)` (src/csr/conv/csc.rs:4-52) on the device."""
        dev = csc.device(device).to_csr()
        rp, ci, va = dev.download()
        out = cls._trusted(csc.nrows(), csc.ncols(), rp, ci, va)
        out._dev[device] = dev
        return out

    @classmethod
    def from_(cls, other, device: int = 0):
        return cls.from_csc(other, device) if isinstance(other, CscMatrix) else cls.from_coo(other, device)


class CscMatrix(_Compressed):
    """Compressed sparse column matrix (reference src/csc.rs:66-72)."""
    _kind = "csc"
    _dev_cls = DeviceCsc

    @classmethod
    def new(cls, nrows, ncols, colptr, rowind, values):
        return cls(nrows, ncols, colptr, rowind, values)

    def colptr(self) -> np.ndarray:
        return self._ptr

    def rowind(self) -> np.ndarray:
        return self._ind

    @classmethod
    def from_coo(cls, coo: "CooMatrix", device: int = 0) -> "CscMatrix":
        """`CscMatrix::from(&coo)` (src/csc/conv/coo.rs:3-116) on the device."""
        d = coo.upload(device)
        dev = d.assemble_csc()
        d.close()
        cp, ri, va = dev.download()
        out = cls._trusted(coo.nrows(), coo.ncols(), cp, ri, va)
        out._dev[device] = dev
        return out

    @classmethod
    def from_csr(cls, csr: "CsrMatrix", device: int = 0) -> "CscMatrix":
        """`CscMatrix::from(&csr)` (src/csc/conv/csr.rs:4-52) on the device."""
        dev = csr.device(device).to_csc()
        cp, ri, va = dev.download()
        out = cls._trusted(csr.nrows(), csr.ncols(), cp, ri, va)
        out._dev[device] = dev
        return out

    @classmethod
    def from_(cls, csr, device: int = 0):
        return cls.from_csr(csr, device)


# --------------------------------------------------------------------------
# CooMatrix (host container; reference src/coo.rs:53-57)
# --------------------------------------------------------------------------
class CooMatrix:
    """Coordinate format: insertion order is significant (duplicates are
    summed in that order by the conversion)."""

    def __init__(self, nrows: int, ncols: int, dtype=np.float64):
        if not nrows > 0:
            raise Panic(_ffi.SPAL_ERR_INVARIANT, "assertion failed: nrows > 0")   # src/coo.rs:105
        if not ncols > 0:
            raise Panic(_ffi.SPAL_ERR_INVARIANT, "assertion failed: ncols > 0")   # src/coo.rs:106
        self._nrows, self._ncols = int(nrows), int(ncols)
        self._dtype = np.dtype(dtype)
        self._rows = np.empty(0, dtype=np.uint64)
        self._cols = np.empty(0, dtype=np.uint64)
        self._vals = np.empty(0, dtype=self._dtype)
        self._pending = []  # pushed one by one since the last flush

    @classmethod
    def new(cls, nrows, ncols, dtype=np.float64):
        return cls(nrows, ncols, dtype)

    @classmethod
    def with_capacity(cls, nrows, ncols, capacity, dtype=np.float64):
        return cls(nrows, ncols, dtype)

    @classmethod
    def with_triplets(cls, nrows, ncols, rowind, colind, values):
        """src/coo.rs:260-288"""
        dt = _scalar_dtype(values)
        self = cls(nrows, ncols, dt)
        rows, cols = _idx(rowind), _idx(colind)
        vals = np.ascontiguousarray(values, dtype=dt)
        if rows.size != vals.size:
            raise Panic(_ffi.SPAL_ERR_INVARIANT, "assertion failed: rowind.len() == values.len()")
        if cols.size != vals.size:
            raise Panic(_ffi.SPAL_ERR_INVARIANT, "assertion failed: colind.len() == values.len()")
        if rows.size and int(rows.max()) >= self._nrows:
            raise Panic(_ffi.SPAL_ERR_INDEX_OUT_OF_BOUNDS, "assertion failed: *row < nrows (row < nrows)")
        if cols.size and int(cols.max()) >= self._ncols:
            raise Panic(_ffi.SPAL_ERR_INDEX_OUT_OF_BOUNDS, "assertion failed: *col < ncols (col < ncols)")
        self._rows, self._cols, self._vals = rows, cols, vals
        return self

    @classmethod
    def with_entries(cls, nrows, ncols, entries, dtype=np.float64):
        """src/coo.rs:204-221"""
        entries = list(entries)
        return cls.with_triplets(nrows, ncols, [e[0] for e in entries], [e[1] for e in entries],
                                 np.array([e[2] for e in entries], dtype=dtype))

    def push(self, row: int, col: int, value) -> None:
        """src/coo.rs:431-435"""
        if not (0 <= row < self._nrows):
            raise Panic(_ffi.SPAL_ERR_INDEX_OUT_OF_BOUNDS, "assertion failed: row < self.nrows")
        if not (0 <= col < self._ncols):
            raise Panic(_ffi.SPAL_ERR_INDEX_OUT_OF_BOUNDS, "assertion failed: col < self.ncols")
        self._pending.append((row, col, value))

    def _flush(self):
        if self._pending:
            r, c, v = zip(*self._pending)
            self._rows = np.concatenate([self._rows, np.array(r, dtype=np.uint64)])
            self._cols = np.concatenate([self._cols, np.array(c, dtype=np.uint64)])
            self._vals = np.concatenate([self._vals, np.array(v, dtype=self._dtype)])
            self._pending = []

    def nrows(self) -> int:
        return self._nrows

    def ncols(self) -> int:
        return self._ncols

    def length(self) -> int:
        return self._rows.size + len(self._pending)

    @property
    def dtype(self):
        return self._dtype

    def triplets(self):
        """(rows, cols, values) in insertion order (what `iter()` yields,
        src/coo.rs:491-495, unzipped)."""
        self._flush()
        return self._rows, self._cols, self._vals

    def iter(self):
        r, c, v = self.triplets()
        return zip(r.tolist(), c.tolist(), v.tolist())

    def upload(self, device: int = 0) -> DeviceCoo:
        r, c, v = self.triplets()
        out = vp()
        check(getattr(_ffi.lib(), f"spal_coo_upload_{_sfx(self._dtype)}")(
            C.c_int(device), u64(self._nrows), u64(self._ncols), u64(v.size), _p(r), _p(c), _p(v),
            C.byref(out)))
        return DeviceCoo(out, self._dtype, device, self._nrows, self._ncols, v.size)

    def assemble_csr(self, device: int = 0) -> DeviceCsr:
        r, c, v = self.triplets()
        out = vp()
        check(getattr(_ffi.lib(), f"spal_coo_to_csr_{_sfx(self._dtype)}")(
            C.c_int(device), u64(self._nrows), u64(self._ncols), u64(v.size), _p(r), _p(c), _p(v),
            C.byref(out)))
        return DeviceCsr(out, self._dtype, device)
