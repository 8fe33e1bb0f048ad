"""Host tests of the Chebyshev series, the delta filter and eigsh near sigma: the coefficient function
against its numpy text bit for bit, the text's effectiveness on the 1-D Laplacian (the filter finds interior eigenvalues
that plain eigsh does not), the two-to-one limitation pinned, the names in the header, the library and the Rust binding,
and every refusal that needs no device.  No GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import cheb_ref as cr
from tests import eigsh_ref as er
from tests import near_ref as nr
from tests.test_eigsh_host import lib_jacobi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ([f"spal_{kind}_{what}_{form}{sfx}" for kind in ("csr", "csc") for what in ("cheb_series", "eigsh_near")
          for form in ("", "dev_") for sfx in ("f64", "f32")] + ["spal_cheb_delta_coefficients"])
u = C.c_uint64
d = C.c_double
EDGE = 1.0 - 2.0 ** -52


# ---- the coefficients ----------------------------------------------------------------------------------------------------

def lib_coefficients(degree, gamma, length=None):
    coef = np.full(degree + 1 if length is None else length, 7.0)
    st = _ffi.lib().spal_cheb_delta_coefficients(u(degree), d(gamma), coef.ctypes.data_as(_ffi.f64p), u(coef.size))
    return st, coef


@pytest.mark.parametrize("gamma", [0.0, 0.5, -0.5, EDGE, -EDGE])
@pytest.mark.parametrize("degree", [1, 2, 3, 64, 4096])
def test_the_library_coefficients_are_the_numpy_text_bit_for_bit(degree, gamma):
    st, coef = lib_coefficients(degree, gamma)
    want = nr.delta_coefficients(degree, gamma)
    assert st == 0 and want is not None and coef.tobytes() == want.tobytes()
    assert sp.cheb_delta_coefficients(degree, gamma).tobytes() == want.tobytes()
    # the series is 1 at gamma: sum_i coef_i T_i(gamma), T_i by the text's own recurrence
    m = [1.0, gamma]
    for i in range(2, degree + 1):
        m.append((2.0 * gamma) * m[i - 1] - m[i - 2])
    assert abs(float(np.dot(coef, np.array(m))) - 1.0) <= 1e-12


def test_the_filter_is_nonnegative_and_peaks_at_gamma():
    """Fejer's kernel: rho >= 0 on [-1, 1] (up to rounding) and rho(gamma) = 1 is its maximum."""
    t = np.linspace(-1.0, 1.0, 4001)
    for degree, gamma in ((8, 0.0), (64, 0.3), (64, -0.9), (256, 0.65)):
        rho = np.polynomial.chebyshev.chebval(t, nr.delta_coefficients(degree, gamma))
        assert rho.min() >= -1e-12 and rho.max() <= 1.0 + 1e-12
        assert abs(t[np.argmax(rho)] - gamma) <= 2.0 / 4000 + 1e-15


def test_the_coefficient_refusals():
    for degree, gamma in ((0, 0.0), (4097, 0.0), (5, 1.0), (5, -1.0), (5, 1.5), (5, np.nan), (5, np.inf)):
        st, coef = lib_coefficients(degree, gamma, length=max(degree, 0) + 1 if degree <= 4096 else 8)
        assert st == _ffi.SPAL_ERR_INVALID_ARGUMENT and np.all(coef == 7.0), (degree, gamma)
        assert nr.delta_coefficients(degree, gamma) is None
    for length in (5, 7):                                                  # coef_len != degree + 1
        st, coef = lib_coefficients(5, 0.1, length=length)
        assert st == _ffi.SPAL_ERR_INVALID_ARGUMENT and np.all(coef == 7.0)
    assert _ffi.lib().spal_cheb_delta_coefficients(u(5), d(0.1), None, u(6)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    with pytest.raises(sp.Panic):
        sp.cheb_delta_coefficients(5, 1.0)
    with pytest.raises(sp.Panic):
        sp.cheb_delta_coefficients(0, 0.0)


def test_the_series_text_is_the_chebyshev_sum():
    """On a diagonal matrix s[r] = sum_i coef_i T_i((a_r - c)/e); with coef = e_d it is the unscaled T_d."""
    lo, hi = -1.0, 3.0
    diag = np.linspace(lo, hi, 33)
    n = diag.size
    csr = (np.arange(n + 1), np.arange(n), diag.copy())
    rng = np.random.default_rng(3)
    for degree in (1, 2, 3, 17):
        coef = rng.standard_normal(degree + 1)
        s = nr.cheb_series(*csr, np.ones(n), lo, hi, coef)
        assert np.abs(s - np.polynomial.chebyshev.chebval((diag - 1.0) / 2.0, coef)).max() <= 1e-12
        unit = np.zeros(degree + 1)
        unit[degree] = 1.0
        s, t = nr.cheb_series(*csr, np.ones(n), lo, hi, unit, keep_t=True)
        assert s.tobytes() == (t + 0.0).tobytes() and np.abs(t).max() <= 1.0 + 1e-12


# ---- the text's effectiveness on the 1-D Laplacian ---------------------------------------------------------------------------
N, K, NCV, DEGREE = 400, 4, 20, 64
CASES = {"f64": (np.float64, 1e-10, 1e-9), "f32": (np.float32, 1e-5, 1e-5)}
LAMBDA = 2.0 - 2.0 * np.cos(np.arange(1, N + 1) * np.pi / (N + 1))        # the analytic spectrum


@functools.lru_cache(maxsize=None)
def laplacian(name):
    return cr.laplace_1d_csr(N, CASES[name][0])


def nearest(sigma, k=K):
    return LAMBDA[np.argsort(np.abs(LAMBDA - sigma), kind="stable")[:k]]


@functools.lru_cache(maxsize=None)
def near_run(name, sigma, maxit=60):
    dtype, tol, _ = CASES[name]
    return nr.eigsh_near(laplacian(name), dtype, K, sigma, NCV, tol, maxit, DEGREE, jacobi_fn=lib_jacobi)


@functools.lru_cache(maxsize=None)
def plain_run(name, which):
    dtype, tol, _ = CASES[name]
    csr = laplacian(name)
    return er.eigsh(lambda v: cr.rowsum(*csr, v), N, dtype, K, which, NCV, tol, 60, jacobi_fn=lib_jacobi)


@pytest.mark.parametrize("sigma", [1.0, 3.3])
@pytest.mark.parametrize("name", list(CASES))
def test_the_text_finds_the_eigenvalues_nearest_sigma(name, sigma):
    """Measured on the committed text at degree 64 (restarts / products): f64 sigma 1.0: 2 / 2316, 3.3: 2 / 2316;
    f32 sigma 1.0: 1 / 1800, 3.3: 1 / 1800."""
    dtype, tol, close = CASES[name]
    r = near_run(name, sigma)
    print(name, sigma, "restarts", r["restarts"], "products", r["products"], "theta", r["theta"])
    assert r["reason"] == 0 and r["converged"] == K and r["pairs"] == K
    want = nearest(sigma)
    got = np.sort(r["theta"].astype(np.float64))
    assert np.abs(got - np.sort(want)).max() <= close
    # and the filter is what finds them: plain eigsh with the same k, ncv and 60 restarts returns none of the four
    for which in ("LA", "SA"):
        p = plain_run(name, which)
        assert all(np.abs(want - t).min() > 1e-3 for t in p["theta"].astype(np.float64))
    # the automatic interval: Gershgorin's [0, 4] with its margin of 1/1024 of the width
    assert (r["lo"], r["hi"]) == (0.0 - 4.0 / 1024, 4.0 + 4.0 / 1024) and r["degree"] == DEGREE


@pytest.mark.parametrize("name", list(CASES))
def test_the_two_to_one_limitation_at_the_centre_of_a_symmetric_spectrum(name):
    """sigma = 2.0 is the exact centre of the 1-D Laplacian's spectrum: rho(lambda) = rho(4 - lambda), rho(A) has double
    eigenvalues and a single-vector Lanczos sees one mixed direction per pair.  Inherent in the method: pinned, not
    hidden.  resid is the true residual, so the call says so itself."""
    dtype, tol, _ = CASES[name]
    r = near_run(name, 2.0, maxit=10)
    assert r["reason"] == 1 and r["converged"] == 0 and r["restarts"] == 10 and r["pairs"] == K
    dense = 2.0 * np.eye(N) - np.eye(N, k=1) - np.eye(N, k=-1)
    x = r["X"].astype(np.float64)
    true = np.linalg.norm(dense @ x - x * r["theta"].astype(np.float64), axis=0)
    eps = float(np.finfo(dtype).eps)
    # the same residual, rounded in T: a row's three products and two sums, the Rayleigh quotient, then the norm's tree
    assert np.abs(true - r["resid"].astype(np.float64)).max() <= 64 * eps * 4.0
    assert true.min() > tol * 4.0                                                  # not one of them has converged


# ---- names ---------------------------------------------------------------------------------------------------------------------

def test_the_names_are_declared_exported_and_bound():
    declared = set(_ffi.exported_names())
    lib = _ffi.lib()
    ffi_rs = open(os.path.join(ROOT, "rust_shim", "src", "ffi.rs")).read()
    for name in NAMES:
        assert name in declared and hasattr(lib, name) and f"pub fn {name}(" in ffi_rs, name
    assert "pub struct spal_eigsh_near_info" in ffi_rs
    for cls in (sp.DeviceCsr, sp.DeviceCsc):
        assert all(hasattr(cls, m) for m in ("cheb_series", "cheb_series_dev"))
    for cls in (sp.CsrMatrix, sp.CscMatrix):
        assert hasattr(cls, "cheb_series")
    assert callable(sp.cheb_delta_coefficients)
    header = open(os.path.join(ROOT, "include", "spal.h")).read()
    assert "Rayleigh-Ritz on A in" in header and "automatic choice of the degree" in header


def test_the_info_struct_matches_the_header():
    from spalinalg_amd.matrix import _EigshNearInfoC
    assert [f[0] for f in _EigshNearInfoC._fields_] == ["restarts", "products", "converged", "reason", "solve_ms", "lo", "hi",
                                                        "sigma", "gamma", "degree"]
    assert C.sizeof(_EigshNearInfoC) == 80


# ---- the refusals that need no device --------------------------------------------------------------------------------------------

def laplace_host(n, dtype, kind="csr"):
    rp, ci, va = cr.laplace_1d_csr(n, dtype)
    return (sp.CsrMatrix if kind == "csr" else sp.CscMatrix)(n, n, rp, ci, va)


def test_python_refusals_come_before_a_device_is_touched(monkeypatch):
    a = laplace_host(30, np.float64)
    monkeypatch.setattr(type(a), "device", lambda self, device=0: pytest.fail("a device was touched"))
    good = np.ones(3)
    x = np.ones(30)
    for coef, lo, hi in ((np.ones(1), 0, 4), (np.ones(4098), 0, 4), (good, 4, 0), (good, 1, 1), (good, 0, np.inf),
                         (good, np.nan, 4), (np.array([1.0, np.nan, 0.0]), 0, 4), (np.array([1.0, np.inf]), 0, 4)):
        with pytest.raises(sp.Panic):
            a.cheb_series(x, coef, lo, hi)
    with pytest.raises(sp.Panic):
        a.cheb_series(np.ones(29), good, 0, 4)
    rect = sp.CsrMatrix(2, 3, np.array([0, 1, 2], np.uint64), np.array([0, 1], np.uint64), np.ones(2))
    monkeypatch.setattr(type(rect), "device", lambda self, device=0: pytest.fail("a device was touched"))
    with pytest.raises(sp.Panic):
        rect.cheb_series(np.ones(3), good, 0, 4)
    # eigsh(sigma=...): what scipy would serve by shift-invert is a ValueError that says so
    for kw in (dict(which="SA", filter_degree=64), dict(filter_degree=0), dict(filter_degree=1), dict()):
        with pytest.raises(ValueError, match="no shift-invert.*filter_degree"):
            a.eigsh(2, sigma=1.0, **kw)
    for kw in (dict(sigma=np.nan), dict(sigma=np.inf), dict(sigma=1.0, filter_degree=4097),
               dict(sigma=1.0, filter_interval=(4.0, 0.0)), dict(sigma=1.0, filter_interval=(0.0, np.inf)),
               dict(sigma=0.0, filter_interval=(0.0, 4.0)), dict(sigma=4.0, filter_interval=(0.0, 4.0)),
               dict(sigma=5.0, filter_interval=(0.0, 4.0)), dict(sigma=1.0, k=0), dict(sigma=1.0, k=4, ncv=4),
               dict(sigma=1.0, ncv=31), dict(sigma=1.0, tol=-1.0), dict(sigma=1.0, v0=np.ones(29))):
        kw = dict(dict(k=2, filter_degree=16), **kw)
        with pytest.raises(sp.Panic):
            a.eigsh(**kw)
    with pytest.raises(sp.Panic):
        rect.eigsh(1, sigma=1.0, filter_degree=16)


class FakeHandle(C.Structure):
    """Never dereferenced by the refusals below: they come before the handle is looked at."""
    _fields_ = [("pad", C.c_char * 64)]


@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("sfx,ct", [("f64", C.c_double), ("f32", C.c_float)])
def test_c_refusals_that_need_nothing_of_the_handle(kind, sfx, ct):
    lib = _ffi.lib()
    E = _ffi.SPAL_ERR_INVALID_ARGUMENT
    h = C.cast(C.pointer(FakeHandle()), C.c_void_p)
    x, out = (ct * 8)(), (ct * 8)()
    coef = (C.c_double * 4)(1.0, 0.5, 0.25, 0.125)
    series = getattr(lib, f"spal_{kind}_cheb_series_{sfx}")
    series_dev = getattr(lib, f"spal_{kind}_cheb_series_dev_{sfx}")
    bad_coef = (C.c_double * 4)(1.0, float("nan"), 0.0, 0.0)
    inf_coef = (C.c_double * 4)(1.0, 0.0, float("inf"), 0.0)
    for a_, x_, o_, deg, lo, hi, cf, cl in (
            (None, x, out, 3, 0.0, 4.0, coef, 4), (h, None, out, 3, 0.0, 4.0, coef, 4), (h, x, None, 3, 0.0, 4.0, coef, 4),
            (h, x, out, 3, 0.0, 4.0, None, 4), (h, x, out, 0, 0.0, 4.0, coef, 1), (h, x, out, 4097, 0.0, 4.0, coef, 4098),
            (h, x, out, 3, 0.0, 4.0, coef, 3), (h, x, out, 2, 0.0, 4.0, coef, 4), (h, x, out, 3, float("nan"), 4.0, coef, 4),
            (h, x, out, 3, 0.0, float("inf"), coef, 4), (h, x, out, 3, 4.0, 0.0, coef, 4), (h, x, out, 3, 1.0, 1.0, coef, 4),
            (h, x, out, 3, 0.0, 4.0, bad_coef, 4), (h, x, out, 3, 0.0, 4.0, inf_coef, 4)):
        assert series(a_, x_, u(8), o_, u(8), u(deg), d(lo), d(hi), cf, u(cl)) == E
        assert series_dev(a_, x_, o_, u(deg), d(lo), d(hi), cf, u(cl), None) == E
    near = getattr(lib, f"spal_{kind}_eigsh_near_{sfx}")
    near_dev = getattr(lib, f"spal_{kind}_eigsh_near_dev_{sfx}")
    from spalinalg_amd.matrix import _EigshNearInfoC
    info = _EigshNearInfoC()
    th, rs = (ct * 2)(), (ct * 2)()
    ok = dict(a=h, k=2, sigma=1.0, ncv=6, tol=0.0, degree=16, auto=1, lo=0.0, hi=0.0, th=th, rs=rs, ldx=2, info=C.byref(info))
    for change in (dict(a=None), dict(th=None), dict(rs=None), dict(info=None), dict(k=0), dict(ncv=2), dict(ncv=257),
                   dict(tol=-1.0), dict(tol=float("nan")), dict(degree=1), dict(degree=0), dict(degree=4097),
                   dict(sigma=float("nan")), dict(sigma=float("inf")), dict(auto=2), dict(auto=0, lo=0.0, hi=float("inf")),
                   dict(auto=0, lo=float("nan"), hi=4.0), dict(auto=0, lo=4.0, hi=0.0), dict(auto=0, lo=1.0, hi=4.0),
                   dict(auto=0, lo=0.0, hi=1.0), dict(auto=0, lo=2.0, hi=4.0), dict(ldx=1)):
        p = dict(ok, **change)
        xbuf = (ct * 64)()
        assert near(p["a"], u(p["k"]), d(p["sigma"]), u(p["ncv"]), None, u(0), u(0), d(p["tol"]), u(5), u(p["degree"]),
                    C.c_int(p["auto"]), d(p["lo"]), d(p["hi"]), p["th"], u(2), p["rs"], u(2), xbuf, u(p["ldx"]), u(8), p["info"]) == E, change
        assert near_dev(p["a"], u(p["k"]), d(p["sigma"]), u(p["ncv"]), None, u(0), d(p["tol"]), u(5), u(p["degree"]),
                        C.c_int(p["auto"]), d(p["lo"]), d(p["hi"]), p["th"], p["rs"], xbuf, u(p["ldx"]), None, p["info"]) == E, change
