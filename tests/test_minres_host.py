"""Host tests of the MINRES text (tests/minres_ref.py against numpy.linalg.solve), of its exits, and of every refusal of
the entry points that needs no device.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from spalinalg_amd._ffi import Panic
from tests import ilu_ref as ir
from tests import krylov_ref as kr
from tests import minres_ref as mr
from tests import trsv_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float64, np.float32]
TOL = {np.float64: 1e-10, np.float32: 1e-5}
NAMES = [f"spal_{kind}_minres_{form}{sfx}" for kind in ("csr", "csc") for form in ("", "dev_", "block_", "block_dev_")
         for sfx in ("f64", "f32")]


def dense_of(pattern, values):
    n, rowptr, colind = pattern
    dense = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))
    dense[rows, colind.astype(np.int64)] = values
    return dense


def small(name):
    rng = np.random.default_rng(5)
    if name == "banded":
        return ir.sym(tr.banded(300, 4, 40, rng))
    if name == "bidiagonal":
        return ir.sym(tr.bidiagonal(200))
    return tr.diagonal(65)


def test_indefinite_fill_is_symmetric_with_both_signs_and_a_gap():
    pattern = small("banded")
    values, _ = mr.indefinite_fill(pattern, np.float64, np.random.default_rng(2))
    dense = dense_of(pattern, values)
    assert np.array_equal(dense, dense.T)
    ev = np.linalg.eigvalsh(dense)
    assert ev.min() <= -1 and ev.max() >= 1 and np.abs(ev).min() >= 1
    assert np.abs(np.linalg.eigvalsh(dense - 0.25 * np.eye(pattern[0]))).min() >= 0.75
    spd, _ = kr.spd_fill(pattern, np.float64, np.random.default_rng(2))
    assert np.array_equal(np.abs(values), np.abs(spd))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("shift", [0.0, 0.25])
@pytest.mark.parametrize("name", ["banded", "bidiagonal", "diagonal"])
def test_the_text_solves_small_indefinite_systems(name, shift, jacobi, dtype):
    pattern = small(name)
    values, b = mr.indefinite_fill(pattern, dtype, np.random.default_rng(9))
    a = dense_of(pattern, values).astype(dtype)
    d = np.abs(np.diag(a)).copy()
    tol = TOL[dtype]
    x, info = mr.minres(lambda v: a @ v, (lambda v: v / d) if jacobi else None, b, np.zeros_like(b), shift, tol, 400)
    assert info["reason"] == 0 and 0 < info["iterations"] < 400 and x.dtype == dtype
    shifted = a.astype(np.float64) - shift * np.eye(pattern[0])
    exact = np.linalg.solve(shifted, b.astype(np.float64))
    assert np.linalg.norm(x - exact) <= 10 * tol * np.linalg.norm(exact) * np.linalg.cond(shifted)
    assert mr.true_relative_residual(pattern, values, shift, x, b) <= 2 * tol
    assert info["rhs_sq"] == float(kr.dot(b, (b / d) if jacobi else b))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_estimate_of_the_residual_never_grows(dtype):
    pattern = small("banded")
    values, b = mr.indefinite_fill(pattern, dtype, np.random.default_rng(9))
    a = dense_of(pattern, values).astype(dtype)
    last = np.inf
    for maxit in range(0, 12):
        _, info = mr.minres(lambda v: a @ v, None, b, np.zeros_like(b), 0.0, 0.0, maxit)
        assert info["reason"] == 1 and info["iterations"] == maxit and info["residual_sq"] <= last
        last = info["residual_sq"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_exits(dtype):
    pattern = small("banded")
    values, b = mr.indefinite_fill(pattern, dtype, np.random.default_rng(9))
    a = dense_of(pattern, values).astype(dtype)
    mul = lambda v: a @ v                                                                  # noqa: E731
    x0 = np.random.default_rng(4).uniform(-1, 1, size=b.size).astype(dtype)
    # M = -I: dot(r2, y) < 0, sqrt gives NaN -> reason 2 at it = 0, x is x0
    x, info = mr.minres(mul, lambda v: -v, b, x0, 0.0, 1e-6, 50)
    assert info["reason"] == 2 and info["iterations"] == 0 and x.tobytes() == x0.tobytes()
    assert np.isnan(info["residual_sq"]) and info["rhs_sq"] < 0
    # b = (A - shift I) x0 exactly representable: reason 0 at it = 0
    xi = np.round(x0 * 8).astype(dtype)
    ai = np.round(a * 4).astype(dtype)
    bi = (ai @ xi - dtype(0.25) * xi).astype(dtype)
    x, info = mr.minres(lambda v: ai @ v, None, bi, xi, 0.25, 1e-6, 50)
    assert info["reason"] == 0 and info["iterations"] == 0 and x.tobytes() == xi.tobytes() and info["residual_sq"] == 0
    # b = 0
    x, info = mr.minres(mul, None, np.zeros_like(b), np.zeros_like(b), 0.0, 1e-6, 50)
    assert info["reason"] == 0 and info["iterations"] == 0 and not x.any()
    # maxit = 0
    x, info = mr.minres(mul, None, b, x0, 0.0, 1e-6, 0)
    assert info["reason"] == 1 and info["iterations"] == 0 and x.tobytes() == x0.tobytes()
    # the zero matrix, and shift = d on d I: gamma = 0 -> NaN -> reason 2, no error
    x, info = mr.minres(lambda v: 0 * v, None, b, np.zeros_like(b), 0.0, 1e-6, 50)
    assert info["reason"] == 2 and info["iterations"] == 1
    x, info = mr.minres(lambda v: dtype(3) * v, None, b, np.zeros_like(b), 3.0, 1e-6, 50)
    assert info["reason"] == 2 and info["iterations"] == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_lucky_breakdown_stops_with_reason_0(dtype):
    # n = 1: the Krylov space is exhausted after one step, beta = 0, sn = 0, pp = 0
    x, info = mr.minres(lambda v: dtype(-4) * v, None, np.array([6], dtype=dtype), np.zeros(1, dtype=dtype), 0.0, 1e-6, 50)
    assert info["reason"] == 0 and info["iterations"] == 1 and x[0] == dtype(-1.5) and info["residual_sq"] == 0
    # a diagonal matrix of two distinct |d|, values that keep the arithmetic exact: two steps
    d = np.array([2, -4, 2, -4, 2, -4], dtype=dtype)
    b = np.array([1, 1, 1, 1, 1, 1], dtype=dtype)
    x, info = mr.minres(lambda v: d * v, None, b, np.zeros_like(b), 0.0, 1e-6, 50)
    assert info["reason"] == 0 and info["iterations"] == 2
    assert np.allclose(x, b / d, rtol=1e-6 if dtype == np.float32 else 1e-14)


def test_names_are_declared_exported_and_bound():
    declared = _ffi.exported_names()
    lib = _ffi.lib()
    with open(os.path.join(ROOT, "rust_shim", "src", "ffi.rs")) as f:
        rust = f.read()
    assert len(NAMES) == 16
    for name in NAMES:
        assert name in declared
        assert getattr(lib, name).restype is C.c_int
        assert f"pub fn {name}(" in rust
    with open(os.path.join(ROOT, "include", "spalinalg.hpp")) as f:
        hpp = f.read()
    assert hpp.count(" minres(") >= 2 and hpp.count(" minres_block(") >= 2
    for cls in (sp.CsrMatrix, sp.CscMatrix):
        assert callable(cls.minres) and callable(cls.minres_block)
    for cls in (sp.DeviceCsr, sp.DeviceCsc):
        assert callable(cls.minres) and callable(cls.minres_dev)
        assert callable(cls.minres_block) and callable(cls.minres_block_dev)


def test_entry_points_refuse_without_a_device():
    """null arguments come before any device call, in all sixteen entries"""
    lib = _ffi.lib()
    info = sp.matrix._KrylovInfoC()
    x = np.zeros(3)
    p = x.ctypes.data_as(_ffi.f64p)
    u, d = C.c_uint64, C.c_double
    bad = _ffi.SPAL_ERR_INVALID_ARGUMENT
    for kind in ("csr", "csc"):
        for sfx in ("f64", "f32"):
            assert getattr(lib, f"spal_{kind}_minres_{sfx}")(None, None, d(0.0), p, u(3), p, u(3), d(1e-8), u(5),
                                                             C.byref(info)) == bad
            assert f"spal_{kind}_minres: null argument".encode() in lib.spal_last_error()
            assert getattr(lib, f"spal_{kind}_minres_dev_{sfx}")(None, None, d(0.0), None, None, d(1e-8), u(5), None,
                                                                 C.byref(info)) == bad
            assert f"spal_{kind}_minres_dev: null argument".encode() in lib.spal_last_error()
            assert getattr(lib, f"spal_{kind}_minres_block_{sfx}")(None, None, d(0.0), u(2), p, u(2), u(3), p, u(2), u(3),
                                                                   d(1e-8), u(5), C.byref(info)) == bad
            assert f"spal_{kind}_minres_block: null argument".encode() in lib.spal_last_error()
            assert getattr(lib, f"spal_{kind}_minres_block_dev_{sfx}")(None, None, d(0.0), u(2), None, u(2), None, u(2),
                                                                       d(1e-8), u(5), None, C.byref(info)) == bad
            assert f"spal_{kind}_minres_block: null argument".encode() in lib.spal_last_error()


def test_the_python_layer_refuses_before_any_device_copy():
    n, rowptr, colind = tr.diagonal(4)
    a = sp.CsrMatrix(n, n, rowptr, colind, np.array([1.0, -2.0, 3.0, -4.0]))
    c = sp.CscMatrix(n, n, rowptr, colind, np.array([1.0, -2.0, 3.0, -4.0]))
    wide = sp.CsrMatrix(2, 3, np.array([0, 1, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint64), np.ones(2))
    b = np.ones(n)
    with pytest.raises(Panic, match="not square"):
        wide.minres(np.ones(2))
    with pytest.raises(Panic, match="not square"):
        wide.minres_block(np.ones((2, 2)))
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(Panic, match="shift"):
            a.minres(b, shift=bad)
        with pytest.raises(Panic, match="shift"):
            a.minres_block(np.ones((n, 2)), shift=bad)
    with pytest.raises(Panic, match="b has shape"):
        a.minres(np.ones(n + 1))
    with pytest.raises(Panic, match="b has shape"):
        a.minres(np.ones((n, 1)))
    with pytest.raises(Panic, match="x0 has shape"):
        a.minres(b, x0=np.ones(n + 1))
    with pytest.raises(Panic, match="B has shape"):
        a.minres_block(b)
    with pytest.raises(Panic, match="B has shape"):
        a.minres_block(np.ones((n + 1, 2)))
    with pytest.raises(Panic, match="X0 has shape"):
        a.minres_block(np.ones((n, 2)), X0=np.ones((n, 3)))
    with pytest.raises(TypeError, match="M must be a CsrMatrix"):
        a.minres(b, M=c)
    with pytest.raises(TypeError, match="M must be a CsrMatrix"):
        a.minres_block(np.ones((n, 2)), M=c)
    with pytest.raises(TypeError, match="precond_sweeps needs M"):
        a.minres(b, precond_sweeps=0)
    with pytest.raises(TypeError, match="precond_sweeps needs M"):
        a.minres_block(np.ones((n, 2)), precond_sweeps=0)
