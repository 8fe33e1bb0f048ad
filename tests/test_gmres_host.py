"""Host tests of restarted GMRES: the reference text itself (tests/gmres_ref.py against numpy.linalg.solve, and the cases
that pin its edges), the eight names in the header, the library and the Rust binding, and the refusals that need no
device.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import gmres_ref as gr
from tests import krylov_ref as kr
from tests.test_krylov_host import dense_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float64, np.float32]
NAMES = [f"spal_{kind}_gmres_{form}{sfx}" for kind in ("csr", "csc") for form in ("", "dev_") for sfx in ("f64", "f32")]


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 1e-5)], ids=["f64", "f32"])
@pytest.mark.parametrize("restart", [1, 2, 5, 30, 100])
@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "preconditioned"])
def test_reference_solves_a_small_dense_system(jacobi, restart, dtype, tol):
    a, b = dense_case(60, False, dtype, 11)
    d = np.diag(a).copy()
    prec = (lambda v: v / d) if jacobi else None
    x, info = gr.gmres(lambda v: a @ v, prec, b, np.zeros_like(b), restart, tol, 200)
    assert info["reason"] == 0 and 0 < info["iterations"] <= 200 and x.dtype == dtype
    exact = np.linalg.solve(a.astype(np.float64), b.astype(np.float64))
    assert np.linalg.norm(x - exact) <= 10 * tol * np.linalg.norm(exact) * np.linalg.cond(a.astype(np.float64))
    assert np.linalg.norm(b - a.astype(np.float64) @ x) <= 2 * tol * np.linalg.norm(b)
    assert info["rhs_sq"] == float(kr.dot(b, b))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_cyclic_shift(dtype):
    mul, b, exact = gr.cyclic_shift(8, dtype)
    x0 = np.zeros_like(b)
    _, info = kr.bicgstab(mul, None, b, x0, 1e-6, 200)
    assert info["reason"] == 2 and info["iterations"] == 1            # BiCGStab breaks down on this system
    for restart in (8, 30):
        x, info = gr.gmres(mul, None, b, x0, restart, 1e-6, 200)
        assert info["iterations"] == 8 and info["reason"] == 0 and info["residual_sq"] == 0.0
        assert np.array_equal(x, exact)                                # the NaN v_8 of the lucky breakdown is never read
    x, info = gr.gmres(mul, None, b, x0, 4, 1e-6, 40)
    assert info["reason"] == 1 and info["iterations"] == 40           # GMRES(4) stagnates
    assert np.all(np.isfinite(x))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_edges(dtype):
    rng = np.random.default_rng(8)
    b = rng.uniform(-1, 1, size=10).astype(dtype)
    x0 = rng.uniform(-1, 1, size=10).astype(dtype)
    # zero matrix: cs = 0 / 0
    x, info = gr.gmres(lambda v: 0 * v, None, b, x0, 5, 1e-6, 200)
    assert info["iterations"] == 1 and info["reason"] == 2 and not np.isfinite(info["residual_sq"])
    assert x.tobytes() == x0.tobytes()
    # a diagonal matrix with itself as M: one iteration
    d = rng.uniform(1, 2, size=1025).astype(dtype)
    bd = rng.uniform(-1, 1, size=1025).astype(dtype)
    x, info = gr.gmres(lambda v: d * v, lambda v: v / d, bd, np.zeros_like(bd), 30, 1e-5, 200)
    assert info["iterations"] == 1 and info["reason"] == 0 and np.allclose(x, bd / d, rtol=1e-5)
    # n = 1
    x, info = gr.gmres(lambda v: dtype(3) * v, None, np.array([6], dtype=dtype), np.zeros(1, dtype=dtype), 30, 1e-6, 200)
    assert info["iterations"] == 1 and info["reason"] == 0 and x[0] == 2
    # maxit = 0, b = 0, an exact x0
    a, ba = dense_case(20, False, dtype, 5)
    mul = lambda v: a @ v                                                                  # noqa: E731
    x, info = gr.gmres(mul, None, ba, x0[:10].repeat(2), 5, 1e-6, 0)
    assert info["iterations"] == 0 and info["reason"] == 1 and x.tobytes() == x0[:10].repeat(2).tobytes()
    r0 = ba - mul(x0[:10].repeat(2))
    assert info["residual_sq"] == float(kr.dot(r0, r0))
    x, info = gr.gmres(mul, None, np.zeros_like(ba), np.zeros_like(ba), 5, 1e-6, 50)
    assert info["iterations"] == 0 and info["reason"] == 0 and not x.any()
    tol = 1e-10 if dtype == np.float64 else 1e-5
    exact = gr.gmres(mul, None, ba, np.zeros_like(ba), 30, tol, 100)[0]
    x, info = gr.gmres(mul, None, ba, exact, 30, 100 * tol, 100)
    assert info["iterations"] == 0 and info["reason"] == 0 and x.tobytes() == exact.tobytes()
    # maxit bounds the call in the middle of a cycle
    x, info = gr.gmres(mul, None, ba, np.zeros_like(ba), 5, 0.0, 7)
    assert info["iterations"] == 7 and info["reason"] == 1


def test_names_are_declared_exported_and_bound():
    declared = _ffi.exported_names()
    lib = _ffi.lib()
    with open(os.path.join(ROOT, "rust_shim", "src", "ffi.rs")) as f:
        rust = f.read()
    for name in NAMES:
        assert name in declared
        assert getattr(lib, name).restype is C.c_int
        assert f"pub fn {name}(" in rust
    with open(os.path.join(ROOT, "rust_shim", "src", "device.rs")) as f:
        assert f.read().count("pub fn gmres(") == 2
    for cls in (sp.CsrMatrix, sp.CscMatrix):
        assert callable(cls.gmres)
    for cls in (sp.DeviceCsr, sp.DeviceCsc):
        assert callable(cls.gmres) and callable(cls.gmres_dev)


def test_entry_points_refuse_without_a_device():
    """null arguments and the restart bounds come before any device call"""
    lib = _ffi.lib()
    info = sp.matrix._KrylovInfoC()
    x = np.zeros(3)
    p = x.ctypes.data_as(_ffi.f64p)
    u = C.c_uint64
    assert lib.spal_csr_gmres_f64(None, None, p, u(3), p, u(3), u(30), C.c_double(1e-8), u(5),
                                  C.byref(info)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert b"spal_csr_gmres: null argument" in lib.spal_last_error()
    assert lib.spal_csc_gmres_dev_f32(None, None, None, None, u(30), C.c_double(1e-8), u(5), None,
                                      C.byref(info)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert b"spal_csc_gmres_dev: null argument" in lib.spal_last_error()
    a = sp.CsrMatrix(3, 3, [0, 1, 2, 3], [0, 1, 2], np.ones(3))
    for restart in (0, 257):
        with pytest.raises(sp.Panic, match=f"restart = {restart} must be 1 .. 256"):
            a.gmres(np.ones(3), restart=restart)
    with pytest.raises(sp.Panic, match="b has shape"):
        a.gmres(np.ones(4))
