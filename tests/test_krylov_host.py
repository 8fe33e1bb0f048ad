"""Host tests of the dot product's definition (spal_dot_* against tests/krylov_ref.py, raw bits) and of the reference
loops themselves (against numpy.linalg.solve).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import krylov_ref as kr
from tests import trsv_ref as tr

DTYPES = [np.float64, np.float32]
SIZES = [0, 1, 2, 1023, 1024, 1025, 1024 ** 2 - 1, 1024 ** 2, 1024 ** 2 + 1]


SEED = 2   # checked on the CPU: with these inputs the sequential sum and np.sum differ from the definition at every n >= 1024


def mixed(n, dtype, seed):
    """uniform(-1, 1) * 10^randint(-6, 6): magnitudes far enough apart that the order of the sum shows in its bits."""
    rng = np.random.default_rng(SEED + seed)
    return (rng.uniform(-1, 1, size=n) * 10.0 ** rng.integers(-6, 7, size=n)).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_dot_is_the_definition(n, dtype):
    a, b = mixed(n, dtype, 2 * n + 1), mixed(n, dtype, 2 * n + 2)
    got = sp.dot(a, b)
    ref = kr.dot(a, b)
    assert got.dtype == dtype
    tr.assert_same_bits(np.array([got]), np.array([ref]))
    if n >= 1024:   # another order gives other bits, so the comparison above can tell
        with np.errstate(all="ignore"):
            seq = kr.sequential_sum(a * b)
        assert seq.tobytes() != ref.tobytes()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_dot_zeros_and_nan(dtype):
    one = np.ones(1, dtype=dtype)
    z = sp.dot(np.array([-0.0], dtype=dtype), one)
    assert z == 0 and not np.signbit(z)                 # the padding zeros are added: -0.0 + +0.0 = +0.0
    assert not np.signbit(kr.dot(np.array([-0.0], dtype=dtype), one))
    e = sp.dot(np.zeros(0, dtype=dtype), np.zeros(0, dtype=dtype))
    assert e == 0 and not np.signbit(e)
    a = mixed(3000, dtype, 5)
    a[2049] = np.nan
    assert np.isnan(sp.dot(a, np.ones(3000, dtype=dtype))) and np.isnan(kr.dot(a, np.ones(3000, dtype=dtype)))
    a[2049] = np.inf
    assert sp.dot(a, np.ones(3000, dtype=dtype)) == np.inf


def test_dot_refuses_null_pointers():
    lib = _ffi.lib()
    out = C.c_double(7.0)
    assert lib.spal_dot_f64(None, None, C.c_uint64(3), C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert b"null argument" in lib.spal_last_error()
    assert lib.spal_dot_f64(None, None, C.c_uint64(0), None) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert lib.spal_dot_f64(None, None, C.c_uint64(0), C.byref(out)) == 0 and out.value == 0.0


# ---- the reference loops --------------------------------------------------------------------------------------------

def dense_case(n, spd, dtype, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, size=(n, n))
    if spd:
        a = (a + a.T) / 2
    np.fill_diagonal(a, 0)
    np.fill_diagonal(a, 1 + np.abs(a).sum(axis=1))
    return a.astype(dtype), rng.uniform(-1, 1, size=n).astype(dtype)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 1e-5)], ids=["f64", "f32"])
@pytest.mark.parametrize("method,spd", [("cg", True), ("bicgstab", True), ("bicgstab", False)])
@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "preconditioned"])
def test_reference_loops_solve_small_dense_systems(method, spd, jacobi, dtype, tol):
    a, b = dense_case(60, spd, dtype, 11)
    d = np.diag(a).copy()
    prec = (lambda v: v / d) if jacobi else None
    x, info = kr.METHODS[method](lambda v: a @ v, prec, b, np.zeros_like(b), tol, 200)
    assert info["reason"] == 0 and 0 < info["iterations"] < 60 and x.dtype == dtype
    exact = np.linalg.solve(a.astype(np.float64), b.astype(np.float64))
    assert np.linalg.norm(x - exact) <= 10 * tol * np.linalg.norm(exact) * np.linalg.cond(a.astype(np.float64))
    assert np.linalg.norm(b - a.astype(np.float64) @ x) <= 2 * tol * np.linalg.norm(b)
    assert info["rhs_sq"] == float(kr.dot(b, b))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_diagonal_matrix_with_its_own_factor_takes_the_half_step_exit(dtype):
    rng = np.random.default_rng(3)
    d = rng.uniform(1, 2, size=1025).astype(dtype)
    b = rng.uniform(-1, 1, size=1025).astype(dtype)
    x, info = kr.bicgstab(lambda v: d * v, lambda v: v / d, b, np.zeros_like(b), 1e-5, 200)
    assert info["iterations"] == 1 and info["reason"] == 0
    assert np.allclose(x, b / d, rtol=1e-5)
    x, info = kr.cg(lambda v: d * v, lambda v: v / d, b, np.zeros_like(b), 1e-5, 200)
    assert info["iterations"] == 1 and info["reason"] == 0


@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_maxit_zero_does_nothing(method):
    a, b = dense_case(20, True, np.float64, 5)
    x0 = np.random.default_rng(6).uniform(-1, 1, size=20)
    x, info = kr.METHODS[method](lambda v: a @ v, None, b, x0, 1e-10, 0)
    assert info["iterations"] == 0 and info["reason"] == 1 and np.array_equal(x, x0)
    r0 = b - a @ x0
    assert info["residual_sq"] == float(kr.dot(r0, r0))
    # already converged: reason 0, it = 0, whatever maxit is
    exact = np.linalg.solve(a, b)
    x, info = kr.METHODS[method](lambda v: a @ v, None, b, exact, 1e-6, 50)
    assert info["iterations"] == 0 and info["reason"] == 0 and np.array_equal(x, exact)


@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_zero_matrix_breaks_down_after_one_iteration(method):
    b = np.random.default_rng(8).uniform(-1, 1, size=10)
    x, info = kr.METHODS[method](lambda v: 0 * v, None, b, np.zeros(10), 1e-10, 200)
    assert info["iterations"] == 1 and info["reason"] == 2


def test_spd_fill_is_symmetric_and_dominant():
    from tests import ilu_ref as ir
    pattern = ir.sym(tr.banded(300, 4, 40, np.random.default_rng(1)))
    values, b = kr.spd_fill(pattern, np.float64, np.random.default_rng(2))
    n, rowptr, colind = pattern
    dense = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))
    dense[rows, colind.astype(np.int64)] = values
    assert np.array_equal(dense, dense.T)
    assert np.all(np.diag(dense) > np.abs(dense).sum(axis=1) - np.diag(dense))
    assert np.linalg.eigvalsh(dense).min() > 0
    with pytest.raises(AssertionError):
        kr.spd_fill(tr.bidiagonal(10), np.float64, np.random.default_rng(2))


def test_option_and_entry_points_refuse_without_a_device():
    """the checks that need no device come first"""
    lib = _ffi.lib()
    info = sp.matrix._KrylovInfoC()
    x = np.zeros(3)
    p = x.ctypes.data_as(_ffi.f64p)
    assert lib.spal_csr_krylov_f64(None, 0, None, p, C.c_uint64(3), p, C.c_uint64(3), C.c_double(1e-8), C.c_uint64(5),
                                   C.byref(info)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert b"spal_csr_krylov: null argument" in lib.spal_last_error()
    assert lib.spal_csc_krylov_dev_f32(None, 0, None, None, None, C.c_double(1e-8), C.c_uint64(5), None,
                                       C.byref(info)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
