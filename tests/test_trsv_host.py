"""Host side of the sparse triangular solve: the entry points exist, arguments are checked before any device work, the
level analysis (spal_trsv_levels) agrees with the CPU restatement, and the restatement's two forms agree with each
other bit for bit.  None of this needs a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi

from . import trsv_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE_NAMES = [f"spal_{fmt}_trsv_{form}" for fmt in ("csr", "csc")
                for form in ("analyse", "f64", "f32", "dev_f64", "dev_f32")]
NAMES = ["spal_trsv_levels"] + HANDLE_NAMES
u64 = C.c_uint64


def _levels(pattern, lower=True, unit=False):
    n, rowptr, colind = pattern
    level_of = np.full(n, 2**63, dtype=np.uint64)
    nl = u64(12345)
    st = _ffi.lib().spal_trsv_levels(u64(n), rowptr.ctypes.data_as(_ffi.u64p), colind.ctypes.data_as(_ffi.u64p),
                                     C.c_int(0 if lower else 1), C.c_int(1 if unit else 0),
                                     level_of.ctypes.data_as(_ffi.u64p), C.byref(nl))
    return st, level_of, nl.value


def test_every_new_name_is_declared_and_exported():
    names = _ffi.exported_names()
    lib = _ffi.lib()
    assert len(NAMES) == 11
    for n in NAMES:
        assert n in names
        assert hasattr(lib, n)


def test_rust_ffi_is_in_step_with_the_header():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"]).returncode == 0
    text = open(os.path.join(ROOT, "rust_shim", "src", "ffi.rs")).read()
    for n in NAMES:
        assert f"pub fn {n}(" in text
    assert "pub fn spal_trsv_levels(n: u64, rowptr: *const u64, colind: *const u64, uplo: c_int, unit_diag: c_int, " \
           "level_of: *mut u64, nlevels: *mut u64) -> c_int;" in text


@pytest.mark.parametrize("name", HANDLE_NAMES)
def test_null_handle_is_an_invalid_argument(name):
    fn = getattr(_ffi.lib(), name)
    buf = (C.c_double * 4)()
    if name.endswith("analyse"):
        st = fn(None, C.c_int(0), C.c_int(0), None)
    elif "_dev_" in name:
        st = fn(None, C.c_int(0), C.c_int(0), buf, buf, None)
    else:
        st = fn(None, C.c_int(0), C.c_int(0), buf, u64(4), buf, u64(4))
    assert st == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert b"handle is NULL" in _ffi.lib().spal_last_error()


def test_levels_rejects_null_arrays_and_flags_outside_0_1():
    lib = _ffi.lib()
    n, rowptr, colind = tr.bidiagonal(4)
    out, nl = np.zeros(4, dtype=np.uint64), u64()
    rp, ci, lo = rowptr.ctypes.data_as(_ffi.u64p), colind.ctypes.data_as(_ffi.u64p), out.ctypes.data_as(_ffi.u64p)
    assert lib.spal_trsv_levels(u64(4), None, ci, 0, 0, lo, C.byref(nl)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert lib.spal_trsv_levels(u64(4), rp, None, 0, 0, lo, C.byref(nl)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert lib.spal_trsv_levels(u64(4), rp, ci, 0, 0, None, C.byref(nl)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert lib.spal_trsv_levels(u64(4), rp, ci, 0, 0, lo, None) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    for uplo, unit in ((2, 0), (-1, 0), (0, 2), (1, -1)):
        assert lib.spal_trsv_levels(u64(4), rp, ci, uplo, unit, lo, C.byref(nl)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
        assert b"uplo must be 0 (lower) or 1 (upper)" in lib.spal_last_error()
    assert lib.spal_trsv_levels(u64(4), rp, ci, 0, 0, lo, C.byref(nl)) == _ffi.SPAL_OK
    assert out.tolist() == [0, 1, 2, 3] and nl.value == 4


def _patterns():
    rng = np.random.default_rng(2611)
    rand_lower = tr.banded(700, 3, 699, rng)           # random lower triangle: columns anywhere below the diagonal
    return {
        "random_lower": rand_lower,
        "random_upper": tr.mirror(tr.banded(650, 4, 100, rng)),
        "full": tr.full(500, 5, rng),
        "diagonal": tr.diagonal(300),
        "bidiagonal": tr.bidiagonal(400),
        "bidiagonal_upper": tr.mirror(tr.bidiagonal(400)),
        "chains": tr.chains([1, 2, 2, 5, 9, 30]),
        "arrow": tr.arrow(200),
        "one": tr.diagonal(1),
    }


@pytest.mark.parametrize("name", sorted(_patterns()))
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_levels_agree_with_the_restatement(name, lower):
    pattern = _patterns()[name]
    st, level_of, nl = _levels(pattern, lower)
    assert st == _ffi.SPAL_OK, _ffi.lib().spal_last_error()
    ref, ref_nl = tr.levels(*pattern, lower=lower)
    assert nl == ref_nl
    assert np.array_equal(level_of, ref)
    if name == "diagonal":
        assert nl == 1
    if name == "bidiagonal":
        assert nl == (400 if lower else 1)      # the upper triangle of a lower bidiagonal matrix is its diagonal
    if name == "bidiagonal_upper":
        assert nl == (1 if lower else 400)


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_prescribed_widths_come_back_exactly(lower):
    pattern = tr.prescribed(tr.PRESCRIBED_WIDTHS, np.random.default_rng(7))
    if not lower:
        pattern = tr.mirror(pattern)
    st, level_of, nl = _levels(pattern, lower)
    assert st == _ffi.SPAL_OK
    assert nl == len(tr.PRESCRIBED_WIDTHS)
    assert tuple(tr.level_widths(level_of, nl)) == tr.PRESCRIBED_WIDTHS
    assert np.array_equal(level_of, tr.levels(*pattern, lower=lower)[0])
    if lower:   # rows were laid out in level order
        assert np.array_equal(level_of, np.repeat(np.arange(nl, dtype=np.uint64), tr.PRESCRIBED_WIDTHS))


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_missing_diagonal_names_the_first_row_and_unit_accepts_it(lower):
    pattern = tr.full(60, 4, np.random.default_rng(3))
    for row in (41, 17, 53):          # rows 17, 41 and 53 end up without a diagonal: 17 is the first, whatever the sweep
        pattern = tr.drop_diagonal(pattern, row)
    st, _, _ = _levels(pattern, lower, unit=False)
    assert st == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert b"row 17 stores no diagonal entry" in _ffi.lib().spal_last_error()
    st, level_of, nl = _levels(pattern, lower, unit=True)
    assert st == _ffi.SPAL_OK
    assert np.array_equal(level_of, tr.levels(*pattern, lower=lower)[0])


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_non_square_is_refused(lower):
    # 3 rows, a stored column 3: the matrix has at least 4 columns
    rowptr = np.array([0, 1, 3, 4], dtype=np.uint64)
    colind = np.array([0, 1, 3, 2], dtype=np.uint64)
    st, _, _ = _levels((3, rowptr, colind), lower)
    assert st == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert b"not square" in _ffi.lib().spal_last_error()


HAND_L = np.array([[2, 0, 0, 0], [1, 1, 0, 0], [0, 3, 4, 0], [1, 0, 2, 2]], dtype=np.float64)


def dense_to_csr(a, dtype):
    r, c = np.nonzero(a)
    n, rowptr, colind = tr.from_coo(a.shape[0], r, c)
    return n, rowptr, colind, a[r, c].astype(dtype)       # np.nonzero is row-major: the order from_coo produces


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_hand_example_by_the_reference_loop(dtype):
    n, rp, ci, v = dense_to_csr(HAND_L, dtype)
    x = tr.solve_loop(n, rp, ci, v, np.array([2, 3, 10, 9], dtype=dtype), lower=True)
    assert x.tolist() == [1, 2, 1, 3]
    n, rp, ci, v = dense_to_csr(HAND_L.T, dtype)
    x = tr.solve_loop(n, rp, ci, v, np.array([7, 5, 10, 6], dtype=dtype), lower=False)
    assert x.tolist() == [1, 2, 1, 3]
    st, level_of, nl = _levels((n, rp, ci), lower=False)
    assert st == _ffi.SPAL_OK and nl == 4 and level_of.tolist() == [3, 2, 1, 0]
    st, level_of, nl = _levels(dense_to_csr(HAND_L, dtype)[:3], lower=True)
    assert st == _ffi.SPAL_OK and nl == 4 and level_of.tolist() == [0, 1, 2, 3]
    # a unit diagonal ignores the stored one
    n, rp, ci, v = dense_to_csr(HAND_L, dtype)
    x = tr.solve_loop(n, rp, ci, v, np.array([2, 3, 10, 9], dtype=dtype), lower=True, unit=True)
    assert x.tolist() == [2, 1, 7, -7]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["random_lower", "random_upper", "full", "chains", "arrow", "bidiagonal", "one"])
def test_level_form_of_the_reference_equals_the_loop_bit_for_bit(name, dtype):
    pattern = _patterns()[name]
    rng = np.random.default_rng(99)
    values, b = tr.fill(pattern, dtype, rng)
    for lower in (True, False):
        st, level_of, _ = _levels(pattern, lower)      # the level form takes its levels from the same definition
        assert st == _ffi.SPAL_OK and np.array_equal(level_of, tr.levels(*pattern, lower=lower)[0])
        for unit in (False, True):
            loop = tr.solve_loop(*pattern, values, b, lower=lower, unit=unit)
            tr.assert_same_bits(tr.solve_by_levels(*pattern, values, b, lower=lower, unit=unit), loop)
            if not unit:
                assert np.abs(loop).max() <= np.abs(b).max()       # the diagonal dominance bound of fill()
    # ... also where a zero diagonal sends inf / NaN down the dependency graph
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))
    values = values.copy()
    values[(rows == n // 2) & (colind == n // 2)] = 0
    loop = tr.solve_loop(*pattern, values, b, lower=True)
    assert n == 1 or not np.isfinite(loop[n // 2])
    tr.assert_same_bits(tr.solve_by_levels(*pattern, values, b, lower=True), loop)


@pytest.mark.parametrize("cls", [sp.CsrMatrix, sp.CscMatrix])
def test_binding_refuses_bad_shapes_before_the_device(cls):
    a = cls(2, 3, [0, 1, 2] if cls is sp.CsrMatrix else [0, 1, 2, 2], [0, 1], np.array([1.0, 2.0]))
    with pytest.raises(sp.Panic, match=r"not square \(2 x 3\)"):
        a.solve_triangular(np.ones(2))
    sq = cls(2, 2, [0, 1, 2], [0, 1], np.array([1.0, 2.0]))
    with pytest.raises(sp.Panic, match="b has shape"):
        sq.solve_triangular(np.ones(3))
    with pytest.raises(sp.Panic, match="b has shape"):
        sq.solve_triangular(np.ones((2, 2)))
    assert not a._dev and not sq._dev           # no device copy was made


def test_no_cpu_fallback():
    if sp.device_count() > 0:
        pytest.skip("a GPU is present: the no-device error path cannot be exercised")
    a = sp.CsrMatrix(2, 2, [0, 1, 2], [0, 1], np.array([1.0, 2.0]))
    with pytest.raises(sp.SpalError) as e:
        a.solve_triangular(np.ones(2))
    assert e.value.status == _ffi.SPAL_ERR_NO_DEVICE
