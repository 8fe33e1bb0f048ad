"""Host side of the block triangular solves (spal_*_trsm_*): the sixteen entry points exist, a null handle
answers before anything else, the Python refusals fire before a device copy is made, and nothing falls back to the CPU.
None of this needs a GPU."""
import ctypes as C

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi

NAMES = [f"spal_{fmt}_trsm_{form}{sfx}" for fmt in ("csr", "csc") for form in ("", "dev_", "sweep_", "sweep_dev_")
         for sfx in ("f64", "f32")]


def test_the_sixteen_entry_points_are_declared_and_exported():
    names = _ffi.exported_names()
    lib = _ffi.lib()
    assert len(NAMES) == len(set(NAMES)) == 16
    for n in NAMES:
        assert n in names
        assert hasattr(lib, n)


@pytest.mark.parametrize("name", NAMES)
def test_null_handle_is_an_invalid_argument(name):
    fn = getattr(_ffi.lib(), name)
    u, i, buf = C.c_uint64, C.c_int, (C.c_double * 4)()
    args = [None, i(0), i(0)] + ([u(2)] if "_sweep_" in name else [])          # a, uplo, unit_diag[, sweeps]
    if "_dev_" in name:
        args += [u(1), buf, u(1), buf, u(1), None]                               # k, b, ldb, x, ldx, stream
    else:
        args += [u(1), buf, u(1), u(4), buf, u(1), u(4)]                         # k, b, ldb, b_rows, x, ldx, x_rows
    assert fn(*args) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    msg = _ffi.lib().spal_last_error()
    assert b"handle is NULL" in msg and name.rsplit("_", 1)[0].encode() in msg


@pytest.mark.parametrize("cls", [sp.CsrMatrix, sp.CscMatrix])
def test_bad_shapes_panic_before_the_device(cls):
    sq = cls(3, 3, [0, 1, 2, 3], [0, 1, 2], np.array([1.0, 2.0, 4.0]))
    for sweeps in (None, 2):
        with pytest.raises(sp.Panic, match=r"B has shape \(4, 2\) but the matrix has 3 rows"):
            sq.solve_triangular_block(np.ones((4, 2)), sweeps=sweeps)
        with pytest.raises(sp.Panic, match=r"B has shape \(3, 2, 2\)"):
            sq.solve_triangular_block(np.ones((3, 2, 2)), sweeps=sweeps)
        with pytest.raises(sp.Panic, match=r"B has shape \(\)"):
            sq.solve_triangular_block(np.float64(1.0), sweeps=sweeps)
        with pytest.raises(sp.Panic, match=r"B has shape \(2,\)"):
            sq.solve_triangular_block(np.ones(2), sweeps=sweeps)
    assert not sq._dev             # no device copy was made
    # solve_triangular itself keeps its one 1-D right-hand side: a block is refused there as it always was
    with pytest.raises(sp.Panic, match=r"solve_triangular: b has shape \(3, 2\)"):
        sq.solve_triangular(np.ones((3, 2)))
    assert not sq._dev
    ptr = [0, 1, 2] if cls is sp.CsrMatrix else [0, 1, 1, 2]
    rect = cls(2, 3, ptr, [0, 1] if cls is sp.CscMatrix else [0, 2], np.array([1.0, 2.0]))
    with pytest.raises(sp.Panic, match=r"not square \(2 x 3\)"):
        rect.solve_triangular_block(np.ones((2, 4)))
    with pytest.raises(sp.Panic, match=r"not square \(2 x 3\)"):
        rect.solve_triangular_block(np.ones((2, 4)), sweeps=1)
    assert not rect._dev


@pytest.mark.parametrize("sweeps", [None, 2])
def test_no_cpu_fallback_for_a_block(sweeps):
    if sp.device_count() > 0:
        pytest.skip("a GPU is present: the no-device error path cannot be exercised")
    a = sp.CsrMatrix(3, 3, [0, 1, 2, 3], [0, 1, 2], np.array([1.0, 2.0, 4.0]))
    with pytest.raises(sp.SpalError) as e:
        a.solve_triangular_block(np.ones((3, 2)), sweeps=sweeps)
    assert e.value.status == _ffi.SPAL_ERR_NO_DEVICE
