"""Host side of ILU(0): the entry points exist and check their arguments before any device work, the Rust declarations
are in step, and the CPU restatement (tests/ilu_ref.py) gives the hand answers, in both of its forms.  None of this
needs a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from spalinalg_amd import _ffi

from . import ilu_ref as ir
from . import trsv_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["spal_csr_ilu0", "spal_csc_ilu0"]
DTYPES = [np.float64, np.float32]


def test_every_new_name_is_declared_and_exported():
    names = _ffi.exported_names()
    lib = _ffi.lib()
    for n in NAMES:
        assert n in names
        assert hasattr(lib, n)


def test_rust_ffi_is_in_step_with_the_header():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"]).returncode == 0
    text = open(os.path.join(ROOT, "rust_shim", "src", "ffi.rs")).read()
    assert "pub fn spal_csr_ilu0(a: *mut spal_csr, stream: *mut c_void, out: *mut *mut spal_csr) -> c_int;" in text
    assert "pub fn spal_csc_ilu0(a: *mut spal_csc, stream: *mut c_void, out: *mut *mut spal_csc) -> c_int;" in text
    device = open(os.path.join(ROOT, "rust_shim", "src", "device.rs")).read()
    assert device.count("pub fn ilu0(") == 2


@pytest.mark.parametrize("name", NAMES)
def test_null_arguments_are_refused_and_out_is_not_written(name):
    fn = getattr(_ffi.lib(), name)
    out = C.c_void_p(0x1234)
    assert fn(None, None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert f"{name}: null argument".encode() in _ffi.lib().spal_last_error()
    assert out.value == 0x1234


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", [ir.ilu0_loop, ir.ilu0_rows], ids=["loop", "rows"])
def test_hand_examples_by_the_reference(form, dtype):
    pattern, values = ir.dense_to_csr(ir.HAND_A, dtype)
    assert values.tolist() == [2, 1, 4, 1, 3, 3, -4, -2, 20, -5]
    f = form(*pattern, values)
    assert f.dtype == dtype and f.tolist() == ir.dense_to_csr(ir.HAND_F, dtype)[1].tolist()
    assert f.tolist() == [2, 1, 2, -1, 3, -3, 5, -2, 4, 3]
    # M^-1 (A x) = x for this matrix (its factorisation has no fill, so L U = A)
    x = np.array([1, 2, 1, 3], dtype=dtype)
    b = (ir.HAND_A @ x.astype(np.float64)).astype(dtype)
    y = tr.solve_loop(*pattern, f, b, lower=True, unit=True)
    assert tr.solve_loop(*pattern, f, y, lower=False).tolist() == [1, 2, 1, 3]
    # fill that has nowhere to go is dropped
    pattern, values = ir.dense_to_csr(ir.DROP_A, dtype)
    assert pattern[1].tolist() == [0, 3, 5, 7] and pattern[2].tolist() == [0, 1, 2, 0, 1, 0, 2]
    assert form(*pattern, values).tolist() == [2, 1, 1, 2, 3, 3, 4]


def _patterns():
    rng = np.random.default_rng(1812)
    return {
        "full": ir.full(300, 6, rng),
        "sym_banded": ir.sym(tr.banded(400, 5, 40, rng)),
        "sym_bidiagonal": ir.sym(tr.bidiagonal(200)),
        "sym_dense": ir.sym(tr.dense_triangle(40)),
        "sym_arrow": ir.sym(tr.arrow(150)),
        "fan": ir.fan(130),
        "one": tr.diagonal(1),
    }


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(_patterns()))
def test_row_form_of_the_reference_equals_the_loop_bit_for_bit(name, dtype):
    pattern = _patterns()[name]
    values, _ = ir.fill(pattern, dtype, np.random.default_rng(7))
    loop = ir.ilu0_loop(*pattern, values)
    assert np.isfinite(loop).all()
    ir.assert_same_bits(ir.ilu0_rows(*pattern, values), loop)
    # ... also where a zero pivot sends inf / NaN through the rows that divide by it
    # (row 0 is never updated, so its stored zero is still zero when a later row divides by it)
    values = values.copy()
    values[ir.diag_positions(*pattern)[0]] = 0
    loop = ir.ilu0_loop(*pattern, values)
    ir.assert_same_bits(ir.ilu0_rows(*pattern, values), loop)
    if name != "one":
        assert np.isinf(loop).any() and np.isfinite(loop).any()


def test_sym_keeps_the_lower_pattern_and_its_levels():
    lower = tr.prescribed(tr.PRESCRIBED_WIDTHS, np.random.default_rng(3))
    s = ir.sym(lower)
    level_of, nl = tr.levels(*s, lower=True)
    assert tuple(tr.level_widths(level_of, nl)) == tr.PRESCRIBED_WIDTHS
    n, rowptr, colind = s
    rows = np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))
    below = colind.astype(np.int64) <= rows
    assert np.array_equal(tr.from_coo(n, rows[below], colind[below])[2], lower[2])
    assert ir.rows_with_lower_entries(s) == n - 1
    f = ir.fan(10)
    assert f[1].tolist() == list(range(0, 19, 2)) + [28] and ir.rows_with_lower_entries(f) == 1
