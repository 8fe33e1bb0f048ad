"""Host side of ILU(0) by row sweeps: the entry points exist and check their arguments before any device
work, the Python layer refuses what is no sweep count, the Rust declarations are in step, and the CPU restatement
(tests/ilu_sweep_ref.py) has the properties include/spal.h states -- both of its forms bit-equal, ilu0's bits from
s = levels - 1 on, not before on the structures where rounding cannot hide a missing pass.  None of this needs a GPU."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi

from . import ilu_ref as ir
from . import ilu_sweep_ref as isr
from . import trsv_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["spal_csr_ilu0_sweep", "spal_csc_ilu0_sweep"]
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
    for kind in ("csr", "csc"):
        assert (f"pub fn spal_{kind}_ilu0_sweep(a: *mut spal_{kind}, sweeps: u64, stream: *mut c_void, "
                f"out: *mut *mut spal_{kind}) -> c_int;") in text


@pytest.mark.parametrize("name", NAMES)
def test_null_arguments_are_refused_and_out_is_not_written(name):
    fn = getattr(_ffi.lib(), name)
    out = C.c_void_p(0x1234)
    assert fn(None, C.c_uint64(3), None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert f"{name}: null argument".encode() in _ffi.lib().spal_last_error()
    assert out.value == 0x1234


@pytest.mark.parametrize("cls", [sp.CsrMatrix, sp.CscMatrix])
def test_python_refuses_what_is_no_sweep_count_before_any_device_work(cls):
    a = cls(2, 2, [0, 1, 2], [0, 1], np.array([1.0, 2.0]))
    for bad in (1.5, "3", 2.0, True, [1]):
        with pytest.raises(TypeError, match="sweeps must be None or an integer"):
            a.ilu0(sweeps=bad)
    for bad in (-1, np.int64(-7)):
        with pytest.raises(ValueError, match="sweeps must be >= 0"):
            a.ilu0(sweeps=bad)
    assert not a._dev                                    # nothing was uploaded for any of them


# ---- the reference ----------------------------------------------------------------------------------------------------

def _patterns():
    rng = np.random.default_rng(1909)
    return {
        "sym_bidiagonal": ir.sym(tr.bidiagonal(40)),
        "sym_banded": ir.sym(tr.banded(120, 4, 16, rng)),
        "full": ir.full(200, 5, rng),
        "sym_dense": ir.sym(tr.dense_triangle(30)),
        "sym_arrow": ir.sym(tr.arrow(50)),
        "fan": ir.fan(40),
        "one": tr.diagonal(1),
        "hand": ir.dense_to_csr(ir.HAND_A, np.float64)[0],
    }


NAMES_OF_PATTERNS = sorted(_patterns())


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """(pattern, values, nlevels, ilu0_loop's factor) -- computed once, shared, never written to."""
    pattern = _patterns()[name]
    if name == "hand":
        values = ir.dense_to_csr(ir.HAND_A, dtype)[1]
    else:
        values, _ = ir.fill(pattern, dtype, np.random.default_rng(11))
    nl = tr.levels(*pattern, lower=True)[1]
    exact = ir.ilu0_loop(*pattern, values)
    assert np.isfinite(exact).all()
    for a in (*pattern[1:], values, exact):
        a.setflags(write=False)
    return pattern, values, nl, exact


def _differs(x, ref):
    return not np.array_equal(x.view(np.uint8), ref.view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES_OF_PATTERNS)
def test_rows_form_equals_the_loop_bit_for_bit(name, dtype):
    pattern, values, nl, _ = case(name, dtype)
    for s in sorted({0, 1, 2, 3, nl - 1}):
        loop = isr.ilu0_sweep_loop(*pattern, values, s)
        assert loop.dtype == dtype
        ir.assert_same_bits(isr.ilu0_sweep_rows(*pattern, values, s), loop)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES_OF_PATTERNS)
def test_levels_minus_one_sweeps_and_more_are_ilu0_bit_for_bit(name, dtype):
    pattern, values, nl, exact = case(name, dtype)
    ir.assert_same_bits(isr.ilu0_sweep_loop(*pattern, values, nl - 1), exact)
    ir.assert_same_bits(isr.ilu0_sweep_rows(*pattern, values, nl + 2), exact)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["sym_arrow", "fan"])
def test_one_pass_fewer_is_not_yet_the_factor(name, dtype):
    # (not asserted on the long chains: there rounding makes the sweeps reach the exact bits before levels - 1)
    pattern, values, nl, exact = case(name, dtype)
    assert nl >= 2
    assert _differs(isr.ilu0_sweep_loop(*pattern, values, nl - 2), exact)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("form", [isr.ilu0_sweep_loop, isr.ilu0_sweep_rows], ids=["loop", "rows"])
def test_hand_example(form, dtype):
    pattern, values, nl, exact = case("hand", dtype)
    factor = ir.dense_to_csr(ir.HAND_F, dtype)[1]
    assert nl == 4 and exact.tolist() == factor.tolist()
    assert form(*pattern, values, 3).tolist() == factor.tolist()
    for s in (0, 1, 2):
        assert _differs(form(*pattern, values, s), factor), s
    # pass 1 by hand: row 1 against A's row 0, row 2 against A's row 1, row 3 against A's row 2
    assert form(*pattern, values, 1).tolist() == [2, 1, 2, -1, 3, 3, -13, -2, -5, -15]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES_OF_PATTERNS)
def test_no_sweep_is_a(name, dtype):
    pattern, values, _, _ = case(name, dtype)
    for form in (isr.ilu0_sweep_loop, isr.ilu0_sweep_rows):
        out = form(*pattern, values, 0)
        ir.assert_same_bits(out, values)
        assert out is not values


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("form", [isr.ilu0_sweep_loop, isr.ilu0_sweep_rows], ids=["loop", "rows"])
def test_updates_on_unstored_entries_are_dropped(form, dtype):
    pattern, values = ir.dense_to_csr(ir.DROP_A, dtype)
    # two levels: one pass is the factor, and the updates of (1, 2) and (2, 1) had nowhere to go
    assert tr.levels(*pattern, lower=True)[1] == 2
    for s in (1, 2, 5):
        assert form(*pattern, values, s).tolist() == [2, 1, 1, 2, 3, 3, 4]
    assert form(*pattern, values, 0).tolist() == values.tolist()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_zero_pivot_gives_inf_and_nan_by_position(dtype):
    # every entry stored, a 0.0 at (0, 0): rows 1 and 2 divide by it
    pattern = tr.from_coo(3, np.repeat(np.arange(3), 3), np.tile(np.arange(3), 3))
    values = np.array([0, 1, 1, 1, 1, 1, 1, 1, 1], dtype=dtype)
    exact = ir.ilu0_loop(*pattern, values)
    for s in (1, 2, 3):
        loop = isr.ilu0_sweep_loop(*pattern, values, s)
        ir.assert_same_bits(isr.ilu0_sweep_rows(*pattern, values, s), loop)
        assert np.isinf(loop).any() and np.isnan(loop).any() and np.isfinite(loop).any()
        assert loop[:3].tolist() == [0, 1, 1]            # row 0 is A's in every pass
    ir.assert_same_bits(isr.ilu0_sweep_loop(*pattern, values, 2), exact)       # three levels
    # pass 1 by position: (1,0) = 1/0 = inf, (1,1) = 1 - inf, (2,0) = inf, (2,1) = (1 - inf) / A[1,1] ...
    one = isr.ilu0_sweep_loop(*pattern, values, 1)
    assert np.isposinf(one[3]) and np.isneginf(one[4]) and np.isposinf(one[6])
