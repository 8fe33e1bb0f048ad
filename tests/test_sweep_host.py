"""Host side of the Jacobi sweeps on a triangle (include/spal.h): the restatement's two forms agree bit for
bit, enough sweeps ARE the sequential substitution, a few sweeps on an ILU(0) factor precondition CG nearly as well as
the exact solves, and the entry points exist and check what they can before any device work.  None of this needs a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from spalinalg_amd import _ffi
from tests import ilu_ref as ir
from tests import krylov_ref as kr
from tests import sweep_ref as sw
from tests import trsv_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float64, np.float32]
NAMES = [f"spal_{fmt}_trsv_sweep_{form}" for fmt in ("csr", "csc") for form in ("f64", "f32", "dev_f64", "dev_f32")]
u64 = C.c_uint64


def _lower_pattern(name):
    rng = np.random.default_rng(20261018)
    return {
        "bidiagonal": lambda: tr.bidiagonal(40),
        "banded": lambda: tr.banded(90, 3, 12, rng),
        "chains": lambda: tr.chains([1, 2, 2, 5, 9, 17]),
        "arrow": lambda: tr.arrow(50),
        "prescribed": lambda: tr.prescribed((1, 7, 8, 9, 1, 17, 3, 1), rng),
        "dense": lambda: tr.dense_triangle(24),
        "diagonal": lambda: tr.diagonal(30),
    }[name]()


STRUCTURES = ["bidiagonal", "banded", "chains", "arrow", "prescribed", "dense", "diagonal"]


def _case(name, lower, dtype):
    pattern = _lower_pattern(name)
    if not lower:
        pattern = tr.mirror(pattern)
    values, b = tr.fill(pattern, dtype, np.random.default_rng(STRUCTURES.index(name) * 2 + lower))
    return pattern, values, b


# ---- the entry points ----------------------------------------------------------------------------------------------

def test_every_new_name_is_declared_exported_and_bound_in_rust():
    names, lib = _ffi.exported_names(), _ffi.lib()
    assert len(NAMES) == 8
    text = open(os.path.join(ROOT, "rust_shim", "src", "ffi.rs")).read()
    for n in NAMES:
        assert n in names and hasattr(lib, n)
        assert f"pub fn {n}(a: *mut spal_{n[5:8]}, uplo: c_int, unit_diag: c_int, sweeps: u64, " in text
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"]).returncode == 0


def _call(name, handle, uplo, unit):
    fn, buf = getattr(_ffi.lib(), name), (C.c_double * 4)()
    if "_dev_" in name:
        return fn(handle, C.c_int(uplo), C.c_int(unit), u64(2), buf, buf, None)
    return fn(handle, C.c_int(uplo), C.c_int(unit), u64(2), buf, u64(4), buf, u64(4))


@pytest.mark.parametrize("name", NAMES)
def test_null_handle_and_flags_outside_0_1_are_invalid_arguments(name):
    lib = _ffi.lib()
    assert _call(name, None, 0, 0) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert b"handle is NULL" in lib.spal_last_error() and name[:19].encode() in lib.spal_last_error()
    for uplo, unit, text in ((2, 0, b"uplo = 2"), (-1, 1, b"uplo = -1"), (0, 2, b"unit_diag = 2"), (1, -1, b"unit_diag = -1")):
        assert _call(name, None, uplo, unit) == _ffi.SPAL_ERR_INVALID_ARGUMENT
        assert text in lib.spal_last_error()


def test_option_needs_a_handle():
    lib = _ffi.lib()
    assert lib.spal_csr_set_option(None, b"trsv_sweeps", C.c_int64(3)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert lib.spal_csc_set_option(None, b"trsv_sweeps", C.c_int64(3)) == _ffi.SPAL_ERR_INVALID_ARGUMENT


# ---- the restatement -------------------------------------------------------------------------------------------------

def test_hand_example_by_hand():
    # L = [[2,0,0],[1,1,0],[0,3,4]], b = [2, 3, 10]: x0 = b / d = [1, 3, 2.5]; x1 = [1, (3 - 1*1) / 1, (10 - 3*3) / 4]
    pattern, values = ir.dense_to_csr(np.array([[2, 0, 0], [1, 1, 0], [0, 3, 4]], dtype=np.float64), np.float64)
    b = np.array([2.0, 3.0, 10.0])
    assert sw.sweep_loop(*pattern, values, b, 0).tolist() == [1, 3, 2.5]
    assert sw.sweep_loop(*pattern, values, b, 1).tolist() == [1, 2, 0.25]
    assert sw.sweep_loop(*pattern, values, b, 2).tolist() == [1, 2, 1]
    assert sw.sweep_loop(*pattern, values, b, 1, unit=True).tolist() == [2, 1, 1]       # x0 = b; [2, 3 - 2, 10 - 9]
    assert sw.sweep_loop(*pattern, values, b, 1, lower=False).tolist() == [1, 3, 2.5]   # its upper triangle is its diagonal


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("unit", [False, True], ids=["diag", "unit"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("name", STRUCTURES + ["full"])
def test_the_two_forms_agree_in_bits(name, lower, unit, dtype):
    if name == "full":
        pattern = tr.full(70, 5, np.random.default_rng(3))
        values, b = tr.fill(pattern, dtype, np.random.default_rng(4))
    else:
        pattern, values, b = _case(name, lower, dtype)
    for s in (0, 1, 2, 5):
        sw.assert_same_bits(sw.sweep_vec(*pattern, values, b, s, lower, unit),
                            sw.sweep_loop(*pattern, values, b, s, lower, unit))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("unit", [False, True], ids=["diag", "unit"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("name", STRUCTURES)
def test_levels_minus_one_sweeps_are_the_sequential_substitution(name, lower, unit, dtype):
    pattern, values, b = _case(name, lower, dtype)
    nl = tr.levels(*pattern, lower=lower)[1]
    exact = tr.solve_loop(*pattern, values, b, lower=lower, unit=unit)
    sw.assert_same_bits(sw.sweep_loop(*pattern, values, b, nl - 1, lower, unit), exact)
    sw.assert_same_bits(sw.sweep_loop(*pattern, values, b, nl + 3, lower, unit), exact)     # and stay it
    if name == "bidiagonal":
        # One pass short, the chain's last row is not final yet -- with GENERIC values, every |entry| in (1, 1.5): under
        # fill()'s dominant diagonal what x0 left in the last row shrinks by more than half per row and is gone from the
        # bits long before the chain's end.
        assert nl == 40
        rng = np.random.default_rng(7)
        values = (rng.uniform(1, 1.5, size=values.size) * rng.choice([-1.0, 1.0], size=values.size)).astype(dtype)
        exact = tr.solve_loop(*pattern, values, b, lower=lower, unit=unit)
        sw.assert_same_bits(sw.sweep_loop(*pattern, values, b, nl - 1, lower, unit), exact)
        short = sw.sweep_loop(*pattern, values, b, nl - 2, lower, unit)
        assert short.tobytes() != exact.tobytes()
        last = 39 if lower else 0
        sw.assert_same_bits(np.delete(short, last), np.delete(exact, last))     # ... and only that row


def test_nan_and_inf_sit_where_the_substitution_puts_them():
    pattern = tr.banded(60, 3, 8, np.random.default_rng(5))
    values, b = tr.fill(pattern, np.float64, np.random.default_rng(6))
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))
    values[(rows == 20) & (colind == 20)] = 0
    exact = tr.solve_loop(*pattern, values, b)
    assert np.isinf(exact[20]) and np.isnan(exact).any() and np.isfinite(exact).any()
    nl = tr.levels(*pattern)[1]
    sw.assert_same_bits(sw.sweep_loop(*pattern, values, b, nl - 1), exact)
    sw.assert_same_bits(sw.sweep_vec(*pattern, values, b, nl - 1), exact)


# ---- a few sweeps on an ILU(0) factor as a preconditioner -----------------------------------------------------------------

def _poisson_cg(m, prec):
    pattern, values = sw.poisson2d(m)
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    ci = colind.astype(np.int64)
    mul = lambda v: np.bincount(rows, weights=values * v[ci], minlength=n)      # noqa: E731
    b = np.random.default_rng(16).uniform(-1, 1, size=n)
    return kr.cg(mul, prec, b, np.zeros(n), 1e-8, 500)


def test_three_sweeps_precondition_cg_nearly_as_well_as_the_exact_solves():
    pattern, values = sw.poisson2d(16)
    f = ir.ilu0_loop(*pattern, values)
    sw.assert_same_bits(f, ir.ilu0_rows(*pattern, values))
    nl = max(tr.levels(*pattern, lower=True)[1], tr.levels(*pattern, lower=False)[1])
    assert nl == 31

    def exact(v):
        return tr.solve_by_levels(*pattern, f, tr.solve_by_levels(*pattern, f, v, lower=True, unit=True), lower=False)

    runs = {"none": _poisson_cg(16, None), "exact": _poisson_cg(16, exact)}
    for s in (0, 3, nl - 1):
        runs[s] = _poisson_cg(16, sw.preconditioner(pattern, f, s))
    its = {k: r[1]["iterations"] for k, r in runs.items()}
    print("CG iterations on the 16 x 16 Poisson matrix:", its)
    assert all(r[1]["reason"] == 0 for r in runs.values())
    assert its[3] < its["none"]
    assert its[3] <= 1.25 * its["exact"]
    assert its[nl - 1] == its["exact"]
    sw.assert_same_bits(runs[nl - 1][0], runs["exact"][0])
    sw.assert_same_bits(np.array([runs[nl - 1][1]["residual_sq"]]), np.array([runs["exact"][1]["residual_sq"]]))
