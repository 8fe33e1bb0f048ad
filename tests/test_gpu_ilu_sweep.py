"""ILU(0) by row sweeps on the device against its sequential definition (tests/ilu_sweep_ref.py): raw bits equal, NaN by
position, f64 and f32, CSR and CSC, whatever the geometry and the row forms are -- and, from levels - 1 sweeps on, the
bits of the device's own exact ilu0().

Matrices come from trsv_ref.fill (rows strictly diagonally dominant, so every pass's factor is finite).  The sizes that
matter to the kernel are read from describe()["ilu0_sweep"] once -- B = block_rows, the rows of a workgroup; S =
stage_entries, the entries of a block it stages in LDS; W = wide_stage_entries, the entries of a wide row its wave
stages -- and the boundary cases are built around them: row counts B - 1 / B / B + 1 / 2B + 1 / 3B + 7, a block of more
than S entries (rows in place in global memory), wide rows of W and W + 1 entries (staged, in place)."""
import ctypes as C
import functools
import threading
import zlib

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import gmres_ref as gr
from tests import ilu_ref as ir
from tests import ilu_sweep_ref as isr
from tests import krylov_ref as kr
from tests import sweep_ref as sw
from tests import trsv_ref as tr

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
SWEEPS = (0, 1, 2, 5)
HUGE = 1 << 40
KEYS = {"sweeps", "requested", "launches", "block_rows", "stage_entries", "wide_stage_entries", "rows_row_form",
        "rows_wide_form", "wide_work", "kernel_ms", "call_ms"}


def csr(pattern, values):
    n, rowptr, colind = pattern
    return sp.CsrMatrix(n, n, rowptr, colind, values)


def csc(pattern, values):
    n = pattern[0]
    colptr, rowind, vals, _ = ir.to_csc(pattern, values)
    return sp.CscMatrix(n, n, colptr, rowind, vals)


MAKERS = {"csr": csr, "csc": csc}


@functools.lru_cache(maxsize=None)
def geometry():
    """(B, S, W) as describe() reports them on a swept factor."""
    pattern, values = ir.dense_to_csr(ir.HAND_A, np.float64)
    d = csr(pattern, values).device().ilu0(sweeps=1).describe()["ilu0_sweep"]
    assert set(d) == KEYS
    B, S, W = d["block_rows"], d["stage_entries"], d["wide_stage_entries"]
    assert B >= 1 and 1 <= W <= S
    return B, S, W


def _pattern(name):
    B, S, W = geometry()
    rng = np.random.default_rng(20261019)
    if name == "full":
        return ir.full(2 * B + 1, 6, rng)
    if name == "banded":
        return ir.sym(tr.banded(3 * B + 7, 6, 64, rng))
    if name in ("bidiagonal-", "bidiagonal", "bidiagonal+"):
        return ir.sym(tr.bidiagonal(B + {"-": -1, "l": 0, "+": 1}[name[-1]]))
    if name == "dense":
        return ir.sym(tr.dense_triangle(120))
    if name == "arrow":
        return ir.sym(tr.arrow(S + 1))              # its first and its last block hold more than S entries
    if name == "fan_long":
        return ir.fan(W + 1025)                     # the wide row cannot be staged: updated in place
    if name == "fan_w":
        return ir.fan(W)                            # a wide row of exactly W entries: staged
    if name == "fan_w1":
        return ir.fan(W + 1)                        # ... and of W + 1: in place
    if name == "one":
        return tr.diagonal(1)
    if name == "upper":
        return tr.mirror(tr.banded(2 * B + 3, 4, 32, rng))     # no entry below the diagonal
    raise KeyError(name)


STRUCTURES = ["full", "banded", "bidiagonal-", "bidiagonal", "bidiagonal+", "dense", "arrow", "fan_long", "fan_w", "fan_w1",
              "one", "upper"]


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """(pattern, values, lower levels) -- made once per session, shared, never written to."""
    pattern = _pattern(name)
    values, _ = ir.fill(pattern, dtype, np.random.default_rng(zlib.crc32(("ilu_sweep/" + name).encode())))
    nl = tr.levels(*pattern, lower=True)[1]
    for a in (*pattern[1:], values):
        a.setflags(write=False)
    return pattern, values, nl


@functools.lru_cache(maxsize=None)
def reference(name, dtype, s):
    """The swept factor by the host reference: computed once, shared, never written to."""
    pattern, values, _ = case(name, dtype)
    f = isr.ilu0_sweep_rows(*pattern, values, s)
    f.setflags(write=False)
    return f


def check_factor(f, pattern, ref, kind="csr"):
    """A downloaded factor (CsrMatrix / CscMatrix) has the operand's structure and the reference's bits."""
    n, rowptr, colind = pattern
    if kind == "csr":
        assert np.array_equal(f.rowptr(), rowptr) and np.array_equal(f.colind(), colind)
        ir.assert_same_bits(f.values(), ref)
    else:
        colptr, rowind, vals, _ = ir.to_csc(pattern, ref)
        assert np.array_equal(f.colptr(), colptr) and np.array_equal(f.rowind(), rowind)
        ir.assert_same_bits(f.values(), vals)


# ---- the hand examples ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_hand_examples(kind, dtype):
    for dense in (ir.HAND_A, ir.DROP_A):
        pattern, values = ir.dense_to_csr(dense, dtype)
        a = MAKERS[kind](pattern, values)
        for s in range(5):
            f = a.ilu0(sweeps=s)
            assert f.values().dtype == dtype
            check_factor(f, pattern, isr.ilu0_sweep_loop(*pattern, values, s), kind)
            d = f.device().describe()
            assert d["ilu0_sweep"]["sweeps"] == min(s, pattern[0] - 1) and d["ilu0_sweep"]["requested"] == s
    # four levels: three passes are the factor, two are not yet; A's values untouched
    pattern, values = ir.dense_to_csr(ir.HAND_A, dtype)
    a = csr(pattern, values)
    factor = ir.dense_to_csr(ir.HAND_F, dtype)[1]
    assert a.ilu0(sweeps=3).values().tolist() == factor.tolist()
    assert a.ilu0(sweeps=2).values().tolist() != factor.tolist()
    assert a.ilu0(sweeps=0).values().tolist() == values.tolist()
    assert a.device().download()[2].tolist() == values.tolist()
    pattern, values = ir.dense_to_csr(ir.DROP_A, dtype)
    assert csr(pattern, values).ilu0(sweeps=1).values().tolist() == ir.dense_to_csr(ir.DROP_F, dtype)[1].tolist()


# ---- structures -----------------------------------------------------------------------------------------------------

def test_the_structures_are_the_boundary_cases_they_are_meant_to_be():
    B, S, W = geometry()
    rp = lambda name: case(name, np.float64)[0][1].astype(np.int64)
    assert [case(n, np.float64)[0][0] for n in ("bidiagonal-", "bidiagonal", "bidiagonal+")] == [B - 1, B, B + 1]
    assert case("full", np.float64)[0][0] == 2 * B + 1 and case("banded", np.float64)[0][0] == 3 * B + 7
    a = rp("arrow")
    blocks = [a[min(r + B, a.size - 1)] - a[r] for r in range(0, a.size - 1, B)]
    assert blocks[0] > S and blocks[-1] > S and max(blocks[1:-1]) <= S         # two blocks cannot be staged whole
    assert np.diff(a).max() == S + 1
    assert [int(np.diff(rp(n)).max()) for n in ("fan_w", "fan_w1", "fan_long")] == [W, W + 1, W + 1025]
    assert ir.rows_with_lower_entries(case("upper", np.float64)[0]) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", STRUCTURES)
def test_structure_csr(name, dtype):
    B, S, W = geometry()
    pattern, values, nl = case(name, dtype)
    n, with_lower = pattern[0], ir.rows_with_lower_entries(pattern)
    dev = csr(pattern, values).device()
    for wide_work in (None, 0):     # the default threshold, then every row that can through the wide form
        if wide_work is not None:
            dev.set_option("ilu_wide_work", wide_work)
        for s in SWEEPS:
            f = dev.ilu0(sweeps=s)
            rp, ci, va = f.download()
            assert np.array_equal(rp, pattern[1]) and np.array_equal(ci, pattern[2])
            ir.assert_same_bits(va, reference(name, dtype, s))
            d = f.describe()
            assert "ilu0" not in d and set(d["ilu0_sweep"]) == KEYS
            d = d["ilu0_sweep"]
            assert d["sweeps"] == d["launches"] == min(s, n - 1) and d["requested"] == s
            assert (d["block_rows"], d["stage_entries"], d["wide_stage_entries"]) == (B, S, W)
            assert d["rows_row_form"] + d["rows_wide_form"] == n
            assert d["kernel_ms"] >= 0 and d["call_ms"] >= d["kernel_ms"]
            if d["sweeps"] >= 1:
                assert d["kernel_ms"] > 0
                if wide_work == 0:
                    assert d["rows_wide_form"] == with_lower and d["wide_work"] == 0
                else:
                    assert d["wide_work"] > 0
    ir.assert_same_bits(dev.download()[2], values)      # the operand is only read


@pytest.mark.parametrize("name", STRUCTURES)
def test_structure_csc(name):
    dtype = DTYPES[STRUCTURES.index(name) % 2]
    pattern, values, _ = case(name, dtype)
    a = csc(pattern, values)
    for s in (1, 2):
        check_factor(a.ilu0(sweeps=s), pattern, reference(name, dtype, s), "csc")


# ---- the options ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["full", "arrow", "fan_w", "fan_w1"])
def test_wide_work_settings_give_identical_bits(name, dtype):
    pattern, values, _ = case(name, dtype)
    n, with_lower = pattern[0], ir.rows_with_lower_entries(pattern)
    dev = csr(pattern, values).device()
    for wide_work in (None, 0, HUGE):       # the default first: the option stays where it was last put
        if wide_work is not None:
            dev.set_option("ilu_wide_work", wide_work)
        for s in (1, 2):
            f = dev.ilu0(sweeps=s)
            ir.assert_same_bits(f.download()[2], reference(name, dtype, s))
            d = f.describe()["ilu0_sweep"]
            if wide_work == 0:
                assert d["rows_wide_form"] == with_lower > 0 and d["rows_row_form"] == n - with_lower and d["wide_work"] == 0
            if wide_work == HUGE:
                assert (d["rows_wide_form"], d["rows_row_form"], d["wide_work"]) == (0, n, HUGE)
            if wide_work is None:
                assert d["wide_work"] > 0


# ---- equality with the exact call ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", STRUCTURES)
def test_levels_minus_one_sweeps_are_the_device_s_own_ilu0(name, dtype):
    pattern, values, nl = case(name, dtype)
    a = csr(pattern, values).device()
    exact = a.ilu0().download()[2]
    ir.assert_same_bits(a.ilu0(sweeps=nl - 1).download()[2], exact)
    if name in ("arrow", "fan_w") and nl >= 2:          # where rounding cannot hide a missing pass
        assert a.ilu0(sweeps=nl - 2).download()[2].tobytes() != exact.tobytes()


@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_a_huge_request_is_clamped_to_n_minus_one(kind):
    pattern = ir.sym(tr.banded(300, 5, 30, np.random.default_rng(5)))
    values, _ = ir.fill(pattern, np.float64, np.random.default_rng(6))
    a = MAKERS[kind](pattern, values).device()
    f = a.ilu0(sweeps=10 ** 12)
    d = f.describe()["ilu0_sweep"]
    assert d["sweeps"] == d["launches"] == 299 and d["requested"] == 10 ** 12
    ir.assert_same_bits(f.download()[2], a.ilu0().download()[2])
    exact = ir.ilu0_rows(*pattern, values)
    ir.assert_same_bits(f.download()[2], exact if kind == "csr" else ir.to_csc(pattern, exact)[2])


# ---- no analysis ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_nothing_is_analysed_and_the_factor_is_applied_by_sweeps(kind):
    pattern, values, _ = case("banded", np.float64)
    a = MAKERS[kind](pattern, values)
    dev = a.device()
    assert "trsv" not in dev.describe()
    f = a.ilu0(sweeps=2)
    d = dev.describe()
    assert "trsv" not in d and d.get("trsv", {}).get("analyses", 0) == 0
    assert "ilu0_sweep" not in d and "ilu0" not in d
    df = f.device().describe()
    assert "ilu0_sweep" in df and "ilu0" not in df and "trsv" not in df
    ref = reference("banded", np.float64, 2)
    b = np.random.default_rng(21).uniform(-1, 1, size=pattern[0])
    y = f.solve_triangular(b, lower=True, unit_diagonal=True, sweeps=3)
    sw.assert_same_bits(y, sw.sweep_vec(*pattern, ref, b, 3, True, True))
    sw.assert_same_bits(f.solve_triangular(y, lower=False, sweeps=3), sw.sweep_vec(*pattern, ref, y, 3, False))
    assert "trsv" not in f.device().describe() and "trsv" not in dev.describe()
    # an exact solve on the factor analyses as usual
    tr.assert_same_bits(f.solve_triangular(b, lower=True, unit_diagonal=True),
                        tr.solve_loop(*pattern, ref, b, lower=True, unit=True))
    assert f.device().describe()["trsv"]["analyses"] == 1
    # ... and the exact factorisation of the operand analyses it, as it always did
    ir.assert_same_bits(dev.ilu0().download()[2], a.ilu0().values())
    assert dev.describe()["trsv"]["analyses"] == 1


# ---- solvers ----------------------------------------------------------------------------------------------------------------

TOL = {np.float64: 1e-10, np.float32: 1e-5}
MAXIT = 120


@functools.lru_cache(maxsize=None)
def solver_case(method, dtype):
    """(pattern, values, b, the reference's factor of three sweeps): CG on an SPD banded matrix, BiCGStab and GMRES on an
    unsymmetric banded one.  Shared, read-only."""
    rng = np.random.default_rng(zlib.crc32(("ilu_sweep/" + method).encode()))
    pattern = ir.sym(tr.banded(351, 4, 40, rng))
    values, b = (kr.spd_fill if method == "cg" else tr.fill)(pattern, dtype, rng)
    f = isr.ilu0_sweep_rows(*pattern, values, 3)
    for a in (*pattern[1:], values, b, f):
        a.setflags(write=False)
    return pattern, values, b, f


def same_result(got, ref):
    x, info = got
    xr, ir_ = ref
    sw.assert_same_bits(x, xr)
    assert (info.iterations, info.reason) == (ir_["iterations"], ir_["reason"])
    sw.assert_same_bits(np.array([info.residual_sq]), np.array([ir_["residual_sq"]]))
    sw.assert_same_bits(np.array([info.rhs_sq]), np.array([ir_["rhs_sq"]]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("method", ["cg", "bicgstab", "gmres"])
def test_solvers_preconditioned_by_the_swept_factor(method, kind, dtype):
    pattern, values, b, f = solver_case(method, dtype)
    a = MAKERS[kind](pattern, values)
    m = a.ilu0(sweeps=3)
    check_factor(m, pattern, f, kind)
    mul, prec = (lambda v: a.device().spmv(v)), sw.preconditioner(pattern, f, 3)
    if method == "gmres":
        got = a.gmres(b, M=m, restart=5, tol=TOL[dtype], maxit=MAXIT, precond_sweeps=3)
        ref = gr.gmres(mul, prec, b, np.zeros_like(b), 5, TOL[dtype], MAXIT)
    else:
        got = a.solve(b, method, M=m, tol=TOL[dtype], maxit=MAXIT, precond_sweeps=3)
        ref = kr.METHODS[method](mul, prec, b, np.zeros_like(b), TOL[dtype], MAXIT)
    same_result(got, ref)
    assert got[1].reason == 0 and 0 < got[1].iterations < MAXIT
    # SpMV-shaped from start to finish: neither handle was analysed
    assert "trsv" not in m.device().describe() and "trsv" not in a.device().describe()
    assert a.device().describe()["gmres" if method == "gmres" else "krylov"]["precond_sweeps"] == 3


# ---- refusals -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_refusals_leave_the_operand_usable_and_null_out(kind):
    make = MAKERS[kind]
    cls = sp.CsrMatrix if kind == "csr" else sp.CscMatrix
    fn = getattr(_ffi.lib(), f"spal_{kind}_ilu0_sweep")
    rect = cls(2, 3, [0, 1, 2] if kind == "csr" else [0, 1, 2, 2], [0, 1], np.array([1.0, 2.0])).device()
    out = C.c_void_p(0x1234)     # (never dereferenced: a refused call nulls its out, as ilu0 does)
    assert fn(rect._h, C.c_uint64(2), None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT and out.value is None
    with pytest.raises(sp.Panic, match=r"not square \(2 x 3\)"):
        rect.ilu0(sweeps=2)
    pattern = tr.drop_diagonal(tr.drop_diagonal(ir.full(900, 4, np.random.default_rng(18)), 700), 7)
    values, x = ir.fill(pattern, np.float64, np.random.default_rng(19))
    dev = make(pattern, values).device()
    y = dev.spmv(x)
    for s in (0, 2):
        out = C.c_void_p(0x1234)
        assert fn(dev._h, C.c_uint64(s), None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT and out.value is None
        with pytest.raises(sp.Panic, match=f"spal_{kind}_ilu0_sweep: row 7 stores no diagonal entry"):
            dev.ilu0(sweeps=s)
    assert fn(dev._h, C.c_uint64(2), None, None) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert b"null argument" in _ffi.lib().spal_last_error()
    ir.assert_same_bits(dev.spmv(x), y)                  # the operand multiplies as it did before the refusals
    ir.assert_same_bits(make(pattern, values).device().spmv(x), y)


# ---- IEEE -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_zero_pivot_gives_the_reference_inf_and_nan(kind, dtype):
    # every entry stored, a 0.0 at (0, 0): rows 1 and 2 divide by it
    pattern = tr.from_coo(3, np.repeat(np.arange(3), 3), np.tile(np.arange(3), 3))
    values = np.array([0, 1, 1, 1, 1, 1, 1, 1, 1], dtype=dtype)
    a = MAKERS[kind](pattern, values)
    for wide_work in (None, 0):
        if wide_work is not None:
            a.device().set_option("ilu_wide_work", wide_work)
        for s in (1, 2):
            ref = isr.ilu0_sweep_loop(*pattern, values, s)
            assert np.isinf(ref).any() and np.isnan(ref).any() and np.isfinite(ref).any()
            check_factor(a.ilu0(sweeps=s), pattern, ref, kind)          # status SPAL_OK: no exception


# ---- handles built on the device ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_device_assembled_operand_with_a_swept_ilu0_as_its_first_call(dtype):
    pattern, values, _ = case("full", dtype)
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rowptr.astype(np.int64)))
    perm = np.random.default_rng(17).permutation(colind.size)
    coo = sp.CooMatrix.with_triplets(n, n, rows[perm], colind[perm], values[perm])
    assembled = sp.CsrMatrix.from_coo(coo)
    f = assembled.ilu0(sweeps=2)
    check_factor(f, pattern, reference("full", dtype, 2))
    x = np.random.default_rng(23).uniform(-1, 1, size=n).astype(dtype)
    ir.assert_same_bits(assembled * x, csr(pattern, values) * x)     # its first product comes after, and plans then


# ---- threads ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_two_threads_sweep_one_fresh_handle(kind):
    pattern, values, _ = case("banded", np.float64)
    ref = reference("banded", np.float64, 2)
    dev = MAKERS[kind](pattern, values).device()
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i):
        try:
            gate.wait(timeout=30)
            results[i] = dev.ilu0(sweeps=2).download()[2]
        except Exception as e:          # reported below, from the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "a thread did not return from its factorisation"
    assert not errors, errors
    expect = ref if kind == "csr" else ir.to_csc(pattern, ref)[2]
    ir.assert_same_bits(results[0], expect)
    ir.assert_same_bits(results[1], expect)
    d = dev.describe()
    assert d["trsv_sweep"]["prepared"] == 1 and d["trsv_sweep"]["calls"] == 0 and "trsv" not in d


# ---- a short seeded fuzz ------------------------------------------------------------------------------------------------------

def _fuzz_pattern(rng):
    """A random pattern that stores its diagonal: short rows with columns near and far, and a few long rows."""
    n = int(rng.integers(1, 2001))
    per = int(rng.integers(1, 9))
    i = np.repeat(np.arange(n, dtype=np.int64), per)
    near = np.clip(i + rng.integers(-40, 41, size=i.size), 0, n - 1)
    far = rng.integers(0, n, size=i.size)
    j = np.where(rng.random(i.size) < 0.8, near, far)
    rows, cols = [i], [j]
    for r in rng.integers(0, n, size=int(rng.integers(0, 4))):
        cnt = int(rng.integers(1, n + 1))
        rows.append(np.full(cnt, r, dtype=np.int64))
        cols.append(rng.choice(n, size=cnt, replace=False))
    return tr._with_diag(n, np.concatenate(rows), np.concatenate(cols))


@pytest.mark.parametrize("seed", range(16))
def test_fuzz(seed):
    rng = np.random.default_rng(20261019 + seed)
    pattern = _fuzz_pattern(rng)
    dtype = DTYPES[seed % 2]
    kind = ("csr", "csr", "csc")[seed % 3]
    s = int(rng.integers(0, 5))
    wide_work = (None, 0, 64, 1024)[int(rng.integers(0, 4))]
    values, _ = ir.fill(pattern, dtype, rng)
    a = MAKERS[kind](pattern, values)
    if wide_work is not None:
        a.device().set_option("ilu_wide_work", wide_work)
    check_factor(a.ilu0(sweeps=s), pattern, isr.ilu0_sweep_rows(*pattern, values, s), kind)
