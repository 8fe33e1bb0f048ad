"""ILU(0) on the device against its sequential definition (tests/ilu_ref.py): raw bits equal, NaN by position, f64 and
f32, CSR and CSC, whatever the schedule is.

Matrices come from trsv_ref.fill: rows strictly diagonally dominant, which ILU(0) preserves, so the factors are finite
and comparing bits is meaningful.  Sizes are the smallest that cross a boundary of the code: levels wider than a
workgroup of the level kernel (256) and of the chain kernel (1024), widths 1023 / 1024 / 1025 / 2049, thousands of
one-row levels, rows of thousands of entries on either side of the diagonal, one row longer than the wide form's LDS
staging capacity, and both row forms of every structure."""
import ctypes as C
import functools
import threading
import zlib

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import ilu_ref as ir
from tests import trsv_ref as tr

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
HUGE = 1 << 40
STAGE = 256          # entries of a wide row staged in LDS (describe()["ilu0"]["lds_stage_entries"], asserted below)


def _pattern(name):
    rng = np.random.default_rng(20261018)
    if name == "full":
        return ir.full(4000, 6, rng)                                  # 18 levels, widest 565: levels above 256 rows are launches
    if name == "banded":
        return ir.sym(tr.banded(6007, 6, 512, rng))                   # narrow levels: chains
    if name == "bidiagonal":
        return ir.sym(tr.bidiagonal(5000))                            # 5000 one-row levels
    if name == "prescribed":
        return ir.sym(tr.prescribed(tr.PRESCRIBED_WIDTHS, rng))       # level widths 1023 / 1024 / 1025 / 2049
    if name == "dense":
        return ir.sym(tr.dense_triangle(120))                         # every row reads every earlier row
    if name == "arrow":
        return ir.sym(tr.arrow(3000))                                 # U-parts and L-parts of thousands of entries
    if name == "fan":
        return ir.fan(STAGE + 1025)                                   # one row too long to stage: updated in place
    if name == "one":
        return tr.diagonal(1)
    raise KeyError(name)


STRUCTURES = ["full", "banded", "bidiagonal", "prescribed", "dense", "arrow", "fan", "one"]


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """(pattern, values, reference factor) -- computed once per session, shared, never written to."""
    pattern = _pattern(name)
    values, _ = ir.fill(pattern, dtype, np.random.default_rng(zlib.crc32(name.encode())))
    ref = ir.ilu0_rows(*pattern, values)
    assert np.isfinite(ref).all()
    for a in (*pattern[1:], values, ref):
        a.setflags(write=False)
    return pattern, values, ref


def csr(pattern, values):
    n, rowptr, colind = pattern
    return sp.CsrMatrix(n, n, rowptr, colind, values)


def csc(pattern, values):
    n = pattern[0]
    colptr, rowind, vals, _ = ir.to_csc(pattern, values)
    return sp.CscMatrix(n, n, colptr, rowind, vals)


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
    make = csr if kind == "csr" else csc
    for dense, factor in ((ir.HAND_A, ir.HAND_F), (ir.DROP_A, ir.DROP_F)):
        pattern, values = ir.dense_to_csr(dense, dtype)
        f = make(pattern, values).ilu0()
        expect = ir.dense_to_csr(factor, dtype)[1]
        check_factor(f, pattern, expect, kind)
        assert f.values().dtype == dtype
        if kind == "csr":
            assert f.values().tolist() == expect.tolist()
    # b = A [1, 2, 1, 3]: the lower-unit solve, then the upper solve, on the one result handle
    pattern, values = ir.dense_to_csr(ir.HAND_A, dtype)
    f = make(pattern, values).ilu0()
    b = np.array([4, 9, -4, 5], dtype=dtype)
    y = f.solve_triangular(b, lower=True, unit_diagonal=True)
    assert y.tolist() == [4, 1, -1, 9]
    assert f.solve_triangular(y, lower=False).tolist() == [1, 2, 1, 3]


# ---- structures -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", STRUCTURES)
def test_structure_csr(name, dtype):
    pattern, values, ref = case(name, dtype)
    dev = csr(pattern, values).device()
    level_of, nl = tr.levels(*pattern, lower=True)
    if name == "prescribed":
        assert tuple(tr.level_widths(level_of, nl)) == tr.PRESCRIBED_WIDTHS
    for wide_work in (None, 0):     # the default threshold, then every row that can through the wide form
        if wide_work is not None:
            dev.set_option("ilu_wide_work", wide_work)
        f = dev.ilu0()
        rp, ci, va = f.download()
        assert np.array_equal(rp, pattern[1]) and np.array_equal(ci, pattern[2])
        ir.assert_same_bits(va, ref)
        d = f.describe()["ilu0"]
        assert d["levels"] == nl and d["lds_stage_entries"] == STAGE
        assert d["rows_row_form"] + d["rows_wide_form"] == pattern[0]
        assert d["launches"] >= 1 and d["kernel_ms"] > 0 and d["call_ms"] >= d["kernel_ms"]
        if wide_work == 0:
            assert d["rows_wide_form"] == ir.rows_with_lower_entries(pattern)
    if name == "fan":   # the one row with entries below the diagonal is too long to stage: updated in place
        assert int(np.diff(pattern[1].astype(np.int64)).max()) == STAGE + 1025 and d["rows_wide_form"] == 1


@pytest.mark.parametrize("name", STRUCTURES[::2])
def test_structure_csc(name):
    pattern, values, ref = case(name, np.float64)
    f = csc(pattern, values).ilu0()
    check_factor(f, pattern, ref, "csc")
    assert f.device().describe()["ilu0"]["levels"] == tr.levels(*pattern, lower=True)[1]


# ---- the schedule ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["full", "arrow"])
def test_schedule_settings_give_identical_bits(name):
    pattern, values, ref = case(name, np.float64)
    dev = csr(pattern, values).device()
    n, with_lower = pattern[0], ir.rows_with_lower_entries(pattern)
    for wide_work in (None, 0, HUGE):       # the default first: the option stays where it was last put
        if wide_work is not None:
            dev.set_option("ilu_wide_work", wide_work)
        for chain_rows in (0, 256, HUGE):
            dev.set_option("trsv_chain_rows", chain_rows)
            f = dev.ilu0()
            ir.assert_same_bits(f.download()[2], ref)
            d = f.describe()["ilu0"]
            assert d["chain_rows"] == chain_rows
            if chain_rows == 0:
                assert d["launches"] == d["levels"] and d["chain_launches"] == 0
            if chain_rows == HUGE:
                assert d["launches"] == 1 and d["chain_launches"] == 1
            # rows in both forms, whichever way the threshold is forced
            if wide_work == 0:
                assert (d["rows_wide_form"], d["rows_row_form"]) == (with_lower, n - with_lower)
            if wide_work == HUGE:
                assert (d["rows_wide_form"], d["rows_row_form"]) == (0, n)
            if wide_work is None:
                assert d["wide_work"] > 0
    assert dev.describe()["trsv"]["analyses"] == 1      # nine factorisations, one analysis
    with pytest.raises(sp.Panic, match="ilu_wide_work must be >= 0"):
        dev.set_option("ilu_wide_work", -1)


def test_wide_form_through_a_csc_handle():
    pattern, values, ref = case("banded", np.float64)
    a = csc(pattern, values)
    a.device().set_option("ilu_wide_work", 0)
    f = a.device().ilu0()
    d = f.describe()["ilu0"]
    assert d["rows_wide_form"] == ir.rows_with_lower_entries(pattern) and d["wide_work"] == 0
    ir.assert_same_bits(f.download()[2], ir.to_csc(pattern, ref)[2])


# ---- plans ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_plans_are_built_once_and_handed_to_the_factor(kind):
    pattern, values, ref = case("full", np.float64)
    dev = (csr if kind == "csr" else csc)(pattern, values).device()
    assert "trsv" not in dev.describe()
    f = dev.ilu0()
    da = dev.describe()["trsv"]
    assert da["analyses"] == 1 and "upper" not in da
    df = f.describe()["trsv"]                            # before any solve on the factor
    assert df["analyses"] == 0 and "upper" not in df
    for key in ("levels", "max_level_rows", "launches", "chain_launches", "chain_rows"):
        assert df["lower"][key] == da["lower"][key]
    r = np.random.default_rng(21).uniform(-1, 1, size=pattern[0])
    y = f.trsv(r, lower=True, unit_diagonal=True)
    assert f.describe()["trsv"]["analyses"] == 0         # the copied plan served it
    z = f.trsv(y, lower=False)
    assert f.describe()["trsv"]["analyses"] == 1         # the upper plan is the factor's own
    y_ref = tr.solve_loop(*pattern, ref, r, lower=True, unit=True)
    ir.assert_same_bits(y, y_ref)
    ir.assert_same_bits(z, tr.solve_loop(*pattern, ref, y_ref, lower=False))
    # again: the same bits, nothing analysed
    g = dev.ilu0()
    ir.assert_same_bits(g.download()[2], f.download()[2])
    assert dev.describe()["trsv"]["analyses"] == 1
    # the operand is what it was
    rp, ci, va = dev.download()
    expect = values if kind == "csr" else ir.to_csc(pattern, values)[2]
    ir.assert_same_bits(va, expect)


# ---- IEEE -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_zero_pivot_gives_the_reference_inf_and_nan(kind, dtype):
    # every entry stored, a 0.0 at (0, 0): rows 1 and 2 divide by it
    pattern = tr.from_coo(3, np.repeat(np.arange(3), 3), np.tile(np.arange(3), 3))
    values = np.array([0, 1, 1, 1, 1, 1, 1, 1, 1], dtype=dtype)
    ref = ir.ilu0_loop(*pattern, values)
    assert np.isinf(ref).any() and np.isnan(ref).any() and np.isfinite(ref).any()
    f = (csr if kind == "csr" else csc)(pattern, values).ilu0()          # status SPAL_OK: no exception
    check_factor(f, pattern, ref, kind)


# ---- refusals -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_refusals_leave_the_operand_usable_and_null_out(kind):
    make = csr if kind == "csr" else csc
    cls = sp.CsrMatrix if kind == "csr" else sp.CscMatrix
    fn = getattr(_ffi.lib(), f"spal_{kind}_ilu0")
    rect = cls(2, 3, [0, 1, 2] if kind == "csr" else [0, 1, 2, 2], [0, 1], np.array([1.0, 2.0])).device()
    out = C.c_void_p(0x1234)     # (never dereferenced: a refused call nulls its out, as mul / add / sub / neg do)
    assert fn(rect._h, None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT and out.value is None
    with pytest.raises(sp.Panic, match=r"not square \(2 x 3\)"):
        rect.ilu0()
    pattern = tr.drop_diagonal(tr.drop_diagonal(ir.full(900, 4, np.random.default_rng(18)), 700), 7)
    values, x = ir.fill(pattern, np.float64, np.random.default_rng(19))
    dev = make(pattern, values).device()
    y = dev.spmv(x)
    out = C.c_void_p(0x1234)
    assert fn(dev._h, None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT and out.value is None
    with pytest.raises(sp.Panic, match=f"spal_{kind}_ilu0: row 7 stores no diagonal entry"):
        dev.ilu0()
    assert fn(dev._h, None, None) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert b"null argument" in _ffi.lib().spal_last_error()
    ir.assert_same_bits(dev.spmv(x), y)                  # the operand multiplies as it did before the refusals
    ir.assert_same_bits(make(pattern, values).device().spmv(x), y)


# ---- handles built on the device ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_device_assembled_operand_with_ilu0_as_its_first_call(dtype):
    pattern, values, ref = case("full", dtype)
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rowptr.astype(np.int64)))
    perm = np.random.default_rng(17).permutation(colind.size)
    coo = sp.CooMatrix.with_triplets(n, n, rows[perm], colind[perm], values[perm])
    assembled = sp.CsrMatrix.from_coo(coo)
    f = assembled.ilu0()
    check_factor(f, pattern, ref)
    x = np.random.default_rng(23).uniform(-1, 1, size=n).astype(dtype)
    ir.assert_same_bits(assembled * x, csr(pattern, values) * x)     # its first product comes after, and plans then


# ---- threads --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_two_threads_factorise_one_fresh_handle(kind):
    pattern, values, ref = case("banded", np.float64)
    dev = (csr if kind == "csr" else csc)(pattern, values).device()
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i):
        try:
            gate.wait(timeout=30)
            results[i] = dev.ilu0().download()[2]
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
    assert dev.describe()["trsv"]["analyses"] == 1
