"""Sparse triangular solve on the device against its sequential definition (tests/trsv_ref.py): raw bits equal, NaN by
position, for f64 and f32, lower and upper, CSR and CSC, whatever the launch schedule is.

Matrices come from trsv_ref.fill: values and b in (-1, 1), d_i = 1 + sum |off-diagonal|, so |x| <= max |b| and comparing
bits is meaningful.  Sizes are the smallest that cross a boundary of the code: a level wider than a workgroup of the
level kernel (256) and of the chain kernel (1024), widths 1023 / 1024 / 1025 / 2049, thousands of one-row levels, one
row of 20 000 entries, levels on both sides of the default trsv_chain_rows."""
import functools
import threading
import zlib

import numpy as np
import pytest

import spalinalg_amd as sp
from tests import trsv_ref as tr
from tests.test_trsv_host import HAND_L, dense_to_csr

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
HUGE = 1 << 40


def _lower_pattern(name):
    rng = np.random.default_rng(20261017)
    if name == "diagonal":
        return tr.diagonal(3000)                      # one level, wider than a workgroup
    if name == "bidiagonal":
        return tr.bidiagonal(5000)                    # 5000 levels of one row
    if name == "dense":
        return tr.dense_triangle(300)                 # row lengths 0 .. 299
    if name == "banded":
        return tr.banded(20011, 6, 512, rng)          # 7 entries in a window of 512: about 1000 narrow levels
    if name == "arrow":
        return tr.arrow(20000)                        # one row of 20 000 entries, one level of 19 998 rows
    if name == "chains":
        return tr.chains(np.concatenate([rng.integers(1, 41, size=1500), [200]]))   # 1501 rows narrowing to one
    if name == "prescribed":
        return tr.prescribed(tr.PRESCRIBED_WIDTHS, rng)
    if name == "one":
        return tr.diagonal(1)
    raise KeyError(name)


STRUCTURES = ["diagonal", "bidiagonal", "dense", "banded", "arrow", "chains", "prescribed", "one"]


@functools.lru_cache(maxsize=None)
def case(name, lower, dtype):
    """(pattern, values, b, reference x) -- computed once per session, shared, never written to."""
    pattern = _lower_pattern(name)
    if not lower:
        pattern = tr.mirror(pattern)
    values, b = tr.fill(pattern, dtype, np.random.default_rng(zlib.crc32(f"{name}/{lower}".encode())))
    ref = tr.solve_loop(*pattern, values, b, lower=lower)
    for a in (*pattern[1:], values, b, ref):
        a.setflags(write=False)
    return pattern, values, b, ref


def csr(pattern, values):
    n, rowptr, colind = pattern
    return sp.CsrMatrix(n, n, rowptr, colind, values)


def csc(pattern, values):
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    order = np.lexsort((rows, colind.astype(np.int64)))
    colptr = np.concatenate([[0], np.cumsum(np.bincount(colind.astype(np.int64), minlength=n))]).astype(np.uint64)
    return sp.CscMatrix(n, n, colptr, rows[order].astype(np.uint64), values[order])


# ---- the hand example -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("make", [csr, csc], ids=["csr", "csc"])
def test_hand_example(make, dtype):
    n, rp, ci, v = dense_to_csr(HAND_L, dtype)
    lo = make((n, rp, ci), v)
    n, rp, ci, v = dense_to_csr(HAND_L.T, dtype)
    up = make((n, rp, ci), v)
    bl, bu = np.array([2, 3, 10, 9], dtype=dtype), np.array([7, 5, 10, 6], dtype=dtype)
    assert lo.solve_triangular(bl).tolist() == [1, 2, 1, 3]
    assert up.solve_triangular(bu, lower=False).tolist() == [1, 2, 1, 3]
    assert lo.solve_triangular(bl, unit_diagonal=True).tolist() == [2, 1, 7, -7]
    assert up.solve_triangular(bu, lower=False, unit_diagonal=True).tolist() == [-10, 11, -2, 6]
    # the other triangle of each is its diagonal alone
    assert lo.solve_triangular(bl, lower=False).tolist() == [1, 3, 2.5, 4.5]
    assert up.solve_triangular(bu, lower=True, unit_diagonal=True).tolist() == bu.tolist()
    assert lo.solve_triangular(bl).dtype == dtype


# ---- structures ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("name", STRUCTURES)
def test_structure_csr(name, lower, dtype):
    pattern, values, b, ref = case(name, lower, dtype)
    a = csr(pattern, values)
    tr.assert_same_bits(a.solve_triangular(b, lower=lower), ref)
    d = a.device().describe()["trsv"]["lower" if lower else "upper"]
    level_of, nl = tr.levels(*pattern, lower=lower)
    assert d["levels"] == nl
    assert d["max_level_rows"] == max(tr.level_widths(level_of, nl))
    if name == "prescribed":
        assert d["levels"] == len(tr.PRESCRIBED_WIDTHS) and d["max_level_rows"] == 2049
    assert a.device().describe()["trsv"]["analyses"] == 1


@pytest.mark.parametrize("name", STRUCTURES)
def test_structure_csc(name):
    lower = STRUCTURES.index(name) % 2 == 0
    pattern, values, b, ref = case(name, lower, np.float64)
    a = csc(pattern, values)
    tr.assert_same_bits(a.solve_triangular(b, lower=lower), ref)
    assert a.device().describe()["trsv"]["lower" if lower else "upper"]["levels"] == tr.levels(*pattern, lower=lower)[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_full_matrix_both_triangles_on_one_handle(dtype):
    pattern = tr.full(4000, 6, np.random.default_rng(5))
    values, b = tr.fill(pattern, dtype, np.random.default_rng(6))
    a = csr(pattern, values)
    dev = a.device()
    assert "trsv" not in dev.describe()
    xl, xu = a.solve_triangular(b, lower=True), a.solve_triangular(b, lower=False)
    tr.assert_same_bits(xl, tr.solve_loop(*pattern, values, b, lower=True))
    tr.assert_same_bits(xu, tr.solve_loop(*pattern, values, b, lower=False))
    d = dev.describe()["trsv"]
    assert d["analyses"] == 2 and d["lower"]["levels"] > 1 and d["upper"]["levels"] > 1
    # both plans are cached: the second solves analyse nothing and return the same bits
    tr.assert_same_bits(a.solve_triangular(b, lower=True), xl)
    tr.assert_same_bits(a.solve_triangular(b, lower=False), xu)
    d2 = dev.describe()["trsv"]
    assert d2 == d
    # a symmetric Gauss-Seidel sweep's two halves, with the unit diagonal too
    tr.assert_same_bits(a.solve_triangular(b, lower=False, unit_diagonal=True),
                        tr.solve_loop(*pattern, values, b, lower=False, unit=True))
    assert dev.describe()["trsv"]["analyses"] == 2


def test_banded_200003_rows_by_the_level_form_of_the_reference():
    pattern = tr.banded(200003, 6, 4096, np.random.default_rng(8))
    values, b = tr.fill(pattern, np.float64, np.random.default_rng(9))
    a = csr(pattern, values)
    x = a.solve_triangular(b)
    tr.assert_same_bits(x, tr.solve_by_levels(*pattern, values, b, lower=True))
    d = a.device().describe()["trsv"]["lower"]
    assert d["levels"] > 500 and d["launches"] < d["levels"]


# ---- the schedule ----------------------------------------------------------------------------------------------

def expected_launches(widths, chain_rows):
    """(launches, chain launches): maximal runs of levels of at most chain_rows rows are one chain launch each, every
    wider level is a launch of its own."""
    wide = [w > chain_rows for w in widths]
    runs = sum(1 for i, w in enumerate(wide) if not w and (i == 0 or wide[i - 1]))
    return runs + sum(wide), runs


@pytest.mark.parametrize("name", ["bidiagonal", "prescribed", "chains", "banded"])
def test_schedule_settings_give_identical_bits(name):
    lower = name != "chains"
    pattern, values, b, ref = case(name, lower, np.float64)
    key = "lower" if lower else "upper"
    dev = csr(pattern, values).device()
    widths = tr.level_widths(*tr.levels(*pattern, lower=lower))
    tr.assert_same_bits(dev.trsv(b, lower), ref)                    # the default
    d = dev.describe()["trsv"][key]
    assert d["chain_rows"] >= 1
    assert (d["launches"], d["chain_launches"]) == expected_launches(widths, d["chain_rows"])
    if name == "bidiagonal":
        assert d["launches"] == 1
    dev.set_option("trsv_chain_rows", 0)
    tr.assert_same_bits(dev.trsv(b, lower), ref)
    d = dev.describe()["trsv"][key]
    assert d["launches"] == d["levels"] == len(widths) and d["chain_launches"] == 0 and d["chain_rows"] == 0
    dev.set_option("trsv_chain_rows", HUGE)
    tr.assert_same_bits(dev.trsv(b, lower), ref)
    d = dev.describe()["trsv"][key]
    assert d["launches"] == 1 and d["chain_launches"] == 1
    # a threshold inside the widths: the 1024-row level still goes to the chain kernel, the 1025-row one does not
    dev.set_option("trsv_chain_rows", 1024)
    tr.assert_same_bits(dev.trsv(b, lower), ref)
    d = dev.describe()["trsv"][key]
    assert (d["launches"], d["chain_launches"]) == expected_launches(widths, 1024)
    if name == "prescribed":
        assert (d["launches"], d["chain_launches"]) == (5, 3)
    assert dev.describe()["trsv"]["analyses"] == 1                  # the option re-records launches, it analyses nothing
    with pytest.raises(sp.Panic, match="trsv_chain_rows must be >= 0"):
        dev.set_option("trsv_chain_rows", -1)


def test_wide_level_between_narrow_ones_is_a_launch_of_its_own():
    pattern, values, b, ref = case("arrow", True, np.float64)       # levels of 1, 19 998 and 1 rows
    dev = csr(pattern, values).device()
    dev.set_option("trsv_chain_rows", 4096)
    tr.assert_same_bits(dev.trsv(b), ref)
    d = dev.describe()["trsv"]["lower"]
    assert (d["levels"], d["launches"], d["chain_launches"], d["max_level_rows"]) == (3, 3, 2, 19998)


def test_option_through_a_csc_handle():
    pattern, values, b, ref = case("prescribed", True, np.float64)
    dev = csc(pattern, values).device()
    dev.set_option("trsv_chain_rows", 0)
    tr.assert_same_bits(dev.trsv(b), ref)
    d = dev.describe()["trsv"]["lower"]
    assert d["launches"] == d["levels"] == len(tr.PRESCRIBED_WIDTHS)


# ---- device pointers -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_device_path_in_place_out_of_place_stream_and_back_to_back(dtype):
    import torch
    pattern = tr.full(6000, 5, np.random.default_rng(11))
    values, b = tr.fill(pattern, dtype, np.random.default_rng(12))
    dev = csr(pattern, values).device()
    xl = tr.solve_loop(*pattern, values, b, lower=True)
    xlu = tr.solve_loop(*pattern, values, xl, lower=False)
    bt = torch.from_numpy(b).cuda()
    out = torch.full_like(bt, float("nan"))
    torch.cuda.synchronize()
    # out of place, default stream: b stays as it was
    dev.trsv_dev(bt.data_ptr(), out.data_ptr(), True, False)
    torch.cuda.synchronize()
    tr.assert_same_bits(out.cpu().numpy(), xl)
    tr.assert_same_bits(bt.cpu().numpy(), b)
    # in place, on a stream of the caller's; then the upper solve right behind it, nothing synchronised in between
    st = torch.cuda.Stream()
    dev.trsv_analyse(lower=False, stream=st)
    work = bt.clone()
    torch.cuda.synchronize()
    dev.trsv_dev(work.data_ptr(), work.data_ptr(), True, False, st)
    dev.trsv_dev(work.data_ptr(), work.data_ptr(), False, False, st)
    st.synchronize()
    tr.assert_same_bits(work.cpu().numpy(), xlu)
    assert dev.describe()["trsv"]["analyses"] == 2


# ---- IEEE ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_zero_diagonal_gives_the_reference_inf_and_nan(lower, dtype):
    n = 3001
    pattern = tr.banded(n, 6, 64, np.random.default_rng(13))
    if not lower:
        pattern = tr.mirror(pattern)
    values, b = tr.fill(pattern, dtype, np.random.default_rng(14))
    _, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    isd = rows == colind.astype(np.int64)
    values[~isd] /= 8        # sum |off-diagonal| < 0.75 per row: the unit-diagonal solve stays bounded by 4 max |b|
    values[isd & (rows == n // 2)] = 0
    a = csr(pattern, values)
    ref = tr.solve_loop(*pattern, values, b, lower=lower)
    assert np.isinf(ref[n // 2]) and np.isnan(ref).any() and np.isfinite(ref).any()
    tr.assert_same_bits(a.solve_triangular(b, lower=lower), ref)
    unit = a.solve_triangular(b, lower=lower, unit_diagonal=True)
    assert np.isfinite(unit).all()
    tr.assert_same_bits(unit, tr.solve_loop(*pattern, values, b, lower=lower, unit=True))


# ---- handles built on the device ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_handles_built_on_the_device_solve_like_uploaded_ones(dtype):
    pattern = tr.full(5000, 5, np.random.default_rng(15))
    values, b = tr.fill(pattern, dtype, np.random.default_rng(16))
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rowptr.astype(np.int64)))
    perm = np.random.default_rng(17).permutation(colind.size)
    coo = sp.CooMatrix.with_triplets(n, n, rows[perm], colind[perm], values[perm])
    assembled = sp.CsrMatrix.from_coo(coo)
    assert np.array_equal(assembled.rowptr(), rowptr) and np.array_equal(assembled.colind(), colind)
    host = csr(pattern, values)
    doubled = host + host                      # the device handle of a sum; 2A keeps the dominance of fill()
    for lower in (True, False):
        ref = tr.solve_loop(*pattern, values, b, lower=lower)
        tr.assert_same_bits(assembled.solve_triangular(b, lower=lower), ref)
        tr.assert_same_bits(host.solve_triangular(b, lower=lower), ref)
        ref2 = tr.solve_loop(*pattern, doubled.values(), b, lower=lower)
        tr.assert_same_bits(doubled.solve_triangular(b, lower=lower), ref2)
        tr.assert_same_bits(csr(pattern, doubled.values()).solve_triangular(b, lower=lower), ref2)


# ---- threads -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("make", [csr, csc], ids=["csr", "csc"])
def test_two_threads_take_the_first_solve_of_a_fresh_handle(make):
    pattern, values, b, ref = case("banded", True, np.float64)
    b2 = np.ascontiguousarray(b[::-1])
    ref2 = tr.solve_loop(*pattern, values, b2, lower=True)
    dev = make(pattern, values).device()
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i, rhs):
        try:
            gate.wait(timeout=30)
            results[i] = dev.trsv(rhs)
        except Exception as e:          # reported below, from the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(0, b), daemon=True),
               threading.Thread(target=work, args=(1, b2), daemon=True)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "a thread did not return from its first solve"
    assert not errors, errors
    tr.assert_same_bits(results[0], ref)
    tr.assert_same_bits(results[1], ref2)
    assert dev.describe()["trsv"]["analyses"] == 1


# ---- errors ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_errors_through_the_binding_leave_the_handle_usable(kind):
    make = csr if kind == "csr" else csc
    cls = sp.CsrMatrix if kind == "csr" else sp.CscMatrix
    rect = cls(2, 3, [0, 1, 2] if kind == "csr" else [0, 1, 2, 2], [0, 1], np.array([1.0, 2.0])).device()
    with pytest.raises(sp.Panic, match=r"not square \(2 x 3\)"):
        rect.trsv(np.ones(2))
    with pytest.raises(sp.Panic, match="not square"):
        rect.trsv_analyse()
    pattern = tr.drop_diagonal(tr.drop_diagonal(tr.full(900, 4, np.random.default_rng(18)), 700), 333)
    values, b = tr.fill(pattern, np.float64, np.random.default_rng(19))
    values /= 8
    dev = make(pattern, values).device()
    for lower in (True, False):
        with pytest.raises(sp.Panic, match="row 333 stores no diagonal entry"):
            dev.trsv(b, lower)
        tr.assert_same_bits(dev.trsv(b, lower, unit_diagonal=True),
                            tr.solve_loop(*pattern, values, b, lower=lower, unit=True))
    with pytest.raises(sp.Panic, match="row 333 stores no diagonal entry"):
        dev.trsv_analyse(lower=True)
    pattern, values, b, ref = case("dense", True, np.float64)
    dev = make(pattern, values).device()
    with pytest.raises(sp.Panic, match=r"b.len\(\) = 299"):
        dev.trsv(b[:-1])
    with pytest.raises(sp.Panic, match="handle holds f64 values"):
        dev.trsv(b.astype(np.float32))
    with pytest.raises(sp.Panic, match="uplo = 2"):
        sp._ffi.check(dev._fn("trsv_analyse")(dev._h, 2, 0, None))
    with pytest.raises(sp.Panic, match="unit_diag = 5"):
        sp._ffi.check(dev._fn("trsv_analyse")(dev._h, 0, 5, None))
    with pytest.raises(sp.Panic, match="null vector"):
        dev.trsv_dev(0, 0)
    tr.assert_same_bits(dev.trsv(b), ref)
