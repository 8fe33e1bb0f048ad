"""Triangular solves for a block of right-hand sides on the device (spal_*_trsm_*) against the sequential
definitions applied per column: tests/trsv_ref.py solve_loop for the exact solve, tests/sweep_ref.py sweep_loop for the
sweeps -- raw bits equal, NaN by position, f64 and f32, lower and upper, CSR and CSC, whatever k, the leading dimensions,
the column tile and the launch schedule are.

Matrices come from trsv_ref.fill (values and B in (-1, 1), a dominant diagonal).  A case keeps ONE block of 70 columns
and the reference of a column is computed once, on first use: a block of width k is the first k columns, so every width
shares the same reference columns.  Sizes are the smallest that cross a boundary of the code: a level wider than a
workgroup, level widths 1023 / 1024 / 1025 / 2049, thousands of one-row levels (every chain step narrower than one lane
group), one row of 20 000 entries, a sweep tile whose entries exceed the LDS strip; widths cover a partial tile, the
widest tile, one past it and more columns than a wave has lanes."""
import functools
import zlib

import numpy as np
import pytest

import spalinalg_amd as sp
from tests import sweep_ref as sw
from tests import trsv_ref as tr
from tests.test_gpu_trsv import csc, csr

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
HUGE = 1 << 40
KMAX = 70
SENTINEL = -12345.5
TILES = (1, 2, 4, 8, 16, 32)


def _lower_pattern(name):
    rng = np.random.default_rng(20261019)
    if name == "diagonal":
        return tr.diagonal(3000)                      # one level, wider than a workgroup
    if name == "bidiagonal":
        return tr.bidiagonal(2000)                    # 2000 levels of one row
    if name == "dense":
        return tr.dense_triangle(300)                 # row lengths 0 .. 299; 45 150 entries in two sweep tiles
    if name == "banded":
        return tr.banded(20011, 6, 512, rng)
    if name == "arrow":
        return tr.arrow(20000)                        # one row of 20 000 entries, one level of 19 998 rows
    if name == "prescribed":
        return tr.prescribed(tr.PRESCRIBED_WIDTHS, rng)
    if name == "one":
        return tr.diagonal(1)
    # the sweeps' own, smaller: s passes of the reference cost s times the matrix per column
    if name == "banded701":
        return tr.banded(701, 6, 64, rng)
    if name == "arrow2500":
        return tr.arrow(2500)                         # the tile of the last row exceeds the strip: walked from global memory
    if name == "bidiagonal300":
        return tr.bidiagonal(300)
    raise KeyError(name)


STRUCTURES = ["diagonal", "bidiagonal", "dense", "banded", "arrow", "prescribed", "one"]
# widths of (lower, f64) and of the three other combinations: every structure sees 3 and 33
WIDTHS = {
    "diagonal": ((1, 2, 3, 5, 8, 17, 32, 33, 70), (3, 33)),
    "bidiagonal": ((1, 3, 8, 33, 70), (3, 33)),
    "dense": ((3, 17, 33), (3, 33)),
    "banded": ((3, 33), (3,)),
    "arrow": ((3, 33), (3,)),
    "prescribed": ((2, 3, 32, 33), (3, 33)),
    "one": ((1, 3, 33, 70), (3, 33)),
}


@functools.lru_cache(maxsize=None)
def case(name, lower, dtype):
    """(pattern, values, B of KMAX columns) -- made once per session, shared, never written to."""
    pattern = _lower_pattern(name)
    if not lower:
        pattern = tr.mirror(pattern)
    rng = np.random.default_rng(zlib.crc32(f"trsm/{name}/{lower}".encode()))
    values, _ = tr.fill(pattern, dtype, rng)
    B = rng.uniform(-1, 1, size=(pattern[0], KMAX)).astype(dtype)
    for a in (*pattern[1:], values, B):
        a.setflags(write=False)
    return pattern, values, B


@functools.lru_cache(maxsize=None)
def ref_col(name, lower, dtype, j, unit=False):
    pattern, values, B = case(name, lower, dtype)
    x = tr.solve_loop(*pattern, values, np.ascontiguousarray(B[:, j]), lower=lower, unit=unit)
    x.setflags(write=False)
    return x


def ref_block(name, lower, dtype, k, unit=False):
    return np.stack([ref_col(name, lower, dtype, j, unit) for j in range(k)], axis=1)


@functools.lru_cache(maxsize=None)
def sweep_col(name, lower, dtype, j, s, unit=False):
    pattern, values, B = case(name, lower, dtype)
    x = sw.sweep_loop(*pattern, values, np.ascontiguousarray(B[:, j]), s, lower, unit)
    x.setflags(write=False)
    return x


def sweep_block(name, lower, dtype, k, s, unit=False):
    return np.stack([sweep_col(name, lower, dtype, j, s, unit) for j in range(k)], axis=1)


def exact_columns(pattern, values, B, lower, unit=False):
    return np.stack([tr.solve_loop(*pattern, values, np.ascontiguousarray(B[:, j]), lower=lower, unit=unit)
                     for j in range(B.shape[1])], axis=1)


def sweep_columns(pattern, values, B, s, lower, unit=False):
    return np.stack([sw.sweep_loop(*pattern, values, np.ascontiguousarray(B[:, j]), s, lower, unit)
                     for j in range(B.shape[1])], axis=1)


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def run_dev(dev, B, lower=True, unit=False, sweeps=None, ldb=None, ldx=None, in_place=False):
    """The device form on padded blocks: B's padding is NaN, X's a sentinel, ldb != ldx unless in place.  Checks that
    neither padding changed, that B is as it was, and returns X's k columns."""
    import torch
    n, k = B.shape
    ldb = ldb or k + 3
    ldx = ldb if in_place else (ldx or k + 5)
    Bt = torch.full((n, ldb), float("nan"), dtype=_tdt(B.dtype), device="cuda")
    Bt[:, :k] = torch.from_numpy(np.array(B, order="C")).cuda()
    Xt = Bt if in_place else torch.full((n, ldx), SENTINEL, dtype=Bt.dtype, device="cuda")
    torch.cuda.synchronize()
    if sweeps is None:
        dev.trsm_dev(k, Bt.data_ptr(), ldb, Xt.data_ptr(), ldx, lower, unit)
    else:
        dev.trsm_sweep_dev(k, Bt.data_ptr(), ldb, Xt.data_ptr(), ldx, sweeps, lower, unit)
    torch.cuda.synchronize()
    X, Bh = Xt.cpu().numpy(), Bt.cpu().numpy()
    assert np.isnan(Bh[:, k:]).all(), "the padding of B changed"
    if not in_place:
        assert (X[:, k:] == SENTINEL).all(), "the padding of X was written"
        tr.assert_same_bits(Bh[:, :k], np.ascontiguousarray(B))
    return np.ascontiguousarray(X[:, :k])


# ---- structures ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("name", STRUCTURES)
def test_structure_csr(name, lower, dtype):
    pattern, values, B = case(name, lower, dtype)
    a = csr(pattern, values)
    dev = a.device()
    for k in WIDTHS[name][0 if (lower and dtype == np.float64) else 1]:
        ref = ref_block(name, lower, dtype, k)
        assert not np.isnan(ref).any()
        X = run_dev(dev, B[:, :k], lower)                               # padded, ldb != ldx
        tr.assert_same_bits(X, ref)
        if k == 1:
            tr.assert_same_bits(X[:, 0], dev.trsv(np.ascontiguousarray(B[:, 0]), lower))
        if k == 3:
            tr.assert_same_bits(a.solve_triangular_block(B[:, :k], lower=lower), ref)      # host blocks, packed
            tr.assert_same_bits(run_dev(dev, B[:, :k], lower, in_place=True), ref)
        d = dev.describe()
        assert d["trsv"]["analyses"] == 1
        assert d["trsm"]["k"] == k and d["trsm"]["launches"] == d["trsv"]["lower" if lower else "upper"]["launches"]


@pytest.mark.parametrize("name", STRUCTURES)
def test_structure_csc(name):
    lower = STRUCTURES.index(name) % 2 == 0
    pattern, values, B = case(name, lower, np.float64)
    a = csc(pattern, values)
    for k in WIDTHS[name][1]:
        tr.assert_same_bits(a.solve_triangular_block(B[:, :k], lower=lower), ref_block(name, lower, np.float64, k))
    tr.assert_same_bits(run_dev(a.device(), B[:, :3], lower), ref_block(name, lower, np.float64, 3))
    assert a.device().describe()["trsv"]["analyses"] == 1


# ---- geometry independence ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["banded", "prescribed", "bidiagonal"])
def test_every_column_tile_gives_identical_bits(name):
    pattern, values, B = case(name, True, np.float64)
    dev = csr(pattern, values).device()
    ref = ref_block(name, True, np.float64, 33)
    for tile in TILES:
        dev.set_option("trsm_tile", tile)
        tr.assert_same_bits(run_dev(dev, B[:, :33], True), ref)
        d = dev.describe()["trsm"]
        assert (d["tile"], d["k"], d["column_tiles"]) == (tile, 33, -(-33 // tile))
    dev.set_option("trsm_tile", 0)
    tr.assert_same_bits(run_dev(dev, B[:, :5], True), ref[:, :5])
    assert dev.describe()["trsm"]["tile"] == 8                      # automatic: the narrowest tile that holds k
    tr.assert_same_bits(run_dev(dev, B[:, :33], True), ref)
    assert dev.describe()["trsm"]["tile"] == 32                     # ... at most 32


@pytest.mark.parametrize("name", ["banded", "prescribed", "bidiagonal"])
def test_schedule_settings_give_identical_bits(name):
    pattern, values, B = case(name, True, np.float64)
    dev = csr(pattern, values).device()
    ref = ref_block(name, True, np.float64, 33)
    default = None
    for chain_rows in (None, 0, 1, HUGE):
        if chain_rows is not None:
            dev.set_option("trsv_chain_rows", chain_rows)
        for k in (3, 33):
            tr.assert_same_bits(run_dev(dev, B[:, :k], True), ref[:, :k])
            d = dev.describe()
            assert d["trsm"]["launches"] == d["trsv"]["lower"]["launches"]
        if chain_rows is None:
            default = d["trsv"]["lower"]["launches"]
        if chain_rows == 0:
            assert d["trsm"]["launches"] == d["trsv"]["lower"]["levels"]
        if chain_rows == HUGE:
            assert d["trsm"]["launches"] == 1
    assert default >= 1 and d["trsv"]["analyses"] == 1


# ---- leading dimensions, aliasing, torch -------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_leading_dimensions_in_place_and_column_slices_of_a_wider_tensor(dtype):
    import torch
    pattern, values, B = case("prescribed", True, dtype)
    n = pattern[0]
    dev = csr(pattern, values).device()
    ref = ref_block("prescribed", True, dtype, 17)
    for ldb, ldx in ((17, 40), (64, 18), (19, 17)):
        tr.assert_same_bits(run_dev(dev, B[:, :17], True, ldb=ldb, ldx=ldx), ref)
    tr.assert_same_bits(run_dev(dev, B[:, :17], True, ldb=23, in_place=True), ref)
    tr.assert_same_bits(run_dev(dev, B[:, :17], True, ldb=17, in_place=True), ref)
    # trsm_torch: columns 2 .. 19 of a tensor of 24 columns, the result into columns 1 .. 18 of another one
    wide = torch.full((n, 24), float("nan"), dtype=_tdt(dtype), device="cuda")
    wide[:, 2:19] = torch.from_numpy(np.array(B[:, :17], order="C")).cuda()
    res = torch.full((n, 21), SENTINEL, dtype=wide.dtype, device="cuda")
    out = dev.trsm_torch(wide[:, 2:19], out=res[:, 1:18])
    torch.cuda.synchronize()
    assert out.data_ptr() == res[:, 1:18].data_ptr()
    tr.assert_same_bits(res[:, 1:18].cpu().numpy(), ref)
    assert (res[:, 0] == SENTINEL).all() and (res[:, 18:] == SENTINEL).all()
    fresh = dev.trsm_torch(wide[:, 2:19])
    torch.cuda.synchronize()
    assert fresh.shape == (n, 17) and fresh.is_contiguous()
    tr.assert_same_bits(fresh.cpu().numpy(), ref)
    # in place on the slice: the columns beside it keep their NaN
    view = wide[:, 2:19]
    assert dev.trsm_torch(view, out=view) is view
    torch.cuda.synchronize()
    tr.assert_same_bits(wide[:, 2:19].cpu().numpy(), ref)
    assert torch.isnan(wide[:, :2]).all() and torch.isnan(wide[:, 19:]).all()
    # ... and a sweep through the same door
    sweep = dev.trsm_torch(torch.from_numpy(np.array(B[:, :3], order="C")).cuda(), sweeps=2)
    torch.cuda.synchronize()
    tr.assert_same_bits(sweep.cpu().numpy(), sweep_columns(pattern, values, B[:, :3], 2, True))
    with pytest.raises(sp.Panic, match="out overlaps B"):
        dev.trsm_torch(wide[:, 2:19], out=wide[:, 3:20])
    with pytest.raises(sp.Panic, match="B has 5 rows"):
        dev.trsm_torch(wide[:5, :3])


# ---- values ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_nan_and_inf_in_one_column_stay_in_that_column(lower, dtype):
    pattern, values, B = case("prescribed", lower, dtype)
    n = pattern[0]
    k = 9
    bad = np.ascontiguousarray(B[:, :k]).copy()
    bad[0 if lower else n - 1, 4] = np.nan
    bad[n // 2, 4] = np.inf
    ref = ref_block("prescribed", lower, dtype, k).copy()
    ref[:, 4] = tr.solve_loop(*pattern, values, np.ascontiguousarray(bad[:, 4]), lower=lower)
    assert np.isnan(ref[:, 4]).any() and np.isfinite(np.delete(ref, 4, axis=1)).all()
    dev = csr(pattern, values).device()
    for tile in (0, 2, 32):
        dev.set_option("trsm_tile", tile)
        tr.assert_same_bits(run_dev(dev, bad, lower), ref)
        tr.assert_same_bits(run_dev(dev, bad, lower, sweeps=HUGE), ref)
    tr.assert_same_bits(run_dev(dev, bad, lower, sweeps=2), sweep_columns(pattern, values, bad, 2, lower))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_full_matrix_unit_diagonal_and_the_other_triangle_full_of_nan(dtype):
    pattern = tr.full(1500, 6, np.random.default_rng(5))
    values, _ = tr.fill(pattern, dtype, np.random.default_rng(6))
    n, rowptr, colind = pattern
    values /= 8                    # sum |off-diagonal| < 0.75 per row: the unit-diagonal solve stays bounded
    B = np.random.default_rng(7).uniform(-1, 1, size=(n, 5)).astype(dtype)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    for lower in (True, False):
        poisoned = values.copy()
        poisoned[(colind.astype(np.int64) > rows) if lower else (colind.astype(np.int64) < rows)] = np.nan
        a = csr(pattern, poisoned)
        for unit in (False, True):
            ref = exact_columns(pattern, values, B, lower, unit)
            assert np.isfinite(ref).all()
            tr.assert_same_bits(a.solve_triangular_block(B, lower=lower, unit_diagonal=unit), ref)
            tr.assert_same_bits(run_dev(a.device(), B, lower, unit), ref)
            tr.assert_same_bits(a.solve_triangular_block(B, lower=lower, unit_diagonal=unit, sweeps=2),
                                sweep_columns(pattern, values, B, 2, lower, unit))
    both = csr(pattern, values)
    both.solve_triangular_block(B, lower=True)
    both.solve_triangular_block(B, lower=False)
    assert both.device().describe()["trsv"]["analyses"] == 2


# ---- sweeps ----------------------------------------------------------------------------------------------------------

SWEEP_STRUCTURES = {"banded701": (3, 33), "dense": (3, 17), "arrow2500": (3, 33), "bidiagonal300": (3, 33)}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("name", list(SWEEP_STRUCTURES))
def test_sweeps_are_the_sequential_text_per_column(name, lower, dtype):
    pattern, values, B = case(name, lower, dtype)
    nl = tr.levels(*pattern, lower=lower)[1]
    a = csr(pattern, values)
    dev = a.device()
    first = lower and dtype == np.float64
    for k in (SWEEP_STRUCTURES[name] if first else SWEEP_STRUCTURES[name][:1]):
        for s in (0, 1, 2, 3):
            ref = sweep_block(name, lower, dtype, k, s)
            tr.assert_same_bits(run_dev(dev, B[:, :k], lower, sweeps=s), ref)
            d = dev.describe()["trsm"]
            assert d["launches"] == 1 + s and d["k"] == k
            if k == 3:
                tr.assert_same_bits(a.solve_triangular_block(B[:, :k], lower=lower, sweeps=s), ref)
                tr.assert_same_bits(run_dev(dev, B[:, :k], lower, sweeps=s, in_place=True), ref)
                tr.assert_same_bits(run_dev(dev, B[:, :k], lower, True, sweeps=s), sweep_block(name, lower, dtype, k, s, True))
    assert "trsv" not in dev.describe() and dev.describe()["trsv_sweep"]["prepared"] == 1
    # from levels - 1 on: the exact block solve's bits, the sequential substitution's per column
    k = SWEEP_STRUCTURES[name][-1 if first else 0]
    exact = ref_block(name, lower, dtype, k)
    for s in (nl - 1, HUGE):
        tr.assert_same_bits(run_dev(dev, B[:, :k], lower, sweeps=s), exact)
        assert dev.describe()["trsm"]["launches"] == 1 + min(s, pattern[0] - 1)      # clamped to n - 1
    if name == "bidiagonal300":
        assert run_dev(dev, B[:, :k], lower, sweeps=5).tobytes() != exact.tobytes()      # five passes are not yet the solve
    assert "trsv" not in dev.describe()
    tr.assert_same_bits(run_dev(dev, B[:, :k], lower), exact)
    d = dev.describe()["trsm"]
    assert d["calls"] == 1 and d["sweep_calls"] > 4


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("name", ["banded", "arrow"])
def test_sweeps_on_the_exact_solve_s_sizes(name, lower, dtype):
    """banded(20011, 6, 512) and arrow(20000) themselves, three columns.  The clamped count is run on the band only: on
    the arrow it is 19 999 passes that each walk a row of 20 000 entries in stored order, minutes of device time for a
    path arrow2500 above takes in the same way."""
    pattern, values, B = case(name, lower, dtype)
    nl = tr.levels(*pattern, lower=lower)[1]
    dev = csr(pattern, values).device()
    k = 3
    for s in (0, 1, 2, 3):
        tr.assert_same_bits(run_dev(dev, B[:, :k], lower, sweeps=s), sweep_block(name, lower, dtype, k, s))
    exact = ref_block(name, lower, dtype, k)
    for s in (nl - 1,) + ((HUGE,) if name == "banded" else ()):
        tr.assert_same_bits(run_dev(dev, B[:, :k], lower, sweeps=s), exact)
        assert dev.describe()["trsm"]["launches"] == 1 + min(s, pattern[0] - 1)
    assert "trsv" not in dev.describe()


@pytest.mark.parametrize("name", list(SWEEP_STRUCTURES))
def test_sweeps_csc_and_every_tile(name):
    lower = list(SWEEP_STRUCTURES).index(name) % 2 == 0
    pattern, values, B = case(name, lower, np.float64)
    a = csc(pattern, values)
    ref = sweep_block(name, lower, np.float64, 3, 2)
    tr.assert_same_bits(a.solve_triangular_block(B[:, :3], lower=lower, sweeps=2), ref)
    k = SWEEP_STRUCTURES[name][-1] if lower else 3
    ref = sweep_block(name, lower, np.float64, k, 2)
    for tile in TILES:
        a.device().set_option("trsm_tile", tile)
        tr.assert_same_bits(run_dev(a.device(), B[:, :k], lower, sweeps=2), ref)
        assert a.device().describe()["trsm"]["tile"] == tile


# ---- shared state ------------------------------------------------------------------------------------------------------

def test_vector_and_block_solves_share_one_plan_and_describe_reports_the_last_call():
    pattern, values, B = case("prescribed", True, np.float64)
    dev = csr(pattern, values).device()
    assert "trsm" not in dev.describe()
    tr.assert_same_bits(dev.trsv(np.ascontiguousarray(B[:, 0])), ref_col("prescribed", True, np.float64, 0))
    launches = dev.describe()["trsv"]["lower"]["launches"]
    assert "trsm" not in dev.describe()
    for n_call, k in enumerate((1, 70), start=1):
        tr.assert_same_bits(dev.trsm(B[:, :k]), ref_block("prescribed", True, np.float64, k))
        d = dev.describe()
        assert d["trsv"]["analyses"] == 1
        assert d["trsm"] == {"tile": min(32, k), "k": k, "column_tiles": -(-k // 32), "launches": launches,
                             "calls": n_call, "sweep_calls": 0}
    # ... and the reverse: a block first, then a vector
    dev = csr(pattern, values).device()
    dev.trsm(B[:, :3])
    dev.trsv(np.ascontiguousarray(B[:, 0]))
    dev.trsm_sweep(B[:, :3], 1)
    d = dev.describe()
    assert d["trsv"]["analyses"] == 1 and (d["trsm"]["calls"], d["trsm"]["sweep_calls"]) == (1, 1)
    assert d["trsm"]["launches"] == 2


# ---- refusals through the C ABI --------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_refusals_answer_with_their_status_and_message(kind):
    import ctypes as C
    from spalinalg_amd import _ffi
    make = csr if kind == "csr" else csc
    u, i = C.c_uint64, C.c_int
    pattern, values, B = case("prescribed", True, np.float64)
    n = pattern[0]
    dev = make(pattern, values).device()
    b = np.ascontiguousarray(B[:, :4])
    x = np.empty_like(b)
    p = lambda arr: arr.ctypes.data_as(C.c_void_p)

    def host(name, k, ldb, b_rows, ldx, x_rows, sweeps=None, bb=b, xx=x, uplo=0, unit=0):
        args = [dev._h, i(uplo), i(unit)] + ([u(sweeps)] if sweeps is not None else [])
        return dev._fn(name)(*args, u(k), p(bb), u(ldb), u(b_rows), p(xx), u(ldx), u(x_rows))

    def refused(status, text, code):
        assert code == status
        assert text in _ffi.lib().spal_last_error().decode()

    for name, s in (("trsm_f64", None), ("trsm_sweep_f64", 2)):
        fn = f"spal_{kind}_{name[:-4]}"
        refused(1, f"{fn}: k = 0", host(name, 0, 4, n, 4, n, s))
        refused(1, f"{fn}: ldb = 3 is less than k = 4", host(name, 4, 3, n, 4, n, s))
        refused(1, f"{fn}: ldx = 2 is less than k = 4", host(name, 4, 4, n, 2, n, s))
        refused(1, f"{fn}: B has {n - 1} rows and X has {n} rows but the matrix has {n} rows", host(name, 4, 4, n - 1, 4, n, s))
        refused(1, f"{fn}: B has {n} rows and X has {n + 1} rows", host(name, 4, 4, n, 4, n + 1, s))
        refused(1, f"{fn}: uplo = 2", host(name, 4, 4, n, 4, n, s, uplo=2))
        refused(1, f"{fn}: unit_diag = 3", host(name, 4, 4, n, 4, n, s, unit=3))
        refused(1, f"{fn}: null block of vectors", dev._fn(name)(dev._h, i(0), i(0), *([u(s)] if s is not None else []), u(4),
                                                                  None, u(4), u(n), p(x), u(4), u(n)))
        refused(1, f"{fn}: in place (x == b) needs ldx == ldb", host(name, 2, 4, n, 2, n, s, xx=b))
        refused(1, f"{fn}: handle holds f64 values", host(name.replace("f64", "f32"), 4, 4, n, 4, n, s))
    refused(1, f"spal_{kind}_trsm_dev: null block of vectors",
            dev._fn("trsm_dev_f64")(dev._h, i(0), i(0), u(4), None, u(4), None, u(4), None))
    refused(1, f"spal_{kind}_trsm_sweep_dev: k = 0",
            dev._fn("trsm_sweep_dev_f64")(dev._h, i(0), i(0), u(1), u(0), p(b), u(4), p(x), u(4), None))
    assert "trsm" not in dev.describe() and "trsv" not in dev.describe()         # nothing ran, nothing was analysed
    for bad in (-1, 3, 5, 64, 33):
        with pytest.raises(sp.Panic, match="trsm_tile must be 0 \\(automatic\\) or one of 1, 2, 4, 8, 16, 32"):
            dev.set_option("trsm_tile", bad)
    # a matrix that is not square, a missing diagonal
    cls = sp.CsrMatrix if kind == "csr" else sp.CscMatrix
    rect = cls(2, 3, [0, 1, 2] if kind == "csr" else [0, 1, 2, 2], [0, 1], np.array([1.0, 2.0])).device()
    with pytest.raises(sp.Panic, match=rf"spal_{kind}_trsm: the matrix is not square \(2 x 3\)"):
        rect.trsm(np.ones((2, 2)))
    with pytest.raises(sp.Panic, match=rf"spal_{kind}_trsm_sweep: the matrix is not square \(2 x 3\)"):
        rect.trsm_sweep(np.ones((2, 2)), 1)
    holes = tr.drop_diagonal(tr.drop_diagonal(tr.full(900, 4, np.random.default_rng(18)), 700), 333)
    hv, _ = tr.fill(holes, np.float64, np.random.default_rng(19))
    hv /= 8
    hb = np.random.default_rng(20).uniform(-1, 1, size=(900, 3))
    hd = make(holes, hv).device()
    for lower in (True, False):
        with pytest.raises(sp.Panic, match=rf"spal_{kind}_trsm: row 333 stores no diagonal entry"):
            hd.trsm(hb, lower)
        with pytest.raises(sp.Panic, match=rf"spal_{kind}_trsm_sweep: row 333 stores no diagonal entry"):
            hd.trsm_sweep(hb, 1, lower)
        tr.assert_same_bits(hd.trsm(hb, lower, unit_diagonal=True), exact_columns(holes, hv, hb, lower, True))
    # the handle is still usable
    tr.assert_same_bits(dev.trsm(b), ref_block("prescribed", True, np.float64, 4))


# ---- a small fuzz ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(24))
def test_fuzz(seed):
    rng = np.random.default_rng(977 + seed)
    n = int(rng.integers(1, 1500)) if seed % 6 else int(rng.integers(3000, 4001))
    if seed % 2:
        pattern = tr.full(n, int(rng.integers(1, 7)), rng)
    else:
        pattern = tr.banded(n, int(rng.integers(1, 7)), int(rng.integers(1, 200)), rng)
        if rng.integers(2):
            pattern = tr.mirror(pattern)
    dtype = DTYPES[int(rng.integers(2))]
    lower, unit = bool(rng.integers(2)), bool(rng.integers(2))
    k = int(rng.integers(1, 41)) if seed % 6 else int(rng.integers(1, 6))
    values, _ = tr.fill(pattern, dtype, rng)
    if unit:
        values /= 8
    B = rng.uniform(-1, 1, size=(n, k)).astype(dtype)
    a = (csc if seed % 5 == 0 else csr)(pattern, values)
    dev = a.device()
    dev.set_option("trsm_tile", int(rng.choice((0,) + TILES)))
    dev.set_option("trsv_chain_rows", int(rng.choice((0, 1, 7, 256, 1024, HUGE))))
    ldb, ldx = k + int(rng.integers(0, 9)), k + int(rng.integers(0, 9))
    in_place = bool(rng.integers(3) == 0)
    exact = exact_columns(pattern, values, B, lower, unit)
    tr.assert_same_bits(run_dev(dev, B, lower, unit, ldb=ldb, ldx=ldx, in_place=in_place), exact)
    s = int(rng.integers(0, 4))
    tr.assert_same_bits(run_dev(dev, B, lower, unit, sweeps=s, ldb=ldb, ldx=ldx, in_place=in_place),
                        sweep_columns(pattern, values, B, s, lower, unit))
    tr.assert_same_bits(a.solve_triangular_block(B, lower=lower, unit_diagonal=unit, sweeps=HUGE), exact)
    assert dev.describe()["trsv"]["analyses"] == 1
