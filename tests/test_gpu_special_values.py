"""GPU: signed zeros, infinities, NaN and subnormals through every SpMV / SpMM path, and the leak check.

One case per path.  Each first asserts through describe() that the path it names is the one that runs, then compares the
product of the planted inputs (tests/special_cases.py) with the oracle's under assert_special_parity, then runs the leak
check: with every column that the rows of R do not reference poisoned (NaN, +inf, -inf), the rows of R must come out as
they do without the poison -- bit for bit on the deterministic paths, finite and within the tolerance on the atomic ones.
What a path promises (bits, or a tolerance) is DESIGN 3.2d's table, not what its kernel happens to do."""
import numpy as np
import pytest

import spalinalg_amd as sp
from tests import special_cases as sc

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
_REFS = {}


def inputs(oracle, name, dtype):
    """the structure's planted inputs, the oracle's product and the leak check's vectors: computed once, never written"""
    key = (name, np.dtype(dtype))
    if key not in _REFS:
        n, nc, rp, ci, s = sc.case(name, dtype)
        R = sc.leak_rows(n)
        x_fin = sc.ordinary(np.random.default_rng(9), nc, dtype)
        c = dict(n=n, nc=nc, rp=rp, ci=ci, va=s["values"], x=s["x"], s=s, lens=np.diff(rp.astype(np.int64)),
                 y_ref=oracle.csr_spmv(rp, ci, s["values"], s["x"]), bound=sc.spmv_bound(rp, ci, s["values"], s["x"], oracle),
                 x_fin=x_fin, x_poison=sc.poison_complement(rp, ci, nc, R, x_fin), in_R=sc.rows_mask(n, R),
                 bound_fin=sc.spmv_bound(rp, ci, s["values"], x_fin, oracle), tol=sc.TOL[np.dtype(dtype)])
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = c
    return _REFS[key]


def check(c, spmv, exact, deterministic=True, what=None):
    """the special-value comparison, then the leak check, of one configuration of one path"""
    try:
        sc.assert_special_parity(spmv(c["x"]), c["y_ref"], exact, c["bound"], c["tol"])
        m = c["in_R"]
        y0, y1 = spmv(c["x_fin"]), spmv(c["x_poison"])
        if deterministic:
            sc.assert_special_parity(y1[m], y0[m], True, None, None)
        else:
            sc.assert_special_parity(y1[m], y0[m], False, c["bound_fin"][m], c["tol"])
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from e


def csr_device(c):
    return sp.CsrMatrix(c["n"], c["nc"], c["rp"], c["ci"], c["va"]).device()


def set_options(dev, opts):
    for k, v in opts.items():
        dev.set_option(k, v)


# ---- the stream kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_tiles_with_an_lds_window(oracle, dtype):
    """Ragged rows of 0 ... 24 entries, 70 001 x 3000, one super-tile per workgroup with its window of x in LDS: every tile
    height the rows allow, skewed strips or not, persistent or not, non-temporal stores.  Bits."""
    c = inputs(oracle, "ragged_lds", dtype)
    dev = csr_device(c)
    dev.set_option("slide_on", 0)
    for rpt in (0, 64, 32, 12, 8):
        dev.set_option("rows_per_tile", rpt)
        for opts in ({"skew": 0, "persistent": 0, "nt_store": 0}, {"skew": 1, "persistent": 1, "nt_store": 0},
                     {"skew": 0, "persistent": 1, "nt_store": 1}, {"skew": 1, "persistent": 0, "nt_store": 1}):
            set_options(dev, opts)
            d = dev.describe()
            assert d["kernel"] == "stream" and d["slide"] == 0 and d["rows_per_tile"] == (rpt or 64), d
            assert d["stream_row_fraction"] == 1.0 and d["overflow_tiles"] == 0 and d["lds_row_fraction"] > 0.9, d
            assert d["skew"] == opts["skew"] and d["nt_store"] == opts["nt_store"], d
            assert rpt not in (0, 64) or d["persistent"] == opts["persistent"], d
            check(c, dev.spmv, True, what=(rpt, opts))


@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_tall_tiles(oracle, dtype):
    """Rows of 0 ... 3 entries: tiles of 256 and 128 rows, a lane summing four / two adjacent rows.  Bits."""
    c = inputs(oracle, "short_rows", dtype)
    dev = csr_device(c)
    dev.set_option("slide_on", 0)
    for rpt in (0, 128, 64):
        dev.set_option("rows_per_tile", rpt)
        for persistent in (0, 1):
            dev.set_option("persistent", persistent)
            d = dev.describe()
            assert d["kernel"] == "stream" and d["slide"] == 0 and d["rows_per_tile"] == (rpt or 256), d
            assert d["stream_row_fraction"] == 1.0 and d["overflow_tiles"] == 0, d
            check(c, dev.spmv, True, what=(rpt, persistent))


@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_global_mode(oracle, dtype):
    """A band of 20 000 columns: no window of x fits LDS, the stream kernel gathers through L2 (32-bit columns).  Bits."""
    c = inputs(oracle, "global_banded", dtype)
    dev = csr_device(c)
    set_options(dev, {"panel_on": 0, "slide_on": 0})
    for persistent in (0, 1):
        dev.set_option("persistent", persistent)
        d = dev.describe()
        assert d["kernel"] == "stream" and d["stream_row_fraction"] == 1.0 and d["lds_row_fraction"] < 0.05, d
        assert d["slide"] == 0 and d["panel_tiles"] == 0 and d["overflow_tiles"] == 0 and d["persistent"] == persistent, d
        check(c, dev.spmv, True, what=persistent)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["slide_banded14", "slide_ragged"])
def test_sliding_window(oracle, dtype, name):
    """The sliding-window kernel on a band of 14 per row (uniform rows: rowptr read or not) and on ragged rows, whose tiles
    above 1024 entries it takes in halves; runs dealt differently, grid sizes.  Bits on every row."""
    c = inputs(oracle, name, dtype)
    dev = csr_device(c)
    dev.set_option("slide_on", 1)
    uniform = name == "slide_banded14"
    reads_rowptr = 0
    for opts in ({}, {"uniform_rows": 0}, {"uniform_rows": 1, "slide_run": 3}, {"slide_run": 0, "persistent_blocks": 64},
                 {"persistent_blocks": 4096, "nt_store": 1}):
        set_options(dev, opts)
        reads_rowptr = 1 - opts.get("uniform_rows", 1 - reads_rowptr)
        d = dev.describe()
        assert d["kernel"] == "stream" and d["slide"] == 1 and d["ring_pages"] > 0 and d["overflow_tiles"] == 0, d
        assert (d["uniform_row_fraction"] == 1.0) == (uniform and not reads_rowptr) and (d["split_tiles"] > 0) == (not uniform), d
        check(c, dev.spmv, True, what=opts)


def _overflow_tiles(c, rpt=64, slack=0):
    """rows of the tiles that hold more than 1024 (- slack) entries, counted from the tile's first entry's even place"""
    rp = c["rp"].astype(np.int64)
    starts = np.arange(0, c["n"], rpt)
    ends = np.minimum(starts + rpt, c["n"])
    big = (rp[ends] - (rp[starts] & ~1)) > 1024 - slack
    return big, np.repeat(big, ends - starts)


@pytest.mark.parametrize("dtype", DTYPES)
def test_overflow_kernel(oracle, dtype):
    """The same ragged rows on the one-super-tile-per-workgroup kernels: the tiles above 1024 entries go to the overflow
    kernel, whose rows are tree sums (tolerance); every other row keeps the reference's bits."""
    c = inputs(oracle, "slide_ragged", dtype)
    dev = csr_device(c)
    set_options(dev, {"rows_per_tile": 64, "slide_on": 0})
    big, _ = _overflow_tiles(c)
    near, near_rows = _overflow_tiles(c, slack=4)       # (a tile within four entries of the limit: either kernel)
    for persistent in (0, 1):
        dev.set_option("persistent", persistent)
        d = dev.describe()
        assert d["kernel"] == "stream" and d["slide"] == 0 and d["rows_per_tile"] == 64 and d["persistent"] == persistent, d
        assert 20 < int(big.sum()) <= d["overflow_tiles"] <= int(near.sum()), (d, int(big.sum()), int(near.sum()))
        check(c, dev.spmv, ~near_rows, what=persistent)


@pytest.mark.parametrize("dtype", DTYPES)
def test_column_panels(oracle, dtype):
    """A band wider than the LDS window (16 384 columns of f64, 40 000 of f32): entries in registers, x in panels.  Bits."""
    c = inputs(oracle, "panels" if dtype == np.float64 else "panels_wide", dtype)
    dev = csr_device(c)
    for opts in ({}, {"persistent": 1}, {"persistent": 0, "nt_store": 1}):
        set_options(dev, opts)
        d = dev.describe()
        assert d["kernel"] == "stream" and d["slide"] == 0 and d["panel_tiles"] > 0 and d["overflow_tiles"] == 0, d
        assert d["stream_row_fraction"] == 1.0, d
        check(c, dev.spmv, True, what=opts)


@pytest.mark.parametrize("dtype", DTYPES)
def test_column_blocked(oracle, dtype):
    """3000 x 9000, columns anywhere, column blocks of 2048: the entry-parallel form and the rows form.  Bits."""
    c = inputs(oracle, "cblock", dtype)
    dev = csr_device(c)
    set_options(dev, {"cblock_shift": 11, "cblock": 1})
    for form in (0, 1):
        dev.set_option("cblock_form", form)
        d = dev.describe()
        assert d["kernel"] == "cblock" and d["cblock_form"] == ("rows" if form else "entry") and d["cblock_cols"] == 2048, d
        check(c, dev.spmv, True, what=form)


# ---- skewed row lengths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["bw_a", "bw_a_windowless", "bw_b", "bw_c", "pareto"])
def test_block_window(oracle, dtype, name):
    """The block-window kernel: rows of at most 32 entries are one thread's, summed in the reference's order from the first
    product on, across a pass boundary too (bits -- a row of -0.0 alone stays -0.0); longer rows are tree sums (tolerance).
    The pareto matrix carries, in every block of 4096 rows, a row cut by a pass boundary whose first segment is all -0.0,
    between two dedicated rows."""
    c = inputs(oracle, name, dtype)
    dev = csr_device(c)
    dev.set_option("blockwin", 1)
    d = dev.describe()
    assert d["kernel"] == "blockwin" and d["block_rows"] in (512, 1024, 2048, 4096) and d["thread_rows_up_to"] == 32, d
    assert (d["window_columns"] > 0) == (name != "bw_a_windowless") and d["window_columns"] % 256 == 0, d
    assert d["blocks"] == -(-c["n"] // d["block_rows"]) and sc.BW_TALLEST % d["block_rows"] == 0, d
    thread_rows = c["lens"] <= 32
    if name == "pareto":
        s = c["s"]
        assert s["cut"].size >= 5 and thread_rows[s["cut"]].all() and (~thread_rows).sum() > 100
    check(c, dev.spmv, thread_rows, what=d)
    # x at an address that is no multiple of 16: the window is staged by the scalar loop
    import torch
    xo = torch.empty(c["nc"] + 3, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")[(1 if dtype == np.float64 else 3):][:c["nc"]]
    assert xo.data_ptr() % 16 != 0
    yo = torch.empty(c["n"], dtype=xo.dtype, device="cuda")

    def unaligned(x):
        xo.copy_(torch.from_numpy(np.array(x)))
        yo.fill_(float("nan"))
        dev.spmv_dev(xo.data_ptr(), yo.data_ptr())
        torch.cuda.synchronize()
        return yo.cpu().numpy()

    check(c, unaligned, thread_rows, what="x not 16-byte aligned")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("threshold", [1, 16, 128])
def test_row_split(oracle, dtype, threshold):
    """A = A_short + A_long: the rows up to the threshold keep the reference's bits, the listed rows are tree sums (tolerance).
    The short part is A with the long rows emptied, under a stream plan of its own: where that plan leaves a tile of more than
    1024 entries to the overflow kernel (threshold 16 at its own choice of 128 rows per tile), that tile's rows -- and only they --
    are tree sums too; at 64 rows per tile no tile of rows of at most 16 entries exceeds the strip."""
    c = inputs(oracle, "pareto", dtype)
    dev = csr_device(c)
    set_options(dev, {"blockwin": 0, "row_split_threshold": threshold, "row_split": 1})
    lens = c["lens"]
    is_short = lens <= threshold
    short_rp = np.concatenate([[0], np.cumsum(np.where(is_short, lens, 0))])
    for rpt in (0, 64):
        dev.set_option("rows_per_tile", rpt)          # (forwarded to the short part)
        d = dev.describe()
        assert d["kernel"] == "split" and d["split_threshold"] == threshold and d["split_long_rows"] == int((~is_short).sum()), d
        short = d["short_part"]
        brief = {k: short[k] for k in ("kernel", "rows_per_tile", "stream_row_fraction", "overflow_tiles", "panel_tiles", "slide")}
        assert short["kernel"] == "stream" and short["slide"] == 0 and (rpt == 0 or short["rows_per_tile"] == rpt), brief
        # the short part's tiles above 1024 entries (a tile within four entries of the limit: either kernel), in pieces of 64 rows
        height = short["rows_per_tile"]
        starts = np.arange(0, c["n"], height)
        ends = np.minimum(starts + height, c["n"])
        entries = short_rp[ends] - (short_rp[starts] & ~1)
        big, near = entries > 1024, entries > 1020
        pieces = lambda m: int((-(-(ends - starts)[m] // 64)).sum())
        assert pieces(big) <= short["overflow_tiles"] <= pieces(near), (brief, pieces(big), pieces(near))
        left = round((1.0 - short["stream_row_fraction"]) * c["n"])
        assert int((ends - starts)[big].sum()) <= left <= int((ends - starts)[near].sum()), (brief, left)
        if threshold != 16 or rpt == 64:
            assert not near.any() and short["stream_row_fraction"] == 1.0, brief      # every short row: bits
        else:
            assert big.sum() >= 5, brief                                                # the masked form is the one that runs
        check(c, dev.spmv, is_short & ~np.repeat(near, ends - starts), what=brief)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("unroll", [1, 2, 4])
def test_vector_kernel(oracle, dtype, unroll):
    """Lanes share a row and add their partial sums in a tree, starting from +0.0: the tolerance, NaN and inf exactly where the
    reference has them (a row's idle lanes and clamped loads contribute nothing)."""
    c = inputs(oracle, "vector", dtype)
    dev = csr_device(c)
    for lanes in (2, 4, 8, 16, 32, 64):
        for lds_x in (0, 1):
            set_options(dev, {"blockwin": 0, "row_split": 0, "kernel": 1, "lanes_per_row": lanes, "unroll": unroll, "lds_x": lds_x})
            d = dev.describe()
            assert d["kernel"] == "vector" and d["lanes_per_row"] == lanes and d["unroll"] == unroll and d["lds_x"] == lds_x, d
            check(c, dev.spmv, False, what=(lanes, lds_x))


# ---- CSC ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_csc_paths(oracle, dtype):
    """CSC handles: the default (transposed once, then the CSR kernels) returns the reference's bits; the scatter paths (row
    tiles, LDS-privatised column tiles with either flush, global atomics) add in any order from +0.0: the tolerance.  The f32
    LDS and global atomic adds keep subnormals on gfx950: the subnormal rows get no allowance."""
    c = inputs(oracle, "csc_band", dtype)
    cp, ri, cv = oracle.transpose(c["n"], c["nc"], c["rp"], c["ci"], c["va"])
    sc.assert_special_parity(oracle.csc_spmv(c["n"], cp, ri, cv, c["x"]), c["y_ref"], True, None, None)    # one reference, two formats
    dev = sp.CscMatrix(c["n"], c["nc"], cp, ri, cv).device()
    assert dev.describe()["kernel"] == "transposed_csr"
    check(c, dev.spmv, True, what="transposed")
    dev.set_option("kernel", 1)
    d = dev.describe()
    assert d["kernel"] == "lds_privatised_scatter" and d["row_tiles"] == 1, d
    check(c, dev.spmv, False, deterministic=False, what=d)
    dev.set_option("row_tiles", 0)
    for flush, names in ((0, ("global_atomics", "neighbour_handoff")), (1, ("windows_then_reduce",))):
        dev.set_option("flush", flush)
        d = dev.describe()
        assert d["kernel"] == "lds_privatised_scatter" and d["row_tiles"] == 0 and d["flush"] in names, d
        check(c, dev.spmv, False, deterministic=False, what=d)
    set_options(dev, {"flush": 0, "lds": 0})
    d = dev.describe()
    assert d["kernel"] == "atomic_scatter", d
    check(c, dev.spmv, False, deterministic=False, what=d)


# ---- SpMM -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_spmm(oracle, dtype, fmt):
    """Y = A X for k = 1, 5 and 32 vectors, each with the specials at the same columns and signs of its own, X a column slice
    of a wider block (ldx > k).  Bits, column by column; the poisoned columns of X reach no row of R."""
    import torch
    c = inputs(oracle, "ragged_lds", dtype)
    if fmt == "csr":
        dev = csr_device(c)
    else:
        dev = sp.CscMatrix(c["n"], c["nc"], *oracle.transpose(c["n"], c["nc"], c["rp"], c["ci"], c["va"])).device()
    rng = np.random.default_rng(32)
    signs = rng.choice([-1.0, 1.0], (c["nc"], 32)).astype(dtype)
    signs[:, 0] = 1
    wide = {"x": c["x"][:, None] * signs, "x_fin": c["x_fin"][:, None] * signs, "x_poison": c["x_poison"][:, None] * signs}
    refs = np.stack([oracle.csr_spmv(c["rp"], c["ci"], c["va"], np.ascontiguousarray(wide["x"][:, j])) for j in range(32)], axis=1)
    assert np.array_equal(sc.bits(refs[:, 0])[~np.isnan(refs[:, 0])], sc.bits(c["y_ref"])[~np.isnan(c["y_ref"])])
    padded = {k: torch.from_numpy(np.concatenate([np.full((c["nc"], 3), np.nan, dtype=dtype), v], axis=1)).cuda() for k, v in wide.items()}
    assert all(X.stride(0) == 35 for X in padded.values())
    for k in (1, 5, 32):
        Y = dev.spmm(np.ascontiguousarray(wide["x"][:, :k]))
        assert dev.describe()["spmm"]["k"] == k
        got = {name: dev.spmm_torch(X[:, 3:3 + k]).cpu().numpy() for name, X in padded.items()}      # ldx = 35 > k
        for j in range(k):
            sc.assert_special_parity(Y[:, j], refs[:, j], True, None, None)
            sc.assert_special_parity(got["x"][:, j], refs[:, j], True, None, None)
            m = c["in_R"]
            sc.assert_special_parity(got["x_poison"][m, j], got["x_fin"][m, j], True, None, None)


# ---- virtual shards -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_virtual_shards(oracle, dtype):
    """Three row shards on one GPU, every exchange path of the handle: the windows of x scattered, broadcast, or exchanged as
    halos between products.  Bits; what lies outside a shard's window or halo reaches none of its rows."""
    c = inputs(oracle, "mg_band", dtype)
    a = sp.CsrMatrix(c["n"], c["nc"], c["rp"], c["ci"], c["va"])
    mg = sp.MultiGpuCsr(a, 3, devices=[0, 0, 0])
    assert mg.ngpus == 3 and mg.transport == "copy" and np.all(np.diff(mg.partition().astype(np.int64)) > 0)

    def local(x):
        mg.set_x(x)
        mg.scatter_x()
        mg.spmv_local()
        mg.gather_y()
        return mg.y_gathered().copy()

    def resident(x):
        mg.set_x(x)
        mg.broadcast_x()
        mg.spmv_resident()
        return mg.y_allgathered().copy()

    check(c, mg.spmv, True, what="host call")
    check(c, local, True, what="scatter, local products, gather")
    check(c, resident, True, what="broadcast, resident product, all-gather")
    # x <- A x three times with the halo exchange, against three oracle products
    mg.set_x(c["x"])
    mg.scatter_x()
    v = c["x"]
    for _ in range(3):
        mg.spmv_halo()
        v = oracle.csr_spmv(c["rp"], c["ci"], c["va"], v)
    mg.gather_y()
    sc.assert_special_parity(mg.y_gathered(), v, True, None, None)
    assert np.isfinite(v).any() and np.isnan(v).any()
    check(c, local, True, what="a plain product after the halo exchanges")
    mg.close()
