"""The structure zoo of tests/lazy_cases.py, checked on the CPU: every case is valid CSR, its triplets assemble to its
arrays bit for bit under the oracle, and it meets -- or does not meet -- the planner's automatic row-split test as its
name says.  tests/test_gpu_lazy_plan.py relies on all three."""
import numpy as np
import pytest

from tests import lazy_cases as zoo


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("name", zoo.NAMES)
def test_case_is_valid_csr(oracle, name):
    c = zoo.case(name)
    assert oracle.validate(c.nrows, c.ncols, c.rowptr, c.colind, c.values.size) == 0
    assert c.rowptr.dtype == np.uint64 and c.colind.dtype == np.uint64 and c.rowptr.size == c.nrows + 1
    assert c.rows.size == c.cols.size == c.vals.size == int(c.rowptr[-1])
    assert not np.any(c.values == 0)                      # (the assembly drops zeros: none may be stored)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", zoo.NAMES)
def test_triplets_assemble_to_the_case(oracle, name, dtype):
    c = zoo.case(name, dtype)
    assert c.values.dtype == dtype and c.vals.dtype == dtype
    p, i, w = oracle.coo_to_csr(c.nrows, c.ncols, c.rows, c.cols, c.vals)
    assert np.array_equal(p, c.rowptr) and np.array_equal(i, c.colind)
    assert np.array_equal(_bits(w), _bits(c.values))
    if c.vals.size > 1:                                   # shuffled: neither the case's order nor its reverse
        rows = c.rows.astype(np.int64)
        assert np.any(np.diff(rows) < 0) and np.any(np.diff(rows) > 0)
    f64 = zoo.case(name, np.float64)                      # one pattern, one insertion order for both dtypes
    assert np.array_equal(c.rowptr, f64.rowptr) and np.array_equal(c.colind, f64.colind)
    assert np.array_equal(c.rows, f64.rows) and np.array_equal(c.cols, f64.cols)


@pytest.mark.parametrize("name", zoo.NAMES)
def test_case_stays_on_its_planner_path(name):
    """csr_try_row_split's automatic test (row_split = -1, threshold 128), recomputed: long rows in a tenth of the
    64-row tiles, the short rows keep a quarter of the entries at no more than 64 per row.  Met by the four skewed
    cases, by none of the others."""
    c = zoo.case(name)
    hit, ntiles, nnz_short, nnz = zoo.split_counts(c.nrows, c.rowptr)
    met = hit * 10 >= ntiles and nnz_short >= nnz // 4 and nnz_short / c.nrows <= 64.0 and hit > 0 and nnz_short > 0
    assert met == zoo.auto_split_met(c.nrows, c.rowptr)
    assert met == (name in zoo.SKEWED), (name, hit, ntiles, nnz_short, nnz)
    if name == "empty":
        assert nnz == 0                                   # (nnz == 0 is never planned lazily)


def test_case_shapes_and_edges():
    """What each case is the smallest of."""
    lens = {n: np.diff(zoo.case(n).rowptr.astype(np.int64)) for n in zoo.NAMES}
    det = zoo.case("skew_det")
    assert (det.nrows, det.ncols) == (2048, 2048) and zoo.split_counts(2048, det.rowptr)[:2] == (7, 32)
    assert np.array_equal(np.flatnonzero(lens["skew_det"] > 128), np.arange(7, 2048, 320))
    assert set(lens["skew_det"]) == {5, 200}
    c511 = zoo.case("skew_511")
    assert c511.nrows == 511 and np.array_equal(c511.rowptr, det.rowptr[:512])          # skew_det's first rows
    assert np.array_equal(c511.colind, det.colind[:int(det.rowptr[511])])
    for name in ("skew_pareto", "skew_far"):
        c, l = zoo.case(name), lens[name]
        assert c.nrows == 6000 and l[0] == 0 and l[4] == 0 and l[5] == 1 and not l[700:1300].any()
        assert l[1] > 1024                                # a heavy row: a workgroup of its own in the split
        # ... and the two sides of the thread / wave limit of the block-window kernel are both present
        assert (l == 32).any() and (l == 33).any()
    # (3000 draws: a few coincide and are merged)
    assert zoo.case("skew_far").ncols == 300_008 and 2900 < lens["skew_far"][1] <= 3000 and tuple(lens["skew_far"][2:4]) == (33, 32)
    far = zoo.case("skew_far")
    assert int(far.colind.max()) > 290_000                # columns anywhere: no LDS window holds a block's
    par = zoo.case("skew_pareto")
    rows = np.repeat(np.arange(6000, dtype=np.int64), lens["skew_pareto"])
    assert np.abs(par.colind.astype(np.int64) - rows).max() <= 2000
    assert lens["banded"].min() == lens["banded"].max() == 14 and zoo.case("banded").nrows == 40_000
    assert zoo.case("ragged").nrows == 20_000 and 1 <= lens["ragged"].min() and lens["ragged"].max() <= 27
    assert zoo.case("long_rows").nrows == 3000 and lens["long_rows"].min() >= 300 and lens["long_rows"].max() <= 400
    assert lens["long_rows"].mean() > 120.0               # above the stream kernels' mean: the vector kernel
    hollow = zoo.case("hollow")
    assert (hollow.nrows, hollow.ncols) == (3000, 4099) and not lens["hollow"][:-100].any() and lens["hollow"][-100:].all()
    empty = zoo.case("empty")
    assert (empty.nrows, empty.ncols) == (700, 701) and empty.values.size == 0
    for name in zoo.SQUARE:
        assert zoo.case(name).nrows == zoo.case(name).ncols


def test_random_skewed_assemblies_qualify(oracle):
    """The six randomised assemblies of test_coo_assembly_randomised_skewed: what the ORACLE assembles from each meets the
    row-split test (duplicates are summed, none cancels: the pattern is the drawn one), at most one seed in six had to
    draw again, and between them the seeds cover more than one height, duplicate rate and dtype."""
    regenerated, heights, dtypes, dups = 0, set(), set(), set()
    for seed in range(zoo.RANDOM_SEEDS):
        nrows, r, c, v, sub = zoo.random_skewed_coo(seed)
        regenerated += 1 if sub else 0
        p, i, w = oracle.coo_to_csr(nrows, nrows, r, c, v)
        assert zoo.auto_split_met(nrows, p), seed
        heights.add(nrows); dtypes.add(v.dtype); dups.add(r.size > int(p[-1]))
    assert regenerated <= 1, regenerated
    assert len(heights) > 1 and len(dtypes) == 2 and dups == {False, True}, (heights, dtypes, dups)
