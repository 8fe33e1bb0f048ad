"""The aggregation AMG on the device against its sequential text (tests/amg_ref.py): the hierarchy (aggregates, every
level's structure and value bits, the level sizes), one cycle bit for bit whatever "amg_tail_rows" is, the stream
contract of apply_dev, CG and BiCGStab preconditioned by the cycle, lifetime and refusals.  CSR and CSC, f64 and f32.

References are computed once per session and shared (treat them as read-only)."""
import ctypes as C
import functools

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import amg_cases as ac
from tests import amg_ref as ar
from tests import trsv_ref as tr

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
KINDS = ["csr", "csc"]
TAIL_CLAMP = 4096


def _matrix(kind, pattern, values):
    n, rowptr, colind = pattern
    csr = sp.CsrMatrix(n, n, rowptr, colind, values)
    return csr if kind == "csr" else sp.CscMatrix.from_csr(csr)


def _kw_device(kw):
    """amg_ref's keywords as a.amg()'s"""
    kw = dict(kw)
    gamma = kw.pop("gamma", 1)
    return dict(kw, cycle="v" if gamma == 1 else "w")


def _nonsymmetric_grid(dtype):
    """the 32 x 32 grid with its upper off-diagonal entries scaled: not symmetric, still diagonally dominant"""
    pattern, values = ar.stencil((32, 32), dtype)
    rows = np.repeat(np.arange(pattern[0]), np.diff(pattern[1].astype(np.int64)))
    values = values.copy()
    values[pattern[2].astype(np.int64) > rows] *= dtype(0.625)
    return pattern, values


def _zero_diagonal(dtype):
    """the path of 40 with a stored 0.0 at (7, 7)"""
    pattern, values = ar.path(40, dtype)
    values = values.copy()
    values[ar.diagonal_positions(pattern)[7]] = 0.0
    return pattern, values


INPUTS = {
    "grid_32x32": lambda dt: ar.stencil((32, 32), dt),
    "grid_33x31": lambda dt: ar.stencil((33, 31), dt),
    "grid_10x10x10": lambda dt: ar.stencil((10, 10, 10), dt),
    "descending_path_3000": lambda dt: ar.descending_path(3000, 0, dt),
    "star_one_sided": lambda dt: ar.star(5001, False, dt),
    "star_two_sided": lambda dt: ar.star(5001, True, dt),
    "star_3000": lambda dt: ar.star(3001, True, dt),           # below the tail's clamp: the hub inside the tail kernel
    "hubs": lambda dt: ar.hubs(dtype=dt),                      # rows and aggregates around 32 entries and steps of 64
    "diagonal": lambda dt: ar.diagonal(300, dt),
    "cancelling": lambda dt: ar.cancelling(dt),
    "path_70001": lambda dt: ar.path(70001, dt),
    "nonsymmetric_grid": _nonsymmetric_grid,
    "zero_diagonal": _zero_diagonal,
}


@functools.lru_cache(maxsize=None)
def _input(name, dtype):
    return INPUTS[name](dtype)


@functools.lru_cache(maxsize=None)
def _reference(name, dtype, kw=()):
    pattern, values = _input(name, dtype)
    return ar.Hierarchy(pattern, values, **dict(kw))


def _check_hierarchy(g, h):
    d = g.describe()
    assert d["levels"] == len(h.levels) and d["rows"] == h.rows, (d["rows"], h.rows)
    assert d["stopped_by"] == h.stopped_by
    assert d["nnz"] == [int(lv.pattern[1][-1]) for lv in h.levels]
    assert d["aggregates"] == [lv.nagg or 0 for lv in h.levels]
    for l, lv in enumerate(h.levels):
        m = g.level(l)
        assert m.nrows() == lv.n and m.ncols() == lv.n
        assert np.array_equal(m.rowptr(), lv.pattern[1]) and np.array_equal(m.colind(), lv.pattern[2])
        tr.assert_same_bits(m.values(), lv.values)
        if lv.agg is not None:
            assert np.array_equal(g.aggregates(l), lv.agg.astype(np.uint64))
            assert d["rounds"][l] == ac.level_rounds(lv, h.p["seed"])    # the round rule decides every vertex's round
    with pytest.raises(sp.Panic, match="no coarser level"):
        g.aggregates(len(h.levels) - 1)


# ---- 1. the hierarchy ---------------------------------------------------------------------------------------------------

HIERARCHY_CASES = [
    ("grid_32x32", ()), ("grid_33x31", ()), ("grid_10x10x10", ()), ("descending_path_3000", ()),
    ("star_one_sided", ()), ("star_two_sided", ()), ("hubs", (("coarse_rows", 4),)), ("diagonal", (("coarse_rows", 0),)),
    ("cancelling", (("coarse_rows", 2),)), ("path_70001", ()),
    ("grid_32x32", (("max_levels", 1),)), ("grid_32x32", (("max_levels", 2),)),
    ("grid_32x32", (("coarse_rows", 0),)), ("grid_32x32", (("coarse_rows", 10**9),)), ("grid_32x32", (("seed", 2**32 + 7),)),
]


# (the large chain runs once per format and once per dtype)
HIERARCHY_RUNS = [(n, k, kind, dt) for n, k in HIERARCHY_CASES for kind in KINDS for dt in DTYPES
                  if n != "path_70001" or (kind == "csc") == (dt == np.float32)]


def _id(name, kw, kind, dtype):
    return f"{name}-{dict(kw)}-{kind}-{'f64' if dtype == np.float64 else 'f32'}"


@pytest.mark.parametrize("name,kw,kind,dtype", HIERARCHY_RUNS, ids=[_id(*r) for r in HIERARCHY_RUNS])
def test_hierarchy_is_the_text(name, kw, kind, dtype):
    h = _reference(name, dtype, kw)
    a = _matrix(kind, *_input(name, dtype))
    g = a.amg(**_kw_device(dict(kw)))
    _check_hierarchy(g, h)
    g.close()


def test_hierarchy_stop_rules():
    assert _reference("diagonal", np.float64, (("coarse_rows", 0),)).stopped_by == "no_coarsening"
    assert len(_reference("diagonal", np.float64, (("coarse_rows", 0),)).levels) == 1
    assert _reference("cancelling", np.float64, (("coarse_rows", 2),)).stopped_by == "diagonal"
    assert _reference("grid_32x32", np.float64, (("max_levels", 2),)).stopped_by == "max_levels"
    assert _reference("grid_32x32", np.float64, (("coarse_rows", 0),)).stopped_by == "no_coarsening"
    assert _reference("grid_32x32", np.float64, (("seed", 2**32 + 7),)).rows == ar.Hierarchy(
        *_input("grid_32x32", np.float64), seed=7).rows


# ---- 2. the cycle -------------------------------------------------------------------------------------------------------

def _rhs(n, dtype, seed=5):
    return np.random.default_rng(seed).standard_normal(n).astype(dtype)


def _apply_all_tails(g, b):
    """apply(b) with the tail off, at its default and at the clamp: the three results are the same bits"""
    default = g.describe()["tail_rows"]
    out = []
    for rows in (0, default, TAIL_CLAMP, 10**9):
        g.set_option("amg_tail_rows", rows)
        d = g.describe()
        assert d["tail_rows"] == min(rows, TAIL_CLAMP)
        first = [l for l, n in enumerate(d["rows"]) if n <= d["tail_rows"]]
        assert d["tail_from_level"] == (first[0] if first else d["levels"])
        out.append(g.apply(b))
    g.set_option("amg_tail_rows", default)
    for x in out[1:]:
        tr.assert_same_bits(x, out[0])
    return out[0]


CYCLE_PARAMS = [(), (("nu", 1), ("coarse_sweeps", 1)), (("nu", 3), ("gamma", 2)), (("gamma", 2), ("alpha", 1.5), ("omega", 0.8)),
                (("nu", 1), ("gamma", 2), ("coarse_sweeps", 1), ("alpha", 1.5))]
CYCLE_INPUTS = ["grid_32x32", "grid_33x31", "grid_10x10x10", "star_two_sided", "star_one_sided", "star_3000", "hubs", "descending_path_3000", "path_70001"]


# every parameter set, format and dtype on the small grid; the other inputs on two sets, as CSR f64 and CSC f32
CYCLE_RUNS = [(n, k, kind, dt) for n in CYCLE_INPUTS for k in CYCLE_PARAMS for kind in KINDS for dt in DTYPES
              if n == "grid_32x32" or (k in (CYCLE_PARAMS[0], CYCLE_PARAMS[3]) and (kind == "csc") == (dt == np.float32))]


@pytest.mark.parametrize("name,kw,kind,dtype", CYCLE_RUNS, ids=[_id(*r) for r in CYCLE_RUNS])
def test_cycle_is_the_text(name, kw, kind, dtype):
    if name == "hubs":
        kw = kw + (("coarse_rows", 4),)                               # more than two levels: aggregates of many members
    h = _reference(name, dtype, kw)
    a = _matrix(kind, *_input(name, dtype))
    g = a.amg(**_kw_device(dict(kw)))
    b = _rhs(h.levels[0].n, dtype)
    tr.assert_same_bits(_apply_all_tails(g, b), h.cycle(b))
    g.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kw", [(("coarse_rows", 0), ("coarse_sweeps", 1)), (("coarse_rows", 0), ("coarse_sweeps", 16))], ids=["1", "16"])
def test_one_level_is_damped_jacobi(kw, dtype):
    h = _reference("diagonal", dtype, kw)
    assert len(h.levels) == 1
    g = _matrix("csr", *_input("diagonal", dtype)).amg(**_kw_device(dict(kw)))
    b = _rhs(300, dtype)
    tr.assert_same_bits(_apply_all_tails(g, b), h.cycle(b))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_special_values_go_by_position(kind, dtype):
    h = _reference("grid_32x32", dtype, (("gamma", 2),))
    g = _matrix(kind, *_input("grid_32x32", dtype)).amg(cycle="w")
    for value in (np.nan, np.inf):
        b = _rhs(1024, dtype)
        b[517] = value
        ref = h.cycle(b)
        assert not np.all(np.isfinite(ref))
        tr.assert_same_bits(_apply_all_tails(g, b), ref)
    zero = _apply_all_tails(g, np.zeros(1024, dtype=dtype))
    tr.assert_same_bits(zero, np.zeros(1024, dtype=dtype))          # +0.0 everywhere
    tr.assert_same_bits(zero, h.cycle(np.zeros(1024, dtype=dtype)))
    # a stored zero diagonal is no error: the text's inf / NaN
    kw = (("coarse_rows", 8),)
    hz = _reference("zero_diagonal", dtype, kw)
    gz = _matrix(kind, *_input("zero_diagonal", dtype)).amg(coarse_rows=8)
    b = _rhs(40, dtype)
    ref = hz.cycle(b)
    assert np.isnan(ref).any() or np.isinf(ref).any()
    tr.assert_same_bits(_apply_all_tails(gz, b), ref)


# ---- 3. apply_dev -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_apply_dev_two_streams_capture_and_aliasing(dtype):
    import torch
    h = _reference("grid_32x32", dtype)
    g = _matrix("csr", *_input("grid_32x32", dtype)).amg()
    g.set_option("amg_tail_rows", 100)                              # wide launches and the tail both take part
    b1, b2 = _rhs(1024, dtype, 1), _rhs(1024, dtype, 2)
    t1, t2 = torch.tensor(b1).cuda(), torch.tensor(b2).cuda()
    x1, x2 = torch.empty_like(t1), torch.empty_like(t2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):                                              # the handle's work vectors are shared: the calls serialise
        g.apply_dev(t1.data_ptr(), x1.data_ptr(), s1)
        g.apply_dev(t2.data_ptr(), x2.data_ptr(), s2)
    s1.synchronize()
    s2.synchronize()
    tr.assert_same_bits(x1.cpu().numpy(), h.cycle(b1))
    tr.assert_same_bits(x2.cpu().numpy(), h.cycle(b2))
    with pytest.raises(sp.Panic, match="x == b"):
        g.apply_dev(t1.data_ptr(), t1.data_ptr(), s1)
    with pytest.raises(sp.Panic, match="handle holds"):
        g.apply_dev(t1.data_ptr(), x1.data_ptr(), s1, dtype=np.float32 if dtype == np.float64 else np.float64)
    # a capturing stream is refused and the capture stays valid
    graph = torch.cuda.CUDAGraph()
    y = torch.zeros_like(t1)
    with torch.cuda.graph(graph, stream=s1):
        with pytest.raises(sp.Panic, match="cannot be captured"):
            g.apply_dev(t1.data_ptr(), x1.data_ptr(), torch.cuda.current_stream())
        y.add_(t1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, t1)


# ---- 4. Krylov ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("method,name", [("cg", "grid_32x32"), ("bicgstab", "grid_32x32"), ("bicgstab", "nonsymmetric_grid")])
def test_krylov_with_amg_is_the_loop(method, name, kind, dtype):
    """The reference loop runs with the device's own (deterministic) product as `mul` and the TEXT's cycle as M^-1."""
    a = _matrix(kind, *_input(name, dtype))
    g = a.amg()
    h = _reference(name, dtype)
    mul = lambda v: a.device().spmv(v)                                                        # noqa: E731
    b = _rhs(1024, dtype, 11)
    tol = 1e-8 if dtype == np.float64 else 1e-4
    for maxit in (0, 1, 7, 200):
        xr, ref = ar.solve(h, mul, b, method, tol, maxit)
        for check_every in ((1, 3, 8) if maxit in (7, 200) else (1,)):
            a.device().set_option("krylov_check_every", check_every)
            x, info = a.solve(b, method, M=g, tol=tol, maxit=maxit)
            tr.assert_same_bits(x, xr)
            assert info.iterations == ref["iterations"] and info.reason == ref["reason"]
            assert np.array([info.residual_sq]).tobytes() == np.array([ref["residual_sq"]]).tobytes()
            k = a.device().describe()["krylov"]
            assert k["precond"] == "amg" and k["preconditioned"] == 1 and k["check_every"] == check_every
        if maxit == 200:
            assert ref["reason"] == 0
            if method == "cg" and dtype == np.float64:
                plain = ar.solve(None, mul, b, method, tol, 1000)[1]["iterations"]
                print("cg iterations: plain", plain, "amg", ref["iterations"])
                assert 2 * ref["iterations"] <= plain, (ref["iterations"], plain)
    # the objects written by the existing calls do not change
    a.solve(b, method, tol=tol, maxit=3)
    assert "precond" not in a.device().describe()["krylov"]


@pytest.mark.parametrize("kind", KINDS)
def test_krylov_accepts_a_hierarchy_of_another_matrix_and_refuses_mismatches(kind):
    dtype = np.float64
    a = _matrix(kind, *_input("grid_32x32", dtype))
    other = _matrix(kind, *_input("nonsymmetric_grid", dtype))
    g = other.amg()
    h = _reference("nonsymmetric_grid", dtype)
    b = _rhs(1024, dtype, 11)
    xr, ref = ar.solve(h, lambda v: a.device().spmv(v), b, "bicgstab", 1e-8, 50)
    x, info = a.solve(b, "bicgstab", M=g, tol=1e-8, maxit=50)
    tr.assert_same_bits(x, xr)
    assert info.iterations == ref["iterations"] and info.reason == ref["reason"]
    with pytest.raises(sp.Panic, match="1023 rows|the hierarchy has 1024 rows"):
        _matrix(kind, *ar.stencil((33, 31), dtype)).solve(_rhs(1023, dtype), M=g)
    a32 = _matrix(kind, *_input("grid_32x32", np.float32))
    with pytest.raises(sp.Panic, match="element sizes"):
        a32.solve(_rhs(1024, np.float32), M=g)
    if sp.device_count() > 1:
        with pytest.raises(sp.Panic, match="devices"):
            a.solve(b, M=g, device=1)
    lib = _ffi.lib()
    info_c = (C.c_byte * 64)()
    x = np.zeros_like(b)
    st = getattr(lib, f"spal_{kind}_krylov_amg_f64")(a.device()._h, 0, None, b.ctypes.data_as(_ffi.f64p), C.c_uint64(1024),
                                                     x.ctypes.data_as(_ffi.f64p), C.c_uint64(1024), C.c_double(1e-8),
                                                     C.c_uint64(5), info_c)
    assert st == _ffi.SPAL_ERR_INVALID_ARGUMENT and "null argument" in lib.spal_last_error().decode()


# ---- 5. lifetime, 6. refusals ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_hierarchy_outlives_its_matrix(kind):
    dtype = np.float64
    a = _matrix(kind, *_input("grid_32x32", dtype))
    g = a.amg()
    a.device().close()
    del a
    sp.cache_trim()
    h = _reference("grid_32x32", dtype)
    b = _rhs(1024, dtype)
    tr.assert_same_bits(g.apply(b), h.cycle(b))
    _check_hierarchy(g, h)
    g.close()
    g.close()


def test_refusals_through_the_abi():
    dtype = np.float64
    a = _matrix("csr", *_input("grid_32x32", dtype))
    g = a.amg()
    b = _rhs(1024, dtype)
    for call in (lambda: a.gmres(b, M=g), lambda: a.solve_block(np.stack([b, b], 1), M=g),
                 lambda: a.gmres_block(np.stack([b, b], 1), M=g), lambda: a.solve(b, M=g, precond_sweeps=3),
                 lambda: a.device().gmres(b, M=g), lambda: a.device().krylov_block(np.stack([b, b], 1), M=g)):
        with pytest.raises(TypeError, match="Amg"):
            call()
    with pytest.raises(sp.Panic, match="b.len\\(\\) = 1023"):
        g.apply(b[:-1])
    with pytest.raises(sp.Panic, match="handle holds f64"):
        g.apply(b.astype(np.float32))
    with pytest.raises(sp.Panic, match="unknown option"):
        g.set_option("tail", 1)
    with pytest.raises(sp.Panic, match="amg_tail_rows must be >= 0"):
        g.set_option("amg_tail_rows", -1)
    with pytest.raises(sp.Panic, match="level = 9"):
        g.level(9)
    # a level-0 row without a stored diagonal: the message names the first such row
    pattern, values = _input("grid_32x32", dtype)
    hole = tr.drop_diagonal(tr.drop_diagonal(pattern, 700), 33)
    keep = np.ones(values.size, dtype=bool)
    keep[ar.diagonal_positions(pattern)[[33, 700]]] = False
    for kind in KINDS:
        with pytest.raises(sp.Panic, match="row 33 stores no diagonal"):
            _matrix(kind, hole, values[keep]).amg()
