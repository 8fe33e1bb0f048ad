"""MINRES on the device against its sequential text (tests/minres_ref.py): raw bits equal, f64 and f32, CSR and CSC, with
and without a preconditioner and a shift, whatever the poll interval, the column tile and the other columns are.

The text runs with the device's own spmv / solve_triangular as callables (those are deterministic, so the comparison is
bit for bit whichever SpMV kernel the plan picks).  Inputs were checked on the CPU with the text first: every solving
case reaches reason 0 inside maxit = 400 with a true relative residual of at most 1.04 tol."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import krylov_ref as kr
from tests import minres_ref as mr
from tests import trsv_ref as tr
from tests.test_gpu_krylov import _pattern, make

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
TOL = {np.float64: 1e-10, np.float32: 1e-5}
MAXIT = 400
G = 4096 * 1024      # the elements one trip of the first-level grid covers


@functools.lru_cache(maxsize=None)
def case(name, dtype, fill="indefinite"):
    """(pattern, values, b).  Shared, read-only."""
    pattern = _pattern(name)
    rng = np.random.default_rng(zlib.crc32(("minres/" + name).encode()))
    values, b = (mr.indefinite_fill if fill == "indefinite" else kr.spd_fill)(pattern, dtype, rng)
    for a in (*pattern[1:], values, b):
        a.setflags(write=False)
    return pattern, values, b


def abs_diagonal(kind, pattern, values):
    """D: the diagonal handle holding |a_ii|; with precond_sweeps=0, M^-1 v = v / |a_ii|."""
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    d = np.abs(values[rows == colind.astype(np.int64)])
    assert d.size == n
    return make(kind, tr.diagonal(n), d)


def device_ops(a, f, sweeps=None):
    """The device's own product and preconditioner as callables for the text."""
    mul = lambda v: a.device().spmv(v)                                                      # noqa: E731
    if f is None:
        return mul, None
    if sweeps is None or sweeps < 0:
        return mul, lambda v: f.solve_triangular(f.solve_triangular(v, True, True), False)
    return mul, lambda v: f.solve_triangular(f.solve_triangular(v, True, True, sweeps=sweeps), False, False, sweeps=sweeps)


def same_result(got, ref, what=""):
    x, info = got
    xr, ir_ = ref
    tr.assert_same_bits(x, xr)
    assert (info.iterations, info.reason) == (ir_["iterations"], ir_["reason"]), what
    tr.assert_same_bits(np.array([info.residual_sq]), np.array([ir_["residual_sq"]]))
    tr.assert_same_bits(np.array([info.rhs_sq]), np.array([ir_["rhs_sq"]]))


# ---- 1. the vector form is the text on the device's own operations ----------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("prec", [False, True], ids=["plain", "D"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("shift", [0.0, 0.25])
@pytest.mark.parametrize("name", ["banded", "bidiagonal", "diagonal", "one"])
def test_minres_is_the_text(name, shift, kind, prec, dtype):
    pattern, values, b = case(name, dtype)
    tol = TOL[dtype]
    a = make(kind, pattern, values)
    f = abs_diagonal(kind, pattern, values) if prec else None
    x, info = a.minres(b, M=f, shift=shift, tol=tol, maxit=MAXIT, precond_sweeps=0 if prec else None)
    ref = mr.minres(*device_ops(a, f, 0), b, np.zeros_like(b), shift, tol, MAXIT)
    print(name, shift, kind, prec, dtype.__name__, "iterations", info.iterations, "true residual / tol",
          mr.true_relative_residual(pattern, values, shift, x, b) / tol)
    same_result((x, info), ref)
    assert info.reason == 0 and x.dtype == dtype
    # the factor 2 covers the drift between the recurrence and the true residual only: the bits are already equal
    assert mr.true_relative_residual(pattern, values, shift, x, b) <= 2 * tol
    d = a.device().describe()["krylov"]
    assert d["method"] == "minres" and d["shift"] == shift and d["preconditioned"] == int(prec)
    assert d["iterations"] == info.iterations and d["reason"] == 0 and d["precond_sweeps"] == (0 if prec else -1)
    assert d["check_every"] == (1 if prec else 8) and d["polls"] >= 1 and d["solve_ms"] > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("sweeps", [None, 2], ids=["exact", "sweeps2"])
def test_minres_on_a_definite_matrix_with_its_ilu0(sweeps, dtype):
    pattern, values, b = case("banded", dtype, "spd")
    tol = TOL[dtype]
    a = make("csr", pattern, values)
    f = a.ilu0()
    x, info = a.minres(b, M=f, tol=tol, maxit=MAXIT, precond_sweeps=sweeps)
    same_result((x, info), mr.minres(*device_ops(a, f, sweeps), b, np.zeros_like(b), 0.0, tol, MAXIT))
    assert info.reason == 0 and kr.true_relative_residual(pattern, values, x, b) <= 2 * tol


# ---- 2. every new update past one trip of the grid ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_case(name, dtype):
    """(pattern, values, b) of G + 1 rows, so that every first-level launch takes a second tile in workgroup 0."""
    n = G + 1
    rng = np.random.default_rng(zlib.crc32(f"minres/long/{name}".encode()))
    if name == "tridiagonal":
        cols = (np.repeat(np.arange(n, dtype=np.int64), 3).reshape(n, 3) + np.array([-1, 0, 1])).ravel()[1:-1]
        rowptr = np.concatenate([[0, 2], 2 + 3 * np.arange(1, n - 1, dtype=np.int64), [3 * n - 2]]).astype(np.uint64)
        pattern = (n, rowptr, cols.astype(np.uint64))
    else:
        pattern = tr.diagonal(n)
    values, b = mr.indefinite_fill(pattern, dtype, rng)
    for a in (*pattern[1:], values, b):
        a.setflags(write=False)
    return pattern, values, b


# V_MR_R0, V_MR_V, V_MR_T1, V_MR_T2, V_MR_WX by the first case; V_MR_T2_PRE (and V_DOT behind M^-1) by the second
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name,prec,maxit", [("tridiagonal", False, 3), ("diagonal", True, 3)], ids=["plain", "D"])
def test_updates_past_one_trip_of_the_grid(name, prec, maxit, dtype):
    pattern, values, b = long_case(name, dtype)
    assert -(-pattern[0] // 1024) == 4096 + 1
    a = make("csr", pattern, values)
    f = abs_diagonal("csr", pattern, values) if prec else None
    x, info = a.minres(b, M=f, shift=0.25, tol=TOL[dtype], maxit=maxit, precond_sweeps=0 if prec else None)
    hp = None
    if prec:
        d = np.abs(values)
        hp = lambda v: v / d                                                               # noqa: E731
    ref = mr.minres(lambda v: a.device().spmv(v), hp, b, np.zeros_like(b), 0.25, TOL[dtype], maxit)
    same_result((x, info), ref)
    assert info.iterations >= 1


# ---- 3. scalars and stopping -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("prec", [False, True], ids=["plain", "D"])
def test_poll_interval_and_maxit_change_no_bit(prec, dtype):
    pattern, values, b = case("banded", dtype)
    tol = TOL[dtype]
    a = make("csr", pattern, values)
    f = abs_diagonal("csr", pattern, values) if prec else None
    ops = device_ops(a, f, 0)
    x0 = np.random.default_rng(3).uniform(-1, 1, size=b.size).astype(dtype)
    full = mr.minres(*ops, b, x0, 0.25, tol, MAXIT)
    assert full[1]["reason"] == 0
    for every in (1, 2, 3, 8):
        a.device().set_option("krylov_check_every", every)
        got = a.minres(b, M=f, shift=0.25, x0=x0, tol=tol, maxit=MAXIT, precond_sweeps=0 if prec else None)
        same_result(got, full, f"check_every {every}")                   # x AT the stop, whatever the interval
        d = a.device().describe()["krylov"]
        assert d["check_every"] == every and d["polls"] == -(-full[1]["iterations"] // every)
    a.device().set_option("krylov_check_every", 3)
    last = np.inf
    for maxit in (0, 1, 4, 7):
        got = a.minres(b, M=f, shift=0.25, x0=x0, tol=tol, maxit=maxit, precond_sweeps=0 if prec else None)
        same_result(got, mr.minres(*ops, b, x0, 0.25, tol, maxit), f"maxit {maxit}")
        assert got[1].reason == 1 and got[1].iterations == maxit and got[1].residual_sq <= last
        last = got[1].residual_sq
        if maxit == 0:
            tr.assert_same_bits(got[0], x0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_breakdowns_are_reasons_not_errors(kind, dtype):
    pattern, values, b = case("diagonal", dtype)
    n = pattern[0]
    a = make(kind, pattern, values)
    x0 = np.random.default_rng(5).uniform(-1, 1, size=n).astype(dtype)
    # M = -I (sweeps 0): dot(r2, y) < 0 -> NaN: reason 2 at it = 0, x is x0
    neg = make(kind, pattern, -np.ones(n, dtype=dtype))
    x, info = a.minres(b, M=neg, x0=x0, tol=TOL[dtype], maxit=20, precond_sweeps=0)
    assert info.reason == 2 and info.iterations == 0 and np.isnan(info.residual_sq) and info.rhs_sq < 0
    tr.assert_same_bits(x, x0)
    same_result((x, info), mr.minres(lambda v: a.device().spmv(v), lambda v: v / dtype(-1), b, x0, 0.0, TOL[dtype], 20))
    # the zero matrix with shift = 0, and shift = d on d I: gamma = 0 -> reason 2, no error
    zero = make(kind, pattern, np.zeros(n, dtype=dtype))
    for m, shift in ((zero, 0.0), (make(kind, pattern, np.full(n, 3, dtype=dtype)), 3.0)):
        x, info = m.minres(b, shift=shift, tol=TOL[dtype], maxit=20)
        assert info.reason == 2 and info.iterations == 1
        same_result((x, info), mr.minres(lambda v: m.device().spmv(v), None, b, np.zeros_like(b), shift, TOL[dtype], 20))
    # b = 0: reason 0 at 0 iterations
    x, info = a.minres(np.zeros_like(b), tol=TOL[dtype], maxit=20)
    assert info.reason == 0 and info.iterations == 0 and not x.any() and info.rhs_sq == 0


# ---- 4. the block form --------------------------------------------------------------------------------------------------

def mixed_block(a_dense_mul, b, x0, k, shift, seed):
    """(B, X0): column 0 random, column 1 zero, column 2 = (A - shift I) x0 for its x0, column 3 holds a NaN; the rest
    random at other scales.  k = 1 keeps the random column alone."""
    rng = np.random.default_rng(seed)
    n = b.size
    B = (rng.uniform(-1, 1, size=(n, k)) * 10.0 ** rng.integers(-2, 3, size=k)).astype(b.dtype)
    X0 = rng.uniform(-1, 1, size=(n, k)).astype(b.dtype)
    B[:, 0] = b
    if k > 1:
        B[:, 1] = 0
        X0[:, 1] = 0
    if k > 2:
        xi = np.round(X0[:, 2] * 8).astype(b.dtype)
        X0[:, 2] = xi
        B[:, 2] = a_dense_mul(xi) - b.dtype.type(shift) * xi
    if k > 3:
        B[n // 2, 3] = np.nan
    return B, X0


def block_dev_call(a, f, shift, B, X0, ldb, ldx, tol, maxit, stream=None):
    """The _dev form on torch tensors with padded rows: NaN in B's padding, a sentinel in X's.  Returns (X, infos)."""
    import torch
    n, k = B.shape
    tdt = torch.float64 if B.dtype == np.float64 else torch.float32
    Bw = torch.full((n, ldb), float("nan"), dtype=tdt, device="cuda")
    Xw = torch.full((n, ldx), -77.0, dtype=tdt, device="cuda")
    Bw[:, :k] = torch.tensor(B).cuda()
    Xw[:, :k] = torch.tensor(X0).cuda()
    torch.cuda.synchronize()
    infos = a.device().minres_block_dev(k, Bw.data_ptr(), ldb, Xw.data_ptr(), ldx, None if f is None else f.device(),
                                        shift, tol, maxit, stream)
    torch.cuda.synchronize()
    Xh, Bh = Xw.cpu().numpy(), Bw.cpu().numpy()
    assert np.all(Xh[:, k:] == -77.0) and np.all(np.isnan(Bh[:, k:]))      # the padding survives
    return np.ascontiguousarray(Xh[:, :k]), infos


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("prec", [False, True], ids=["plain", "D"])
@pytest.mark.parametrize("k", [1, 3, 8, 33])
def test_block_columns_are_the_vector_calls(k, prec, dtype):
    """values scaled to quarters of integers on the bidiagonal pattern keep column 2's b = (A - shift I) x0 exact"""
    pattern, values, b = case("bidiagonal", dtype)
    values = (np.round(values * 4) / 4).astype(dtype)
    tol, shift, maxit = TOL[dtype], 0.25, 60
    a = make("csr", pattern, values)
    a.device().set_option("stream_row_max", 1024)      # every row through the stream kernel: sequential sums
    assert a.device().describe()["kernel"] == "stream"
    f = abs_diagonal("csr", pattern, values) if prec else None
    sweeps = 0 if prec else None
    B, X0 = mixed_block(lambda v: a.device().spmv(v), b, None, k, shift, 11 + k)
    singles = [a.minres(np.ascontiguousarray(B[:, j]), M=f, shift=shift, x0=np.ascontiguousarray(X0[:, j]), tol=tol,
                        maxit=maxit, precond_sweeps=sweeps) for j in range(k)]
    if k > 1:
        assert singles[1][1].reason == 0 and singles[1][1].iterations == 0
    if k > 2:
        assert singles[2][1].reason == 0 and singles[2][1].iterations == 0
    if k > 3:
        assert singles[3][1].reason == 2
    assert singles[0][1].iterations > 3

    def same_as_singles(X, infos, what):
        assert X.shape == B.shape and len(infos) == k
        for j in range(k):
            ref = (singles[j][0], dict(singles[j][1]))
            same_result((np.ascontiguousarray(X[:, j]), infos[j]), ref, f"{what}, column {j}")
        assert len({i.solve_ms for i in infos}) == 1

    for tile in (0, 1, 4):
        a.device().set_option("krylov_tile", tile)
        same_as_singles(*a.minres_block(B, M=f, shift=shift, X0=X0, tol=tol, maxit=maxit, precond_sweeps=sweeps), f"tile {tile}")
        d = a.device().describe()["krylov_block"]
        assert d["method"] == "minres" and d["shift"] == shift and d["k"] == k and (tile == 0 or d["tile"] == tile)
        same_as_singles(*block_dev_call(a, f, shift, B, X0, k + 3, k + 1, tol, maxit), f"tile {tile}, padded")
    a.device().set_option("krylov_tile", 0)
    for every in (1, 3, 8):
        a.device().set_option("krylov_check_every", every)
        same_as_singles(*a.minres_block(B, M=f, shift=shift, X0=X0, tol=tol, maxit=maxit, precond_sweeps=sweeps),
                        f"check_every {every}")


# ---- 5. streams, capture, refusals ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_dev_forms_on_a_side_stream(dtype):
    import torch
    pattern, values, b = case("banded", dtype)
    tol = TOL[dtype]
    a = make("csr", pattern, values)
    f = abs_diagonal("csr", pattern, values)
    f.device().set_option("trsv_sweeps", 0)
    want = a.minres(b, M=f, shift=0.25, tol=tol, maxit=MAXIT)
    s = torch.cuda.Stream()
    bt = torch.tensor(np.array(b)).cuda()
    xt = torch.zeros_like(bt)
    torch.cuda.synchronize()
    info = a.device().minres_dev(bt.data_ptr(), xt.data_ptr(), f.device(), 0.25, tol, MAXIT, s)
    same_result((xt.cpu().numpy(), info), (want[0], dict(want[1])))
    B = np.ascontiguousarray(np.stack([b, 2 * b], axis=1))
    X, infos = block_dev_call(a, f, 0.25, B, np.zeros_like(B), 5, 2, tol, MAXIT, stream=s)
    wantb = a.minres_block(B, M=f, shift=0.25, tol=tol, maxit=MAXIT)
    for j in range(2):
        same_result((np.ascontiguousarray(X[:, j]), infos[j]), (np.ascontiguousarray(wantb[0][:, j]), dict(wantb[1][j])))


@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_refusals_on_a_device(kind):
    import torch
    lib = _ffi.lib()
    pattern, values, b = case("banded", np.float64)
    n = pattern[0]
    a = make(kind, pattern, values)
    dev = a.device()
    host = getattr(lib, f"spal_{kind}_minres_f64")
    devf = getattr(lib, f"spal_{kind}_minres_dev_f64")
    blockf = getattr(lib, f"spal_{kind}_minres_block_f64")
    info = (sp.matrix._KrylovInfoC * 2)()
    x = np.zeros(n)
    B = np.ascontiguousarray(np.stack([b, b], axis=1))
    X = np.zeros_like(B)
    pb, px = b.ctypes.data_as(_ffi.f64p), x.ctypes.data_as(_ffi.f64p)
    pB, pX = B.ctypes.data_as(_ffi.f64p), X.ctypes.data_as(_ffi.f64p)
    u, d = C.c_uint64, C.c_double

    def call(h=dev._h, m=None, shift=0.0, b_len=n, x_len=n, tol=1e-10):
        return host(h, m, d(shift), pb, u(b_len), px, u(x_len), d(tol), u(5), info)

    def block(h=dev._h, m=None, shift=0.0, k=2, ldb=2, ldx=2, b_rows=n, x_rows=n):
        return blockf(h, m, d(shift), u(k), pB, u(ldb), u(b_rows), pX, u(ldx), u(x_rows), d(1e-10), u(5), info)

    def refused(text, got, who=f"spal_{kind}_minres:"):
        assert got == _ffi.SPAL_ERR_INVALID_ARGUMENT, lib.spal_last_error()
        msg = lib.spal_last_error().decode()
        assert text in msg and msg.startswith(who), msg

    for bad in (float("nan"), float("inf"), float("-inf")):
        refused("must be finite", call(shift=bad))
        refused("must be finite", block(shift=bad), f"spal_{kind}_minres_block:")
    refused("b.len()", call(b_len=n - 1))
    for bad in (-1e-3, float("nan")):
        refused("must be >= 0", call(tol=bad))
    f32 = make(kind, pattern, values.astype(np.float32)).device()
    refused("handle holds f32 values", call(h=f32._h))
    refused("element sizes 8 and 4", call(m=f32._h))
    small = make(kind, *case("diagonal", np.float64)[:2]).device()
    refused("the preconditioner is 1025 x 1025", call(m=small._h))
    blk = f"spal_{kind}_minres_block:"
    refused("k = 0", block(k=0), blk)
    refused("ldb = 1 is less than k = 2", block(ldb=1), blk)
    refused("ldx = 1 is less than k = 2", block(ldx=1), blk)
    refused(f"B has {n - 1} rows", block(b_rows=n - 1), blk)
    bt = torch.tensor(np.array(b)).cuda()
    refused("x_dev == b_dev", devf(dev._h, None, d(0.0), C.c_void_p(bt.data_ptr()), C.c_void_p(bt.data_ptr()), d(1e-10),
                                   u(5), None, info), f"spal_{kind}_minres_dev:")
    # a capturing stream: refused, and the capture is the caller's to end
    xt = torch.zeros_like(bt)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            got = devf(dev._h, None, d(0.0), C.c_void_p(bt.data_ptr()), C.c_void_p(xt.data_ptr()), d(1e-10), u(5),
                       C.c_void_p(s.cuda_stream), info)
            msg = lib.spal_last_error().decode()
        finally:
            g.capture_end()
    assert got == _ffi.SPAL_ERR_INVALID_ARGUMENT and "cannot be captured into a graph" in msg
    # the existing entry points still have two methods
    assert lib.spal_csr_krylov_f64(dev._h if kind == "csr" else None, 2, None, pb, u(n), px, u(n), d(1e-10), u(5),
                                   info) == _ffi.SPAL_ERR_INVALID_ARGUMENT


def test_row_block_handles_are_refused(monkeypatch):
    """a handle held as row blocks (the limit lowered for the test) has no MINRES, as A or as M"""
    import spal_synth as synth
    rp, ci, va = synth.banded_csr(2000, 2000, 4, 64, 3)
    monkeypatch.setenv("SPAL_CSR_PART_ENTRIES", "3000")
    big = sp.CsrMatrix(2000, 2000, rp, ci, va)
    assert big.device().describe()["kernel"] == "row_blocks"
    monkeypatch.delenv("SPAL_CSR_PART_ENTRIES")
    small = sp.CsrMatrix(2000, 2000, rp, ci, va)
    for a, m in ((big, None), (small, big)):
        with pytest.raises(sp.SpalError, match="spal_csr_minres: .*row blocks") as e:
            a.minres(np.ones(2000), M=m, maxit=3)
        assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED
        with pytest.raises(sp.SpalError, match="spal_csr_minres_block: .*row blocks") as e:
            a.minres_block(np.ones((2000, 2)), M=m, maxit=3)
        assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED
