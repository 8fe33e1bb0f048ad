"""CG and BiCGStab on a block of right-hand sides (spal_*_krylov_block_*) against the sequential text, column
by column: raw bits of x, iterations, reason, residual_sq and rhs_sq, f64 and f32, CSR and CSC, with and without a factor.

The reference for column j is the tests/krylov_ref.py loop on B[:, j] and X0[:, j], fed by the device's own operations
on that one column -- spmm on an (n, 1) block, solve_triangular / its sweeps on the factor -- and, for one case per
method, by pure host operations (oracle.csr_spmv, trsv_ref.solve_by_levels).  Nothing in the reference knows about the
other columns, the leading dimensions, the column tile or the poll interval.

The inputs of the mixed block (a zero column, a NaN column, a column that reaches maxit, columns in the span of 1, 2, 3
and 6 eigenvectors, which Krylov methods solve in that many iterations) were tried on the CPU first; the test asserts
the mix from the reference, it does not skip."""
import ctypes as C
import functools
import threading
import zlib

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import ilu_ref as ir
from tests import krylov_ref as kr
from tests import solver_cases as sc
from tests import trsv_ref as tr
from tests.test_gpu_krylov import MAXIT, TOL, case, make

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
# rows one trip of the block first-level grid covers: 1024 workgroups along the rows (kBlockMaxGrid in
# spal_krylov_block.hip), a tile of 1024 rows each.  LONG_N = that + 1: workgroup 0 alone takes a second tile, and the
# 1025 tile sums need two upper levels (1025 -> 2 -> 1).
BLOCK_G = 1024 * 1024
LONG_N = BLOCK_G + 1


# ---- the per-column reference -----------------------------------------------------------------------------------------

def column_ops(a, f, sweeps=None, count=None):
    """The device's own product and preconditioner on ONE column, as callables for the reference loops.  `count`: a
    list whose first element counts the products."""
    dev = a.device()

    def mul(v):
        if count is not None:
            count[0] += 1
        return dev.spmm(np.ascontiguousarray(v.reshape(-1, 1)))[:, 0]

    if f is None:
        return mul, None
    if sweeps is None or sweeps < 0:
        return mul, lambda v: f.solve_triangular(f.solve_triangular(v, True, True), False)
    return mul, lambda v: f.solve_triangular(f.solve_triangular(v, True, True, sweeps=sweeps), False, False, sweeps=sweeps)


def reference(method, ops, B, X0, tol, maxit):
    return [kr.METHODS[method](*ops, np.ascontiguousarray(B[:, j]), np.ascontiguousarray(X0[:, j]), tol, maxit)
            for j in range(B.shape[1])]


def same_column(x, info, ref, what=""):
    xr, ir_ = ref
    tr.assert_same_bits(x, xr)
    assert (info.iterations, info.reason) == (ir_["iterations"], ir_["reason"]), what
    tr.assert_same_bits(np.array([info.residual_sq]), np.array([ir_["residual_sq"]]))
    tr.assert_same_bits(np.array([info.rhs_sq]), np.array([ir_["rhs_sq"]]))


def same_block(got, refs):
    X, infos = got
    assert X.shape[1] == len(infos) == len(refs)
    for j, ref in enumerate(refs):
        same_column(np.ascontiguousarray(X[:, j]), infos[j], ref, f"column {j}")
    assert len({i.solve_ms for i in infos}) == 1 and infos[0].solve_ms > 0


def block_of(b, k, seed):
    """(n, k): column 0 is b, the others uniform(-1, 1) scaled by powers of ten, so that no two columns agree."""
    rng = np.random.default_rng(seed)
    B = rng.uniform(-1, 1, size=(b.size, k)) * 10.0 ** rng.integers(-2, 3, size=k)
    B[:, 0] = b
    return B.astype(b.dtype)


# ---- 1. the matrices of the vector solver's tests ----------------------------------------------------------------------

# (matrix, method, kind, with M = a.ilu0(), dtype, k): k in {1, 2, 3, 5, 8, 17, 33, 70} spread over the cases
BLOCK_CASES = [
    ("banded", "cg", "csr", False, np.float64, 3),
    ("banded", "cg", "csc", True, np.float32, 2),
    ("banded", "bicgstab", "csr", True, np.float64, 5),
    ("banded", "bicgstab", "csc", False, np.float32, 2),
    ("full", "bicgstab", "csr", False, np.float64, 2),
    ("full", "bicgstab", "csc", True, np.float32, 3),
    ("bidiagonal", "cg", "csr", True, np.float64, 8),
    ("bidiagonal", "cg", "csc", False, np.float32, 1),
    ("bidiagonal", "bicgstab", "csc", True, np.float32, 5),
    ("diagonal", "cg", "csr", False, np.float64, 17),
    ("diagonal", "bicgstab", "csr", True, np.float32, 33),
    ("diagonal", "bicgstab", "csc", False, np.float64, 8),
    ("one", "cg", "csr", False, np.float64, 70),
    ("one", "bicgstab", "csc", True, np.float32, 70),
]


@pytest.mark.parametrize("name,method,kind,prec,dtype,k", BLOCK_CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[2]}-{'ilu0' if c[3] else 'plain'}-{np.dtype(c[4]).name}-k{c[5]}"
                              for c in BLOCK_CASES])
def test_every_column_is_the_reference_loop(name, method, kind, prec, dtype, k):
    pattern, values, b = case(name, method, dtype)
    tol = TOL[dtype]
    maxit = MAXIT
    a = make(kind, pattern, values)
    f = a.ilu0() if prec else None
    B = block_of(b, k, zlib.crc32(f"{name}{method}{k}".encode()))
    got = a.solve_block(B, method, M=f, tol=tol, maxit=maxit)
    refs = reference(method, column_ops(a, f), B, np.zeros_like(B), tol, maxit)
    same_block(got, refs)
    assert got[0].dtype == dtype and got[0].shape == B.shape
    assert all(i.reason == 0 for i in got[1])
    if prec and name in ("bidiagonal", "diagonal", "one"):
        assert all(i.iterations == 1 for i in got[1])     # M = A exactly: BiCGStab leaves by the half-step exit
    d = a.device().describe()["krylov_block"]
    assert d["method"] == method and d["k"] == k and d["preconditioned"] == int(prec)
    assert d["precond_sweeps"] == -1 and d["tile"] == min(32, 1 << (k - 1).bit_length())
    assert d["iterations_min"] == min(i.iterations for i in got[1])
    assert d["iterations_max"] == max(i.iterations for i in got[1])
    assert d["converged"] == sum(i.reason == 0 for i in got[1])
    assert d["check_every"] == (1 if prec else 8) and d["polls"] >= 1 and d["solve_ms"] > 0
    assert "krylov" not in a.device().describe()           # the vector calls' object stays theirs


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_block_against_pure_host_operations(oracle, method, dtype):
    pattern, values, b = case("bidiagonal", method, dtype)
    n, rowptr, colind = pattern
    tol = TOL[dtype]
    fv = ir.ilu0_rows(n, rowptr, colind, values)
    mul = lambda v: oracle.csr_spmv(rowptr, colind, values, v)                               # noqa: E731
    hp = lambda v: tr.solve_by_levels(n, rowptr, colind, fv,                                # noqa: E731
                                      tr.solve_by_levels(n, rowptr, colind, fv, v, True, True), False, False)
    a = make("csr", pattern, values)
    B = block_of(b, 3, 5)
    X0 = np.zeros_like(B)
    same_block(a.solve_block(B, method, tol=tol, maxit=MAXIT), reference(method, (mul, None), B, X0, tol, MAXIT))
    same_block(a.solve_block(B, method, M=a.ilu0(), tol=tol, maxit=MAXIT), reference(method, (mul, hp), B, X0, tol, MAXIT))


# ---- 2. a block whose columns stop at different points -----------------------------------------------------------------

MIX_N = 1100
MIX_MAXIT = 8


@functools.lru_cache(maxsize=None)
def mixed_case(dtype):
    """A symmetric positive definite banded matrix of 1100 rows (two tiles) and eight right-hand sides:
    0 zeros (reason 0 at it = 0); 1 holds a NaN (reason 2 at it = 0); 2, 7, 3, 4 lie in the span of 1, 2, 3, 6
    eigenvectors (that many iterations; BiCGStab tends to finish them in a half step); 5 is in general position (the
    condition number is 11: not solved in 8 iterations, reason 1); 6 is in general position and starts near its
    solution."""
    rng = np.random.default_rng(20261019)
    pattern = ir.sym(tr.banded(MIX_N, 3, 30, rng))
    values, _ = kr.spd_fill(pattern, np.float64, rng)
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))
    dense = np.zeros((n, n))
    dense[rows, colind.astype(np.int64)] = values
    _, v = np.linalg.eigh(dense)
    B = np.zeros((n, 8))
    B[:, 1] = rng.uniform(-1, 1, n)
    B[77, 1] = np.nan
    B[:, 2] = v[:, 40]
    B[:, 3] = v[:, [3, 500, 900]].sum(axis=1)
    B[:, 4] = v[:, [10, 200, 400, 600, 800, 1000]].sum(axis=1)
    B[:, 5] = rng.uniform(-1, 1, n)
    B[:, 6] = rng.uniform(-1, 1, n)
    B[:, 7] = v[:, [1, 2]].sum(axis=1)
    X0 = np.zeros((n, 8))
    X0[:, 6] = np.linalg.solve(dense, B[:, 6]) * (1 + 1e-3)
    out = pattern, values.astype(dtype), B.astype(dtype), X0.astype(dtype)
    for arr in (*pattern[1:], *out[1:]):
        arr.setflags(write=False)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_columns_that_stop_at_different_points(method, kind, dtype):
    pattern, values, B, X0 = mixed_case(dtype)
    tol = TOL[dtype]
    a = make(kind, pattern, values)
    refs, half = [], []
    for j in range(B.shape[1]):
        count = [0]
        ref = kr.METHODS[method](*column_ops(a, None, count=count), np.ascontiguousarray(B[:, j]),
                                 np.ascontiguousarray(X0[:, j]), tol, MIX_MAXIT)
        refs.append(ref)
        # BiCGStab multiplies once for r0 and twice per iteration, but once in an iteration that leaves by the half step
        half.append(method == "bicgstab" and ref[1]["iterations"] > 0 and count[0] == 2 * ref[1]["iterations"])
    its = [r[1]["iterations"] for r in refs]
    reasons = [r[1]["reason"] for r in refs]
    assert (its[0], reasons[0]) == (0, 0) and (its[1], reasons[1]) == (0, 2) and (its[5], reasons[5]) == (MIX_MAXIT, 1)
    assert len(set(its)) >= 3 and set(reasons) == {0, 1, 2}
    if method == "bicgstab":
        moved = [h for h, it in zip(half, its) if it > 0]
        assert any(moved) and not all(moved)                 # some columns leave by the half-step exit, some do not
    for every in (1, 8):
        a.device().set_option("krylov_check_every", every)
        got = a.solve_block(B, method, X0=X0, tol=tol, maxit=MIX_MAXIT)
        same_block(got, refs)                                # a finished column's x is what it was at ITS stop
    tr.assert_same_bits(got[0][:, 0], X0[:, 0])
    tr.assert_same_bits(got[0][:, 1], X0[:, 1])              # the NaN column never moved
    # ... and the NaN column left every other column alone: the same block with that column replaced
    B2 = B.copy()
    B2[:, 1] = B[:, 5]
    other = a.solve_block(B2, method, X0=X0, tol=tol, maxit=MIX_MAXIT)
    keep = [0, 2, 3, 4, 5, 6, 7]
    tr.assert_same_bits(other[0][:, keep], got[0][:, keep])
    tr.assert_same_bits(other[0][:, 1], got[0][:, 5])
    for j in keep:      # (a NaN residual_sq is column 1's alone)
        assert (other[1][j].iterations, other[1][j].reason, other[1][j].residual_sq) == \
               (got[1][j].iterations, got[1][j].reason, got[1][j].residual_sq)
    d = a.device().describe()["krylov_block"]
    assert (d["iterations_min"], d["iterations_max"], d["converged"]) == (0, MIX_MAXIT, sum(r == 0 for r in reasons))


# ---- 3. the bits do not depend on the geometry --------------------------------------------------------------------------

def dev_call(a, f, method, B, X0, ldb, ldx, tol, maxit, stream=None):
    """The _dev form on torch tensors with padded rows: NaN in B's padding, a sentinel in X's.  Returns (X, infos)."""
    import torch
    n, k = B.shape
    tdt = torch.float64 if B.dtype == np.float64 else torch.float32
    Bw = torch.full((n, ldb), float("nan"), dtype=tdt, device="cuda")
    Xw = torch.full((n, ldx), -77.0, dtype=tdt, device="cuda")
    Bw[:, :k] = torch.tensor(B).cuda()
    Xw[:, :k] = torch.tensor(X0).cuda()
    torch.cuda.synchronize()
    infos = a.device().krylov_block_dev(k, Bw.data_ptr(), ldb, Xw.data_ptr(), ldx, method,
                                        None if f is None else f.device(), tol, maxit, stream)
    torch.cuda.synchronize()
    Xh, Bh = Xw.cpu().numpy(), Bw.cpu().numpy()
    assert np.all(Xh[:, k:] == -77.0) and np.all(np.isnan(Bh[:, k:]))      # the padding survives
    tr.assert_same_bits(Bh[:, :k], B)
    return np.ascontiguousarray(Xh[:, :k]), infos


@pytest.mark.parametrize("method,prec", [("cg", True), ("bicgstab", False)], ids=["cg-ilu0", "bicgstab-plain"])
def test_tile_poll_interval_and_leading_dimensions_change_nothing(method, prec):
    dtype = np.float64
    pattern, values, b = case("banded", method, dtype)
    a = make("csr", pattern, values)
    f = a.ilu0() if prec else None
    k, tol, maxit = 5, TOL[dtype], 12          # at most 12 iterations: the columns stop at different points or not at all
    B = block_of(b, k, 31)
    B[:, 3] = 0                                  # ... but one that stops at once
    X0 = np.zeros_like(B)
    singles = [a.solve_block(np.ascontiguousarray(B[:, j:j + 1]), method, M=f, tol=tol, maxit=maxit) for j in range(k)]

    def same_as_singles(X, infos):
        for j in range(k):
            tr.assert_same_bits(X[:, j], singles[j][0][:, 0])
            s = singles[j][1][0]
            assert (infos[j].iterations, infos[j].reason, infos[j].residual_sq, infos[j].rhs_sq) == \
                   (s.iterations, s.reason, s.residual_sq, s.rhs_sq)

    itmax = max(s[1][0].iterations for s in singles)
    assert singles[3][1][0].iterations == 0 and itmax > 3
    for tile in (1, 2, 4, 8, 16, 32):
        a.device().set_option("krylov_tile", tile)
        same_as_singles(*a.solve_block(B, method, M=f, tol=tol, maxit=maxit))
        assert a.device().describe()["krylov_block"]["tile"] == tile
    a.device().set_option("krylov_tile", 0)
    for every in (1, 3, 8, 64):
        a.device().set_option("krylov_check_every", every)
        same_as_singles(*a.solve_block(B, method, M=f, tol=tol, maxit=maxit))
        d = a.device().describe()["krylov_block"]
        assert d["check_every"] == every and d["polls"] == -(-itmax // every)      # the poll after the last stop is the last
    for ldb, ldx, tile in ((5, 9, 0), (8, 5, 2), (11, 7, 4)):
        a.device().set_option("krylov_tile", tile)
        same_as_singles(*dev_call(a, f, method, B, X0, ldb, ldx, tol, maxit))
    with pytest.raises(sp.Panic, match="krylov_tile must be 0"):
        a.device().set_option("krylov_tile", 3)


# ---- 4. the vector call -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
@pytest.mark.parametrize("name", ["banded", "bidiagonal"])
def test_a_column_is_what_the_vector_call_returns(name, method, dtype):
    pattern, values, b = case(name, method, dtype)
    tol = TOL[dtype]
    a = make("csr", pattern, values)
    a.device().set_option("stream_row_max", 1024)      # every row through the stream kernel: sequential sums
    assert a.device().describe()["kernel"] == "stream"
    f = a.ilu0()
    B = block_of(b, 3, 8)
    for M in (None, f):
        X, infos = a.solve_block(B, method, M=M, tol=tol, maxit=MAXIT)
        for j in range(3):
            x, info = a.solve(np.ascontiguousarray(B[:, j]), method, M=M, tol=tol, maxit=MAXIT)
            tr.assert_same_bits(X[:, j], x)
            assert (infos[j].iterations, infos[j].reason) == (info.iterations, info.reason)
            assert (infos[j].residual_sq, infos[j].rhs_sq) == (info.residual_sq, info.rhs_sq)


# ---- 5. the shapes of the reduction ---------------------------------------------------------------------------------------

def diagonal_system(n, k, dtype, seed):
    rng = np.random.default_rng(seed)
    pattern = tr.diagonal(n)
    values = rng.uniform(0.5, 2, size=n).astype(dtype)
    return pattern, values, rng.uniform(-1, 1, size=(n, k)).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025])
def test_tile_boundaries(n, method, dtype):
    pattern, values, B = diagonal_system(n, 3, dtype, n)
    a = make("csr", pattern, values)
    hm = lambda v: values * v                                                                # noqa: E731
    got = a.solve_block(B, method, tol=TOL[dtype], maxit=6)
    same_block(got, reference(method, (hm, None), B, np.zeros_like(B), TOL[dtype], 6))


# (method, with M = the matrix itself, maxit).  With more tiles than first-level workgroups and two upper levels, between
# them: V_INIT, V_COPY_DOT, V_DOT, V_CG_XR, V_CG_P (CG); V_BI_P, V_BI_S, V_DOT2, V_BI_XR (BiCGStab, plain); V_BI_HALF
# (BiCGStab with M = A: the half-step exit).  A diagonal matrix's product and solve are one rounding each on the host.
LONG_BLOCK = [("cg", False, 2), ("bicgstab", False, 2), ("bicgstab", True, MAXIT), ("cg", True, MAXIT)]


@functools.lru_cache(maxsize=None)
def long_system(dtype):
    out = diagonal_system(LONG_N, 2, dtype, 99)
    for arr in (out[1], out[2]):
        arr.setflags(write=False)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("method,prec,maxit", LONG_BLOCK, ids=["cg", "bicgstab", "bicgstab-half-step", "cg-m"])
def test_more_tiles_than_workgroups_and_two_upper_levels(method, prec, maxit, dtype):
    pattern, values, B = long_system(dtype)
    assert -(-LONG_N // 1024) == 1024 + 1
    a = make("csr", pattern, values)
    hm = lambda v: values * v                                                                # noqa: E731
    hp = (lambda v: v / values) if prec else None      # the unit lower solve of a diagonal matrix copies, the upper divides
    got = a.solve_block(B, method, M=a if prec else None, tol=TOL[dtype], maxit=maxit)
    same_block(got, reference(method, (hm, hp), B, np.zeros_like(B), TOL[dtype], maxit))
    if prec:
        assert all((i.reason, i.iterations) == (0, 1) for i in got[1])
    else:
        assert all((i.reason, i.iterations) == (1, maxit) for i in got[1])


# ---- 6. other behaviour ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_maxit_zero_and_a_solved_start(method, kind):
    pattern, values, b = case("banded", method, np.float64)
    a = make(kind, pattern, values)
    B = block_of(b, 3, 12)
    X0 = np.random.default_rng(5).uniform(-1, 1, size=B.shape)
    X, infos = a.solve_block(B, method, X0=X0, tol=1e-10, maxit=0)
    tr.assert_same_bits(X, X0)
    mul = column_ops(a, None)[0]
    for j, info in enumerate(infos):
        r0 = B[:, j] - mul(np.ascontiguousarray(X0[:, j]))
        assert (info.iterations, info.reason) == (0, 1)
        assert info.residual_sq == float(kr.dot(r0, r0)) and info.rhs_sq == float(kr.dot(B[:, j], B[:, j]))
    exact = a.solve_block(B, method, tol=1e-10, maxit=MAXIT)[0]
    X, infos = a.solve_block(B, method, X0=exact, tol=1e-8, maxit=MAXIT)
    assert all((i.iterations, i.reason) == (0, 0) for i in infos)
    tr.assert_same_bits(X, exact)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_zero_matrix_breaks_down_in_every_column(method, dtype):
    pattern, _, b = case("banded", method, dtype)
    a = make("csr", pattern, np.zeros(pattern[2].size, dtype=dtype))
    B = block_of(b, 3, 4)
    X, infos = a.solve_block(B, method, tol=TOL[dtype], maxit=MAXIT)
    assert all((i.reason, i.iterations) == (2, 1) and not np.isfinite(i.residual_sq) for i in infos)
    same_block((X, infos), reference(method, column_ops(a, None), B, np.zeros_like(B), TOL[dtype], MAXIT))


@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_refusals(kind):
    import torch
    lib = _ffi.lib()
    pattern, values, b = case("full", "bicgstab", np.float64)
    n = pattern[0]
    a = make(kind, pattern, values)
    dev = a.device()
    host = getattr(lib, f"spal_{kind}_krylov_block_f64")
    devf = getattr(lib, f"spal_{kind}_krylov_block_dev_f64")
    cinfo = (sp.matrix._KrylovInfoC * 2)()
    B = block_of(b, 2, 1)
    X = np.zeros_like(B)
    pb, px = B.ctypes.data_as(_ffi.f64p), X.ctypes.data_as(_ffi.f64p)
    u = C.c_uint64

    def call(h=dev._h, method=1, m=None, k=2, b_=pb, ldb=2, b_rows=n, x_=px, ldx=2, x_rows=n, tol=1e-10, info=cinfo):
        return host(h, method, m, u(k), b_, u(ldb), u(b_rows), x_, u(ldx), u(x_rows), C.c_double(tol), u(5), info)

    def refused(status, text, got):
        assert got == status, lib.spal_last_error()
        msg = lib.spal_last_error().decode()
        assert text in msg and msg.startswith(f"spal_{kind}_krylov_block:"), msg

    inv = _ffi.SPAL_ERR_INVALID_ARGUMENT
    refused(inv, "null argument", call(h=None))
    refused(inv, "null argument", call(b_=None))
    refused(inv, "null argument", call(x_=None))
    refused(inv, "null argument", call(info=None))
    refused(inv, "k = 0", call(k=0))
    refused(inv, "ldb = 1 is less than k = 2", call(ldb=1))
    refused(inv, "ldx = 1 is less than k = 2", call(ldx=1))
    refused(inv, f"B has {n - 1} rows", call(b_rows=n - 1))
    refused(inv, f"X has {n + 1} rows", call(x_rows=n + 1))
    refused(inv, "method = 2 must be 0 (CG) or 1 (BiCGStab)", call(method=2))
    for bad in (-1e-3, float("nan")):
        refused(inv, "must be >= 0", call(tol=bad))
    f32 = make(kind, pattern, values.astype(np.float32)).device()
    refused(inv, "handle holds f32 values", call(h=f32._h))
    refused(inv, "element sizes 8 and 4", call(m=f32._h))
    cls = sp.CsrMatrix if kind == "csr" else sp.CscMatrix
    rect = cls(2, 3, [0, 1, 2] if kind == "csr" else [0, 1, 2, 2], [0, 1], np.array([1.0, 2.0])).device()
    refused(inv, "not square (2 x 3)", call(h=rect._h, b_rows=2, x_rows=2))
    small = make(kind, *case("diagonal", "cg", np.float64)[:2]).device()
    refused(inv, "the preconditioner is 1025 x 1025", call(m=small._h))
    nodiag_pattern = tr.drop_diagonal(pattern, 7)
    nodiag = make(kind, nodiag_pattern, np.ones(nodiag_pattern[2].size)).device()
    assert call(m=nodiag._h) == inv and "row 7 stores no diagonal entry" in lib.spal_last_error().decode()
    bt = torch.tensor(B).cuda()
    refused(inv, "x_dev == b_dev", devf(dev._h, 1, None, u(2), C.c_void_p(bt.data_ptr()), u(2), C.c_void_p(bt.data_ptr()),
                                         u(2), C.c_double(1e-10), u(5), None, cinfo))
    # a capturing stream: refused, and the capture is the caller's to end
    xt = torch.zeros_like(bt)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            got = devf(dev._h, 1, None, u(2), C.c_void_p(bt.data_ptr()), u(2), C.c_void_p(xt.data_ptr()), u(2),
                       C.c_double(1e-10), u(5), C.c_void_p(s.cuda_stream), cinfo)
            msg = lib.spal_last_error().decode()
        finally:
            g.capture_end()
    assert got == inv and "cannot be captured into a graph" in msg
    # Python's own refusals
    with pytest.raises(sp.Panic, match=r"X0 has shape \(3, 2\)"):
        a.solve_block(B, X0=np.zeros((3, 2)))
    with pytest.raises(sp.Panic, match=r"B has shape"):
        a.solve_block(b)
    with pytest.raises(sp.Panic, match=r"solve: b has shape"):
        a.solve(B)


def test_row_block_handles_are_refused(monkeypatch):
    """a handle held as row blocks (the limit lowered for the test) has no block solver, as A or as M"""
    import spal_synth as synth
    rp, ci, va = synth.banded_csr(2000, 2000, 4, 64, 3)
    monkeypatch.setenv("SPAL_CSR_PART_ENTRIES", "3000")
    big = sp.CsrMatrix(2000, 2000, rp, ci, va)
    assert big.device().describe()["kernel"] == "row_blocks"
    monkeypatch.delenv("SPAL_CSR_PART_ENTRIES")
    small = sp.CsrMatrix(2000, 2000, rp, ci, va)
    B = np.ones((2000, 2))
    for a, m in ((big, None), (small, big)):
        for method in ("cg", "bicgstab"):
            with pytest.raises(sp.SpalError, match="spal_csr_krylov_block: .*row blocks") as e:
                a.solve_block(B, method, M=m, maxit=3)
            assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_dev_form_on_a_side_stream_with_strided_tensors(kind, dtype):
    import torch
    pattern, values, b = case("banded", "bicgstab", dtype)
    a = make(kind, pattern, values)
    f = a.ilu0()
    B = block_of(b, 3, 21)
    tol = TOL[dtype]
    want = a.solve_block(B, "bicgstab", M=f, tol=tol, maxit=MAXIT)
    s = torch.cuda.Stream()
    got = dev_call(a, f, "bicgstab", B, np.zeros_like(B), 7, 4, tol, MAXIT, stream=s)
    tr.assert_same_bits(got[0], want[0])
    assert [(i.iterations, i.reason, i.residual_sq) for i in got[1]] == \
           [(i.iterations, i.reason, i.residual_sq) for i in want[1]]
    f.device().set_option("trsv_sweeps", 2)      # the sweeps go through the side stream's scratch block, grown before the loop
    want = a.solve_block(B, "bicgstab", M=f, tol=tol, maxit=6)
    same_block(want, reference("bicgstab", column_ops(a, f, sweeps=2), B, np.zeros_like(B), tol, 6))
    got = dev_call(a, f, "bicgstab", B, np.zeros_like(B), 7, 4, tol, 6, stream=s)
    tr.assert_same_bits(got[0], want[0])
    assert a.device().describe()["krylov_block"]["precond_sweeps"] == 2


@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_two_threads_solve_blocks_on_one_handle(kind):
    pattern, values, b = case("banded", "bicgstab", np.float64)
    a = make(kind, pattern, values)
    f = a.ilu0()
    Bs = [block_of(b, 3, 1), block_of(b, 5, 2)]
    expect = [a.solve_block(B, "bicgstab", M=f, tol=1e-10, maxit=MAXIT) for B in Bs]
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i):
        try:
            gate.wait(timeout=30)
            results[i] = a.solve_block(Bs[i], "bicgstab", M=f, tol=1e-10, maxit=MAXIT)
        except Exception as e:          # reported below, from the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a thread did not return from its solve"
    assert not errors, errors
    for got, want in zip(results, expect):
        tr.assert_same_bits(got[0], want[0])
        assert [(i.iterations, i.reason, i.residual_sq) for i in got[1]] == \
               [(i.iterations, i.reason, i.residual_sq) for i in want[1]]


# ---- 7. fuzz ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(24))
def test_fuzz_against_the_per_column_reference(seed):
    """The seeded solver cases (structure, method, preconditioner none / exact / sweeps, dtype, format, poll interval,
    maxit) with a drawn k, leading dimensions and column tile."""
    pattern, values, b, x0, knobs = sc.case(seed)
    rng = np.random.default_rng(977 + seed)
    n, dtype = pattern[0], knobs["dtype"].type
    k = int(rng.choice([1, 2, 3, 4, 6, 9, 19]))
    ldb, ldx = k + int(rng.integers(0, 4)), k + int(rng.integers(0, 4))
    tile = int(rng.choice([0, 1, 2, 4, 8, 16, 32]))
    prec = "none" if knobs["dropped"] else knobs["prec"]      # a factor needs every diagonal
    a = make(knobs["kind"], pattern, values)
    f = None if prec == "none" else a.ilu0()
    sweeps = sc.PREC_SWEEPS.get(prec)
    if sweeps is not None:
        f.device().set_option("trsv_sweeps", sweeps)
    a.device().set_option("krylov_tile", tile)
    a.device().set_option("krylov_check_every", knobs["check_every"])
    B = block_of(b, k, seed)
    X0 = block_of(x0, k, 1000 + seed)
    if k > 1:
        B[:, k - 1] = 0                       # a column that stops at once, next to the ones that run
    maxit = knobs["maxit"]
    got = dev_call(a, f, knobs["method"], B, X0, ldb, ldx, knobs["tol"], maxit)
    refs = reference(knobs["method"], column_ops(a, f, sweeps=sweeps), B, X0, knobs["tol"], maxit)
    for j, ref in enumerate(refs):
        same_column(got[0][:, j], got[1][j], ref, f"seed {seed} column {j}")
