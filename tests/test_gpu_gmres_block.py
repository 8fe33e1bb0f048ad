"""Restarted GMRES on a block of right-hand sides (spal_*_gmres_block_*) against the sequential text, column
by column: raw bits of x, iterations, reason, residual_sq and rhs_sq, f64 and f32, CSR and CSC, with and without a factor.

The reference for column j is tests/gmres_ref.gmres on B[:, j] and X0[:, j], fed by the device's own operations on that
one column (column_ops of the block Krylov test: spmm on an (n, 1) block, solve_triangular / its sweeps on the factor)
or, on diagonal matrices, by one host rounding per element.  Nothing in the reference knows about the other columns, the
common cycles, the leading dimensions, the column tile, the batch of basis blocks or the poll interval.

The mixed block (a zero column, columns in the span of 1, 2, 3, 6 and 7 eigenvalue classes of a diagonal matrix, a column
with a NaN) was run on the CPU first: its columns end at different steps of different cycles, with all three reasons and
a lucky breakdown.  The tests take those facts from the reference run and assert them; nothing is skipped."""
import ctypes as C
import functools
import threading
import zlib

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import gmres_ref as gr
from tests import solver_cases as sc
from tests import trsv_ref as tr
from tests.test_gpu_gmres import MAXIT, TOL, case, make, setup
from tests.test_gpu_krylov_block import LONG_N, block_of, column_ops, same_block, same_column

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
DESCRIBE_KEYS = {"restart", "k", "preconditioned", "precond_sweeps", "tile", "iterations_min", "iterations_max", "cycles",
                 "steps", "converged", "check_every", "polls", "dot_batch", "basis_bytes", "solve_ms"}


def reference(ops, B, X0, restart, tol, maxit):
    return [gr.gmres(*ops, np.ascontiguousarray(B[:, j]), np.ascontiguousarray(X0[:, j]), restart, tol, maxit)
            for j in range(B.shape[1])]


def mode_ops(a, mode):
    """(M, precond_sweeps, (mul, prec) on one column) of a mode of the vector GMRES test"""
    m, sweeps, _ = setup(a, mode)
    return m, sweeps, column_ops(a, m, sweeps=sweeps)


def infos_of(got):
    return [(i.iterations, i.reason, i.residual_sq, i.rhs_sq) for i in got[1]]


def same_bits_and_infos(got, want):
    tr.assert_same_bits(got[0], want[0])
    a, b = np.array(infos_of(got)), np.array(infos_of(want))
    tr.assert_same_bits(a, b)


# ---- 1. the matrices of the vector solver's tests ----------------------------------------------------------------------

# (matrix, kind, mode, dtype, k, restart): k in {1, 2, 3, 5, 8, 17, 33, 70} and restart in {1, 2, 5, 30} spread over them
BLOCK_CASES = [
    ("full", "csr", "none", np.float64, 3, 30),
    ("full", "csc", "ilu0", np.float32, 2, 5),
    ("full", "csr", "ilu0-sweeps2", np.float32, 5, 2),
    ("full", "csc", "jacobi", np.float64, 2, 30),
    ("banded", "csr", "ilu0", np.float64, 5, 30),
    ("banded", "csc", "none", np.float32, 2, 30),
    ("banded", "csr", "jacobi", np.float32, 3, 5),
    ("banded", "csc", "ilu0-sweeps2", np.float64, 2, 1),
    ("bidiagonal", "csr", "ilu0", np.float64, 8, 30),
    ("bidiagonal", "csc", "none", np.float32, 1, 5),
    ("bidiagonal", "csr", "ilu0-sweeps2", np.float64, 3, 2),
    ("diagonal", "csr", "none", np.float64, 17, 30),
    ("diagonal", "csc", "ilu0", np.float32, 33, 1),
    ("diagonal", "csr", "jacobi", np.float32, 8, 2),
    ("one", "csr", "none", np.float64, 70, 30),
    ("one", "csc", "ilu0", np.float32, 70, 5),
]


@pytest.mark.parametrize("name,kind,mode,dtype,k,restart", BLOCK_CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[2]}-{np.dtype(c[3]).name}-k{c[4]}-m{c[5]}" for c in BLOCK_CASES])
def test_every_column_is_the_reference_loop(name, kind, mode, dtype, k, restart):
    pattern, values, b = case(name, dtype)
    tol = TOL[dtype]
    maxit = MAXIT if restart >= 5 else 12          # short restarts converge slowly: cut them, reason 1 is a result too
    a = make(kind, pattern, values)
    m, sweeps, ops = mode_ops(a, mode)
    B = block_of(b, k, zlib.crc32(f"gmres{name}{k}".encode()))
    got = a.gmres_block(B, M=m, restart=restart, tol=tol, maxit=maxit, precond_sweeps=sweeps)
    refs = reference(ops, B, np.zeros_like(B), restart, tol, maxit)
    same_block(got, refs)
    assert got[0].dtype == dtype and got[0].shape == B.shape
    if restart >= 5:
        assert all(i.reason == 0 for i in got[1])
    d = a.device().describe()["gmres_block"]
    assert set(d) == DESCRIBE_KEYS
    assert d["restart"] == restart and d["k"] == k and d["preconditioned"] == int(m is not None)
    assert d["precond_sweeps"] == (-1 if sweeps is None else sweeps) and d["tile"] == min(32, 1 << (k - 1).bit_length())
    its = [i.iterations for i in got[1]]
    assert (d["iterations_min"], d["iterations_max"]) == (min(its), max(its))
    assert d["converged"] == sum(i.reason == 0 for i in got[1])
    assert d["steps"] * k >= sum(its) and d["cycles"] >= -(-max(its) // restart)
    assert d["check_every"] == (8 if mode == "none" else 1) and d["polls"] >= 1 and d["solve_ms"] > 0
    nblk = restart + 1 + 2 + (2 if mode != "none" else 0)
    assert d["basis_bytes"] == nblk * (-(-pattern[0] * k // 64) * 64) * np.dtype(dtype).itemsize
    assert "gmres" not in a.device().describe() and "krylov_block" not in a.device().describe()


# ---- 2. a mixed block whose columns part ways ---------------------------------------------------------------------------

MIX_N = 1025
MIX_RUNS = [(4, 200), (4, 5), (1, 200), (2, 3), (30, 200)]      # (restart, maxit)
MIX_CLASSES = [1, 2, 3, 6, 7]


@functools.lru_cache(maxsize=None)
def mixed_case(dtype):
    """diag(1 + i % 7) and seven right-hand sides: zeros; 1 + 0.25 e on the rows of class e < c for c = 1, 2, 3, 6, 7
    (in the span of c eigenvalue classes: GMRES needs c steps, the last one a lucky breakdown when restart allows it); a
    column with one NaN."""
    cls = np.arange(MIX_N) % 7
    d = (1 + cls).astype(dtype)
    B = np.zeros((MIX_N, 7), dtype=dtype)
    for col, c in enumerate(MIX_CLASSES, start=1):
        B[:, col] = np.where(cls < c, 1 + 0.25 * cls, 0)
    B[:, 6] = np.linspace(-1, 1, MIX_N)
    B[300, 6] = np.nan
    X0 = np.zeros_like(B)
    X0[:, 6] = 0.5
    for arr in (d, B, X0):
        arr.setflags(write=False)
    return tr.diagonal(MIX_N), d, B, X0


@functools.lru_cache(maxsize=None)
def mixed_refs(dtype, restart, maxit):
    _, d, B, X0 = mixed_case(dtype)
    return reference((lambda v: d * v, None), B, X0, restart, TOL[dtype], maxit)      # one rounding per element, as on the device


def test_the_mixed_block_parts_ways_on_the_cpu():
    """what the reference says about the input, so that the device test below hits what it is meant to hit"""
    refs = mixed_refs(np.float64, 4, 200)
    its = [r[1]["iterations"] for r in refs]
    reasons = [r[1]["reason"] for r in refs]
    assert (its[0], reasons[0]) == (0, 0) and (its[6], reasons[6]) == (0, 2)
    assert its[1:4] == [1, 2, 3] and reasons[1:6] == [0] * 5          # three early ends of the first cycle ...
    assert its[4] > 4 and its[5] > 4 and its[4] != its[5]              # ... and two columns that need several cycles
    assert len({it % 4 for it in its[1:6]}) >= 3                       # different steps of their cycles
    for restart, maxit, at_least in ((4, 5, 2), (2, 3, 3)):
        r = mixed_refs(np.float64, restart, maxit)
        assert sum((c[1]["reason"], c[1]["iterations"]) == (1, maxit) for c in r) >= at_least
    assert {c[1]["reason"] for c in mixed_refs(np.float64, 2, 3)} == {0, 1, 2}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("restart,maxit", MIX_RUNS, ids=[f"m{r}-maxit{m}" for r, m in MIX_RUNS])
def test_columns_that_part_ways(restart, maxit, kind, dtype):
    pattern, d, B, X0 = mixed_case(dtype)
    a = make(kind, pattern, d)
    refs = mixed_refs(dtype, restart, maxit)
    its = [r[1]["iterations"] for r in refs]
    reasons = [r[1]["reason"] for r in refs]
    for every in (1, 8):
        a.device().set_option("krylov_check_every", every)
        got = a.gmres_block(B, X0=X0, restart=restart, tol=TOL[dtype], maxit=maxit)
        same_block(got, refs)                                # a column's x is what it was at ITS stop
    tr.assert_same_bits(got[0][:, 0], X0[:, 0])
    tr.assert_same_bits(got[0][:, 6], X0[:, 6])              # the NaN column never moved
    desc = a.device().describe()["gmres_block"]
    assert (desc["iterations_min"], desc["iterations_max"]) == (min(its), max(its))
    assert desc["converged"] == sum(r == 0 for r in reasons)
    assert desc["cycles"] >= max(-(-it // restart) for it in its) and desc["steps"] * 7 >= sum(its)
    # the NaN column left every other column alone: the same block with that column replaced
    B2, X2 = B.copy(), X0.copy()
    B2[:, 6], X2[:, 6] = B[:, 5], X0[:, 5]
    other = a.gmres_block(B2, X0=X2, restart=restart, tol=TOL[dtype], maxit=maxit)
    tr.assert_same_bits(other[0][:, :6], got[0][:, :6])
    tr.assert_same_bits(other[0][:, 6], got[0][:, 5])
    assert infos_of(other)[:6] == infos_of(got)[:6] and infos_of(other)[6] == infos_of(got)[5]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_zero_matrix_breaks_down_in_every_column(dtype):
    pattern, _, b = case("banded", dtype)
    a = make("csr", pattern, np.zeros(pattern[2].size, dtype=dtype))
    B = block_of(b, 3, 4)
    X0 = np.random.default_rng(6).uniform(-1, 1, size=B.shape).astype(dtype)
    X, infos = a.gmres_block(B, X0=X0, restart=30, tol=TOL[dtype], maxit=MAXIT)
    assert all((i.reason, i.iterations) == (2, 1) and not np.isfinite(i.residual_sq) for i in infos)
    tr.assert_same_bits(X, X0)
    same_block((X, infos), reference(column_ops(a, None), B, X0, 30, TOL[dtype], MAXIT))


# ---- 3. the bits do not depend on the geometry --------------------------------------------------------------------------

def dev_call(a, f, B, X0, ldb, ldx, restart, tol, maxit, stream=None):
    """The _dev form on torch tensors with padded rows: NaN in B's padding, a sentinel in X's.  Returns (X, infos)."""
    import torch
    n, k = B.shape
    tdt = torch.float64 if B.dtype == np.float64 else torch.float32
    Bw = torch.full((n, ldb), float("nan"), dtype=tdt, device="cuda")
    Xw = torch.full((n, ldx), -77.0, dtype=tdt, device="cuda")
    Bw[:, :k] = torch.tensor(B).cuda()
    Xw[:, :k] = torch.tensor(X0).cuda()
    torch.cuda.synchronize()
    infos = a.device().gmres_block_dev(k, Bw.data_ptr(), ldb, Xw.data_ptr(), ldx, None if f is None else f.device(),
                                       restart, tol, maxit, stream)
    torch.cuda.synchronize()
    Xh, Bh = Xw.cpu().numpy(), Bw.cpu().numpy()
    assert np.all(Xh[:, k:] == -77.0) and np.all(np.isnan(Bh[:, k:]))      # the padding survives
    tr.assert_same_bits(Bh[:, :k], B)
    return np.ascontiguousarray(Xh[:, :k]), infos


@pytest.mark.parametrize("k,mode", [(3, "ilu0"), (33, "none")], ids=["k3-ilu0", "k33-plain"])
def test_tile_poll_interval_and_leading_dimensions_change_nothing(k, mode):
    dtype = np.float64
    pattern, values, b = case("banded", dtype)
    a = make("csr", pattern, values)
    f, _, _ = setup(a, mode)
    restart, tol, maxit = 4, TOL[dtype], 10      # two full cycles and half of a third: the columns stop inside it or not at all
    B = block_of(b, k, 31)
    B[:, 1] = 0                                  # ... but one that stops at once
    B[:, 2] = B[:, 0] * 1e-3
    X0 = np.zeros_like(B)
    # ... and columns that start close to their solutions: measured, they stop at 5 and 4 (plain) and inside the first cycle (ilu0)
    for j, near in (((0, 1e-9), (2, 3e-10)) if mode == "none" else ((2, 1e-7),)):
        X0[:, j] = a.gmres(np.ascontiguousarray(B[:, j]), M=f, restart=30, tol=near, maxit=MAXIT)[0]
    singles = [a.gmres_block(np.ascontiguousarray(B[:, j:j + 1]), M=f, X0=np.ascontiguousarray(X0[:, j:j + 1]),
                             restart=restart, tol=tol, maxit=maxit) for j in range(k)]
    want = (np.concatenate([s[0] for s in singles], axis=1), [s[1][0] for s in singles])
    its = [i.iterations for i in want[1]]
    assert its[1] == 0 and len(set(its)) >= 3       # the columns stop at different points

    for tile in (1, 2, 4, 8, 16, 32):
        a.device().set_option("krylov_tile", tile)
        same_bits_and_infos(a.gmres_block(B, M=f, X0=X0, restart=restart, tol=tol, maxit=maxit), want)
        assert a.device().describe()["gmres_block"]["tile"] == tile
    a.device().set_option("krylov_tile", 0)
    for every in (1, 3, 8, 1000):
        a.device().set_option("krylov_check_every", every)
        same_bits_and_infos(a.gmres_block(B, M=f, X0=X0, restart=restart, tol=tol, maxit=maxit), want)
        d = a.device().describe()["gmres_block"]
        assert d["check_every"] == every and d["steps"] * k >= sum(its)
    for ldb, ldx, tile in ((k, k + 4, 0), (k + 5, k, 2), (k + 8, k + 2, 4)):
        a.device().set_option("krylov_tile", tile)
        same_bits_and_infos(dev_call(a, f, B, X0, ldb, ldx, restart, tol, maxit), want)
    with pytest.raises(sp.Panic, match="krylov_tile must be 0"):
        a.device().set_option("krylov_tile", 3)
    # what the other columns hold does not reach column 0
    a.device().set_option("krylov_tile", 0)
    rng = np.random.default_rng(9)
    B2 = np.ascontiguousarray(B[:, ::-1])
    B2[:, 1:] = rng.uniform(-100, 100, size=(B.shape[0], k - 1))
    B2[:, 0] = B[:, 0]
    B2[5, 1] = np.inf
    got = a.gmres_block(B2, M=f, X0=np.ascontiguousarray(X0[:, ::-1] * 0 + X0[:, :1]), restart=restart, tol=tol, maxit=maxit)
    tr.assert_same_bits(got[0][:, 0], want[0][:, 0])
    assert infos_of(got)[0] == infos_of(want)[0]


# ---- 4. the batches of the two kernels ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_batch_boundaries(dtype):
    """tol = 0 and maxit = restart: one full cycle, whose last step's orthogonalisation crosses every batch boundary"""
    pattern, values, b = case("full", dtype)
    a = make("csr", pattern, values)
    B = block_of(b, 3, 17)
    a.gmres_block(B, restart=1, maxit=1)
    batch = a.device().describe()["gmres_block"]["dot_batch"]
    assert 1 <= batch <= 64
    ops = column_ops(a, None)
    for restart in sorted({max(1, batch - 1), batch, batch + 1, 2 * batch + 1}):
        got = a.gmres_block(B, restart=restart, tol=0.0, maxit=restart)
        same_block(got, reference(ops, B, np.zeros_like(B), restart, 0.0, restart))
        d = a.device().describe()["gmres_block"]
        assert all((i.reason, i.iterations) == (1, restart) for i in got[1])
        assert (d["cycles"], d["steps"]) == (1, restart)


# ---- 5. sizes -------------------------------------------------------------------------------------------------------------

def diagonal_system(n, k, dtype, seed):
    rng = np.random.default_rng(seed)
    values = rng.uniform(0.5, 2, size=n).astype(dtype)
    return tr.diagonal(n), values, rng.uniform(-1, 1, size=(n, k)).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_tile_boundaries(n, dtype):
    pattern, values, B = diagonal_system(n, 3, dtype, n)
    a = make("csr", pattern, values)
    got = a.gmres_block(B, restart=3, tol=TOL[dtype], maxit=7)
    same_block(got, reference((lambda v: values * v, None), B, np.zeros_like(B), 3, TOL[dtype], 7))


@functools.lru_cache(maxsize=None)
def long_case(dtype):
    """bidiagonal, 1024 * 1024 + 1 rows: 1025 tiles, so workgroup 0 takes a second one and the sums need two upper levels"""
    n = LONG_N
    rng = np.random.default_rng(99)
    rowptr = np.concatenate([np.zeros(1, dtype=np.uint64), 1 + 2 * np.arange(n, dtype=np.uint64)])
    colind = np.repeat(np.arange(n, dtype=np.int64), 2).reshape(n, 2) + np.array([-1, 0])
    colind = colind.ravel()[1:].astype(np.uint64)
    diag = rng.uniform(1, 2, size=n).astype(dtype)
    sub = rng.uniform(-0.5, 0.5, size=n).astype(dtype)
    values = np.stack([sub, diag], axis=1).ravel()[1:].copy()
    B = rng.uniform(-1, 1, size=(n, 2)).astype(dtype)
    for arr in (rowptr, colind, values, B, diag, sub):
        arr.setflags(write=False)
    return (n, rowptr, colind), values, B, diag, sub


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_more_tiles_than_workgroups_and_two_upper_levels(dtype):
    pattern, values, B, diag, sub = long_case(dtype)
    assert -(-LONG_N // 1024) == 1024 + 1
    a = make("csr", pattern, values)

    def mul(v):      # ascending columns, the first product assigned, no FMA
        y = diag * v
        y[1:] = sub[1:] * v[:-1] + y[1:]
        return y

    tr.assert_same_bits(a.device().spmm(np.ascontiguousarray(B[:, :1]))[:, 0], mul(B[:, 0]))
    got = a.gmres_block(B, restart=2, tol=TOL[dtype], maxit=2)
    same_block(got, reference((mul, None), B, np.zeros_like(B), 2, TOL[dtype], 2))
    assert all((i.reason, i.iterations) == (1, 2) for i in got[1])


# ---- 6. the vector call ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["banded", "bidiagonal"])
def test_a_column_is_what_the_vector_call_returns(name, dtype):
    pattern, values, b = case(name, dtype)
    tol = TOL[dtype]
    a = make("csr", pattern, values)
    a.device().set_option("stream_row_max", 1024)      # every row through the stream kernel: sequential sums
    assert a.device().describe()["kernel"] == "stream"
    f = a.ilu0()
    B = block_of(b, 3, 8)
    for M in (None, f):
        X, infos = a.gmres_block(B, M=M, restart=6, tol=tol, maxit=MAXIT)
        for j in range(3):
            x, info = a.gmres(np.ascontiguousarray(B[:, j]), M=M, restart=6, tol=tol, maxit=MAXIT)
            tr.assert_same_bits(X[:, j], x)
            assert (infos[j].iterations, infos[j].reason) == (info.iterations, info.reason)
            assert (infos[j].residual_sq, infos[j].rhs_sq) == (info.residual_sq, info.rhs_sq)
    assert set(a.device().describe()["gmres"]) and set(a.device().describe()["gmres_block"]) == DESCRIBE_KEYS


# ---- 7. other behaviour ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_maxit_zero_and_a_start_that_is_not_zero(kind):
    pattern, values, b = case("banded", np.float64)
    a = make(kind, pattern, values)
    B = block_of(b, 3, 12)
    X0 = np.random.default_rng(5).uniform(-1, 1, size=B.shape)
    ops = column_ops(a, None)
    X, infos = a.gmres_block(B, X0=X0, restart=30, tol=1e-10, maxit=0)
    tr.assert_same_bits(X, X0)
    assert all((i.iterations, i.reason) == (0, 1) for i in infos)
    same_block((X, infos), reference(ops, B, X0, 30, 1e-10, 0))
    d = a.device().describe()["gmres_block"]
    assert (d["steps"], d["cycles"], d["polls"]) == (0, 0, 1)
    got = a.gmres_block(B, X0=X0, restart=7, tol=1e-10, maxit=MAXIT)
    same_block(got, reference(ops, B, X0, 7, 1e-10, MAXIT))
    assert all(i.reason == 0 for i in got[1])
    X, infos = a.gmres_block(B, X0=got[0], restart=7, tol=1e-8, maxit=MAXIT)
    assert all((i.iterations, i.reason) == (0, 0) for i in infos)
    tr.assert_same_bits(X, got[0])


@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_refusals(kind):
    import torch
    lib = _ffi.lib()
    pattern, values, b = case("full", np.float64)
    n = pattern[0]
    a = make(kind, pattern, values)
    dev = a.device()
    host = getattr(lib, f"spal_{kind}_gmres_block_f64")
    devf = getattr(lib, f"spal_{kind}_gmres_block_dev_f64")
    cinfo = (sp.matrix._KrylovInfoC * 2)()
    B = block_of(b, 2, 1)
    X = np.zeros_like(B)
    pb, px = B.ctypes.data_as(_ffi.f64p), X.ctypes.data_as(_ffi.f64p)
    u = C.c_uint64

    def call(h=dev._h, m=None, k=2, b_=pb, ldb=2, b_rows=n, x_=px, ldx=2, x_rows=n, restart=5, tol=1e-10, info=cinfo):
        return host(h, m, u(k), b_, u(ldb), u(b_rows), x_, u(ldx), u(x_rows), u(restart), C.c_double(tol), u(5), info)

    def refused(status, text, got):
        assert got == status, lib.spal_last_error()
        msg = lib.spal_last_error().decode()
        assert text in msg and msg.startswith(f"spal_{kind}_gmres_block:"), msg

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
    refused(inv, "restart = 0 must be 1 .. 256 (one Hessenberg column element per thread", call(restart=0))
    refused(inv, "restart = 257 must be 1 .. 256", call(restart=257))
    for bad in (-1e-3, float("nan")):
        refused(inv, "must be >= 0", call(tol=bad))
    f32 = make(kind, pattern, values.astype(np.float32)).device()
    refused(inv, "handle holds f32 values", call(h=f32._h))
    refused(inv, "element sizes 8 and 4", call(m=f32._h))
    cls = sp.CsrMatrix if kind == "csr" else sp.CscMatrix
    rect = cls(2, 3, [0, 1, 2] if kind == "csr" else [0, 1, 2, 2], [0, 1], np.array([1.0, 2.0])).device()
    refused(inv, "not square (2 x 3)", call(h=rect._h, b_rows=2, x_rows=2))
    small = make(kind, *case("diagonal", np.float64)[:2]).device()
    refused(inv, "the preconditioner is 1025 x 1025", call(m=small._h))
    nodiag_pattern = tr.drop_diagonal(pattern, 7)
    nodiag = make(kind, nodiag_pattern, np.ones(nodiag_pattern[2].size)).device()
    assert call(m=nodiag._h) == inv and "row 7 stores no diagonal entry" in lib.spal_last_error().decode()
    tr.assert_same_bits(X, np.zeros_like(B))                 # nothing was written
    bt = torch.tensor(B).cuda()
    xt = torch.zeros_like(bt)

    def dcall(x_, k=2, restart=5, stream=None):
        return devf(dev._h, None, u(k), C.c_void_p(bt.data_ptr()), u(2), C.c_void_p(x_.data_ptr()), u(2), u(restart),
                    C.c_double(1e-10), u(5), stream, cinfo)

    refused(inv, "x_dev == b_dev", dcall(bt))
    refused(inv, "k = 0", dcall(xt, k=0))
    refused(inv, "restart = 0 must be", dcall(xt, restart=0))
    refused(inv, "restart = 257 must be", dcall(xt, restart=257))
    # a capturing stream: refused, and the capture is the caller's to end
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            got = dcall(xt, stream=C.c_void_p(s.cuda_stream))
            msg = lib.spal_last_error().decode()
        finally:
            g.capture_end()
    assert got == inv and "cannot be captured into a graph" in msg
    assert not xt.cpu().numpy().any()
    # Python's own refusals
    with pytest.raises(sp.Panic, match=r"gmres_block: X0 has shape \(3, 2\)"):
        a.gmres_block(B, X0=np.zeros((3, 2)))
    with pytest.raises(sp.Panic, match=r"gmres_block: B has shape"):
        a.gmres_block(b)
    for bad in (0, 257):
        with pytest.raises(sp.Panic, match=rf"gmres_block: restart = {bad} must be 1 \.\. 256"):
            a.gmres_block(B, restart=bad)
    with pytest.raises(TypeError):
        a.gmres_block(B, M=make("csc" if kind == "csr" else "csr", pattern, values))
    # the handle works as before
    got = a.gmres_block(B, restart=5, tol=1e-10, maxit=MAXIT)
    same_block(got, reference(column_ops(a, None), B, np.zeros_like(B), 5, 1e-10, MAXIT))


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
        with pytest.raises(sp.SpalError, match="spal_csr_gmres_block: .*row blocks") as e:
            a.gmres_block(B, M=m, maxit=3)
        assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_dev_form_on_a_side_stream_with_strided_tensors(kind, dtype):
    import torch
    pattern, values, b = case("banded", dtype)
    a = make(kind, pattern, values)
    f = a.ilu0()
    B = block_of(b, 3, 21)
    tol = TOL[dtype]
    want = a.gmres_block(B, M=f, restart=3, tol=tol, maxit=MAXIT)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    got = dev_call(a, f, B, np.zeros_like(B), 7, 4, 3, tol, MAXIT, stream=s)
    same_bits_and_infos(got, want)
    f.device().set_option("trsv_sweeps", 2)      # the sweeps go through the side stream's scratch block, grown before the loop
    want = a.gmres_block(B, M=f, restart=3, tol=tol, maxit=7)
    same_block(want, reference(column_ops(a, f, sweeps=2), B, np.zeros_like(B), 3, tol, 7))
    got = dev_call(a, f, B, np.zeros_like(B), 7, 4, 3, tol, 7, stream=s)
    same_bits_and_infos(got, want)
    assert a.device().describe()["gmres_block"]["precond_sweeps"] == 2


@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_two_threads_solve_blocks_on_one_handle(kind):
    pattern, values, b = case("banded", np.float64)
    a = make(kind, pattern, values)
    f = a.ilu0()
    Bs = [block_of(b, 3, 1), block_of(b, 5, 2)]
    expect = [a.gmres_block(B, M=f, restart=4, tol=1e-10, maxit=MAXIT) for B in Bs]
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i):
        try:
            gate.wait(timeout=30)
            results[i] = a.gmres_block(Bs[i], M=f, restart=4, tol=1e-10, maxit=MAXIT)
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
        same_bits_and_infos(got, want)


# ---- 8. fuzz ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(24))
def test_fuzz_against_the_per_column_reference(seed):
    """The seeded solver cases (structure, preconditioner none / exact / sweeps, dtype, format, poll interval, maxit) with
    a drawn k <= 9, restart <= 6, leading dimensions and column tile."""
    pattern, values, b, x0, knobs = sc.case(seed)
    rng = np.random.default_rng(1977 + seed)
    k = int(rng.choice([1, 2, 3, 4, 6, 9]))
    restart = int(rng.integers(1, 7))
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
    maxit = min(knobs["maxit"], 20)
    got = dev_call(a, f, B, X0, ldb, ldx, restart, knobs["tol"], maxit)
    refs = reference(column_ops(a, f, sweeps=sweeps), B, X0, restart, knobs["tol"], maxit)
    for j, ref in enumerate(refs):
        same_column(got[0][:, j], got[1][j], ref, f"seed {seed} column {j}")
