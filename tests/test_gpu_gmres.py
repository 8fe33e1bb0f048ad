"""Restarted GMRES on the device against its sequential text (tests/gmres_ref.py): raw bits equal, f64 and f32, CSR and
CSC, without a preconditioner, with an ILU(0) factor applied by exact solves or by sweeps, and with the Jacobi
preconditioner, whatever the poll interval is.

As in tests/test_gpu_krylov.py the reference runs with the device's own spmv / solve_triangular as callables (those are
deterministic, so the comparison is bit for bit whichever SpMV kernel the plan picks) and, on two structures whose rows
all go through the stream kernel, with pure host operations."""
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
from tests import krylov_ref as kr
from tests import trsv_ref as tr

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
TOL = {np.float64: 1e-10, np.float32: 1e-5}
MAXIT = 200
G = 4096 * 1024      # the elements one trip of the first-level grid covers
PATTERNS = [("full", 4000), ("banded", 6007), ("bidiagonal", 5000), ("diagonal", 1025), ("one", 1)]
MODES = ["none", "ilu0", "ilu0-sweeps2", "jacobi"]      # M: none, a.ilu0(), a.ilu0() by 2 sweeps, a itself by 0 sweeps
DESCRIBE_KEYS = {"restart", "preconditioned", "precond_sweeps", "iterations", "cycles", "reason", "check_every", "polls",
                 "dot_batch", "basis_bytes", "solve_ms"}


def _pattern(name):
    rng = np.random.default_rng(20261018)
    if name == "banded":
        return ir.sym(tr.banded(6007, 6, 512, rng))          # chains; n no multiple of 1024
    if name == "full":
        return ir.full(4000, 6, rng)                         # not symmetric
    if name == "bidiagonal":
        return ir.sym(tr.bidiagonal(5000))
    if name == "diagonal":
        return tr.diagonal(1025)
    if name == "one":
        return tr.diagonal(1)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """(pattern, values, b) with trsv_ref.fill's values: diagonally dominant, not symmetric.  Shared, read-only."""
    pattern = _pattern(name)
    assert pattern[0] == dict(PATTERNS)[name]
    values, b = tr.fill(pattern, dtype, np.random.default_rng(zlib.crc32(("gmres/" + name).encode())))
    for a in (*pattern[1:], values, b):
        a.setflags(write=False)
    return pattern, values, b


def make(kind, pattern, values):
    n, rowptr, colind = pattern
    if kind == "csr":
        return sp.CsrMatrix(n, n, rowptr, colind, values)
    colptr, rowind, vals, _ = ir.to_csc(pattern, values)
    return sp.CscMatrix(n, n, colptr, rowind, vals)


def setup(a, mode):
    """(M, precond_sweeps, the reference's prec) of a mode; the reference applies M by the device's own operations."""
    if mode == "none":
        return None, None, None
    if mode == "jacobi":
        return a, 0, lambda v: a.solve_triangular(a.solve_triangular(v, True, True, sweeps=0), False, False, sweeps=0)
    f = a.ilu0()
    if mode == "ilu0":
        return f, None, lambda v: f.solve_triangular(f.solve_triangular(v, True, True), False)
    return f, 2, lambda v: f.solve_triangular(f.solve_triangular(v, True, True, sweeps=2), False, False, sweeps=2)


def same_result(got, ref):
    x, info = got
    xr, ir_ = ref
    tr.assert_same_bits(x, xr)
    assert (info.iterations, info.reason) == (ir_["iterations"], ir_["reason"])
    tr.assert_same_bits(np.array([info.residual_sq]), np.array([ir_["residual_sq"]]))
    tr.assert_same_bits(np.array([info.rhs_sq]), np.array([ir_["rhs_sq"]]))


def check(a, mode, b, restart, tol, maxit, x0=None):
    """One call against the text on the device's own operations; returns (x, info)."""
    m, sweeps, prec = setup(a, mode)
    got = a.gmres(b, M=m, x0=x0, restart=restart, tol=tol, maxit=maxit, precond_sweeps=sweeps)
    start = np.zeros_like(b) if x0 is None else x0
    ref = gr.gmres(lambda v: a.device().spmv(v), prec, b, start, restart, tol, maxit)
    same_result(got, ref)
    d = a.device().describe()["gmres"]
    assert d["restart"] == restart and d["preconditioned"] == int(m is not None) and d["iterations"] == got[1].iterations
    assert d["precond_sweeps"] == (-1 if sweeps is None else sweeps) and d["reason"] == got[1].reason
    return got


# ---- 1. bits against the text on the device's own operations -----------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("name", [p[0] for p in PATTERNS])
def test_gmres_is_the_text(name, kind, mode, dtype):
    pattern, values, b = case(name, dtype)
    a = make(kind, pattern, values)
    x, info = check(a, mode, b, 30, TOL[dtype], MAXIT)
    assert info.reason == 0 and x.dtype == dtype
    assert kr.true_relative_residual(pattern, values, x, b) <= 2 * TOL[dtype]
    if name in ("diagonal", "one") or (name == "bidiagonal" and mode == "ilu0"):
        assert info.iterations == 1            # M = A exactly, or A v_0 is a multiple of v_0 ...
    d = a.device().describe()["gmres"]
    assert set(d) == DESCRIBE_KEYS
    assert d["check_every"] == (8 if mode == "none" else 1) and d["polls"] >= 1 and d["solve_ms"] > 0 and d["cycles"] >= 1
    nvec = 31 + 2 + (2 if mode != "none" else 0) + (2 if mode in ("ilu0-sweeps2", "jacobi") else 0)
    assert d["basis_bytes"] == nvec * (-(-pattern[0] // 64) * 64) * np.dtype(dtype).itemsize
    assert "krylov" not in a.device().describe()     # left to CG and BiCGStab


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("mode", ["none", "ilu0-sweeps2"])
@pytest.mark.parametrize("restart", [1, 3])
@pytest.mark.parametrize("name", ["full", "banded"])
def test_short_restarts(name, restart, mode, dtype):
    pattern, values, b = case(name, dtype)
    a = make("csr", pattern, values)
    x, info = check(a, mode, b, restart, TOL[dtype], MAXIT)
    assert info.reason == 0 and a.device().describe()["gmres"]["cycles"] >= -(-info.iterations // restart)


# ---- 2. against pure host operations ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("prec", [False, True], ids=["plain", "ilu0"])
@pytest.mark.parametrize("name", ["banded", "bidiagonal"])
def test_gmres_against_pure_host_operations(oracle, name, prec, dtype):
    pattern, values, b = case(name, dtype)
    n, rowptr, colind = pattern
    tol = TOL[dtype]
    mul = lambda v: oracle.csr_spmv(rowptr, colind, values, v)                               # noqa: E731
    hp = None
    if prec:
        fv = ir.ilu0_rows(n, rowptr, colind, values)
        hp = lambda v: tr.solve_by_levels(n, rowptr, colind, fv,                            # noqa: E731
                                          tr.solve_by_levels(n, rowptr, colind, fv, v, True, True), False, False)
    ref = gr.gmres(mul, hp, b, np.zeros_like(b), 30, tol, MAXIT)
    a = make("csr", pattern, values)
    # every row through the stream kernel, whose sums are the sequential ones (tests/test_gpu_krylov.py explains)
    a.device().set_option("stream_row_max", 1024)
    d = a.device().describe()
    assert d["kernel"] == "stream" and d["overflow_tiles"] == 0 and d["stream_row_fraction"] == 1.0
    same_result(a.gmres(b, M=a.ilu0() if prec else None, restart=30, tol=tol, maxit=MAXIT), ref)
    assert ref[1]["reason"] == 0


# ---- 3. the batches of the two kernels ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_batch_boundaries(dtype):
    """j + 1 passes B - 1, B, B + 1 and 2 B + 1 within ONE cycle"""
    pattern, values, b = case("full", dtype)
    a = make("csr", pattern, values)
    a.gmres(b, restart=1, maxit=1)
    batch = a.device().describe()["gmres"]["dot_batch"]
    assert 1 <= batch <= 64
    m = 2 * batch + 2
    x, info = check(a, "none", b, m, 0.0, m)
    assert (info.reason, info.iterations) == (1, m) and a.device().describe()["gmres"]["cycles"] == 1


# ---- 4. past one trip of the grid, three levels of reduce() ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_case(dtype):
    n = G + 1
    cols = (np.repeat(np.arange(n, dtype=np.int64), 3).reshape(n, 3) + np.array([-1, 0, 1])).ravel()[1:-1]
    rowptr = np.concatenate([[0, 2], 2 + 3 * np.arange(1, n - 1, dtype=np.int64), [3 * n - 2]]).astype(np.uint64)
    pattern = (n, rowptr, cols.astype(np.uint64))
    values, b = tr.fill(pattern, dtype, np.random.default_rng(zlib.crc32(b"gmres/long")))
    for a in (*pattern[1:], values, b):
        a.setflags(write=False)
    return pattern, values, b


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_past_one_trip_of_the_grid(dtype):
    """every first-level launch takes a second tile in workgroup 0, and 4097 tile sums need a third level; a full cycle, a
    restart and one more step"""
    pattern, values, b = long_case(dtype)
    assert -(-pattern[0] // 1024) == 4096 + 1
    a = make("csr", pattern, values)
    x, info = check(a, "none", b, 2, TOL[dtype], 3)
    assert (info.reason, info.iterations) == (1, 3) and a.device().describe()["gmres"]["cycles"] == 2


# ---- 5. the poll interval -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["none", "ilu0-sweeps2"])
def test_check_every_changes_nothing(mode):
    pattern, values, b = case("banded", np.float64)
    a = make("csr", pattern, values)
    first = check(a, mode, b, 5, 1e-10, MAXIT)
    assert first[1].reason == 0 and first[1].iterations > 5          # (on the CPU: 49 and 8 iterations, so the stop falls
    #                                                                   inside a cycle ...
    m, sweeps, _ = setup(a, mode)
    polls = {}
    for every in (1, 2, 3, 8, 64):                                    # ... and, for 2, 3, 8 and 64, inside a batch)
        a.device().set_option("krylov_check_every", every)
        x, info = a.gmres(b, M=m, restart=5, tol=1e-10, maxit=MAXIT, precond_sweeps=sweeps)
        tr.assert_same_bits(x, first[0])
        assert (info.iterations, info.reason, info.residual_sq) == (first[1].iterations, 0, first[1].residual_sq)
        d = a.device().describe()["gmres"]
        assert d["check_every"] == every
        polls[every] = d["polls"]
    assert polls[1] > polls[2] > polls[8] and polls[8] == polls[64]   # the host polls at the end of every cycle at the latest
    # maxit in the middle of a batch and of a cycle
    a.device().set_option("krylov_check_every", 3)
    x, info = a.gmres(b, M=m, restart=5, tol=1e-10, maxit=7, precond_sweeps=sweeps)
    ref = check(a, mode, b, 5, 1e-10, 7)
    assert (info.iterations, info.reason) == (7, 1)
    tr.assert_same_bits(x, ref[0])


# ---- 6. edges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_maxit_zero_and_exact_x0(kind):
    pattern, values, b = case("banded", np.float64)
    a = make(kind, pattern, values)
    x0 = np.random.default_rng(5).uniform(-1, 1, size=b.size)
    x, info = check(a, "none", b, 30, 1e-10, 0, x0=x0)
    assert (info.reason, info.iterations) == (1, 0)
    tr.assert_same_bits(x, x0)
    r0 = b - a.device().spmv(x0)
    assert info.residual_sq == float(kr.dot(r0, r0)) and info.rhs_sq == float(kr.dot(b, b))
    exact = a.gmres(b, restart=30, tol=1e-10, maxit=MAXIT)[0]
    x, info = check(a, "none", b, 30, 1e-8, MAXIT, x0=exact)
    assert (info.reason, info.iterations) == (0, 0)
    tr.assert_same_bits(x, exact)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_zero_matrix_and_nan(dtype):
    pattern, values, b = case("banded", dtype)
    a = make("csr", pattern, np.zeros(pattern[2].size, dtype=dtype))
    x0 = np.random.default_rng(6).uniform(-1, 1, size=b.size).astype(dtype)
    x, info = check(a, "none", b, 30, TOL[dtype], MAXIT, x0=x0)         # SPAL_OK: a breakdown is no error
    assert (info.reason, info.iterations) == (2, 1) and not np.isfinite(info.residual_sq)
    tr.assert_same_bits(x, x0)
    bad = b.copy()
    bad[4097] = np.nan
    a = make("csr", pattern, values)
    x, info = check(a, "none", bad, 30, TOL[dtype], MAXIT, x0=x0)
    assert (info.reason, info.iterations) == (2, 0)
    tr.assert_same_bits(x, x0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_cyclic_shift(kind, dtype):
    """BiCGStab breaks down; GMRES(8) and GMRES(30) take 8 steps and are exact -- the NaN v_8 of the lucky breakdown is
    written and never read; GMRES(4) stagnates"""
    n = 8
    rows = np.arange(n, dtype=np.int64)
    pattern = tr.from_coo(n, rows, (rows - 1) % n)
    a = make(kind, pattern, np.ones(n, dtype=dtype))
    mul, b, exact = gr.cyclic_shift(n, dtype)
    tr.assert_same_bits(a.device().spmv(np.arange(n, dtype=dtype)), mul(np.arange(n, dtype=dtype)))
    assert a.solve(b, "bicgstab", tol=1e-6, maxit=MAXIT)[1].reason == 2
    for restart in (8, 30):
        x, info = check(a, "none", b, restart, 1e-6, MAXIT)
        assert (info.reason, info.iterations, info.residual_sq) == (0, 8, 0.0)
        tr.assert_same_bits(x, exact)
    x, info = check(a, "none", b, 4, 1e-6, 40)
    assert (info.reason, info.iterations) == (1, 40) and np.all(np.isfinite(x))
    same_result((x, info), gr.gmres(mul, None, b, np.zeros_like(b), 4, 1e-6, 40))


# ---- 7. two threads, one handle; the device-pointer form ---------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_two_threads_solve_on_one_handle(kind):
    pattern, values, b = case("banded", np.float64)
    a = make(kind, pattern, values)
    f = a.ilu0()
    bs = [b, np.random.default_rng(77).uniform(-1, 1, size=b.size)]
    expect = [a.gmres(v, M=f, restart=4, tol=1e-10, maxit=MAXIT) for v in bs]
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i):
        try:
            gate.wait(timeout=30)
            results[i] = a.gmres(bs[i], M=f, restart=4, tol=1e-10, maxit=MAXIT)
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
        assert (got[1].iterations, got[1].reason, got[1].residual_sq) == (want[1].iterations, 0, want[1].residual_sq)


def test_device_pointer_form_on_a_stream():
    import torch
    pattern, values, b = case("banded", np.float32)
    a = make("csr", pattern, values)
    f = a.ilu0()
    want = a.gmres(b, M=f, restart=3, tol=1e-5, maxit=MAXIT)
    bt = torch.tensor(b).cuda()
    xt = torch.zeros_like(bt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    info = a.device().gmres_dev(bt.data_ptr(), xt.data_ptr(), M=f.device(), restart=3, tol=1e-5, maxit=MAXIT, stream=s)
    tr.assert_same_bits(xt.cpu().numpy(), want[0])               # the call has synchronised its stream
    assert (info.iterations, info.reason, info.residual_sq) == (want[1].iterations, 0, want[1].residual_sq)
    tr.assert_same_bits(bt.cpu().numpy(), b)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_refusals(kind):
    import torch
    lib = _ffi.lib()
    pattern, values, b = case("full", np.float64)
    n = pattern[0]
    a = make(kind, pattern, values)
    dev = a.device()
    f = a.ilu0().device()
    x0, info = dev.gmres(b, M=f, restart=5, tol=1e-10, maxit=MAXIT)
    host = getattr(lib, f"spal_{kind}_gmres_f64")
    devf = getattr(lib, f"spal_{kind}_gmres_dev_f64")
    cinfo = sp.matrix._KrylovInfoC()
    x = np.zeros(n)
    pb, px = b.ctypes.data_as(_ffi.f64p), x.ctypes.data_as(_ffi.f64p)
    u = C.c_uint64

    def refused(status, text, call):
        assert call() == status, lib.spal_last_error()
        assert text in lib.spal_last_error().decode(), lib.spal_last_error()

    def call(a_=dev._h, m_=None, b_=pb, nb=n, x_=px, nx=n, restart=5, tol=1e-10, info_=C.byref(cinfo), fn=host):
        return lambda: fn(a_, m_, b_, u(nb), x_, u(nx), u(restart), C.c_double(tol), u(5), info_)

    inv, fn = _ffi.SPAL_ERR_INVALID_ARGUMENT, f"spal_{kind}_gmres"
    refused(inv, fn + ": null argument", call(a_=None))
    refused(inv, "null argument", call(b_=None))
    refused(inv, "null argument", call(x_=None))
    refused(inv, "null argument", call(info_=None))
    refused(inv, f"b.len() = {n - 1}", call(nb=n - 1))
    refused(inv, f"x.len() = {n + 1}", call(nx=n + 1))
    refused(inv, "restart = 0 must be 1 .. 256 (one Hessenberg column element per thread", call(restart=0))
    refused(inv, "restart = 257 must be 1 .. 256", call(restart=257))
    for bad in (-1e-3, float("nan")):
        refused(inv, "must be >= 0", call(tol=bad))
    x32 = x.astype(np.float32).ctypes.data_as(_ffi.f32p)
    refused(inv, "handle holds f64 values", call(b_=x32, x_=x32, fn=getattr(lib, f"spal_{kind}_gmres_f32")))
    cls = sp.CsrMatrix if kind == "csr" else sp.CscMatrix
    rect = cls(2, 3, [0, 1, 2] if kind == "csr" else [0, 1, 2, 2], [0, 1], np.array([1.0, 2.0])).device()
    refused(inv, "not square (2 x 3)", call(a_=rect._h, nb=2, nx=2))
    small = make(kind, *case("diagonal", np.float64)[:2]).device()
    refused(inv, "the preconditioner is 1025 x 1025", call(m_=small._h))
    f32 = make(kind, pattern, values.astype(np.float32)).device()
    refused(inv, "element sizes 8 and 4", call(m_=f32._h))
    nodiag_pattern = tr.drop_diagonal(pattern, 7)
    nodiag = make(kind, nodiag_pattern, np.ones(nodiag_pattern[2].size)).device()
    refused(inv, "row 7 stores no diagonal entry", call(m_=nodiag._h))
    bt = torch.tensor(b).cuda()
    xt = torch.zeros_like(bt)

    def dcall(b_, x_, restart=5, stream=None):
        return lambda: devf(dev._h, None, b_, x_, u(restart), C.c_double(1e-10), u(5), stream, C.byref(cinfo))

    refused(inv, "x_dev == b_dev", dcall(C.c_void_p(bt.data_ptr()), C.c_void_p(bt.data_ptr())))
    refused(inv, fn + "_dev: null argument", dcall(C.c_void_p(bt.data_ptr()), None))
    refused(inv, "restart = 1000 must be 1 .. 256", dcall(C.c_void_p(bt.data_ptr()), C.c_void_p(xt.data_ptr()), restart=1000))
    # a capturing stream
    xt.fill_(0.0)                                # (the fill kernel is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()               # never replayed
    seen = None
    with torch.cuda.graph(graph):
        xt.fill_(0.0)                            # (so that the graph is not empty)
        capturing = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        status = dcall(C.c_void_p(bt.data_ptr()), C.c_void_p(xt.data_ptr()), stream=capturing)()
        seen = (status, lib.spal_last_error().decode())
    torch.cuda.synchronize()
    assert seen[0] == inv and "cannot be captured into a graph" in seen[1], seen
    del graph
    with pytest.raises(sp.Panic, match="must be 'cg' or 'bicgstab'"):
        a.solve(b, "gmres")
    with pytest.raises(TypeError):
        a.gmres(b, M=make("csc" if kind == "csr" else "csr", pattern, values))
    # the handles work as before
    sp.cache_trim()
    x1, info1 = dev.gmres(b, M=f, restart=5, tol=1e-10, maxit=MAXIT)
    tr.assert_same_bits(x1, x0)
    assert info1.iterations == info.iterations


def test_row_block_handles_are_refused(monkeypatch):
    """a handle held as row blocks (the limit lowered for the test) has no solver, as A or as M: SPAL_ERR_UNSUPPORTED"""
    import spal_synth as synth
    rp, ci, va = synth.banded_csr(2000, 2000, 4, 64, 3)
    monkeypatch.setenv("SPAL_CSR_PART_ENTRIES", "3000")
    big = sp.CsrMatrix(2000, 2000, rp, ci, va)
    assert big.device().describe()["kernel"] == "row_blocks"
    monkeypatch.delenv("SPAL_CSR_PART_ENTRIES")
    small = sp.CsrMatrix(2000, 2000, rp, ci, va)
    b = np.ones(2000)
    for a, m in ((big, None), (small, big)):
        with pytest.raises(sp.SpalError, match="row blocks") as e:
            a.gmres(b, M=m, maxit=3)
        assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED
