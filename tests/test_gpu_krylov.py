"""The dot product, CG and BiCGStab on the device against their sequential text (tests/krylov_ref.py): raw bits equal,
f64 and f32, CSR and CSC, with and without an ILU(0) factor, whatever the poll interval is.

The reference loops run with the device's own spmv / solve_triangular as callables (those are deterministic, so the
comparison is bit for bit whichever SpMV kernel the plan picks) and, on two structures whose rows all go through the
stream kernel (which sums a row left to right), with pure host operations (oracle.csr_spmv, trsv_ref.solve_by_levels), which keeps the first comparison from
being only self-consistent.  Inputs were checked on the CPU with the reference first: every solving case reaches reason 0
inside maxit = 200 with a true relative residual below tol."""
import ctypes as C
import functools
import os
import subprocess
import sys
import threading
import zlib

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import ilu_ref as ir
from tests import krylov_ref as kr
from tests import trsv_ref as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float64, np.float32]
TOL = {np.float64: 1e-10, np.float32: 1e-5}
MAXIT = 200
G = 4096 * 1024      # the elements one trip of the first-level grid covers: 4096 workgroups (kMaxGrid), a tile of 1024 each
# G: the last size of one trip; G + 1: workgroup 0 alone takes a second tile; 3 G - 1023: three tiles each, the last one
# of a single element, and a second level of 12 tiles
SIZES = [0, 1, 2, 1023, 1024, 1025, 1024 ** 2 - 1, 1024 ** 2, 1024 ** 2 + 1, G, G + 1, 3 * G - 1023]


# ---- 1. the dot product ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_dot_dev_is_the_definition(n, dtype):
    import torch
    from tests.test_krylov_host import mixed
    a, b = mixed(n, dtype, 2 * n + 1), mixed(n, dtype, 2 * n + 2)
    ref = kr.dot(a, b)
    at, bt = torch.tensor(a).cuda(), torch.tensor(b).cuda()
    out = torch.full((1,), float("nan"), dtype=at.dtype, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    sp.dot_dev(dtype, at.data_ptr(), bt.data_ptr(), n, out.data_ptr(), 0, s)
    s.synchronize()
    tr.assert_same_bits(out.cpu().numpy(), np.array([ref]))
    if n >= 1024:
        with np.errstate(all="ignore"):
            assert kr.sequential_sum(a * b).tobytes() != ref.tobytes()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_dot_dev_zeros_and_nan(dtype):
    import torch

    def run(a, b):
        at, bt = torch.tensor(a).cuda(), torch.tensor(b).cuda()
        out = torch.full((1,), 7.0, dtype=at.dtype, device="cuda")
        torch.cuda.synchronize()
        sp.dot_dev(dtype, at.data_ptr(), bt.data_ptr(), a.size, out.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy()[0]

    z = run(np.array([-0.0], dtype=dtype), np.ones(1, dtype=dtype))
    assert z == 0 and not np.signbit(z)
    a = np.ones(3000, dtype=dtype)
    a[2049] = np.nan
    assert np.isnan(run(a, np.ones(3000, dtype=dtype)))


# ---- matrices -------------------------------------------------------------------------------------------------------

def _pattern(name):
    rng = np.random.default_rng(20261018)
    if name == "banded":
        return ir.sym(tr.banded(6007, 6, 512, rng))          # chains; n no multiple of 1024
    if name == "full":
        return ir.full(4000, 6, rng)                         # not symmetric: BiCGStab only
    if name == "bidiagonal":
        return ir.sym(tr.bidiagonal(5000))
    if name == "diagonal":
        return tr.diagonal(1025)
    if name == "one":
        return tr.diagonal(1)
    raise KeyError(name)


CASES = [("banded", "cg"), ("banded", "bicgstab"), ("full", "bicgstab"), ("bidiagonal", "cg"), ("bidiagonal", "bicgstab"),
         ("diagonal", "cg"), ("diagonal", "bicgstab"), ("one", "cg"), ("one", "bicgstab")]


@functools.lru_cache(maxsize=None)
def case(name, method, dtype):
    """(pattern, values, b): CG gets symmetric positive definite values, BiCGStab trsv_ref.fill's.  Shared, read-only."""
    pattern = _pattern(name)
    rng = np.random.default_rng(zlib.crc32((name + method).encode()))
    values, b = kr.spd_fill(pattern, dtype, rng) if method == "cg" else tr.fill(pattern, dtype, rng)
    for a in (*pattern[1:], values, b):
        a.setflags(write=False)
    return pattern, values, b


def make(kind, pattern, values):
    n, rowptr, colind = pattern
    if kind == "csr":
        return sp.CsrMatrix(n, n, rowptr, colind, values)
    colptr, rowind, vals, _ = ir.to_csc(pattern, values)
    return sp.CscMatrix(n, n, colptr, rowind, vals)


def device_ops(a, f):
    """The device's own product and preconditioner as callables for the reference loops."""
    mul = lambda v: a.device().spmv(v)                                                      # noqa: E731
    prec = None if f is None else (lambda v: f.solve_triangular(f.solve_triangular(v, True, True), False))
    return mul, prec


def same_result(got, ref):
    x, info = got
    xr, ir_ = ref
    tr.assert_same_bits(x, xr)
    assert info.iterations == ir_["iterations"] and info.reason == ir_["reason"]
    tr.assert_same_bits(np.array([info.residual_sq]), np.array([ir_["residual_sq"]]))
    assert info.rhs_sq == ir_["rhs_sq"]


# ---- 2. both methods against the device-operation reference ------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("prec", [False, True], ids=["plain", "ilu0"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("name,method", CASES)
def test_solve_is_the_reference_loop(name, method, kind, prec, dtype):
    pattern, values, b = case(name, method, dtype)
    tol = TOL[dtype]
    a = make(kind, pattern, values)
    f = a.ilu0() if prec else None
    x, info = a.solve(b, method, M=f, tol=tol, maxit=MAXIT)
    ref = kr.METHODS[method](*device_ops(a, f), b, np.zeros_like(b), tol, MAXIT)
    same_result((x, info), ref)
    assert info.reason == 0 and x.dtype == dtype
    if prec and name in ("bidiagonal", "diagonal", "one"):
        assert info.iterations == 1          # M = A exactly: BiCGStab leaves by the half-step exit
    assert info.residual_sq <= float(dtype(dtype(tol * tol) * dtype(info.rhs_sq)))
    # the factor 2 covers the drift between the recurrence and the true residual only: the bits are already equal
    assert kr.true_relative_residual(pattern, values, x, b) <= 2 * tol
    d = a.device().describe()["krylov"]
    assert d["method"] == method and d["preconditioned"] == int(prec) and d["iterations"] == info.iterations
    assert d["reason"] == 0 and d["check_every"] == (1 if prec else 8) and d["polls"] >= 1 and d["solve_ms"] > 0


# ---- 2b. the fused updates past one trip of the grid ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_case(name, dtype):
    """(pattern, values, b) of G + 1 rows, so that every first-level launch takes a second tile in workgroup 0:
    "tridiagonal" is symmetric positive definite (krylov_ref.spd_fill), "diagonal" holds d in [0.5, 2).  Shared, read-only."""
    n = G + 1
    rng = np.random.default_rng(zlib.crc32(f"long/{name}".encode()))
    if name == "tridiagonal":
        cols = (np.repeat(np.arange(n, dtype=np.int64), 3).reshape(n, 3) + np.array([-1, 0, 1])).ravel()[1:-1]
        rowptr = np.concatenate([[0, 2], 2 + 3 * np.arange(1, n - 1, dtype=np.int64), [3 * n - 2]]).astype(np.uint64)
        pattern = (n, rowptr, cols.astype(np.uint64))
        values, b = kr.spd_fill(pattern, dtype, rng)
    else:
        pattern = tr.diagonal(n)
        values = rng.uniform(0.5, 2, size=n).astype(dtype)
        b = rng.uniform(-1, 1, size=n).astype(dtype)
    for a in (*pattern[1:], values, b):
        a.setflags(write=False)
    return pattern, values, b


# (matrix, method, with M = a.ilu0(), maxit).  Between them the cases launch every VecOp with more tiles than workgroups:
# V_INIT, V_COPY_DOT, V_DOT, V_CG_XR, V_CG_P by CG; V_BI_P, V_BI_S, V_DOT2, V_BI_XR by BiCGStab; V_BI_HALF where the
# preconditioner is the matrix itself and BiCGStab leaves by the half step.
LONG_CASES = [("tridiagonal", "cg", False, 3), ("tridiagonal", "bicgstab", False, 2), ("diagonal", "bicgstab", True, MAXIT),
              ("diagonal", "cg", True, MAXIT)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name,method,prec,maxit", LONG_CASES, ids=["cg", "bicgstab", "bicgstab-half-step", "cg-ilu0"])
def test_fused_updates_past_one_trip_of_the_grid(name, method, prec, maxit, dtype):
    pattern, values, b = long_case(name, dtype)
    assert -(-pattern[0] // 1024) == 4096 + 1
    tol = TOL[dtype]
    a = make("csr", pattern, values)
    f = hp = None
    if prec:
        f = a.ilu0()
        tr.assert_same_bits(f.values(), values)      # the factor of a diagonal matrix is the matrix
        # ... so the two solves of the host preconditioner are: nothing (the unit lower triangle), then one division
        hp = lambda v: v / values                                                            # noqa: E731
    ref = kr.METHODS[method](lambda v: a.device().spmv(v), hp, b, np.zeros_like(b), tol, maxit)
    got = a.solve(b, method, M=f, tol=tol, maxit=maxit)
    same_result(got, ref)
    if prec and method == "bicgstab":
        assert (got[1].reason, got[1].iterations) == (0, 1)     # the half-step exit: V_BI_HALF has applied x += alpha ph
    if not prec:
        assert (got[1].reason, got[1].iterations) == (1, maxit)


# ---- 3. the pure-host reference --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("prec", [False, True], ids=["plain", "ilu0"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
@pytest.mark.parametrize("name", ["banded", "bidiagonal"])
def test_solve_against_pure_host_operations(oracle, name, method, prec, dtype):
    pattern, values, b = case(name, method, dtype)
    n, rowptr, colind = pattern
    tol = TOL[dtype]
    mul = lambda v: oracle.csr_spmv(rowptr, colind, values, v)                               # noqa: E731
    hp = None
    if prec:
        fv = ir.ilu0_rows(n, rowptr, colind, values)
        hp = lambda v: tr.solve_by_levels(n, rowptr, colind, fv,                            # noqa: E731
                                          tr.solve_by_levels(n, rowptr, colind, fv, v, True, True), False, False)
    ref = kr.METHODS[method](mul, hp, b, np.zeros_like(b), tol, MAXIT)
    a = make("csr", pattern, values)
    # Row 0 of the banded pattern has 437 entries (column 0 collects every clamped draw of rows 1 .. 512), and the default
    # plan leaves the 64-row tile of a row above 128 entries to the overflow kernel, which sums in another order.  With
    # the limit raised every row goes through the stream kernel, whose sums are the sequential ones.
    a.device().set_option("stream_row_max", 1024)
    d = a.device().describe()
    assert d["kernel"] == "stream" and d["overflow_tiles"] == 0 and d["stream_row_fraction"] == 1.0
    x = np.random.default_rng(9).uniform(-1, 1, size=n).astype(dtype)
    tr.assert_same_bits(a.device().spmv(x), mul(x))
    same_result(a.solve(b, method, M=a.ilu0() if prec else None, tol=tol, maxit=MAXIT), ref)


# ---- 4. the poll interval --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method,prec", [("cg", False), ("bicgstab", False), ("cg", True), ("bicgstab", True)])
def test_check_every_changes_nothing(method, prec):
    pattern, values, b = case("banded", method, np.float64)
    a = make("csr", pattern, values)
    f = a.ilu0() if prec else None
    first = a.solve(b, method, M=f, tol=1e-10, maxit=MAXIT)
    assert first[1].reason == 0
    for every in (1, 3, 1000):
        a.device().set_option("krylov_check_every", every)
        x, info = a.solve(b, method, M=f, tol=1e-10, maxit=MAXIT)
        tr.assert_same_bits(x, first[0])
        assert (info.iterations, info.reason, info.residual_sq) == (first[1].iterations, 0, first[1].residual_sq)
        d = a.device().describe()["krylov"]
        assert d["check_every"] == every and d["polls"] == -(-info.iterations // every)   # the poll after the stop is the last
    with pytest.raises(sp.Panic, match="krylov_check_every must be >= 1"):
        a.device().set_option("krylov_check_every", 0)


# ---- 5. maxit --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_maxit_limits(method, kind):
    pattern, values, b = case("banded", method, np.float64)
    a = make(kind, pattern, values)
    ops = device_ops(a, None)
    x0 = np.random.default_rng(5).uniform(-1, 1, size=b.size)
    for every in (None, 2):
        if every:
            a.device().set_option("krylov_check_every", every)
        x, info = a.solve(b, method, x0=x0, tol=1e-10, maxit=3)
        assert info.reason == 1 and info.iterations == 3
        same_result((x, info), kr.METHODS[method](*ops, b, x0, 1e-10, 3))
    x, info = a.solve(b, method, x0=x0, tol=1e-10, maxit=0)
    assert info.reason == 1 and info.iterations == 0
    tr.assert_same_bits(x, x0)
    r0 = b - ops[0](x0)
    assert info.residual_sq == float(kr.dot(r0, r0)) and info.rhs_sq == float(kr.dot(b, b))
    # x0 already solves the system: reason 0 at it = 0
    exact = a.solve(b, method, tol=1e-10, maxit=MAXIT)[0]
    x, info = a.solve(b, method, x0=exact, tol=1e-8, maxit=MAXIT)
    assert info.reason == 0 and info.iterations == 0
    tr.assert_same_bits(x, exact)


# ---- 6. breakdown ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_zero_matrix_is_a_breakdown_not_an_error(method, dtype):
    pattern, _, b = case("banded", method, dtype)
    a = make("csr", pattern, np.zeros(pattern[2].size, dtype=dtype))
    x, info = a.solve(b, method, tol=TOL[dtype], maxit=MAXIT)          # SPAL_OK: no exception
    assert info.reason == 2 and info.iterations == 1 and not np.isfinite(info.residual_sq)
    same_result((x, info), kr.METHODS[method](*device_ops(a, None), b, np.zeros_like(b), TOL[dtype], MAXIT))


# ---- 7. first touch, under a wall-clock guard of its own -------------------------------------------------------------

_FIRST_TOUCH = """
import sys
sys.path.insert(0, {root!r})
import numpy as np
import spalinalg_amd as sp
from tests import krylov_ref as kr, lazy_cases as zoo, trsv_ref as tr
c = zoo.case("skew_det")
n = c.nrows
rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(c.rowptr.astype(np.int64)))
d = np.arange(n, dtype=np.int64)
pattern = tr.from_coo(n, np.concatenate([rows, d]), np.concatenate([c.colind.astype(np.int64), d]))
assert zoo.auto_split_met(n, pattern[1])
values, b = tr.fill(pattern, np.float64, np.random.default_rng(7))
r = np.repeat(np.arange(n, dtype=np.uint64), np.diff(pattern[1].astype(np.int64)))
perm = np.random.default_rng(8).permutation(values.size)
a = sp.CsrMatrix.from_coo(sp.CooMatrix.with_triplets(n, n, r[perm], pattern[2][perm], values[perm]))
m = a.ilu0()                                  # the lower solve plan; the product plan and m's upper plan do not exist yet
assert "upper" not in m.device().describe()["trsv"]
x, info = a.solve(b, "bicgstab", M=m, tol=1e-10, maxit=3)
assert a.device().describe()["kernel"] in ("split", "blockwin")
mul = lambda v: a.device().spmv(v)
prec = lambda v: m.solve_triangular(m.solve_triangular(v, True, True), False)
xr, ref = kr.bicgstab(mul, prec, b, np.zeros_like(b), 1e-10, 3)
tr.assert_same_bits(x, xr)
assert (info.iterations, info.reason, info.residual_sq) == (ref["iterations"], ref["reason"], ref["residual_sq"])
print("first touch ok", info.iterations, info.reason)
"""


def test_first_product_and_upper_plan_are_the_solvers():
    out = subprocess.run([sys.executable, "-c", _FIRST_TOUCH.format(root=ROOT)], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "first touch ok" in out.stdout


# ---- 8. two threads, one handle --------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_two_threads_solve_on_one_handle(kind):
    pattern, values, b = case("banded", "bicgstab", np.float64)
    a = make(kind, pattern, values)
    f = a.ilu0()
    bs = [b, np.random.default_rng(77).uniform(-1, 1, size=b.size)]
    expect = [a.solve(v, "bicgstab", M=f, tol=1e-10, maxit=MAXIT) for v in bs]
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i):
        try:
            gate.wait(timeout=30)
            results[i] = a.solve(bs[i], "bicgstab", M=f, tol=1e-10, maxit=MAXIT)
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


# ---- 9. refusals -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_refusals(kind):
    lib = _ffi.lib()
    pattern, values, b = case("full", "bicgstab", np.float64)
    n = pattern[0]
    a = make(kind, pattern, values)
    dev = a.device()
    f = a.ilu0().device()
    x0, info = dev.krylov(b, "bicgstab", M=f, tol=1e-10, maxit=MAXIT)
    host = getattr(lib, f"spal_{kind}_krylov_f64")
    devf = getattr(lib, f"spal_{kind}_krylov_dev_f64")
    cinfo = sp.matrix._KrylovInfoC()
    x = np.zeros(n)
    pb, px = b.ctypes.data_as(_ffi.f64p), x.ctypes.data_as(_ffi.f64p)

    def refused(status, text, call):
        assert call() == status, lib.spal_last_error()
        assert text in lib.spal_last_error().decode(), lib.spal_last_error()

    inv, fn = _ffi.SPAL_ERR_INVALID_ARGUMENT, f"spal_{kind}_krylov"
    args = (C.c_uint64(n), px, C.c_uint64(n), C.c_double(1e-10), C.c_uint64(5), C.byref(cinfo))
    refused(inv, fn + ": null argument", lambda: host(None, 0, None, pb, *args))
    refused(inv, "null argument", lambda: host(dev._h, 0, None, None, *args))
    refused(inv, "null argument", lambda: host(dev._h, 0, None, pb, C.c_uint64(n), None, *args[2:]))
    refused(inv, "null argument", lambda: host(dev._h, 0, None, pb, *args[:-1], None))
    refused(inv, f"b.len() = {n - 1}", lambda: host(dev._h, 0, None, pb, C.c_uint64(n - 1), *args[1:]))
    refused(inv, f"x.len() = {n + 1}", lambda: host(dev._h, 0, None, pb, C.c_uint64(n), px, C.c_uint64(n + 1), *args[3:]))
    refused(inv, "method = 2 must be 0 (CG) or 1 (BiCGStab)", lambda: host(dev._h, 2, None, pb, *args))
    refused(inv, "method = -1", lambda: host(dev._h, -1, None, pb, *args))
    for bad in (-1e-3, float("nan")):
        refused(inv, "must be >= 0", lambda: host(dev._h, 0, None, pb, C.c_uint64(n), px, C.c_uint64(n), C.c_double(bad),
                                                  C.c_uint64(5), C.byref(cinfo)))
    refused(inv, "handle holds f64 values",
            lambda: getattr(lib, f"spal_{kind}_krylov_f32")(dev._h, 0, None, x.astype(np.float32).ctypes.data_as(_ffi.f32p),
                                                            C.c_uint64(n), x.astype(np.float32).ctypes.data_as(_ffi.f32p),
                                                            *args[2:]))
    cls = sp.CsrMatrix if kind == "csr" else sp.CscMatrix
    rect = cls(2, 3, [0, 1, 2] if kind == "csr" else [0, 1, 2, 2], [0, 1], np.array([1.0, 2.0])).device()
    refused(inv, "not square (2 x 3)", lambda: host(rect._h, 0, None, pb, C.c_uint64(2), px, C.c_uint64(2), *args[3:]))
    small = make(kind, *case("diagonal", "cg", np.float64)[:2]).device()
    refused(inv, "the preconditioner is 1025 x 1025", lambda: host(dev._h, 0, small._h, pb, *args))
    f32 = make(kind, pattern, values.astype(np.float32)).device()
    refused(inv, "element sizes 8 and 4", lambda: host(dev._h, 0, f32._h, pb, *args))
    nodiag_pattern = tr.drop_diagonal(pattern, 7)
    nodiag = make(kind, nodiag_pattern, np.ones(nodiag_pattern[2].size)).device()
    refused(inv, "row 7 stores no diagonal entry", lambda: host(dev._h, 1, nodiag._h, pb, *args))
    import torch
    bt = torch.tensor(b).cuda()
    refused(inv, "x_dev == b_dev", lambda: devf(dev._h, 0, None, C.c_void_p(bt.data_ptr()), C.c_void_p(bt.data_ptr()),
                                               C.c_double(1e-10), C.c_uint64(5), None, C.byref(cinfo)))
    refused(inv, "null argument", lambda: devf(dev._h, 0, None, C.c_void_p(bt.data_ptr()), None, C.c_double(1e-10),
                                               C.c_uint64(5), None, C.byref(cinfo)))
    with pytest.raises(sp.Panic, match="must be 'cg' or 'bicgstab'"):
        a.solve(b, "gmres")
    with pytest.raises(TypeError):
        a.solve(b, "cg", M=make("csc" if kind == "csr" else "csr", pattern, values))
    # the handles work as before (every block a refused call took is owned by a scope guard: the library keeps no
    # allocator counters a test could read)
    sp.cache_trim()
    x1, info1 = dev.krylov(b, "bicgstab", M=f, tol=1e-10, maxit=MAXIT)
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
        for method in ("cg", "bicgstab"):
            with pytest.raises(sp.SpalError, match="row blocks") as e:
                a.solve(b, method, M=m, maxit=3)
            assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED


# ---- the device-pointer form -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_device_pointer_form_on_a_stream(method):
    import torch
    pattern, values, b = case("banded", method, np.float32)
    a = make("csr", pattern, values)
    f = a.ilu0()
    want = a.solve(b, method, M=f, tol=1e-5, maxit=MAXIT)
    bt = torch.tensor(b).cuda()
    xt = torch.zeros_like(bt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    info = a.device().krylov_dev(bt.data_ptr(), xt.data_ptr(), method, M=f.device(), tol=1e-5, maxit=MAXIT, stream=s)
    tr.assert_same_bits(xt.cpu().numpy(), want[0])               # the call has synchronised its stream
    assert (info.iterations, info.reason, info.residual_sq) == (want[1].iterations, 0, want[1].residual_sq)
    tr.assert_same_bits(bt.cpu().numpy(), b)


# ---- 10. the C ABI from C ---------------------------------------------------------------------------------------------

def test_c_abi_demo():
    exe = os.path.join(ROOT, "tests", "c", "krylov_demo")
    lib = os.path.join(ROOT, "spalinalg_amd", "lib")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "krylov_demo.c"), "-o", exe, "-L", lib, "-lspal_hip", "-lm",
                           f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "krylov demo ok" in out.stdout
