"""eigsh on the device against its sequential text (tests/eigsh_ref.py) on the directed cases and the seeded random
matrices of tests/eigsh_cases.py: raw bits of theta, resid and X, and restarts, products, converged and reason, through
`check` of tests/test_gpu_eigsh.py.  There is no tolerance anywhere in this file.

The directed cases reach the exits no hand-made input reaches: exhaustion (hn == 0) at step L of a phase, on either side
of the basis batch of 8, where every later launch of the phase must return before it writes; stop 2 decided in the
middle of a phase and after restarts, followed by a good call on the same handle (stale flags would show); LDS rotation
tiles of 512 and 1024 rows, two or three of them with a partial last one; one rotation tile more than the grid has
workgroups; ncv == n.  Exhaustion AFTER a restart is not reachable: the rotated basis is no longer exact, so hn == 0
cannot be constructed there.  tests/test_eigsh_cases_host.py asserts on the CPU what the text does on every case here.

The case of 524 289 rows takes 1.5 s in f64 and 0.7 s (ncv = 17) and 2.3 s (ncv = 33) in f32; the longest is ncv == n
= 256 at 3.4 s.  Nearly all of either is the text on the CPU."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import eigsh_cases as ec
from tests import trsv_ref as tr
from tests.test_gpu_eigsh import check, lib_jacobi, make

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
KINDS = ["csr", "csc"]
FILL = 9
same = tr.assert_same_bits


def c_call(dev, kind, dtype, k, which, ncv, v0, tol, maxit):
    """The C entry on buffers filled with FILL: (theta, resid, x, info), x of shape (n, k)."""
    n = dev.shape()[0]
    ct = _ffi.f64p if dtype == np.float64 else _ffi.f32p
    theta, resid, x = np.full(k, FILL, dtype), np.full(k, FILL, dtype), np.full((n, k), FILL, dtype)
    info = sp.matrix._EigshInfoC()
    u = C.c_uint64
    fn = getattr(_ffi.lib(), f"spal_{kind}_eigsh_{'f64' if dtype == np.float64 else 'f32'}")
    assert fn(dev._h, u(k), C.c_int(0 if which == "LA" else 1), u(ncv), v0.ctypes.data_as(ct), u(n), u(0), C.c_double(tol), u(maxit),
              theta.ctypes.data_as(ct), u(k), resid.ctypes.data_as(ct), u(k), x.ctypes.data_as(ct), u(k), u(n), C.byref(info)) == 0
    return theta, resid, x, info


# ---- 1. exhaustion at step L ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("L", ec.EXHAUSTION_L)
def test_exhaustion_in_the_middle_of_a_phase(L, dtype):
    mat = ec.exhaustion(L, dtype)
    n, ncv = ec.EXHAUSTION_N, ec.EXHAUSTION_NCV
    v0 = ec.e0(n, dtype)
    for kind in KINDS:
        for form in (1, 2):
            a = make(kind, mat)
            (theta, X, info), ref = check(a, n, dtype, 3, "LA", ncv, 1e-6, 5, v0=v0, rotate=form)
            assert (info.products, info.restarts) == (L, 0) and (info.reason, X.shape[1]) == ((0, 3) if L >= 3 else (3, L))
            (theta, X, info), ref = check(a, n, dtype, L + 1, "SA", ncv, 1e-6, 5, v0=v0)
            assert (info.products, info.restarts, info.reason, info.converged, X.shape[1]) == (L, 0, 3, L, L)
            # what lies past the pairs found keeps its fill
            th, rs, x, cinfo = c_call(a.device(), kind, dtype, L + 1, "SA", ncv, v0, 1e-6, 5)
            assert (cinfo.reason, cinfo.products, cinfo.converged) == (3, L, L)
            same(th[:L], ref["theta"])
            same(rs[:L], ref["resid"])
            same(x[:, :L], ref["X"])
            assert np.all(th[L:] == FILL) and np.all(rs[L:] == FILL) and np.all(x[:, L:] == FILL)


# ---- 2. stop 2 in the middle of a phase and after restarts ----------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_overflow_in_the_middle_of_a_phase_and_after_restarts(kind, dtype):
    n, k = ec.OVERFLOW_N, ec.OVERFLOW_K
    v0 = ec.e0(n, dtype)
    far = np.zeros(n, dtype=dtype)
    far[n - 1] = 1.0                                                # from here the large coupling is never multiplied
    o = ec.OVERFLOW_RESTARTED
    cases = [(p, ec.OVERFLOW_NCV, p + 1, 0) for p in ec.OVERFLOW_P] + [(o["p"], o["ncv"], o["products"], o["restarts"])]
    for i, (p, ncv, products, restarts) in enumerate(cases):
        a = make(kind, ec.overflow(p, dtype))
        (theta, X, info), _ = check(a, n, dtype, k, "LA", ncv, 1e-6, 5, v0=v0, rotate=1 + i % 2)
        assert (info.reason, info.products, info.restarts, info.converged) == (2, products, restarts, 0)
        assert theta.size == 0 and X.shape == (n, 0)
        th, rs, x, cinfo = c_call(a.device(), kind, dtype, k, "LA", ncv, v0, 1e-6, 5)
        assert (cinfo.reason, cinfo.products, cinfo.restarts) == (2, products, restarts)
        assert np.all(th == FILL) and np.all(rs == FILL) and np.all(x == FILL)
        # a good call on the same handle: the text's bits (stale flags in the head would show here)
        (theta, X, info), _ = check(a, n, dtype, k, "LA", ncv, 1e-6, 0 if restarts == 0 else 2, v0=far)
        assert info.reason in (0, 1) and X.shape == (n, k) and np.isfinite(X).all()


# ---- 3. the rotation's tiles ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,ncv", ec.ROTATION_TILES)
def test_large_rotation_tiles(n, ncv, dtype):
    mat = ec.banded(n, dtype)
    a = make("csr", mat)
    (theta, X, info), _ = check(a, n, dtype, 1, "LA", ncv, ec.TOL[np.dtype(dtype)], 2, rotate=2)
    d = a.device().describe()["eigsh"]
    rows = ec.rot_tile_rows(ncv, np.dtype(dtype).itemsize)
    assert (d["rotate"], d["rotate_tile_rows"]) == ("lds", rows) and rows in (512, 1024) and n > rows and n % rows
    assert info.restarts == 2 and d["rotate_ms"] > 0.0
    b = make("csr", mat)
    b.device().set_option("eigsh_rotate", 1)
    theta1, X1, info1 = b.eigsh(1, "LA", ncv, tol=ec.TOL[np.dtype(dtype)], maxit=2)
    assert b.device().describe()["eigsh"]["rotate"] == "batch"
    same(theta1, theta)
    same(X1, X)
    same(info1.resid, info.resid)


@pytest.mark.parametrize("kind,dtype,ncv", [("csr", np.float64, ec.MANY_TILES["ncv"]), ("csc", np.float32, ec.MANY_TILES["ncv"]),
                                            ("csc", np.float32, ec.MANY_TILES["ncv_f32"])], ids=["csr-f64-17", "csc-f32-17", "csc-f32-33"])
def test_more_rotation_tiles_than_workgroups(kind, dtype, ncv):
    """n = 8192 * 64 + 1: with tiles of 64 rows (f64 at ncv = 17, f32 at ncv = 33) workgroup 0 of rotate_lds walks a second
    tile, the partial one.  (f32 at ncv = 17 has tiles of 128 rows, one per workgroup.)"""
    t_start = time.perf_counter()
    mt = ec.MANY_TILES
    n, k = mt["n"], mt["k"]
    mat = ec.laplacian_plus(n, dtype)
    a = make(kind, mat)
    (theta, X, info), _ = check(a, n, dtype, k, "SA", ncv, ec.TOL[np.dtype(dtype)], mt["maxit"], jacobi_fn=lib_jacobi, rotate=2)
    d = a.device().describe()["eigsh"]
    rows = ec.rot_tile_rows(ncv, np.dtype(dtype).itemsize)
    assert (d["rotate"], d["rotate_tile_rows"], info.restarts, info.reason) == ("lds", rows, 1, 1)
    assert (-(-n // rows) > ec.ROT_MAX_GRID) == (rows == 64)
    b = make(kind, mat)
    b.device().set_option("eigsh_rotate", 1)
    theta1, X1, info1 = b.eigsh(k, "SA", ncv, tol=ec.TOL[np.dtype(dtype)], maxit=mt["maxit"])
    same(theta1, theta)
    same(X1, X)
    same(info1.resid, info.resid)
    print(f"eigsh {n} rows {kind} {np.dtype(dtype).name} ncv {ncv}: tiles of {rows} rows, {info.products} products, "
          f"{time.perf_counter() - t_start:.2f} s")


# ---- 4. ncv == n ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,k", ec.FULL_BASIS)
def test_a_basis_of_the_whole_space(n, k, dtype):
    mat = ec.banded(n, dtype)
    for kind, form in (("csr", 1), ("csc", 2)):
        (theta, X, info), _ = check(make(kind, mat), n, dtype, k, "LA", n, ec.default_tol(dtype) * 100, 1,
                                    jacobi_fn=lib_jacobi if n > 24 else None, rotate=form)
        assert info.reason in (0, 1, 3) and X.shape == (n, k)


# ---- 5. the fuzz ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(int(os.environ.get("SPAL_FUZZ_SEEDS", "24"))))   # (more seeds: a longer soak)
def test_eigsh_is_its_sequential_text(seed):
    t_start = time.perf_counter()
    mat, k = ec.case(seed)
    n, dtype = k["n"], k["dtype"].type
    jacobi_fn = lib_jacobi if k["jacobi"] == "lib" else None
    a = make(k["kind"], mat)
    (theta, X, info), ref = check(a, n, dtype, k["k"], k["which"], k["ncv"], k["tol"], k["maxit"], v0=k["v0"], seed=k["seed"],
                                  jacobi_fn=jacobi_fn, rotate=k["rotate"])
    assert info.reason in (0, 1)
    # the other rotation form on a fresh handle: the same bits
    b = make(k["kind"], mat)
    b.device().set_option("eigsh_rotate", 3 - k["rotate"])
    theta1, X1, info1 = b.eigsh(k["k"], k["which"], k["ncv"], k["v0"], k["seed"], k["tol"], k["maxit"])
    assert b.device().describe()["eigsh"]["rotate"] == ("batch" if k["rotate"] == 2 else "lds")
    same(theta1, theta)
    same(X1, X)
    same(info1.resid, info.resid)
    assert (info1.restarts, info1.products, info1.converged, info1.reason) == (info.restarts, info.products, info.converged, info.reason)
    # device pointers, a stream of the caller's, ldx > k
    if seed % 3 == 0:
        import torch
        kk = k["k"]
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        xt = torch.full((n, kk + 3), 7, dtype=tdt, device="cuda")
        v0t = None if k["v0"] is None else torch.tensor(np.array(k["v0"])).cuda()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        th2, rs2 = np.zeros(kk, dtype), np.zeros(kk, dtype)
        info2 = b.device().eigsh_dev(kk, th2, rs2, xt.data_ptr(), kk + 3, which=k["which"], ncv=k["ncv"],
                                     v0_ptr=0 if v0t is None else v0t.data_ptr(), seed=k["seed"], tol=k["tol"], maxit=k["maxit"], stream=s)
        got = xt.cpu().numpy()                                      # the call has synchronised its stream
        same(got[:, :kk], X)
        assert np.all(got[:, kk:] == 7) and (info2.restarts, info2.products, info2.reason) == (info.restarts, info.products, info.reason)
        same(th2, theta)
        same(rs2, info.resid)
    print(f"eigsh fuzz seed {seed}: n {n} {k['kind']} {k['dtype'].name} {k['cls']} ncv {k['ncv']} k {k['k']} {k['which']} "
          f"tol {k['tol']:.0e} maxit {k['maxit']} rotate {k['rotate']} (reason, restarts, products) "
          f"{(info.reason, info.restarts, info.products)} {time.perf_counter() - t_start:.2f} s")
