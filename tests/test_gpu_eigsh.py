"""eigsh on the device against its sequential text (tests/eigsh_ref.py): raw bits of theta, resid and X equal, and
restarts, products, converged and reason, f64 and f32, CSR and CSC, LA and SA.

As in tests/test_gpu_gmres.py the reference runs with the device's own spmv as its product (deterministic, so the
comparison is bit for bit whichever SpMV kernel the plan picks).  The sizes put the dot's tiles of 1024 and the vector
loads of 4 on both sides, ncv and keep the basis batch of 8 and the rotation batch of 8."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import eigsh_ref as er
from tests import gmres_ref as gr
from tests import ilu_ref as ir
from tests import krylov_ref as kr
from tests import trsv_ref as tr

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
TOL = {np.float64: 1e-10, np.float32: 1e-5}
DESCRIBE_KEYS = {"k", "which", "ncv", "keep", "restarts", "products", "converged", "reason", "polls", "rotate",
                 "rotate_tile_rows", "basis_bytes", "rotate_ms", "solve_ms"}


def lib_jacobi(S):
    """tests/eigsh_ref.jacobi's bits from the library's host routine (tests/test_eigsh_host.py compares the two)"""
    S = np.ascontiguousarray(S, dtype=np.float64)
    m = S.shape[0]
    theta, Y, sweeps = np.zeros(m), np.zeros((m, m)), C.c_uint64()
    assert _ffi.lib().spal_eigsh_jacobi(C.c_uint64(m), S.ctypes.data_as(_ffi.f64p), theta.ctypes.data_as(_ffi.f64p),
                                        Y.ctypes.data_as(_ffi.f64p), C.byref(sweeps)) == 0
    return theta, Y, sweeps.value


@functools.lru_cache(maxsize=None)
def named(name, dtype):
    """(n, rowptr, colind, values) of A1 / A2; shared, read-only"""
    dense = er.laplace_1d_plus() if name == "A1" else er.laplace_2d_plus()
    out = er.dense_to_csr(dense, dtype)
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def banded(n, dtype):
    """a small banded symmetric matrix, as the solver fuzz's: (n, rowptr, colind, values)"""
    rng = np.random.default_rng(zlib.crc32(f"eigsh/{n}".encode()))
    pattern = ir.sym(tr.banded(n, 3, min(12, max(n - 1, 1)), rng))
    values, _ = kr.spd_fill(pattern, dtype, rng)
    for a in (*pattern[1:], values):
        a.setflags(write=False)
    return (*pattern, values)


def make(kind, mat):
    n, rowptr, colind, values = mat
    if kind == "csr":
        return sp.CsrMatrix(n, n, rowptr, colind, values)
    colptr, rowind, vals, _ = ir.to_csc((n, rowptr, colind), values)
    return sp.CscMatrix(n, n, colptr, rowind, vals)


def check(a, n, dtype, k, which, ncv, tol, maxit, v0=None, seed=0, jacobi_fn=None, rotate=None):
    """One call against the text on the device's own product (tol = 0 is the machine epsilon); returns (got, ref)."""
    dev = a.device()
    if rotate is not None:
        dev.set_option("eigsh_rotate", rotate)
    theta, X, info = a.eigsh(k, which, ncv, v0, seed, tol, maxit)
    ref = er.eigsh(lambda v: dev.spmv(v), n, dtype, k, which, ncv, tol or float(np.finfo(dtype).eps), maxit, v0, seed, jacobi_fn)
    assert (info.restarts, info.products, info.converged, info.reason) == \
        (ref["restarts"], ref["products"], ref["converged"], ref["reason"])
    tr.assert_same_bits(theta, ref["theta"])
    tr.assert_same_bits(info.resid, ref["resid"])
    tr.assert_same_bits(X, ref["X"])
    d = dev.describe()["eigsh"]
    assert set(d) == DESCRIBE_KEYS
    assert (d["k"], d["which"], d["ncv"], d["keep"]) == (k, which, ncv, er.keep_of(k, ncv))
    assert (d["restarts"], d["products"], d["reason"], d["polls"]) == (info.restarts, info.products, info.reason, info.restarts + 1)
    nvec = (ncv + 1) + 1 + (ncv + 1 if d["rotate"] == "batch" else 0)      # the basis, w, and a second basis out of place
    assert d["basis_bytes"] == nvec * (-(-n // 64) * 64) * np.dtype(dtype).itemsize
    return (theta, X, info), ref


# ---- 1. bits against the text --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("which", ["LA", "SA"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("name,k,ncv", [("A1", 4, 16), ("A2", 3, 9)])
def test_eigsh_is_the_text_and_converges(name, k, ncv, kind, which, dtype):
    mat = named(name, dtype)
    (theta, X, info), _ = check(make(kind, mat), mat[0], dtype, k, which, ncv, TOL[dtype], 100)
    assert info.reason == 0 and info.converged == k and info.restarts >= 3
    dense = (er.laplace_1d_plus() if name == "A1" else er.laplace_2d_plus())
    lam = np.linalg.eigvalsh(dense)
    want = lam[::-1][:k] if which == "LA" else lam[:k]
    x64, t64 = X.astype(np.float64), theta.astype(np.float64)
    res = np.linalg.norm(dense.astype(dtype).astype(np.float64) @ x64 - x64 * t64, axis=0) / np.linalg.norm(x64, axis=0)
    assert np.all(res <= 2 * TOL[dtype] * np.abs(lam).max())
    assert np.all(np.abs(t64 - want) <= res + (1e-12 + np.finfo(dtype).eps) * np.abs(lam).max())   # theta is rounded to the dtype


# n on both sides of the tiles of 1024 and the loads of 4; ncv on both sides of the batch of 8; keep = 1, 5, 8, 9, 12, 63
SHAPES = [(9, 2, 1), (9, 8, 7), (255, 8, 1), (256, 9, 1), (256, 9, 8), (257, 16, 1), (257, 16, 15), (1023, 17, 1),
          (1023, 17, 16), (1025, 64, 63), (1025, 16, 8), (4099, 8, 3)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,ncv,k", SHAPES)
def test_sizes_batches_and_keep(n, ncv, k, dtype):
    which = "LA" if (n + ncv + k) % 2 else "SA"
    kind = "csc" if n in (256, 1025) else "csr"
    _, ref = check(make(kind, banded(n, dtype)), n, dtype, k, which, ncv, TOL[dtype], 2)
    assert ref["reason"] in (0, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_largest_basis(dtype):
    """ncv = 256 on n = 300 with the LDS row tiles ("eigsh_rotate" = 2): the rotation tile's largest m -- in f64 one tile of
    64 rows x 256 values, 128 KiB of dynamic LDS, past the opt-in -- in a restart IN PLACE (keep = 129: 17 batches of
    outputs) and in the final rotation; bits against the text, and against the batched form."""
    mat = banded(300, dtype)
    a = make("csr", mat)
    (theta, X, info), ref = check(a, 300, dtype, 2, "LA", 256, 1e-300, 1, jacobi_fn=lib_jacobi, rotate=2)
    d = a.device().describe()["eigsh"]
    assert (ref["products"], ref["restarts"], ref["reason"]) == (256 + 256 - 129, 1, 1)
    assert (d["rotate"], d["keep"], d["rotate_tile_rows"]) == ("lds", 129, 64) and d["rotate_ms"] > 0.0
    b = make("csr", mat)
    b.device().set_option("eigsh_rotate", 1)
    theta1, X1, info1 = b.eigsh(2, "LA", 256, tol=1e-300, maxit=1)
    assert b.device().describe()["eigsh"]["rotate"] == "batch" and info1.restarts == 1
    tr.assert_same_bits(theta1, theta)
    tr.assert_same_bits(X1, X)
    tr.assert_same_bits(info1.resid, info.resid)


# ---- 2. restart and exit paths -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("maxit", [0, 1])
def test_maxit_bounds_the_restarts(maxit):
    mat = named("A1", np.float64)
    (_, X, info), _ = check(make("csr", mat), mat[0], np.float64, 3, "SA", 9, 1e-10, maxit)
    assert info.reason == 1 and info.restarts == maxit and X.shape == (200, 3)


def test_convergence_in_the_first_phase_rotates_once():
    n = 40                                                       # two eigenvalues far above the rest
    values = np.concatenate([np.linspace(0.0, 1.0, n - 2), [100.0, 200.0]])
    ptr = np.arange(n + 1, dtype=np.uint64)
    a = sp.CsrMatrix(n, n, ptr, ptr[:-1].copy(), values)
    (theta, X, info), _ = check(a, n, np.float64, 2, "LA", 20, 1e-8, 5)
    assert info.reason == 0 and info.restarts == 0 and info.products == 20
    assert a.device().describe()["eigsh"]["rotate_ms"] == 0.0
    assert np.allclose(theta, [200.0, 100.0], rtol=1e-12)


# ---- 3. start vectors ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_callers_start_vector_and_the_seed(dtype):
    mat = named("A2", dtype)
    a = make("csr", mat)
    v0 = np.random.default_rng(5).uniform(-1, 1, size=mat[0]).astype(dtype)
    check(a, mat[0], dtype, 2, "LA", 8, TOL[dtype], 3, v0=v0)
    (t7, _, _), _ = check(a, mat[0], dtype, 2, "LA", 8, TOL[dtype], 3, seed=7)
    (tw, _, _), _ = check(a, mat[0], dtype, 2, "LA", 8, TOL[dtype], 3, seed=(1 << 32) + 7)
    tr.assert_same_bits(t7, tw)                              # only seed mod 2^32 enters


def test_e0_on_a_diagonal_matrix_exhausts_the_space():
    n = 12
    ptr = np.arange(n + 1, dtype=np.uint64)
    a = sp.CsrMatrix(n, n, ptr, ptr[:-1].copy(), np.arange(2, n + 2, dtype=np.float64))
    e0 = np.zeros(n)
    e0[0] = 1.0
    (theta, X, info), _ = check(a, n, np.float64, 2, "LA", 6, 1e-10, 5, v0=e0)
    assert info.reason == 3 and info.products == 1 and info.converged == 1 and theta.tolist() == [2.0] and X.shape == (n, 1)
    assert np.array_equal(X[:, 0], e0)
    (theta, X, info), _ = check(a, n, np.float64, 1, "LA", 6, 1e-10, 5, v0=e0)
    assert info.reason == 0 and info.products == 1 and theta.tolist() == [2.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_values_that_are_not_finite_stop_with_reason_2(dtype):
    mat = named("A2", dtype)
    n = mat[0]
    v0 = np.ones(n, dtype=dtype)
    v0[5] = np.nan
    (theta, X, info), _ = check(make("csr", mat), n, dtype, 2, "LA", 8, TOL[dtype], 3, v0=v0)
    assert info.reason == 2 and info.converged == 0 and theta.size == 0 and X.shape == (n, 0) and info.products == 1
    values = mat[3].copy()
    values[7] = np.inf
    (theta, X, info), _ = check(make("csr", (n, mat[1], mat[2], values)), n, dtype, 2, "SA", 8, TOL[dtype], 3)
    assert info.reason == 2 and theta.size == 0
    # through the C entry: theta, resid and x are left as they were
    dev = make("csr", mat).device()
    ct = _ffi.f64p if dtype == np.float64 else _ffi.f32p
    theta, resid, x = np.full(2, 9, dtype), np.full(2, 9, dtype), np.full((n, 2), 9, dtype)
    cinfo = sp.matrix._EigshInfoC()
    u = C.c_uint64
    fn = getattr(_ffi.lib(), f"spal_csr_eigsh_{'f64' if dtype == np.float64 else 'f32'}")
    assert fn(dev._h, u(2), C.c_int(0), u(8), v0.ctypes.data_as(ct), u(n), u(0), C.c_double(1e-6), u(3),
              theta.ctypes.data_as(ct), u(2), resid.ctypes.data_as(ct), u(2), x.ctypes.data_as(ct), u(2), u(n),
              C.byref(cinfo)) == 0
    assert cinfo.reason == 2 and np.all(theta == 9) and np.all(resid == 9) and np.all(x == 9)


# ---- 4. output layout ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_values_only_padding_and_the_device_form(dtype):
    import torch
    mat = named("A1", dtype)
    n, k, ncv = mat[0], 3, 12
    a = make("csr", mat)
    dev = a.device()
    want_theta, want_x, want = a.eigsh(k, "SA", ncv, tol=TOL[dtype], maxit=4)
    theta, X, info = a.eigsh(k, "SA", ncv, tol=TOL[dtype], maxit=4, return_eigenvectors=False)     # x = NULL
    assert X is None and (info.restarts, info.products, info.reason) == (want.restarts, want.products, want.reason)
    tr.assert_same_bits(theta, want_theta)
    # ldx > k through the host entry: the padding is untouched
    ct = _ffi.f64p if dtype == np.float64 else _ffi.f32p
    sfx = "f64" if dtype == np.float64 else "f32"
    u = C.c_uint64
    th, rs, x = np.zeros(k, dtype), np.zeros(k, dtype), np.full((n, k + 2), 7, dtype)
    cinfo = sp.matrix._EigshInfoC()
    assert getattr(_ffi.lib(), f"spal_csr_eigsh_{sfx}")(dev._h, u(k), C.c_int(1), u(ncv), None, u(0), u(0), C.c_double(TOL[dtype]),
                                                        u(4), th.ctypes.data_as(ct), u(k), rs.ctypes.data_as(ct), u(k),
                                                        x.ctypes.data_as(ct), u(k + 2), u(n), C.byref(cinfo)) == 0
    tr.assert_same_bits(x[:, :k], want_x)
    assert np.all(x[:, k:] == 7)
    # device pointers, a stream of the caller's, ldx > k
    xt = torch.full((n, k + 1), 7, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    th2, rs2 = np.zeros(k, dtype), np.zeros(k, dtype)
    info2 = dev.eigsh_dev(k, th2, rs2, xt.data_ptr(), k + 1, which="SA", ncv=ncv, tol=TOL[dtype], maxit=4, stream=s)
    got = xt.cpu().numpy()                                       # the call has synchronised its stream
    tr.assert_same_bits(got[:, :k], want_x)
    assert np.all(got[:, k] == 7) and (info2.restarts, info2.reason) == (want.restarts, want.reason)
    tr.assert_same_bits(th2, want_theta)
    tr.assert_same_bits(rs2, want.resid)


@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_refusals_that_read_the_handle_and_a_capturing_stream(kind):
    import torch
    lib = _ffi.lib()
    mat = named("A2", np.float64)
    n = mat[0]
    dev = make(kind, mat).device()
    u = C.c_uint64
    th, rs, x = np.zeros(2), np.zeros(2), np.zeros((n, 2))
    th32 = np.zeros(2, np.float32)
    cinfo = sp.matrix._EigshInfoC()
    inv = _ffi.SPAL_ERR_INVALID_ARGUMENT
    p = lambda a: a.ctypes.data_as(_ffi.f64p)                                                  # noqa: E731
    host = getattr(lib, f"spal_{kind}_eigsh_f64")

    def call(h=dev._h, k=2, ncv=8, v0=None, v0_len=0, tl=2, rl=2, xr=n, fn=host):
        return fn(h, u(k), C.c_int(0), u(ncv), v0, u(v0_len), u(0), C.c_double(1e-8), u(3), p(th), u(tl), p(rs), u(rl), p(x), u(2),
                  u(xr), C.byref(cinfo))

    def refused(text, status):
        assert status == inv and text in lib.spal_last_error().decode(), (status, lib.spal_last_error())

    refused("handle holds f64 values", getattr(lib, f"spal_{kind}_eigsh_f32")(
        dev._h, u(2), C.c_int(0), u(8), None, u(0), u(0), C.c_double(1e-8), u(3), th32.ctypes.data_as(_ffi.f32p), u(2),
        th32.ctypes.data_as(_ffi.f32p), u(2), None, u(2), u(n), C.byref(cinfo)))
    refused(f"ncv = 200 exceeds the matrix's {n} rows", call(ncv=200))
    refused("theta.len() = 3", call(tl=3))
    refused("resid.len() = 1", call(rl=1))
    refused(f"X has {n - 1} rows", call(xr=n - 1))
    refused("v0.len() = 5", call(v0=p(np.zeros(5)), v0_len=5))
    wide = sp.CsrMatrix(3, 4, [0, 1, 2, 3], [0, 1, 3], np.ones(3)) if kind == "csr" else sp.CscMatrix(3, 4, [0, 1, 2, 2, 3], [0, 1, 2], np.ones(3))
    refused("the matrix is not square (3 x 4)", call(h=wide.device()._h, k=1, ncv=2, tl=1, rl=1, xr=3))
    assert not th.any() and not x.any()
    with pytest.raises(sp.Panic, match="eigsh_rotate must be 0"):
        dev.set_option("eigsh_rotate", 3)
    # a capturing stream
    xt = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()               # never replayed
    with torch.cuda.graph(graph):
        xt.fill_(0.0)                            # (so that the graph is not empty)
        capturing = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        status = getattr(lib, f"spal_{kind}_eigsh_dev_f64")(dev._h, u(2), C.c_int(0), u(8), None, u(0), C.c_double(1e-8), u(3), p(th),
                                                            p(rs), C.c_void_p(xt.data_ptr()), u(2), capturing, C.byref(cinfo))
        seen = (status, lib.spal_last_error().decode())
    torch.cuda.synchronize()
    assert seen[0] == inv and "cannot be captured into a graph" in seen[1], seen
    del graph


# ---- 5. independence, the shared kernels, memory -------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,ncv,k", [(1025, 17, 1), (257, 64, 20)])
def test_bits_do_not_depend_on_the_rotation_form(n, ncv, k, dtype):
    mat = banded(n, dtype)
    got = []
    for form in (1, 2):
        a = make("csr", mat)
        (theta, X, info), _ = check(a, n, dtype, k, "LA", ncv, TOL[dtype], 3, rotate=form)
        assert a.device().describe()["eigsh"]["rotate"] == ("batch" if form == 1 else "lds") and info.restarts >= 1
        got.append((theta, X, info.resid))
    for x, y in zip(*got):
        tr.assert_same_bits(x, y)
    a = make("csr", mat)
    a.device().set_option("krylov_check_every", 1)               # unused here
    theta, X, _ = a.eigsh(k, "LA", ncv, tol=TOL[dtype], maxit=3)
    tr.assert_same_bits(theta, got[0][0])
    tr.assert_same_bits(X, got[0][1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_gmres_still_returns_its_text_from_the_shared_kernels(dtype):
    mat = banded(1025, dtype)
    a = make("csr", mat)
    b = np.random.default_rng(3).uniform(-1, 1, size=1025).astype(dtype)
    x, info = a.gmres(b, restart=17, tol=TOL[dtype], maxit=60)
    xr, ir_ = gr.gmres(lambda v: a.device().spmv(v), None, b, np.zeros_like(b), 17, TOL[dtype], 60)
    tr.assert_same_bits(x, xr)
    assert (info.iterations, info.reason) == (ir_["iterations"], ir_["reason"])
    tr.assert_same_bits(np.array([info.residual_sq]), np.array([ir_["residual_sq"]]))


def test_a_second_call_takes_no_new_device_memory():
    """The library keeps freed blocks in its cache, so an identical call is served from it: the driver's free memory is
    what it was after the first call."""
    import torch
    mat = banded(4099, np.float64)
    a = make("csr", mat)
    first = a.eigsh(3, "LA", 16, tol=1e-10, maxit=2)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    second = a.eigsh(3, "LA", 16, tol=1e-10, maxit=2)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free1
    tr.assert_same_bits(first[1], second[1])
    assert first[2].restarts == second[2].restarts == 2


def test_row_block_handles_are_refused(monkeypatch):
    """a handle held as row blocks (the limit lowered for the test) has no eigsh: SPAL_ERR_UNSUPPORTED, by its message"""
    import spal_synth as synth
    rp, ci, va = synth.banded_csr(2000, 2000, 4, 64, 3)
    monkeypatch.setenv("SPAL_CSR_PART_ENTRIES", "3000")
    big = sp.CsrMatrix(2000, 2000, rp, ci, va)
    assert big.device().describe()["kernel"] == "row_blocks"
    monkeypatch.delenv("SPAL_CSR_PART_ENTRIES")
    with pytest.raises(sp.SpalError, match=r"spal_csr_eigsh: an operand of more than 2\^32 - 65537 entries \(row blocks\)") as e:
        big.eigsh(2, ncv=8, maxit=3)
    assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED
    assert "eigsh" not in big.device().describe()
    th, rs = np.zeros(2), np.zeros(2)
    with pytest.raises(sp.SpalError, match="spal_csr_eigsh_dev: an operand of more than") as e:
        big.device().eigsh_dev(2, th, rs, 0, 2, ncv=8, maxit=3)
    assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED and not th.any()
