"""The Chebyshev filter on the device against its sequential text (tests/cheb_ref.py): cheb_apply, gershgorin and filtered
eigsh return the text's raw bits, f64 and f32, CSR and CSC; the claim the feature exists for (plain eigsh stops at maxit on
the clustered ends of the 1-D Laplacian, the filtered call converges, and its pairs hold up in float64); and the edges of
the driver.

The step kernel gives a workgroup 256 consecutive rows and walks their entries in chunks of 16 KiB of products (2048 f64,
4096 f32 entries; option "cheb_chunk" moves the boundaries).  The matrices below are the smallest that put rows, empty
rows and whole workgroups on every side of those two sizes; they need not be symmetric."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import cheb_ref as cr
from tests import eigsh_ref as er
from tests import gmres_ref as gr
from tests import ilu_ref as ir
from tests import trsv_ref as tr
from tests.test_gpu_eigsh import banded, lib_jacobi, named

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
ROWS = 256                                     # rows of a workgroup
DEGREES = (1, 2, 3, 8)                         # both parities of the buffer rotation
INTERVAL = (-1.0, 1.0, 1.5)                    # lo, hi, a0: every row's |entries| sum to at most 1
DESCRIBE_KEYS = {"k", "which", "ncv", "keep", "degree", "interval", "lo", "hi", "a0", "glo", "ghi", "warm_restarts",
                 "warm_products", "restarts", "products", "converged", "reason", "polls", "chunk", "basis_bytes",
                 "residual_ms", "solve_ms"}
u = C.c_uint64
dbl = C.c_double


def sfx(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def from_rows(n, rows, dtype, rng):
    """rows: {row: sorted columns}; values uniform in (-1, 1) / the row's length, so that p(A) stays of order 1"""
    rowptr = np.zeros(n + 1, dtype=np.uint64)
    cols, vals = [], []
    for r in range(n):
        c = np.asarray(rows.get(r, ()), dtype=np.uint64)
        rowptr[r + 1] = rowptr[r] + c.size
        cols.append(c)
        vals.append(rng.uniform(-1, 1, c.size) / max(c.size, 1))
    return n, rowptr, np.concatenate(cols) if cols else np.zeros(0, np.uint64), np.concatenate(vals).astype(dtype)


def some(rng, n, count):
    return np.sort(rng.choice(n, size=min(count, n), replace=False))


@functools.lru_cache(maxsize=None)
def shape(name, dtype):
    """(n, rowptr, colind, values); shared, read-only"""
    rng = np.random.default_rng(zlib.crc32(f"cheb/{name}".encode()))
    if name == "one":
        mat = from_rows(1, {0: [0]}, dtype, rng)
    elif name == "one-empty":
        mat = from_rows(1, {}, dtype, rng)
    elif name == "empty-rows":                  # empty at the start, in the middle (across a workgroup's edge), at the end
        n = 3 * ROWS - 20
        mat = from_rows(n, {r: np.union1d(some(rng, n, 5), [r] if r % 3 == 0 else []).astype(np.int64)
                            for r in range(n) if 9 < r < 250 or 262 < r < n - 10}, dtype, rng)
    elif name in ("rows-1", "rows", "rows+1"):  # the last workgroup has 255 rows, is full, has one row
        n = ROWS + {"rows-1": -1, "rows": 0, "rows+1": 1}[name]
        mat = from_rows(n, {r: some(rng, n, 1 + r % 7) for r in range(n)}, dtype, rng)
    elif name == "straddle":                    # 20 entries per row: 5120 per workgroup, over both default chunks
        n = 2 * ROWS + 77
        mat = from_rows(n, {r: some(rng, n, 20) for r in range(n)}, dtype, rng)
    elif name == "long-row":                    # one row longer than any chunk (5000 entries), beside short rows
        n = 5000
        rows = {r: some(rng, n, 2) for r in range(n)}
        rows[2500] = np.arange(n)
        mat = from_rows(n, rows, dtype, rng)
    elif name == "one-row":                     # all entries in one row
        n = 3000
        mat = from_rows(n, {1234: np.arange(n)}, dtype, rng)
    elif name == "negative-zeros":              # rows whose products are all -0.0, beside ordinary rows
        n = 300
        mat = from_rows(n, {r: some(rng, n, 4) for r in range(n)}, dtype, rng)
    elif name == "nan-inf":
        n = 2 * ROWS + 3
        mat = list(from_rows(n, {r: some(rng, n, 3) for r in range(n)}, dtype, rng))
        mat[3][int(mat[1][40])] = np.nan        # the first entry of row 40
        mat[3][int(mat[1][400])] = np.inf       # ... and of row 400
        mat = tuple(mat)
    else:
        raise KeyError(name)
    for a in mat[1:]:
        a.setflags(write=False)
    return mat


SHAPES = ["one", "one-empty", "empty-rows", "rows-1", "rows", "rows+1", "straddle", "long-row", "one-row", "negative-zeros",
          "nan-inf"]


def start(name, n, dtype, mat):
    rng = np.random.default_rng(n)
    x = rng.uniform(-1, 1, n).astype(dtype)
    if name == "negative-zeros":                # rows 0 .. 49: negative values times +0.0
        _, rowptr, colind, values = mat
        for r in range(50):
            p = slice(int(rowptr[r]), int(rowptr[r + 1]))
            x[colind[p].astype(np.int64)] = 0.0
    return x


def make(kind, mat):
    n, rowptr, colind, values = mat
    if kind == "csr":
        return sp.CsrMatrix(n, n, rowptr, colind, values)
    colptr, rowind, vals, _ = ir.to_csc((n, rowptr, colind), values)
    return sp.CscMatrix(n, n, colptr, rowind, vals)


# ---- 1. cheb_apply ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("name", SHAPES)
def test_cheb_apply_is_the_text(name, kind, dtype):
    mat = shape(name, dtype)
    n = mat[0]
    if name == "negative-zeros":
        values = -np.abs(mat[3])
        mat = (n, mat[1], mat[2], values)
    a = make(kind, mat)
    x = start(name, n, dtype, mat)
    lo, hi, a0 = INTERVAL
    for degree in DEGREES:
        got = a.cheb_apply(x, degree, lo, hi, a0)
        want = cr.cheb_apply(mat[1], mat[2], mat[3], x, degree, lo, hi, a0)
        tr.assert_same_bits(got, want)
    if name == "negative-zeros":                # t_1 of those rows is alpha * (+0.0 - cT * x[r]): the sum itself is +0.0
        q = cr.rowsum(mat[1], mat[2], mat[3], x)
        assert np.all(q[:50] == 0) and not np.signbit(q[:50]).any()
    if name == "nan-inf":                       # one step: exactly the two rows; the text says where they go from there
        t1 = a.cheb_apply(x, 1, lo, hi, a0)
        assert np.flatnonzero(~np.isfinite(t1)).tolist() == [40, 400] and np.isnan(t1[40]) and np.isinf(t1[400])
        assert np.isnan(got).sum() > 2


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["straddle", "long-row", "empty-rows"])
def test_the_chunk_does_not_change_the_bits(name, dtype):
    mat = shape(name, dtype)
    a = make("csr", mat)
    dev = a.device()
    x = start(name, mat[0], dtype, mat)
    want = cr.cheb_apply(mat[1], mat[2], mat[3], x, 3, *INTERVAL)
    for chunk in (256, 512, 1024, 2048, 4096, 0):
        dev.set_option("cheb_chunk", chunk)
        tr.assert_same_bits(a.cheb_apply(x, 3, *INTERVAL), want)
    with pytest.raises(sp.Panic, match="cheb_chunk must be 0"):
        dev.set_option("cheb_chunk", 300)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_the_device_form_with_offsets_and_a_stream(kind, dtype):
    import torch
    mat = shape("straddle", dtype)
    n = mat[0]
    dev = make(kind, mat).device()
    x = start("straddle", n, dtype, mat)
    tt = torch.float64 if dtype == np.float64 else torch.float32
    xin = torch.full((n + 37,), 7, dtype=tt, device="cuda")
    xin[5:5 + n] = torch.from_numpy(x).cuda()
    out = torch.full((n + 11,), 7, dtype=tt, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    size = np.dtype(dtype).itemsize
    for degree in DEGREES:
        dev.cheb_apply_dev(xin.data_ptr() + 5 * size, out.data_ptr() + 3 * size, degree, *INTERVAL, stream=s)
        s.synchronize()
        got = out.cpu().numpy()
        tr.assert_same_bits(got[3:3 + n], cr.cheb_apply(mat[1], mat[2], mat[3], x, degree, *INTERVAL))
        assert np.all(got[:3] == 7) and np.all(got[3 + n:] == 7)
    back = xin.cpu().numpy()
    assert np.all(back[:5] == 7) and np.all(back[5 + n:] == 7) and np.array_equal(back[5:5 + n], x)      # x is only read
    with pytest.raises(sp.Panic, match="out overlaps x"):
        dev.cheb_apply_dev(xin.data_ptr(), xin.data_ptr() + 8 * size, 2, *INTERVAL)


# ---- 2. gershgorin ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("name", ["one", "one-empty", "empty-rows", "rows+1", "long-row", "one-row", "nan-inf"])
def test_gershgorin_is_the_text(name, kind, dtype):
    mat = shape(name, dtype)                    # random columns: most rows store no diagonal
    got = make(kind, mat).gershgorin()
    want = cr.gershgorin(*mat[1:])
    if name == "nan-inf":
        assert all(np.isnan(v) for v in got) and all(np.isnan(v) for v in want)
    else:
        assert got == (float(want[0]), float(want[1]))
    if name == "empty-rows":
        rows = np.repeat(np.arange(mat[0]), np.diff(mat[1].astype(np.int64)))
        assert mat[0] // 4 < np.count_nonzero(rows == mat[2].astype(np.int64)) < mat[0] // 2     # a third of the rows store theirs


# ---- 3. filtered eigsh: the text's bits, and the claim ---------------------------------------------------------------------
N, K, NCV, MAXIT = 400, 4, 20, 60
CASES = {np.float64: (1e-10, 8), np.float32: (1e-5, 16)}
GIVEN = {"LA": (0.0, 3.92), "SA": (0.08, 4.0)}


@functools.lru_cache(maxsize=None)
def laplacian(dtype):
    rowptr, colind, values = cr.laplace_1d_csr(N, dtype)
    for a in (rowptr, colind, values):
        a.setflags(write=False)
    return N, rowptr, colind, values


def check(a, mat, dtype, k, which, ncv, tol, maxit, degree, interval=None, warmup=5, v0=None, seed=0):
    """One filtered call against the text: the warm-up on the device's own product, as eigsh's tests run the plain text,
    the filtered phases on the text's rowsum."""
    dev = a.device()
    theta, X, info = a.eigsh(k, which, ncv, v0, seed, tol, maxit, filter_degree=degree, filter_interval=interval, filter_warmup=warmup)
    ref = cr.eigsh_filtered(mat[1:], dtype, k, which, ncv, tol, maxit, degree, interval, warmup, v0, seed, lib_jacobi,
                            mul_plain=lambda v: dev.spmv(v))
    assert (info.restarts, info.products, info.converged, info.reason, info.warm_restarts, info.warm_products, info.degree) == \
        (ref["restarts"], ref["products"], ref["converged"], ref["reason"], ref["warm_restarts"], ref["warm_products"], degree)
    assert (info.lo, info.hi) == (ref["lo"], ref["hi"]) and (info.a0 == ref["a0"] or (np.isnan(info.a0) and np.isnan(ref["a0"])))
    tr.assert_same_bits(theta, ref["theta"])
    tr.assert_same_bits(info.resid, ref["resid"])
    tr.assert_same_bits(X, ref["X"])
    d = dev.describe()["eigsh_filter"]
    assert set(d) == DESCRIBE_KEYS
    assert (d["k"], d["which"], d["ncv"], d["degree"], d["interval"]) == (k, which, ncv, degree, "auto" if interval is None else "given")
    assert (d["restarts"], d["products"], d["reason"], d["lo"], d["hi"]) == (info.restarts, info.products, info.reason, info.lo, info.hi)
    return (theta, X, info), ref


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("interval", ["auto", "given"])
@pytest.mark.parametrize("which", ["LA", "SA"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_filtered_eigsh_is_the_text_and_converges(kind, which, interval, dtype):
    tol, degree = CASES[dtype]
    mat = laplacian(dtype)
    (theta, X, info), _ = check(make(kind, mat), mat, dtype, K, which, NCV, tol, MAXIT, degree, None if interval == "auto" else GIVEN[which])
    assert info.reason == 0 and info.converged == K and info.restarts <= 12
    assert (info.warm_restarts, info.warm_products) == ((5, NCV + 5 * 8) if interval == "auto" else (0, 0))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["LA", "SA"])
def test_the_claim_plain_stops_at_maxit_and_the_filtered_call_converges(which, dtype):
    """The filtered call's pairs, checked in float64: r = A x - theta x with the returned theta and X.

    The device accepted res_c <= tol * scale, res_c computed in T from the same theta and x.  What float64 can find beyond
    that is T's rounding in forming r: a row of the 1-D Laplacian is L = 3 products and L additions, so
    |fl(q_i) - q_i| <= (L + 1) eps (|A| |x|)_i; the product th * x_i and the subtraction add eps |th x_i| and eps |r_i|.
    With || |A| || <= scale (Gershgorin's bound holds for |A|) and |th| <= scale that is
        ||r64 - r_T|| <= eps * scale * ||x|| * (L + 1 + 1) + eps * ||r||,
    and the dot's tree and the square root make res_c itself wrong by a factor within 1 +- 13 eps (ten levels, the products,
    the root).  theta's own rounding needs no slack: both sides use the value that was returned."""
    tol, degree = CASES[dtype]
    mat = laplacian(dtype)
    a = make("csr", mat)
    _, _, plain = a.eigsh(K, which, NCV, tol=tol, maxit=MAXIT)
    assert plain.reason == 1 and plain.restarts == MAXIT and plain.converged < K
    theta, X, info = a.eigsh(K, which, NCV, tol=tol, maxit=MAXIT, filter_degree=degree)
    assert info.reason == 0 and info.converged == K and info.restarts < plain.restarts // 4
    glo, ghi = a.gershgorin()
    assert (glo, ghi) == (0.0, 4.0)
    scale, eps = 4.0, float(np.finfo(dtype).eps)
    dense = 2.0 * np.eye(N) - np.eye(N, k=1) - np.eye(N, k=-1)
    x64, th64 = X.astype(np.float64), theta.astype(np.float64)
    res64 = np.linalg.norm(dense @ x64 - x64 * th64, axis=0)
    slack = eps * scale * np.linalg.norm(x64, axis=0) * 5 + eps * res64
    print(which, sfx(dtype), "restarts", plain.restarts, "->", info.restarts, "res64 / (tol scale)", res64 / (tol * scale))
    assert np.all(res64 <= tol * scale * (1 + 13 * eps) + slack)
    assert np.all(info.resid.astype(np.float64) <= tol * scale)
    lam = np.linalg.eigvalsh(dense)
    want = lam[::-1][:K] if which == "LA" else lam[:K]
    assert np.abs(th64 - want).max() <= (1e-9 if dtype == np.float64 else 1e-4)


# ---- 4. the edges of the driver ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_filter_degree_0_is_todays_eigsh(dtype):
    mat = named("A1", dtype)
    n = mat[0]
    a = make("csr", mat)
    tol = CASES[dtype][0]
    t0, x0, i0 = a.eigsh(3, "SA", 12, tol=tol, maxit=4)
    t1, x1, i1 = a.eigsh(3, "SA", 12, tol=tol, maxit=4, filter_degree=0, filter_interval=(0.0, 1.0), filter_warmup=9)
    ref = er.eigsh(lambda v: a.device().spmv(v), n, dtype, 3, "SA", 12, tol, 4, jacobi_fn=lib_jacobi)
    for got in ((t0, x0, i0), (t1, x1, i1)):
        tr.assert_same_bits(got[0], ref["theta"])
        tr.assert_same_bits(got[1], ref["X"])
        tr.assert_same_bits(got[2].resid, ref["resid"])
        assert (got[2].restarts, got[2].products, got[2].reason) == (ref["restarts"], ref["products"], ref["reason"])
        assert "warm_restarts" not in got[2]
    assert "eigsh_filter" not in a.device().describe()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_warm_up_that_converges_is_the_result(dtype):
    mat = named("A1", dtype)
    a = make("csr", mat)
    tol = CASES[dtype][0]
    t0, x0, i0 = a.eigsh(4, "LA", 16, tol=tol, maxit=100)
    assert i0.reason == 0 and i0.restarts >= 1
    (theta, X, info), _ = check(a, mat, dtype, 4, "LA", 16, tol, 500, 8, warmup=100)
    tr.assert_same_bits(theta, t0)
    tr.assert_same_bits(X, x0)
    tr.assert_same_bits(info.resid, i0.resid)
    assert (info.reason, info.restarts, info.products) == (0, i0.restarts, i0.products)
    assert (info.warm_restarts, info.warm_products, info.lo, info.hi) == (i0.restarts, i0.products, 0.0, 0.0)


@pytest.mark.parametrize("maxit", [0, 2])
def test_maxit_bounds_the_filtered_restarts(maxit):
    mat = laplacian(np.float64)
    (theta, X, info), _ = check(make("csr", mat), mat, np.float64, K, "LA", NCV, 1e-10, maxit, 8)
    steps = NCV + maxit * (NCV - er.keep_of(K, NCV))
    assert (info.reason, info.restarts, info.warm_restarts) == (1, maxit, maxit) and theta.size == K
    assert (info.products, info.warm_products) == (steps * 8 + (maxit + 1) * K, steps)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_values_that_are_not_finite_stop_with_reason_2(dtype):
    tol, degree = CASES[dtype]
    mat = laplacian(dtype)
    values = mat[3].copy()
    values[7] = np.nan
    bad = (N, mat[1], mat[2], values)
    (theta, X, info), _ = check(make("csr", bad), bad, dtype, K, "LA", NCV, tol, 5, degree)        # Gershgorin sees it
    assert info.reason == 2 and theta.size == 0 and X.shape == (N, 0) and info.products == 0 and np.isnan(info.a0)
    d = make("csr", bad).device()
    d.eigsh(K, "LA", NCV, tol=tol, maxit=5, filter_degree=degree)
    d = d.describe()["eigsh_filter"]             # bounds that are not finite are null there
    assert (d["glo"], d["ghi"], d["a0"], d["reason"]) == (None, None, None, 2)
    v0 = np.ones(N, dtype=dtype)
    v0[5] = np.inf
    (theta, X, info), _ = check(make("csr", mat), mat, dtype, K, "SA", NCV, tol, 5, degree, GIVEN["SA"], v0=v0)   # the first step does
    assert info.reason == 2 and theta.size == 0 and info.converged == 0 and info.products == degree
    # through the C entry with a given interval: theta, resid and x are left as they were
    dev = make("csr", mat).device()
    ct = _ffi.f64p if dtype == np.float64 else _ffi.f32p
    th, rs, x = np.full(K, 9, dtype), np.full(K, 9, dtype), np.full((N, K), 9, dtype)
    cinfo = sp.matrix._EigshFilterInfoC()
    fn = getattr(_ffi.lib(), f"spal_csr_eigsh_filtered_{sfx(dtype)}")
    assert fn(dev._h, u(K), C.c_int(1), u(NCV), v0.ctypes.data_as(ct), u(N), u(0), dbl(tol), u(5), u(degree), C.c_int(0), dbl(0.08),
              dbl(4.0), u(5), th.ctypes.data_as(ct), u(K), rs.ctypes.data_as(ct), u(K), x.ctypes.data_as(ct), u(K), u(N),
              C.byref(cinfo)) == 0
    assert cinfo.reason == 2 and np.all(th == 9) and np.all(rs == 9) and np.all(x == 9)


def test_a_degenerate_cut_falls_back_to_the_warm_up():
    """3 I: Gershgorin's interval is the point 3, so no cut lies strictly inside it"""
    n = 12
    mat = (n, np.arange(n + 1, dtype=np.uint64), np.arange(n, dtype=np.uint64), np.full(n, 3.0))
    a = make("csr", mat)
    v0 = np.arange(1.0, n + 1.0)
    (theta, X, info), ref = check(a, mat, np.float64, 1, "LA", 4, 0.0, 0, 4, warmup=0, v0=v0)
    assert a.gershgorin() == (3.0, 3.0)
    assert (info.lo, info.hi, info.a0) == (0.0, 0.0, 3.0) and info.warm_restarts == info.restarts and info.warm_products == info.products


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_chunk_rotation_form_and_ldx_do_not_change_the_bits(dtype):
    import torch
    tol, degree = CASES[dtype]
    mat = laplacian(dtype)
    a = make("csr", mat)
    want_theta, want_x, want = a.eigsh(K, "LA", NCV, tol=tol, maxit=2, filter_degree=degree, filter_interval=GIVEN["LA"])
    assert want.restarts == 2 and want.reason == 1
    for chunk, rotate in ((256, 0), (4096, 1), (0, 2)):
        b = make("csr", mat)
        b.device().set_option("cheb_chunk", chunk)
        b.device().set_option("eigsh_rotate", rotate)
        theta, X, info = b.eigsh(K, "LA", NCV, tol=tol, maxit=2, filter_degree=degree, filter_interval=GIVEN["LA"])
        tr.assert_same_bits(theta, want_theta)
        tr.assert_same_bits(X, want_x)
        tr.assert_same_bits(info.resid, want.resid)
        assert b.device().describe()["eigsh_filter"]["chunk"] == chunk
    # values only; then device pointers, a stream of the caller's, ldx > k
    theta, X, info = a.eigsh(K, "LA", NCV, tol=tol, maxit=2, filter_degree=degree, filter_interval=GIVEN["LA"], return_eigenvectors=False)
    assert X is None
    tr.assert_same_bits(theta, want_theta)
    xt = torch.full((N, K + 1), 7, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    th, rs = np.zeros(K, dtype), np.zeros(K, dtype)
    info2 = a.device().eigsh_dev(K, th, rs, xt.data_ptr(), K + 1, which="LA", ncv=NCV, tol=tol, maxit=2, stream=s, filter_degree=degree,
                                 filter_interval=GIVEN["LA"])
    got = xt.cpu().numpy()                      # the call has synchronised its stream
    tr.assert_same_bits(got[:, :K], want_x)
    assert np.all(got[:, K] == 7) and (info2.restarts, info2.reason, info2.products) == (want.restarts, want.reason, want.products)
    tr.assert_same_bits(th, want_theta)
    tr.assert_same_bits(rs, want.resid)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_workspace_and_the_polls_of_both_rotation_forms(dtype):
    """n = 257, so the vectors' stride (320) is not n.  The block holds the basis (ncv + 1 vectors), w, the recurrence's
    work vector and, for the out-of-place rotation, a second basis.  A given interval: no warm-up, and every phase polls
    twice, for the head and for the true pairs."""
    n, k, ncv = 257, 3, 9
    tol, degree = CASES[dtype]
    mat = (n, *cr.laplace_1d_csr(n, dtype))
    got = {}
    for rotate in (1, 2):
        a = make("csr", mat)
        a.device().set_option("eigsh_rotate", rotate)
        got[rotate], _ = check(a, mat, dtype, k, "LA", ncv, tol, 2, degree, GIVEN["LA"])
        info = got[rotate][2]
        d = a.device().describe()["eigsh_filter"]
        print(sfx(dtype), "rotate", rotate, "basis_bytes", d["basis_bytes"], "polls", d["polls"], "restarts", info.restarts,
              "reason", info.reason)
        nvec = (ncv + 1) + 2 + (ncv + 1 if rotate == 1 else 0)
        assert d["basis_bytes"] == nvec * 320 * np.dtype(dtype).itemsize
        assert info.reason in (0, 1, 3) and d["polls"] == 2 * (info.restarts + 1)
        assert (info.warm_restarts, info.warm_products) == (0, 0)
    (t1, x1, i1), (t2, x2, i2) = got[1], got[2]
    tr.assert_same_bits(t1, t2)
    tr.assert_same_bits(x1, x2)
    tr.assert_same_bits(i1.resid, i2.resid)
    assert (i1.restarts, i1.products, i1.converged, i1.reason, i1.lo, i1.hi, i1.a0) == \
        (i2.restarts, i2.products, i2.converged, i2.reason, i2.lo, i2.hi, i2.a0)


def test_a_second_call_takes_no_new_device_memory():
    import torch
    mat = banded(4099, np.float64)
    a = make("csr", mat)
    first = a.eigsh(3, "LA", 16, tol=1e-10, maxit=2, filter_degree=4, filter_warmup=1)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    second = a.eigsh(3, "LA", 16, tol=1e-10, maxit=2, filter_degree=4, filter_warmup=1)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free1
    tr.assert_same_bits(first[1], second[1])
    assert first[2].restarts == second[2].restarts and first[2].warm_restarts == 1


@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_refusals_that_read_the_handle_and_a_capturing_stream(kind):
    import torch
    lib = _ffi.lib()
    mat = laplacian(np.float64)
    a = make(kind, mat)
    dev = a.device()
    inv = _ffi.SPAL_ERR_INVALID_ARGUMENT
    # the place of a0 needs Gershgorin's bounds: [0, 4] here
    with pytest.raises(sp.Panic, match=r"a0 = 4 \(Gershgorin's upper bound\) must lie strictly above the interval \[0, 5\]"):
        a.eigsh(K, "LA", NCV, filter_degree=8, filter_interval=(0.0, 5.0))
    with pytest.raises(sp.Panic, match="must lie strictly above"):
        a.eigsh(K, "LA", NCV, filter_degree=8, filter_interval=(0.0, 4.0))
    with pytest.raises(sp.Panic, match=r"a0 = 0 \(Gershgorin's lower bound\) must lie strictly below"):
        a.eigsh(K, "SA", NCV, filter_degree=8, filter_interval=(-1.0, 4.0))
    x32, out32 = np.ones(N, np.float32), np.zeros(N, np.float32)
    assert getattr(lib, f"spal_{kind}_cheb_apply_f32")(dev._h, x32.ctypes.data_as(_ffi.f32p), u(N), out32.ctypes.data_as(_ffi.f32p), u(N),
                                                       u(2), dbl(0.0), dbl(1.0), dbl(2.0)) == inv
    assert "handle holds f64 values" in lib.spal_last_error().decode() and not out32.any()
    wide = sp.CsrMatrix(3, 4, [0, 1, 2, 3], [0, 1, 3], np.ones(3)) if kind == "csr" else sp.CscMatrix(3, 4, [0, 1, 2, 2, 3], [0, 1, 2], np.ones(3))
    with pytest.raises(sp.Panic, match=r"not square \(3 x 4\)"):
        wide.device().gershgorin()
    p = lambda v: v.ctypes.data_as(_ffi.f64p)                                                  # noqa: E731
    th, rs = np.zeros(K), np.zeros(K)
    xt = torch.zeros((N, K), dtype=torch.float64, device="cuda")
    vin = torch.ones(N, dtype=torch.float64, device="cuda")
    cinfo = sp.matrix._EigshFilterInfoC()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()               # never replayed
    with torch.cuda.graph(graph):
        xt.fill_(0.0)                            # (so that the graph is not empty)
        capturing = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        s1 = getattr(lib, f"spal_{kind}_eigsh_filtered_dev_f64")(dev._h, u(K), C.c_int(0), u(NCV), None, u(0), dbl(1e-8), u(3), u(8),
                                                                 C.c_int(1), dbl(0.0), dbl(0.0), u(5), p(th), p(rs),
                                                                 C.c_void_p(xt.data_ptr()), u(K), capturing, C.byref(cinfo))
        m1 = lib.spal_last_error().decode()
        s2 = getattr(lib, f"spal_{kind}_cheb_apply_dev_f64")(dev._h, C.c_void_p(vin.data_ptr()), C.c_void_p(xt.data_ptr()), u(3),
                                                             dbl(0.0), dbl(1.0), dbl(2.0), capturing)
        m2 = lib.spal_last_error().decode()
    torch.cuda.synchronize()
    assert s1 == inv and "cannot be captured into a graph" in m1, (s1, m1)
    assert s2 == inv and "cannot be captured into a graph" in m2, (s2, m2)
    del graph
    assert not th.any()


def test_row_block_handles_are_refused(monkeypatch):
    import spal_synth as synth
    rp, ci, va = synth.banded_csr(2000, 2000, 4, 64, 3)
    monkeypatch.setenv("SPAL_CSR_PART_ENTRIES", "3000")
    big = sp.CsrMatrix(2000, 2000, rp, ci, va)
    assert big.device().describe()["kernel"] == "row_blocks"
    monkeypatch.delenv("SPAL_CSR_PART_ENTRIES")
    for call, who in ((lambda: big.eigsh(2, ncv=8, maxit=3, filter_degree=4), "spal_csr_eigsh_filtered"),
                      (lambda: big.cheb_apply(np.ones(2000), 2, 0.0, 1.0, 2.0), "spal_csr_cheb_apply"),
                      (lambda: big.gershgorin(), "spal_csr_gershgorin")):
        with pytest.raises(sp.SpalError, match=who + r": an operand of more than 2\^32 - 65537 entries \(row blocks\)") as e:
            call()
        assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED
    assert "eigsh_filter" not in big.device().describe()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gmres_and_eigsh_still_return_their_texts_after_a_filtered_call(dtype):
    mat = banded(1025, dtype)
    n = mat[0]
    a = make("csr", mat)
    tol = CASES[dtype][0]
    _, _, finfo = a.eigsh(2, "LA", 12, tol=tol, maxit=2, filter_degree=4, filter_warmup=1)
    assert finfo.degree == 4 and "eigsh_filter" in a.device().describe()
    b = np.random.default_rng(3).uniform(-1, 1, size=n).astype(dtype)
    x, info = a.gmres(b, restart=17, tol=tol, maxit=60)
    xr, ir_ = gr.gmres(lambda v: a.device().spmv(v), None, b, np.zeros_like(b), 17, tol, 60)
    tr.assert_same_bits(x, xr)
    assert (info.iterations, info.reason) == (ir_["iterations"], ir_["reason"])
    theta, X, einfo = a.eigsh(2, "LA", 12, tol=tol, maxit=3)
    ref = er.eigsh(lambda v: a.device().spmv(v), n, dtype, 2, "LA", 12, tol, 3, jacobi_fn=lib_jacobi)
    tr.assert_same_bits(theta, ref["theta"])
    tr.assert_same_bits(X, ref["X"])
    assert (einfo.restarts, einfo.products, einfo.reason) == (ref["restarts"], ref["products"], ref["reason"])
