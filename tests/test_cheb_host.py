"""Host tests of the Chebyshev filter: the text itself (tests/cheb_ref.py) -- rowsum, the coefficients,
cheb_apply as a polynomial, gershgorin -- the discriminating inputs of filtered eigsh confirmed on the CPU text alone
(plain eigsh does not converge where the filtered text does), the names in the header, the library, the Rust binding and
the C++ mirror, and every refusal that needs no device.  No GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import cheb_ref as cr
from tests import eigsh_ref as er
from tests.test_eigsh_host import lib_jacobi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ([f"spal_{kind}_{what}_{form}{sfx}" for kind in ("csr", "csc") for what in ("cheb_apply", "eigsh_filtered")
          for form in ("", "dev_") for sfx in ("f64", "f32")] + ["spal_csr_gershgorin", "spal_csc_gershgorin"])
u = C.c_uint64
d = C.c_double


# ---- the text ------------------------------------------------------------------------------------------------------------

def random_csr(n, rng, dtype, density=0.3):
    dense = rng.standard_normal((n, n)) * (rng.random((n, n)) < density)
    return dense, er.dense_to_csr(dense, dtype)[1:]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_rowsum_is_the_sequential_sum_of_rounded_products(dtype):
    rng = np.random.default_rng(7)
    dense, (rowptr, colind, values) = random_csr(37, rng, dtype)
    y = rng.standard_normal(37).astype(dtype)
    got = cr.rowsum(rowptr, colind, values, y)
    for r in range(37):
        acc = dtype(0)
        for p in range(int(rowptr[r]), int(rowptr[r + 1])):
            acc = dtype(acc + dtype(values[p] * y[int(colind[p])]))
        assert acc.tobytes() == got[r].tobytes()
    # a row of -0.0 products stays +0.0 + -0.0 = +0.0; an empty row is +0.0
    z = cr.rowsum([0, 2, 2], [0, 1], np.array([-1.0, 0.0], dtype), np.array([0.0, -3.0], dtype))
    assert not np.signbit(z).any()


def test_csc_to_csr_orders_a_rows_entries_by_column():
    rng = np.random.default_rng(8)
    dense, (rowptr, colind, values) = random_csr(23, rng, np.float64)
    _, colptr, rowind, cvals = er.dense_to_csr(dense.T.copy(), np.float64)
    rp, ci, va = cr.csc_to_csr(23, colptr, rowind, cvals)
    assert np.array_equal(rp, rowptr) and np.array_equal(ci, colind) and np.array_equal(va, values)


@pytest.mark.parametrize("degree", [1, 2, 3, 8, 40])
def test_cheb_apply_is_the_scaled_chebyshev_polynomial(degree):
    """On a diagonal matrix t_d[r] = T_d((a_r - c) / e) / T_d((a0 - c) / e): 1 at a0, at most 1 / T_d(.) inside [lo, hi],
    monotone towards a0 outside.  The recurrence's rounding is a few eps per step: 1e-12 for d <= 40 is generous."""
    lo, hi, a0 = 0.5, 3.0, 4.0
    diag = np.concatenate([np.linspace(lo, hi, 21), np.linspace(hi, a0, 9)[1:]])
    n = diag.size
    csr = (np.arange(n + 1), np.arange(n), diag.copy())
    t = cr.cheb_apply(*csr, np.ones(n), degree, lo, hi, a0)
    c, e = (lo + hi) / 2, (hi - lo) / 2
    want = np.polynomial.chebyshev.chebval((diag - c) / e, [0] * degree + [1]) / np.polynomial.chebyshev.chebval((a0 - c) / e, [0] * degree + [1])
    assert np.abs(t - want).max() <= 1e-12
    assert t[-1] == pytest.approx(1.0, abs=1e-12) and np.all(np.diff(t[20:]) > 0)
    assert np.abs(t[:21]).max() <= 1.0 / np.polynomial.chebyshev.chebval((a0 - c) / e, [0] * degree + [1]) + 1e-12


def test_the_coefficients_stay_bounded_in_f32_at_every_degree():
    for lo, hi, a0 in ((0.0, 3.9, 4.0), (0.1, 4.0, 0.0), (-1e6, 1e6, 1.0000001e6)):
        alpha, beta, cT = cr.coefficients(256, lo, hi, a0, np.float32)
        assert alpha.dtype == np.float32 and np.all(np.isfinite(alpha)) and np.all(np.isfinite(beta)) and beta[0] == 0
        assert np.all(np.abs(beta) <= 1.0)                       # s_{i-1} s_i with |s_i| < 1
    assert cr.check_interval(0, 0, 1, 2) == "degree" and cr.check_interval(257, 0, 1, 2) == "degree"
    assert cr.check_interval(3, 0, np.inf, 2) == "not finite" and cr.check_interval(3, 1, 1, 2) == "lo >= hi"
    assert cr.check_interval(3, 0, 1, 1) == "a0 inside" and cr.check_interval(3, 0, 1, 0) == "a0 inside"
    assert cr.check_interval(3, 0, 1, -0.5) is None and cr.check_interval(256, 0, 1, 1.5) is None


def test_gershgorin_encloses_and_handles_rows_without_a_diagonal():
    rng = np.random.default_rng(9)
    dense = rng.standard_normal((30, 30))
    dense = dense + dense.T
    dense[4, 4] = dense[17, 17] = 0.0            # rows without a stored diagonal
    dense[9, :] = dense[:, 9] = 0.0              # an empty row
    lam = np.linalg.eigvalsh(dense)
    glo, ghi = cr.gershgorin(*er.dense_to_csr(dense, np.float64)[1:])
    off = np.abs(dense).sum(axis=1) - np.abs(np.diag(dense))
    assert glo <= lam[0] and lam[-1] <= ghi
    assert glo == pytest.approx((np.diag(dense) - off).min(), rel=1e-14) and ghi == pytest.approx((np.diag(dense) + off).max(), rel=1e-14)
    assert cr.gershgorin([0, 1, 2], [1, 0], np.array([2.0, -3.0], np.float32)) == (-3.0, 3.0)
    assert cr.gershgorin([0, 0], [], np.zeros(0)) == (0.0, 0.0)
    assert all(np.isnan(v) for v in cr.gershgorin([0, 1, 2], [0, 1], np.array([1.0, np.inf])))


# ---- the discriminating inputs, on the CPU text alone ---------------------------------------------------------------------
N, K, NCV, MAXIT = 400, 4, 20, 60
CASES = {"f64": (np.float64, 1e-10, 8, 1e-9), "f32": (np.float32, 1e-5, 16, 1e-4)}
GIVEN = {"LA": (0.0, 3.92), "SA": (0.08, 4.0)}     # Gershgorin gives [0, 4]: 2 % of its width off the wanted end


@functools.lru_cache(maxsize=None)
def laplacian(name):
    dtype = CASES[name][0]
    return cr.laplace_1d_csr(N, dtype), np.linalg.eigvalsh(2.0 * np.eye(N) - np.eye(N, k=1) - np.eye(N, k=-1))


@pytest.mark.parametrize("which", ["LA", "SA"])
@pytest.mark.parametrize("name", list(CASES))
def test_plain_eigsh_does_not_converge_on_the_clustered_ends(name, which):
    dtype, tol, _, _ = CASES[name]
    csr, _ = laplacian(name)
    r = er.eigsh(lambda v: cr.rowsum(*csr, v), N, dtype, K, which, NCV, tol, MAXIT, jacobi_fn=lib_jacobi)
    assert (r["reason"], r["restarts"]) == (1, MAXIT) and r["converged"] < K


@pytest.mark.parametrize("interval", ["auto", "given"])
@pytest.mark.parametrize("which", ["LA", "SA"])
@pytest.mark.parametrize("name", list(CASES))
def test_the_filtered_text_converges_where_plain_does_not(name, which, interval):
    """Measured on the committed text (sequential row sums, the Jacobi text), restarts / products of the filtered run:
    f64 d = 8:  LA auto 8 / 708 (after a warm-up of 5 / 60), LA given 9 / 776, SA auto 7 / 640, SA given 9 / 776;
    f32 d = 16: LA auto 3 / 720, LA given 3 / 720, SA auto 2 / 588, SA given 3 / 720."""
    dtype, tol, degree, close = CASES[name]
    csr, lam = laplacian(name)
    r = cr.eigsh_filtered(csr, dtype, K, which, NCV, tol, MAXIT, degree, None if interval == "auto" else GIVEN[which], jacobi_fn=lib_jacobi)
    print(name, which, interval, "restarts", r["restarts"], "products", r["products"], "warm", r["warm_restarts"], r["warm_products"])
    assert r["reason"] == 0 and r["converged"] == K and r["pairs"] == K and r["restarts"] <= 12
    assert (r["warm_restarts"], r["warm_products"]) == ((5, 20 + 5 * 8) if interval == "auto" else (0, 0))
    want = lam[::-1][:K] if which == "LA" else lam[:K]
    assert np.abs(r["theta"].astype(np.float64) - want).max() <= close
    assert np.all(r["resid"].astype(np.float64) <= tol * 4.0)
    x = r["X"].astype(np.float64)
    dense = 2.0 * np.eye(N) - np.eye(N, k=1) - np.eye(N, k=-1)
    true = np.linalg.norm(dense @ x - x * r["theta"].astype(np.float64), axis=0)
    assert np.all(true <= 2 * tol * 4.0)


@pytest.mark.parametrize("which", ["LA", "SA"])
@pytest.mark.parametrize("name", list(CASES))
def test_tol_zero_is_reached(name, which):
    """tol = 0 stands for 256 eps.  16 eps is NOT reached by the f64 LA case: its residuals stall at 66 eps * scale
    (5.9e-14 .. 1.2e-13 against scale = 4) after 60 restarts; the other three cases stall at 3 .. 33 eps * scale."""
    dtype, _, degree, _ = CASES[name]
    csr, _ = laplacian(name)
    r = cr.eigsh_filtered(csr, dtype, K, which, NCV, 0, MAXIT, degree, jacobi_fn=lib_jacobi)
    assert r["reason"] == 0 and np.all(r["resid"] <= 256 * np.finfo(dtype).eps * 4.0)


def test_exits_of_the_filtered_text():
    dm = np.arange(2.0, 14.0)
    csr = (np.arange(13), np.arange(12), dm)
    e0 = np.zeros(12)
    e0[0] = 1
    # the space is exhausted at jj = 1 < k: reason 3, one pair, converged = nk
    r = cr.eigsh_filtered(csr, np.float64, 2, "LA", 6, 1e-10, 5, 3, (0.0, 12.0), v0=e0)
    assert (r["reason"], r["pairs"], r["converged"], r["products"]) == (3, 1, 1, 3 + 1) and r["theta"].tolist() == [2.0]
    # a warm-up that converges is the call's result
    r = cr.eigsh_filtered(csr, np.float64, 2, "LA", 6, 1e-10, 50, 3, warmup=40)
    plain = er.eigsh(lambda v: dm * v, 12, np.float64, 2, "LA", 6, 1e-10, 40)
    assert r["reason"] == 0 and (r["lo"], r["hi"]) == (0.0, 0.0) and r["warm_restarts"] == r["restarts"] == plain["restarts"]
    assert r["theta"].tobytes() == plain["theta"].tobytes() and r["X"].tobytes() == plain["X"].tobytes()
    # maxit bounds the filtered restarts; the warm-up is min(warmup, maxit)
    lap, _ = laplacian("f64")
    for maxit in (0, 2):
        r = cr.eigsh_filtered(lap, np.float64, K, "LA", NCV, 1e-10, maxit, 8, jacobi_fn=lib_jacobi)
        steps = NCV + maxit * (NCV - er.keep_of(K, NCV))
        assert (r["reason"], r["restarts"], r["warm_restarts"]) == (1, maxit, maxit)
        assert r["products"] == steps * 8 + (maxit + 1) * K and r["warm_products"] == steps
    # a value that is not finite: reason 2, nothing written
    bad = (lap[0], lap[1], lap[2].copy())
    bad[2][7] = np.nan
    r = cr.eigsh_filtered(bad, np.float64, K, "LA", NCV, 1e-10, 5, 8)
    assert (r["reason"], r["pairs"], r["converged"]) == (2, 0, 0) and np.isnan(r["a0"])
    # a degenerate cut: a matrix whose Gershgorin interval is one point
    eye = (np.arange(13), np.arange(12), np.full(12, 3.0))
    r = cr.eigsh_filtered(eye, np.float64, 1, "LA", 4, 0.0, 0, 4, warmup=0, v0=np.arange(1.0, 13.0))
    assert (r["lo"], r["hi"]) == (0.0, 0.0) and r["warm_restarts"] == r["restarts"]


# ---- names and refusals -----------------------------------------------------------------------------------------------------

def test_names_are_declared_exported_and_bound():
    declared = _ffi.exported_names()
    lib = _ffi.lib()
    with open(os.path.join(ROOT, "rust_shim", "src", "ffi.rs")) as f:
        rust = f.read()
    for name in NAMES:
        assert name in declared
        assert getattr(lib, name).restype is C.c_int
        assert f"pub fn {name}(" in rust
    assert "pub struct spal_eigsh_filter_info" in rust
    with open(os.path.join(ROOT, "include", "spalinalg.hpp")) as f:
        hpp = f.read()
    assert hpp.count("FilteredEigenpairs<T> eigsh_filtered(") == 2 and hpp.count("std::vector<T> cheb_apply(") == 2
    assert hpp.count("std::pair<double, double> gershgorin()") == 2
    for cls in (sp.CsrMatrix, sp.CscMatrix):
        assert callable(cls.cheb_apply) and callable(cls.gershgorin)
    for cls in (sp.DeviceCsr, sp.DeviceCsc):
        assert callable(cls.cheb_apply) and callable(cls.cheb_apply_dev) and callable(cls.gershgorin)
    assert C.sizeof(sp.matrix._EigshFilterInfoC) == 88


def fake_handle(elem_size=0, nrows=0, ncols=0):
    """A block of zeros stands in for a handle; both handle types begin {int device, int elem_size, u64 nrows, u64 ncols}."""
    buf = C.create_string_buffer(1 << 16)
    C.c_int.from_buffer(buf, 4).value = elem_size
    u.from_buffer(buf, 8).value = nrows
    u.from_buffer(buf, 16).value = ncols
    return buf


@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("sfx,ct,dt", [("f64", _ffi.f64p, np.float64), ("f32", _ffi.f32p, np.float32)])
def test_cheb_apply_refuses_without_a_device(kind, sfx, ct, dt):
    lib = _ffi.lib()
    inv = _ffi.SPAL_ERR_INVALID_ARGUMENT
    host, devf = getattr(lib, f"spal_{kind}_cheb_apply_{sfx}"), getattr(lib, f"spal_{kind}_cheb_apply_dev_{sfx}")
    size = np.dtype(dt).itemsize
    good = fake_handle(size, 6, 6)
    x, out = np.full(12, 9, dt), np.full(6, 9, dt)
    p = lambda a, off=0: C.cast(a.ctypes.data + off * size, ct)                                  # noqa: E731

    def call(h=good, xp=p(x), op=p(out), xl=6, ol=6, degree=3, lo=0.0, hi=1.0, a0=2.0):
        return host(h, xp, u(xl), op, u(ol), u(degree), d(lo), d(hi), d(a0))

    def dcall(h=good, xp=p(x), op=p(out), xl=6, ol=6, degree=3, lo=0.0, hi=1.0, a0=2.0):
        return devf(h, xp, op, u(degree), d(lo), d(hi), d(a0), None)

    for f, who in ((call, f"spal_{kind}_cheb_apply:"), (dcall, f"spal_{kind}_cheb_apply_dev:")):
        def refused(text, status):
            msg = lib.spal_last_error().decode()
            assert status == inv and msg.startswith(who) and text in msg, (status, msg)

        refused("null argument", f(h=None))
        refused("null argument", f(xp=None))
        refused("null argument", f(op=None))
        refused("degree must be 1 .. 256", f(degree=0))
        refused("degree must be 1 .. 256", f(degree=257))
        for bad in (float("nan"), float("inf"), -float("inf")):
            refused("must be finite", f(lo=bad))
            refused("must be finite", f(hi=bad))
            refused("must be finite", f(a0=bad))
        refused("lo must be less than hi", f(lo=1.0, hi=1.0))
        refused("lo must be less than hi", f(lo=2.0, hi=1.0, a0=3.0))
        refused("a0 must lie outside", f(a0=0.5))
        refused("a0 must lie outside", f(a0=0.0))
        refused("a0 must lie outside", f(a0=1.0))
        refused("handle holds", f(h=fake_handle(12 - size, 6, 6)))
        refused("not square (6 x 7)", f(h=fake_handle(size, 6, 7)))
        refused("out overlaps x", f(op=p(x)))
        refused("out overlaps x", f(op=p(x, 5)))
        refused("out overlaps x", f(xp=p(x, 3), op=p(x)))
    assert host(good, p(x), u(5), p(out), u(6), u(3), d(0.0), d(1.0), d(2.0)) == inv and b"x.len() = 5" in lib.spal_last_error()
    assert host(good, p(x), u(6), p(out), u(7), u(3), d(0.0), d(1.0), d(2.0)) == inv and b"out.len() = 7" in lib.spal_last_error()
    assert np.all(x == 9) and np.all(out == 9)
    g = getattr(lib, f"spal_{kind}_gershgorin")
    two = (d * 2)()
    assert g(None, two, two) == inv and g(good, None, two) == inv and g(good, two, None) == inv
    assert g(fake_handle(size, 6, 7), two, two) == inv and b"not square" in lib.spal_last_error()
    assert g(fake_handle(size, 0, 0), two, two) == inv and b"no rows" in lib.spal_last_error()


@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("sfx,ct,dt", [("f64", _ffi.f64p, np.float64), ("f32", _ffi.f32p, np.float32)])
def test_eigsh_filtered_refuses_without_a_device(kind, sfx, ct, dt):
    lib = _ffi.lib()
    inv = _ffi.SPAL_ERR_INVALID_ARGUMENT
    host, devf = getattr(lib, f"spal_{kind}_eigsh_filtered_{sfx}"), getattr(lib, f"spal_{kind}_eigsh_filtered_dev_{sfx}")
    size = np.dtype(dt).itemsize
    good = fake_handle(size, 12, 12)
    theta, resid, x = np.full(4, 9, dt), np.full(4, 9, dt), np.full((12, 4), 9, dt)
    info = sp.matrix._EigshFilterInfoC()
    p = lambda a: a.ctypes.data_as(ct)                                                       # noqa: E731

    def call(h=good, k=2, which=0, ncv=8, tol=1e-8, degree=8, auto=1, lo=0.0, hi=1.0, th=p(theta), rs=p(resid), ldx=4, inf=C.byref(info)):
        return host(h, u(k), C.c_int(which), u(ncv), None, u(0), u(0), d(tol), u(3), u(degree), C.c_int(auto), d(lo), d(hi), u(5),
                    th, u(k), rs, u(k), p(x), u(ldx), u(12), inf)

    def dcall(h=good, k=2, which=0, ncv=8, tol=1e-8, degree=8, auto=1, lo=0.0, hi=1.0, th=p(theta), rs=p(resid), ldx=4, inf=C.byref(info)):
        return devf(h, u(k), C.c_int(which), u(ncv), None, u(0), d(tol), u(3), u(degree), C.c_int(auto), d(lo), d(hi), u(5), th, rs,
                    p(x), u(ldx), None, inf)

    for f, who in ((call, f"spal_{kind}_eigsh_filtered:"), (dcall, f"spal_{kind}_eigsh_filtered_dev:")):
        def refused(text, status):
            msg = lib.spal_last_error().decode()
            assert status == inv and msg.startswith(who) and text in msg, (status, msg)

        refused("null argument", f(h=None))
        refused("null argument", f(th=None))
        refused("null argument", f(rs=None))
        refused("null argument", f(inf=None))
        refused("degree = 0 must be 1 .. 256", f(degree=0))
        refused("degree = 257 must be 1 .. 256", f(degree=257))
        refused("auto = 2 must be 0 or 1", f(auto=2))
        refused("must be finite with lo < hi", f(auto=0, lo=1.0, hi=1.0))
        refused("must be finite with lo < hi", f(auto=0, lo=float("nan")))
        refused("must be finite with lo < hi", f(auto=0, hi=float("inf")))
        refused("k = 0", f(k=0))
        refused("ncv = 2 must be greater than k = 2", f(ncv=2))
        refused("ncv = 257 must be at most 256", f(ncv=257))
        refused("which = 2 must be 0 (LA) or 1 (SA)", f(which=2))
        refused("must be finite and >= 0", f(tol=-1e-3))
        refused("ldx = 1 is less than k = 2", f(ldx=1))
        refused("handle holds", f(h=fake_handle(12 - size, 12, 12)))
        refused("not square (12 x 13)", f(h=fake_handle(size, 12, 13)))
        refused("ncv = 8 exceeds the matrix's 6 rows", f(h=fake_handle(size, 6, 6)))
    assert np.all(theta == 9) and np.all(resid == 9) and np.all(x == 9)


def test_python_refuses_before_any_device_copy():
    a = sp.CsrMatrix(3, 3, [0, 1, 2, 3], [0, 1, 2], np.ones(3))
    wide = sp.CsrMatrix(3, 4, [0, 1, 2, 3], [0, 1, 3], np.ones(3))
    c = sp.CscMatrix(3, 3, [0, 1, 2, 3], [0, 1, 2], np.ones(3, dtype=np.float32))
    with pytest.raises(sp.Panic, match=r"not square \(3 x 4\)"):
        wide.cheb_apply(np.ones(4), 2, 0.0, 1.0, 2.0)
    with pytest.raises(sp.Panic, match=r"not square \(3 x 4\)"):
        wide.gershgorin()
    for m in (a, c):
        with pytest.raises(sp.Panic, match="degree = 0 must be 1 .. 256"):
            m.cheb_apply(np.ones(3), 0, 0.0, 1.0, 2.0)
        with pytest.raises(sp.Panic, match="degree = 257 must be 1 .. 256"):
            m.cheb_apply(np.ones(3), 257, 0.0, 1.0, 2.0)
        with pytest.raises(sp.Panic, match="must be finite"):
            m.cheb_apply(np.ones(3), 2, 0.0, np.inf, 2.0)
        with pytest.raises(sp.Panic, match="must be less than hi"):
            m.cheb_apply(np.ones(3), 2, 1.0, 1.0, 2.0)
        with pytest.raises(sp.Panic, match="must lie outside"):
            m.cheb_apply(np.ones(3), 2, 0.0, 1.0, 1.0)
        with pytest.raises(sp.Panic, match="x has shape"):
            m.cheb_apply(np.ones(4), 2, 0.0, 1.0, 2.0)
        with pytest.raises(sp.Panic, match="filter_degree = 300 must be 0"):
            m.eigsh(1, ncv=2, filter_degree=300)
        with pytest.raises(sp.Panic, match="filter_degree = -1 must be 0"):
            m.eigsh(1, ncv=2, filter_degree=-1)
        with pytest.raises(sp.Panic, match="filter_interval"):
            m.eigsh(1, ncv=2, filter_degree=4, filter_interval=(1.0, 1.0))
        with pytest.raises(sp.Panic, match="filter_warmup = -1"):
            m.eigsh(1, ncv=2, filter_degree=4, filter_warmup=-1)
        with pytest.raises(sp.Panic, match="ncv = 3 must be greater than k = 6"):
            m.eigsh(filter_degree=4)                               # eigsh's own refusals come first
    assert sp.matrix._filter_args(8, None, 5) == (8, 1, 0.0, 0.0, 5) and sp.matrix._filter_args(8, (1, 2.5), 0) == (8, 0, 1.0, 2.5, 0)
