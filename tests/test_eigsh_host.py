"""Host tests of eigsh: the Jacobi text (tests/eigsh_ref.jacobi and the library's spal_eigsh_jacobi, bit for bit the
same) against numpy.linalg.eigvalsh, the effectiveness of the whole text (tests/eigsh_ref.eigsh) on two matrices, the
documented behaviour on a multiple eigenvalue, the names in the header, the library and the Rust binding, and the refusals
that need no device.  No GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import eigsh_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
NAMES = ["spal_eigsh_jacobi"] + [f"spal_{kind}_eigsh_{form}{sfx}" for kind in ("csr", "csc") for form in ("", "dev_")
                                 for sfx in ("f64", "f32")]
u = C.c_uint64


def lib_jacobi(S):
    S = np.ascontiguousarray(S, dtype=np.float64)
    m = S.shape[0]
    theta, Y, sweeps = np.zeros(m), np.zeros((m, m)), u()
    status = _ffi.lib().spal_eigsh_jacobi(u(m), S.ctypes.data_as(_ffi.f64p), theta.ctypes.data_as(_ffi.f64p),
                                          Y.ctypes.data_as(_ffi.f64p), C.byref(sweeps))
    assert status == 0, _ffi.lib().spal_last_error()
    return theta, Y, sweeps.value


def jacobi_cases():
    rng = np.random.default_rng(20261020)
    for m in (1, 2, 9, 24):
        yield f"diagonal-{m}", np.diag(rng.uniform(-3, 3, m))
        a = rng.standard_normal((m, m))
        yield f"random-{m}", a + a.T
        a = rng.standard_normal((m, m))
        a = a + a.T
        a[m // 2, :] = 0
        a[:, m // 2] = 0
        yield f"zero-row-{m}", a
        a = rng.standard_normal((m, m))
        yield f"huge-{m}", (a + a.T) * 1e150                       # theta * theta overflows nowhere it matters
        if m > 1:
            t = np.diag(rng.uniform(0, 4, m)) + np.diag(rng.uniform(-1, 1, m - 1), 1)
            yield f"tridiagonal-{m}", t + np.triu(t, 1).T
    yield "equal-diagonal-2", np.array([[2.0, 1.0], [1.0, 2.0]])
    yield "zero-9", np.zeros((9, 9))


JACOBI = dict(jacobi_cases())


@pytest.mark.parametrize("name", list(JACOBI))
def test_jacobi_against_eigvalsh(name):
    """Measured on the committed text over these cases: max |S Y - Y diag(theta)| = 3.86 eps ||S||_2, the largest error of
    an eigenvalue against eigvalsh 7.07 eps ||S||_2, |Y^T Y - I| <= 38 eps (order 24).  Asserted: twice that -- a second
    correct implementation of cyclic Jacobi may differ by a rounding or two per rotation."""
    S = JACOBI[name]
    m = S.shape[0]
    theta, Y, sweeps = er.jacobi(S)
    t2, Y2, s2 = lib_jacobi(S)
    assert theta.tobytes() == t2.tobytes() and Y.tobytes() == Y2.tobytes() and sweeps == s2     # one text, two languages
    assert sweeps < 12
    norm = np.linalg.norm(S, 2)
    print(name, "sweeps", sweeps, "residual / (eps ||S||)", np.abs(S @ Y - Y * theta).max() / (EPS * norm) if norm else 0.0)
    assert np.abs(S @ Y - Y * theta).max() <= 2 * 3.86 * EPS * norm
    assert np.abs(np.sort(theta) - np.linalg.eigvalsh(S)).max() <= 2 * 7.07 * EPS * norm
    assert np.abs(Y.T @ Y - np.eye(m)).max() <= 2 * 38 * EPS
    if name.startswith("diagonal") or name == "zero-9":
        assert sweeps == 0 and np.array_equal(theta, np.diag(S)) and np.array_equal(Y, np.eye(m))
    if name == "equal-diagonal-2":
        assert sorted(theta.tolist()) == [1.0, 3.0]


def test_ritz_orders_and_keeps_ties_by_position():
    S = np.diag([2.0, 5.0, 2.0, -1.0])
    theta, Y, res = er.ritz(S, 0.5, er.LA, lib_jacobi)
    assert theta.tolist() == [5.0, 2.0, 2.0, -1.0] and np.array_equal(np.argmax(np.abs(Y), axis=0), [1, 0, 2, 3])
    theta, Y, res = er.ritz(S, 0.5, er.SA, lib_jacobi)
    assert theta.tolist() == [-1.0, 2.0, 2.0, 5.0] and np.array_equal(np.argmax(np.abs(Y), axis=0), [3, 0, 2, 1])
    assert res.tolist() == [0.5, 0.0, 0.0, 0.0]
    S[1, 2] = S[2, 1] = np.inf
    assert er.ritz(S, 0.5, er.LA) is None


@functools.lru_cache(maxsize=None)
def spectrum(name):
    dense = er.laplace_1d_plus() if name == "A1" else er.laplace_2d_plus()
    dense.setflags(write=False)
    return dense, np.linalg.eigvalsh(dense)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 1e-5)], ids=["f64", "f32"])
@pytest.mark.parametrize("which", ["LA", "SA"])
@pytest.mark.parametrize("k,ncv", [(1, 8), (3, 9), (4, 16), (6, 24)])
@pytest.mark.parametrize("name", ["A1", "A2"])
def test_the_text_finds_the_extreme_pairs(name, k, ncv, which, dtype, tol):
    """Measured on the committed text over the 32 cases: at most 79 restarts (A1, f64, k = 3, ncv = 9, SA), the largest
    true residual 0.932 of tol * max|lambda| (A1, f64, k = 1, ncv = 8, SA)."""
    dense, lam = spectrum(name)
    n = dense.shape[0]
    a = dense.astype(dtype)
    # the projected problems of the f32 cases go through the LIBRARY's Jacobi, those of the f64 cases through numpy's
    r = er.eigsh(lambda v: a @ v, n, dtype, k, which, ncv, tol, 100, jacobi_fn=lib_jacobi if dtype == np.float32 else None)
    assert r["reason"] == 0 and r["restarts"] <= 100 and r["converged"] == k and r["pairs"] == k
    assert r["theta"].dtype == dtype and r["X"].shape == (n, k)
    x, theta = r["X"].astype(np.float64), r["theta"].astype(np.float64)
    res = np.linalg.norm(dense @ x - x * theta, axis=0) / np.linalg.norm(x, axis=0)
    top = np.abs(lam).max()
    print(name, k, ncv, which, "restarts", r["restarts"], "residual / (tol max|lambda|)", (res / (tol * top)).max())
    assert np.all(res <= 2 * tol * top)
    want = lam[::-1][:k] if which == "LA" else lam[:k]
    assert np.all(np.abs(theta - want) <= res + 1e-12 * top)      # IN ORDER: a missed eigenvalue shows here


def test_a_double_eigenvalue_is_returned_once():
    """The plain 2-D Laplacian has double eigenvalues; a single-vector Lanczos iteration sees one direction of each
    eigenspace: the values returned are the DISTINCT extreme eigenvalues, one copy each."""
    dense = er.laplace_2d(13)
    lam = np.linalg.eigvalsh(dense)
    distinct = lam[::-1][np.concatenate([[True], np.diff(lam[::-1]) < -1e-9])]
    assert abs(lam[-2] - lam[-3]) < 1e-12 and distinct[1] - distinct[2] > 1e-3
    r = er.eigsh(lambda v: dense @ v, 169, np.float64, 3, "LA", 16, 1e-10, 100, jacobi_fn=lib_jacobi)
    assert r["reason"] == 0
    own = er.eigsh(lambda v: dense @ v, 169, np.float64, 3, "LA", 16, 1e-10, 100)       # numpy's Jacobi: the same bits
    assert own["restarts"] == r["restarts"] and own["theta"].tobytes() == r["theta"].tobytes() and own["X"].tobytes() == r["X"].tobytes()
    assert np.allclose(r["theta"], distinct[:3], rtol=0, atol=1e-8)
    assert not np.allclose(r["theta"], lam[::-1][:3], rtol=0, atol=1e-8)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [9, 1025, 4099])
def test_the_batched_gram_schmidt_pass_is_gmres_refs(n, dtype):
    from tests import gmres_ref as gr
    rng = np.random.default_rng(n)
    V = [rng.standard_normal(n).astype(dtype) for _ in range(5)]
    w = rng.standard_normal(n).astype(dtype)
    f1, w1 = gr._project(V, w, dtype)
    f2, w2 = er._project(V, w, dtype)
    assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(f1, f2)) and w1.tobytes() == w2.tobytes()


def test_exits_of_the_text():
    d = np.arange(2.0, 14.0)
    e0 = np.zeros(12)
    e0[0] = 1
    r = er.eigsh(lambda v: d * v, 12, np.float64, 2, "LA", 6, 1e-10, 5, v0=e0, jacobi_fn=lib_jacobi)
    assert (r["reason"], r["products"], r["pairs"], r["converged"]) == (3, 1, 1, 1) and r["theta"].tolist() == [2.0]
    r = er.eigsh(lambda v: d * v, 12, np.float64, 1, "SA", 6, 1e-10, 5, v0=e0)
    assert (r["reason"], r["products"], r["pairs"]) == (0, 1, 1) and np.array_equal(r["X"][:, 0], e0)
    bad = np.ones(12)
    bad[3] = np.nan
    r = er.eigsh(lambda v: d * v, 12, np.float64, 2, "LA", 6, 1e-10, 5, v0=bad)
    assert (r["reason"], r["pairs"], r["converged"], r["products"]) == (2, 0, 0, 1)
    for maxit in (0, 1):
        r = er.eigsh(lambda v: d.astype(np.float32) * v, 12, np.float32, 2, "LA", 4, 0.0, maxit, jacobi_fn=lib_jacobi)
        assert (r["reason"], r["restarts"], r["products"]) == (1, maxit, 4 + maxit * (4 - er.keep_of(2, 4)))
    assert [er.keep_of(k, ncv) for k, ncv in ((1, 2), (6, 20), (6, 30), (63, 64), (1, 17))] == [1, 13, 18, 63, 9]
    v = er.default_start(5, 0, np.float32)
    assert v.dtype == np.float32 and v[0] == np.float32(1 / 2 ** 24) and v[1] == np.float32(((1753845952 >> 8) + 1) / 2 ** 24)
    assert np.array_equal(er.default_start(5, (1 << 32) + 7, np.float64), er.default_start(5, 7, np.float64))


def test_names_are_declared_exported_and_bound():
    declared = _ffi.exported_names()
    lib = _ffi.lib()
    with open(os.path.join(ROOT, "rust_shim", "src", "ffi.rs")) as f:
        rust = f.read()
    for name in NAMES:
        assert name in declared
        assert getattr(lib, name).restype is C.c_int
        assert f"pub fn {name}(" in rust
    assert "pub struct spal_eigsh_info" in rust
    with open(os.path.join(ROOT, "include", "spalinalg.hpp")) as f:
        assert f.read().count("Eigenpairs<T> eigsh(") == 2
    for cls in (sp.CsrMatrix, sp.CscMatrix):
        assert callable(cls.eigsh)
    for cls in (sp.DeviceCsr, sp.DeviceCsc):
        assert callable(cls.eigsh) and callable(cls.eigsh_dev)


@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("sfx,ct,dt", [("f64", _ffi.f64p, np.float64), ("f32", _ffi.f32p, np.float32)])
def test_entry_points_refuse_without_a_device(kind, sfx, ct, dt):
    """Everything that needs nothing of the handle comes before the handle is read: a block of zeros stands in for it."""
    lib = _ffi.lib()
    inv = _ffi.SPAL_ERR_INVALID_ARGUMENT
    host, devf = getattr(lib, f"spal_{kind}_eigsh_{sfx}"), getattr(lib, f"spal_{kind}_eigsh_dev_{sfx}")
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    theta, resid, x = np.full(4, 9, dt), np.full(4, 9, dt), np.full((12, 4), 9, dt)
    info = sp.matrix._EigshInfoC()
    p = lambda a: a.ctypes.data_as(ct)                                                       # noqa: E731

    def call(h=fake, k=2, which=0, ncv=8, tol=1e-8, th=p(theta), rs=p(resid), ldx=4, inf=C.byref(info)):
        return host(h, u(k), C.c_int(which), u(ncv), None, u(0), u(0), C.c_double(tol), u(3), th, u(k), rs, u(k), p(x), u(ldx), u(12), inf)

    def dcall(h=fake, k=2, which=0, ncv=8, tol=1e-8, th=p(theta), rs=p(resid), ldx=4, inf=C.byref(info)):
        return devf(h, u(k), C.c_int(which), u(ncv), None, u(0), C.c_double(tol), u(3), th, rs, p(x), u(ldx), None, inf)

    for f, who in ((call, f"spal_{kind}_eigsh:"), (dcall, f"spal_{kind}_eigsh_dev:")):
        def refused(text, status):
            msg = lib.spal_last_error().decode()
            assert status == inv and msg.startswith(who) and text in msg, (status, msg)

        refused("null argument", f(h=None))
        refused("null argument", f(th=None))
        refused("null argument", f(rs=None))
        refused("null argument", f(inf=None))
        refused("k = 0", f(k=0))
        refused("ncv = 2 must be greater than k = 2", f(ncv=2))
        refused("ncv = 1 must be greater than k = 2", f(ncv=1))
        refused("ncv = 257 must be at most 256", f(ncv=257))
        refused("which = 2 must be 0 (LA) or 1 (SA)", f(which=2))
        refused("which = -1 must be 0 (LA) or 1 (SA)", f(which=-1))
        refused("must be finite and >= 0", f(tol=-1e-3))
        refused("must be finite and >= 0", f(tol=float("nan")))
        refused("must be finite and >= 0", f(tol=float("inf")))
        refused("ldx = 1 is less than k = 2", f(ldx=1))
    assert np.all(theta == 9) and np.all(resid == 9) and np.all(x == 9)
    assert lib.spal_eigsh_jacobi(u(0), p(theta), p(theta), p(theta), None) == inv
    assert lib.spal_eigsh_jacobi(u(2), None, p(theta), p(theta), None) == inv
    asym = np.array([[1.0, 2.0], [3.0, 4.0]])
    out = np.zeros(4)
    assert lib.spal_eigsh_jacobi(u(2), asym.ctypes.data_as(_ffi.f64p), out.ctypes.data_as(_ffi.f64p),
                                 out.ctypes.data_as(_ffi.f64p), None) == inv and b"not symmetric" in lib.spal_last_error()


def test_python_refuses_before_any_device_copy():
    a = sp.CsrMatrix(3, 3, [0, 1, 2, 3], [0, 1, 2], np.ones(3))
    wide = sp.CsrMatrix(3, 4, [0, 1, 2, 3], [0, 1, 3], np.ones(3))
    c = sp.CscMatrix(3, 3, [0, 1, 2, 3], [0, 1, 2], np.ones(3, dtype=np.float32))
    with pytest.raises(sp.Panic, match=r"not square \(3 x 4\)"):
        wide.eigsh(1)
    for m in (a, c):
        with pytest.raises(sp.Panic, match="ncv = 3 must be greater than k = 6"):
            m.eigsh()                                              # the default k = 6 on three rows
        with pytest.raises(sp.Panic, match="k = 0"):
            m.eigsh(0)
        with pytest.raises(sp.Panic, match="ncv = 5 must be at most 256 and at most the matrix's 3 rows"):
            m.eigsh(1, ncv=5)
        with pytest.raises(sp.Panic, match="must be 'LA' or 'SA'"):
            m.eigsh(1, which="LM")
        with pytest.raises(sp.Panic, match="tol = -1.0 must be finite"):
            m.eigsh(1, tol=-1)
        with pytest.raises(sp.Panic, match="v0 has shape"):
            m.eigsh(1, v0=np.ones(4))
    assert sp.matrix._eigsh_args(1000, 1000, 6, None, 0, np.float32) == (6, 20, float(np.finfo(np.float32).eps))
    assert sp.matrix._eigsh_args(1000, 1000, 12, None, 1e-3, np.float64) == (12, 25, 1e-3)
    assert sp.matrix._eigsh_args(10, 10, 3, None, 0, np.float64)[1] == 10
