"""The KPM moments without a device (include/spal.h): the probe hash, the text's doubling identities against
the direct moments, the trace check against numpy's eigenvalues, the count estimator on the numpy text, the refusals that
come before a device is touched, and the names, the bindings and the info struct."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import cheb_ref as cr
from tests import kpm_ref as K
from tests.krylov_ref import dot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [f"spal_{kind}_kpm_moments_{dev}{sfx}" for kind in ("csr", "csc") for dev in ("", "dev_") for sfx in ("f64", "f32")]
u, d = C.c_uint64, C.c_double


# ---- the probes ------------------------------------------------------------------------------------------------------------------

def test_mix32_has_the_headers_pinned_values():
    assert [K.mix32(v) for v in range(4)] == [0, 1753845952, 3507691905, 1408362973]
    from spalinalg_amd.matrix import _mix32
    assert _mix32(np.arange(4, dtype=np.uint32)).tolist() == [0, 1753845952, 3507691905, 1408362973]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,k,seed", [(1, 1, 0), (37, 5, 0), (300, 9, 7), (64, 3, 2**32 - 1), (40, 4, 2**32 + 7), (33, 256, 12345)])
def test_kpm_probes_is_the_scalar_loop(dtype, n, k, seed):
    z = sp.kpm_probes(n, k, seed, dtype)
    assert z.dtype == dtype and z.shape == (n, k)
    assert np.array_equal(z, K.probes_scalar(n, k, seed, dtype))
    assert set(np.unique(z)) <= {-1.0, 1.0}


def test_only_seed_mod_2_32_enters():
    assert np.array_equal(sp.kpm_probes(50, 4, 2**32 + 7), sp.kpm_probes(50, 4, 7))
    assert not np.array_equal(sp.kpm_probes(50, 4, 8), sp.kpm_probes(50, 4, 7))


def test_the_columns_differ_and_are_no_shifts_of_each_other():
    n, k = 512, 8
    z = sp.kpm_probes(n, k, 0)
    assert abs(z.mean()) < 4 / np.sqrt(n * k)            # +-1 in about equal numbers
    for j in range(k):
        for jp in range(k):
            for s in range(-8, 9):
                if j == jp and s == 0:
                    continue
                a = z[max(s, 0):n + min(s, 0), j]
                b = z[max(-s, 0):n + min(-s, 0), jp]
                agree = np.mean(a == b)
                assert 0.35 < agree < 0.65, (j, jp, s, agree)   # neither a copy nor a negated copy: 4 sigma is 0.09


# ---- the text --------------------------------------------------------------------------------------------------------------------

def test_the_block_text_is_the_column_text_and_its_dot_is_the_dot():
    rng = np.random.default_rng(5)
    for dtype in (np.float64, np.float32):
        csr = K.poisson2d(40, dtype)                      # 1600 rows: two dot tiles
        Z = rng.standard_normal((1600, 3)).astype(dtype)
        A, B = Z, Z[::-1].copy()
        assert np.array_equal(K.dots(A, B), np.array([dot(A[:, j].copy(), B[:, j].copy()) for j in range(3)], dtype=dtype))
        assert np.array_equal(K.rowsum_block(*csr, Z)[:, 1], cr.rowsum(*csr, Z[:, 1].copy()))
        mu = K.moments(csr, Z, 7, (-0.1, 8.1))
        for j in range(3):
            assert np.array_equal(mu[:, j], K.moments_column(*csr, Z[:, j], 7, -0.1, 8.1).astype(np.float64))


def test_the_doubling_identities_give_the_direct_moments():
    """mu_{2i} = 2 (t_i, t_i) - mu_0 and mu_{2i+1} = 2 (t_{i+1}, t_i) - mu_1 against dot(z, t_i), float64, 6 rows.  Both
    sides carry the recurrence's rounding, at most about 8 d^2 eps |z|^2 (see the trace check below)."""
    a = np.array([[2.0, -1, 0, 0, 0, 0.5], [-1, 2, -1, 0, 0, 0], [0, -1, 3, -1, 0, 0], [0, 0, -1, 2, -1, 0],
                  [0, 0, 0, -1, 1, -1], [0.5, 0, 0, 0, -1, 2]])
    csr = K.from_dense(a, np.float64)
    lam = np.linalg.eigvalsh(a)
    lo, hi = lam[0] - 0.1, lam[-1] + 0.1
    rng = np.random.default_rng(1)
    for degree in (1, 2, 3, 8, 9):
        z = rng.standard_normal(6)
        mu = K.moments_column(*csr, z, degree, lo, hi)
        direct = K.moments_direct(csr, z, degree, lo, hi)
        assert mu.shape == direct.shape == (degree + 1,)
        assert np.max(np.abs(mu - direct)) <= 8 * degree**2 * np.finfo(np.float64).eps * (z @ z)


def chebyshev_traces(csr, degree, lo, hi):
    lam = np.linalg.eigvalsh(K.to_dense(csr))
    th = np.arccos((lam - (lo + hi) / 2) / ((hi - lo) / 2))
    return np.array([np.cos(i * th).sum() for i in range(degree + 1)])


def trace_tolerance(n, degree, eps):
    """A local error of a recurrence step is at most (r + 3) eps |t| with r <= 5 entries per row, so 8 eps; it reaches
    t_i through the recurrence of the second kind, whose values are at most i - j + 1: |dt_i| <= 4 i^2 eps |z|.  A moment
    doubles the index: 2 (t_i, t_i) errs by 4 |t_i| |dt_i| <= 16 (d/2)^2 eps = 4 d^2 eps for a unit probe, and the dot's
    own rounding is far below that.  n columns are summed: 4 n d^2 eps, doubled for the reference's arccos and cos."""
    return 8 * n * degree**2 * eps


@pytest.mark.parametrize("name", ["laplace1d_64", "poisson_8x8"])
def test_the_moments_of_the_identity_are_the_chebyshev_traces(name):
    csr = K.laplace1d(64, np.float64) if name == "laplace1d_64" else K.poisson2d(8, np.float64)
    degree = 128
    lo, hi = K.auto_interval(*csr)
    mu = K.moments(csr, np.eye(64), degree, (lo, hi))
    gap = np.max(np.abs(mu.sum(axis=1) - chebyshev_traces(csr, degree, lo, hi)))
    print(name, "largest gap", gap)
    assert gap <= trace_tolerance(64, degree, np.finfo(np.float64).eps)


# ---- the estimator ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def estimator_case(name, dtype_name):
    dtype = np.dtype(dtype_name).type
    csr = K.laplace1d(400, dtype) if name == "laplace1d" else K.poisson2d(20, dtype)
    lam = np.linalg.eigvalsh(K.to_dense(csr))
    lo, hi = K.auto_interval(*csr)
    hashed = K.moments(csr, sp.kpm_probes(400, 32, 0, dtype), 128, (lo, hi))
    identity = K.moments(csr, np.eye(400, dtype=dtype), 128, (lo, hi)) if dtype is np.float64 else None
    return lam, lo, hi, hashed, identity


# what the text gives on this matrix (estimate - exact, hashed probes, seed 0, 32 probes, degree 128, Jackson):
#   float64: 1-D Laplacian [0, 1]: -5.155;  Poisson 20x20 [2, 5]: -1.527;  Poisson 20x20 [0, 1]: -2.098
#   float32: the same to three decimals (-5.155, -1.527, -2.098)
#   identity probes, float64 (the truncation and the damping alone): -2.681, -1.633, +0.653
ESTIMATOR_CASES = [("laplace1d", 0.0, 1.0, 133, -2.7), ("poisson", 2.0, 5.0, 208, -1.6), ("poisson", 0.0, 1.0, 30, 0.7)]


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("name,a,b,exact,identity_error", ESTIMATOR_CASES)
def test_the_count_estimate_is_within_three_percent_of_n(name, a, b, exact, identity_error, dtype_name):
    lam, lo, hi, hashed, identity = estimator_case(name, dtype_name)
    assert int(((lam >= a) & (lam <= b)).sum()) == exact
    est, se = sp.kpm_count(hashed, lo, hi, a, b, damping="jackson")
    print(name, dtype_name, [a, b], "exact", exact, "estimate %.3f" % est, "error %.3f" % (est - exact), "standard error %.3f" % se)
    assert abs(est - exact) <= 12                        # 3 % of n = 400
    assert 0 < se < 12
    if identity is not None:
        est_i, se_i = sp.kpm_count(identity.sum(axis=1), lo, hi, a, b)
        print("   identity probes: error %.3f" % (est_i - exact))
        assert abs((est_i - exact) - identity_error) <= 0.05 and se_i == 0.0


def test_the_density_integrates_to_n_and_the_dampings_are_what_they_say():
    lam, lo, hi, hashed, _ = estimator_case("poisson", "float64")
    x = np.linspace(lo, hi, 4001)[1:-1]
    rho = sp.kpm_density(hashed, lo, hi, x)
    assert rho.min() > -1e-9                              # Jackson's kernel is nonnegative
    assert abs(np.sum(rho) * (x[1] - x[0]) - 400) < 2
    assert sp.kpm_density(hashed, lo, hi, [lo - 1, hi + 1]).tolist() == [0.0, 0.0]
    total, _ = sp.kpm_count(hashed, lo, hi, lo, hi)
    assert abs(total - 400) < 1e-9                        # +-1 probes: mu_0 = n exactly
    g = sp.kpm_damping(128, "jackson")
    assert g.shape == (129,) and abs(g[0] - 1) < 1e-15 and np.all(np.diff(g) < 0) and 0 < g[-1] < 1e-3
    assert np.array_equal(sp.kpm_damping(4, "fejer"), np.array([5, 4, 3, 2, 1]) / 5)
    with pytest.raises(ValueError):
        sp.kpm_damping(4, "lorentz")


# ---- names and layout ------------------------------------------------------------------------------------------------------------

def test_the_names_are_declared_exported_and_bound():
    declared = set(_ffi.exported_names())
    lib = _ffi.lib()
    ffi_rs = open(os.path.join(ROOT, "rust_shim", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "spalinalg.hpp")).read()
    for name in NAMES:
        assert name in declared and hasattr(lib, name) and f"pub fn {name}(" in ffi_rs and name in hpp, name
    assert "pub struct spal_kpm_info" in ffi_rs and "kpm_moments" in hpp
    for cls in (sp.DeviceCsr, sp.DeviceCsc):
        assert all(hasattr(cls, m) for m in ("kpm_moments", "kpm_moments_dev"))
    for cls in (sp.CsrMatrix, sp.CscMatrix):
        assert all(hasattr(cls, m) for m in ("kpm_moments", "eig_count", "spectral_density"))
    assert all(callable(getattr(sp, f)) for f in ("kpm_probes", "kpm_damping", "kpm_density", "kpm_count"))
    header = open(os.path.join(ROOT, "include", "spal.h")).read()
    assert "Rayleigh-Ritz on A in" in header and "automatic choice of the degree" in header and "kpm_moments(A; d, Z)" in header


def test_the_info_struct_matches_the_header():
    from spalinalg_amd.matrix import _KpmInfoC
    assert [f[0] for f in _KpmInfoC._fields_] == ["products", "lo", "hi", "glo", "ghi", "degree", "probes", "solve_ms"]
    assert C.sizeof(_KpmInfoC) == 64
    header = open(os.path.join(ROOT, "include", "spal.h")).read()
    body = header.split("typedef struct spal_kpm_info {")[1].split("}")[0]
    assert "".join(body.split()) == "uint64_tproducts;doublelo,hi,glo,ghi;uint64_tdegree,probes;doublesolve_ms;"


# ---- the refusals that need no device --------------------------------------------------------------------------------------------

def test_python_refusals_come_before_a_device_is_touched(monkeypatch):
    rp, ci, va = K.laplace1d(30, np.float64)
    a = sp.CsrMatrix(30, 30, rp, ci, va)
    monkeypatch.setattr(type(a), "device", lambda self, device=0: pytest.fail("a device was touched"))
    for kw in (dict(degree=0), dict(degree=4097), dict(probes=0), dict(probes=257), dict(interval=(4.0, 0.0)),
               dict(interval=(1.0, 1.0)), dict(interval=(0.0, np.inf)), dict(interval=(np.nan, 4.0)), dict(Z=np.ones((29, 2))),
               dict(Z=np.ones(30)), dict(Z=np.ones((30, 257)))):
        kw = dict(dict(degree=8), **kw)
        with pytest.raises(sp.Panic):
            a.kpm_moments(**kw)
    with pytest.raises(sp.Panic):
        a.eig_count(0.0, 1.0, degree=0)
    with pytest.raises(sp.Panic):
        a.spectral_density([1.0], probes=0)
    rect = sp.CsrMatrix(2, 3, np.array([0, 1, 2], np.uint64), np.array([0, 1], np.uint64), np.ones(2))
    monkeypatch.setattr(type(rect), "device", lambda self, device=0: pytest.fail("a device was touched"))
    with pytest.raises(sp.Panic):
        rect.kpm_moments(8)


class FakeHandle(C.Structure):
    """Zeroed and never used as a handle: every refusal below comes before the device is touched."""
    _fields_ = [("pad", C.c_char * 64)]


@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("sfx,ct", [("f64", C.c_double), ("f32", C.c_float)])
def test_c_refusals_on_a_stand_in_handle(kind, sfx, ct):
    from spalinalg_amd.matrix import _KpmInfoC
    lib = _ffi.lib()
    E = _ffi.SPAL_ERR_INVALID_ARGUMENT
    h = C.cast(C.pointer(FakeHandle()), C.c_void_p)
    host = getattr(lib, f"spal_{kind}_kpm_moments_{sfx}")
    dev = getattr(lib, f"spal_{kind}_kpm_moments_dev_{sfx}")
    info = _KpmInfoC()
    mu = (C.c_double * 64)()
    z = (ct * 64)()
    ok = dict(a=h, degree=3, k=2, auto=0, lo=0.0, hi=4.0, z=None, z_rows=0, ldz=2, mu=mu, mu_len=8, info=C.byref(info))
    for change in (dict(a=None), dict(mu=None), dict(info=None), dict(degree=0), dict(degree=4097), dict(k=0), dict(k=257),
                   dict(mu_len=7), dict(mu_len=9), dict(z=z, ldz=1), dict(auto=2), dict(auto=-1), dict(lo=float("nan")),
                   dict(hi=float("inf")), dict(lo=4.0, hi=0.0), dict(lo=1.0, hi=1.0)):
        p = dict(ok, **change)
        assert host(p["a"], u(p["degree"]), u(p["k"]), u(0), C.c_int(p["auto"]), d(p["lo"]), d(p["hi"]), p["z"], u(p["z_rows"]),
                    u(p["ldz"]), p["mu"], u(p["mu_len"]), p["info"]) == E, change
        assert dev(p["a"], u(p["degree"]), u(p["k"]), u(0), C.c_int(p["auto"]), d(p["lo"]), d(p["hi"]), p["z"], u(p["ldz"]),
                   p["mu"], u(p["mu_len"]), None, p["info"]) == E, change
    # the host form alone knows the caller's rows: the stand-in has none
    assert host(h, u(3), u(2), u(0), C.c_int(0), d(0.0), d(4.0), z, u(5), u(2), mu, u(8), C.byref(info)) == E
    assert b"z_rows" in lib.spal_last_error()
