"""The KPM moments on the device against the text (include/spal.h; tests/kpm_ref.py): bits, not
tolerances -- f32 and f64, CSR and CSC, at the dot tile's edges (a workgroup of the step owns 1024 rows), every column tile,
chunk and form, special values, the _dev form, and the refusals that read the handle.  The two analytic checks (the
Chebyshev traces, the count) are the only comparisons with a tolerance."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import cheb_ref as cr
from tests import kpm_ref as K
from tests import near_ref as nr
from tests import trsv_ref as tr
from tests.test_gpu_cheb import from_rows, make, sfx, some
from tests.test_kpm_host import chebyshev_traces, trace_tolerance

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
TILE = 1024                                    # rows of a workgroup = dot's tile
LO, HI = -1.0, 1.0                             # every row's |entries| sum to at most 1
DESCRIBE_KEYS = {"degree", "probes", "steps", "tile", "form", "chunk", "lo", "hi", "launches", "solve_ms"}
u, dbl = C.c_uint64, C.c_double


@functools.lru_cache(maxsize=None)
def shape(name, dtype):
    """(n, rowptr, colind, values); shared, read-only"""
    rng = np.random.default_rng(zlib.crc32(f"kpm/{name}".encode()))
    if name.startswith("n="):                   # 1 + r % 7 entries per row
        n = int(name[2:])
        mat = from_rows(n, {r: some(rng, n, 1 + r % 7) for r in range(n)}, dtype, rng)
    elif name == "empty-rows":                  # one empty row; empty at a workgroup's start, across its edge and at the end
        n = 2 * TILE + 100
        empty = set(range(10)) | {500} | set(range(TILE - 9, TILE + 12)) | set(range(2 * TILE, 2 * TILE + 5)) | set(range(n - 10, n))
        mat = from_rows(n, {r: some(rng, n, 5) for r in range(n) if r not in empty}, dtype, rng)
    elif name == "row-5000":                    # one row longer than any chunk, beside rows of 2
        n = 6000
        rows = {r: some(rng, n, 2) for r in range(n)}
        rows[1500] = some(rng, n, 5000)
        mat = from_rows(n, rows, dtype, rng)
    elif name == "one-row":                     # all entries in one row
        n = 1500
        mat = from_rows(n, {700: some(rng, n, 1200)}, dtype, rng)
    elif name == "diagonal-2^20+1":             # a third level of the dot
        n = TILE * TILE + 1
        mat = (n, np.arange(n + 1, dtype=np.uint64), np.arange(n, dtype=np.uint64), rng.uniform(-1, 1, n).astype(dtype))
    else:
        raise KeyError(name)
    for a in mat[1:]:
        a.setflags(write=False)
    return mat


@functools.lru_cache(maxsize=None)
def text(name, dtype, k, degree, seed=5):
    """the text's moments of the hashed probes on [LO, HI]; shared, read-only"""
    mat = shape(name, dtype)
    mu = K.moments(mat[1:], sp.kpm_probes(mat[0], k, seed, dtype), degree, (LO, HI))
    mu.setflags(write=False)
    return mu


SHAPES = ["n=1", "n=255", "n=1023", "n=1024", "n=1025", "n=2049", "empty-rows", "row-5000", "one-row"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("name", SHAPES)
def test_the_moments_are_the_text(name, kind, dtype):
    a = make(kind, shape(name, dtype))
    mu, info = a.kpm_moments(9, probes=3, seed=5, interval=(LO, HI))
    assert mu.dtype == np.float64 and mu.shape == (10, 3)
    tr.assert_same_bits(mu, text(name, dtype, 3, 9))
    assert (info.products, info.degree, info.probes, info.lo, info.hi, info.glo, info.ghi) == (5, 9, 3, LO, HI, 0.0, 0.0)
    assert info.solve_ms > 0
    d = a.device().describe()["kpm"]
    assert set(d) == DESCRIBE_KEYS
    assert (d["degree"], d["probes"], d["steps"], d["tile"], d["form"], d["lo"], d["hi"]) == (9, 3, 5, 4, 1, LO, HI)
    assert d["launches"] == 1 + 2 * 5


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_width_and_both_parities_of_the_degree(dtype):
    a = make("csr", shape("n=1025", dtype))
    wide = text("n=1025", dtype, 33, 3)
    for k in (1, 3, 8, 9, 33):
        mu, _ = a.kpm_moments(3, probes=k, seed=5, interval=(LO, HI))
        tr.assert_same_bits(mu, text("n=1025", dtype, k, 3))
        tr.assert_same_bits(mu, np.ascontiguousarray(wide[:, :k]))        # a column does not depend on k
    for degree in (1, 2, 3, 8, 9):
        mu, info = a.kpm_moments(degree, probes=3, seed=5, interval=(LO, HI))
        assert mu.shape == (degree + 1, 3) and info.products == (degree + 1) // 2
        tr.assert_same_bits(mu, text("n=1025", dtype, 3, degree))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_third_level_of_the_dot(dtype):
    a = make("csr", shape("diagonal-2^20+1", dtype))
    mu, _ = a.kpm_moments(2, probes=1, seed=5, interval=(LO, HI))
    tr.assert_same_bits(mu, text("diagonal-2^20+1", dtype, 1, 2))
    assert mu[0, 0] == TILE * TILE + 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["row-5000", "n=2049"])
def test_chunk_tile_and_form_do_not_change_the_bits(name, dtype):
    mat = shape(name, dtype)
    dev = make("csr", mat).device()
    ref = text(name, dtype, 9, 4)
    size = np.dtype(dtype).itemsize
    try:
        for chunk in (0, 256, 512, 1024, 2048, 4096):
            dev.set_option("cheb_chunk", chunk)
            for tile in (0, 1, 2, 4, 8):
                dev.set_option("kpm_tile", tile)
                for form in (0, 1, 2):
                    if form == 0 and (chunk, tile) != (0, 0):
                        continue
                    dev.set_option("kpm_form", form)
                    mu, _ = dev.kpm_moments(4, probes=9, seed=5, interval=(LO, HI))
                    tr.assert_same_bits(mu, ref)
                    d = dev.describe()["kpm"]
                    kt = tile or 8
                    assert (d["tile"], d["form"]) == (kt, 2 if form == 2 else 1)
                    assert d["chunk"] == min(chunk or 16384 // size, 32768 // (kt * size))
                    assert d["launches"] == 1 + (3 if form == 2 else 2) * 2
    finally:
        for key in ("cheb_chunk", "kpm_tile", "kpm_form"):
            dev.set_option(key, 0)
    for key, bad in (("kpm_tile", 3), ("kpm_tile", 16), ("kpm_tile", -1), ("kpm_form", 3), ("kpm_form", -1)):
        with pytest.raises(sp.Panic):
            dev.set_option(key, bad)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_a_given_block_its_leading_dimension_and_special_values(kind, dtype):
    mat = shape("n=1025", dtype)
    n = mat[0]
    a = make(kind, mat)
    k = 5
    # the hashed block, given: the same bits; ldz > k with a poisoned padding that stays what it was
    big = np.full((n, k + 3), 7, dtype=dtype)
    big[:, :k] = sp.kpm_probes(n, k, 5, dtype)
    before = big.copy()
    mu, info = a.kpm_moments(4, interval=(LO, HI), Z=big[:, :k])
    tr.assert_same_bits(mu, text("n=1025", dtype, k, 4))
    assert info.probes == k and np.array_equal(big, before)
    # a general block with -0.0 and zeros in it, on a matrix whose products are -0.0
    rng = np.random.default_rng(11)
    Z = rng.uniform(-1, 1, (n, k)).astype(dtype)
    Z[::7, 0], Z[3::7, 0], Z[:, 4] = -0.0, 0.0, -0.0
    negz = (n, mat[1], mat[2], np.where(np.arange(mat[3].size) % 3 == 0, -0.0, mat[3]).astype(dtype))
    for m in (mat, negz):
        am = make(kind, m)
        tr.assert_same_bits(am.kpm_moments(5, interval=(LO, HI), Z=Z)[0], K.moments(m[1:], Z, 5, (LO, HI)))
    # one NaN and one inf in ONE column: the others are what they were
    clean = a.kpm_moments(5, interval=(LO, HI), Z=Z)[0]
    bad = Z.copy()
    bad[100, 1], bad[900, 1] = np.nan, np.inf
    got = a.kpm_moments(5, interval=(LO, HI), Z=bad)[0]
    tr.assert_same_bits(got, K.moments(mat[1:], bad, 5, (LO, HI)))
    others = [0, 2, 3, 4]
    tr.assert_same_bits(np.ascontiguousarray(got[:, others]), np.ascontiguousarray(clean[:, others]))
    assert not np.isfinite(got[:, 1]).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_the_automatic_interval_is_gershgorins_with_the_margin(kind, dtype):
    csr = K.laplace1d(1025, dtype)
    a = make(kind, (1025, *csr))
    glo, ghi = cr.gershgorin(*csr)
    lo, hi = nr.auto_interval(glo, ghi)
    mu, info = a.kpm_moments(6, probes=4, seed=1)
    assert (info.glo, info.ghi, info.lo, info.hi) == (glo, ghi, lo, hi)
    tr.assert_same_bits(mu, K.moments(csr, sp.kpm_probes(1025, 4, 1, dtype), 6))
    given, ginfo = a.kpm_moments(6, probes=4, seed=1, interval=(lo, hi))
    tr.assert_same_bits(given, mu)
    assert (ginfo.glo, ginfo.ghi, ginfo.lo, ginfo.hi) == (0.0, 0.0, lo, hi)
    # a value that is not finite: no automatic interval, and nothing is returned
    vals = csr[2].copy()
    vals[7] = np.inf
    with pytest.raises(sp.Panic, match="Gershgorin's bounds are not finite"):
        make(kind, (1025, csr[0], csr[1], vals)).kpm_moments(6, probes=4)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_the_device_form_at_offsets_into_poisoned_buffers(kind, dtype):
    import torch
    mat = shape("n=2049", dtype)
    n = mat[0]
    dev = make(kind, mat).device()
    tt = torch.float64 if dtype == np.float64 else torch.float32
    size = np.dtype(dtype).itemsize
    k, ldz = 3, 5
    Z = sp.kpm_probes(n, k, 5, dtype)
    buf = torch.full((n * ldz + 9,), 7, dtype=tt, device="cuda")
    buf[3:3 + n * ldz].view(n, ldz)[:, :k] = torch.from_numpy(Z).cuda()
    before = buf.cpu().numpy()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    for _ in range(2):                          # the second call reuses the stream's scratch
        mu, _ = dev.kpm_moments_dev(9, k, interval=(LO, HI), z_ptr=buf.data_ptr() + 3 * size, ldz=ldz, stream=s)
        hashed, _ = dev.kpm_moments_dev(9, k, seed=5, interval=(LO, HI), stream=s)
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    again, _ = dev.kpm_moments_dev(9, k, interval=(LO, HI), z_ptr=buf.data_ptr() + 3 * size, ldz=ldz, stream=s)
    auto, _ = dev.kpm_moments_dev(9, k, seed=5, stream=s)
    auto2, _ = dev.kpm_moments_dev(9, k, seed=5, stream=s)
    assert torch.cuda.mem_get_info()[0] == free
    for got in (mu, hashed, again):
        tr.assert_same_bits(got, text("n=2049", dtype, k, 9))
    tr.assert_same_bits(auto, auto2)
    assert np.array_equal(buf.cpu().numpy(), before)                          # the block is only read
    with pytest.raises(sp.Panic, match="ldz must be at least k"):
        dev.kpm_moments_dev(9, k, interval=(LO, HI), z_ptr=buf.data_ptr(), ldz=k - 1, stream=s)


@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_refusals_that_read_the_handle_and_a_capturing_stream(kind):
    import torch
    lib = _ffi.lib()
    mat = shape("n=255", np.float64)
    n = mat[0]
    dev = make(kind, mat).device()
    inv = _ffi.SPAL_ERR_INVALID_ARGUMENT
    mu = np.zeros(8)
    info = sp.matrix._KpmInfoC()
    mp = mu.ctypes.data_as(_ffi.f64p)
    assert getattr(lib, f"spal_{kind}_kpm_moments_f32")(dev._h, u(3), u(2), u(0), C.c_int(0), dbl(LO), dbl(HI), None, u(0), u(2), mp, u(8),
                                                        C.byref(info)) == inv
    assert "handle holds f64 values" in lib.spal_last_error().decode() and not mu.any()
    z = np.ones((n, 2))
    zp = z.ctypes.data_as(_ffi.f64p)
    fn = getattr(lib, f"spal_{kind}_kpm_moments_f64")
    assert fn(dev._h, u(3), u(2), u(0), C.c_int(0), dbl(LO), dbl(HI), zp, u(n - 1), u(2), mp, u(8), C.byref(info)) == inv
    assert "z_rows" in lib.spal_last_error().decode() and not mu.any()
    wide = sp.CsrMatrix(3, 4, [0, 1, 2, 3], [0, 1, 3], np.ones(3)) if kind == "csr" else sp.CscMatrix(3, 4, [0, 1, 2, 2, 3], [0, 1, 2], np.ones(3))
    with pytest.raises(sp.Panic, match=r"not square \(3 x 4\)"):
        wide.device().kpm_moments(3, probes=2, interval=(LO, HI))
    xt = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()               # never replayed
    with torch.cuda.graph(graph):
        xt.fill_(0.0)                            # (so that the graph is not empty)
        capturing = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        s1 = getattr(lib, f"spal_{kind}_kpm_moments_dev_f64")(dev._h, u(3), u(2), u(0), C.c_int(0), dbl(LO), dbl(HI), None, u(2), mp, u(8),
                                                              capturing, C.byref(info))
        m1 = lib.spal_last_error().decode()
    torch.cuda.synchronize()
    assert s1 == inv and "cannot be captured into a graph" in m1, (s1, m1)
    del graph
    assert not mu.any() and "kpm" not in dev.describe()


def test_row_block_handles_are_refused(monkeypatch):
    import spal_synth as synth
    rp, ci, va = synth.banded_csr(2000, 2000, 4, 64, 3)
    monkeypatch.setenv("SPAL_CSR_PART_ENTRIES", "3000")
    big = sp.CsrMatrix(2000, 2000, rp, ci, va)
    assert big.device().describe()["kernel"] == "row_blocks"
    monkeypatch.delenv("SPAL_CSR_PART_ENTRIES")
    with pytest.raises(sp.SpalError, match=r"spal_csr_kpm_moments: an operand of more than 2\^32 - 65537 entries \(row blocks\)") as e:
        big.kpm_moments(4, probes=2, interval=(LO, HI))
    assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED
    assert "kpm" not in big.device().describe()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_chebyshev_calls_and_eigsh_give_their_old_bits_after_a_kpm_call(dtype):
    mat = shape("n=1025", dtype)
    n, rowptr, colind, values = mat
    a = make("csr", mat)
    x = np.random.default_rng(3).uniform(-1, 1, n).astype(dtype)
    coef = np.random.default_rng(4).uniform(-1, 1, 6)
    lap = make("csr", (400, *K.laplace1d(400, dtype)))

    def old():
        theta, X, info = lap.eigsh(2, "LA", ncv=12, tol=1e-4, maxit=40)
        return a.cheb_apply(x, 5, -0.5, 0.5, 1.5), a.cheb_series(x, coef, LO, HI), theta, X, info.resid

    first = old()
    tr.assert_same_bits(first[0], cr.cheb_apply(rowptr, colind, values, x, 5, -0.5, 0.5, 1.5))
    tr.assert_same_bits(first[1], nr.cheb_series(rowptr, colind, values, x, LO, HI, coef))
    a.device().set_option("kpm_form", 2)
    a.kpm_moments(5, probes=9, interval=(LO, HI))
    a.device().set_option("kpm_form", 0)
    a.kpm_moments(5, probes=3, interval=(LO, HI))
    lap.kpm_moments(5, probes=3)
    for got, was in zip(old(), first):
        tr.assert_same_bits(got, was)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["laplace1d_64", "poisson_8x8"])
def test_the_moments_of_the_identity_are_the_chebyshev_traces_through_the_device(name, dtype):
    csr = K.laplace1d(64, dtype) if name == "laplace1d_64" else K.poisson2d(8, dtype)
    degree = 128
    lo, hi = K.auto_interval(*csr)
    mu, info = make("csr", (64, *csr)).kpm_moments(degree, Z=np.eye(64, dtype=dtype))
    assert (info.lo, info.hi, info.probes) == (lo, hi, 64)
    tr.assert_same_bits(mu, K.moments(csr, np.eye(64, dtype=dtype), degree))
    gap = np.max(np.abs(mu.sum(axis=1) - chebyshev_traces(csr, degree, lo, hi)))
    print(name, sfx(dtype), "largest gap", gap)
    assert gap <= trace_tolerance(64, degree, np.finfo(dtype).eps)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_eig_count_and_spectral_density_are_the_host_functions_of_the_texts_moments(dtype):
    csr = K.poisson2d(20, dtype)
    a = make("csr", (400, *csr))
    lo, hi = K.auto_interval(*csr)
    ref = K.moments(csr, sp.kpm_probes(400, 32, 0, dtype), 128, (lo, hi))
    assert a.eig_count(2.0, 5.0) == sp.kpm_count(ref, lo, hi, 2.0, 5.0)
    assert a.eig_count(0.0, 1.0, damping="fejer") == sp.kpm_count(ref, lo, hi, 0.0, 1.0, damping="fejer")
    est, se = a.eig_count(2.0, 5.0)
    assert abs(est - 208) <= 12 and 0 < se < 12       # the bound of tests/test_kpm_host.py
    pts = np.linspace(0.5, 7.5, 15)
    assert np.array_equal(a.spectral_density(pts), sp.kpm_density(ref, lo, hi, pts))
