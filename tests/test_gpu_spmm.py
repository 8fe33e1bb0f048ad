"""GPU: Y = A * X for a dense row-major block of k vectors (spal_csr_spmm_* / spal_csc_spmm_*) against the CPU oracle,
one oracle SpMV per column: oracle.csr_spmv for CSR, oracle.csc_spmv for CSC.  Every comparison is exact: values equal
as raw bits, NaN by position (a NaN's payload is not part of the contract).  Nothing is sampled: the oracle does every
row of every column."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

import spalinalg_amd as sp
import spal_synth as synth
from spalinalg_amd import _ffi
from tests.test_gpu_spadd import power_law
from tests.util import random_csr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 64, 100)
TILES = (1, 2, 4, 8, 16, 32)
DTYPES = [np.float64, np.float32]


def bits_of(dtype):
    return np.uint64 if np.dtype(dtype) == np.float64 else np.uint32


def assert_bits(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn)
    b = bits_of(got.dtype)
    bad = np.argwhere((np.ascontiguousarray(got).view(b) != np.ascontiguousarray(ref).view(b)) & ~gn)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), [(got[tuple(i)], ref[tuple(i)]) for i in bad[:5]])


def block(ncols, k, dtype, seed=11):
    """(ncols, k) block of vectors in (-1, 1), C-contiguous"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (ncols, k)).astype(dtype)


def csr_ref(oracle, rp, ci, va, X):
    X = np.asarray(X)
    return np.stack([oracle.csr_spmv(rp, ci, va, np.ascontiguousarray(X[:, j])) for j in range(X.shape[1])], axis=1)


def csc_ref(oracle, nrows, cp, ri, va, X):
    X = np.asarray(X)
    return np.stack([oracle.csc_spmv(nrows, cp, ri, va, np.ascontiguousarray(X[:, j])) for j in range(X.shape[1])],
                    axis=1)


def make(fmt, oracle, nrows, ncols, rp, ci, va):
    """(matrix of `fmt`, its reference function X -> Y) from CSR arrays"""
    if fmt == "csr":
        return sp.CsrMatrix(nrows, ncols, rp, ci, va), lambda X: csr_ref(oracle, rp, ci, va, X)
    cp, ri, cv = oracle.transpose(nrows, ncols, rp, ci, va)
    return sp.CscMatrix(nrows, ncols, cp, ri, cv), lambda X: csc_ref(oracle, nrows, cp, ri, cv, X)


# ---- 1. known answer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_g5_columns_as_one_block(kats, oracle, dtype):
    g = kats["G5_csc_mul"]
    a = g["lhs"]
    vals = np.array(a["values"], dtype=dtype)
    X = np.array([c["x"] for c in g["spmv"]], dtype=dtype).T.copy()      # 3 x 4
    Y = np.array([c["y"] for c in g["spmv"]], dtype=dtype).T             # 5 x 4
    csc = sp.CscMatrix(a["nrows"], a["ncols"], a["colptr"], a["rowind"], vals)
    rp, ci, rv = oracle.transpose(a["ncols"], a["nrows"], a["colptr"], a["rowind"], vals)
    csr = sp.CsrMatrix(a["nrows"], a["ncols"], rp, ci, rv)
    for m in (csc, csr):
        for got in (m @ X, m * X, m.device().spmm(X)):
            assert got.dtype == np.dtype(dtype) and got.shape == (5, 4)
            assert got.tolist() == Y.tolist()
    d = csr.device().describe()["spmm"]
    assert d["k"] == 4 and d["tile"] == 4 and d["column_tiles"] == 1 and d["long_rows"] == 0, d
    assert csc.device().describe()["spmm"]["k"] == 4


# ---- 2. random parity --------------------------------------------------------------------------------------------
def _matrix(case, dtype):
    rng = np.random.default_rng(sorted(CASES).index(case) + 100)
    if case == "banded":
        n = 100_003
        return (n, n) + tuple(synth.banded_csr(n, n, 14, 4096, synth.matrix_seed(3), dtype=dtype))
    if case == "ragged":
        n = 60_011
        return (n, n) + tuple(synth.ragged_csr(n, n, 4096, 5, dtype=dtype))
    if case == "anywhere":
        return (3000, 2500) + tuple(random_csr(rng, 3000, 2500, density=0.004, dtype=dtype, empty_rows=0.1))
    if case == "tall":
        return (20_000, 37) + tuple(random_csr(rng, 20_000, 37, density=0.2, dtype=dtype))
    if case == "wide":
        return (41, 30_000) + tuple(random_csr(rng, 41, 30_000, density=0.01, dtype=dtype))
    if case == "one_row":
        return (1, 5000) + tuple(random_csr(rng, 1, 5000, density=0.3, dtype=dtype, empty_rows=0.0))
    if case == "one_col":
        return (5000, 1) + tuple(random_csr(rng, 5000, 1, density=0.6, dtype=dtype))
    if case == "all_empty":
        return (700, 300) + tuple(random_csr(rng, 700, 300, density=0.5, dtype=dtype, empty_rows=1.0))
    raise KeyError(case)


CASES = ("banded", "ragged", "anywhere", "tall", "wide", "one_row", "one_col", "all_empty")


@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_random_parity_every_k(oracle, case, dtype, fmt):
    nrows, ncols, rp, ci, va = _matrix(case, dtype)
    m, ref = make(fmt, oracle, nrows, ncols, rp, ci, va)
    X = block(ncols, max(KS), dtype)
    Y_ref = ref(X)                     # column j of the result does not depend on k: one oracle run serves every k
    if fmt == "csc":                   # ... and the two oracles agree on these inputs: a CSC failure is the device's
        assert_bits(Y_ref, csr_ref(oracle, rp, ci, va, X))
    if case == "all_empty":
        assert int(rp[-1]) == 0 and not np.signbit(Y_ref).any() and not Y_ref.any()
    for k in KS:
        Y = m @ np.ascontiguousarray(X[:, :k])
        assert Y.shape == (nrows, k)
        assert_bits(Y, Y_ref[:, :k])
        if case == "all_empty":
            assert not np.signbit(Y).any()
    d = m.device().describe()["spmm"]
    assert d["k"] == KS[-1] and d["column_tiles"] == -(-KS[-1] // d["tile"]), d


# ---- 3. every instantiated column tile ------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["banded", "power_law"])
def test_every_tile_gives_the_same_bits(oracle, kind, dtype, fmt):
    if kind == "banded":
        n = 50_021
        rp, ci, va = synth.banded_csr(n, n, 14, 4096, 7, dtype=dtype)
    else:
        n = 20_000
        rp, ci, va = power_law(n, 21, dtype=dtype)
    m, ref = make(fmt, oracle, n, n, rp, ci, va)
    dev = m.device()
    for k in (5, 40):
        X = block(n, k, dtype, seed=k)
        Y_ref = ref(X)
        for tile in TILES:
            dev.set_option("spmm_tile", tile)
            assert_bits(dev.spmm(X), Y_ref)
            d = dev.describe()["spmm"]
            assert d["tile"] == tile and d["k"] == k and d["column_tiles"] == -(-k // tile), d
        dev.set_option("spmm_tile", 0)
        assert_bits(dev.spmm(X), Y_ref)
    for bad in (3, 64, -1, 12):
        with pytest.raises(sp.Panic, match="spmm_tile"):
            dev.set_option("spmm_tile", bad)
    assert_bits(dev.spmm(X), Y_ref)          # still usable, still automatic


# ---- 4. skew -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_power_law_rows(oracle, dtype, fmt):
    n = 30_000
    rp, ci, va = power_law(n, 5, dtype=dtype)
    assert int(np.diff(rp.astype(np.int64)).max()) > 3000      # (5000 drawn, duplicates merged)
    m, ref = make(fmt, oracle, n, n, rp, ci, va)
    for k in (1, 8, 13, 70):
        X = block(n, k, dtype, seed=k)
        assert_bits(m @ X, ref(X))
    d = m.device().describe()["spmm"]
    assert d["long_rows"] == int((np.diff(rp.astype(np.int64)) > d["long_row_threshold"]).sum()) > 0, d


@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_very_long_row_among_short_ones(oracle, dtype, fmt):
    n, long_row, long_len = 250_000, 1234, 200_017
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 6, n)
    lens[long_row] = long_len
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    rows = np.repeat(np.arange(n), lens)
    # strictly increasing columns in every row: a random start, then steps of one
    start = rng.integers(0, n - 6, n)
    start[long_row] = 17
    ci = (start[rows] + (np.arange(rows.size) - rp[:-1].astype(np.int64)[rows])).astype(np.uint64)
    va = rng.uniform(-1, 1, ci.size).astype(dtype)
    m, ref = make(fmt, oracle, n, n, rp, ci, va)
    for k in (3, 8):
        X = block(n, k, dtype, seed=k)
        assert_bits(m @ X, ref(X))
    assert m.device().describe()["spmm"]["long_rows"] == 1


# ---- 5. leading dimensions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_leading_dimensions_and_untouched_padding(oracle, dtype, fmt):
    n = 30_011
    rp, ci, va = synth.banded_csr(n, n, 14, 4096, 4, dtype=dtype)
    m, ref = make(fmt, oracle, n, n, rp, ci, va)
    dev = m.device()
    sfx = "f64" if dtype == np.float64 else "f32"
    fn = getattr(_ffi.lib(), f"spal_{fmt}_spmm_{sfx}")
    for k, ldx, ldy in ((5, 7, 11), (8, 8, 9), (3, 16, 3), (1, 2, 3), (20, 21, 33)):
        Xw = block(n, ldx, dtype, seed=ldx)
        Yw = np.full((n, ldy), np.nan, dtype=dtype)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _ffi.check(fn(dev._h, C.c_uint64(k), p(Xw), C.c_uint64(ldx), C.c_uint64(n), p(Yw), C.c_uint64(ldy),
                      C.c_uint64(n)))
        assert_bits(Yw[:, :k], ref(Xw[:, :k]))
        assert np.isnan(Yw[:, k:]).all()          # the padding is still the NaN that was put there


@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_torch_column_slice_and_padded_out(oracle, dtype, fmt):
    import torch
    n = 20_003
    rp, ci, va = synth.banded_csr(n, n, 14, 4096, 6, dtype=dtype)
    m, ref = make(fmt, oracle, n, n, rp, ci, va)
    dev = m.device()
    Xw = block(n, 9, dtype)
    Xt = torch.from_numpy(Xw).cuda()
    Y = dev.spmm_torch(Xt[:, 2:6])                 # stride(0) = 9, k = 4: no copy
    torch.cuda.synchronize()
    Y_ref = ref(Xw[:, 2:6])
    assert tuple(Y.shape) == (n, 4)
    assert_bits(Y.cpu().numpy(), Y_ref)
    out = torch.full((n, 11), float("nan"), dtype=Xt.dtype, device="cuda")
    assert dev.spmm_torch(Xt[:, 2:6], out=out[:, 3:7]) is not None
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert_bits(o[:, 3:7], Y_ref)
    assert np.isnan(o[:, :3]).all() and np.isnan(o[:, 7:]).all()
    with pytest.raises(sp.Panic, match="ncols == rhs.nrows"):
        dev.spmm_torch(Xt[:-1])
    with pytest.raises(sp.Panic, match="unit stride"):
        dev.spmm_torch(Xt[:, ::2])
    with pytest.raises(sp.Panic):
        dev.spmm_torch(Xt.to(torch.float32 if dtype == np.float64 else torch.float64))


# ---- 6. special values ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(oracle, dtype, fmt):
    fi = np.finfo(dtype)
    sub = fi.smallest_subnormal
    nrows, ncols = 8, 6
    rows = [
        [(2, -3.5)],                                   # X[2] = 0.0: the only product is -v * 0.0 = -0.0, assigned
        [(1, np.inf)],                                 # X[1] = 0.0 in column 0: inf * 0 = NaN
        [(0, -0.0), (3, 1.0)],                         # -0.0 * x first, then + a finite product
        [(0, sub), (4, sub * 3)],                      # subnormal values
        [(3, fi.max), (4, fi.max), (5, -fi.max)],      # overflow to +inf, then inf - big = inf
        [(0, np.inf), (5, -np.inf)],                   # inf - inf = NaN where both X are positive
        [],                                            # +0.0
        [(1, np.nan), (2, 1.0)],
    ]
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    ci = np.array([c for r in rows for c, _ in r], dtype=np.uint64)
    va = np.array([v for r in rows for _, v in r], dtype=dtype)
    X = np.array([[1.0, -0.0, sub, 0.5],
                  [0.0, 2.0, -np.inf, np.nan],
                  [0.0, -0.0, 1.0, sub],
                  [1.5, sub, -1.0, 0.25],
                  [2.0, 0.5, sub * 2, -0.0],
                  [1.0, 3.0, 0.0, np.inf]], dtype=dtype)
    m, ref = make(fmt, oracle, nrows, ncols, rp, ci, va)
    Y_ref = ref(X)
    assert np.signbit(Y_ref[0, 0]) and Y_ref[0, 0] == 0.0 and np.isnan(Y_ref[1, 0])      # (the cases are what they say)
    assert not np.signbit(Y_ref[6]).any() and np.isnan(Y_ref[5, 0]) and np.isinf(Y_ref[4, 0])
    dev = m.device()
    for tile in (0,) + TILES:
        dev.set_option("spmm_tile", tile)
        assert_bits(dev.spmm(X), Y_ref)
    assert_bits(m @ X, Y_ref)


# ---- 7. row-block handle ------------------------------------------------------------------------------------------------
def test_row_block_handle(oracle, monkeypatch):
    monkeypatch.setenv("SPAL_CSR_PART_ENTRIES", "300000")
    n = 200_000 + 37
    rp, ci, va = synth.banded_csr(n, n, 14, 4096, 3)
    a = sp.CsrMatrix(n, n, rp, ci, va)
    dev = a.device()
    d = dev.describe()
    assert d["kernel"] == "row_blocks" and d["parts"] >= 9, d
    X = block(n, 8, np.float64)
    Y_ref = csr_ref(oracle, rp, ci, va, X)
    assert_bits(a @ X, Y_ref)
    Yw = np.full((n, 10), np.nan)
    _ffi.check(_ffi.lib().spal_csr_spmm_f64(dev._h, C.c_uint64(8), X.ctypes.data_as(C.c_void_p), C.c_uint64(8),
                                            C.c_uint64(n), Yw.ctypes.data_as(C.c_void_p), C.c_uint64(10), C.c_uint64(n)))
    assert_bits(Yw[:, :8], Y_ref)
    assert np.isnan(Yw[:, 8:]).all()
    s = dev.describe()["spmm"]
    assert s["k"] == 8 and s["tile"] == 8, s


# ---- 8. device-assembled handle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_first_product_on_a_device_assembled_handle(oracle, dtype):
    n = 40_000
    r, c, v = synth.coo(n, n, 500_000, synth.matrix_seed(5), 10, 1, dtype=dtype)
    csr = sp.CsrMatrix.from_coo(sp.CooMatrix.with_triplets(n, n, r, c, v))
    X = block(n, 6, dtype)
    Y = csr @ X                                   # the first product of any kind on this handle
    assert_bits(Y, csr_ref(oracle, csr.rowptr(), csr.colind(), csr.values(), X))
    csc = sp.CscMatrix.from_coo(sp.CooMatrix.with_triplets(n, n, r, c, v))
    assert_bits(csc @ X, csc_ref(oracle, n, csc.colptr(), csc.rowind(), csc.values(), X))


# ---- 9. streams and threads -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_non_default_stream_and_concurrent_callers(oracle, fmt):
    import torch
    n = 60_000
    rp, ci, va = synth.banded_csr(n, n, 14, 4096, 8)
    m, ref = make(fmt, oracle, n, n, rp, ci, va)
    dev = m.device()
    X = block(n, 6, np.float64)
    Xt = torch.from_numpy(X).cuda()
    Yt = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    dev.spmm_dev(6, Xt.data_ptr(), 6, Yt.data_ptr(), 6, stream=st)
    st.synchronize()
    assert_bits(Yt.cpu().numpy(), ref(X))

    ks = (3, 8, 17, 2)
    Xs = [block(n, k, np.float64, seed=100 + k) for k in ks]
    refs = [ref(x) for x in Xs]
    Xts = [torch.from_numpy(x).cuda() for x in Xs]
    torch.cuda.synchronize()
    outs, errs = [None] * len(ks), []

    def work(i):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(5):
                    y = dev.spmm_torch(Xts[i])
            s.synchronize()
            outs[i] = y.cpu().numpy()
        except Exception as e:      # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(ks))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for got, want in zip(outs, refs):
        assert_bits(got, want)


# ---- 10. error paths with a live handle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_error_paths_leave_the_handle_usable(oracle, fmt):
    import torch
    n = 5000
    rp, ci, va = synth.banded_csr(n, n, 14, 4096, 2)
    m, ref = make(fmt, oracle, n, n, rp, ci, va)
    dev = m.device()
    L = _ffi.lib()
    X = block(n, 4, np.float64)
    Y = np.empty((n, 4))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    u = C.c_uint64
    host, host32 = getattr(L, f"spal_{fmt}_spmm_f64"), getattr(L, f"spal_{fmt}_spmm_f32")
    devf = getattr(L, f"spal_{fmt}_spmm_dev_f64")

    def bad(status_call, text):
        assert status_call == _ffi.SPAL_ERR_INVALID_ARGUMENT
        assert text in L.spal_last_error().decode(), L.spal_last_error()

    bad(host(dev._h, u(0), p(X), u(4), u(n), p(Y), u(4), u(n)), "k = 0")
    bad(host(dev._h, u(4), p(X), u(3), u(n), p(Y), u(4), u(n)), "ldx = 3 is less than k = 4")
    bad(host(dev._h, u(4), p(X), u(4), u(n), p(Y), u(2), u(n)), "ldy = 2 is less than k = 4")
    bad(host(dev._h, u(4), p(X), u(4), u(n - 1), p(Y), u(4), u(n)),
        f"assertion failed: ncols == rhs.nrows (left: {n}, right: {n - 1})")
    bad(host(dev._h, u(4), p(X), u(4), u(n), p(Y), u(4), u(n + 1)), f"Y has {n + 1} rows but nrows = {n}")
    bad(host(dev._h, u(4), None, u(4), u(n), p(Y), u(4), u(n)), "null")
    bad(host32(dev._h, u(4), p(X), u(4), u(n), p(Y), u(4), u(n)), "handle holds f64 values")
    bad(devf(dev._h, u(0), C.c_void_p(8), u(4), C.c_void_p(8), u(4), None), "k = 0")
    bad(devf(dev._h, u(4), C.c_void_p(8), u(3), C.c_void_p(8), u(4), None), "ldx = 3")
    bad(devf(dev._h, u(4), C.c_void_p(8), u(4), C.c_void_p(8), u(3), None), "ldy = 3")
    bad(devf(dev._h, u(4), None, u(4), C.c_void_p(8), u(4), None), "null")
    bad(getattr(L, f"spal_{fmt}_spmm_dev_f32")(dev._h, u(4), C.c_void_p(8), u(4), C.c_void_p(8), u(4), None),
        "handle holds f64 values")
    buf = torch.zeros((n + 1, 6), dtype=torch.float64, device="cuda")
    with pytest.raises(sp.Panic, match="overlaps"):
        dev.spmm_torch(buf[:n], out=buf[1:])
    with pytest.raises(sp.Panic, match="overlaps"):
        dev.spmm_torch(buf[:n, :3], out=buf[:n, 2:5])     # column ranges of one buffer that share column 2
    with pytest.raises(sp.Panic, match="overlaps"):
        dev.spmm_torch(buf[:n, 4:6], out=buf.view(-1)[5:5 + 6 * n].view(n, 6)[:, 0:2])    # ... or do, a row apart
    buf[:n, :2] = torch.from_numpy(X[:, :2]).cuda()
    dev.spmm_torch(buf[:n, :2], out=buf[:n, 3:5])         # disjoint column ranges of one buffer are fine
    torch.cuda.synchronize()
    assert_bits(buf[:n, 3:5].cpu().numpy(), ref(X[:, :2]))
    with pytest.raises(sp.Panic, match=r"ncols == rhs.nrows \(left: 5000, right: 4999\)"):
        m @ X[:-1]
    with pytest.raises(TypeError):
        m @ np.ones((n, 2, 2))
    assert_bits(m @ X, ref(X))                      # after all that: still right
    assert json.dumps(dev.describe()["spmm"])


# ---- CSC handles on the scatter route; graph capture ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_csc_scatter_route_handle_still_multiplies_on_the_csr_twin(oracle, dtype):
    n = 30_000
    rp, ci, va = synth.banded_csr(n, n, 14, 4096, 9, dtype=dtype)
    m, ref = make("csc", oracle, n, n, rp, ci, va)
    dev = m.device()
    dev.set_option("kernel", 1)               # SpMV by atomic scatter from now on; SpMM has no such form
    X = block(n, 6, dtype)
    assert_bits(dev.spmm(X), ref(X))
    assert dev.describe()["spmm"]["k"] == 6
    dev.spmv(np.ascontiguousarray(X[:, 0]))   # the handle's own product still runs


def test_first_call_on_a_device_assembled_handle_inside_a_graph_capture(oracle):
    import torch
    n = 20_000
    r, c, v = synth.coo(n, n, 200_000, synth.matrix_seed(5), 10, 1)
    csr = sp.CsrMatrix.from_coo(sp.CooMatrix.with_triplets(n, n, r, c, v))
    dev = csr.device()
    X = block(n, 8, np.float64)
    Xt = torch.from_numpy(X).cuda()
    Yt = torch.full((n, 8), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):             # nothing ran on the handle before: no plan is needed, none is built
        dev.spmm_torch(Xt, out=Yt)
    graph.replay()
    torch.cuda.synchronize()
    assert_bits(Yt.cpu().numpy(), csr_ref(oracle, csr.rowptr(), csr.colind(), csr.values(), X))
