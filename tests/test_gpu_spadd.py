"""GPU: C = A + B, A - B and -A for CSR and CSC (spal_csr_add / _sub / _neg, spal_csc_*) against the CPU restatement
of the reference's operators (tests/spadd_ref.py).  Every comparison is exact: indices equal, values equal as raw bits
(NaN by position: a NaN's payload is not part of the contract)."""
import json
import os
import threading

import numpy as np
import pytest

import spalinalg_amd as sp
import spal_synth as synth
from spalinalg_amd import _ffi
from tests import spadd_ref
from tests.util import assert_spmv_close, random_csr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_MIN = 16


def assert_same(got, ref):
    (gp, gi, gv), (rp, ri, rv) = got, ref
    assert np.array_equal(np.asarray(gp, dtype=np.uint64), np.asarray(rp, dtype=np.uint64))
    assert np.array_equal(np.asarray(gi, dtype=np.uint64), np.asarray(ri, dtype=np.uint64))
    gv, rv = np.asarray(gv), np.asarray(rv)
    assert gv.dtype == rv.dtype and gv.shape == rv.shape
    gn, rn = np.isnan(gv), np.isnan(rv)
    assert np.array_equal(gn, rn)
    bits = np.uint64 if gv.dtype == np.float64 else np.uint32
    assert np.array_equal(gv[~gn].view(bits), rv[~rn].view(bits))


def arrays(m):
    if isinstance(m, sp.CsrMatrix):
        return m.rowptr(), m.colind(), m.values()
    return m.colptr(), m.rowind(), m.values()


def matrix(fmt, nmajor, nminor, arr):
    """a CsrMatrix (nmajor x nminor) or a CscMatrix (nminor x nmajor) over arrays compressed by the major index"""
    return sp.CsrMatrix(nmajor, nminor, *arr) if fmt == "csr" else sp.CscMatrix(nminor, nmajor, *arr)


def device_op(fmt, op, nmajor, nminor, a, b, tile=0):
    """the device result (options on the left operand) and the restatement's arrays"""
    A, B = matrix(fmt, nmajor, nminor, a), matrix(fmt, nmajor, nminor, b)
    if tile:
        A.device().set_option("spadd_tile", tile)
    C = A + B if op == "add" else A - B
    assert type(C) is type(A) and (C.nrows(), C.ncols()) == (A.nrows(), A.ncols())
    return C, spadd_ref.add_sub_fast(nmajor, nminor, a, b, op == "sub")


@pytest.fixture(scope="module")
def ops_kats():
    with open(os.path.join(ROOT, "tests", "golden", "reference_ops_kats.json")) as f:
        return json.load(f)


def kat_matrix(m, dtype):
    if "rowptr" in m:
        return sp.CsrMatrix(m["nrows"], m["ncols"], m["rowptr"], m["colind"], np.array(m["values"], dtype=dtype))
    return sp.CscMatrix(m["nrows"], m["ncols"], m["colptr"], m["rowind"], np.array(m["values"], dtype=dtype))


# ---- 1. the reference's known-answer tests ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["csr_add", "csr_sub", "csr_neg", "csc_add", "csc_sub", "csc_neg"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_kats(ops_kats, name, dtype):
    k = ops_kats[name]
    o = k["out"]
    A = kat_matrix(k["lhs"], dtype)
    if k["op"] == "neg":
        results = [-A, type(A)._trusted(A.nrows(), A.ncols(), *A.device().neg().download())]
    else:
        B = kat_matrix(k["rhs"], dtype)
        dev = getattr(A.device(), k["op"])(B.device())
        results = [A + B if k["op"] == "add" else A - B, type(A)._trusted(A.nrows(), A.ncols(), *dev.download())]
    for C in results:
        assert (C.nrows(), C.ncols()) == (o["nrows"], o["ncols"])
        p, i, v = arrays(C)
        assert p.tolist() == o.get("rowptr", o.get("colptr")) and i.tolist() == o.get("colind", o.get("rowind"))
        assert v.dtype == dtype and v.tolist() == o["values"]


# ---- 2. random parity ------------------------------------------------------------------------------------------
def power_law(n, seed, dtype=np.float64, maxlen=5000, scale=6, half_window=5000):
    """power-law row lengths, columns near the rows; rows 1 and 2 longer than the default tile"""
    rng = np.random.default_rng(seed)
    lens = np.minimum((rng.pareto(1.6, n) * scale + 1).astype(np.int64), maxlen)
    lens[:3] = (0, maxlen, 2 * 2048 + 1)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = np.clip(rows - half_window + rng.integers(0, 2 * half_window, rows.size), 0, n - 1)
    key = np.unique(rows * n + cols)
    r2, c2 = key // n, key % n
    rp = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=n))]).astype(np.uint64)
    return rp, c2.astype(np.uint64), rng.uniform(-1, 1, c2.size).astype(dtype)


def _pair(case, dtype):
    """(nmajor, nminor, a, b) of one parity case, arrays compressed by the major index"""
    rng = np.random.default_rng(sorted(CASES).index(case) + 1)
    if case == "1x1":
        one = lambda v: (np.array([0, 1], np.uint64), np.array([0], np.uint64), np.array([v], dtype))
        return 1, 1, one(0.75), one(-0.25)
    if case == "nnz0_a":
        return 60, 50, random_csr(rng, 60, 50, density=0.5, empty_rows=1.0, dtype=dtype), random_csr(rng, 60, 50, density=0.3, dtype=dtype)
    if case == "nnz0_b":
        return 60, 50, random_csr(rng, 60, 50, density=0.3, dtype=dtype), random_csr(rng, 60, 50, density=0.5, empty_rows=1.0, dtype=dtype)
    if case == "both_empty":
        e = random_csr(rng, 60, 50, density=0.5, empty_rows=1.0, dtype=dtype)
        return 60, 50, e, e
    if case == "identical":
        a = random_csr(rng, 500, 400, density=0.05, dtype=dtype)
        return 500, 400, a, (a[0], a[1], rng.uniform(-1, 1, a[2].size).astype(dtype))
    if case == "disjoint":
        a = random_csr(rng, 500, 400, density=0.05, dtype=dtype)
        b = random_csr(rng, 500, 400, density=0.05, dtype=dtype)
        return 500, 800, (a[0], a[1] * 2, a[2]), (b[0], b[1] * 2 + 1, b[2])
    if case == "empty_rows":
        return 3000, 2500, random_csr(rng, 3000, 2500, density=0.003, empty_rows=0.4, dtype=dtype), \
            random_csr(rng, 3000, 2500, density=0.003, empty_rows=0.4, dtype=dtype)
    if case == "rows_1_400":
        rl = lambda r: r.integers(1, 401)
        return 400, 1200, random_csr(rng, 400, 1200, row_len=rl, empty_rows=0.0, dtype=dtype), \
            random_csr(rng, 400, 1200, row_len=rl, empty_rows=0.0, dtype=dtype)
    n = 20_000   # power law, rows longer than the default tile
    return n, n, power_law(n, 7, dtype), power_law(n, 8, dtype)


CASES = ("1x1", "nnz0_a", "nnz0_b", "both_empty", "identical", "disjoint", "empty_rows", "rows_1_400", "power_law")


@pytest.mark.parametrize("tile", [0, TILE_MIN])
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("op", ["add", "sub"])
@pytest.mark.parametrize("case", CASES)
def test_random_parity(case, op, dtype, fmt, tile):
    nmaj, nmin, a, b = _pair(case, dtype)
    C, ref = device_op(fmt, op, nmaj, nmin, a, b, tile)
    assert_same(arrays(C), ref)
    d = C.device().describe()["spadd"]
    assert d["op"] == op and d["nnz"] == int(ref[0][-1]) and d["tile"] == (tile or 2048)
    assert d["matched"] == spadd_ref.matched(nmaj, a, b)


# ---- 3. non-square shapes --------------------------------------------------------------------------------------
# The reference labels its transposed intermediate with the untransposed dimensions: for nrows > ncols
# its final transpose indexes out of bounds (a panic), for nrows < ncols it loses the entries in columns >= nrows and
# labels the result ncols x nrows.  The device returns the union for every shape, as the loop form with the F9 fix.
@pytest.mark.parametrize("shape", [(3, 7), (7, 3), (1, 900), (900, 1)])
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("op", ["add", "sub"])
def test_non_square_union(shape, fmt, op):
    m, n = shape
    nmaj, nmin = (m, n) if fmt == "csr" else (n, m)
    rng = np.random.default_rng(m * 7 + n)
    a = random_csr(rng, nmaj, nmin, density=0.5, empty_rows=0.2)
    b = random_csr(rng, nmaj, nmin, density=0.5, empty_rows=0.2)
    A, B = matrix(fmt, nmaj, nmin, a), matrix(fmt, nmaj, nmin, b)
    C = A + B if op == "add" else A - B
    assert (C.nrows(), C.ncols()) == (m, n)
    assert_same(arrays(C), spadd_ref.add_sub_loop(nmaj, nmin, a, b, op == "sub"))


# ---- 4. witnesses ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_minus_a_keeps_positive_zeros(fmt, dtype):
    rng = np.random.default_rng(21)
    a = random_csr(rng, 300, 300, density=0.05, dtype=dtype)
    A = matrix(fmt, 300, 300, a)
    C = A - A
    p, i, v = arrays(C)
    assert C.nnz() == A.nnz() and np.array_equal(p, a[0]) and np.array_equal(i, a[1])
    assert np.all(v == 0) and not np.signbit(v).any()
    assert C.device().describe()["spadd"]["matched"] == A.nnz()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_signed_zeros(dtype):
    z = lambda v: np.array(v, dtype=dtype)
    A = sp.CsrMatrix(1, 3, [0, 2], [0, 1], z([-0.0, 0.0]))
    B = sp.CsrMatrix(1, 3, [0, 3], [0, 1, 2], z([-0.0, -0.0, 0.0]))
    S = A + B                       # -0 + -0 = -0, +0 + -0 = +0, B-only +0 stays +0
    assert S.values().view(np.uint64 if dtype == np.float64 else np.uint32).tolist() == \
        z([-0.0, 0.0, 0.0]).view(np.uint64 if dtype == np.float64 else np.uint32).tolist()
    D = A - B                       # -0 - -0 = +0, +0 - -0 = +0, B-only +0 under Sub: -b = -0.0 (sub.rs:47)
    assert np.signbit(D.values()).tolist() == [False, False, True]
    assert D.values().tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("op", ["add", "sub"])
def test_subnormal_sums_are_bit_exact(dtype, op):
    """Subnormal operands and results: a flush to zero anywhere gives 0.0 here."""
    fi = np.finfo(dtype)
    tiny = fi.smallest_subnormal
    a_vals = np.array([3 * tiny, 5 * tiny, fi.tiny, fi.tiny, tiny], dtype=dtype)
    b_vals = np.array([tiny, 2 * tiny, np.negative(fi.tiny / 2), fi.tiny / 4, 7 * tiny], dtype=dtype)
    a = (np.array([0, 5], np.uint64), np.arange(5, dtype=np.uint64), a_vals)
    b = (np.array([0, 5], np.uint64), np.arange(5, dtype=np.uint64), b_vals)
    C, ref = device_op("csr", op, 1, 5, a, b)
    assert_same(arrays(C), ref)
    assert (np.abs(ref[2]) < fi.tiny).sum() >= 2 and np.all(ref[2] != 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_inf_minus_inf_is_nan_at_its_position(dtype):
    a = (np.array([0, 2, 3], np.uint64), np.array([0, 1, 1], np.uint64), np.array([np.inf, 1.0, -np.inf], dtype))
    b = (np.array([0, 1, 3], np.uint64), np.array([0, 0, 1], np.uint64), np.array([np.inf, 2.0, np.inf], dtype))
    for op in ("add", "sub"):
        C, ref = device_op("csr", op, 2, 2, a, b)
        assert_same(arrays(C), ref)
    C = sp.CsrMatrix(2, 2, *a) - sp.CsrMatrix(2, 2, *b)
    assert np.isnan(C.values()).tolist() == [True, False, False, False]


# ---- 5. Neg ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nnz", [0, 1, 7, 1003])
def test_neg_flips_the_sign_bit(fmt, dtype, nnz):
    fi = np.finfo(dtype)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, fi.smallest_subnormal, -fi.tiny / 3, 1.5],
                       dtype=dtype)
    rng = np.random.default_rng(nnz)
    n = 1100
    cols = np.sort(rng.choice(n, size=nnz, replace=False)).astype(np.uint64)
    ptr = np.zeros(n + 1, np.uint64)   # all entries in major line 3: the others empty
    ptr[4:] = nnz
    vals = rng.uniform(-1, 1, nnz).astype(dtype)
    vals[: min(nnz, special.size)] = special[: min(nnz, special.size)]
    A = matrix(fmt, n, n, (ptr, cols, vals))
    Ad = A.device()
    N = Ad.neg()
    Ad.close()                            # the result is independent of A's handle
    p, i, v = N.download()
    bits = np.uint64 if dtype == np.float64 else np.uint32
    sign = bits(1) << bits(63 if dtype == np.float64 else 31)
    assert np.array_equal(p, ptr) and np.array_equal(i, cols)
    assert np.array_equal(v.view(bits), vals.view(bits) ^ sign)
    d = N.describe()["spadd"]
    assert d["op"] == "neg" and d["nnz"] == nnz
    x = np.ones(n, dtype=dtype)
    y = N.spmv(x)
    assert y.shape == (n,)
    # the Python operator
    M = -matrix(fmt, n, n, (ptr, cols, vals))
    assert np.array_equal(M.values().view(bits), vals.view(bits) ^ sign)


# ---- 6. tile boundaries ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [TILE_MIN, 32, 64, 0])
@pytest.mark.parametrize("op", ["add", "sub"])
def test_pairs_straddle_tile_boundaries(tile, op):
    """Every position matched, at every offset against the tile grid (a leading A-only entry shifts the pairs by one)."""
    rng = np.random.default_rng(5)
    n = 3000
    for lead in (False, True):
        a = random_csr(rng, n, n, row_len=lambda r: r.integers(0, 9), empty_rows=0.1)
        b = (a[0], a[1], rng.uniform(-1, 1, a[2].size))
        if lead:   # an extra A-only entry in column 0 of every row whose first column is > 0
            cnt = np.diff(a[0].astype(np.int64))
            starts = a[0][:-1].astype(np.int64)
            add = (cnt == 0) | (a[1][np.minimum(starts, a[1].size - 1)] > 0)
            rows = np.repeat(np.arange(n), cnt)
            r2 = np.concatenate([rows, np.nonzero(add)[0]])
            c2 = np.concatenate([a[1].astype(np.int64), np.zeros(int(add.sum()), np.int64)])
            v2 = np.concatenate([a[2], rng.uniform(-1, 1, int(add.sum()))])
            o = np.lexsort((c2, r2))
            a = (np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=n))]).astype(np.uint64),
                 c2[o].astype(np.uint64), v2[o])
        for fmt in ("csr", "csc"):
            C, ref = device_op(fmt, op, n, n, a, b, tile)
            assert_same(arrays(C), ref)
            assert C.device().describe()["spadd"]["matched"] == b[2].size


@pytest.mark.timeout(600)
@pytest.mark.parametrize("tile", [TILE_MIN, 0])
def test_dense_row_longer_than_many_tiles(tile):
    rng = np.random.default_rng(6)
    n = 300_000
    ca = np.sort(rng.choice(n, size=200_000, replace=False)).astype(np.uint64)
    cb = np.sort(rng.choice(n, size=200_000, replace=False)).astype(np.uint64)
    # 3 rows: empty, the dense row, a short row
    a = (np.array([0, 0, 200_000, 200_003], np.uint64), np.concatenate([ca, [1, 5, 9]]).astype(np.uint64),
         rng.uniform(-1, 1, 200_003))
    b = (np.array([0, 0, 200_000, 200_001], np.uint64), np.concatenate([cb, [5]]).astype(np.uint64),
         rng.uniform(-1, 1, 200_001))
    for op in ("add", "sub"):
        for fmt in ("csr", "csc"):
            C, ref = device_op(fmt, op, 3, n, a, b, tile)
            assert_same(arrays(C), ref)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("tile", [TILE_MIN, 0])
def test_stretches_of_empty_rows(tile):
    """3M rows, a few dozen holding entries: stretches of more than 10^6 rows empty in both operands, at the head, in
    the middle and at the tail."""
    rng = np.random.default_rng(8)
    m, n = 3_000_000, 64
    def sparse_rows(rows):
        lens = np.zeros(m, np.int64)
        lens[rows] = rng.integers(1, 20, len(rows))
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        ci = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in lens[rows]]).astype(np.uint64)
        return rp, ci, rng.uniform(-1, 1, ci.size)
    rows_a = np.array(sorted({1_100_000, 1_100_001, 1_100_005} | set(range(1_200_000, 1_200_010))))
    rows_b = np.array(sorted({1_100_001, 1_100_002} | set(range(1_200_005, 1_200_020)) | {1_850_000}))
    a, b = sparse_rows(rows_a), sparse_rows(rows_b)
    for op in ("add", "sub"):
        C, ref = device_op("csr", op, m, n, a, b, tile)
        assert_same(arrays(C), ref)
        rp = arrays(C)[0]
        assert rp[0] == 0 and rp[1_000_000] == 0 and rp[-1] == rp[2_000_000] == C.nnz()


# ---- 7. the result is a full handle ----------------------------------------------------------------------------
def test_result_is_a_full_handle(oracle):
    n = 200_000
    a = synth.banded_csr(n, n, 14, 4096, 5)
    b = synth.banded_csr(n, n, 14, 4096, 6)
    A, B = sp.CsrMatrix(n, n, *a), sp.CsrMatrix(n, n, *b)
    C = A + B
    ref = spadd_ref.add_sub_fast(n, n, a, b, False)
    assert_same(arrays(C), ref)
    rp, ci, va = ref
    x = synth.vector(n)
    y_ref = oracle.csr_spmv(rp, ci, va, x)
    dev = C.device()
    d = dev.describe()
    assert d["spadd"]["nnz"] == int(rp[-1]) and d["spadd"]["matched"] == spadd_ref.matched(n, a, b)
    assert d["spadd"]["kernel_ms"] > 0 and d["spadd"]["tiles"] == -(-(int(a[0][-1]) + int(b[0][-1])) // 2048)
    y = dev.spmv(x)
    if d.get("stream_row_fraction") == 1.0:
        assert np.array_equal(y.view(np.uint64), y_ref.view(np.uint64))
    else:   # (super-tiles of the vector fallback agree to rounding, as in the SpMV tests)
        assert_spmv_close(y, y_ref, oracle.csr_abs_bound(rp, ci, va, x), 1e-10)
    assert_same(dev.to_csc().download(), oracle.transpose(n, n, rp, ci, va))
    assert_same(arrays(C * A), oracle.csr_mul((n, n), ref, (n, n), a))
    D = C - B
    assert_same(arrays(D), spadd_ref.add_sub_fast(n, n, ref, b, True))
    assert "spadd" not in A.device().describe()


@pytest.mark.timeout(600)
def test_skewed_result_plans_eagerly(oracle):
    """A sum whose rows are skewed enough for the row split: the result is planned inside the call (a lazily planned
    handle could reach the block-window / split decision re-entrantly); a hang fails this test."""
    n = 400_000
    a = power_law(n, 11)
    z = (np.zeros(n + 1, np.uint64), np.zeros(0, np.uint64), np.zeros(0))
    C = sp.CsrMatrix(n, n, *a) + sp.CsrMatrix(n, n, *z)     # (A + 0 = A, bit for bit)
    assert_same(arrays(C), a)
    dev = C.device()
    d = dev.describe()
    assert d["kernel"] in ("split", "blockwin"), d
    assert d["spadd"]["plan_ms"] > 0
    x = synth.vector(n)
    rp, ci, va = a
    assert_spmv_close(dev.spmv(x), oracle.csr_spmv(rp, ci, va, x), oracle.csr_abs_bound(rp, ci, va, x), 1e-10)


# ---- 8. concurrency and streams --------------------------------------------------------------------------------
def test_two_threads_same_operands():
    rng = np.random.default_rng(9)
    n = 20_000
    a = random_csr(rng, n, n, row_len=lambda r: r.integers(0, 40))
    b = random_csr(rng, n, n, row_len=lambda r: r.integers(0, 40))
    da, db = sp.CsrMatrix(n, n, *a).device(), sp.CsrMatrix(n, n, *b).device()
    out = [None] * 4

    def work(k):
        out[k] = (da.add(db) if k % 2 == 0 else da.sub(db)).download()

    th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(4):
        assert_same(out[k], spadd_ref.add_sub_fast(n, n, a, b, k % 2 == 1))


def test_user_stream():
    import torch
    rng = np.random.default_rng(10)
    n = 20_000
    a = random_csr(rng, n, n, row_len=lambda r: r.integers(0, 40), dtype=np.float32)
    b = random_csr(rng, n, n, row_len=lambda r: r.integers(0, 40), dtype=np.float32)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        C = sp.CsrMatrix(n, n, *a).device().sub(sp.CsrMatrix(n, n, *b).device(), stream=s)
        Cc = sp.CscMatrix(n, n, *a).device().add(sp.CscMatrix(n, n, *b).device(), stream=s)
        N = sp.CsrMatrix(n, n, *a).device().neg(stream=s)
    assert_same(C.download(), spadd_ref.add_sub_fast(n, n, a, b, True))
    assert_same(Cc.download(), spadd_ref.add_sub_fast(n, n, a, b, False))
    assert_same(N.download(), spadd_ref.neg(a))


# ---- 9. size ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_banded_1m_seeds_3_and_4():
    n = 1_000_000
    a = synth.banded_csr(n, n, 14, 4096, synth.matrix_seed(3))
    b = synth.banded_csr(n, n, 14, 4096, synth.matrix_seed(4))
    A, B = sp.CsrMatrix(n, n, *a), sp.CsrMatrix(n, n, *b)
    for op in ("add", "sub"):
        C = A + B if op == "add" else A - B
        ref = spadd_ref.add_sub_fast(n, n, a, b, op == "sub")
        assert_same(arrays(C), ref)
        assert C.device().describe()["spadd"]["matched"] == spadd_ref.matched(n, a, b)


# ---- 10. errors ------------------------------------------------------------------------------------------------
def test_errors(monkeypatch):
    a = sp.CsrMatrix(2, 3, [0, 1, 2], [0, 2], np.array([1.0, 2.0]))
    b = sp.CsrMatrix(3, 2, [0, 1, 1, 2], [0, 1], np.array([1.0, 2.0]))
    c = sp.CsrMatrix(2, 2, [0, 1, 2], [0, 1], np.array([1.0, 2.0]))
    # the two shape assertions, in their order, through the device entry points
    with pytest.raises(sp.Panic, match=r"assertion failed: nrows == rhs.nrows \(left: 2, right: 3\)"):
        a.device().add(b.device())
    with pytest.raises(sp.Panic, match=r"assertion failed: ncols == rhs.ncols \(left: 3, right: 2\)"):
        a.device().sub(c.device())
    ac = sp.CscMatrix(2, 3, [0, 1, 1, 2], [0, 1], np.array([1.0, 2.0]))
    bc = sp.CscMatrix(3, 2, [0, 1, 2], [0, 2], np.array([1.0, 2.0]))
    with pytest.raises(sp.Panic, match=r"nrows == rhs.nrows \(left: 2, right: 3\)"):
        ac.device().add(bc.device())
    # mixed element sizes
    a32 = sp.CsrMatrix(2, 3, [0, 1, 2], [0, 2], np.array([1.0, 2.0], dtype=np.float32))
    with pytest.raises(sp.Panic, match="element sizes"):
        a + a32
    with pytest.raises(sp.Panic, match="element sizes"):
        sp.CscMatrix(2, 3, [0, 1, 1, 2], [0, 1], np.array([1.0, 2.0], dtype=np.float32)) - ac
    # row-block operands (more entries than one set of 32-bit offsets; the limit lowered for the test)
    monkeypatch.setenv("SPAL_CSR_PART_ENTRIES", "3000")
    rp, ci, va = synth.banded_csr(2000, 2000, 4, 64, 3)
    big = sp.CsrMatrix(2000, 2000, rp, ci, va)
    assert big.device().describe()["kernel"] == "row_blocks"
    monkeypatch.delenv("SPAL_CSR_PART_ENTRIES")
    small = sp.CsrMatrix(2000, 2000, rp, ci, va)
    for lhs, rhs in ((big, small), (small, big)):
        for f in (lambda x, y: x + y, lambda x, y: x - y):
            with pytest.raises(sp.SpalError) as e:
                f(lhs, rhs)
            assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED
    with pytest.raises(sp.SpalError) as e:
        -big
    assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED
    # the option: 0 or a power of two in [16, 2048]
    for fmt_dev in (small.device(), sp.CscMatrix(2, 3, [0, 1, 1, 2], [0, 1], np.array([1.0, 2.0])).device()):
        for bad in (-1, 3, 8, 100, 4096, 1 << 20):
            with pytest.raises(sp.Panic, match="spadd_tile"):
                fmt_dev.set_option("spadd_tile", bad)
        for good in (0, 16, 256, 2048):
            fmt_dev.set_option("spadd_tile", good)
