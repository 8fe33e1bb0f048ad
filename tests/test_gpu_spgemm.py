"""GPU: C = A * B, sparse x sparse (spal_csr_mul / spal_csc_mul) against the oracle's literal restatement of the
reference's `Mul` (oracle.csr_mul / oracle.csc_mul).  Every comparison is exact: indices equal, values equal as raw
bits (NaN by position: a NaN's payload is not part of the contract)."""
import threading

import numpy as np
import pytest

import spalinalg_amd as sp
import spal_synth as synth
from spalinalg_amd import _ffi
from tests import spgemm_cases
from tests.util import assert_spmv_close, random_csr

pytestmark = pytest.mark.gpu

LDS_TIERS = ("g16", "g32", "wave", "block4k", "block8k")


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


def csr_product(oracle, a_shape, a, b_shape, b, **opts):
    """device CSR product (options on the left operand) and the oracle's; returns (C, reference arrays)"""
    A, B = sp.CsrMatrix(*a_shape, *a), sp.CsrMatrix(*b_shape, *b)
    for k, v in opts.items():
        A.device().set_option(k, v)
    C = A * B
    assert (C.nrows(), C.ncols()) == (a_shape[0], b_shape[1])
    return C, oracle.csr_mul(a_shape, a, b_shape, b)


# ---- 1. the reference's known-answer test ----------------------------------------------------------------------
def test_g5_csc_mul(kats, oracle):
    g = kats["G5_csc_mul"]
    a, b, o = g["lhs"], g["rhs"], g["out"]
    for dt in (np.float64, np.float32):
        A = sp.CscMatrix(a["nrows"], a["ncols"], a["colptr"], a["rowind"], np.array(a["values"], dtype=dt))
        B = sp.CscMatrix(b["nrows"], b["ncols"], b["colptr"], b["rowind"], np.array(b["values"], dtype=dt))
        C = A * B
        assert isinstance(C, sp.CscMatrix) and (C.nrows(), C.ncols()) == (o["nrows"], o["ncols"])
        assert C.colptr().tolist() == o["colptr"] and C.rowind().tolist() == o["rowind"]
        assert C.values().tolist() == o["values"] and C.values().dtype == dt
        # the CSR form of the same product equals the transpose of `out`
        ar = oracle.transpose(a["ncols"], a["nrows"], a["colptr"], a["rowind"], np.array(a["values"], dtype=dt))
        br = oracle.transpose(b["ncols"], b["nrows"], b["colptr"], b["rowind"], np.array(b["values"], dtype=dt))
        Cr = sp.CsrMatrix(a["nrows"], a["ncols"], *ar) @ sp.CsrMatrix(b["nrows"], b["ncols"], *br)
        ref = oracle.transpose(o["ncols"], o["nrows"], o["colptr"], o["rowind"], np.array(o["values"], dtype=dt))
        assert_same(arrays(Cr), ref)


# ---- 2. random parity ------------------------------------------------------------------------------------------
CASES = {
    "1x1": (1, 1, 1, dict(density=1.0, empty_rows=0.0), dict(density=1.0, empty_rows=0.0)),
    "nnz0_a": (7, 5, 6, dict(density=0.5, empty_rows=1.0), dict(density=0.5)),
    "nnz0_b": (7, 5, 6, dict(density=0.5), dict(density=0.5, empty_rows=1.0)),
    "empty_rows": (200, 150, 170, dict(density=0.05, empty_rows=0.4), dict(density=0.05, empty_rows=0.4)),
    "rectangular": (37, 53, 29, dict(density=0.2), dict(density=0.3)),
    "long_b_rows": (300, 200, 3000, dict(row_len=lambda r: r.integers(1, 6)),
                    dict(row_len=lambda r: r.integers(1, 400), empty_rows=0.05)),
    "thousands": (3000, 2500, 2800, dict(density=0.004), dict(density=0.004)),
}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", sorted(CASES))
def test_random_parity(oracle, case, dtype):
    m, n, p, ka, kb = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case) + 1)
    a = random_csr(rng, m, n, dtype=dtype, **ka)
    b = random_csr(rng, n, p, dtype=dtype, **kb)
    C, ref = csr_product(oracle, (m, n), a, (n, p), b)
    assert_same(arrays(C), ref)
    # CSC: the same arrays read as the CSC arrays of A^T (n x m) and B^T (p x n): B^T * A^T = (AB)^T
    Ct = sp.CscMatrix(p, n, *b) * sp.CscMatrix(n, m, *a)
    assert_same(arrays(Ct), oracle.csc_mul((p, n), b, (n, m), a))
    assert_same(arrays(Ct), ref)       # (the CSC arrays of (AB)^T are the CSR arrays of AB)


def test_zero_dimensions_are_refused_at_construction():
    """m, n or p = 0: CsrMatrix::new asserts nrows > 0 and ncols > 0 (src/csr.rs:144-156), so no operand of a product
    can have a zero dimension -- the binding refuses it where the reference panics."""
    for shape, ptr in (((0, 3), [0]), ((3, 0), [0, 0, 0, 0])):
        with pytest.raises(sp.Panic):
            sp.CsrMatrix(*shape, ptr, [], np.array([]))
        with pytest.raises(sp.Panic):
            sp.CscMatrix(shape[1], shape[0], ptr, [], np.array([]))


# ---- 3. semantics ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_exact_zero_sum_is_kept(oracle, dtype):
    A = sp.CsrMatrix(1, 2, [0, 2], [0, 1], np.array([1, 1], dtype=dtype))
    B = sp.CsrMatrix(2, 1, [0, 1, 2], [0, 0], np.array([1, -1], dtype=dtype))
    C = A * B
    assert C.nnz() == 1 and C.colind().tolist() == [0]
    assert C.values()[0] == 0 and not np.signbit(C.values()[0])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lone_negative_times_zero_is_negative_zero(dtype):
    A = sp.CsrMatrix(1, 1, [0, 1], [0], np.array([-1], dtype=dtype))
    B = sp.CsrMatrix(1, 1, [0, 1], [0], np.array([0], dtype=dtype))
    C = A * B
    assert C.nnz() == 1 and C.values()[0] == 0 and np.signbit(C.values()[0])


def _order_witness(blen, dtype=np.float64):
    """Row 0 of A = [1e16, -1e16, 1] at k = 0, 1, 2; B's rows 0..2 hold `blen` entries each, with 1.0 at column j.
    C[0, j] = ((1e16 - 1e16) + 1) = 1 only in k order; any order that does not add the 1 last gives 0."""
    rng = np.random.default_rng(blen)
    j = blen // 2 + 3
    a = (np.array([0, 3], dtype=np.uint64), np.array([0, 1, 2], dtype=np.uint64), np.array([1e16, -1e16, 1.0], dtype=dtype))
    rows = []
    for _ in range(3):
        cols = np.sort(rng.choice(np.arange(blen + 8), size=blen, replace=False))
        if j not in cols:
            cols[np.argmin(np.abs(cols - j))] = j
            cols = np.unique(cols)
        rows.append(cols)
    bp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.uint64)
    bc = np.concatenate(rows).astype(np.uint64)
    bv = rng.uniform(-1, 1, bc.size).astype(dtype)
    bv[bc == j] = 1.0
    return a, (bp, bc, bv), blen + 8, j


@pytest.mark.parametrize("blen,opts,tier", [
    (1, {}, "g16"),                                   # a short row
    (80, {}, "g32"),                                  # B rows longer than a group of 32: three steps per k
    (300, {}, "wave"),                                # ... than a wave: five steps per k
    (300, {"spgemm_route": 2}, "large"),              # forced to the large-row tier
    (80, {"spgemm_lds_cap": 16}, "large"),
])
def test_order_witness(oracle, blen, opts, tier):
    a, b, p, j = _order_witness(blen)
    C, ref = csr_product(oracle, (1, 3), a, (3, p), b, **opts)
    assert_same(arrays(C), ref)
    row = dict(zip(C.colind().tolist(), C.values().tolist()))
    assert row[j] == 1.0
    d = C.device().describe()["spgemm"]
    assert d["tier_rows"][tier] == 1, d


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_inf_and_nan_inputs(oracle, dtype):
    rng = np.random.default_rng(5)
    a = random_csr(rng, 300, 200, density=0.05, dtype=dtype)
    b = random_csr(rng, 200, 250, density=0.05, dtype=dtype)
    for arr in (a[2], b[2]):
        idx = rng.choice(arr.size, size=12, replace=False)
        arr[idx[:4]] = np.inf
        arr[idx[4:8]] = -np.inf
        arr[idx[8:]] = np.nan
    C, ref = csr_product(oracle, (300, 200), a, (200, 250), b)
    assert np.isnan(ref[2]).any() and np.isinf(ref[2]).any()
    assert_same(arrays(C), ref)


# ---- 4. every route, bit for bit -------------------------------------------------------------------------------
def power_law(n, seed, dtype=np.float64, maxlen=3000, scale=4, half_window=2000):
    """power-law row lengths, columns near the rows (the generator of the row-split SpMV test)"""
    rng = np.random.default_rng(seed)
    lens = np.minimum((rng.pareto(1.6, n) * scale + 1).astype(np.int64), maxlen)
    lens[:3] = (0, maxlen, 129)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = np.clip(rows - half_window + rng.integers(0, 2 * half_window, rows.size), 0, n - 1)
    key = np.unique(rows * n + cols)
    r2, c2 = key // n, key % n
    rp = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=n))]).astype(np.uint64)
    return rp, c2.astype(np.uint64), rng.uniform(-1, 1, c2.size).astype(dtype)


def power_law_operand_arrays(synth):
    """(n, power-law A, banded B); tests/test_spgemm_cases_host.py checks on the CPU that under route 1 both A * A and
    A * B put a row in every LDS tier"""
    n = 50_000
    a = power_law(n, 17)
    b = synth.banded_csr(n, n, 14, 4096, 3)
    return n, a, b


@pytest.fixture(scope="module")
def power_law_operands():
    return power_law_operand_arrays(synth)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("rhs", ["self", "banded"])
def test_every_route_bit_for_bit(oracle, power_law_operands, rhs):
    n, a, banded = power_law_operands
    b = a if rhs == "self" else banded
    ref = oracle.csr_mul((n, n), a, (n, n), b)
    route_of = {"auto": (0, 0), "lds": (1, 0), "large": (2, 0), "cap": (0, 48)}
    runs = {}
    for name, opts in (("auto", {}), ("lds", {"spgemm_route": 1}), ("large", {"spgemm_route": 2}),
                       ("cap", {"spgemm_lds_cap": 48})):
        A, B = sp.CsrMatrix(n, n, *a), sp.CsrMatrix(n, n, *b)
        for k, v in opts.items():
            A.device().set_option(k, v)
        C = A * B
        assert_same(arrays(C), ref)
        d = C.device().describe()["spgemm"]
        assert d["nnz"] == int(ref[0][-1]) and d["products"] > 0 and d["plan_ms"] >= 0, d
        t = d["tier_rows"]
        assert sum(t.values()) == n
        assert spgemm_cases.reported(d) == spgemm_cases.expected(a, b, *route_of[name], nnz=int(ref[0][-1])), d
        if name == "auto":
            assert t["g16"] > 0 and t["large"] > 0, t
        elif name == "lds":
            assert sum(t[k] for k in LDS_TIERS) > 0 and t["block8k"] + t["large"] > 0, t
            assert all(t[k] > 0 for k in LDS_TIERS), t
        elif name == "large":
            assert d["route"] == 2 and sum(t[k] for k in LDS_TIERS) == 0 and t["large"] == n - t["empty"], t
        else:
            assert t["g16"] > 0 and t["g32"] == t["wave"] == t["block4k"] == t["block8k"] == 0 and t["large"] > 0, t
        runs[name] = arrays(C)
    for name in runs:
        assert_same(runs[name], runs["auto"])


# ---- 5. the result is a full handle ----------------------------------------------------------------------------
def test_result_is_a_full_handle(oracle):
    n = 200_000
    a = synth.banded_csr(n, n, 14, 4096, 5)
    C = sp.CsrMatrix(n, n, *a) * sp.CsrMatrix(n, n, *a)
    rp, ci, va = arrays(C)
    x = synth.vector(n)
    y_ref = oracle.csr_spmv(rp, ci, va, x)
    dev = C.device()
    d = dev.describe()
    y = dev.spmv(x)
    if d.get("stream_row_fraction") == 1.0:
        assert np.array_equal(y.view(np.uint64), y_ref.view(np.uint64))
    else:   # (super-tiles of the vector fallback agree to rounding, as in the SpMV tests)
        assert_spmv_close(y, y_ref, oracle.csr_abs_bound(rp, ci, va, x), 1e-10)
    csc = dev.to_csc()
    assert_same(csc.download(), oracle.transpose(n, n, rp, ci, va))


@pytest.mark.timeout(600)
def test_skewed_result_plans_eagerly(oracle):
    """A product whose rows are skewed enough for the row split: the result is planned inside the call (a lazily
    planned handle could reach the block-window / split decision re-entrantly); a hang fails this test."""
    n = 400_000
    a = power_law(n, 11, maxlen=5000, scale=6, half_window=5000)
    e = sp.CsrMatrix.eye(n)
    C = sp.CsrMatrix(n, n, *a) * e          # (A * I = A, bit for bit)
    assert_same(arrays(C), a)
    dev = C.device()
    d = dev.describe()
    assert d["kernel"] in ("split", "blockwin"), d
    assert d["spgemm"]["plan_ms"] > 0
    x = synth.vector(n)
    rp, ci, va = a
    assert_spmv_close(dev.spmv(x), oracle.csr_spmv(rp, ci, va, x), oracle.csr_abs_bound(rp, ci, va, x), 1e-10)


# ---- 6. concurrency and streams --------------------------------------------------------------------------------
def test_two_threads_same_operands(oracle):
    rng = np.random.default_rng(9)
    n = 20_000
    a = random_csr(rng, n, n, row_len=lambda r: r.integers(0, 40))
    A, B = sp.CsrMatrix(n, n, *a), sp.CsrMatrix(n, n, *a)
    da, db = A.device(), B.device()
    out = [None, None]

    def work(k):
        out[k] = da.mul(db).download()

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    ref = oracle.csr_mul((n, n), a, (n, n), a)
    assert_same(out[0], ref)
    assert_same(out[1], ref)


def test_user_stream(oracle):
    import torch
    rng = np.random.default_rng(10)
    n = 20_000
    a = random_csr(rng, n, n, row_len=lambda r: r.integers(0, 40), dtype=np.float32)
    A = sp.CsrMatrix(n, n, *a)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        C = A.device().mul(A.device(), stream=s)
    assert_same(C.download(), oracle.csr_mul((n, n), a, (n, n), a))
    Cc = sp.CscMatrix(n, n, *a).device().mul(sp.CscMatrix(n, n, *a).device(), stream=s)
    assert_same(Cc.download(), oracle.csc_mul((n, n), a, (n, n), a))


# ---- 7. size ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_banded_1m_a_times_a(oracle):
    n = 1_000_000
    a = synth.banded_csr(n, n, 14, 4096, synth.matrix_seed(3))
    A = sp.CsrMatrix(n, n, *a)
    C = A * A
    d = C.device().describe()["spgemm"]
    assert d["products"] == 196 * n
    assert_same(arrays(C), oracle.csr_mul((n, n), a, (n, n), a))


# ---- 8. errors -------------------------------------------------------------------------------------------------
def test_errors(monkeypatch):
    a = sp.CsrMatrix(2, 3, [0, 1, 2], [0, 2], np.array([1.0, 2.0]))
    with pytest.raises(sp.Panic, match="ncols == rhs.nrows"):
        a * a
    # mismatch through the device entry point too
    with pytest.raises(sp.Panic, match=r"left: 3, right: 2"):
        a.device().mul(a.device())
    # mixed element sizes
    b32 = sp.CsrMatrix(3, 2, [0, 1, 1, 2], [0, 1], np.array([1.0, 2.0], dtype=np.float32))
    with pytest.raises(sp.Panic, match="element sizes"):
        a * b32
    # row-block operands (more entries than one set of 32-bit offsets; the limit lowered for the test)
    monkeypatch.setenv("SPAL_CSR_PART_ENTRIES", "3000")
    rp, ci, va = synth.banded_csr(2000, 2000, 4, 64, 3)
    big = sp.CsrMatrix(2000, 2000, rp, ci, va)
    assert big.device().describe()["kernel"] == "row_blocks"
    monkeypatch.delenv("SPAL_CSR_PART_ENTRIES")
    small = sp.CsrMatrix(2000, 2000, rp, ci, va)
    for lhs, rhs in ((big, small), (small, big)):
        with pytest.raises(sp.SpalError) as e:
            lhs * rhs
        assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED
    # unknown option values
    with pytest.raises(sp.Panic):
        small.device().set_option("spgemm_route", 3)
    with pytest.raises(sp.Panic):
        small.device().set_option("spgemm_lds_cap", 1 << 20)
