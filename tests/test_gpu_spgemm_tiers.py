"""GPU: every tier of the sparse x sparse product (spal_csr_mul / spal_csc_mul) at its boundaries, with constructed
inputs (tests/spgemm_cases.py; what the generators promise is checked on the CPU by tests/test_spgemm_cases_host.py).

Every comparison is exact against oracle.csr_mul / oracle.csc_mul (indices equal, values equal as raw bits, NaN by
position), and every product's describe()["spgemm"] must EQUAL the host mirror's expectation: the whole tier_rows
dict, products, large_products and nnz."""
import functools
import os
import time

import numpy as np
import pytest

import spalinalg_amd as sp
import spal_synth as synth
from spalinalg_amd import _ffi
from tests import spadd_ref
from tests import spgemm_cases as sc
from tests.test_gpu_spgemm import arrays, assert_same

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
FORMATS = ["csr", "csc"]
FUZZ_SEEDS = int(os.environ.get("SPAL_SPGEMM_FUZZ_SEEDS", "16"))      # (more seeds: a longer soak)


def matrices(case, fmt):
    """(user-level left operand, right operand) of the case's product: CSR A * B, or the same arrays as the CSC
    matrices B^T (p x n) * A^T (n x m)"""
    if fmt == "csr":
        return sp.CsrMatrix(case.m, case.n, *case.a), sp.CsrMatrix(case.n, case.p, *case.b)
    return sp.CscMatrix(case.p, case.n, *case.b), sp.CscMatrix(case.n, case.m, *case.a)


def reference(oracle, case, fmt):
    ref = oracle.csr_mul((case.m, case.n), case.a, (case.n, case.p), case.b)
    if fmt == "csc":      # (the CSC arrays of (AB)^T are the CSR arrays of AB)
        assert_same(oracle.csc_mul((case.p, case.n), case.b, (case.n, case.m), case.a), ref)
    return ref


def check_product(left, right, case, ref, route=0, cap=0):
    """sets the options on the LEFT operand's handle, multiplies, compares bits and the whole describe() object"""
    left.device().set_option("spgemm_route", route)
    left.device().set_option("spgemm_lds_cap", cap)
    C = left * right
    assert type(C) is type(left)
    assert_same(arrays(C), ref)
    d = C.device().describe()["spgemm"]
    assert d["route"] == route
    assert sc.reported(d) == sc.expected(case.a, case.b, route, cap, nnz=int(ref[0][-1])), d
    return C, d


def row_of(ref_or_arrays, i):
    rp, ci, va = ref_or_arrays
    return dict(zip(ci[int(rp[i]):int(rp[i + 1])].tolist(), va[int(rp[i]):int(rp[i + 1])].tolist()))


# ---- a. tier boundaries ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def boundary_case(dtype):
    return sc.boundaries(1, dtype)


BOUNDARY_CONFIGS = [(0, 0), (1, 0), (2, 0)] + [(0, c) for c in sc.BOUNDARY_CAPS]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route,cap", BOUNDARY_CONFIGS)
def test_boundaries(oracle, route, cap, dtype, fmt):
    """ub = 1, 2, 63 .. 4097 built three ways with three column shapes each; rows with ub = cap are LDS rows, rows with
    ub = cap + 1 large ones (tests/test_spgemm_cases_host.py::test_boundaries_claims, and the describe() equality)."""
    case = boundary_case(dtype)
    left, right = matrices(case, fmt)
    _, d = check_product(left, right, case, reference(oracle, case, fmt), route, cap)
    if route == 1:
        assert all(d["tier_rows"][t] > 0 for t in sc.LDS_TIERS) and d["tier_rows"]["large"] > 0


# ---- b. the order witness in every tier ------------------------------------------------------------------------
WITNESS_RUNS = [(t, o) for t, (_, o) in sorted(sc.WITNESS.items())] + [("large", {"spgemm_lds_cap": 16})]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tier,opts", WITNESS_RUNS, ids=[f"{t}-{'-'.join(map(str, o.values())) or 'auto'}" for t, o in WITNESS_RUNS])
def test_order_witness_every_tier(oracle, tier, opts, dtype, fmt):
    """[1e16, -1e16, 1] sums to 1 in ascending k only; sums of up to 2048 order-sensitive products beside it"""
    case = sc.order_witness(tier, dtype)
    ref = reference(oracle, case, fmt)
    left, right = matrices(case, fmt)
    C, d = check_product(left, right, case, ref, opts.get("spgemm_route", 0), opts.get("spgemm_lds_cap", 0))
    assert d["tier_rows"][tier] == case.m - 1 and d["tier_rows"]["empty"] == 1
    for i, r in enumerate(case.rows):
        if r["kind"] == "three":
            assert row_of(arrays(C), i)[r["witness"]] == 1.0


# ---- c. hash worst cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", [0, 1])
def test_hash_worst_cases(oracle, route, dtype, fmt):
    """every key homed in the table's top slots, or in its last one: chains that wrap and grow to the row's length;
    claimed at one step and added at a later one; column ncols - 1 = 2^20 - 1.  (Route 0 sends the 4096-product rows to
    the large tier.)"""
    case = sc.hash_worst(dtype)
    left, right = matrices(case, fmt)
    _, d = check_product(left, right, case, reference(oracle, case, fmt), route, 0)
    assert d["tier_rows"]["block8k" if route == 1 else "large"] == 3


WIDE_NCOLS = (1 << 27) - 2


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
def test_hash_worst_cases_wide(oracle, dtype):
    """The same key sets with column ncols - 1 at ncols = 2^27 - 2: CSR and the LDS route only.  The eager plan of a
    CSR handle allocates a vector of ncols elements, the large tier transposes over B.ncols and a CSC handle holds
    ncols + 1 pointers; 2^27 - 2 is the largest ncols that keeps each of these (and the oracle's u64 pointers) below
    1 GiB."""
    case = sc.hash_worst(dtype, ncols=WIDE_NCOLS)
    assert int(case.b[1].max()) == WIDE_NCOLS - 1
    left, right = matrices(case, "csr")
    _, d = check_product(left, right, case, reference(oracle, case, "csr"), 1, 0)
    assert d["tier_rows"]["large"] == 0


# ---- d. run shapes of the large tier ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route,cap", [(2, 0), (0, 48), (0, 0)])
@pytest.mark.parametrize("p", [1, 1 << 20])
def test_large_tier_runs(oracle, p, route, cap, dtype, fmt):
    """runs of 2 .. 5000 equal columns with heads at chunk offsets 0, 63, 64, 255, rows of 256 k and 256 k +- 1
    products, single-run and all-distinct rows, between LDS-tier rows; B.ncols = 1 (every row ONE run) and 2^20"""
    case = sc.large_runs(dtype, p)
    left, right = matrices(case, fmt)
    _, d = check_product(left, right, case, reference(oracle, case, fmt), route, cap)
    assert d["tier_rows"]["large"] >= len(sc.RUN_ROWS)         # (every constructed row holds more than 2048 products)


# ---- e. the two 32-bit limits ----------------------------------------------------------------------------------
def column_and_row(m, p, dtype, rng):
    """A = m x 1 with every row stored, B = 1 x p dense: m * p products, every row of C holds p entries"""
    a = (np.arange(m + 1, dtype=np.uint64), np.zeros(m, dtype=np.uint64), sc.order_sensitive_values(rng, m, dtype))
    b = (np.array([0, p], dtype=np.uint64), np.arange(p, dtype=np.uint64), sc.order_sensitive_values(rng, p, dtype))
    return sc.Case(m, 1, p, a, b, None)


def refused(left, right):
    t0 = time.perf_counter()
    with pytest.raises(sp.SpalError) as e:
        left.device().mul(right.device())
    assert e.value.status == _ffi.SPAL_ERR_UNSUPPORTED
    return time.perf_counter() - t0, str(e.value)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_large_products_limit(oracle, dtype, fmt):
    """70 000 x 1 times 1 x 70 000: 4.9e9 products, all in the large tier -- refused before the expand buffers are
    allocated; the same handles then multiply the other way round (1 x 1, one run of 70 000 products)."""
    rng = np.random.default_rng(70)
    case = column_and_row(70_000, 70_000, dtype, rng)
    assert sc.expected(case.a, case.b)["large_products"] == 4_900_000_000 > 0xFFFFFFFF - 65536
    left, right = matrices(case, fmt)
    _, msg = refused(left, right)
    assert "4900000000 products" in msg
    # the same handles the other way round: (1 x 70 000) * (70 000 x 1), in CSR and in CSC alike the CSR product of
    # case.b's arrays times case.a's -- one row, one run of 70 000 products
    C = right * left
    fn = oracle.csr_mul if fmt == "csr" else oracle.csc_mul
    ref = fn((1, 70_000), (case.b if fmt == "csr" else case.a), (70_000, 1), (case.a if fmt == "csr" else case.b))
    assert_same(arrays(C), ref)
    want = sc.expected(case.b, case.a, nnz=1)
    assert want["tier_rows"]["large"] == 1 and want["large_products"] == 70_000
    assert sc.reported(C.device().describe()["spgemm"]) == want


# Timed once on an MI355X: the refused call (count, 1 050 000 symbolic block8k rows = 4.3e9 insertions, scan) returns
# after 0.01 s and the whole test takes 0.17 s behind other tests.  Five times that is below what a first
# test of a process spends on initialising the device, so the limit is 10 s.
@pytest.mark.timeout(10)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nnz_limit(oracle, dtype, fmt):
    """Route 1, 1 050 000 x 1 times 1 x 4096: every row a full block8k table, nnz(C) = 4.3e9 -- refused after the symbolic
    pass, before C is allocated; small products on the same handles afterwards."""
    rng = np.random.default_rng(71)
    m, p = 1_050_000, 4096
    case = column_and_row(m, p, dtype, rng)
    e = sc.expected(case.a, case.b, 1, 0)
    assert e["tier_rows"]["block8k"] == m and e["large_products"] == 0 and e["products"] > 0xFFFFFFFF - 65536
    left, right = matrices(case, fmt)
    left.device().set_option("spgemm_route", 1)
    seconds, msg = refused(left, right)
    print(f"nnz limit: refused after {seconds:.2f} s ({np.dtype(dtype).name}, {fmt})")
    assert f"{m * p} entries" in msg
    # the same handles, each with a small partner
    small_b = (np.array([0, 3], dtype=np.uint64), np.arange(3, dtype=np.uint64), sc.order_sensitive_values(rng, 3, dtype))
    small_a = (np.arange(6, dtype=np.uint64), np.zeros(5, dtype=np.uint64), sc.order_sensitive_values(rng, 5, dtype))
    A, B = (left, right) if fmt == "csr" else (right, left)         # the holders of case.a (m x 1) and case.b (1 x p)
    for ca in (sc.Case(m, 1, 3, case.a, small_b, None), sc.Case(5, 1, p, small_a, case.b, None)):
        ref = reference(oracle, ca, fmt)
        mine_l, mine_r = matrices(ca, fmt)
        if ca.m == m:      # case.a's handle with a new small partner
            l, r = (A, mine_r) if fmt == "csr" else (mine_l, A)
        else:
            l, r = (mine_l, B) if fmt == "csr" else (B, mine_r)
        route = 1 if l is left else 0
        C = l * r
        assert_same(arrays(C), ref)
        assert sc.reported(C.device().describe()["spgemm"]) == sc.expected(ca.a, ca.b, route, 0, nnz=int(ref[0][-1]))


# ---- f. chains on device handles -------------------------------------------------------------------------------
class Chain:
    """device handles and their CPU twins, one format: every step is downloaded and compared"""

    def __init__(self, oracle, fmt, n):
        self.oracle, self.fmt, self.n = oracle, fmt, n

    def upload(self, arr):
        cls = sp.CsrMatrix if self.fmt == "csr" else sp.CscMatrix
        return cls(self.n, self.n, *arr).device(), arr

    def same(self, dev, ref):
        assert_same(dev.download(), ref)
        return dev, ref

    def mul(self, x, y, route=0, cap=0):
        (dx, rx), (dy, ry) = x, y
        fn = self.oracle.csr_mul if self.fmt == "csr" else self.oracle.csc_mul
        ref = fn((self.n, self.n), rx, (self.n, self.n), ry)
        out = dx.mul(dy)
        inner = (rx, ry) if self.fmt == "csr" else (ry, rx)      # (the CSC product runs B's arrays times A's)
        d = out.describe()["spgemm"]
        assert d["route"] == route
        assert sc.reported(d) == sc.expected(*inner, route, cap, nnz=int(ref[0][-1])), d
        return self.same(out, ref)

    def add_sub(self, x, y, sub):
        (dx, rx), (dy, ry) = x, y
        return self.same(dx.sub(dy) if sub else dx.add(dy), spadd_ref.add_sub_fast(self.n, self.n, rx, ry, sub))

    def neg(self, x):
        return self.same(x[0].neg(), spadd_ref.neg(x[1]))

    def flip(self, x):
        """to the other format and a Chain of it"""
        other = Chain(self.oracle, "csc" if self.fmt == "csr" else "csr", self.n)
        dev = x[0].to_csc() if self.fmt == "csr" else x[0].to_csr()
        return other, other.same(dev, self.oracle.transpose(self.n, self.n, *x[1]))


def square(rng, n, per_row, dtype):
    """n x n, `per_row` entries per row in a band of 6 * per_row columns, order-sensitive values"""
    rp, ci, _ = synth.banded_csr(n, n, per_row, 6 * per_row, int(rng.integers(1 << 30)))
    return rp, ci, sc.order_sensitive_values(rng, ci.size, dtype)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_chains_on_device_handles(oracle, dtype, fmt):
    """results of mul / add / sub / neg / to_csc / to_csr (adopted device arrays with their spare tail) as operands"""
    rng = np.random.default_rng(90)
    n = 3000
    ch = Chain(oracle, fmt, n)
    A, B, C = (ch.upload(square(rng, n, k, dtype)) for k in (9, 12, 30))
    # ((A * B) - C) * (-A), with options set on the result handle (A * B) - C
    D = ch.add_sub(ch.mul(A, B), C, True)
    D[0].set_option("spgemm_lds_cap", 100)
    R = ch.mul(D, ch.neg(A), cap=100)
    t = R[0].describe()["spgemm"]["tier_rows"]
    assert t["large"] > 0 and t["wave"] == t["block4k"] == t["block8k"] == 0       # the cap took effect ...
    D[0].set_option("spgemm_route", 2)
    R2 = ch.mul(D, ch.neg(A), route=2, cap=100)
    assert R2[0].describe()["spgemm"]["tier_rows"]["large"] == n                   # ... and so did the route
    assert_same(R2[0].download(), R[1])
    # (A + B) * (A - B)
    ch.mul(ch.add_sub(A, B, False), ch.add_sub(A, B, True))
    # (A * B) and (B * A) through the other format, multiplied there, and back
    other, X = ch.flip(ch.mul(A, B))
    _, Y = ch.flip(ch.mul(B, A))
    X[0].set_option("spgemm_route", 1)
    back, Z = other.flip(other.mul(X, Y, route=1))
    assert back.fmt == fmt
    # A * (A * (A * A)) on a banded matrix
    P = ch.mul(A, ch.mul(A, ch.mul(A, A)))
    assert P[0].describe()["spgemm"]["products"] > 100 * n


# ---- g. whose options the CSC product reads --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_csc_product_reads_the_left_operands_options(oracle, dtype):
    """options on the left operand.  spal_csc_mul runs the CSR product of B's arrays times A's arrays, and
    still it is `a`, the user-level left operand, whose spgemm_route / spgemm_lds_cap count."""
    case = boundary_case(dtype)
    ref = reference(oracle, case, "csc")
    with_a = sc.expected(case.a, case.b, 0, 64, nnz=int(ref[0][-1]))
    with_b = sc.expected(case.a, case.b, 0, 4096, nnz=int(ref[0][-1]))
    assert with_a["tier_rows"] != with_b["tier_rows"]
    a, b = matrices(case, "csc")
    a.device().set_option("spgemm_lds_cap", 64)
    b.device().set_option("spgemm_lds_cap", 4096)
    C = a * b
    assert_same(arrays(C), ref)
    assert sc.reported(C.device().describe()["spgemm"]) == with_a
    b.device().set_option("spgemm_route", 2)                      # nor does b's route count
    d = (a * b).device().describe()["spgemm"]
    assert d["route"] == 0 and sc.reported(d) == with_a
    a.device().set_option("spgemm_route", 2)
    d = (a * b).device().describe()["spgemm"]
    assert d["route"] == 2 and sc.reported(d) == sc.expected(case.a, case.b, 2, 64, nnz=int(ref[0][-1]))
    # the CSR product of the same arrays: its left operand is A
    A, B = matrices(case, "csr")
    A.device().set_option("spgemm_lds_cap", 64)
    B.device().set_option("spgemm_lds_cap", 4096)
    assert sc.reported((A * B).device().describe()["spgemm"]) == with_a


# ---- h. fuzz ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz(oracle, seed):
    """shapes, row-length laws, special values, dtype, format, route and cap by seed; the default 16 seeds reach every
    tier (tests/test_spgemm_cases_host.py::test_fuzz_seeds_cover_every_tier)"""
    case, dtype, fmt, opts = sc.fuzz(seed)
    left, right = matrices(case, fmt)
    check_product(left, right, case, reference(oracle, case, fmt), opts["spgemm_route"], opts["spgemm_lds_cap"])
