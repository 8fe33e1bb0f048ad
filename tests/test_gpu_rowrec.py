"""Row records under the sliding kernel (csr_rowrec.hpp): one Elias-Fano record per row of 12, 14 or 16 entries instead of
the row's 16-bit window positions.  The decode delivers exactly the positions col16 would have, per lane, and the
products and sums are the sliding kernel's own: every result here is compared bit for bit (np.array_equal) with the CPU
oracle, and with the same handle's result under "rowrec_on" 0 -- and, on the f64 handles, whose values pack
(csr_valpack.hpp), under "valpack_on" 0 and 1: test_gpu_slide_forms.run_forms forces each form in turn.  The structures are
those of tests/slide_cases.py."""
import numpy as np
import pytest

import spalinalg_amd as sp
import spal_synth as synth
from tests import slide_cases as cases
from tests.slide_cases import hand_built      # (the builders live there now)
from tests.test_gpu_slide_forms import ALL, TWO, run_forms

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
W = 4096


def bits(y):
    return y.view(np.uint64 if y.dtype == np.float64 else np.uint32)


def both_forms(dev, x, y_ref):
    """The product with the records and with col16 on the same handle -- and, the values of an f64 handle here being
    draws of m * 2^-52, with packed values: every form is reached (run_forms asserts it) and gives the oracle's bits."""
    dev.set_option("rowrec_on", 1)
    d = dev.describe()
    assert d["slide"] == 1 and d["rowrec"] == 1 and d["rowrec_on"] == 1 and d["rowrec_failed"] == 0, d
    out = run_forms(dev, x, ALL if d["dtype"] == "f64" else TWO, y_ref)
    y0, y1 = out["col16"], out["records"]
    assert dev.describe()["rowrec_on"] == 1
    assert np.array_equal(y0, y_ref)
    assert np.array_equal(y1, y_ref)
    assert np.array_equal(bits(y1), bits(y0))


def values(rng, size, dtype):
    return rng.uniform(-1, 1, size).astype(dtype)


@pytest.fixture(scope="module")
def bands(oracle):
    """banded_csr with 12, 14 and 16 per row at n = 40 037 (last tile and last step partial), f64 and f32, with the
    oracle's product: computed once."""
    n = 40_000 + 37
    out = {}
    for dtype in DTYPES:
        x = synth.vector(n, dtype=dtype)
        for L in (12, 14, 16):
            rp, ci, va = synth.banded_csr(n, n, L, W, 100 + L, dtype=dtype)
            out[(L, np.dtype(dtype))] = (n, rp, ci, va, x, oracle.csr_spmv(rp, ci, va, x))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [12, 14, 16])
def test_uniform_bands_bit_for_bit(bands, L, dtype):
    n, rp, ci, va, x, y_ref = bands[(L, np.dtype(dtype))]
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    if L * np.dtype(dtype).itemsize == 128:
        # rows of 128 bytes get skewed product strips, which the sliding kernel does not have: no records by default
        d = dev.describe()
        assert d["skew"] == 1 and d["slide"] == 0 and "rowrec" not in d, d   # (the keys come with the sliding plan)
        assert np.array_equal(dev.spmv(x), y_ref)
        dev.set_option("skew", 0)
    d = dev.describe()
    assert d["rowrec_bytes_per_row"] == (20 if L <= 14 else 24) and d["index_bits"] == 16, d
    assert d["rowrec_max_span"] >= W - 1, d
    both_forms(dev, x, y_ref)
    for key, value, back in (("slide_run", 3, 0), ("persistent_blocks", 64, 0), ("nt_store", 1, 0), ("prefetch", 1, 1)):
        dev.set_option(key, value)
        both_forms(dev, x, y_ref)
        dev.set_option(key, back)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [64, 65, 257])
def test_small_matrices(oracle, n, dtype):
    """one tile; one row in the last tile; one row in the last step (ncols holds the band)"""
    nc = 6000
    rp, ci, va = synth.banded_csr(n, nc, 14, W, 7, dtype=dtype)
    x = synth.vector(nc, dtype=dtype)
    dev = sp.CsrMatrix(n, nc, rp, ci, va).device()
    d = dev.describe()
    assert d["rowrec"] == 1 and d["slide"] == 0 and d["rowrec_on"] == 0, d   # (so few tiles are mostly re-reads: not by default)
    dev.set_option("slide_on", 1)                                             # ... but by name
    both_forms(dev, x, oracle.csr_spmv(rp, ci, va, x))


@pytest.mark.parametrize("dtype", DTYPES)
def test_hand_built_rows(oracle, dtype):
    rng = np.random.default_rng(14)
    n = 40_000 + 37
    # the widest row a record of 14 columns holds: 39 - 12 = 27 whole pages and a low byte
    top = 27 * 256 + 255
    assert top == cases.max_span(14)
    for span, on in ((top, 1), (top + 1, 0)):
        rp, ci = hand_built(n, 20_000, span)
        va, x = values(rng, ci.size, dtype), values(rng, n, dtype)
        y_ref = oracle.csr_spmv(rp, ci, va, x)
        dev = sp.CsrMatrix(n, n, rp, ci, va).device()
        dev.set_option("window_pages", 40)      # (the step of the wide row needs 30 pages)
        d = dev.describe()
        assert d["slide"] == 1 and d["rowrec_failed"] == 0, d
        assert d["rowrec_max_span"] == top, d    # (the ring is wider than the record's reach: the bits decide)
        assert d["rowrec"] == on and d["rowrec_on"] == on, d
        if on:
            R = d["ring_pages"] * 256
            wraps = [r for r in range(0, n - 600, 97) if r % R >= R - 256]
            assert wraps, d                       # a row whose positions wrap the ring
            assert set(wraps) <= set(cases.wrapping_rows(ci, 14, R).tolist())
            both_forms(dev, x, y_ref)
        else:
            assert np.array_equal(dev.spmv(x), y_ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_jumps_between_steps(oracle, dtype):
    """block-diagonal sections of rows of 14 whose column ranges jump forwards and backwards between steps: entering
    pages on both sides, disjoint windows, synchronous page loads; ncols odd (x ends inside a 16-byte vector)"""
    rng = np.random.default_rng(5)
    n, nc = 40_000, 50_001
    rp, ci = cases.block_jumps(rng, n, nc, 14)
    va, x = values(rng, ci.size, dtype), values(rng, nc, dtype)
    y_ref = oracle.csr_spmv(rp, ci, va, x)
    dev = sp.CsrMatrix(n, nc, rp, ci, va).device()
    both_forms(dev, x, y_ref)
    dev.set_option("slide_run", 5)
    both_forms(dev, x, y_ref)


def test_ineligible_rows_keep_col16(oracle):
    n = 40_000 + 37
    x = synth.vector(n)
    for rp, ci, va in (synth.banded_csr(n, n, 10, W, 3), synth.ragged_csr(n, n, W, 3),
                       synth.banded_csr(n, n, 13, W, 3), synth.banded_csr(n, n, 18, W, 3)):
        dev = sp.CsrMatrix(n, n, rp, ci, va).device()
        d = dev.describe()
        assert d["rowrec"] == 0 and d["rowrec_on"] == 0 and d["rowrec_failed"] == 0, d
        assert np.array_equal(dev.spmv(x), oracle.csr_spmv(rp, ci, va, x))


def test_unaligned_x_falls_back(bands):
    """x off a 16-byte boundary: the one-super-tile kernels run on col16, which stays resident beside the records"""
    import torch
    n, rp, ci, va, x, y_ref = bands[(14, np.dtype(np.float64))]
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    assert dev.describe()["rowrec_on"] == 1
    big = torch.zeros(n + 8, dtype=torch.float64, device="cuda")
    xs = big[1:n + 1]
    xs.copy_(torch.from_numpy(x))
    assert xs.data_ptr() % 16 == 8
    assert np.array_equal(dev.spmv_torch(xs).cpu().numpy(), y_ref)
    xa = big[2:n + 2]
    xa.copy_(torch.from_numpy(x))
    assert xa.data_ptr() % 16 == 0
    assert np.array_equal(dev.spmv_torch(xa).cpu().numpy(), y_ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(dtype):
    """NaN, +-Inf and -0.0 in the values and in x: the records change where a position comes from, not one operand --
    the bit patterns are those of the same handle streaming col16"""
    rng = np.random.default_rng(9)
    n = 10_000 + 37
    rp, ci, va = synth.banded_csr(n, n, 14, W, 5, dtype=dtype)
    x = synth.vector(n, dtype=dtype)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], dtype=dtype)
    at = rng.choice(va.size, size=va.size // 50, replace=False)
    va[at] = special[rng.integers(0, special.size, at.size)]
    at = rng.choice(n, size=n // 50, replace=False)
    x[at] = special[rng.integers(0, special.size, at.size)]
    rows = np.arange(0, n, 11)                  # rows that are -0.0 throughout: the sum must keep the sign
    for r in rows:
        va[r * 14:(r + 1) * 14] = -0.0
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    d = dev.describe()
    assert d["rowrec"] == 1 and d["rowrec_on"] == 1, d
    y1 = dev.spmv(x)
    dev.set_option("rowrec_on", 0)
    y0 = dev.spmv(x)
    assert np.array_equal(bits(y1), bits(y0))
    assert np.isnan(y1).any() and np.isinf(y1).any()
