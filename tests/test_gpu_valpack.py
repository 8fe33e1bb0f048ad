"""Packed values under the sliding kernel's record form (csr_valpack.hpp): where every f64 value of a matrix of uniform
rows is k * 2^e with k inside 53 / 54 bits, a row streams one fixed-point block (80 / 96 / 112 B) instead of its values.
The decode returns the stored doubles bit for bit and the products and sums are formed per row exactly as the strip
forms them, so every result here is compared bit for bit (np.array_equal on the bit patterns) with the CPU oracle, and
with the same handle's result under "valpack_on" 0 and under "rowrec_on" 0."""
import numpy as np
import pytest

import spalinalg_amd as sp
import spal_synth as synth
from tests.test_gpu_slide_forms import ALL, TWO, run_forms

pytestmark = pytest.mark.gpu
W = 4096


def bits(y):
    return y.view(np.uint64 if y.dtype == np.float64 else np.uint32)


def all_forms(dev, x, y_ref, packed=True):
    """The product with packed values, with plain values on the record form, and with col16: the oracle's bits."""
    d = dev.describe()
    assert d["slide"] == 1 and d["rowrec"] == 1 and d["rowrec_on"] == 1, d
    assert d["valpack"] == (1 if packed else 0) and d["valpack_on"] == d["valpack"] and d["valpack_failed"] == 0, d
    out = run_forms(dev, x, ALL if packed else TWO, y_ref)      # every form reached, none beyond those named
    d = dev.describe()
    assert d["rowrec_on"] == 1 and d["valpack_on"] == d["valpack"], d
    for y in out.values():
        assert np.array_equal(bits(y), bits(y_ref))


def band_columns(n, nc, L, seed):
    rp, ci, _ = synth.banded_csr(n, nc, L, W, seed)
    return rp, ci


@pytest.fixture(scope="module")
def bands(oracle):
    """banded_csr with 12 and 14 per row at n = 40 037 (last tile and last step partial) with the oracle's product:
    computed once."""
    n = 40_000 + 37
    x = synth.vector(n)
    out = {}
    for L in (12, 14):
        rp, ci, va = synth.banded_csr(n, n, L, W, 100 + L)
        out[L] = (n, rp, ci, va, x, oracle.csr_spmv(rp, ci, va, x))
    return out


@pytest.mark.parametrize("L", [12, 14])
def test_uniform_bands_bit_for_bit(bands, L):
    n, rp, ci, va, x, y_ref = bands[L]
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    d = dev.describe()
    assert d["valpack"] == 1 and d["valpack_bits"] == 53 and d["valpack_exp"] == -52, d
    assert d["valpack_bytes_per_row"] == (96 if L == 14 else 80), d
    assert d["valpack_build_ms"] > 0 and d["valpack_us"] == [0.0, 0.0], d
    all_forms(dev, x, y_ref)
    for key, value, back in (("slide_run", 3, 0), ("persistent_blocks", 64, 0), ("nt_store", 1, 0), ("prefetch", 1, 1)):
        dev.set_option(key, value)
        all_forms(dev, x, y_ref)
        dev.set_option(key, back)


def test_rows_of_16_pack_without_skew(oracle):
    """rows of 128 bytes get skewed strips and no sliding kernel by default; under "skew" 0 they have records and blocks
    of 112 B"""
    n = 10_000 + 37
    rp, ci, va = synth.banded_csr(n, n, 16, W, 116)
    x = synth.vector(n)
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    assert "valpack" not in dev.describe()
    dev.set_option("skew", 0)
    assert dev.describe()["valpack_bytes_per_row"] == 112
    all_forms(dev, x, oracle.csr_spmv(rp, ci, va, x))


@pytest.mark.parametrize("n", [64, 65, 257])
def test_small_matrices(oracle, n):
    """one tile; one row in the last tile; one row in the last step (ncols holds the band)"""
    nc = 6000
    rp, ci, va = synth.banded_csr(n, nc, 14, W, 7)
    x = synth.vector(nc)
    dev = sp.CsrMatrix(n, nc, rp, ci, va).device()
    d = dev.describe()
    assert d["valpack"] == 1 and d["slide"] == 0 and d["valpack_on"] == 0, d   # (so few tiles: the sliding kernel not by default)
    dev.set_option("slide_on", 1)                                               # ... but by name
    all_forms(dev, x, oracle.csr_spmv(rp, ci, va, x))


def test_integer_values_and_stored_zeros(oracle):
    rng = np.random.default_rng(21)
    n = 10_000 + 37
    rp, ci = band_columns(n, n, 14, 31)
    va = rng.integers(-1000, 1001, ci.size).astype(np.float64)
    va[va == 0] = 1.0
    va[1] = 3.0                                          # (an odd value: the quantum is 2^0 whatever was drawn)
    va[[0, 14 * 63 + 13, 14 * 64, va.size - 1]] = 0.0   # explicit stored zeros: first and last entry, around a tile's end
    x = rng.uniform(-1, 1, n)
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    d = dev.describe()
    assert d["valpack"] == 1 and d["valpack_exp"] == 0 and d["valpack_bits"] == 11, d
    all_forms(dev, x, oracle.csr_spmv(rp, ci, va, x))


def test_a_tiny_quantum(oracle):
    """values k * 2^-1000: products with x of ordinary size stay normal, and the bits are the oracle's"""
    rng = np.random.default_rng(22)
    n = 10_000 + 37
    rp, ci = band_columns(n, n, 14, 32)
    k = rng.integers(-(1 << 40), 1 << 40, ci.size)
    k[0] = 1
    va = np.ldexp(k.astype(np.float64), -1000)
    x = rng.uniform(-1, 1, n)
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    d = dev.describe()
    assert d["valpack"] == 1 and d["valpack_exp"] == -1000 and d["valpack_bits"] <= 42, d
    all_forms(dev, x, oracle.csr_spmv(rp, ci, va, x))


def test_extremes_next_to_each_other(oracle):
    """rows that mix k = +-(2^53 - 1), the widest a 54-bit field holds short of -2^53, with k = 1"""
    rng = np.random.default_rng(23)
    n = 10_000 + 37
    rp, ci = band_columns(n, n, 14, 33)
    top = float((1 << 53) - 1)
    va = rng.choice(np.array([top, -top, 1.0, -1.0]), ci.size)
    va[:4] = [top, 1.0, -top, 1.0]
    x = rng.uniform(-1, 1, n)
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    d = dev.describe()
    assert d["valpack"] == 1 and d["valpack_exp"] == 0 and d["valpack_bits"] == 54, d
    all_forms(dev, x, oracle.csr_spmv(rp, ci, va, x))


@pytest.mark.parametrize("odd", ["nan", "negative zero", "third", "one bit too many"])
def test_one_value_that_does_not_pack(oracle, odd):
    """n = 4096 with the odd value in the last row: no packed array, no failure, the product still the oracle's bits"""
    rng = np.random.default_rng(24)
    n = 4096
    rp, ci = band_columns(n, n, 14, 34)
    va = rng.integers(-1000, 1001, ci.size).astype(np.float64)
    va[va == 0] = 1.0
    va[1] = 3.0
    va[-3] = {"nan": np.nan, "negative zero": -0.0, "third": 1.0 / 3.0, "one bit too many": float(1 << 53)}[odd]
    x = rng.uniform(-1, 1, n)
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    d = dev.describe()
    assert d["rowrec"] == 1 and d["valpack"] == 0 and d["valpack_on"] == 0 and d["valpack_failed"] == 0, d
    assert d["valpack_bytes_per_row"] == 0, d
    y_ref = oracle.csr_spmv(rp, ci, va, x)
    y = dev.spmv(x)
    assert np.array_equal(bits(y), bits(y_ref))
    dev.set_option("rowrec_on", 0)
    assert np.array_equal(bits(dev.spmv(x)), bits(y_ref))


def test_f32_handles_have_no_packed_values(oracle):
    n = 40_000 + 37
    rp, ci, va = synth.banded_csr(n, n, 14, W, 114, dtype=np.float32)
    x = synth.vector(n, dtype=np.float32)
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    d = dev.describe()
    assert d["slide"] == 1 and d["rowrec"] == 1 and not [k for k in d if k.startswith("valpack")], d
    with pytest.raises(sp.Panic):
        dev.set_option("valpack", 2)
    dev.set_option("valpack", 1)                 # the option is the plan's; an f32 handle has nothing to pack
    assert "valpack" not in dev.describe()
    assert np.array_equal(bits(dev.spmv(x)), bits(oracle.csr_spmv(rp, ci, va, x)))
