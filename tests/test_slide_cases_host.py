"""The inputs of tests/test_gpu_slide_forms.py (tests/slide_cases.py), checked with numpy and the oracle alone (no GPU).

Every structure is valid CSR of exactly L ascending columns per row; hand_built keeps a wrapping row whatever ring the
planner picks; the constants restated in Python are the headers'; packs() returns on every value class what the class
states, from how it plants its values; the special-operand layout carries -0.0, NaN and +-Inf rows in the oracle's product,
the last row of the matrix among the -0.0; and the randomised generator reaches every length, pattern and dtype."""
import os
import subprocess

import numpy as np
import pytest

import spal_synth as synth
from tests import slide_cases as cases
from tests import special_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spalinalg_amd", "csrc")
N = 40_000 + 37
SEEDS = 24


def check_structure(oracle, n, nc, rp, ci, L, nvalues=None):
    assert rp.dtype == np.uint64 and ci.dtype == np.uint64 and rp.size == n + 1
    assert oracle.validate(n, nc, rp, ci, ci.size if nvalues is None else nvalues) == 0
    assert np.array_equal(rp, np.arange(n + 1, dtype=np.uint64) * L)          # exactly L per row
    t = ci.astype(np.int64).reshape(n, L)
    assert np.all(np.diff(t, axis=1) > 0) and t.min() >= 0 and t.max() < nc   # strictly ascending, inside ncols


def test_the_constants_are_the_headers(tmp_path):
    exe = str(tmp_path / "slide_bounds")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "slide_bounds.cpp"), "-o", exe])
    seen = 0
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        what, *v = line.split()
        v = [int(q) for q in v]
        if what == "span":
            assert cases.max_span(v[0], v[1]) == v[2], line
            seen += 1
        elif what == "width":
            assert cases.value_width(v[0]) == v[1], line
        elif what == "exp":
            assert (cases.EXP_MIN, cases.EXP_MAX) == tuple(v), line
        else:
            assert what == "high_bits" and cases.HIGH_BITS == v[0], line
    assert seen == 3 * 256
    # the widest encodable row: (39 - (L - 2)) whole pages and a low byte of 255
    assert [cases.max_span(L) for L in cases.LENGTHS] == [29 * 256 + 255, 27 * 256 + 255, 25 * 256 + 255]


@pytest.mark.parametrize("L", cases.LENGTHS)
def test_hand_built_rows(oracle, L):
    top = cases.max_span(L)
    for span in (top, top + 1):
        rp, ci = cases.hand_built(N, 20_000, span, L)
        check_structure(oracle, N, N, rp, ci, L)
        t = ci.astype(np.int64).reshape(N, L)
        spans = t[:, -1] - t[:, 0]
        assert spans[20_000] == span and np.all(np.delete(spans, 20_000) <= cases.SPREAD_SPAN)
        spread = np.flatnonzero(spans == cases.SPREAD_SPAN)
        assert spread.size > 400 and np.all(spread % cases.SPREAD_EVERY == 0)
        low = set((t[spread] & 255).reshape(-1).tolist())
        assert {0, 1, 255} <= low
        one_page = np.flatnonzero((spans == 255) & (t[:, 0] % 256 == 0))
        assert one_page.size > 300


def test_hand_built_is_its_row_by_row_text():
    """the table hand_built fills at once against the rule spelled out a row at a time (uniform_rows checks each row)"""
    n, wide_row, wide_span = 12_000 + 37, 2000, cases.max_span(14)

    def cols(r):
        if r == wide_row:
            return [r + k for k in range(13)] + [r + wide_span]
        if r % 97 == 0 and r + 600 < n:
            return [r + k for k in (0, 3, 50, 255, 256, 257, 300, 301, 400, 511, 512, 513, 599, 600)]
        if r % 97 == 5 and (r // 256) * 256 + 256 <= n:
            p = (r // 256) * 256
            return [p + k for k in (0, 1, 17, 30, 31, 64, 100, 127, 128, 200, 201, 250, 254, 255)]
        c0 = min(max(r - 7, 0), n - 14)
        return [c0 + k for k in range(14)]
    rp, ci = cases.uniform_rows(n, n, cols)
    rp2, ci2 = cases.hand_built(n, wide_row, wide_span, 14)
    assert np.array_equal(rp, rp2) and np.array_equal(ci, ci2)


@pytest.mark.parametrize("n", [N, 66_001])
@pytest.mark.parametrize("L", cases.LENGTHS)
def test_hand_built_wraps_every_ring(L, n):
    """For every ring of R = 256 p positions, p in [8, 255], that leaves room below the matrix's last column for a row
    of 600 columns past it (R + 700 <= n), one of the rows that spread over 600 columns starts inside the ring's last
    256 positions and wraps: whichever ring a plan picks, the GPU test meets the wrap.  At n = 66 001 that is every
    p up to 255 -- the descriptor's limit; at the GPU test's n = 40 037 every p up to 153, and LDS holds no ring above
    144 pages (160 KB less the strips, in f32 pages of 1 KB)."""
    rp, ci = cases.hand_built(n, 20_000, cases.max_span(L), L)
    t = ci.astype(np.int64).reshape(n, L)
    spread = np.flatnonzero(t[:, -1] - t[:, 0] == cases.SPREAD_SPAN)
    reached = []
    for p in range(8, 256):
        R = 256 * p
        if R + 700 > n:
            continue
        rows = cases.wrapping_rows(ci, L, R)
        assert np.intersect1d(rows, spread[spread % R >= R - 256]).size > 0, p
        reached.append(p)
    assert reached == list(range(8, 256 if n > N else 154)) and reached[-1] >= 144


@pytest.mark.parametrize("L", cases.LENGTHS)
def test_block_jumps(oracle, L):
    n, nc = 40_000, 50_001
    rp, ci = cases.block_jumps(np.random.default_rng(5), n, nc, L)
    check_structure(oracle, n, nc, rp, ci, L)
    t = ci.astype(np.int64).reshape(n, L)
    first = t[:, 0].reshape(-1)[::cases.JUMP_ROWS]
    jumps = np.diff(first)
    assert (jumps > 20_000).any() and (jumps < -20_000).any()          # forwards and backwards, windows apart
    assert np.all(t[:, -1] - t[:, 0] < cases.JUMP_SPAN) and (t[:, -1] == nc - 1).sum() > 500
    assert nc % 2 == 1


@pytest.mark.parametrize("L", cases.LENGTHS)
def test_packs_on_every_value_class(L):
    W = cases.value_width(L)
    for name, make in cases.VALUE_CLASSES.items():
        for size in (8, 64 * L + 5):
            va, expected = make(np.random.default_rng(3), size, L)
            assert va.dtype == np.float64 and va.size == size
            assert cases.packs(va, L) == expected, (name, size)
            assert expected[0] == (name in cases.PACKING), name
    assert cases.VALUE_CLASSES["extremes"](np.random.default_rng(0), 8, L)[1] == (True, 0, W)
    assert cases.VALUE_CLASSES["most_negative"](np.random.default_rng(0), 8, L)[1] == (True, 0, W + 1)
    # the bounds, one step to each side
    one = lambda k, e: np.array([np.ldexp(float(k), e), np.ldexp(3.0, e)])
    assert cases.packs(one(1 << 30, cases.EXP_MIN), L) == (True, cases.EXP_MIN, 32)
    assert cases.packs(one(1 << 30, cases.EXP_MAX), L) == (True, cases.EXP_MAX, 32)
    assert cases.packs(one(1 << 30, cases.EXP_MAX + 1), L)[0] is False
    assert cases.packs(np.array([2.0 ** -1023, 2.0 ** -1000]), L)[0] is False
    assert cases.packs(np.array([2.0 ** -1022, 2.0 ** -1000]), L) == (True, -1022, 24)
    assert cases.packs(np.array([-float(1 << (W - 1)), 1.0]), L) == (True, 0, W + 1)
    assert cases.packs(np.array([float(1 << (W - 1)), 1.0]), L)[0] is False
    assert cases.packs(np.array([float((1 << (W - 1)) - 1), -1.0]), L) == (True, 0, W)
    assert cases.packs(np.array([0.0, 0.0]), L) == (True, 0, 1)
    for odd in (np.nan, np.inf, -np.inf, -0.0):
        assert cases.packs(np.array([1.0, odd]), L)[0] is False
    # a third alone is 53 bits of 2^-54; among integers it is not a multiple of any quantum they fit beside
    assert cases.packs(np.array([1.0 / 3.0, 1000.0]), L)[0] is False


@pytest.mark.parametrize("L", cases.LENGTHS)
def test_synthetic_band_values_pack(L):
    """spal_synth's values are draws of m * 2^-52: they pack under every row length"""
    _, _, va = synth.banded_csr(N, N, L, 4096, 100 + L)
    assert cases.packs(va, L) == (True, -52, 53)
    rng = np.random.default_rng(14)
    assert cases.packs(rng.uniform(-1, 1, 1000), L) == (True, -52, 53)


@pytest.mark.parametrize("L", cases.LENGTHS)
def test_special_layout(oracle, L):
    s = cases.special_layout(L)
    n, rp, ci, va, x = s["n"], s["rowptr"], s["colind"], s["values"], s["x"]
    check_structure(oracle, n, n, rp, ci, L)
    assert n % 64 and n % 256                                   # pad rows in the last tile and in the last step
    assert cases.packs(va, L) == (True, 0, 11)
    for special in sc.x_specials(np.float64):
        assert np.isnan(x).any() if np.isnan(special) else (sc.bits(x) == sc.bits(np.array([special]))[0]).any(), special
    t, v = ci.astype(np.int64).reshape(n, L), va.reshape(n, L)
    zero_rows, neg = s["zero_rows"], s["neg_zero_rows"]
    assert np.all(sc.bits(v[zero_rows]) == 0) and np.array_equal(np.flatnonzero((v == 0).all(axis=1)), zero_rows)
    assert np.all(zero_rows[:3] == (0, 11, 22)) and n - 1 in neg and {63, 64, 319, 320} <= set(neg.tolist())
    assert np.all((x[t[neg]] < 0) & np.isfinite(x[t[neg]]))     # negative, ordinary x under them
    for tile in (0, 2, 3):
        assert sc.bits(va)[tile * 64 * L] == 0 and sc.bits(va)[(tile + 1) * 64 * L - 1] == 0
    assert np.count_nonzero(v[[127, 128, 191, 192, 255]]) > 0   # (inside rows of ordinary values)
    y = oracle.csr_spmv(rp, ci, va, x)
    neg_zero = sc.bits(np.array([-0.0]))[0]
    assert np.all(sc.bits(y)[neg] == neg_zero) and neg.size >= 100
    assert sc.bits(y)[n - 1] == neg_zero                        # the all-zero last row
    others = np.setdiff1d(zero_rows, neg)
    assert (sc.bits(y)[others] == 0).any()                      # +0.0 where the signs under a row of zeros mix
    nan_zero_rows = others[np.isnan(y[others])]
    assert nan_zero_rows.size >= 4                              # +0.0 * Inf (or NaN) under a row of zeros: NaN
    assert any(np.isinf(x[t[r]]).any() and not np.isnan(x[t[r]]).any() for r in nan_zero_rows)
    assert np.isnan(y).sum() >= 8 and np.isposinf(y).sum() >= 2 and np.isneginf(y).sum() >= 2
    assert np.isfinite(y).mean() > 0.5


def test_fuzz_cases_are_valid_and_cover(oracle):
    seen = {"L": set(), "pattern": set(), "n": set(), "dtype": set(), "class": set(), "wide": set(), "special": set()}
    for seed in range(SEEDS):
        c = cases.fuzz_case(seed)
        check_structure(oracle, c["n"], c["ncols"], c["rowptr"], c["colind"], c["L"], c["values"].size)
        assert c["values"].dtype == c["dtype"] == c["x"].dtype and c["x"].size == c["ncols"]
        assert c["dtype"] == (np.float64 if seed % 3 else np.float32) and c["n"] >= cases.MIN_ROWS
        if c["dtype"] == np.float64:
            assert cases.packs(c["values"], c["L"]) == c["expected"], (seed, c["value_class"])
        if c["pattern"] in cases.SLIDING:
            t = c["colind"].astype(np.int64).reshape(c["n"], c["L"])
            assert (t[:, -1] - t[:, 0]).max() <= min(6000, cases.max_span(c["L"]))     # every row fits a record
            seen["wide"].add(c["window_pages"])
            seen["L"].add((c["L"], c["dtype"].itemsize))
            seen["n"].add(c["n"])
            seen["class"].add(c["expected"][0])
            seen["special"].add((c["special_x"], c["dtype"].itemsize))
        seen["pattern"].add(c["pattern"])
    assert seen["pattern"] == set(cases.PATTERNS) and seen["wide"] == {0, 40}
    assert {L for L, _ in seen["L"]} == set(cases.LENGTHS) and {b for _, b in seen["L"]} == {4, 8}
    assert cases.MIN_ROWS in seen["n"] and len(seen["n"]) >= 5
    assert seen["class"] == {True, False} and (True, 8) in seen["special"] and (False, 8) in seen["special"]
    assert [cases.fuzz_case(s)["n"] for s in (0, 1)] == [cases.MIN_ROWS] * 2
