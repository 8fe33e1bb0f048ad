"""Inputs for the three forms of the sliding CSR kernel -- col16, row records (csr_rowrec.hpp), packed values
(csr_valpack.hpp) -- on matrices of uniform rows of 12, 14 or 16 entries: column structures that stress the ring and the
records, value classes on both sides of every bound of the packing rule, the packing rule itself restated in Python
integers, a layout of special operands, and the generator of the randomised test.

No GPU import: tests/test_slide_cases_host.py checks every builder and the rule with the oracle alone;
tests/test_gpu_slide_forms.py, test_gpu_rowrec.py and test_gpu_valpack.py run the kernels on the same inputs."""
import functools

import numpy as np

from tests import special_cases as sc

LENGTHS = (12, 14, 16)
PAGE = 256                     # csr_kernels.hpp: kPageCols
HIGH_BITS = 40                 # csr_rowrec.hpp: kRowrecHighBits
EXP_MIN, EXP_MAX = -1022, 970  # csr_valpack.hpp: the quantum 2^e is normal, (2^53) * 2^e finite
# The fewest rows at which the planner gives records (rowrec_plan, spal_csr_slide.hip): it wants the sliding plan's tiles
# to issue exactly L / 2 loads per array ("slide_S == L / 2"), and slide_S is the most 128-entry steps one tile of 64 rows
# needs.  Only a FULL tile of 64 rows of L entries needs L / 2; a matrix of fewer than 64 rows has one partial tile and
# keeps col16.
MIN_ROWS = 64


def value_width(L):
    """W: the signed bits of a field of a row block (csr_valpack.hpp: 53 for rows of 12, 54 for 14 and 16)"""
    return 53 if L == 12 else 54


def max_span(L, ring_pages=None):
    """rowrec_max_span: the widest row (last column - first) a record of L columns holds.  The L - 1 high parts are
    kept in unary in 40 bits -- bit (d >> 8) + (k - 1) for column k -- so the last one may be 39 - (L - 2) whole pages,
    with any low byte; and the row must fit the ring of ring_pages * 256 positions."""
    by_bits = (HIGH_BITS - 1 - (L - 2)) * PAGE + (PAGE - 1)
    if ring_pages is None:
        return by_bits
    return 0 if ring_pages == 0 else min(by_bits, ring_pages * PAGE - 1)


# ---- column structures ------------------------------------------------------------------------------------------------------
def uniform_rows(n, nc, cols_of_row, L=14):
    """rowptr and colind of n rows of L columns each; cols_of_row(r) gives row r's, checked ascending and inside nc"""
    ci = np.empty((n, L), dtype=np.uint64)
    for r in range(n):
        c = np.asarray(cols_of_row(r), dtype=np.uint64)
        assert c.size == L and np.all(np.diff(c.astype(np.int64)) > 0) and c[-1] < nc, (r, c)
        ci[r] = c
    return np.arange(n + 1, dtype=np.uint64) * L, ci.reshape(-1)


def from_table(ci, nc):
    """rowptr and colind of a table [n][L] of columns (checked: ascending inside every row, inside nc)"""
    ci = np.asarray(ci, dtype=np.int64)
    n, L = ci.shape
    assert np.all(np.diff(ci, axis=1) > 0) and ci.min() >= 0 and ci.max() < nc
    return np.arange(n + 1, dtype=np.uint64) * L, ci.reshape(-1).astype(np.uint64)


def ascending(rng, n, L, m):
    """[n][L] distinct ascending integers in [0, m) per row"""
    assert m >= L
    return np.sort(rng.integers(0, m - L + 1, (n, L)), axis=1) + np.arange(L)


# offsets of the rows that spread over 600 columns: low bytes 255 / 0 / 1 on both sides of two page boundaries
_SPREAD = {12: (0, 50, 255, 256, 257, 300, 400, 511, 512, 513, 599, 600),
           14: (0, 3, 50, 255, 256, 257, 300, 301, 400, 511, 512, 513, 599, 600),
           16: (0, 1, 3, 50, 255, 256, 257, 300, 301, 400, 511, 512, 513, 514, 599, 600)}
# ... and of the rows that hold all their columns in one page
_IN_PAGE = {12: (0, 1, 17, 31, 64, 100, 127, 128, 200, 250, 254, 255),
            14: (0, 1, 17, 30, 31, 64, 100, 127, 128, 200, 201, 250, 254, 255),
            16: (0, 1, 2, 17, 30, 31, 64, 100, 127, 128, 200, 201, 250, 253, 254, 255)}
SPREAD_EVERY, SPREAD_SPAN = 97, 600


def hand_built(n, wide_row, wide_span, L=14):
    """n x n, L per row.  Most rows hold consecutive columns around the diagonal (the first and the last rows clamped
    to the matrix); every 97th row spreads over 600 columns with low bytes 255 / 0 / 1 around a page boundary (whatever
    the ring's size R <= n - 700, one of them starts within 256 positions of the ring's end and wraps: 97 < 256); every
    97th + 5 row holds all its columns in the page of the diagonal; row `wide_row` spans `wide_span` columns."""
    r = np.arange(n, dtype=np.int64)
    ci = np.clip(r - L // 2, 0, n - L)[:, None] + np.arange(L)
    spread = r[(r % SPREAD_EVERY == 0) & (r + SPREAD_SPAN < n)]
    ci[spread] = spread[:, None] + np.asarray(_SPREAD[L])
    page = (r // PAGE) * PAGE
    one = r[(r % SPREAD_EVERY == 5) & (page + PAGE <= n)]
    ci[one] = page[one][:, None] + np.asarray(_IN_PAGE[L])
    ci[wide_row] = [wide_row + k for k in range(L - 1)] + [wide_row + wide_span]
    return from_table(ci, n)


def wrapping_rows(ci, L, R):
    """rows whose ring positions (column mod R) wrap: the first column's position lies above the last one's"""
    t = np.asarray(ci, dtype=np.int64).reshape(-1, L)
    return np.flatnonzero(t[:, 0] % R > t[:, -1] % R)


JUMP_ROWS, JUMP_SPAN = 2048, 2049


def block_jumps(rng, n, nc, L=14):
    """n x nc, L per row: block-diagonal sections of 2048 rows whose column ranges jump forwards and backwards between
    steps (entering pages on both sides, disjoint windows, synchronous page loads); inside a section the row's 2049
    columns slide with the row.  The rows clamped to the matrix's right edge end on its last column (with nc odd: inside
    a 16-byte vector of x).  nc >= 4200, so that two sections lie apart."""
    assert nc >= 4200
    top = nc - JUMP_SPAN
    starts = np.array([0, (3 * nc) // 5, nc // 25, top - 1000, (22 * nc) // 25, nc // 5, top - JUMP_ROWS, 0], dtype=np.int64)
    r = np.arange(n, dtype=np.int64)
    base = np.minimum(starts[(r // JUMP_ROWS) % starts.size] + r % JUMP_ROWS, top)
    t = base[:, None] + ascending(rng, n, L, JUMP_SPAN)
    t[base == top, -1] = nc - 1
    return from_table(t, nc)


def band(rng, n, nc, L, width):
    """L columns inside `width` columns that slide down the diagonal, clamped to the matrix (nc >= width)"""
    assert L <= width <= nc
    base = np.minimum(np.arange(n, dtype=np.int64), nc - width)
    return from_table(base[:, None] + ascending(rng, n, L, width), nc)


def clusters(rng, n, nc, L, width):
    """five clusters of 40 columns at fixed places inside `width` columns that slide down the diagonal (a stencil)"""
    assert 200 <= width <= nc
    bases = np.sort(rng.choice(width // 40, 5, replace=False)) * 40
    slot = ascending(rng, n, L, 200)
    base = np.minimum(np.arange(n, dtype=np.int64), nc - width)
    return from_table(base[:, None] + bases[slot // 40] + slot % 40, nc)


def anywhere(rng, n, nc, L):
    return from_table(ascending(rng, n, L, nc), nc)


# ---- the packing rule -------------------------------------------------------------------------------------------------------
def packs(values, L):
    """(packs, e, bits) of f64 values under rows of L, from the rule of csr_valpack.hpp: every value is k * 2^e for one
    quantum 2^e, e in [-1022, 970], every k fits W = value_width(L) signed bits, and no value is NaN, Inf or -0.0.
    e is the largest exponent that divides every value (0 where all are +0.0) and bits is what describe() prints: the
    bits of the largest |k| and one for the sign -- W + 1 for k = -2^(W-1), which W signed bits hold, as for
    k = +2^(W-1), which they do not.  (False, None, None) where the values do not pack."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    no = (False, None, None)
    if not np.all(np.isfinite(v)) or np.any((v == 0) & np.signbit(v)):
        return no
    nz = v[v != 0]
    if nz.size == 0:
        return (True, 0, 1)
    frac, ex = np.frexp(nz)                                 # nz = frac * 2^ex, 0.5 <= |frac| < 1, exact (subnormals too)
    mant = np.ldexp(np.abs(frac), 53).astype(np.int64)      # |nz| = mant * 2^(ex - 53), 2^52 <= mant < 2^53
    ex = ex.astype(np.int64) - 53
    low = mant & -mant                                      # the lowest set bit
    tz = np.round(np.log2(low.astype(np.float64))).astype(np.int64)
    e = int((ex + tz).min())
    k_of = lambda i: (int(mant[i]) >> int(tz[i])) << (int(ex[i] + tz[i]) - e)     # |nz[i]| / 2^e, a Python integer
    k_max = k_of(int(np.argmax(nz))) if nz.max() > 0 else 0
    k_min = k_of(int(np.argmin(nz))) if nz.min() < 0 else 0
    W = value_width(L)
    if not (EXP_MIN <= e <= EXP_MAX) or k_max > (1 << (W - 1)) - 1 or k_min > (1 << (W - 1)):
        return no
    return (True, e, 1 + max(k_max, k_min).bit_length())


# ---- value classes ----------------------------------------------------------------------------------------------------------
# name -> f(rng, size, L) -> (f64 values, (packs, e, bits)): the expected triple is stated by the class, from how it
# plants its values, not computed by packs().  size >= 8.
def _signs(rng, size):
    return rng.choice(np.array([-1, 1], dtype=np.int64), size)


def _integers(rng, size, L):
    k = rng.integers(1, 1001, size) * _signs(rng, size)
    k[:3] = (3, -1000, 1)                                   # an odd one: e = 0; the largest: 10 bits and the sign
    return k.astype(np.float64), (True, 0, 11)


def _unit_draws(rng, size, L):
    # what rng.uniform(-1, 1) returns: m * 2^-52, |m| < 2^52
    k = rng.integers(-(1 << 52) + 1, 1 << 52, size)
    k[:2] = ((1 << 52) - 1, -3)
    return np.ldexp(k.astype(np.float64), -52), (True, -52, 53)


def _born_f32(rng, size, L):
    # f32 numbers in +-[0.5, 1): k * 2^-24, 2^23 <= |k| < 2^24
    v = (rng.uniform(0.5, 1.0, size) * _signs(rng, size)).astype(np.float32)
    v[0] = np.float32(1.0) - np.float32(2.0 ** -24)         # k = 2^24 - 1, odd
    return v.astype(np.float64), (True, -24, 25)


def _scaled(e, lo_bits=20, hi_bits=40):
    def make(rng, size, L):
        k = rng.integers(1 << lo_bits, 1 << hi_bits, size) * _signs(rng, size)
        k[:2] = ((1 << hi_bits) - 1, -(1 << lo_bits) - 1)   # the widest, and an odd one
        return np.ldexp(k.astype(np.float64), e), (True, e, hi_bits + 1)
    return make


def _drawn_quantum(rng, size, L):
    return _scaled(int(rng.integers(EXP_MIN, EXP_MAX + 1)))(rng, size, L)


def _quantum_min_units(rng, size, L):
    # k = +-1 at e = -1022: every product with |x| < 1 and every sum of them is subnormal
    return np.ldexp(_signs(rng, size).astype(np.float64), EXP_MIN), (True, EXP_MIN, 2)


def _zeros_only(rng, size, L):
    return np.zeros(size), (True, 0, 1)


def _extremes(rng, size, L):
    W = value_width(L)
    top = float((1 << (W - 1)) - 1)
    v = rng.choice(np.array([top, -top, 1.0, -1.0]), size)
    v[:4] = (top, 1.0, -top, -1.0)
    return v, (True, 0, W)


def _most_negative(rng, size, L):
    W = value_width(L)
    v = rng.choice(np.array([1.0, -1.0, 3.0]), size)
    v[:2] = (-float(1 << (W - 1)), 1.0)
    return v, (True, 0, W + 1)


def _one_too_large(rng, size, L):
    W = value_width(L)
    v = rng.choice(np.array([1.0, -1.0, 3.0]), size)
    v[:2] = (float(1 << (W - 1)), 1.0)
    return v, (False, None, None)


def _quantum_below(rng, size, L):
    v, _ = _scaled(EXP_MIN)(rng, size, L)
    v[size // 2] = 2.0 ** -1023                             # a subnormal whose lowest bit is 2^-1023
    return v, (False, None, None)


def _quantum_above(rng, size, L):
    k = rng.integers(1, 1 << 20, size) * _signs(rng, size)
    k[0] = 3
    return np.ldexp(k.astype(np.float64), EXP_MAX + 1), (False, None, None)


def _far_apart(rng, size, L):
    v = rng.choice(np.array([1.0, -1.0]), size)
    v[size // 2] = float(1 << value_width(L))               # k = 2^W beside k = 1
    return v, (False, None, None)


def _with_one(odd):
    def make(rng, size, L):
        v, _ = _integers(rng, size, L)
        v[size - 3] = odd
        return v, (False, None, None)
    return make


VALUE_CLASSES = {
    "integers": _integers, "unit_draws": _unit_draws, "born_f32": _born_f32, "drawn_quantum": _drawn_quantum,
    "quantum_min": _scaled(EXP_MIN), "quantum_max": _scaled(EXP_MAX), "quantum_min_units": _quantum_min_units,
    "zeros_only": _zeros_only, "extremes": _extremes, "most_negative": _most_negative,
    "one_too_large": _one_too_large, "quantum_below": _quantum_below, "quantum_above": _quantum_above,
    "far_apart": _far_apart, "one_nan": _with_one(np.nan), "one_inf": _with_one(np.inf),
    "one_negative_zero": _with_one(-0.0), "a_third": _with_one(1.0 / 3.0),
}
PACKING = ("integers", "unit_draws", "born_f32", "drawn_quantum", "quantum_min", "quantum_max", "quantum_min_units",
           "zeros_only", "extremes", "most_negative")


def half_to_one(rng, size, dtype=np.float64):
    """+-[0.5, 1): with values k * 2^e, |k| >= 2^20, every product is normal and every sum of 16 finite"""
    return (rng.uniform(0.5, 1.0, size) * rng.choice([-1.0, 1.0], size)).astype(dtype)


def special_x(rng, nc, dtype):
    """half_to_one with special_cases.x_specials in turn at special_cases.special_columns"""
    x = half_to_one(rng, nc, dtype)
    cols = sc.special_columns(nc, rng)
    sx = sc.x_specials(dtype)
    x[cols] = sx[np.arange(cols.size) % sx.size]
    return x


# ---- special operands under packable values -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def special_layout(L, n=10_037, width=4096, seed=41):
    """n x n, L per row inside a band, values that pack (non-zero integers and stored +0.0), x with every special:
      - every 11th row stores +0.0 only.  Under every 8th of them (and under the rows below) x is made negative and
        ordinary: the row's first product is -0.0 and is ASSIGNED, every further one adds -0.0: the result is -0.0.
        The other rows of zeros meet x as it comes: +0.0, -0.0, or NaN where an Inf or NaN lies under them;
      - the rows on both sides of a tile's end (63 | 64, 64 * 5 - 1 | 64 * 5, the last full tile's end) and the last
        row of the matrix store +0.0 only, with negative x under them;
      - stored zeros at the first and the last entry of tiles 0, 2 and 3 (inside rows of ordinary values).
    Returns a dict: n, L, rowptr, colind, values, x, zero_rows, neg_zero_rows (all read-only)."""
    rng = np.random.default_rng(seed + L)
    rp, ci = band(rng, n, n, L, width)
    va = (rng.integers(1, 1001, ci.size) * _signs(rng, ci.size)).astype(np.float64)
    va[:2] = (3.0, 1000.0)
    x = special_x(rng, n, np.float64)
    zero_rows = np.arange(0, n, 11)
    last_tile = (n // 64) * 64
    edges = np.array([63, 64, 64 * 5 - 1, 64 * 5, last_tile - 1, last_tile, n - 1])
    neg_zero_rows = np.unique(np.concatenate([zero_rows[::8], edges]))
    zero_rows = np.unique(np.concatenate([zero_rows, edges]))
    t = ci.reshape(n, L).astype(np.int64)
    under = np.unique(t[neg_zero_rows])
    x[under] = -rng.uniform(0.5, 1.0, under.size)
    va.reshape(n, L)[zero_rows] = 0.0
    for tile in (0, 2, 3):
        va[tile * 64 * L] = 0.0
        va[(tile + 1) * 64 * L - 1] = 0.0
    out = {"n": n, "L": L, "rowptr": rp, "colind": ci, "values": va, "x": x, "zero_rows": zero_rows,
           "neg_zero_rows": neg_zero_rows}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---- the randomised test's generator --------------------------------------------------------------------------------------
FUZZ_ROWS = (64, 65, 255, 257, 1000, 4097, 20_011)          # (64 = MIN_ROWS: no plan below it has records)
FUZZ_COLS = (256, 257, 2049, 0, 40_000, 300_007)            # (0: ncols = nrows)
PATTERNS = ("band", "clusters", "jumps", "anywhere")
SLIDING = PATTERNS[:3]
# A super-tile of 1024 rows is staged whole where its span holds at most the plan's page budget; the automatic budget
# of an f64 plan is 24 pages.  Rows that slide with the diagonal span width + 1023 columns per super-tile, and a page
# more for the alignment: above this width the test asks for 40 pages ("window_pages"), as for the widest record.
WIDE = 24 * PAGE - 1024 - PAGE


def fuzz_case(seed):
    """The case of a seed: dtype f64 on two seeds of three, x special on one seed of three (independently); L, n,
    ncols, the column pattern, the band's width and the value class are drawn.  Seeds 0 and 1 sit on MIN_ROWS with a
    sliding pattern.  ncols is raised to hold the pattern: the band's width; 4200 for the block jumps; 40 000 for
    "anywhere", so that no super-tile's columns fit a window and the plan has no sliding kernel at all."""
    rng = np.random.default_rng(7000 + seed)
    dtype = np.dtype(np.float64 if seed % 3 else np.float32)
    special = (seed // 3) % 3 == 2
    L = int(rng.choice(LENGTHS))
    n = int(rng.choice(FUZZ_ROWS))
    nc = int(rng.choice(FUZZ_COLS)) or n
    pattern = str(rng.choice(PATTERNS))
    width = int(rng.integers(L, 6001))
    if seed < 2:
        n, pattern = MIN_ROWS, SLIDING[seed]
    if pattern == "band":
        nc = max(nc, width, PAGE)
        rp, ci = band(rng, n, nc, L, width)
    elif pattern == "clusters":
        width = max(width, 200)
        nc = max(nc, width, PAGE)
        rp, ci = clusters(rng, n, nc, L, width)
    elif pattern == "jumps":
        width = JUMP_SPAN
        nc = max(nc, 4200)
        rp, ci = block_jumps(rng, n, nc, L)
    else:
        nc = max(nc, 40_000)
        rp, ci = anywhere(rng, n, nc, L)
    if dtype == np.float64:
        name = str(rng.choice(sorted(VALUE_CLASSES)))
        va, expected = VALUE_CLASSES[name](rng, ci.size, L)
    else:
        name = "f32"
        va = rng.uniform(-1, 1, ci.size).astype(np.float32)
        if rng.random() < 1 / 3:
            va[rng.integers(0, va.size, 3)] = np.array([np.nan, np.inf, -0.0], dtype=np.float32)
        expected = (False, None, None)
    x = special_x(rng, nc, dtype) if special else half_to_one(rng, nc, dtype)
    return {"seed": seed, "dtype": dtype, "L": L, "n": n, "ncols": nc, "pattern": pattern, "width": width,
            "value_class": name, "expected": expected, "special_x": special, "rowptr": rp, "colind": ci, "values": va,
            "x": x, "window_pages": 40 if pattern in SLIDING and width > WIDE else 0}
