"""Special values for the product kernels: inputs with signed zeros, infinities, NaN and subnormals planted on purpose,
the rule that compares a product holding them with the oracle's, and the inputs of the leak check.

No GPU import: tests/test_special_cases_host.py checks, with the oracle alone, that every structure below carries every
class of row and that the rule rejects what it must; tests/test_gpu_special_values.py runs the kernels on the same inputs.

What a path promises: NaN and +-inf reach exactly the rows that reference them, on every path.  The paths
that keep the reference's order of additions return its bits -- -0.0 and subnormals included; the tree-summed and atomic
paths accumulate from +0.0, agree to the tolerance of tests/util.assert_spmv_close and may return +0.0 for -0.0."""
import functools

import numpy as np

from tests.util import assert_spmv_close

TOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-4}
CLASSES = ("neg_zero", "plus_minus_zero", "inf_minus_inf", "subnormal_product", "subnormal_sum")   # (+ "empty")
PER_CLASS = 8
BW_PASS, BW_UNIT, BW_TALLEST = 3072, 512, 4096     # spal_csr_blockwin.hip: entries per pass, rows per unit, tallest block


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def x_specials(dtype):
    """+0.0, -0.0, +inf, -inf, NaN, the smallest subnormal, the value just below the smallest normal"""
    dtype = np.dtype(dtype)
    tiny = np.finfo(dtype).tiny
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.nextafter(dtype.type(0), dtype.type(1)),
                     np.nextafter(tiny, dtype.type(0))], dtype=dtype)


def ordinary(rng, n, dtype):
    """+-[0.25, 1): finite, normal, nonzero"""
    return (rng.uniform(0.25, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(dtype)


def special_columns(ncols, rng):
    """Column 0, column ncols - 1, both sides of every multiple of 256 up to 4096, ~0.2 % of random columns."""
    fixed = [0, ncols - 1]
    for m in range(256, 4096 + 1, 256):
        fixed += [m - 1, m]
    fixed = [c for c in fixed if 0 <= c < ncols]
    rand = rng.choice(ncols, max(1, ncols // 500), replace=False)
    return np.unique(np.concatenate([np.asarray(fixed, dtype=np.int64), rand.astype(np.int64)]))


def cut_rows(rp):
    """Rows of the structure that a pass boundary of the block-window kernel cuts WHATEVER block height the plan picks: in a
    block that starts at a multiple of the tallest height (a block start at every height), the row that holds entry
    first + 3072 strictly inside, provided it lies in the block's first unit of 512 rows (where the lowest height's passes
    still count from the same first entry).  Only rows of 2 ... 32 entries (one thread sums them) whose neighbours are
    rows of 2 ... 32 entries too."""
    rp = np.asarray(rp, dtype=np.int64)
    n = rp.size - 1
    out = []
    for r0 in range(0, n, BW_TALLEST):
        e = rp[r0] + BW_PASS
        r = int(np.searchsorted(rp, e, side="right")) - 1
        if r <= r0 or r + 1 >= min(r0 + BW_UNIT, n) or not rp[r] < e < rp[r + 1]:
            continue
        if all(2 <= rp[q + 1] - rp[q] <= 32 for q in (r - 1, r, r + 1)):
            out.append(r)
    return np.asarray(out, dtype=np.int64)


def special_inputs(rp, ci, ncols, seed, dtype, cuts=False):
    """values and x for the structure (rp, ci) with special values planted, and the dedicated rows by class.

    Returns a dict: "values", "x", "rows" ({class: row indices}; "empty" are the structure's rows without entries), and
    with cuts=True "cut", "cut_before", "cut_after": the rows of cut_rows(rp) and their neighbours."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    rp = np.asarray(rp, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    n, nnz = rp.size - 1, int(rp[-1])
    lens = np.diff(rp)
    tiny = np.finfo(dtype).tiny
    # x: ordinary numbers, the specials in turn at the chosen columns
    x = ordinary(rng, ncols, dtype)
    cols = special_columns(ncols, rng)
    sx = x_specials(dtype)
    x[cols] = sx[np.arange(cols.size) % sx.size]
    is_special = np.zeros(ncols, dtype=bool)
    is_special[cols] = True
    # values: ordinary numbers; stored zeros of both signs at ~0.5 %, +-inf, NaN and subnormals at ~0.2 % of the entries
    va = rng.uniform(-1, 1, nnz).astype(dtype)
    if nnz:
        z = rng.choice(nnz, max(2, nnz // 200), replace=False)
        va[z] = np.array([0.0, -0.0], dtype=dtype)[np.arange(z.size) % 2]
        s = rng.choice(nnz, max(5, nnz // 500), replace=False)
        sub = np.nextafter(dtype.type(0), dtype.type(1))
        sv = np.array([np.inf, sub, -np.inf, tiny / 8, np.nan, -sub * 5], dtype=dtype)
        va[s] = sv[np.arange(s.size) % sv.size]
        # a stored zero times +-inf is the reference's NaN: every second entry under an infinite x stores a zero
        under_inf = np.flatnonzero(np.isinf(x[ci]))[::2]
        va[under_inf] = np.array([0.0, -0.0], dtype=dtype)[np.arange(under_inf.size) % 2]
    # dedicated rows: 2 ... 32 entries (one lane, one thread in every kernel), every column an ordinary x
    row_of = np.repeat(np.arange(n), lens)
    touched = np.bincount(row_of, weights=is_special[ci], minlength=n) > 0
    cand = (lens >= 2) & (lens <= 32) & ~touched
    out = {"rows": {"empty": np.flatnonzero(lens == 0)}}
    planted = {}
    if cuts:
        cut = cut_rows(rp)
        cut = cut[cand[cut] & cand[cut - 1] & cand[cut + 1]]
        out["cut"], out["cut_before"], out["cut_after"] = cut, cut - 1, cut + 1
        for k, r in enumerate(cut):
            planted[int(r)] = ("cut", k)
            planted[int(r) - 1] = (CLASSES[k % len(CLASSES)], k)
            planted[int(r) + 1] = (CLASSES[(k + 2) % len(CLASSES)], k)
        cand[np.concatenate([cut - 1, cut, cut + 1])] = False
    pool = np.flatnonzero(cand)
    want = PER_CLASS * len(CLASSES)
    assert pool.size >= want, f"the structure has {pool.size} rows of 2 ... 32 ordinary entries, {want} are needed"
    chosen = pool[np.linspace(0, pool.size - 1, want).astype(np.int64)]      # spread over the whole matrix
    for k, r in enumerate(chosen):
        planted[int(r)] = (CLASSES[k % len(CLASSES)], k)
    rows = {c: [] for c in CLASSES}
    zero_for = lambda xs, neg: np.where((xs > 0) == neg, -0.0, 0.0).astype(dtype)     # v with v * xs == (-0.0 if neg else +0.0)
    for r, (cls, k) in planted.items():
        e0, e1 = int(rp[r]), int(rp[r + 1])
        xs = x[ci[e0:e1]]
        if cls == "cut":
            # the first segment (before the pass boundary) is all -0.0; the second one -0.0 too (the carry itself is the
            # row's result) or ordinary numbers, in turn
            first = int(rp[r // BW_TALLEST * BW_TALLEST]) + BW_PASS - e0
            v = zero_for(xs, True)
            if k % 2:
                v[first:] = rng.uniform(0.25, 1, e1 - e0 - first).astype(dtype)
            va[e0:e1] = v
            if k % 2 == 0:
                rows["neg_zero"].append(r)
            continue
        if cls == "neg_zero":                       # every product -0.0: the reference returns -0.0
            v = zero_for(xs, True)
        elif cls == "plus_minus_zero":              # (+0.0) + (-0.0) + ...: +0.0
            v = zero_for(xs, True)
            v[0] = zero_for(xs[:1], False)[0]
        elif cls == "inf_minus_inf":                # +inf then -inf: NaN
            v = rng.uniform(-1, 1, e1 - e0).astype(dtype)
            v[0] = np.copysign(np.inf, xs[0])
            v[1] = -np.copysign(np.inf, xs[1])
        elif cls == "subnormal_product":            # one subnormal product, the others signed zeros
            v = zero_for(xs, k % 2 == 0)
            v[0] = dtype.type(tiny / 4) / xs[0]
        else:                                       # "subnormal_sum": two normal products that cancel into a subnormal
            v = zero_for(xs, k % 2 == 0)
            v[0] = dtype.type(tiny * 1.5) / xs[0]
            v[1] = -dtype.type(tiny * 1.25) / xs[1]
        va[e0:e1] = v
        rows[cls].append(r)
    out["rows"].update({c: np.asarray(sorted(v), dtype=np.int64) for c, v in rows.items()})
    out["values"], out["x"] = va, x
    return out


def spmv_bound(rp, ci, values, x, oracle):
    """sum |a||x| of the finite inputs (what the finite rows are measured against), as test_gpu_csr_spmv.check does"""
    clean = lambda a: np.nan_to_num(np.asarray(a, dtype=np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    return oracle.csr_abs_bound(rp, ci, clean(values), clean(x))


def assert_special_parity(y, y_ref, exact, bound, tol):
    """NaN at the same places (payload and sign of a NaN are the compiler's and the hardware's choice), +-inf at the same
    places with their signs; where `exact` (True, False or a row mask) every other element on its bit pattern (-0.0 and
    subnormals included); elsewhere the criterion of assert_spmv_close, without its absolute slack where the reference is
    subnormal."""
    y, y_ref = np.asarray(y), np.asarray(y_ref)
    assert y.shape == y_ref.shape and y.dtype == y_ref.dtype
    nan = np.isnan(y_ref)
    wrong = np.flatnonzero(np.isnan(y) != nan)
    assert wrong.size == 0, f"NaN at other places than the reference's: rows {wrong[:8]}, y {y[wrong[:8]]}, ref {y_ref[wrong[:8]]}"
    inf = np.isinf(y_ref)
    wrong = np.flatnonzero((np.isinf(y) != inf) | (inf & (y != y_ref)))
    assert wrong.size == 0, f"inf at other places or of another sign: rows {wrong[:8]}, y {y[wrong[:8]]}, ref {y_ref[wrong[:8]]}"
    exact = np.broadcast_to(np.asarray(exact, dtype=bool), y.shape)
    sel = exact & ~nan
    wrong = np.flatnonzero(sel & (bits(y) != bits(y_ref)))
    assert wrong.size == 0, (f"{wrong.size} rows differ in their bits: rows {wrong[:8]}, y {y[wrong[:8]]!r} "
                             f"({bits(y)[wrong[:8]]}), ref {y_ref[wrong[:8]]!r} ({bits(y_ref)[wrong[:8]]})")
    rest = ~exact & np.isfinite(y_ref)
    if rest.any():
        b = np.asarray(bound, dtype=np.float64)
        assert_spmv_close(y[rest], y_ref[rest], b[rest], tol)
        # a subnormal of the reference: the criterion's absolute 1e-300 lies above every f64 subnormal and would take a flushed
        # one -- these rows are held to tol * bound alone
        sub = rest & (y_ref != 0) & (np.abs(y_ref) < np.finfo(y_ref.dtype).tiny)
        err = np.abs(y[sub].astype(np.float64) - y_ref[sub].astype(np.float64))
        wrong = np.flatnonzero(sub)[err > tol * b[sub]]
        assert wrong.size == 0, f"subnormal rows beyond the tolerance (flushed?): rows {wrong[:8]}, y {y[wrong[:8]]!r}, ref {y_ref[wrong[:8]]!r}"


def leak_rows(n):
    """R: two long stretches of rows whose ends fall inside a tile"""
    return [(3, n // 4 + 3), (n // 2 + 5, 3 * n // 4 + 5)]


def rows_mask(n, R):
    m = np.zeros(n, dtype=bool)
    for lo, hi in R:
        m[lo:hi] = True
    return m


def poison_complement(rp, ci, ncols, R, x):
    """A copy of x in which every column that no row of R references holds NaN, +inf, -inf in turn."""
    rp = np.asarray(rp, dtype=np.int64)
    used = np.zeros(ncols, dtype=bool)
    for lo, hi in R:
        used[np.asarray(ci[int(rp[lo]):int(rp[hi])], dtype=np.int64)] = True
    xp = np.array(x, copy=True)
    free = np.flatnonzero(~used)
    xp[free] = np.array([np.nan, np.inf, -np.inf], dtype=xp.dtype)[np.arange(free.size) % 3]
    return xp


# ---- the structures of tests/test_gpu_special_values.py ---------------------------------------------------------------------
def from_row_cols(n, rows, cols, ncols):
    key = np.unique(np.asarray(rows, dtype=np.int64) * ncols + np.asarray(cols, dtype=np.int64))
    rp = np.concatenate([[0], np.cumsum(np.bincount(key // ncols, minlength=n))]).astype(np.uint64)
    return rp, (key % ncols).astype(np.uint64)


def near_rows(rng, lens, ncols, spread):
    """rows of the given lengths, their columns within `spread` of the row's own place (distinct inside a row: a row may come
    out a little shorter than asked)"""
    n = lens.size
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    centre = rows * ncols // n
    cols = np.clip(centre - spread // 2 + rng.integers(0, spread, rows.size), 0, ncols - 1)
    return from_row_cols(n, rows, cols, ncols)


def empty_some_rows(rp, ci, rows):
    """the same structure with the given rows emptied"""
    rp = np.asarray(rp, dtype=np.int64)
    lens = np.diff(rp)
    keep = np.ones(lens.size, dtype=bool)
    keep[np.asarray(rows, dtype=np.int64)] = False
    sel = np.repeat(keep, lens)
    return np.concatenate([[0], np.cumsum(lens * keep)]).astype(np.uint64), np.asarray(ci)[sel].astype(np.uint64)


def spread_rows(n, k=12):
    """k rows spread over the matrix, none at a tile's first place"""
    return (np.linspace(0, n - 1, k + 2)[1:-1].astype(np.int64) | 1)


def _synth(kind, n, per_row, window, seed, empties=True):
    import spal_synth as synth
    if kind == "ragged":
        rp, ci, _ = synth.ragged_csr(n, n, window, seed)
    else:
        rp, ci, _ = synth.banded_csr(n, n, per_row, window, seed)
    if empties:
        rp, ci = empty_some_rows(rp, ci, spread_rows(n))
    return n, n, rp, ci


def _ragged_lds():
    # rows of 0 ... 24 entries, 70 001 x 3000, columns within 512 of the row's place (so that half the rows leave columns unused)
    rng = np.random.default_rng(2)
    n, nc = 70_001, 3000
    lens = rng.integers(0, 25, n)
    lens[rng.random(n) < 0.1] = 0
    return (n, nc) + near_rows(rng, lens, nc, 512)


def _short_rows():
    # rows of 0 ... 3 entries within 300 columns of the diagonal: tiles of 256 rows, a lane sums four adjacent rows
    rng = np.random.default_rng(8)
    n = 70_001
    return (n, n) + near_rows(rng, rng.integers(0, 4, n), n, 600)


def _cblock():
    rng = np.random.default_rng(3)
    n, nc = 3000, 9000
    lens = rng.integers(0, 6, n)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    return (n, nc) + from_row_cols(n, rows, rng.integers(0, nc, rows.size), nc)


def _vector():
    # rows shorter, equal to and longer than every lane width, columns within 750 of the row's place, one row of 5000 entries last
    rng = np.random.default_rng(14)
    n, nc = 3001, 6000
    # (the rows of 130 and 700 entries are rarer than the others: a long row seldom stays finite)
    lens = rng.choice([0, 1, 2, 7, 14, 16, 17, 31, 33, 64, 65, 130, 700], n, p=[0.085] * 11 + [0.045, 0.02])
    lens[-1] = 0
    rp, ci = near_rows(rng, lens, nc, 1500)
    long_cols = np.sort(rng.choice(nc, 5000, replace=False)).astype(np.uint64)
    rp[-1] += 5000
    return n, nc, rp, np.concatenate([ci, long_cols])


def _bw_edge(which):
    """cases (a), (a'), (b), (c) of test_block_window_kernel_edge_shapes; (c) with 400 rows of entries instead of 100 (the
    dedicated rows need 40 short ones)"""
    rng = np.random.default_rng(21 + which)
    if which in (0, 1):
        n, nc, spread = 5000, 50_001, (6000, 40_000)[which]
        lens = rng.integers(1, 4, n)
        lens[2500] = spread
        lens[100:4900:400] = 0
    elif which == 2:
        n, nc, spread = 700, 701, 701
        lens = rng.integers(0, 6, n)
        lens[:10] = 0
        lens[200] = 701                            # (outside the leak check's rows: it references every column)
    else:
        n, nc, spread = 3000, 4099, 600
        lens = np.zeros(n, np.int64)
        lens[-400:] = rng.integers(1, 200, 400)
        lens[-400::2] = rng.integers(2, 20, 200)
        lens[-7:-1:2] = 0
    ci = []
    for r, k in enumerate(lens):
        k = int(min(k, nc))
        lo = max(0, min(nc - min(spread, nc), int(r * nc / n) - spread // 2))
        ci.append(lo + np.sort(rng.choice(min(spread, nc - lo), k, replace=False)))
    rp = np.concatenate([[0], np.cumsum([c.size for c in ci])]).astype(np.uint64)
    return n, nc, rp, np.concatenate(ci).astype(np.uint64)


def _pareto():
    """Power-law row lengths, columns within 2000 of the row, about 20 000 rows.  Every block of 4096 rows begins with 310 rows
    of exactly ten entries: entry 3072 of the block -- a pass boundary at every block height -- falls inside row 307, after
    its second entry; rows 306 and 308 are its neighbours."""
    rng = np.random.default_rng(12)
    n = 20_001
    lens = np.minimum((rng.pareto(1.6, n) * 6 + 1).astype(np.int64), 2000)
    lens[5200:5206] = (0, 9000, 33, 32, 0, 1)     # a row across three passes, the two sides of the thread / wave limit
    lens[700:1300:50] = 0
    lens[-3:] = (0, 40, 0)
    head = np.concatenate([np.arange(r0, min(r0 + 310, n)) for r0 in range(0, n, BW_TALLEST)])
    lens[head] = 0                                # (filled below, without duplicates)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    # columns within 2000 of the row (the leak check's rows then leave a fifth of the columns unused), the long row's within 5000
    half = np.where(rows == 5201, 5000, 2000)
    cols = np.clip(rows - half + rng.integers(0, 2 * half, rows.size), 0, n - 1)
    hr = np.repeat(head, 10)
    hc = np.clip(hr - 2000, 0, n - 4000) + 397 * np.tile(np.arange(10), head.size) + rng.integers(0, 300, hr.size)
    return (n, n) + from_row_cols(n, np.concatenate([rows, hr]), np.concatenate([cols, hc]), n)


STRUCTURES = {
    # name: (builder, has the structure rows without entries, are block-window cut rows planted)
    "ragged_lds": (_ragged_lds, True, False),
    "short_rows": (_short_rows, True, False),
    "global_banded": (lambda: _synth("banded", 300_000, 14, 20_000, 5), True, False),
    "slide_banded14": (lambda: _synth("banded", 180_333, 14, 4096, 77, empties=False), False, False),   # (uniform rows: the
    # sliding kernel's form that does not read rowptr takes a matrix whose rows ALL have one length -- none can be empty)
    "slide_ragged": (lambda: _synth("ragged", 180_333, 0, 4096, 77), True, False),
    "panels": (lambda: _synth("banded", 150_017, 14, 16_384, 5), True, False),
    "panels_wide": (lambda: _synth("banded", 150_017, 14, 40_000, 5), True, False),
    "cblock": (_cblock, True, False),
    "bw_a": (lambda: _bw_edge(0), True, False),
    "bw_a_windowless": (lambda: _bw_edge(1), True, False),
    "bw_b": (lambda: _bw_edge(2), True, False),
    "bw_c": (lambda: _bw_edge(3), True, False),
    "pareto": (_pareto, True, True),
    "vector": (_vector, True, False),
    "csc_band": (lambda: _synth("banded", 30_000, 14, 2048, 21), True, False),
    "mg_band": (lambda: _synth("banded", 120_000, 14, 4096, 17), True, False),
}


@functools.lru_cache(maxsize=None)
def structure(name):
    n, nc, rp, ci = STRUCTURES[name][0]()
    rp.setflags(write=False)
    ci.setflags(write=False)
    return n, nc, rp, ci


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """(nrows, ncols, rowptr, colind, special_inputs(...)) of a structure, generated once per process and left unchanged"""
    n, nc, rp, ci = structure(name)
    s = special_inputs(rp, ci, nc, seed=sum(map(ord, name)), dtype=dtype, cuts=STRUCTURES[name][2])
    s["values"].setflags(write=False)
    s["x"].setflags(write=False)
    return n, nc, rp, ci, s
