"""A small zoo of matrix structures, one per path the CSR planner can take (test infrastructure, host only).

A handle assembled on the device from COO triplets is planned lazily: whoever first needs the plan builds it (DESIGN,
"the contract of the lazy plan").  tests/test_gpu_lazy_plan.py takes every case here through that route and through the
upload from host arrays, which plans inside the create call.  Each case is the smallest at which the planner still
takes the path it is named for; tests/test_lazy_cases_host.py checks on the CPU that it still does, so no case can
drift off its path and pass vacuously on the GPU.

`case(name, dtype)` returns a `Case`: valid CSR arrays plus the same matrix as COO triplets in a shuffled insertion
order (no duplicates, no zeros: the assembly must return the CSR arrays bit for bit).  Cases are built once per process
and shared; nobody writes to their arrays.
"""
import collections
import functools

import numpy as np

import spal_synth as synth

Case = collections.namedtuple("Case", "name nrows ncols rowptr colind values rows cols vals")

SKEWED = ("skew_det", "skew_pareto", "skew_far", "skew_511")                 # meet the automatic row-split test
OTHERS = ("banded", "ragged", "long_rows", "hollow", "empty")               # ... and do not
NAMES = SKEWED + OTHERS
SQUARE = ("skew_det", "skew_pareto", "banded", "ragged")

SPLIT_THRESHOLD = 128        # CsrPlan::split_threshold: a row above it is a long row
PARETO_SEED = 3


def split_counts(nrows, rowptr, threshold=SPLIT_THRESHOLD):
    """(64-row tiles that hold a long row, tiles, entries of the short rows, entries): what csr_try_row_split counts."""
    lens = np.diff(np.asarray(rowptr).astype(np.int64))
    long_ = lens > threshold
    ntiles = (nrows + 63) // 64
    padded = np.zeros(ntiles * 64, dtype=bool)
    padded[:nrows] = long_
    tiles_hit = int(padded.reshape(ntiles, 64).any(axis=1).sum())
    nnz = int(lens.sum())
    return tiles_hit, ntiles, nnz - int(lens[long_].sum()), nnz


def auto_split_met(nrows, rowptr, threshold=SPLIT_THRESHOLD):
    """The automatic row-split test of csr_try_row_split (row_split = -1), restated: long rows keep a tenth of the
    64-row tiles from streaming, the short rows keep a quarter of the entries and average at most 64 per row."""
    tiles_hit, ntiles, nnz_short, nnz = split_counts(nrows, rowptr, threshold)
    if nrows < 2 or nnz == 0 or nnz_short == 0 or tiles_hit == 0:
        return False
    return tiles_hit * 10 >= ntiles and nnz_short >= nnz // 4 and nnz_short / nrows <= 64.0


def _csr_from_keys(nrows, ncols, rows, cols):
    """rows, cols (int64, duplicates allowed) -> rowptr, colind of the deduplicated pattern."""
    key = np.unique(rows * np.int64(ncols) + cols)
    r, c = key // ncols, key % ncols
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=nrows))]).astype(np.uint64)
    return rp, c.astype(np.uint64)


def _values(rng, n, dtype):
    v = rng.uniform(-1, 1, n).astype(dtype)
    v[v == 0] = 0.5        # (a stored zero would be dropped by the assembly)
    return v


def pareto_lengths(rng, nrows):
    """Power-law row lengths with the edge rows of test_block_window_kernel_on_power_law_rows: a row of several
    passes, the two sides of the thread / wave limit (33, 32), empty rows, and a run of empty rows longer than a
    block's unit where the matrix is tall enough to have one."""
    lens = np.minimum((rng.pareto(1.6, nrows) * 6 + 1).astype(np.int64), 3000)
    lens[:6] = (0, 3000, 33, 32, 0, 1)
    lens[700:1300] = 0
    return lens


def pareto_pattern(rng, nrows, ncols, half_window):
    """`pareto_lengths` rows; columns within +-half_window of the row (None: anywhere), deduplicated."""
    lens = pareto_lengths(rng, nrows)
    rows = np.repeat(np.arange(nrows, dtype=np.int64), lens)
    if half_window is None:
        cols = rng.integers(0, ncols, rows.size)
    else:
        cols = np.clip(rows - half_window + rng.integers(0, 2 * half_window, rows.size), 0, ncols - 1)
    return _csr_from_keys(nrows, ncols, rows, cols)


def _skew_det(nrows):
    """2048 x 2048: five entries within +-40 of the diagonal in every row, 200 within +-400 in rows 7, 327, 647, ...;
    `nrows` < 2048 keeps the first rows only (all 2048 columns)."""
    n = 2048
    rng = np.random.default_rng(2048)
    rows, cols = [], []
    for r in range(n):
        k, half = (200, 400) if r % 320 == 7 else (5, 40)
        lo, hi = max(0, r - half), min(n, r + half + 1)
        rows.append(np.full(k, r, dtype=np.int64))
        cols.append(lo + rng.choice(hi - lo, k, replace=False))
    rows, cols = np.concatenate(rows), np.concatenate(cols).astype(np.int64)
    keep = rows < nrows
    return (nrows, n) + _csr_from_keys(nrows, n, rows[keep], cols[keep])


def _ragged():
    """20 000 rows of 1 ... 27 entries in a band of 4096 columns."""
    n, band = 20_000, 4096
    rng = np.random.default_rng(27)
    lens = rng.integers(1, 28, n)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = np.clip(rows - band // 2 + rng.integers(0, band, rows.size), 0, n - 1)
    return (n, n) + _csr_from_keys(n, n, rows, cols)


def _long_rows():
    """3000 rows of 300 ... 400 distinct columns out of 5000 (test_long_rows_go_to_the_vector_kernel, longer rows)."""
    nr, nc = 3000, 5000
    rng = np.random.default_rng(140)
    lens = rng.integers(300, 401, nr)
    ci = np.concatenate([np.sort(rng.choice(nc, int(k), replace=False)) for k in lens])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return nr, nc, rp, ci.astype(np.uint64)


def _hollow():
    """3000 x 4099, only the last 100 rows hold entries (test_block_window_kernel_edge_shapes, case c)."""
    nr, nc, spread = 3000, 4099, 600
    rng = np.random.default_rng(21)
    lens = np.zeros(nr, np.int64)
    lens[-100:] = rng.integers(1, 200, 100)
    ci = []
    for r in range(nr - 100, nr):
        lo = max(0, min(nc - spread, int(r * nc / nr) - spread // 2))
        ci.append(lo + np.sort(rng.choice(spread, int(lens[r]), replace=False)))
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return nr, nc, rp, np.concatenate(ci).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _pattern(name):
    if name == "skew_det":
        return _skew_det(2048)
    if name == "skew_511":
        return _skew_det(511)
    if name == "skew_pareto":
        return (6000, 6000) + pareto_pattern(np.random.default_rng(PARETO_SEED), 6000, 6000, 2000)
    if name == "skew_far":
        return (6000, 300_008) + pareto_pattern(np.random.default_rng(PARETO_SEED), 6000, 300_008, None)
    if name == "banded":
        rp, ci, _ = synth.banded_csr(40_000, 40_000, 14, 2048, 17)
        return 40_000, 40_000, rp, ci
    if name == "ragged":
        return _ragged()
    if name == "long_rows":
        return _long_rows()
    if name == "hollow":
        return _hollow()
    if name == "empty":
        return 700, 701, np.zeros(701, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _case(name, dtype_name):
    dtype = np.dtype(dtype_name)
    nrows, ncols, rp, ci = _pattern(name)
    rng = np.random.default_rng(1000 + NAMES.index(name))
    va = _values(rng, ci.size, dtype)
    rows = np.repeat(np.arange(nrows, dtype=np.uint64), np.diff(rp.astype(np.int64)))
    perm = rng.permutation(ci.size)                      # the insertion order
    out = Case(name, nrows, ncols, rp, ci, va, rows[perm], ci[perm], va[perm])
    for a in out[3:]:
        a.setflags(write=False)
    return out


def case(name, dtype=np.float64) -> Case:
    return _case(name, np.dtype(dtype).name)


def x_for(c: Case) -> np.ndarray:
    """The right-hand side every test of a case multiplies by (seeded by the shape)."""
    return np.random.default_rng(c.ncols).uniform(-1, 1, c.ncols).astype(c.values.dtype)


# ---- randomised assemblies that meet the row-split test (test_coo_assembly_randomised_skewed) ---------------------------
RANDOM_SEEDS = 6


def _random_skewed_once(rng, dtype):
    nrows = int(rng.choice([600, 5000, 20_000]))
    dup_rate = float(rng.choice([0.0, 0.05, 0.5]))
    order = int(rng.choice(3))                            # 0 sorted, 1 reversed, 2 shuffled
    rp, ci = pareto_pattern(rng, nrows, nrows, 2000)
    r = np.repeat(np.arange(nrows, dtype=np.int64), np.diff(rp.astype(np.int64)))
    c = ci.astype(np.int64)
    n = r.size
    extra = np.flatnonzero(rng.random(n) < dup_rate)      # duplicates of stored positions, summed in insertion order
    r, c = np.concatenate([r, r[extra]]), np.concatenate([c, c[extra]])
    v = _values(rng, r.size, dtype)
    o = np.lexsort((c, r))                                # (stable: a duplicate stays behind its original)
    if order == 1:
        o = o[::-1]
    elif order == 2:
        o = rng.permutation(r.size)
    return nrows, r[o].astype(np.uint64), c[o].astype(np.uint64), v[o]


def random_skewed_coo(seed):
    """(nrows, rows, cols, vals, regenerated): a square power-law matrix as triplets -- height, duplicate rate and
    insertion order at random -- whose pattern meets the automatic row-split test; `regenerated` counts the draws
    thrown away because theirs did not.  Seeds 0 ... RANDOM_SEEDS - 1; every third one is f32."""
    dtype = np.float32 if seed % 3 == 2 else np.float64
    for sub in range(8):
        nrows, r, c, v = _random_skewed_once(np.random.default_rng(9000 + 100 * seed + sub), dtype)
        key = np.unique(r.astype(np.int64) * nrows + c.astype(np.int64))
        rp = np.concatenate([[0], np.cumsum(np.bincount(key // nrows, minlength=nrows))])
        if auto_split_met(nrows, rp):
            return nrows, r, c, v, sub
    raise AssertionError(f"seed {seed}: no draw met the row-split test")
