"""Seeded random inputs for the solver stack -- the exact triangular solves, the Jacobi sweeps, ILU(0), CG and BiCGStab --
and two host restatements of what describe() must report about their schedules (test infrastructure, plain numpy, no
GPU).

The hand-made structures of tests/trsv_ref.py isolate one boundary each.  `case(seed)` mixes them inside one matrix:
row-length laws, column placements that give deep chains or wide levels, stretches of diagonal-only rows, stretches
whose rows all read the one row in front of them (a wide level in the middle of narrow ones), planted rows of
hundreds or thousands of entries, three ways to fill the other triangle, and now and then a missing diagonal.  The
knobs that steer the device's schedule (trsv_chain_rows, ilu_wide_work, sweep counts, the Krylov method, its
preconditioner, poll interval and maxit) are dealt or drawn with the matrix.  tests/test_solver_cases_host.py holds the
default seeds to the conditions the device test relies on, so that it cannot pass by testing nothing.

`expected_launches` and `expected_wide_rows` are written from the text of include/spal.h and DESIGN 3.11 / 3.12, not
from the kernels.
"""
import functools

import numpy as np

from . import ilu_ref as ir
from . import krylov_ref as kr
from . import sweep_ref as sw
from . import trsv_ref as tr

DEFAULT_SEEDS = 24
BASE_SEED = 20261100

SIZES = (1, 2, 255, 256, 257, 1025, 3000, 5000, 8000)
# n by seed % 12 (the placement goes by seed % 3, so every placement meets the three large sizes); the two smallest sizes
# take the places of seeds 22 and 23 of every 24
N_TABLE = (8000, 3000, 5000, 257, 8000, 1025, 5000, 255, 3000, 8000, 256, 5000)
LAWS = ("constant", "uniform", "pareto", "two_regions")
PLACEMENTS = ("near", "anywhere", "blocks")
WINDOWS = (1, 4, 64, 600)
BLOCKS = (255, 256, 257, 1023, 1024, 1025, 2049)
HEAVY = (255, 256, 257, 700, 2047, 2048, 2049, 2600)
PARETO_CAP = 3000
STRETCH = 1500
OTHER = ("transpose", "nothing", "independent")
CHAIN_ROWS = (0, 1, 64, 256, 1024, 1025, 1 << 40)
WIDE_WORK = (0, 8, 64, 4096, None, 1 << 40)          # None: the handle's default ...
WIDE_WORK_DEFAULT = 4096                             # ... kIluWideWorkDefault (the host test reads spal_internal.hpp)
METHODS = ("cg", "bicgstab")
PRECS = ("none", "exact", "sweeps0", "sweeps2")
PREC_SWEEPS = {"sweeps0": 0, "sweeps2": 2}
CHECK_EVERY = (1, 2, 3, 8)
MAXIT = (0, 1, 4, 7)
TOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-5}
# The host reference of s sweeps costs s times the longest row numpy operations: the drawn sweep count stays below this
# product (the counts 0, 1, 2 do not depend on it, and from levels - 1 on the reference is the exact solve).
SWEEP_BUDGET = 30_000


# ---- the two restatements --------------------------------------------------------------------------------------------

def expected_launches(level_widths, chain_rows):
    """(launches, chain launches) of a triangle whose levels hold `level_widths` rows: a maximal run of consecutive
    levels of at most `chain_rows` rows is one chain launch, every other level is a launch of its own."""
    launches = chains = 0
    in_run = False
    for w in level_widths:
        if w <= chain_rows:
            if not in_run:
                launches, chains = launches + 1, chains + 1
            in_run = True
        else:
            launches += 1
            in_run = False
    return launches, chains


def row_work(pattern):
    """(work, rows with an entry below the diagonal): work[i] = the sum, over the stored (i, k) with k < i, of the number
    of entries row k stores past its diagonal -- the updates ILU(0) looks for in row i."""
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    cols = colind.astype(np.int64)
    past = np.bincount(rows[cols > rows], minlength=n)
    below = cols < rows
    work = np.bincount(rows[below], weights=past[cols[below]], minlength=n).astype(np.int64)
    return work, np.bincount(rows[below], minlength=n) > 0


def expected_wide_rows(pattern, wide_work):
    """How many rows ILU(0) takes in its wide form: those with an entry below the diagonal and work >= wide_work."""
    work, has_lower = row_work(pattern)
    return int((has_lower & (work >= wide_work)).sum())


# ---- the lower triangle ----------------------------------------------------------------------------------------------

def _lengths(rng, law, n):
    if law == "constant":
        lens = np.full(n, int(rng.choice([1, 2, 3, 6])))
    elif law == "uniform":
        lens = rng.integers(0, int(rng.choice([3, 8, 16])) + 1, n)
    elif law == "pareto":
        lens = np.minimum((rng.pareto(1.5, n) * 2 + 1).astype(np.int64), PARETO_CAP)
    elif law == "two_regions":
        lens = np.where(np.arange(n) < n // 2, rng.integers(0, 3, n), rng.integers(4, 12, n))
    else:
        raise AssertionError(law)
    return lens.astype(np.int64)


def _lower(rng, n, law, placement):
    """Entries strictly below the diagonal as (rows, cols), and the diagonal-only stretches [(first, end)].  Duplicate
    draws fall together later, so a row may come out shorter than its drawn length."""
    i = np.arange(n, dtype=np.int64)
    lens = np.minimum(_lengths(rng, law, n), i)
    fan = np.full(n, -1, dtype=np.int64)            # the one row a row of a fan stretch reads
    bare = []
    for _ in range(int(rng.integers(0, 4))):
        a, ln = int(rng.integers(0, n)), int(rng.integers(1, STRETCH + 1))
        if rng.random() < 0.5:
            bare.append((a, min(a + ln, n)))        # these rows store their diagonal alone
        else:
            fan[a:a + ln] = max(a - 1, 0)           # these read the row in front of the stretch alone: one level
            lens[a:a + ln] = 1 if a else 0
    rows = np.repeat(i, lens)
    u = rng.random(rows.size)
    if placement == "near":
        w = int(rng.choice(WINDOWS))
        cols = rows - 1 - (u * np.minimum(w, rows)).astype(np.int64)
    elif placement == "anywhere":
        cols = (u * rows).astype(np.int64)
    elif placement == "blocks":
        blk = int(rng.choice(BLOCKS))
        first = (rows // blk - 1) * blk             # the block in front; block 0 reads nothing
        cols = np.where(first >= 0, first + (u * blk).astype(np.int64), -1)
    else:
        raise AssertionError(placement)
    cols = np.where(fan[rows] >= 0, fan[rows], cols)
    keep = cols >= 0
    rows, cols = [rows[keep]], [cols[keep]]
    for _ in range(int(rng.integers(1, 5))):        # planted rows, their columns anywhere below
        h = int(rng.choice(HEAVY))
        r = int(rng.integers(min(h, n - 1), n))
        c = rng.choice(r, size=min(h, r), replace=False) if r else np.empty(0, dtype=np.int64)
        rows.append(np.full(c.size, r, dtype=np.int64))
        cols.append(c.astype(np.int64))
    return np.concatenate(rows), np.concatenate(cols), bare


def first_row_without_diagonal(pattern):
    """The first row that stores no (i, i), or None."""
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    has = np.zeros(n, dtype=bool)
    has[rows[rows == colind.astype(np.int64)]] = True
    missing = np.flatnonzero(~has)
    return int(missing[0]) if missing.size else None


def _sweep_counts(rng, pattern, lower, nlevels):
    """0, 1, 2, one drawn value in [3, levels) (kept inside SWEEP_BUDGET), levels - 1 and levels + 3."""
    p0, p1, _, _ = sw.triangle_ranges(*pattern, lower)
    longest = int((p1 - p0).max()) if pattern[0] else 0
    counts = {0, 1, 2, max(nlevels - 1, 0), nlevels + 3}
    hi = min(nlevels, 3 + SWEEP_BUDGET // max(longest, 1))
    if hi > 3:
        counts.add(int(rng.integers(3, hi)))
    return tuple(sorted(counts))


# ---- a case ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(seed):
    """(pattern, values, b, x0, knobs) of one seed; built once per process, shared, read-only.

    knobs: n, law, placement, other, dropped (the rows whose diagonal is not stored, ascending; () on five seeds in six),
    dtype, kind ("csr" / "csc"), chain_rows and chain_rows_2, wide_work, levels = {True: lower, False: upper},
    sweeps = {True: counts for the lower triangle, False: for the upper}, method, prec, check_every and check_every_2,
    maxit, tol, in_place."""
    rng = np.random.default_rng(BASE_SEED + seed)
    n = {22: 1, 23: 2}.get(seed % 24, N_TABLE[seed % 12])
    placement = PLACEMENTS[seed % 3]
    method = METHODS[seed % 2]
    prec = PRECS[(seed // 2) % 4]
    dropping = seed % 6 == 5                        # (odd seeds: BiCGStab's, so every CG seed keeps its diagonal)
    law = LAWS[int(rng.integers(len(LAWS)))]
    other = OTHER[int(rng.integers(len(OTHER)))]

    lr, lc, bare = _lower(rng, n, law, placement)
    rows, cols = [lr], [lc]
    if other == "transpose":
        rows.append(lc)
        cols.append(lr)
    elif other == "independent":
        ur, uc, more = _lower(rng, n, LAWS[int(rng.integers(len(LAWS)))], PLACEMENTS[int(rng.integers(3))])
        rows.append(n - 1 - ur)
        cols.append(n - 1 - uc)
        bare += [(n - e, n - a) for a, e in more]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    if method == "cg":                              # CG wants a symmetric matrix: the union with the transpose
        rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    alone = np.zeros(n, dtype=bool)
    for a, e in bare:
        alone[a:e] = True
    keep = ~alone[rows] & (~alone[cols] if method == "cg" else True)
    d = np.arange(n, dtype=np.int64)
    dropped = ()
    if dropping:
        dropped = tuple(sorted(int(r) for r in rng.choice(n, size=min(n, int(rng.integers(1, 4))), replace=False)))
        d = np.setdiff1d(d, dropped)
    pattern = tr.from_coo(n, np.concatenate([rows[keep], d]), np.concatenate([cols[keep], d]))

    dtype = np.dtype((np.float64, np.float32)[int(rng.integers(2))])
    values, b = (kr.spd_fill if method == "cg" else tr.fill)(pattern, dtype, rng)
    x0 = rng.uniform(-1, 1, size=n).astype(dtype)
    levels = {lower: tr.levels(*pattern, lower=lower)[1] for lower in (True, False)}
    chain_rows = CHAIN_ROWS[seed % len(CHAIN_ROWS)]
    every = rng.choice(CHECK_EVERY, size=2, replace=False)
    knobs = dict(
        n=n, law=law, placement=placement, other=other, dropped=dropped, dtype=dtype,
        kind=("csr", "csc")[int(rng.integers(2))],
        chain_rows=chain_rows,
        chain_rows_2=int(rng.choice([c for c in CHAIN_ROWS if c != chain_rows])),
        wide_work=WIDE_WORK[(seed // 2) % len(WIDE_WORK)],
        levels=levels,
        sweeps={lower: _sweep_counts(rng, pattern, lower, levels[lower]) for lower in (True, False)},
        method=method, prec=prec, check_every=int(every[0]), check_every_2=int(every[1]),
        # the three seeds of every 24 that share a method and a preconditioner get three different limits
        maxit=MAXIT[(seed + seed // 8) % len(MAXIT)], tol=TOL[dtype], in_place=bool(rng.random() < 0.5))
    for a in (*pattern[1:], values, b, x0):
        a.setflags(write=False)
    return pattern, values, b, x0, knobs


def host_preconditioner(pattern, factor_values, prec):
    """v -> M^-1 v on the host for a preconditioner mode of PRECS: None, the two exact solves on the factor, or its
    sweeps."""
    if prec == "none":
        return None
    if prec == "exact":
        return lambda v: tr.solve_by_levels(*pattern, factor_values,
                                            tr.solve_by_levels(*pattern, factor_values, v, True, True), False, False)
    return sw.preconditioner(pattern, factor_values, PREC_SWEEPS[prec])


def to_handle_arrays(kind, pattern, values):
    """(ptr, ind, values) as the constructor of a handle of `kind` takes them."""
    if kind == "csr":
        return pattern[1], pattern[2], values
    colptr, rowind, vals, _ = ir.to_csc(pattern, values)
    return colptr, rowind, vals
