"""Seeded random inputs for the aggregation AMG and a host restatement of what describe()["rounds"] must report (test
infrastructure, plain numpy, no GPU).

The hand-made inputs of tests/amg_ref.py are grids, paths, stars and `hubs`.  `case(seed)` mixes, inside one matrix, what
none of them has: an irregular main graph (random edges inside a window of 2, 50 or n, stored both ways on half the
seeds and one way, in a drawn direction, on the others), about 5 % of isolated vertices, one or two hubs whose row -- and, for the first, whose
aggregate -- has a length around kLong = 32 and the steps of 64, now and then a separate path laid along descending
priority (its rounds land around the poll batches 8, 8 + 16, 8 + 16 + 32 while the rest of the graph finished long ago),
and on the integer seeds a separate path with zero row sums, whose aggregates' sums cancel exactly: the COO assembly drops
the coarse diagonal and the "diagonal" rule stops the build some levels down.  n puts level 0 on both sides of 256
(kThreads), 1024 (kTailThreads, the default "amg_tail_rows") and 4096 (the clamp); "amg_tail_rows" settings are computed
from the reference's level sizes so that every seed moves the tail's first level.

A descending path of L vertices is decided in L - 1 rounds (its two ends have degree 1, so the second vertex of the
order is the first root and the first vertex joins it in round 1 beside the third): the lengths 9, 25 and 57 give
exactly 8, 24 and 56 rounds -- the last round of a batch -- and 10, 26 and 58 the first of the next.  That is why
PATH_LENGTHS holds one length more at each batch than the round counts it aims at.

tests/test_amg_cases_host.py holds the default seeds to the conditions the device test relies on.
"""
import functools

import numpy as np

from . import amg_ref as ar
from . import colour_ref as cr

DEFAULT_SEEDS = 24
BASE_SEED = 20261900

N_TABLE = (1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 12000)
WINDOWS = (2, 50, None)                              # None: n
HUB_LENGTHS = (31, 32, 33, 63, 64, 65, 129, 300)
PATH_LENGTHS = (7, 8, 9, 10, 23, 24, 25, 26, 55, 56, 57, 58)
ZERO_SUM_LENGTHS = (5, 12, 40, 120)
SEEDS = (0, 7, 2**32 + 5, 2**40 + 123)
MAX_LEVELS = (1, 2, 3, 16)
COARSE_ROWS = (0, 4, 64, 10**9)
# max_levels by seed % 12 (16 elsewhere; 1 on seed % 24 == 13) and the seeds (mod 12) whose coarse_rows is 10^9: a single
# level.  The other seeds take 0, 4 and 64 in turn, so the integer seeds and the seeds with a path all build levels.
MAX_LEVELS_DEAL = {5: 2, 8: 3}
SINGLE_LEVEL = (0, 2)
NU = (1, 2, 3, 16)
COARSE_SWEEPS = (1, 2, 16, 17)
OMEGA = (2.0 / 3.0, 0.8, 1.0)
ALPHA = (1.0, 1.5, 0.75)
METHODS = ("cg", "bicgstab")
MAXIT = (0, 1, 4)
TOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-5}
TAIL_DEFAULT, TAIL_CLAMP = 1024, 4096                # kTailRowsDefault, kTailRowsMax (the host test reads spal_amg.hip)


# ---- the rounds ------------------------------------------------------------------------------------------------------

def expected_rounds(pattern, seed=0):
    """describe()["rounds"] of a level with this pattern.  In round r the device decides a vertex if a neighbour of higher
    priority was a root before round r, or if all of them were decided before it.  So, by descending priority:
    round(v) = 0 without such a neighbour; 1 + the smallest round of the roots among them, if there is one; else 1 + the
    largest round among them.  The value reported is 1 + the last round that decided a vertex."""
    n = pattern[0]
    if n == 0:
        return 0
    ptr, nbr = cr.adjacency(pattern)
    prio = ar.priorities(pattern, seed)
    rank = np.empty(n, dtype=np.int64)
    order = np.argsort(prio)[::-1]
    rank[order] = np.arange(n)
    ptr_l, nbr_l, rank_l = ptr.tolist(), nbr.tolist(), rank.tolist()
    rnd, root = [0] * n, [False] * n
    for v in order.tolist():
        higher = [u for u in nbr_l[ptr_l[v]:ptr_l[v + 1]] if rank_l[u] < rank_l[v]]
        roots = [rnd[u] for u in higher if root[u]]
        if not higher:
            root[v] = True
        elif roots:
            rnd[v] = 1 + min(roots)
        else:
            root[v], rnd[v] = True, 1 + max(rnd[u] for u in higher)
    return 1 + max(rnd)


def level_rounds(level, seed):
    """expected_rounds of an amg_ref.Level that has a coarser one, computed once per level object"""
    if getattr(level, "expected_rounds", None) is None:
        level.expected_rounds = expected_rounds(level.pattern, seed)
    return level.expected_rounds


# ---- the graph -------------------------------------------------------------------------------------------------------

def _fits(lengths, room):
    return [x for x in lengths if x <= room]


def _build(seed, rng, n, knob_seed):
    """(rows, cols, vals as float64, what) without the diagonal's values settled: the off-diagonal entries, each once."""
    symmetric = (seed + seed // 12) % 2 == 0
    integers = seed % 3 == 0
    ids = rng.permutation(n).astype(np.int64)
    used = 0
    rows, cols, vals = [], [], []
    what = dict(symmetric=symmetric, integers=integers, hubs=(), path=0, zero_sum=0, isolated=0)

    def take(count):
        nonlocal used
        out = ids[used:used + count]
        used += count
        return out

    def edges(a, b, both, value):
        """the entries (a, b), and (b, a) if `both`; value(size) draws that many off-diagonal values"""
        rows.append(a), cols.append(b), vals.append(value(a.size))
        if both:
            rows.append(b), cols.append(a), vals.append(value(a.size))

    if integers:
        draw = lambda m: np.where(rng.random(m) < 0.1, 1.0, -1.0) * rng.integers(1, 4, m)     # noqa: E731
    else:
        draw = lambda m: -(0.1 + rng.random(m))                                               # noqa: E731

    # the first hub: a star of its own, so its row and its aggregate hold exactly `length` entries / members
    hubs = []
    room = n // 2
    fit = _fits(HUB_LENGTHS, room)
    if fit:
        length = int(rng.choice(fit))
        one_sided = bool(rng.random() < 0.4)
        block = take(length)
        edges(np.full(length - 1, block[0]), block[1:], not one_sided, draw)
        hubs.append((int(block[0]), length, one_sided))
    # a path along descending priority, a component of its own (its inner vertices have degree 2, so the keys order it)
    if seed % 3 == 1:
        fit = _fits(PATH_LENGTHS, n - used - 2)
        if fit:
            length = int(fit[(5 * (seed // 3)) % len(fit)])   # (the default seeds: 24, 57, 10, 8, 25, 58)
            block = take(length)
            block = block[np.argsort(cr.keys(n, knob_seed)[block])[::-1]]
            edges(block[:-1], block[1:], True, draw)
            what["path"] = length
    # integers: a path whose rows sum to zero, a component of its own; once it is one aggregate its sum cancels
    zero_sum = np.empty(0, dtype=np.int64)
    if integers:
        fit = _fits(ZERO_SUM_LENGTHS, (n - used) // 2)
        if fit:
            length = int(fit[(seed // 3) % len(fit)])
            zero_sum = take(length)
            edges(zero_sum[:-1], zero_sum[1:], True, lambda m: np.full(m, -1.0))
            what["zero_sum"] = length
    # isolated vertices
    what["isolated"] = count = int(round(0.05 * n)) if n - used > 8 else 0
    take(count)
    # the main graph on what is left: random edges inside a window, by position in `rest`
    rest = np.sort(ids[used:])
    m = rest.size
    if m >= 2:
        window = WINDOWS[(seed + seed // 12) % 3] or m
        per = int(rng.choice([1, 2, 3]))
        a = np.repeat(np.arange(m, dtype=np.int64), per)
        b = (a + rng.integers(1, min(window, m - 1) + 1, a.size)) % m     # (wraps round: every vertex has an edge)
        key = np.unique(np.minimum(a, b) * m + np.maximum(a, b))
        a, b = rest[key // m], rest[key % m]
        flip = rng.random(a.size) < 0.5                 # one-sided: the stored direction is drawn
        a, b = np.where(flip, b, a), np.where(flip, a, b)
        edges(a, b, symmetric, draw)
        # the second hub sits inside the main graph: its row has `length` entries with the diagonal
        fit = _fits(HUB_LENGTHS, m // 2)
        if fit and rng.random() < 0.7:
            length = int(rng.choice(fit))
            hub = int(rest[int(rng.integers(m))])
            beside = set(np.concatenate([a[b == hub], b[a == hub], [hub]]).tolist())
            stored = len(beside) if symmetric else 1 + int((a == hub).sum())      # entries of the hub's row so far
            leaves = np.array([v for v in rng.permutation(rest).tolist() if v not in beside][:max(length - stored, 0)],
                              dtype=np.int64)
            one_sided = bool(rng.random() < 0.4)
            edges(np.full(leaves.size, hub), leaves, not one_sided, draw)
            hubs.append((hub, length, one_sided))
    what["hubs"] = tuple(hubs)
    rows = np.concatenate(rows) if rows else np.empty(0, dtype=np.int64)
    cols = np.concatenate(cols) if cols else np.empty(0, dtype=np.int64)
    vals = np.concatenate(vals) if vals else np.empty(0)
    # the diagonal: dominant over the row's and the column's entries; exactly the row's sum on the zero-sum path
    weight = np.bincount(rows, weights=np.abs(vals), minlength=n) + np.bincount(cols, weights=np.abs(vals), minlength=n)
    if integers:
        diag = weight + rng.integers(0, 3, n) + (weight == 0)
        diag[zero_sum] = np.bincount(rows, weights=np.abs(vals), minlength=n)[zero_sum]
    else:
        diag = weight * (1.0 + rng.random(n)) + 0.1 + rng.random(n)
    d = np.arange(n, dtype=np.int64)
    return np.concatenate([rows, d]), np.concatenate([cols, d]), np.concatenate([vals, diag]), what


def tail_settings(rng, rows):
    """0, rows[l] - 1 and rows[l] of a drawn level l, the default and the clamp: each once, ascending"""
    l = int(rng.integers(len(rows)))
    return tuple(sorted({0, max(rows[l] - 1, 0), rows[l], TAIL_DEFAULT, TAIL_CLAMP}))


def tail_from_level(rows, tail_rows):
    """the first level of at most min(tail_rows, the clamp) rows; the number of levels if there is none"""
    first = [l for l, n in enumerate(rows) if n <= min(tail_rows, TAIL_CLAMP)]
    return first[0] if first else len(rows)


@functools.lru_cache(maxsize=None)
def case(seed):
    """(pattern, values, b, knobs) of one seed; built once per process, shared, read-only.

    knobs: n, what (the parts of the graph), kind, dtype, params (the keywords of amg_ref.Hierarchy), method, maxit, tol,
    tails (the "amg_tail_rows" settings)."""
    rng = np.random.default_rng(BASE_SEED + seed)
    n = N_TABLE[seed % 12]
    dtype = np.dtype((np.float64, np.float32)[(seed // 2 + seed // 12) % 2])
    params = dict(
        seed=SEEDS[int(rng.integers(len(SEEDS)))],
        max_levels=1 if seed % 24 == 13 else MAX_LEVELS_DEAL.get(seed % 12, 16),
        coarse_rows=10**9 if seed % 12 in SINGLE_LEVEL else COARSE_ROWS[(seed + seed // 12) % 3],
        nu=NU[int(rng.integers(len(NU)))],
        coarse_sweeps=COARSE_SWEEPS[int(rng.integers(len(COARSE_SWEEPS)))],
        gamma=1 + (seed // 2 + seed // 8) % 2,
        omega=OMEGA[int(rng.integers(len(OMEGA)))],
        alpha=ALPHA[int(rng.integers(len(ALPHA)))])
    if seed % 8 == 5:                                   # the W-cycle's bookkeeping with nothing between two visits
        params.update(nu=1, coarse_sweeps=1, gamma=2)
    rows, cols, vals, what = _build(seed, rng, n, params["seed"])
    pattern, values = ar.from_triplets(n, rows, cols, vals, dtype)
    b = rng.standard_normal(n).astype(dtype)
    knobs = dict(n=n, what=what, kind=("csr", "csc")[int(rng.integers(2))], dtype=dtype, params=params,
                 method=METHODS[int(rng.integers(2))], maxit=MAXIT[(seed + seed // 3) % 3], tol=TOL[dtype])
    for a in (*pattern[1:], values, b):
        a.setflags(write=False)
    knobs["tails"] = tail_settings(rng, reference(seed, pattern, values, params).rows)
    return pattern, values, b, knobs


_REFERENCES = {}


def reference(seed, pattern=None, values=None, params=None):
    """amg_ref.Hierarchy of case(seed), built once per process and shared (treat it as read-only)"""
    if seed not in _REFERENCES:
        if pattern is None:
            case(seed)
        else:
            _REFERENCES[seed] = ar.Hierarchy(pattern, values, **params)
    return _REFERENCES[seed]
