"""Seeded random inputs for the multicolour ordering -- colour, permute, multicolour -- and for the solve path it was
built for: ILU(0) exactly and by row sweeps, the triangular solves by sweeps, CG / BiCGStab / GMRES on the permuted
system (test infrastructure, plain numpy, no GPU).

The hand-made structures of tests/colour_ref.py isolate one boundary each.  `case(seed)` takes the matrix of
tests/solver_cases.py (n <= 8000, planted rows of thousands of entries, fan and bare stretches, three placements, now
and then a missing diagonal) and plants, from dealt tables:

* a dense random block on the odd seeds: m vertices spread over the rows, every pair an edge with the dealt density,
  every edge stored in ONE direction chosen at random, so that half of every neighbourhood is visible through A^T only.
  Such a block needs more than 64 colours (m = 400 at density 0.9: more than 128) and, unlike a clique, leaves holes
  in the 64-colour windows: a vertex takes colour c >= 64 while a neighbour visited before it holds a larger colour of
  the same window;
* runs of empty rows on the seeds of EMPTY: rows AND columns cleared, the diagonal too, at the front, at the back and
  in the middle -- what the bisection of permute's gather has to skip.  On one seed (n = 2) nothing is left: nnz = 0.

The rows solver_cases leaves without a diagonal stay without one.  A seed with a row without a diagonal is coloured and
permuted like any other; ILU(0) and the solves must refuse it by the name of its first such row.

The knobs dealt with the matrix: the colouring seed (0, 7, 2^32 - 1, 2^32 + 7 -- which must colour as 7 does -- and a
drawn 64-bit value), a second one, kind and dtype (solver_cases' draw), one more permutation (identity, reversal,
random, or a rotation that moves the empty runs), the Krylov method (cg on the seeds that are still symmetric positive
definite), maxit, the stream (None or the caller's), the handle's origin (uploaded, or assembled on the device from
shuffled triplets), which ordering call is the handle's first, and on two seeds an operand that is itself a device
result (a + a, a @ a).  `chain(rounds)` is colour_ref.key_chain at the round counts where a batch of rounds between two
polls ends (8, 24, 56, 120) and one past them.  tests/test_ordering_cases_host.py holds the default seeds to the
conditions the device test relies on.
"""
import functools

import numpy as np

from . import colour_ref as cr
from . import krylov_ref as kr
from . import solver_cases as sc
from . import trsv_ref as tr

DEFAULT_SEEDS = 24
BASE_SEED = 20261900

BLOCK_M = (400, 160, 260, 70)                        # by (seed // 2) % 4, on the odd seeds with n >= BLOCK_MIN_N
BLOCK_DENSITY = (0.7, 0.9, 0.5)                      # by (seed // 2) % 3: all twelve pairs in 24 seeds
BLOCK_MIN_N = 255
# seed % 24 -> where the runs of empty rows sit (the seeds on which solver_cases drops a diagonal anyway)
EMPTY = {5: ("front", "middle"), 11: ("back",), 17: ("front", "middle", "back"), 23: ("front", "back")}
RUN_LENGTHS = (1, 2, 70, 300)                        # drawn per run, cut to a quarter of n (at least one row)
CSEEDS = (0, 7, 2**32 - 1, 2**32 + 7, None)          # None: a drawn value in [2^32, 2^64)
PERM_KINDS = ("reversal", "rotation", "random", "identity")      # by (seed + seed // 4) % 4
METHODS = ("cg", "bicgstab", "gmres")
MAXIT = (1, 4, 7)
STREAMS = (None, "caller")
ORIGINS = ("assembled", "uploaded")
FIRST_CALLS = ("colour", "multicolour", "permute")
OPERANDS = {7: "spgemm", 14: "spadd"}                # seed % 24 -> the operand is a @ a (n = 255) / a + a (n = 5000)
GMRES_RESTART = 3
CHAIN_ROUNDS = (8, 9, 24, 25, 56, 57, 120, 121)      # the ends of the first four batches of rounds, and one past them


def chain(rounds):
    """A path whose keys (seed 0) descend along it: `rounds` rounds, 2 colours."""
    return cr.key_chain(rounds)


def batch_of(rounds):
    """The index of the batch (8, 16, 32, ... rounds between two polls) in which round number `rounds` falls."""
    b, end = 0, 8
    while rounds > end:
        b, end = b + 1, end + (8 << (b + 1))
    return b


def _coo(pattern):
    n, rowptr, colind = pattern
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64))), colind.astype(np.int64)


def _block(rng, n, m, density):
    """(rows, cols, members): every pair of the m members with probability `density`, stored in one direction."""
    members = np.sort(rng.choice(n, size=m, replace=False))
    i, j = np.triu_indices(m, 1)
    keep = rng.random(i.size) < density
    i, j = members[i[keep]], members[j[keep]]
    flip = rng.random(i.size) < 0.5
    return np.where(flip, j, i), np.where(flip, i, j), members


def _empty_runs(rng, n, places):
    """[(place, first, end)]: disjoint runs inside their third of the rows (the front run starts at row 0, the back run
    ends at row n)."""
    runs = []
    for place in places:
        ln = max(1, min(int(rng.choice(RUN_LENGTHS)), n // 4))
        if place == "front":
            a = 0
        elif place == "back":
            a = n - ln
        else:
            a = int(rng.integers(n // 3, max(n // 3 + 1, 2 * n // 3 - ln)))
        runs.append((place, a, a + ln))
    return runs


def _permutation(rng, n, kind, runs):
    i = np.arange(n, dtype=np.uint64)
    if kind == "identity":
        return i
    if kind == "reversal":
        return i[::-1].copy()
    if kind == "random":
        return rng.permutation(n).astype(np.uint64)
    # rotation: new row i' is old row (i' + shift) mod n; the shift takes a front run into the middle and splits or
    # moves the others
    shift = (n - n // 2 - (runs[0][2] - runs[0][1]) // 2) % n if runs else n // 3
    return np.roll(i, -int(shift)).copy()


@functools.lru_cache(maxsize=None)
def case(seed):
    """(pattern, values, b, x0, knobs) of one seed; built once per process, shared, read-only.

    knobs: n, dtype, kind, block = (m, density, members) or None, empty_runs = [(place, first, end)], dropped (the rows
    without a stored diagonal, ascending), symmetric, cseed, cseed2, perm_kind, perm, method, maxit, tol, stream, origin,
    first_call, operand ("plain" / "spadd" / "spgemm"), special (the dealt permutation moves the special values)."""
    rng = np.random.default_rng(BASE_SEED + seed)
    base, _, _, _, k0 = sc.case(seed)
    n = base[0]
    rows, cols = _coo(base)
    s24 = seed % 24

    block = None
    if seed % 2 == 1 and n >= BLOCK_MIN_N:
        m, density = BLOCK_M[(seed // 2) % len(BLOCK_M)], BLOCK_DENSITY[(seed // 2) % len(BLOCK_DENSITY)]
        br, bc, members = _block(rng, n, m, density)
        rows, cols = np.concatenate([rows, br]), np.concatenate([cols, bc])
        members.setflags(write=False)
        block = (m, density, members)
    runs = _empty_runs(rng, n, EMPTY.get(s24, ()))
    if runs:
        cleared = np.zeros(n, dtype=bool)
        for _, a, e in runs:
            cleared[a:e] = True
        keep = ~cleared[rows] & ~cleared[cols]
        rows, cols = rows[keep], cols[keep]
    pattern = tr.from_coo(n, rows, cols)
    stored = np.zeros(n, dtype=bool)
    stored[rows[rows == cols]] = True
    dropped = tuple(np.flatnonzero(~stored).tolist())

    symmetric = k0["method"] == "cg" and block is None       # solver_cases made it symmetric and nothing here undid that
    dtype = k0["dtype"]
    values, b = (kr.spd_fill if symmetric else tr.fill)(pattern, dtype, rng)
    x0 = rng.uniform(-1, 1, size=n).astype(dtype)

    drawn = [int(rng.integers(2**32, 2**64, dtype=np.uint64)) for _ in range(2)]
    cseed, cseed2 = CSEEDS[seed % len(CSEEDS)], CSEEDS[(seed + 2) % len(CSEEDS)]
    cseed, cseed2 = (drawn[0] if cseed is None else cseed), (drawn[1] if cseed2 is None else cseed2)
    perm_kind = PERM_KINDS[(seed + seed // 4) % len(PERM_KINDS)]
    perm = _permutation(rng, n, perm_kind, runs)
    method = METHODS[seed % 3]
    if method == "cg" and not symmetric:
        method = METHODS[1 + (seed // 3) % 2]
    knobs = dict(
        n=n, dtype=dtype, kind=k0["kind"], block=block, empty_runs=runs, dropped=dropped, symmetric=symmetric,
        cseed=cseed, cseed2=cseed2, perm_kind=perm_kind, perm=perm, method=method,
        maxit=MAXIT[(seed + seed // 3) % len(MAXIT)], tol=sc.TOL[dtype], stream=STREAMS[(seed // 2) % 2],
        origin=ORIGINS[(seed // 3) % 2], first_call=FIRST_CALLS[(seed // 6) % 3], operand=OPERANDS.get(s24, "plain"),
        special=seed % 4 == 2)
    for a in (*pattern[1:], values, b, x0, perm):
        a.setflags(write=False)
    return pattern, values, b, x0, knobs


@functools.lru_cache(maxsize=None)
def reference(seed):
    """colour_ref.greedy of the seed's pattern at its colouring seed, computed once per process (read-only)."""
    pattern, _, _, _, k = case(seed)
    colours, ncolours, rounds = cr.greedy(pattern, k["cseed"])
    colours.setflags(write=False)
    return colours, ncolours, rounds


def holes(pattern, colours, cseed):
    """How many vertices take a colour c >= 64 while a neighbour visited before them (a higher key) holds a colour in
    (c, 64 * (c // 64) + 64): the window's mask is no prefix there."""
    ptr, nbr = cr.adjacency(pattern)
    key = cr.keys(pattern[0], cseed)
    src = np.repeat(np.arange(pattern[0], dtype=np.int64), np.diff(ptr))
    c, cn = colours.astype(np.int64)[src], colours.astype(np.int64)[nbr]
    hit = (c >= 64) & (key[nbr] > key[src]) & (cn > c) & (cn < 64 * (c // 64) + 64)
    return int(np.unique(src[hit]).size)


def csr_view(kind, n, ptr, ind, val):
    """((n, rowptr, colind), values by rows) of a handle's downloaded arrays."""
    ptr, ind = np.asarray(ptr, dtype=np.uint64), np.asarray(ind, dtype=np.uint64)
    if kind == "csr":
        return (n, ptr, ind), np.asarray(val)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr.astype(np.int64)))
    order = np.lexsort((cols, ind.astype(np.int64)))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ind.astype(np.int64), minlength=n))]).astype(np.uint64)
    return (n, rowptr, cols[order].astype(np.uint64)), np.asarray(val)[order]
