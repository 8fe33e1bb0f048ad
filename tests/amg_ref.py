"""CPU restatement of the aggregation AMG (include/spal.h) and the matrices its tests use.

`aggregate` is THE aggregation text: degrees of the symmetrised graph, prio = deg << 32 | mix32(i + seed), vertices by
descending priority, a vertex a root iff no neighbour is one already, every other vertex joined to its neighbouring root
of highest priority, roots numbered by ascending row.  `coarse` sends the triplets (agg[i], agg[j], v) in storage order
through the oracle's COO -> CSR text.  `Hierarchy` builds the levels by the four rules and `cycle` is the cycle; the
sequential sums are vectorised ACROSS rows, entry rank by entry rank, which keeps each row's order.  `solve` runs the two
loops of tests/krylov_ref.py with cycle(0, .) as M^-1.
"""
import numpy as np

from . import colour_ref as cr
from . import krylov_ref as kr

DEFAULTS = dict(seed=0, max_levels=16, coarse_rows=64, nu=2, coarse_sweeps=16, gamma=1, omega=2.0 / 3.0, alpha=1.0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def priorities(pattern, seed=0):
    ptr, _ = cr.adjacency(pattern)
    deg = np.minimum(np.diff(ptr), 2**31 - 1).astype(np.uint64)
    return (deg << np.uint64(32)) | cr.keys(pattern[0], seed)


def aggregate(pattern, seed=0):
    """(agg as uint64, nagg)"""
    n = pattern[0]
    if n == 0:
        return np.zeros(0, dtype=np.uint64), 0
    ptr, nbr = cr.adjacency(pattern)
    prio = priorities(pattern, seed)
    root = np.zeros(n, dtype=bool)
    for v in np.argsort(prio)[::-1].tolist():
        root[v] = not root[nbr[ptr[v]:ptr[v + 1]]].any()
    number = np.cumsum(root) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    keep = root[nbr] & ~root[src]
    s, c = src[keep], nbr[keep]
    order = np.lexsort((prio[c], s))                   # by vertex, then by the neighbouring root's priority
    s, c = s[order], c[order]
    last = np.ones(s.size, dtype=bool)
    last[:-1] = s[1:] != s[:-1]
    rootof = np.arange(n, dtype=np.int64)
    rootof[s[last]] = c[last]
    assert np.all(root[rootof])                        # maximal: every vertex has a root beside it
    return number[rootof].astype(np.uint64), int(root.sum())


def _rows(pattern):
    n, rowptr, _ = pattern
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))


def coarse(pattern, values, agg, nagg):
    """((nagg, rowptr, colind), values) of A_{l+1}"""
    import oracle
    a = agg.astype(np.int64)
    p, i, v = oracle.coo_to_csr(nagg, nagg, a[_rows(pattern)].astype(np.uint64),
                                a[pattern[2].astype(np.int64)].astype(np.uint64), values)
    return (nagg, p, i), v


def diagonal_positions(pattern):
    """position of the stored (i, i) of every row, -1 where there is none"""
    n, rowptr, colind = pattern
    pos = np.full(n, -1, dtype=np.int64)
    rows = _rows(pattern)
    hit = np.nonzero(rows == colind.astype(np.int64))[0]
    pos[rows[hit]] = hit
    return pos


class _Ranked:
    """acc[i] = +0.0 + t[ptr[i]] + t[ptr[i] + 1] + ... in order, for all i at once: one vector add per entry rank."""

    def __init__(self, ptr):
        ptr = np.asarray(ptr, dtype=np.int64)
        self.n = ptr.size - 1
        self.start = ptr[:-1]
        length = np.diff(ptr)
        self.by_length = np.argsort(-length, kind="stable")
        self.alive = [int(np.count_nonzero(length > k)) for k in range(int(length.max()) if self.n else 0)]

    def sum(self, term, dtype):
        acc = np.zeros(self.n, dtype=dtype)
        for k, m in enumerate(self.alive):
            rows = self.by_length[:m]
            acc[rows] = acc[rows] + term(self.start[rows] + k)
        return acc


class Level:
    def __init__(self, pattern, values, omega):
        self.pattern, self.values = pattern, values
        self.n = pattern[0]
        self.ind = pattern[2].astype(np.int64)
        self.ranked = _Ranked(pattern[1])
        self.dpos = diagonal_positions(pattern)
        self.agg = self.nagg = self.members = None
        dt = values.dtype.type
        with np.errstate(all="ignore"):
            self.w = (dt(omega) / values[self.dpos]) if self.n and np.all(self.dpos >= 0) else None

    def rowsum(self, x):
        return self.ranked.sum(lambda q: self.values[q] * x[self.ind[q]], self.values.dtype)

    def set_aggregates(self, agg, nagg):
        self.agg, self.nagg = agg.astype(np.int64), nagg
        self.mem = np.argsort(self.agg, kind="stable")
        mptr = np.concatenate([[0], np.cumsum(np.bincount(self.agg, minlength=nagg))])
        self.members = _Ranked(mptr)

    def restrict(self, r):
        return self.members.sum(lambda q: r[self.mem[q]], r.dtype)


class Hierarchy:
    def __init__(self, pattern, values, **kw):
        self.p = p = params(**kw)
        self.levels = [Level(pattern, np.asarray(values), p["omega"])]
        assert self.levels[0].w is not None, "a level-0 row stores no diagonal"
        while True:
            lv = self.levels[-1]
            if not lv.n > p["coarse_rows"]:
                self.stopped_by = "coarse_rows"
                break
            if not len(self.levels) < p["max_levels"]:
                self.stopped_by = "max_levels"
                break
            agg, nagg = aggregate(lv.pattern, p["seed"])
            if not nagg < lv.n:
                self.stopped_by = "no_coarsening"
                break
            nxt = Level(*coarse(lv.pattern, lv.values, agg, nagg), p["omega"])
            if nxt.w is None:
                self.stopped_by = "diagonal"
                break
            lv.set_aggregates(agg, nagg)
            self.levels.append(nxt)

    @property
    def rows(self):
        return [lv.n for lv in self.levels]

    def cycle(self, b, l=0):
        p, lv = self.p, self.levels[l]
        dt = b.dtype.type
        last = l == len(self.levels) - 1
        with np.errstate(all="ignore"):
            x = lv.w * b
            smooth = lambda x: x + (lv.w * (b - lv.rowsum(x)))     # noqa: E731
            for _ in range((p["coarse_sweeps"] if last else p["nu"]) - 1):
                x = smooth(x)
            if last:
                return x
            for _ in range(p["gamma"]):
                r = b - lv.rowsum(x)
                e = self.cycle(lv.restrict(r), l + 1)
                x = x + (dt(p["alpha"]) * e[lv.agg])
            for _ in range(p["nu"]):
                x = smooth(x)
            return x


def solve(h, mul, b, method, tol, maxit, x0=None):
    """The loop of tests/krylov_ref.py with M^-1 v = cycle(0, v); `mul` is the product (h is None: no preconditioner)."""
    x0 = np.zeros_like(b) if x0 is None else x0
    return kr.METHODS[method](mul, None if h is None else (lambda v: h.cycle(v)), b, x0, tol, maxit)


# ---- matrices ---------------------------------------------------------------------------------------------------------
def from_triplets(n, rows, cols, vals, dtype=np.float64):
    """((n, rowptr, colind), values): entries ordered by (row, col); the triplets hold no duplicates"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.lexsort((cols, rows))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.uint64)
    assert np.unique(rows * n + cols).size == rows.size
    return (n, rowptr, cols[order].astype(np.uint64)), np.asarray(vals, dtype=dtype)[order]


def stencil(shape, dtype=np.float64):
    """The 5-point (2-D) or 7-point (3-D) Laplacian on a grid of `shape`, Dirichlet: diagonal 2 * dims, neighbours -1."""
    idx = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(idx.size, 2.0 * len(shape))]
    for ax in range(len(shape)):
        lo = np.take(idx, np.arange(shape[ax] - 1), axis=ax).ravel()
        hi = np.take(idx, np.arange(1, shape[ax]), axis=ax).ravel()
        rows += [lo, hi]
        cols += [hi, lo]
        vals += [np.full(lo.size, -1.0)] * 2
    return from_triplets(idx.size, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), dtype)


def path(n, dtype=np.float64):
    return stencil((n,), dtype)


def star(n, two_sided, dtype=np.float64):
    """vertex 0 beside every other: row 0 holds (0, j); rows j hold (j, 0) only when two_sided.  Diagonal n (dominant)."""
    j = np.arange(1, n, dtype=np.int64)
    d = np.arange(n, dtype=np.int64)
    rows, cols, vals = [d, np.zeros(n - 1, dtype=np.int64)], [d, j], [np.full(n, float(n)), np.full(n - 1, -1.0)]
    if two_sided:
        rows, cols, vals = rows + [j], cols + [np.zeros(n - 1, dtype=np.int64)], vals + [np.full(n - 1, -1.0)]
    return from_triplets(n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), dtype)


HUB_LENGTHS = (31, 32, 33, 34, 63, 64, 65, 66, 127, 128, 129, 130, 200)


def hubs(lengths=HUB_LENGTHS, dtype=np.float64):
    """Hub k (vertex k) is beside lengths[k] - 1 leaves of its own, stored both ways, so that with its diagonal its row
    holds lengths[k] entries and its aggregate as many members: rows and aggregates on both sides of 32 entries (where a
    wave takes a row over from its thread) and of whole steps of 64.  The leaves of one hub form a path, so the coarse
    levels keep some structure.  The values differ from entry to entry: an order of additions shows."""
    n = len(lengths) + sum(lengths) - len(lengths)
    d = np.arange(n, dtype=np.int64)
    rows, cols, first = [d], [d], len(lengths)
    for k, length in enumerate(lengths):
        leaves = first + np.arange(length - 1, dtype=np.int64)
        first += length - 1
        hub = np.full(leaves.size, k, dtype=np.int64)
        rows += [hub, leaves, leaves[:-1], leaves[1:]]
        cols += [leaves, hub, leaves[1:], leaves[:-1]]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = np.where(rows == cols, 300.0 + rows % 5, -1.0 / (1.0 + (3 * rows + 7 * cols) % 11))
    return from_triplets(n, rows, cols, vals, dtype)


def diagonal(n, dtype=np.float64):
    d = np.arange(n, dtype=np.int64)
    return from_triplets(n, d, d, 1.0 + d % 7, dtype)


def descending_path(n, seed=0, dtype=np.float64):
    """A path through all vertices in descending-priority order: every inner vertex has degree 2, so the order is the
    keys', and the roots are decided one round after the other along it."""
    order = np.argsort(cr.keys(n, seed))[::-1].astype(np.int64)
    a, b = order[:-1], order[1:]
    d = np.arange(n, dtype=np.int64)
    return from_triplets(n, np.concatenate([d, a, b]), np.concatenate([d, b, a]),
                         np.concatenate([np.full(n, 2.0), np.full(2 * (n - 1), -1.0)]), dtype)


def cancelling(dtype=np.float64):
    """The path of 8 (aggregates [0,1,1,2,2,2,3,3] at seed 0) with values chosen so that the coarse (1, 1) entry
    -- the sum of (1,1), (1,2), (2,1), (2,2) -- is exactly zero and dropped: the "diagonal" rule stops the build."""
    pattern, values = path(8, dtype)
    values = values.copy()
    n, rowptr, colind = pattern
    rows = _rows(pattern)
    for (i, j), v in {(1, 1): 1.0, (1, 2): -1.0, (2, 1): -1.0, (2, 2): 1.0}.items():
        values[np.nonzero((rows == i) & (colind.astype(np.int64) == j))[0][0]] = v
    return pattern, values
