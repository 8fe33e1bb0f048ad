"""CPU restatement of the multicolour ordering (include/spal.h) and the matrices its tests use.

Graph: the vertices are the rows of a square A; i ~ j iff i != j and (i, j) or (j, i) is stored.  Priority:
key(i) = mix32((i + seed) mod 2^32).  `greedy` is THE definition: vertices by descending key, each takes the smallest
colour no neighbour visited before it has.  `perm_from_colours` lists the rows by (colour, row): new -> old.  `permute`
is B = P A P^T with B[i'][j'] = A[perm[i']][perm[j']], columns ascending, values moved.
"""
import numpy as np

from . import ilu_ref as ir
from . import trsv_ref as tr

sym, fan = ir.sym, ir.fan
SEEDS = (0, 7, 2**32 - 1)
MIX32_CHECK = {0: 0, 1: 1753845952, 2: 3507691905, 3: 1408362973}


def mix32(x):
    """The hash of the text on a uint32 array (or one value), in 32-bit arithmetic."""
    x = np.atleast_1d(np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF))
    m = np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    x = x ^ (x >> np.uint64(16))
    return x


def keys(n, seed):
    return mix32((np.arange(n, dtype=np.uint64) + np.uint64(seed)) & np.uint64(0xFFFFFFFF))


def adjacency(pattern):
    """(ptr, nbr) of the symmetrised graph without loops, neighbours ascending, each once."""
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    cols = colind.astype(np.int64)
    off = rows != cols
    r, c = np.concatenate([rows[off], cols[off]]), np.concatenate([cols[off], rows[off]])
    key = np.unique(r * n + c)
    r, c = key // n, key % n
    ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    return ptr, c


def greedy(pattern, seed=0):
    """(colour as uint64, ncolours, rounds): rounds = the longest path of descending keys counted in vertices, which
    is the number of Jones-Plassmann rounds (a vertex is coloured one round after the last of its higher-key
    neighbours)."""
    n = pattern[0]
    ptr, nbr = adjacency(pattern)
    k = keys(n, seed)
    colour = np.full(n, -1, dtype=np.int64)
    depth = np.zeros(n, dtype=np.int64)
    for v in np.argsort(k)[::-1].tolist():
        nb = nbr[ptr[v]:ptr[v + 1]]
        seen = nb[colour[nb] >= 0]                 # visited before v: exactly the neighbours with a higher key
        assert np.all(k[seen] > k[v])
        cs = colour[seen]
        used = np.zeros(cs.size + 1, dtype=bool)   # a colour never exceeds the count of visited neighbours
        used[cs[cs <= cs.size]] = True
        colour[v] = int(np.argmin(used))
        depth[v] = (int(depth[seen].max()) if seen.size else 0) + 1
    return colour.astype(np.uint64), (int(colour.max()) + 1 if n else 0), (int(depth.max()) if n else 0)


def perm_from_colours(colour):
    return np.argsort(np.asarray(colour, dtype=np.int64), kind="stable").astype(np.uint64)


def permute(pattern, values, perm):
    """((n, rowptr, colind), values) of P A P^T."""
    n, rowptr, colind = pattern
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    nr, nc = inv[rows], inv[colind.astype(np.int64)]
    order = np.lexsort((nc, nr))
    newptr = np.concatenate([[0], np.cumsum(np.bincount(nr, minlength=n))]).astype(np.uint64)
    return (n, newptr, nc[order].astype(np.uint64)), np.asarray(values)[order]


def is_proper(pattern, colour):
    ptr, nbr = adjacency(pattern)
    src = np.repeat(np.arange(pattern[0], dtype=np.int64), np.diff(ptr))
    return bool(np.all(colour[src] != colour[nbr]))


def max_degree(pattern):
    ptr, _ = adjacency(pattern)
    return int(np.diff(ptr).max()) if pattern[0] else 0


def key_chain(n, seed=0):
    """The worst case for the rounds: a path through all vertices in descending-key order, every edge stored in one
    direction only (alternating), no diagonal.  n rounds, 2 colours."""
    order = np.argsort(keys(n, seed))[::-1].astype(np.int64)
    a, b = order[:-1].copy(), order[1:].copy()
    flip = np.arange(n - 1) % 2 == 1
    a[flip], b[flip] = order[1:][flip], order[:-1][flip]
    return tr.from_coo(n, a, b)


# the hand example: 0 - 1, 0 - 2, 1 - 2, 2 - 3, 3 - 4, with (1, 0), (3, 2) and (4, 3) stored in one direction only.
# Keys at seed 0: key(4) > key(2) > key(1) > key(3) > key(0) = 0.  Visit 4: colour 0; 2: 0; 1 (sees 2): 1;
# 3 (sees 2 and 4, both 0): 1; 0 (sees 1 and 2: colours 1 and 0): 2.  Longest descending path 2 -> 1 -> 0: 3 rounds.
HAND = tr.from_coo(5, [0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4], [0, 2, 0, 2, 0, 1, 2, 2, 3, 3, 4])
HAND_COLOURS = [2, 1, 0, 1, 0]
HAND_PERM = [2, 4, 1, 3, 0]
HAND_ROUNDS = 3


def patterns():
    """name -> pattern: what the host and the device tests colour, with every seed of SEEDS."""
    rng = np.random.default_rng(1811)
    return {
        "hand": HAND,
        "diagonal_1": tr.diagonal(1),
        "diagonal_50": tr.diagonal(50),
        "sym_bidiagonal": sym(tr.bidiagonal(5000)),
        "bidiagonal": tr.bidiagonal(5000),          # edges seen from one side through A^T only
        "full": tr.full(4000, 6, rng),
        "sym_banded": sym(tr.banded(6007, 6, 512, rng)),
        "sym_prescribed": sym(tr.prescribed(tr.PRESCRIBED_WIDTHS, rng)),
        "dense_64": tr.dense_triangle(64),          # 64, 65, 130 colours: the boundaries of the 64-colour windows
        "dense_65": tr.dense_triangle(65),
        "dense_130": tr.dense_triangle(130),
        "arrow": tr.arrow(3000),
        "fan": fan(1281),
    }


_CACHE = {}


def reference(name, seed):
    """greedy() of a named pattern, computed once per session and shared (treat the arrays as read-only)."""
    if (name, seed) not in _CACHE:
        _CACHE[(name, seed)] = greedy(patterns_cached()[name], seed)
    return _CACHE[(name, seed)]


def patterns_cached():
    if "patterns" not in _CACHE:
        _CACHE["patterns"] = patterns()
    return _CACHE["patterns"]
