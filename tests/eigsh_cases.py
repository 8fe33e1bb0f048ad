"""Directed and seeded random inputs for eigsh (test infrastructure, plain numpy, no GPU).

The directed builders construct what the hand-made cases of tests/test_gpu_eigsh.py cannot reach:
  `exhaustion(L)`   a weighted path whose Lanczos vectors from v0 = e0 are unit vectors, so all arithmetic is exact and
                    hn == 0 falls at step L - 1, anywhere in a phase and on either side of the basis batch of 8;
  `overflow(p)`     the same path with one coupling of 2^600 (2^100 in f32): dot(w, w) overflows at step p, so stop 2
                    is decided in the middle of a phase, or after restarts;
  ROTATION_TILES    ncv of 2 to 4 on n of 1025 to 2050: LDS rotation tiles of 512 and 1024 rows, two or three of them,
                    the last one partial (`rot_tile_rows` restates the kernel's choice);
  MANY_TILES        n = 8192 * 64 + 1 with tiles of 64 rows: one tile more than the rotation's grid has workgroups;
  FULL_BASIS        ncv == n.
Exhaustion AFTER a restart is not reachable: the rotated basis is no longer exact, so hn == 0 cannot be constructed there.

`case(seed)` is the fuzz: a symmetric matrix from the banded and the random patterns of the solver tests, its values
from five classes (SPD, indefinite, scaled down, scaled up, clustered), and the arguments of the call.
tests/test_eigsh_cases_host.py asserts the text's behaviour on the directed cases and what the default seeds reach.
"""
import functools

import numpy as np

from . import eigsh_ref as er
from . import ilu_ref as ir
from . import krylov_ref as kr
from . import trsv_ref as tr

DEFAULT_SEEDS = 24
BASE_SEED = 20262000

N_TABLE = (2, 3, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4099, 20_000)
NCV_TABLE = (2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 100)
CLASSES = ("spd", "indefinite", "scaled_down", "scaled_up", "clustered")
SCALE = {("scaled_down", 8): 1e-20, ("scaled_up", 8): 1e+20, ("scaled_down", 4): 1e-12, ("scaled_up", 4): 1e+12}
MAXIT = (0, 1, 2, 3)
SEEDS = (0, 7, 2**32 + 5, 2**40 + 123)
SMALL = 300                                          # up to here the host test compares with numpy.linalg.eigvalsh
SMALL_MAXIT = 300
LIB_JACOBI_FROM = 25                                 # ncv from which the reference takes the library's Jacobi routine

ROT_MIN_ROWS, ROT_MAX_ROWS, ROT_LDS_TARGET, ROT_MAX_GRID = 64, 1024, 16 * 1024, 8192


def rot_tile_rows(m, itemsize, target=ROT_LDS_TARGET):
    """rows of an LDS rotation tile for m basis vectors: doubled from 64 while two tiles stay within the target, to 1024"""
    r = ROT_MIN_ROWS
    while r < ROT_MAX_ROWS and 2 * r * m * itemsize <= target:
        r *= 2
    return r


TOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-5}      # the tolerances of tests/test_gpu_eigsh.py


def default_tol(dtype):
    """what the library takes for tol = 0: the machine epsilon"""
    return float(np.finfo(dtype).eps)


def readonly(mat):
    for a in mat[1:]:
        a.setflags(write=False)
    return mat


def host_mul(mat):
    """v -> A v on the host: the products in float64, summed by numpy, rounded to the values' dtype.  A stand-in for the
    device's spmv where the text runs alone on the CPU."""
    n, rowptr, colind, values = mat
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    cols, v64 = colind.astype(np.int64), values.astype(np.float64)

    def mul(x):
        with np.errstate(all="ignore"):
            return np.bincount(rows, weights=v64 * x.astype(np.float64)[cols], minlength=n).astype(values.dtype)
    return mul


def dense(mat):
    n, rowptr, colind, values = mat
    a = np.zeros((n, n))
    a[np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64))), colind.astype(np.int64)] = values
    return a


def e0(n, dtype):
    v = np.zeros(n, dtype=dtype)
    v[0] = 1.0
    return v


# ---- the directed cases ----------------------------------------------------------------------------------------------

def _tridiagonal(diag, off, dtype):
    """(n, rowptr, colind, values) of the symmetric tridiagonal matrix; an off-diagonal of 0.0 is not stored"""
    n = diag.size
    i = np.flatnonzero(off != 0)
    d = np.arange(n, dtype=np.int64)
    rows, cols = np.concatenate([d, i, i + 1]), np.concatenate([d, i + 1, i])
    vals = np.concatenate([diag, off[i], off[i]])
    order = np.lexsort((cols, rows))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.uint64)
    return readonly((n, rowptr, cols[order].astype(np.uint64), vals[order].astype(dtype)))


EXHAUSTION_L = (2, 7, 8, 9, 16, 17)
EXHAUSTION_N, EXHAUSTION_NCV = 40, 20


@functools.lru_cache(maxsize=None)
def exhaustion(L, dtype, n=EXHAUSTION_N):
    """The weighted path: 2.0 between the nodes 0 .. L - 1, diagonal (i % 5) + 1, 0.25 between the nodes from L on and
    nothing between L - 1 and L.  From v0 = e0 the Krylov space is span(e_0 .. e_{L-1})."""
    i = np.arange(n - 1)
    off = np.where(i < L - 1, 2.0, np.where(i >= L, 0.25, 0.0))
    return _tridiagonal((np.arange(n) % 5 + 1).astype(np.float64), off, dtype)


OVERFLOW_P = (0, 3, 7, 8, 9, 15, 16)                 # with ncv = 20: reason 2 after p + 1 products, no restart
OVERFLOW_RESTARTED = dict(p=9, ncv=6, products=10, restarts=2)
OVERFLOW_N, OVERFLOW_NCV, OVERFLOW_K = 40, 20, 2


@functools.lru_cache(maxsize=None)
def overflow(p, dtype, n=OVERFLOW_N):
    """The path with 2.0 throughout and diagonal (i % 5) + 1, but (p, p + 1) and (p + 1, p) are 2^600 (2^100 in f32):
    finite, and its square is not."""
    off = np.full(n - 1, 2.0)
    off[p] = 2.0 ** (600 if np.dtype(dtype) == np.float64 else 100)
    return _tridiagonal((np.arange(n) % 5 + 1).astype(np.float64), off, dtype)


@functools.lru_cache(maxsize=None)
def banded(n, dtype):
    """a small banded SPD matrix, as tests/test_gpu_eigsh.py's"""
    rng = np.random.default_rng(BASE_SEED + n)
    pattern = ir.sym(tr.banded(n, 3, min(12, max(n - 1, 1)), rng))
    values, _ = kr.spd_fill(pattern, dtype, rng)
    return readonly((*pattern, values))


ROTATION_TILES = [(n, ncv) for n in (1025, 2049, 2050) for ncv in (2, 3, 4)]            # k = 1, maxit = 2
# With ncv = 17 a tile has 64 rows in f64 and 128 in f32; ncv = 33 gives f32 its tile of 64 rows, so both dtypes walk a
# second tile: tile 8192 goes to workgroup 0.
MANY_TILES = dict(n=ROT_MAX_GRID * 64 + 1, ncv=17, ncv_f32=33, k=1, maxit=1)
FULL_BASIS = [(n, k) for n in (2, 9, 64, 256) for k in sorted({1, n - 1})]             # ncv = n


@functools.lru_cache(maxsize=None)
def laplacian_plus(n, dtype):
    """the 1-D Laplacian plus a slowly varying diagonal: a long tridiagonal matrix whose values differ from row to row"""
    return _tridiagonal(2.0 + (np.arange(n) % 1000) / 1000.0, np.full(n - 1, -1.0), dtype)


# ---- the fuzz --------------------------------------------------------------------------------------------------------

def _pattern(rng, n, seed):
    if seed % 2 == 0 or n < 4:
        return ir.sym(tr.banded(n, int(rng.choice([1, 2, 3])), min(int(rng.choice([1, 12, 600])), max(n - 1, 1)), rng))
    per = int(rng.choice([1, 2, 4]))
    i = np.repeat(np.arange(n, dtype=np.int64), per)
    j = rng.integers(0, n, i.size)
    d = np.arange(n, dtype=np.int64)
    return tr.from_coo(n, np.concatenate([i, j, d]), np.concatenate([j, i, d]))


def _values(rng, pattern, dtype, cls):
    n, rowptr, colind = pattern
    values, _ = kr.spd_fill(pattern, np.float64, rng)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    isd = rows == colind.astype(np.int64)
    if cls == "indefinite":                          # a zero-mean diagonal
        d = rng.standard_normal(n) * 3.0
        values[isd] = d - d.mean()
    elif cls == "clustered":                         # few distinct diagonal values, coupled by 1e-6
        values[~isd] *= 1e-6
        values[isd] = rng.choice([1.0, 2.0, 2.5, 7.0], size=n)
    elif cls in ("scaled_down", "scaled_up"):
        values = values * SCALE[cls, np.dtype(dtype).itemsize]
    return values.astype(dtype)


@functools.lru_cache(maxsize=None)
def case(seed):
    """(mat, knobs) of one seed: mat = (n, rowptr, colind, values); built once per process, shared, read-only.

    knobs: n, cls, dtype, kind, k, which, ncv, tol (0: the machine epsilon), maxit, v0 (None or a vector), seed, rotate
    (1: batched, 2: LDS tiles), jacobi ("lib" from ncv = 25 on)."""
    rng = np.random.default_rng(BASE_SEED + seed)
    n = N_TABLE[seed % len(N_TABLE)]
    cls = CLASSES[(seed + seed // 15) % len(CLASSES)]
    dtype = np.dtype((np.float64, np.float32)[(seed // 2 + seed // 15) % 2])
    ncv = min(NCV_TABLE[(5 * seed + seed // 12) % len(NCV_TABLE)], n)
    k = (1, max(ncv // 2, 1), ncv - 1)[seed % 3]
    pattern = _pattern(rng, n, seed)
    values = _values(rng, pattern, dtype, cls)
    tol = (0.0, TOL[dtype], 1e-2)[int(rng.integers(3))]
    maxit = MAXIT[int(rng.integers(len(MAXIT)))]
    if n <= SMALL and seed % 6 != 5:                 # the small sizes mostly run to convergence: the host test compares
        tol, maxit = TOL[dtype], SMALL_MAXIT         # their values with numpy.linalg.eigvalsh.  (A value converged to 1e-2
                                                     # may have passed an eigenvalue by, and at the machine epsilon the
                                                     # true residual's own rounding exceeds the bound.)
    v0 = rng.uniform(-1, 1, size=n).astype(dtype) if rng.random() < 0.4 else None
    knobs = dict(n=n, cls=cls, dtype=dtype, kind=("csr", "csc")[(seed + seed // 5) % 2], k=k, which=("LA", "SA")[(seed // 3) % 2],
                 ncv=ncv, tol=tol, maxit=maxit, v0=v0, seed=SEEDS[int(rng.integers(len(SEEDS)))],
                 rotate=1 + (seed + seed // 4) % 2, jacobi="lib" if ncv >= LIB_JACOBI_FROM else "numpy")
    if v0 is not None:
        v0.setflags(write=False)
    return readonly((*pattern, values)), knobs


def text(mat, k, mul=None, jacobi_fn=None):
    """the text on a case's knobs, with the host product unless `mul` is given"""
    dtype = k["dtype"].type
    return er.eigsh(mul or host_mul(mat), mat[0], dtype, k["k"], k["which"], k["ncv"], k["tol"] or default_tol(dtype), k["maxit"],
                    k["v0"], k["seed"], jacobi_fn)
