"""CPU restatement of FSAI (include/spal.h) and the matrices its tests use.

`row` is the text's Cholesky and back-substitution on one local system, `fsai` the whole factor.  Everything is computed
in the dtype T of the values: every product is rounded before the difference or sum it enters, and every element of C
sees its k loop in the text's order (the loop over k is sequential; the elements r of one column, which are independent
of each other, go through it side by side as numpy vectors -- the same operations on the same operands).
A matrix is (n, rowptr, colind, values) with uint64 indices, columns ascending inside a row.
"""
import numpy as np

CAP_DEFAULT = 32


# ---- the text -------------------------------------------------------------------------------------------------------------
def reject_diag(aii, dt):
    with np.errstate(all="ignore"):
        if aii > 0 and np.isfinite(aii):
            d = dt(1) / np.sqrt(dt(aii))
            if np.isfinite(d):
                return dt(d)
    return dt(1)


def row(B, dtype):
    """(g, rejected) for the local system B (m x m; only the lower triangle is read)."""
    dt = np.dtype(dtype).type
    B = np.asarray(B, dtype=dtype)
    m = B.shape[0]
    C = np.zeros((m, m), dtype=dtype)
    g = np.zeros(m, dtype=dtype)
    rejected = False
    with np.errstate(all="ignore"):
        for j in range(m):
            col = B[j:, j].copy()                       # elements (r, j), r = j .. m - 1; r = j is d
            for k in range(j):
                col = col - (C[j:, k] * C[j, k])
            d = col[0]
            if not (d > 0 and np.isfinite(d)):
                rejected = True
                break
            cjj = np.sqrt(d)
            C[j, j] = cjj
            C[j + 1:, j] = col[1:] / cjj
        if not rejected:
            g[m - 1] = dt(1) / C[m - 1, m - 1]
            for t in range(m - 2, -1, -1):
                s = dt(0)
                for u in range(t + 1, m):
                    s = dt(s + dt(C[u, t] * g[u]))
                g[t] = dt(dt(0) - s) / C[t, t]
            rejected = not bool(np.all(np.isfinite(g)))
        if rejected:
            g[:] = 0
            g[m - 1] = reject_diag(B[m - 1, m - 1], dt)
    return g, int(rejected)


def pack_lower(B):
    B = np.asarray(B)
    return np.ascontiguousarray(B[np.tril_indices(B.shape[0])])


def fsai(a, pattern=None, cap=CAP_DEFAULT):
    """(G, rejected, max_row): G = (n, rowptr, colind, values) of the text for the matrix `a` on the structure of
    `pattern` (None: a's own)."""
    n, rowptr, colind, values = a
    dtype = values.dtype
    sp_, si_ = (rowptr, colind) if pattern is None else (pattern[1], pattern[2])
    rp, ci = rowptr.astype(np.int64), colind.astype(np.int64)
    sp_, si_ = sp_.astype(np.int64), si_.astype(np.int64)
    lower = [dict() for _ in range(n)]                  # the stored entries on or below the diagonal, by row
    for i in range(n):
        for q in range(rp[i], rp[i + 1]):
            if ci[q] <= i:
                lower[i][int(ci[q])] = values[q]
    gptr = np.zeros(n + 1, dtype=np.uint64)
    gind, gval = [], []
    rejected = max_row = 0
    for i in range(n):
        Q = [int(c) for c in si_[sp_[i]:sp_[i + 1]] if c <= i]
        assert Q and Q[-1] == i, f"row {i} of the pattern stores no diagonal entry"
        m = min(len(Q), cap)
        max_row = max(max_row, m)
        P = Q[len(Q) - m:]
        B = np.zeros((m, m), dtype=dtype)
        for s in range(m):
            held = lower[P[s]]
            for t in range(s + 1):
                if P[t] in held:
                    B[s, t] = held[P[t]]
        g, rej = row(B, dtype)
        rejected += rej
        gind += Q
        gval += [np.zeros(len(Q) - m, dtype=dtype), g]
        gptr[i + 1] = gptr[i] + len(Q)
    G = (n, gptr, np.array(gind, dtype=np.uint64), np.concatenate(gval) if gval else np.zeros(0, dtype=dtype))
    return G, rejected, max_row


def transpose(G):
    """Gt as a CSR matrix: a stable sort of the entries by column (values moved bit for bit)."""
    n, rowptr, colind, values = G
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    order = np.argsort(colind.astype(np.int64), kind="stable")
    tptr = np.zeros(n + 1, dtype=np.uint64)
    tptr[1:] = np.cumsum(np.bincount(colind.astype(np.int64), minlength=n))
    return n, tptr, rows[order].astype(np.uint64), values[order]


def spmv_seq(mat, x):
    """Sequential row sums in the values' dtype: acc = +0.0; acc = acc + (v * x[j]) in storage order."""
    n, rowptr, colind, values = mat
    rp, ci = rowptr.astype(np.int64), colind.astype(np.int64)
    y = np.zeros(n, dtype=values.dtype)
    lens = np.diff(rp)
    with np.errstate(all="ignore"):
        for k in range(int(lens.max()) if n else 0):      # the k-th entry of every row that has one, side by side
            live = np.flatnonzero(lens > k)
            q = rp[live] + k
            y[live] = y[live] + values[q] * x[ci[q]]
    return y


def apply(G, Gt, v):
    return spmv_seq(Gt, spmv_seq(G, v))


def dense(mat):
    n, rowptr, colind, values = mat
    D = np.zeros((n, n), dtype=np.float64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    D[rows, colind.astype(np.int64)] = values
    return D


# ---- matrices -------------------------------------------------------------------------------------------------------------
def from_triplets(n, r, c, v, dtype):
    """Sorted by (row, column); a duplicate keeps its LAST value."""
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    v = np.asarray(v)
    key = r * n + c
    order = np.argsort(key, kind="stable")
    key, v = key[order], v[order]
    last = np.append(key[1:] != key[:-1], True)
    key, v = key[last], v[last]
    rowptr = np.zeros(n + 1, dtype=np.uint64)
    rowptr[1:] = np.cumsum(np.bincount(key // n, minlength=n))
    return n, rowptr, (key % n).astype(np.uint64), v.astype(dtype)


def readonly(mat):
    for a in mat[1:]:
        a.setflags(write=False)
    return mat


def poisson2d(m, dtype):
    """the 5-point Laplacian on an m x m grid: 4 on the diagonal, -1 to the four neighbours"""
    idx = np.arange(m * m).reshape(m, m)
    r, c, v = [idx.ravel()], [idx.ravel()], [4 * np.ones(m * m)]
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        r += [a.ravel(), b.ravel()]
        c += [b.ravel(), a.ravel()]
        v += [-np.ones(a.size), -np.ones(a.size)]
    return from_triplets(m * m, np.concatenate(r), np.concatenate(c), np.concatenate(v), dtype)


def symmetric(n, i, j, w, dtype, dominant=True, diag=None):
    """The symmetric matrix with w[k] at (i[k], j[k]) and (j[k], i[k]), i != j, and the diagonal 1 + the row's sum of
    |off-diagonal| (`dominant`: symmetric positive definite) or `diag`."""
    i, j, w = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64), np.asarray(w, dtype=np.float64)
    off = np.bincount(np.concatenate([i, j]), weights=np.abs(np.concatenate([w, w])), minlength=n)
    d = 1.0 + off if dominant else np.asarray(diag, dtype=np.float64)
    k = np.arange(n, dtype=np.int64)
    return from_triplets(n, np.concatenate([i, j, k]), np.concatenate([j, i, k]), np.concatenate([w, w, d]), dtype)


def band(n, width, dtype, seed=0):
    """Symmetric positive definite; row i holds min(i + 1, width) entries on or below the diagonal."""
    rng = np.random.default_rng(1000 + seed)
    i = np.repeat(np.arange(n, dtype=np.int64), width - 1)
    j = i - np.tile(np.arange(1, width, dtype=np.int64), n)
    keep = j >= 0
    i, j = i[keep], j[keep]
    return symmetric(n, i, j, rng.uniform(-1, 1, size=i.size), dtype)


def dense_spd(n, dtype, seed=0):
    i, j = np.tril_indices(n, -1)
    return symmetric(n, i, j, np.random.default_rng(2000 + seed).uniform(-1, 1, size=i.size), dtype)


def arrow(n, dtype):
    """A dense last row and column beside the diagonal."""
    j = np.arange(n - 1, dtype=np.int64)
    return symmetric(n, np.full(n - 1, n - 1), j, np.random.default_rng(3000).uniform(-1, 1, size=n - 1), dtype)


def diagonal_pattern(n, dtype=np.float64):
    d = np.arange(n, dtype=np.int64)
    return from_triplets(n, d, d, np.ones(n), dtype)


def product_pattern(a, b):
    """The structure of a @ b (every structural product kept), values 1."""
    D = (np.abs(dense(a)) > 0).astype(np.float32) @ (np.abs(dense(b)) > 0).astype(np.float32)
    r, c = np.nonzero(D)
    return from_triplets(a[0], r, c, np.ones(r.size), np.float64)


def with_values(mat, where, value):
    """A copy with the stored entries (r, c) in `where` set to `value`."""
    n, rowptr, colind, values = mat
    values = values.copy()
    for r, c in where:
        s, e = int(rowptr[r]), int(rowptr[r + 1])
        q = s + int(np.searchsorted(colind[s:e].astype(np.int64), c))
        assert q < e and colind[q] == c
        values[q] = value
    return n, rowptr, colind, values


def fuzz_case(rng):
    """(matrix, cap): a random symmetric pattern, n <= 300, rows of up to 80 entries on or below the diagonal; values
    diagonally dominant, or in a quarter of the cases a diagonal drawn from [-0.5, 2.5) whatever the row's sum."""
    n = int(rng.integers(1, 301))
    dtype = np.float64 if rng.integers(2) else np.float32
    longest = int(rng.integers(1, 81))
    i, j = [], []
    for r in range(1, n):
        k = int(rng.integers(0, min(longest, r) + 1))
        lo = max(0, r - int(rng.integers(k, 4 * k + 2)))
        c = rng.choice(np.arange(lo, r), size=min(k, r - lo), replace=False)
        i += [r] * c.size
        j += c.tolist()
    w = rng.uniform(-1, 1, size=len(i))
    if rng.integers(4) == 0:
        mat = symmetric(n, i, j, w, dtype, dominant=False, diag=rng.uniform(-0.5, 2.5, size=n))
    else:
        mat = symmetric(n, i, j, w, dtype)
    return readonly(mat), int(rng.integers(1, 65))
