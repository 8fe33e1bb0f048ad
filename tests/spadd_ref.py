"""CPU restatement of the reference's Add / Sub / Neg for compressed matrices (test infrastructure, not the library).

Every function works on arrays compressed by the MAJOR index: (ptr, ind, values) of a CSR matrix with nmajor = nrows,
or of a CSC matrix with nmajor = ncols (the CSC arrays of A are the CSR arrays of A^T, and A^T + B^T = (A + B)^T).

* ``add_sub_loop``: line by line the loop of src/csr/ops/add.rs:12-73 / sub.rs:12-73 (transpose both operands, merge
  every row through the `set` / `vec` workspace, transpose back), with the intermediate labelled with the TRANSPOSED
  dimensions.  The reference labels it with the untransposed ones, which is only right for square inputs.
* ``add_sub_fast``: the same result vectorised (a lexsort on (major, minor, operand), adjacent duplicates merged), for
  large cases.
* ``neg``: src/csr/ops/neg.rs:5-17.
"""
import numpy as np

import oracle


def add_sub_loop(nmajor, nminor, a, b, sub):
    dt = np.asarray(a[2]).dtype
    # let (lhs, rhs) = (self.transpose(), rhs.transpose()): nminor x nmajor
    lp, li, lv = oracle.transpose(nmajor, nminor, a[0], a[1], np.asarray(a[2], dtype=dt))
    rp, ri, rv = oracle.transpose(nmajor, nminor, b[0], b[1], np.asarray(b[2], dtype=dt))
    lp, li, rp, ri = (x.astype(np.int64) for x in (lp, li, rp, ri))
    ptr, ind, values = [], [], []
    seen = np.zeros(nmajor, dtype=np.int64)          # `set`, over lhs.ncols() = nmajor
    vec = np.zeros(nmajor, dtype=dt)
    nz = 0
    for row in range(nminor):                        # lhs.nrows()
        ptr.append(nz)
        for p in range(lp[row], lp[row + 1]):
            col = li[p]
            if seen[col] < row + 1:
                seen[col] = row + 1
                ind.append(col)
                vec[col] = lv[p]
                nz += 1
            else:
                vec[col] = np.add(vec[col], lv[p], dtype=dt)
        for p in range(rp[row], rp[row + 1]):
            col = ri[p]
            if seen[col] < row + 1:
                seen[col] = row + 1
                ind.append(col)
                vec[col] = np.negative(rv[p]) if sub else rv[p]
                nz += 1
            else:
                vec[col] = np.subtract(vec[col], rv[p], dtype=dt) if sub else np.add(vec[col], rv[p], dtype=dt)
        for p in range(ptr[row], nz):
            values.append(vec[ind[p]])
    ptr.append(nz)
    # the output is nminor x nmajor (the F9 fix: the reference writes nmajor x nminor here), transposed back
    return oracle.transpose(nminor, nmajor, np.array(ptr, dtype=np.uint64), np.array(ind, dtype=np.uint64),
                            np.array(values, dtype=dt))


def add_sub_fast(nmajor, nminor, a, b, sub):
    (ap, ai, av), (bp, bi, bv) = a, b
    ap, bp = np.asarray(ap, dtype=np.int64), np.asarray(bp, dtype=np.int64)
    av, bv = np.asarray(av), np.asarray(bv)
    dt = av.dtype
    maj = np.concatenate([np.repeat(np.arange(nmajor, dtype=np.int64), np.diff(ap)),
                          np.repeat(np.arange(nmajor, dtype=np.int64), np.diff(bp))])
    mino = np.concatenate([np.asarray(ai, dtype=np.int64), np.asarray(bi, dtype=np.int64)])
    src = np.concatenate([np.zeros(av.size, dtype=np.int8), np.ones(bv.size, dtype=np.int8)])
    val = np.concatenate([av, bv.astype(dt, copy=False)])
    order = np.lexsort((src, mino, maj))
    M, N, S, V = maj[order], mino[order], src[order], val[order]
    dup = np.zeros(M.size, dtype=bool)               # a B entry right behind the A entry of its position
    dup[1:] = (M[1:] == M[:-1]) & (N[1:] == N[:-1])
    out = V.copy()
    if sub:
        b_only = (S == 1) & ~dup
        out[b_only] = np.negative(V[b_only])
    pair = np.nonzero(dup)[0] - 1                    # the A entry of every matched pair
    with np.errstate(invalid="ignore"):              # (inf - inf is a NaN, as in the reference)
        out[pair] = np.subtract(V[pair], V[pair + 1]) if sub else np.add(V[pair], V[pair + 1])
    keep = ~dup
    ptr = np.concatenate([[0], np.cumsum(np.bincount(M[keep], minlength=nmajor))]).astype(np.uint64)
    return ptr, N[keep].astype(np.uint64), out[keep]


def neg(a):
    p, i, v = a
    return np.asarray(p, dtype=np.uint64), np.asarray(i, dtype=np.uint64), np.negative(np.asarray(v))


def matched(nmajor, a, b):
    """matched pairs (positions stored in both operands)"""
    ap, bp = np.asarray(a[0], dtype=np.int64), np.asarray(b[0], dtype=np.int64)
    ka = np.repeat(np.arange(nmajor, dtype=np.int64), np.diff(ap)) * (1 << 32) + np.asarray(a[1], dtype=np.int64)
    kb = np.repeat(np.arange(nmajor, dtype=np.int64), np.diff(bp)) * (1 << 32) + np.asarray(b[1], dtype=np.int64)
    return int(np.intersect1d(ka, kb, assume_unique=True).size)
