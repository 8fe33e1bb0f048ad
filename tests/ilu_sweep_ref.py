"""CPU restatement of ILU(0) by row sweeps (include/spal.h).

The contract is `ilu0_sweep_loop`: F0 is A's values; in pass t = 1 .. s every row i, on its own, starts as a copy of
A's row i and runs the body of ILU(0)'s loop (tests/ilu_ref.py) with every read of ANOTHER row -- the pivot F[k,k] and
the tail of row k -- taken from F(t-1), while the row's own running values are this pass's.  Products and differences
are rounded separately in the matrix dtype.  `ilu0_sweep_rows` is the same arithmetic with the updates of one (i, k)
taken together as numpy vectors (they touch distinct entries); tests/test_ilu_sweep_host.py proves the two bit-equal
and the device tests use the faster one.  Patterns and values come from ilu_ref / trsv_ref.
"""
import numpy as np

from . import ilu_ref as ir


def ilu0_sweep_loop(n, rowptr, colind, values, sweeps):
    """THE definition, in numpy scalars of the matrix dtype."""
    dt = values.dtype.type
    rp = [int(p) for p in rowptr]
    ci = [int(c) for c in colind]
    dg = [int(d) for d in ir.diag_positions(n, rowptr, colind)]
    prev = values.copy()
    with np.errstate(all="ignore"):
        for _ in range(int(sweeps)):
            f = values.copy()                          # every row starts as A's
            for i in range(n):
                where = {ci[q]: q for q in range(rp[i], rp[i + 1])}
                for p in range(rp[i], dg[i]):
                    k = ci[p]
                    w = dt(f[p] / prev[dg[k]])
                    f[p] = w
                    for pu in range(dg[k] + 1, rp[k + 1]):
                        q = where.get(ci[pu])
                        if q is not None:
                            f[q] = dt(f[q] - dt(w * prev[pu]))
            prev = f
    return prev


def ilu0_sweep_rows(n, rowptr, colind, values, sweeps):
    """ilu0_sweep_loop's arithmetic; the updates of one (i, k) in one numpy operation each (elementwise multiply, then
    elementwise subtract: two roundings, as in the loop)."""
    rp = rowptr.astype(np.int64)
    ci = colind.astype(np.int64)
    dg = ir.diag_positions(n, rowptr, colind)
    prev = values.copy()
    with np.errstate(all="ignore"):
        for _ in range(int(sweeps)):
            f = values.copy()
            for i in range(n):
                e = int(rp[i + 1])
                for p in range(int(rp[i]), int(dg[i])):
                    k = int(ci[p])
                    w = f[p] / prev[dg[k]]
                    f[p] = w
                    u0, u1 = int(dg[k]) + 1, int(rp[k + 1])
                    if u0 == u1 or p + 1 == e:
                        continue
                    tail = ci[p + 1:e]                       # row i past (i, k): ascending
                    at = np.searchsorted(tail, ci[u0:u1])
                    hit = at < tail.size
                    hit[hit] = tail[at[hit]] == ci[u0:u1][hit]
                    q = p + 1 + at[hit]
                    f[q] = f[q] - w * prev[u0:u1][hit]
            prev = f
    return prev
