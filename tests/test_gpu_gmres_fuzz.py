"""Restarted GMRES on seeded random matrices against its sequential text (tests/gmres_ref.py): raw bits, no tolerance,
no case skipped.  Every seed draws a pattern from the generators of tests/trsv_ref.py and tests/ilu_ref.py with n in
[1, 5000], trsv_ref.fill's values, the handle kind, the element type, restart in 1 .. 12, maxit, x0, the poll interval and
the form of M: none, a.ilu0() by exact solves, a.ilu0() by two sweeps, the matrix itself by zero sweeps (Jacobi).  The
reference runs with the device's own spmv / solve_triangular as callables, as tests/test_gpu_gmres.py explains."""
import os
import time

import numpy as np
import pytest

import spalinalg_amd as sp
from tests import gmres_ref as gr
from tests import ilu_ref as ir
from tests import trsv_ref as tr

pytestmark = pytest.mark.gpu

BASE_SEED = 20261018
SHAPES = ["banded", "full", "bidiagonal", "diagonal", "arrow", "banded-sym"]
MODES = ["none", "ilu0", "ilu0-sweeps2", "jacobi"]
CHECK_EVERY = [1, 2, 3, 5, 8, 64]
MAXIT = [0, 1, 7, 40, 200]


def draw(seed):
    rng = np.random.default_rng(BASE_SEED + seed)
    n = 1 if seed % 12 == 11 else int(rng.integers(1, 5001))
    shape = SHAPES[seed % len(SHAPES)]
    if shape == "banded":
        pattern = tr.banded(n, int(rng.integers(1, 7)), int(rng.integers(1, 600)), rng)      # lower triangular
    elif shape == "banded-sym":
        pattern = ir.sym(tr.banded(n, int(rng.integers(1, 7)), int(rng.integers(1, 600)), rng))
    elif shape == "full":
        pattern = ir.full(n, int(rng.integers(1, 9)), rng)
    elif shape == "bidiagonal":
        pattern = ir.sym(tr.bidiagonal(n))
    elif shape == "diagonal":
        pattern = tr.diagonal(n)
    else:
        pattern = tr.arrow(n) if n >= 2 else tr.diagonal(n)
    dtype = (np.float64, np.float32)[int(rng.integers(2))]
    values, b = tr.fill(pattern, dtype, rng)
    knobs = dict(n=n, shape=shape, dtype=dtype, kind=("csr", "csc")[int(rng.integers(2))], mode=MODES[(seed // 2) % len(MODES)],
                 restart=int(rng.integers(1, 13)), maxit=MAXIT[int(rng.integers(len(MAXIT)))],
                 check_every=int(rng.choice(CHECK_EVERY)), tol=1e-10 if dtype == np.float64 else 1e-5,
                 x0=rng.uniform(-1, 1, size=n).astype(dtype) if rng.random() < 0.5 else None)
    return pattern, values, b, knobs


@pytest.mark.parametrize("seed", range(int(os.environ.get("SPAL_FUZZ_SEEDS", "12"))))   # (more seeds: a longer soak)
def test_gmres_is_its_sequential_text(seed):
    t_start = time.perf_counter()
    pattern, values, b, k = draw(seed)
    n = pattern[0]
    if k["kind"] == "csr":
        a = sp.CsrMatrix(n, n, pattern[1], pattern[2], values)
    else:
        colptr, rowind, vals, _ = ir.to_csc(pattern, values)
        a = sp.CscMatrix(n, n, colptr, rowind, vals)
    dev = a.device()
    dev.set_option("krylov_check_every", k["check_every"])
    m = sweeps = prec = None
    if k["mode"] == "jacobi":
        m, sweeps = a, 0
        prec = lambda v: a.solve_triangular(a.solve_triangular(v, True, True, sweeps=0), False, False, sweeps=0)   # noqa: E731
    elif k["mode"] != "none":
        m = a.ilu0()
        sweeps = 2 if k["mode"] == "ilu0-sweeps2" else None
        prec = lambda v: m.solve_triangular(m.solve_triangular(v, True, True, sweeps=sweeps), False, False, sweeps=sweeps)   # noqa: E731
    x, info = a.gmres(b, M=m, x0=k["x0"], restart=k["restart"], tol=k["tol"], maxit=k["maxit"], precond_sweeps=sweeps)
    x0 = np.zeros_like(b) if k["x0"] is None else k["x0"]
    xr, ref = gr.gmres(lambda v: dev.spmv(v), prec, b, x0, k["restart"], k["tol"], k["maxit"])
    tr.assert_same_bits(x, xr)
    assert (info.iterations, info.reason) == (ref["iterations"], ref["reason"])
    tr.assert_same_bits(np.array([info.residual_sq]), np.array([ref["residual_sq"]]))
    assert info.rhs_sq == ref["rhs_sq"]
    d = dev.describe()["gmres"]
    assert d["restart"] == k["restart"] and d["check_every"] == k["check_every"] and d["iterations"] == info.iterations
    assert d["preconditioned"] == int(m is not None) and d["precond_sweeps"] == (-1 if sweeps is None else sweeps)
    assert info.iterations <= k["maxit"] and d["polls"] >= 1
    print(f"gmres fuzz seed {seed}: n {n} {k['shape']} {k['kind']} {np.dtype(k['dtype']).name} {k['mode']} restart "
          f"{k['restart']} maxit {k['maxit']} every {k['check_every']} (reason, iterations) "
          f"{(info.reason, info.iterations)} cycles {d['cycles']} {time.perf_counter() - t_start:.2f} s")
