"""The aggregation AMG on seeded random matrices against its sequential text (tests/amg_ref.py), one handle per seed:
the hierarchy (aggregates, every level's structure and value bits, the stop rule, the ROUNDS each level took), one cycle
under every drawn "amg_tail_rows", CG or BiCGStab preconditioned by the cycle, and a second hierarchy from the same
handle.

Every comparison is of raw bits (NaN by position): the contracts are bitwise, so there is no tolerance anywhere in this
file.  tests/amg_cases.py draws the matrices (irregular graphs with one-sided patterns, isolated vertices, hubs and
aggregates around 32 members and the steps of 64, a descending path beside components that finish early, integer values
whose coarse sums cancel) and the knobs; tests/test_amg_cases_host.py proves on the CPU that the default seeds reach what
this file is there for, and compares the text itself with the mathematics.

The Krylov reference runs with the device's own spmv as its product and the TEXT's cycle as M^-1, as
tests/test_gpu_amg.py::test_krylov_with_amg_is_the_loop does."""
import os
import time

import numpy as np
import pytest

from tests import amg_cases as ac
from tests import amg_ref as ar
from tests import trsv_ref as tr
from tests.test_gpu_amg import _check_hierarchy, _kw_device, _matrix

pytestmark = pytest.mark.gpu

same = tr.assert_same_bits


@pytest.mark.parametrize("seed", range(int(os.environ.get("SPAL_FUZZ_SEEDS", "24"))))   # (more seeds: a longer soak)
def test_amg_is_its_sequential_text(seed):
    t_start = time.perf_counter()
    pattern, values, b, k = ac.case(seed)
    h = ac.reference(seed)
    a = _matrix(k["kind"], pattern, values)
    g = a.amg(**_kw_device(k["params"]))
    _check_hierarchy(g, h)                                          # (rounds included, by amg_cases.expected_rounds)
    d = g.describe()
    rounds = d["rounds"][:len(h.levels) - 1]

    # ---- one cycle, wherever the tail starts ----
    ref = h.cycle(b)
    for tail in k["tails"]:
        g.set_option("amg_tail_rows", tail)
        assert g.describe()["tail_from_level"] == ac.tail_from_level(h.rows, tail), tail
        same(g.apply(b), ref)
    g.set_option("amg_tail_rows", ac.TAIL_DEFAULT)

    # ---- CG / BiCGStab with the cycle as M^-1 ----
    xr, want = ar.solve(h, lambda v: a.device().spmv(v), b, k["method"], k["tol"], k["maxit"])
    x, info = a.solve(b, k["method"], M=g, tol=k["tol"], maxit=k["maxit"])
    same(x, xr)
    assert (info.iterations, info.reason) == (want["iterations"], want["reason"])
    same(np.array([info.residual_sq]), np.array([want["residual_sq"]]))

    # ---- a second hierarchy from the same handle: the same bits throughout (two rounds kernels that raced would show) ----
    g2 = a.amg(**_kw_device(k["params"]))
    _check_hierarchy(g2, h)
    d2 = g2.describe()
    assert all(d2[key] == d[key] for key in ("levels", "rows", "nnz", "aggregates", "rounds", "stopped_by"))
    for l in range(len(h.levels) - 1):
        assert np.array_equal(g2.aggregates(l), g.aggregates(l))
    same(g2.apply(b), ref)
    g2.close()
    g.close()

    print(f"amg fuzz seed {seed}: n {k['n']} {k['kind']} {k['dtype'].name} rows {h.rows} stopped by {h.stopped_by} "
          f"rounds {rounds} gamma {k['params']['gamma']} {k['method']} (reason, iterations) {(info.reason, info.iterations)} "
          f"{time.perf_counter() - t_start:.2f} s")
