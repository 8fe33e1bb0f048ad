"""The solver stack on seeded random matrices against its sequential texts: the exact triangular solves
(tests/trsv_ref.py), the Jacobi sweeps (tests/sweep_ref.py), ILU(0) (tests/ilu_ref.py) and CG / BiCGStab
(tests/krylov_ref.py), one handle per seed, whatever the launch schedule is.

Every comparison is of raw bits (NaN by position): the contracts are bitwise, so there is no tolerance anywhere in this
file.  tests/solver_cases.py draws the matrices (deep chains next to levels wider than a workgroup, rows of thousands
of entries, diagonal-only stretches, missing diagonals) and the knobs; tests/test_solver_cases_host.py proves on the CPU
that the default seeds reach the schedule decisions this file is there for, and that `expected_launches` and
`expected_wide_rows` say something on them.

The Krylov reference runs with the device's own spmv as its product (deterministic, its row sums in the order the plan
gives them, as tests/test_gpu_krylov.py explains) and a preconditioner computed on the host alone.  From
sweeps = levels - 1 on, the sweep reference is the exact solve (the host test proves that on the small seeds with the
loops), which keeps thousands of reference passes over a row of thousands of entries out of this file."""
import os
import time

import numpy as np
import pytest

import spalinalg_amd as sp
from tests import ilu_ref as ir
from tests import krylov_ref as kr
from tests import solver_cases as sc
from tests import sweep_ref as sw
from tests import trsv_ref as tr

pytestmark = pytest.mark.gpu

same = tr.assert_same_bits


def make(kind, pattern, values):
    n = pattern[0]
    ptr, ind, val = sc.to_handle_arrays(kind, pattern, values)
    return (sp.CsrMatrix if kind == "csr" else sp.CscMatrix)(n, n, ptr, ind, val)


def key_of(lower):
    return "lower" if lower else "upper"


def check_plans(dev, widths, chain_rows):
    """describe()["trsv"] of both triangles against the host's levels and launch list."""
    d = dev.describe()["trsv"]
    for lower in (True, False):
        t = d[key_of(lower)]
        assert t["levels"] == len(widths[lower]) and t["max_level_rows"] == max(widths[lower])
        assert (t["launches"], t["chain_launches"]) == sc.expected_launches(widths[lower], chain_rows), (t, chain_rows)
        assert t["chain_rows"] == chain_rows
    assert d["analyses"] == 2


def check_krylov(a, f, pattern, fv, b, x0, k, every):
    """One solve against the reference loop; returns (x, info)."""
    method, mode = k["method"], k["prec"]
    dev = a.device()
    x, info = a.solve(b, method, M=None if mode == "none" else f, x0=x0, tol=k["tol"], maxit=k["maxit"],
                      precond_sweeps=sc.PREC_SWEEPS.get(mode))
    xr, ref = kr.METHODS[method](lambda v: dev.spmv(v), sc.host_preconditioner(pattern, fv, mode), b, x0, k["tol"], k["maxit"])
    same(x, xr)
    assert (info.iterations, info.reason) == (ref["iterations"], ref["reason"])
    same(np.array([info.residual_sq]), np.array([ref["residual_sq"]]))
    assert info.rhs_sq == ref["rhs_sq"]
    d = dev.describe()["krylov"]
    assert d["method"] == method and d["preconditioned"] == int(mode != "none") and d["check_every"] == every
    assert d["precond_sweeps"] == sc.PREC_SWEEPS.get(mode, -1) and d["iterations"] == info.iterations
    # the poll after the stop is the last; a call that stops at iteration 0 still polls once
    assert d["polls"] == max(1, -(-info.iterations // every))
    return x, info


@pytest.mark.parametrize("seed", range(int(os.environ.get("SPAL_FUZZ_SEEDS", "24"))))   # (more seeds: a longer soak)
def test_solver_stack_is_its_sequential_text(seed):
    t_start = time.perf_counter()
    pattern, values, b, x0, k = sc.case(seed)
    n, kind = pattern[0], k["kind"]
    units = (True,) if k["dropped"] else (False, True)
    triangles = [(lower, unit) for lower in (True, False) for unit in units]
    widths = {lower: tr.level_widths(*tr.levels(*pattern, lower=lower)) for lower in (True, False)}
    assert {lower: len(w) for lower, w in widths.items()} == k["levels"]

    a = make(kind, pattern, values)
    dev = a.device()
    dev.set_option("trsv_chain_rows", k["chain_rows"])
    if k["wide_work"] is not None:
        dev.set_option("ilu_wide_work", k["wide_work"])
    dev.set_option("krylov_check_every", k["check_every"])

    # ---- exact solves ----
    exact = {}
    for lower, unit in triangles:
        exact[lower, unit] = tr.solve_by_levels(*pattern, values, b, lower, unit)
        same(dev.trsv(b, lower, unit), exact[lower, unit])
    check_plans(dev, widths, k["chain_rows"])

    # ---- ILU(0) and the factor applied (at the first trsv_chain_rows: the factor's handle inherits it) ----
    f = fv = None
    if not k["dropped"]:
        fv = ir.ilu0_rows(*pattern, values)
        f = a.ilu0()
        fptr, find, fval = sc.to_handle_arrays(kind, pattern, fv)
        if kind == "csr":
            assert np.array_equal(f.rowptr(), fptr) and np.array_equal(f.colind(), find)
        else:
            assert np.array_equal(f.colptr(), fptr) and np.array_equal(f.rowind(), find)
        same(f.values(), fval)
        d = f.device().describe()["ilu0"]
        if k["wide_work"] is not None:
            assert d["wide_work"] == k["wide_work"]
        assert d["rows_wide_form"] == sc.expected_wide_rows(pattern, d["wide_work"]), d
        assert d["rows_row_form"] + d["rows_wide_form"] == n
        assert d["levels"] == len(widths[True]) and d["chain_rows"] == k["chain_rows"]
        assert (d["launches"], d["chain_launches"]) == sc.expected_launches(widths[True], k["chain_rows"]), d
        assert dev.describe()["trsv"]["analyses"] == 2              # the factorisation took the lower plan as it was
        y_ref = tr.solve_by_levels(*pattern, fv, b, True, True)
        y = f.solve_triangular(b, lower=True, unit_diagonal=True)
        same(y, y_ref)
        same(f.solve_triangular(y, lower=False), tr.solve_by_levels(*pattern, fv, y_ref, False, False))
        for s in (0, 2):
            y = f.solve_triangular(b, lower=True, unit_diagonal=True, sweeps=s)
            same(f.solve_triangular(y, lower=False, sweeps=s), sw.preconditioner(pattern, fv, s)(b))

    # ---- another trsv_chain_rows: the same bits, the new launch list, nothing analysed ----
    dev.set_option("trsv_chain_rows", k["chain_rows_2"])
    for lower, unit in triangles:
        same(dev.trsv(b, lower, unit), exact[lower, unit])
    check_plans(dev, widths, k["chain_rows_2"])

    # ---- sweeps ----
    swept = {}
    for lower, unit in triangles:
        nl = k["levels"][lower]
        for s in k["sweeps"][lower]:
            ref = exact[lower, unit] if s >= nl - 1 else sw.sweep_vec(*pattern, values, b, s, lower, unit)
            swept[lower, unit, s] = ref
            same(dev.trsv_sweep(b, s, lower, unit), ref)
    d = dev.describe()
    assert d["trsv_sweep"]["prepared"] == 1 and d["trsv_sweep"]["calls"] == sum(len(k["sweeps"][lo]) for lo, _ in triangles)
    assert d["trsv"]["analyses"] == 2

    # ---- CG / BiCGStab ----
    outcome = None
    if not k["dropped"]:
        x, info = check_krylov(a, f, pattern, fv, b, x0, k, k["check_every"])
        dev.set_option("krylov_check_every", k["check_every_2"])
        x2, info2 = check_krylov(a, f, pattern, fv, b, x0, k, k["check_every_2"])
        same(x2, x)
        assert (info2.iterations, info2.reason, info2.residual_sq) == (info.iterations, info.reason, info.residual_sq)
        outcome = (info.reason, info.iterations)

    # ---- the device forms in place on a stream of the caller's ----
    if k["in_place"]:
        import torch
        st = torch.cuda.Stream()
        bt = torch.tensor(b).cuda()
        for lower, unit in triangles:
            nl = k["levels"][lower]
            work = [bt.clone() for _ in range(3)]
            torch.cuda.synchronize()
            dev.trsv_dev(work[0].data_ptr(), work[0].data_ptr(), lower, unit, st)
            dev.trsv_sweep_dev(work[1].data_ptr(), work[1].data_ptr(), 2, lower, unit, st)
            dev.trsv_sweep_dev(work[2].data_ptr(), work[2].data_ptr(), nl + 3, lower, unit, st)
            st.synchronize()
            same(work[0].cpu().numpy(), exact[lower, unit])
            same(work[1].cpu().numpy(), swept[lower, unit, 2])
            same(work[2].cpu().numpy(), exact[lower, unit])
        same(bt.cpu().numpy(), b)

    # ---- a missing diagonal: refused by name, and the handle goes on solving with a unit diagonal ----
    if k["dropped"]:
        first = k["dropped"][0]
        assert first == sc.first_row_without_diagonal(pattern)
        for lower in (True, False):
            with pytest.raises(sp.Panic, match=rf"spal_{kind}_trsv: row {first} stores no diagonal entry"):
                dev.trsv(b, lower)                                  # (the row the host analysis found)
            for s in (0, 2):
                with pytest.raises(sp.Panic, match=rf"spal_{kind}_trsv_sweep: row {first} stores no diagonal entry"):
                    dev.trsv_sweep(b, s, lower)                     # (the row sweep_prepare's atomic min found)
        with pytest.raises(sp.Panic, match=rf"spal_{kind}_ilu0: row {first} stores no diagonal entry"):
            a.ilu0()
        for lower in (True, False):
            same(dev.trsv(b, lower, unit_diagonal=True), exact[lower, True])
            same(dev.trsv_sweep(b, 2, lower, unit_diagonal=True), swept[lower, True, 2])

    print(f"solver fuzz seed {seed}: n {n} {kind} {k['dtype'].name} levels {k['levels'][True]}/{k['levels'][False]} "
          f"{k['method']}/{k['prec']} maxit {k['maxit']} (reason, iterations) {outcome} "
          f"{time.perf_counter() - t_start:.2f} s")
