#!/usr/bin/env python3
"""Measures FSAI (spal_*_fsai_setup): what setup costs and how it splits, what an application costs beside
one SpMV of the matrix, and what CG preconditioned by it needs to solution -- for the patterns A, A @ A and (A @ A) @ A
-- beside the SAME run's plain CG, CG with AMG (default and alpha = 1.5) and CG with ilu0(sweeps=3) applied by three
sweeps per triangle; and MINRES with M = f beside M = None and Jacobi on Poisson 1000 x 1000.  One JSON record per case
under --out DIR.  Development tool, not part of the package, the tests or bench.py; no time in it is a pass criterion.

    python tools/bench_fsai.py --out profiles/fsai [--cases poisson2d_1000_f64,...] [--reps 5]

cases (generated in numpy; Dirichlet, diagonal 2 * dims, neighbours -1; right-hand side rng(0) standard normal):
    poisson2d_1000_{f64,f32}   the 5-point matrix on 1000 x 1000 (1M rows)
    poisson3d_100_{f64,f32}    the 7-point matrix on 100 x 100 x 100 (1M rows)
    laplace1d_1m_{f64,f32}     the 3-point matrix on 1M points
A record holds, per pattern,
  pattern_ms: the wall time of the product(s) that built the pattern (0 for A);
  setup:      describe() of the factor: setup_ms and its split into structure_ms, kernel_ms (device events around the
              factor kernel), transpose_ms and plan_ms; max_row, the rows of either kernel form, rejected; and the
              factor kernel's entries of G per second;
  apply_ms:   ms per application (device events around --reps applies after two warm-up ones: median, min, max) and
              spmv_ms, one product of `a` measured the same way;
  cg:         tol 1e-8, x0 = 0, at most 5000 iterations: iterations, reason, solve_ms (median of three; one run where
              the solve did not converge), and the time and iteration ratios against plain CG;
  cg_check_every_8: the same solve with the option "krylov_check_every" = 8, plain CG's default, where a preconditioned
              solve polls after every iteration by default; measured last, since the option cannot be unset;
and `baselines` (cg, cg_amg_default, cg_amg_alpha_1.5, cg_ilu0_sweeps3_precond_sweeps3) measured in the same run, and
for poisson2d_1000 `minres` at shift 0: M = None, Jacobi (M = diag |a_ii|, 0 sweeps) and every pattern's factor.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {f"{name}_{sfx}": (shape, dt) for name, shape in (("poisson2d_1000", (1000, 1000)), ("poisson3d_100", (100, 100, 100)),
                                                          ("laplace1d_1m", (1000000,)))
         for sfx, dt in (("f64", np.float64), ("f32", np.float32))}
PATTERNS = ["A", "A2", "A3"]
TOL, MAXIT = 1e-8, 5000


def stencil(shape, dtype):
    """(n, rowptr, colind, values) of the 3- / 5- / 7-point matrix, columns ascending"""
    idx = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(idx.size, 2.0 * len(shape))]
    for ax in range(len(shape)):
        lo = np.take(idx, np.arange(shape[ax] - 1), axis=ax).ravel()
        hi = np.take(idx, np.arange(1, shape[ax]), axis=ax).ravel()
        rows += [lo, hi]
        cols += [hi, lo]
        vals += [np.full(lo.size, -1.0)] * 2
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.argsort(rows * idx.size + cols, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=idx.size))]).astype(np.uint64)
    return idx.size, rowptr, cols[order].astype(np.uint64), vals[order].astype(dtype)


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "reps": len(v)}


def timed(torch, call, st, reps):
    ms = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        call()
        e1.record(st)
        e1.synchronize()
        if i >= 2:                      # two warm-up calls
            ms.append(e0.elapsed_time(e1))
    return spread(ms)


def solve(run, xt):
    ms, info = [], None
    for _ in range(3):
        xt.zero_()
        info = run()
        ms.append(info.solve_ms)
        if info.reason != 0:            # it ran into maxit or broke down: once is enough
            break
    return {"iterations": info.iterations, "reason": info.reason, "solve_ms": spread(ms),
            "relative_residual": float(np.sqrt(info.residual_sq / info.rhs_sq)) if info.rhs_sq else None}


def run_case(name, out_dir, reps):
    import torch
    import spalinalg_amd as sp
    shape, dtype = CASES[name]
    n, rowptr, colind, values = stencil(shape, dtype)
    a = sp.CsrMatrix._trusted(n, n, rowptr, colind, values)
    dev = a.device()
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    bt = torch.tensor(np.random.default_rng(0).standard_normal(n).astype(dtype)).cuda()
    xt = torch.zeros(n, dtype=tdt, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    b, x = bt.data_ptr(), xt.data_ptr()
    cg = lambda M: solve(lambda: dev.krylov_dev(b, x, "cg", M, TOL, MAXIT, st), xt)          # noqa: E731
    rec = {"case": name, "rows": n, "nnz": int(rowptr[-1]), "dtype": np.dtype(dtype).name, "tol": TOL, "maxit": MAXIT,
           "spmv_ms": timed(torch, lambda: dev.spmv_dev(b, x, st), st, reps), "patterns": {}, "baselines": {}}

    rec["baselines"]["cg"] = cg(None)
    for key, kw in (("cg_amg_default", {}), ("cg_amg_alpha_1.5", {"alpha": 1.5})):
        t0 = time.perf_counter()
        g = dev.amg(**kw)
        rec["baselines"][key] = {"setup_call_ms": (time.perf_counter() - t0) * 1e3, **cg(g)}
        g.close()
    ilu = dev.ilu0(sweeps=3)
    ilu.set_option("trsv_sweeps", 3)
    rec["baselines"]["cg_ilu0_sweeps3_precond_sweeps3"] = cg(ilu)
    ilu.close()
    plain = rec["baselines"]["cg"]

    minres = None
    if name.startswith("poisson2d_1000"):
        mres = lambda M: solve(lambda: dev.minres_dev(b, x, M, 0.0, TOL, MAXIT, st), xt)      # noqa: E731
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
        diag = np.abs(values[rows == colind.astype(np.int64)])
        jac = sp.CsrMatrix._trusted(n, n, np.arange(n + 1, dtype=np.uint64), np.arange(n, dtype=np.uint64), diag).device()
        jac.set_option("trsv_sweeps", 0)
        minres = {"shift": 0.0, "none": mres(None), "jacobi": mres(jac)}
        jac.close()

    pattern, built, factors = None, 0.0, {}
    for p in PATTERNS:
        if p != "A":
            t0 = time.perf_counter()
            nxt = dev.mul(dev) if pattern is None else pattern.mul(dev)
            built += (time.perf_counter() - t0) * 1e3
            if pattern is not None:
                pattern.close()
            pattern = nxt
        f = dev.fsai(pattern)
        d = f.describe()
        r = {"pattern_ms": built, "setup": d,
             "factor_entries_per_s": d["nnz"] / (d["kernel_ms"] * 1e-3) if d["kernel_ms"] > 0 else None,
             "apply_ms": timed(torch, lambda: f.apply_dev(b, x, st), st, reps), "cg": cg(f)}
        r["apply_over_spmv"] = r["apply_ms"]["median"] / rec["spmv_ms"]["median"]
        r["cg_vs_plain"] = {"time": r["cg"]["solve_ms"]["median"] / plain["solve_ms"]["median"],
                            "iterations": r["cg"]["iterations"] / max(plain["iterations"], 1),
                            "beats_plain_cg_in_time": bool(r["cg"]["reason"] == 0 and
                                                           r["cg"]["solve_ms"]["median"] < plain["solve_ms"]["median"])}
        if minres is not None:
            minres["fsai_" + p] = mres(f)
        rec["patterns"][p] = r
        factors[p] = f
        print(name, p, "max_row", d["max_row"], "setup", round(d["setup_ms"], 2), "ms (kernel", round(d["kernel_ms"], 3),
              ") apply", round(r["apply_ms"]["median"], 4), "ms | cg", r["cg"]["iterations"], "it",
              round(r["cg"]["solve_ms"]["median"], 2), "ms vs plain", plain["iterations"], "it",
              round(plain["solve_ms"]["median"], 2), "ms", flush=True)
    if pattern is not None:
        pattern.close()
    dev.set_option("krylov_check_every", 8)
    for p, f in factors.items():
        r = rec["patterns"][p]
        r["cg_check_every_8"] = cg(f)
        r["cg_check_every_8_vs_plain"] = {"time": r["cg_check_every_8"]["solve_ms"]["median"] / plain["solve_ms"]["median"],
                                          "beats_plain_cg_in_time": bool(r["cg_check_every_8"]["reason"] == 0 and
                                                                         r["cg_check_every_8"]["solve_ms"]["median"] <
                                                                         plain["solve_ms"]["median"])}
        f.close()
        print(name, p, "check_every 8: cg", r["cg_check_every_8"]["iterations"], "it",
              round(r["cg_check_every_8"]["solve_ms"]["median"], 2), "ms", flush=True)
    if minres is not None:
        rec["minres"] = minres
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"fsai_{name}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    print(name, "baselines", {k: (v["iterations"], round(v["solve_ms"]["median"], 2)) for k, v in rec["baselines"].items()},
          "minres", None if minres is None else {k: (v["iterations"], round(v["solve_ms"]["median"], 2))
                                                 for k, v in minres.items() if k != "shift"}, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    for name in args.cases.split(","):
        run_case(name, args.out, args.reps)


if __name__ == "__main__":
    main()
