#!/usr/bin/env python3
"""Measures the aggregation AMG (spal_*_amg_setup) on the classic hard problem: what setup costs per level,
what a cycle costs (with the single-workgroup tail on and off), and what CG preconditioned by the cycle needs to
solution, beside CG without a preconditioner and CG with ilu0(sweeps=3) applied by three sweeps per triangle on the same
inputs.  One JSON record per case under --out DIR, and the sweep over "amg_tail_rows" as tail_sweep_<case>.json beside
them.  Development tool, not part of the package, the tests or bench.py; no time in it is a pass criterion.

    python tools/bench_amg.py --out profiles/amg [--cases poisson2d_1000_f64,...] [--reps 5]

cases (generated in numpy; Dirichlet, diagonal 2 * dims, neighbours -1; right-hand side rng(0) standard normal):
    poisson2d_1000_{f64,f32}   the 5-point matrix on 1000 x 1000 (1M rows)
    poisson3d_100_{f64,f32}    the 7-point matrix on 100 x 100 x 100 (1M rows)
A record holds
  setup:     the levels' rows, nnz, aggregates, rounds and setup_ms as describe() reports them, and the call's wall time;
  cycles:    for V and W, alpha 1 and 1.5: ms per cycle (device events around --reps applies: median, min, max) with the
             tail at its default and off, the tail's first level, and the smoother's share per level: 2 nu sweeps on A_l
             alone (a one-level hierarchy of level(l)), which is what a V cycle smooths there;
  solves:    tol 1e-8, x0 = 0, at most 5000 iterations: iterations, reason and solve_ms (median of three; one run where
             the solve did not converge) of CG with every cycle variant, of CG
             alone and of CG with ilu0(sweeps=3), precond_sweeps=3; the ratios of the AMG solves against those two;
  tail:      ms per V and W cycle for amg_tail_rows in 0, 256, 512, 1024, 2048, 4096 (the clamp).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"poisson2d_1000_f64": ((1000, 1000), np.float64), "poisson2d_1000_f32": ((1000, 1000), np.float32),
         "poisson3d_100_f64": ((100, 100, 100), np.float64), "poisson3d_100_f32": ((100, 100, 100), np.float32)}
VARIANTS = [("v", 1.0), ("v", 1.5), ("w", 1.0), ("w", 1.5)]
TAIL_ROWS = [0, 256, 512, 1024, 2048, 4096]
TOL, MAXIT = 1e-8, 5000


def stencil(shape, dtype):
    """(n, rowptr, colind, values) of the 5- / 7-point matrix, columns ascending"""
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


def cycle_ms(torch, g, bt, xt, st, reps):
    ms = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        g.apply_dev(bt.data_ptr(), xt.data_ptr(), st)
        e1.record(st)
        e1.synchronize()
        if i >= 2:                      # two warm-up applies
            ms.append(e0.elapsed_time(e1))
    return spread(ms)


def solve(torch, dev, M, bt, xt, st):
    ms, info = [], None
    for _ in range(3):
        xt.zero_()
        info = dev.krylov_dev(bt.data_ptr(), xt.data_ptr(), "cg", M, TOL, MAXIT, st)
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
    rec = {"case": name, "rows": n, "nnz": int(rowptr[-1]), "dtype": np.dtype(dtype).name, "tol": TOL, "maxit": MAXIT,
           "cycles": {}, "solves": {}}

    t0 = time.perf_counter()
    g = dev.amg()
    d = g.describe()
    rec["setup"] = {"call_ms": (time.perf_counter() - t0) * 1e3, **{k: d[k] for k in
                    ("levels", "rows", "nnz", "aggregates", "rounds", "setup_ms", "stopped_by", "tail_rows", "tail_from_level")}}
    nu = d["params"]["nu"]
    smoother = []
    for l in range(d["levels"]):        # 2 nu damped Jacobi sweeps on A_l alone: the smoother's share of a V cycle there
        al = g.level(l).device()
        one = al.amg(max_levels=1, coarse_sweeps=2 * nu)
        one.set_option("amg_tail_rows", 0)
        rows = d["rows"][l]
        b_l, x_l = torch.ones(rows, dtype=tdt, device="cuda"), torch.zeros(rows, dtype=tdt, device="cuda")
        smoother.append(cycle_ms(torch, one, b_l, x_l, st, reps)["median"])
        one.close()
        al.close()
    rec["setup"]["smoother_ms_per_level"] = smoother
    g.close()

    for cyc, alpha in VARIANTS:
        key = f"{cyc}_alpha_{alpha}"
        g = dev.amg(cycle=cyc, alpha=alpha)
        default = g.describe()["tail_rows"]
        on = cycle_ms(torch, g, bt, xt, st, reps)
        g.set_option("amg_tail_rows", 0)
        off = cycle_ms(torch, g, bt, xt, st, reps)
        g.set_option("amg_tail_rows", default)
        rec["cycles"][key] = {"ms_tail_default": on, "ms_tail_off": off, "tail_from_level": g.describe()["tail_from_level"]}
        rec["solves"]["cg_amg_" + key] = solve(torch, dev, g, bt, xt, st)
        if alpha == 1.0:
            sweep = {}
            for rows in TAIL_ROWS:
                g.set_option("amg_tail_rows", rows)
                sweep[str(rows)] = {"ms": cycle_ms(torch, g, bt, xt, st, reps), "tail_from_level": g.describe()["tail_from_level"]}
            rec.setdefault("tail", {})[cyc] = sweep
        g.close()

    rec["solves"]["cg"] = solve(torch, dev, None, bt, xt, st)
    f = dev.ilu0(sweeps=3)
    f.set_option("trsv_sweeps", 3)
    rec["solves"]["cg_ilu0_sweeps3_precond_sweeps3"] = solve(torch, dev, f, bt, xt, st)
    for base in ("cg", "cg_ilu0_sweeps3_precond_sweeps3"):
        t = rec["solves"][base]["solve_ms"]["median"]
        rec.setdefault("ratios", {})[base] = {k: {"time": v["solve_ms"]["median"] / t, "iterations": v["iterations"] /
                                                   max(rec["solves"][base]["iterations"], 1)}
                                              for k, v in rec["solves"].items() if k.startswith("cg_amg_")}
    os.makedirs(out_dir, exist_ok=True)
    tail = rec.pop("tail")
    with open(os.path.join(out_dir, f"amg_{name}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    with open(os.path.join(out_dir, f"tail_sweep_{name}.json"), "w") as fh:
        json.dump({"case": name, "rows_per_level": rec["setup"]["rows"], "ms_per_cycle_by_amg_tail_rows": tail}, fh, indent=1)
    s = rec["solves"]
    print(name, "levels", rec["setup"]["rows"], "| cg", s["cg"]["iterations"], "it", round(s["cg"]["solve_ms"]["median"], 1), "ms",
          "| ilu", s["cg_ilu0_sweeps3_precond_sweeps3"]["iterations"], "it",
          round(s["cg_ilu0_sweeps3_precond_sweeps3"]["solve_ms"]["median"], 1), "ms",
          "|", {k[7:]: (v["iterations"], round(v["solve_ms"]["median"], 1)) for k, v in s.items() if k.startswith("cg_amg_")},
          flush=True)


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
