#!/usr/bin/env python3
"""Measures the multicolour reordering (spal_*_multicolour) and the trade it makes against the natural
order: fewer levels and faster exact triangular solves, against a weaker ILU(0) (more iterations) and an SpMV on a matrix
that has lost its band.  One JSON record per case under --out DIR.  Development tool, not part of the package, the tests
or bench.py; no time in it is a pass criterion.

    python tools/bench_colour.py --out profiles/colour [--cases banded_1m_f64,...] [--iters 10] [--warmup 2]

cases (the inputs of tools/bench_krylov.py and tools/bench_trsv.py):
    banded_1m_{f64,f32}      1M x 1M, 14 draws per row in a window of 4096 around the diagonal, plus the diagonal
    power_law_{f64,f32}      300k rows, power-law row lengths up to 5000, columns near the rows
    anywhere_1m_{f64,f32}    1M x 1M, 7 draws per row anywhere in the row's 1M columns, plus the diagonal
Every case runs in a child process of its own under a time limit; the parent stops at the first child that does not end
normally.  A record holds: colours, rounds, colouring and permute ms (device events, from describe()["ordering"]) and the
wall time of the call; for A and for P A P^T the levels of both triangles, ms per exact solve of each, ILU(0) kernel
ms and SpMV ms (device events around --iters launches after --warmup, three repetitions: median, min, max); and for
BiCGStab and GMRES(30) the iterations, the reason and the total ms of a solve at one tolerance (1e-8 for f64, 1e-5 for
f32, at most 500 iterations; the median of three solves) preconditioned by exact ILU(0) in natural order, by three Jacobi
sweeps per triangle in natural order, and by exact ILU(0) in multicolour order.  x of the multicolour solve, taken back
to the natural order, is checked against the original A in float64 on the host.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_trsv import timed  # noqa: E402

CASES = ("banded_1m_f64", "banded_1m_f32", "power_law_f64", "power_law_f32", "anywhere_1m_f64", "anywhere_1m_f32")
MAXIT = 500
SWEEPS = 3


def make_case(name):
    from tools import bench_krylov, bench_trsv
    return bench_trsv.make_case(name) if name.startswith("power_law") else bench_krylov.make_case(name)


def side(dev, bt, xt, yt, st, iters, warmup):
    """What one ordering costs: levels and ms of both exact solves, ILU(0), one SpMV.  Returns (record, factor handle)."""
    rec = {"spmv_ms": timed(lambda: dev.spmv_dev(bt.data_ptr(), yt.data_ptr(), st), max(iters, 20), warmup + 3),
           "spmv_plan": dev.describe().get("kernel")}
    for lower, key in ((True, "lower"), (False, "upper")):
        plan = dev.trsv_analyse(lower=lower, stream=st)[key]
        rec[key] = {"levels": plan["levels"], "launches": plan["launches"], "analysis_ms": plan["analysis_ms"],
                    "trsv_ms": timed(lambda: dev.trsv_dev(bt.data_ptr(), xt.data_ptr(), lower, False, st), iters, warmup)}
    factors = [dev.ilu0(st) for _ in range(3)]
    kernel = sorted(f.describe()["ilu0"]["kernel_ms"] for f in factors)
    rec["ilu0_kernel_ms"] = {"median": kernel[1], "min": kernel[0], "max": kernel[2], "reps": 3}
    return rec, factors[0]


def solves(dev, factor, sweeps, bt, xt, tol, st):
    """{method: iterations, reason, total ms (median of three solves from x0 = 0)} with `factor` applied exactly
    (sweeps = -1) or by Jacobi sweeps."""
    import numpy as np
    factor.set_option("trsv_sweeps", sweeps)
    out = {}
    for method in ("bicgstab", "gmres30"):
        ms, info = [], None
        for _ in range(3):
            xt.zero_()
            if method == "bicgstab":
                info = dev.krylov_dev(bt.data_ptr(), xt.data_ptr(), "bicgstab", factor, tol, MAXIT, st)
            else:
                info = dev.gmres_dev(bt.data_ptr(), xt.data_ptr(), factor, 30, tol, MAXIT, st)
            ms.append(info.solve_ms)
        out[method] = {"iterations": info.iterations, "reason": info.reason,
                       "total_ms": {"median": float(np.median(ms)), "min": min(ms), "max": max(ms), "reps": 3},
                       "relative_residual": float(np.sqrt(info.residual_sq / info.rhs_sq)) if info.rhs_sq else None}
    factor.set_option("trsv_sweeps", -1)
    return out


def child(name, out_dir, iters, warmup):
    import numpy as np
    import torch
    import spalinalg_amd as sp
    n, rp, ci, va = make_case(name)
    es = va.dtype.itemsize
    tol = 1e-8 if es == 8 else 1e-5
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    st = torch.cuda.current_stream()
    tdt = torch.float64 if es == 8 else torch.float32
    gen = torch.Generator(device="cuda").manual_seed(7)
    bt = torch.rand(n, dtype=tdt, device="cuda", generator=gen) * 2 - 1
    xt, yt, bp = torch.empty_like(bt), torch.empty_like(bt), torch.empty_like(bt)
    torch.cuda.synchronize()
    calls = []
    for _ in range(3):
        t0 = time.perf_counter()
        p = dev.multicolour(0, st)
        calls.append((time.perf_counter() - t0) * 1e3)
    order = p.describe()["ordering"]
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": int(rp[-1]), "iters": iters, "warmup": warmup, "tol": tol,
           "maxit": MAXIT, "colours": order["colours"], "rounds": order["rounds"], "colour_ms": order["colour_ms"],
           "permute_ms": order["permute_ms"],
           "multicolour_call_ms": {"median": float(np.median(calls)), "min": min(calls), "max": max(calls), "reps": 3}}
    rec["natural"], f_nat = side(dev, bt, xt, yt, st, iters, warmup)
    rec["multicolour"], f_mc = side(p, bt, xt, yt, st, iters, warmup)
    rec["solve"] = {"natural_exact": solves(dev, f_nat, -1, bt, xt, tol, st),
                    f"natural_sweeps_{SWEEPS}": solves(dev, f_nat, SWEEPS, bt, xt, tol, st)}
    p.permute_vec_dev(bt.data_ptr(), bp.data_ptr(), False, st)
    rec["solve"]["multicolour_exact"] = solves(p, f_mc, -1, bp, xt, tol, st)
    # the last multicolour solve (GMRES), back in the natural order, against the original A on the host
    p.permute_vec_dev(xt.data_ptr(), yt.data_ptr(), True, st)
    torch.cuda.synchronize()
    x, b = yt.cpu().numpy().astype(np.float64), bt.cpu().numpy().astype(np.float64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
    ax = np.bincount(rows, weights=va.astype(np.float64) * x[ci.astype(np.int64)], minlength=n)
    rec["multicolour_solution_relative_residual_on_a"] = float(np.linalg.norm(b - ax) / np.linalg.norm(b))
    with open(os.path.join(out_dir, f"colour_{name}.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        child(args.child, args.out, args.iters, args.warmup)
        return
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, "--iters", str(args.iters),
               "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
