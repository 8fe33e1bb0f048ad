#!/usr/bin/env python3
"""Measures the Jacobi sweeps on a triangle (spal_csr_trsv_sweep_dev_*) and what they do to a preconditioned
solve.  One JSON record per case under --out DIR.  Development tool, not part of the package, the tests or bench.py.

    python tools/bench_sweep.py --out DIR [--cases banded_1m_f64,banded_1m_f32] [--sweeps -1,0,1,2,3,5] [--every 1,8]
                                [--iters 20] [--reps 3]

cases:
    banded_1m_{f64,f32}   1M x 1M, about 14 entries per row in a window of 4096 around the diagonal, plus the diagonal
Two matrices per case, both with a unit diagonal: the unsymmetric one of tools/bench_krylov.py (off-diagonal values in
(-1/16, 1/16); BiCGStab), and a symmetric one -- seven draws per row and their transposes, (i, j) and (j, i) sharing a
value in (-1/32, 1/32), up to some 30 per row -- which is positive definite by dominance (CG).  Per case the record holds
  * on the ILU(0) factor of the unsymmetric matrix, per triangle: ms per call of the sweep for s = 0, 1, 2, 3, 5 and the
    ms per PASS they imply (the slope from s = 1 to s = 5: x0 and the launch of the call drop out), beside one SpMV on the
    same handle and one exact solve of the same triangle; prepare_ms of the handle;
  * per method (CG on the symmetric matrix, BiCGStab on the unsymmetric one, each with its own ILU(0) factor), per
    "krylov_check_every" of --every and per "trsv_sweeps" of --sweeps (-1: exact solves): iterations, reason, total ms
    (solve_ms: device time of the call, median of --reps) and ms per iteration, at tol 1e-8 (f64) / 1e-5 (f32).
Every case runs in a child process of its own under a time limit; the parent stops at the first child that does not end
normally.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_krylov import make_case as unsymmetric_case, spread  # noqa: E402
from tools.bench_trsv import timed  # noqa: E402

CASES = ("banded_1m_f64", "banded_1m_f32")
PASS_SWEEPS = (0, 1, 2, 3, 5)


def symmetric_case(name):
    """Structurally and numerically symmetric, unit diagonal, off-diagonal sum below 1 in every row."""
    import numpy as np
    dt = np.float64 if name.endswith("f64") else np.float32
    n = 1_000_000
    rng = np.random.default_rng(67)
    i = np.repeat(np.arange(n, dtype=np.int64), 7)
    j = i + rng.integers(-2048, 2048, size=i.size)
    keep = (j >= 0) & (j < n) & (j != i)                                # draws past the border are dropped, not piled onto it
    lo, hi = np.minimum(i, j)[keep], np.maximum(i, j)[keep]
    pair = np.unique(lo * n + hi)
    lo, hi = pair // n, pair % n
    d = np.arange(n, dtype=np.int64)
    v = rng.uniform(-1, 1, size=pair.size) / 32.0                       # one value per unordered pair
    rows, cols, vals = np.concatenate([lo, hi, d]), np.concatenate([hi, lo, d]), np.concatenate([v, v, np.ones(n)])
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.uint64)
    off = np.bincount(rows[rows != cols], weights=np.abs(vals[rows != cols]), minlength=n)
    assert off.max() < 1.0, "not dominant"
    return n, rp, cols.astype(np.uint64), vals.astype(dt)


def passes(f, bt, xt, st, iters):
    """Per triangle of the factor handle f: ms per sweep call by s, ms per pass, one exact solve."""
    out = {}
    for lower, unit, key in ((True, True, "lower"), (False, False, "upper")):
        call = {str(s): timed(lambda: f.trsv_sweep_dev(bt.data_ptr(), xt.data_ptr(), s, lower, unit, st), iters, 3)
                for s in PASS_SWEEPS}
        per_pass = (call["5"]["median"] - call["1"]["median"]) / 4
        f.trsv_analyse(lower, unit)
        exact = timed(lambda: f.trsv_dev(bt.data_ptr(), xt.data_ptr(), lower, unit, st), 3, 1)
        out[key] = {"sweep_call_ms": call, "ms_per_pass": per_pass, "exact_solve_ms": exact,
                    "exact_analysis_ms": f.describe()["trsv"][key]["analysis_ms"]}
    return out


def solves(a, method, bt, xt, st, tol, maxit, sweeps_list, every_list, reps):
    """{check_every: {trsv_sweeps: iterations, reason, total ms, ms per iteration}} with a fresh factor per option value,
    so that the exact solves' analysis is paid where it is used and nowhere else."""
    out = {}
    for every in every_list:
        a.set_option("krylov_check_every", every)
        row = {}
        for s in sweeps_list:
            m = a.ilu0()
            m.set_option("trsv_sweeps", s)
            first, total, info = None, [], None
            for r in range(reps + 1):
                xt.zero_()
                info = a.krylov_dev(bt.data_ptr(), xt.data_ptr(), method, M=m, tol=tol, maxit=maxit, stream=st)
                if r == 0:
                    first = info.solve_ms           # includes the preparation or the two analyses
                else:
                    total.append(info.solve_ms)
            row[str(s)] = {"iterations": info.iterations, "reason": info.reason, "total_ms": spread(total),
                           "first_call_ms": first,
                           "ms_per_iteration": spread([t / max(info.iterations, 1) for t in total]),
                           "polls": a.describe()["krylov"]["polls"]}
            m.close()
        out[str(every)] = row
    return out


def child(name, out_dir, sweeps_list, every_list, iters, reps):
    import numpy as np
    import torch
    import spalinalg_amd as sp
    es = 8 if name.endswith("f64") else 4
    tol, maxit = (1e-8, 500) if es == 8 else (1e-5, 500)
    tdt = torch.float64 if es == 8 else torch.float32
    st = torch.cuda.current_stream()
    n, rp, ci, va = unsymmetric_case(name)
    bt = torch.rand(n, dtype=tdt, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) * 2 - 1
    xt = torch.empty_like(bt)
    torch.cuda.synchronize()
    a = sp.CsrMatrix(n, n, rp, ci, va).device()
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": int(rp[-1]), "iters": iters, "reps": reps, "tol": tol}
    f = a.ilu0()
    rec["factor_spmv_ms"] = timed(lambda: f.spmv_dev(bt.data_ptr(), xt.data_ptr(), st), 20, 5)
    rec["matrix_spmv_ms"] = timed(lambda: a.spmv_dev(bt.data_ptr(), xt.data_ptr(), st), 20, 5)
    rec["triangles"] = passes(f, bt, xt, st, iters)
    rec["trsv_sweep"] = f.describe()["trsv_sweep"]
    for key, tri in rec["triangles"].items():
        tri["pass_over_factor_spmv"] = tri["ms_per_pass"] / rec["factor_spmv_ms"]["median"]
    f.close()
    rec["bicgstab"] = solves(a, "bicgstab", bt, xt, st, tol, maxit, sweeps_list, every_list, reps)
    a.close()
    n, rp, ci, va = symmetric_case(name)
    spd = sp.CsrMatrix(n, n, rp, ci, va).device()
    rec["cg_nnz"] = int(rp[-1])
    rec["cg_spmv_ms"] = timed(lambda: spd.spmv_dev(bt.data_ptr(), xt.data_ptr(), st), 20, 5)
    rec["cg"] = solves(spd, "cg", bt, xt, st, tol, maxit, sweeps_list, every_list, reps)
    assert np.isfinite(xt.cpu().numpy()).all()
    with open(os.path.join(out_dir, f"sweep_{name}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--sweeps", default="-1,0,1,2,3,5")
    ap.add_argument("--every", default="1,8")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        child(args.child, args.out, [int(x) for x in args.sweeps.split(",")], [int(x) for x in args.every.split(",")],
              args.iters, args.reps)
        return
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, f"--sweeps={args.sweeps}",
               "--every", args.every, "--iters", str(args.iters), "--reps", str(args.reps)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
