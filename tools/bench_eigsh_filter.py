#!/usr/bin/env python3
"""Measures the Chebyshev filter on the device (spal_*_cheb_apply_*, spal_*_eigsh_filtered_*): ms per
recurrence step of the fused kernel against the pieces it replaces (the handle's spmv plus one elementwise pass of the
update's traffic), and time to solution of eigsh with and without the filter.  One JSON record per case under --out DIR.
Development tool, not part of the package, the tests or bench.py.

    python tools/bench_eigsh_filter.py --out DIR [--cases banded_1m_f64,...] [--part step|solve|all] [--tol 1e-8]

cases: those of tools/bench_eigsh.py -- banded_1m_{f64,f32} (14 draws per row in a window of 4096 plus the diagonal; NOT
symmetric, so its Ritz values are those of nothing in particular and Gershgorin's discs do not enclose a real spectrum)
and poisson2d_1000_{f64,f32} (the five-point Laplacian on a 1000 x 1000 grid, n = 1M).
step:  t(d) = device time of cheb_apply_dev at degree d; a step of the full form is (t(17) - t(1)) / 16, the first step
       is t(1).  Bytes a step must move: nnz * (sizeof(T) + 4) + 4 n for the matrix, 3 n sizeof(T) for y (gathered, read
       once), x and out.  Fractions are of the 8.0 TB/s HBM peak and of the copy ceiling measured in the same process.
       Against it: spmv_dev (the handle's plan; ANOTHER summation order, so not a substitute) and one torch.addcmul
       (three vectors read, one written: the traffic of the update, not its arithmetic).
solve: k = 6, tol = --tol (1e-8; an f32 residual cannot reach 1e-8 * scale, so f32 is also run at 1e-5), ncv = 20 and
       30, which = LA (and SA on the Poisson matrix): the plain call with maxit = 300 against the filtered call at
       d = 8, 16, 32 with the default warm-up; restarts, products, ms, reason.
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

CASES = ("banded_1m_f64", "banded_1m_f32", "poisson2d_1000_f64", "poisson2d_1000_f32")
HBM_PEAK_GBS = 8000.0
DEGREES = (8, 16, 32)


def step_part(dev, n, nnz, es, rec):
    import torch
    from tools.bench_trsv import timed
    st = torch.cuda.current_stream()
    tdt = torch.float64 if es == 8 else torch.float32
    xt = torch.rand(n, dtype=tdt, device="cuda")
    yt = torch.rand(n, dtype=tdt, device="cuda")
    ot = torch.empty_like(xt)
    big = torch.empty(32 * 1024 * 1024, dtype=torch.float64, device="cuda")
    big2 = torch.empty_like(big)
    torch.cuda.synchronize()
    copy = timed(lambda: big2.copy_(big), 10, 3)
    ceiling = 2 * big.numel() * 8 / (copy["median"] * 1e-3) / 1e9
    del big, big2
    glo, ghi = dev.gershgorin()
    lo, hi, a0 = glo, glo + 0.9 * (ghi - glo), ghi
    t1 = timed(lambda: dev.cheb_apply_dev(xt.data_ptr(), ot.data_ptr(), 1, lo, hi, a0, st), 20, 5)
    t17 = timed(lambda: dev.cheb_apply_dev(xt.data_ptr(), ot.data_ptr(), 17, lo, hi, a0, st), 5, 2)
    spmv = timed(lambda: dev.spmv_dev(xt.data_ptr(), ot.data_ptr(), st), 20, 5)
    update = timed(lambda: torch.addcmul(xt, yt, ot, value=0.5, out=ot), 20, 5)
    step = (t17["median"] - t1["median"]) / 16
    byts = nnz * (es + 4) + 4 * n + 3 * n * es
    rec["step"] = {"gershgorin": [glo, ghi], "first_step_ms": t1, "degree17_ms": t17, "step_ms": step, "bytes": byts,
                   "bytes_per_row": byts / n, "gbs": byts / (step * 1e-3) / 1e9,
                   "fraction_of_hbm_peak": byts / (step * 1e-3) / 1e9 / HBM_PEAK_GBS, "copy_ceiling_gbs": ceiling,
                   "fraction_of_copy_ceiling": byts / (step * 1e-3) / 1e9 / ceiling, "spmv_ms": spmv, "update_ms": update,
                   "spmv_plus_update_ms": spmv["median"] + update["median"],
                   "step_over_spmv_plus_update": step / (spmv["median"] + update["median"]),
                   "chunk": dev.describe().get("eigsh_filter", {}).get("chunk", 0)}


def solve_part(dev, name, rec, tol):
    k = 6
    rec["tol"] = tol
    rec["solve"] = []
    for which in (("LA", "SA") if name.startswith("poisson") else ("LA",)):
        for ncv in (20, 30):
            theta, _, info = dev.eigsh(k, which, ncv, tol=tol, maxit=300, return_eigenvectors=False)
            rec["solve"].append({"which": which, "ncv": ncv, "degree": 0, "solve_ms": info.solve_ms, "restarts": info.restarts,
                                 "products": info.products, "converged": info.converged, "reason": info.reason,
                                 "theta": [float(t) for t in theta]})
            for d in DEGREES:
                theta, _, info = dev.eigsh(k, which, ncv, tol=tol, maxit=300, return_eigenvectors=False, filter_degree=d)
                rec["solve"].append({"which": which, "ncv": ncv, "degree": d, "solve_ms": info.solve_ms, "restarts": info.restarts,
                                     "products": info.products, "warm_restarts": info.warm_restarts,
                                     "warm_products": info.warm_products, "lo": info.lo, "hi": info.hi, "a0": info.a0,
                                     "converged": info.converged, "reason": info.reason, "theta": [float(t) for t in theta],
                                     "resid": [float(r) for r in info.resid],
                                     "residual_ms": dev.describe()["eigsh_filter"]["residual_ms"]})
            print(json.dumps(rec["solve"][-4:]), flush=True)


def child(name, out_dir, part, tol):
    import spalinalg_amd as sp
    from tools.bench_eigsh import make
    n, rp, ci, va = make(name)
    es = va.dtype.itemsize
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": int(rp[-1])}
    if part in ("step", "all"):
        step_part(dev, n, int(rp[-1]), es, rec)
        print(json.dumps(rec["step"]), flush=True)
    if part in ("solve", "all"):
        solve_part(dev, name, rec, tol)
    tag = "" if tol == 1e-8 else f"_tol{tol:g}"
    with open(os.path.join(out_dir, f"eigsh_filter_{part}_{name}{tag}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--part", default="all", choices=("step", "solve", "all"))
    ap.add_argument("--tol", type=float, default=1e-8, help="tolerance of the solve part")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        child(args.child, args.out, args.part, args.tol)
        return
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, "--part", args.part,
               "--tol", repr(args.tol)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
