#!/usr/bin/env python3
"""Measures MINRES on the device (spal_csr_minres_dev_*, spal_csr_minres_block_dev_*).  One JSON record per
case under --out DIR.  Development tool, not part of the package, the tests or bench.py.

    python tools/bench_minres.py --out DIR [--cases banded_1m_f64,...] [--iters 64] [--reps 3] [--ks 1,2,4,8,16,32]

cases:
    banded_1m_{f64,f32}        tools/bench_krylov.py's matrix: 14 draws per row in a window of 4096, plus the diagonal
    poisson2d_1000_{f64,f32}   the 5-point Laplacian on a 1000 x 1000 grid (symmetric positive definite, spectrum in (0, 8))
Per case, with a FIXED number of iterations (tol = 0, so the device never stops early and no launch is frozen; the time
of an iteration does not depend on whether the matrix is symmetric):
    minres / cg                ms per iteration of MINRES and of CG on the same handle, without a preconditioner (median,
                               min, max of --reps solves), and their ratio
    spmv_ms                    one product on the same handle
    python_loop                the same MINRES loop driven from Python: spmv_dev for the product, torch for vectors and
                               dots (each dot comes back to the host, as a caller without device scalars has it)
    block                      for k in --ks: ms per iteration of the block call against k vector calls
On the Poisson cases also `indefinite`: shift = 4 (mid-spectrum), tol = 1e-8, maxit = --solve-maxit: iterations, reason
and solve_ms of MINRES against GMRES(30) and BiCGStab on A - 4 I assembled as a matrix of its own.
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

from tools.bench_krylov import make_case as krylov_case, spread  # noqa: E402
from tools.bench_trsv import timed  # noqa: E402

CASES = ("banded_1m_f64", "banded_1m_f32", "poisson2d_1000_f64", "poisson2d_1000_f32")


def poisson2d(g, dt, shift=0.0):
    """(n, rowptr, colind, values) of the 5-point Laplacian on a g x g grid, minus shift on the diagonal."""
    import numpy as np
    n = g * g
    idx = np.arange(n, dtype=np.int64)
    i, j = idx // g, idx % g
    cols = np.stack([idx - g, idx - 1, idx, idx + 1, idx + g], axis=1)
    keep = np.stack([i > 0, j > 0, np.ones(n, bool), j < g - 1, i < g - 1], axis=1)
    vals = np.broadcast_to(np.array([-1, -1, 4 - shift, -1, -1], dtype=dt), (n, 5))
    rowptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.uint64)
    return n, rowptr, cols[keep].astype(np.uint64), np.ascontiguousarray(vals[keep])


def make_case(name):
    import numpy as np
    kind, t = name.rsplit("_", 1)
    if kind == "poisson2d_1000":
        return poisson2d(1000, np.float64 if t == "f64" else np.float32)
    return krylov_case(name)


def per_iteration(solve, reps):
    per, info = [], None
    for _ in range(reps):
        info = solve()
        per.append(info.solve_ms / max(info.iterations, 1))
    return {"ms_per_iteration": spread(per), "iterations": info.iterations, "reason": info.reason,
            "stopped_early": info.reason != 1}


def python_loop_ms(dev, bt, iters, st):
    """The MINRES text driven from Python, unpreconditioned and unshifted."""
    import math
    import torch

    def mul(v, out):
        dev.spmv_dev(v.data_ptr(), out.data_ptr(), st)
        return out

    x = torch.zeros_like(bt)
    bufs = [torch.zeros_like(bt) for _ in range(3)]
    w, w2 = torch.zeros_like(bt), torch.zeros_like(bt)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(st)
    r1, r2, t = bufs
    r2.copy_(bt).sub_(mul(x, t))
    beta = math.sqrt(torch.dot(r2, r2).item())
    phibar, oldb, dbar, epsln, cs, sn = beta, 0.0, 0.0, 0.0, -1.0, 0.0
    v = r2 / beta
    for it in range(iters):
        mul(v, t)
        if it:
            t.sub_(r1, alpha=beta / oldb)
        alfa = torch.dot(v, t).item()
        t.sub_(r2, alpha=alfa / beta)
        r1, r2, t = r2, t, r1
        oldb, beta = beta, math.sqrt(torch.dot(r2, r2).item())
        oldeps, delta, gbar = epsln, cs * dbar + sn * alfa, sn * dbar - cs * alfa
        epsln, dbar = sn * beta, -cs * beta
        gamma = math.sqrt(gbar * gbar + beta * beta)
        cs, sn = gbar / gamma, beta / gamma
        phi, phibar = cs * phibar, sn * phibar
        w2.mul_(-oldeps).add_(v).sub_(w, alpha=delta).div_(gamma)      # over w1, as the device does
        w, w2 = w2, w
        x.add_(w, alpha=phi)
        torch.mul(r2, 1.0 / beta, out=v)
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def child(name, out_dir, iters, reps, ks, solve_maxit):
    import numpy as np
    import torch
    import spalinalg_amd as sp
    n, rp, ci, va = make_case(name)
    es = va.dtype.itemsize
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    st = torch.cuda.current_stream()
    tdt = torch.float64 if es == 8 else torch.float32
    gen = torch.Generator(device="cuda").manual_seed(7)
    bt = torch.rand(n, dtype=tdt, device="cuda", generator=gen) * 2 - 1
    xt = torch.empty_like(bt)
    torch.cuda.synchronize()
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": int(rp[-1]), "iterations_timed": iters,
           "spmv_ms": timed(lambda: dev.spmv_dev(bt.data_ptr(), xt.data_ptr(), st), 20, 5)}

    def minres():
        xt.zero_()
        return dev.minres_dev(bt.data_ptr(), xt.data_ptr(), None, 0.0, 0.0, iters, st)

    def cg():
        xt.zero_()
        return dev.krylov_dev(bt.data_ptr(), xt.data_ptr(), "cg", None, 0.0, iters, st)

    rec["minres"] = per_iteration(minres, reps)
    rec["cg"] = per_iteration(cg, reps)
    rec["minres_over_cg"] = rec["minres"]["ms_per_iteration"]["median"] / rec["cg"]["ms_per_iteration"]["median"]
    vec_ms = rec["minres"]["ms_per_iteration"]["median"] - rec["spmv_ms"]["median"]
    rec["minres_vector_kernels"] = {"bytes_per_iteration": 15 * n * es, "ms_per_iteration": vec_ms,
                                    "gbs": 15 * n * es / (vec_ms * 1e-3) / 1e9 if vec_ms > 0 else None}
    rec["python_loop_ms_per_iteration"] = python_loop_ms(dev, bt, iters, st)
    rec["block"] = {}
    for k in ks:
        Bt = torch.rand((n, k), dtype=tdt, device="cuda", generator=gen) * 2 - 1
        Xt = torch.empty_like(Bt)

        def block():
            Xt.zero_()
            return dev.minres_block_dev(k, Bt.data_ptr(), k, Xt.data_ptr(), k, None, 0.0, 0.0, iters, st)[0]

        r = per_iteration(block, reps)
        r["k_vector_calls_ms_per_iteration"] = k * rec["minres"]["ms_per_iteration"]["median"]
        r["gain"] = r["k_vector_calls_ms_per_iteration"] / r["ms_per_iteration"]["median"]
        rec["block"][str(k)] = r
        del Bt, Xt
    if name.startswith("poisson2d"):
        shift = 4.0
        sn, srp, sci, sva = poisson2d(1000, va.dtype.type, shift)
        shifted = sp.CsrMatrix(sn, sn, srp, sci, sva).device()
        runs = {}
        for label, solve in (
                ("minres", lambda: dev.minres_dev(bt.data_ptr(), xt.data_ptr(), None, shift, 1e-8, solve_maxit, st)),
                ("gmres30", lambda: shifted.gmres_dev(bt.data_ptr(), xt.data_ptr(), None, 30, 1e-8, solve_maxit, st)),
                ("bicgstab", lambda: shifted.krylov_dev(bt.data_ptr(), xt.data_ptr(), "bicgstab", None, 1e-8, solve_maxit, st))):
            xt.zero_()
            info = solve()
            runs[label] = {"iterations": info.iterations, "reason": info.reason, "solve_ms": info.solve_ms,
                           "residual_sq_over_rhs_sq": info.residual_sq / info.rhs_sq if info.rhs_sq else None}
        rec["indefinite"] = {"shift": shift, "tol": 1e-8, "maxit": solve_maxit, **runs}
    assert np.isfinite(rec["minres"]["ms_per_iteration"]["median"])
    with open(os.path.join(out_dir, f"minres_{name}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--solve-maxit", type=int, default=20000)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    ks = [int(x) for x in args.ks.split(",") if x]
    if args.child:
        child(args.child, args.out, args.iters, args.reps, ks, args.solve_maxit)
        return
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, "--iters", str(args.iters),
               "--reps", str(args.reps), "--ks", args.ks, "--solve-maxit", str(args.solve_maxit)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
