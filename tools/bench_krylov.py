#!/usr/bin/env python3
"""Measures the Krylov solvers on the device (spal_csr_krylov_dev_*): ms per iteration of CG without a preconditioner
and of BiCGStab with the ILU(0) factor, over a sweep of "krylov_check_every", beside two baselines -- the parts (one SpMV
on the same handle plus two solves on the factor) and what a caller could do before: the same loop driven from Python
with spmv_dev / trsv_dev and torch vector operations.  One JSON record per case under --out DIR.  Development tool, not
part of the package, the tests or bench.py.

    python tools/bench_krylov.py --out DIR [--cases banded_1m_f64,...] [--every 1,2,4,8,16,32] [--cg-iters 64]
                                 [--bicg-iters 4] [--reps 3]

cases:
    banded_{1m,10m}_{f64,f32}   14 draws per row in a window of 4096 around the diagonal, plus the diagonal
    anywhere_1m_{f64,f32}       1M x 1M, 7 draws per row anywhere in the row's 1M columns, plus the diagonal
Off-diagonal values are uniform in (-1/16, 1/16) and the diagonal is 1.  Every solve runs a FIXED number of iterations
(tol = 0, so the device never stops early and no launch is frozen): the time of an iteration does not depend on whether
the matrix is symmetric, so CG is timed on the same matrices; a record whose reason is not 1 (maxit) is marked.
Per case: spmv_ms, the two solves on the factor, the copy ceiling (a device-to-device copy of 256 MB, bytes read plus
bytes written over its time), and per method {check_every: ms per iteration (median, min, max of --reps solves), polls};
for unpreconditioned CG also the vector kernels' share: (ms per iteration - spmv_ms) against the 11 n elements an
iteration's three vector passes move.  Every case runs in a child process of its own under a time limit; the parent
stops at the first child that does not end normally.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_trsv import csr_from_rows, timed  # noqa: E402

CASES = ("banded_1m_f64", "banded_1m_f32", "anywhere_1m_f64", "anywhere_1m_f32", "banded_10m_f64", "banded_10m_f32")


def make_case(name):
    import numpy as np
    kind, t = name.rsplit("_", 1)
    dt = np.float64 if t == "f64" else np.float32
    rng = np.random.default_rng(61)
    n = 10_000_000 if kind == "banded_10m" else 1_000_000
    if kind.startswith("banded"):
        draws = rng.integers(-2048, 2048, size=(n, 15), dtype=np.int32)
        draws[:, 0] = 0
        draws += np.arange(n, dtype=np.int32)[:, None]
    else:
        draws = rng.integers(0, n, size=(n, 8), dtype=np.int32)
        draws[:, 0] = np.arange(n, dtype=np.int32)
    rp, ci = csr_from_rows(n, draws)
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp.astype(np.int64)))
    va = (rng.uniform(-1, 1, ci.size) / 16.0).astype(dt)
    va[rows == ci] = 1
    return n, rp, ci, va


def spread(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "reps": len(xs)}


def solve_sweep(dev, method, m, bt, xt, iters, every_list, reps, st):
    """{check_every: ms per iteration, polls} of --reps solves of exactly `iters` iterations each."""
    out = {}
    for every in every_list:
        dev.set_option("krylov_check_every", every)
        per, info = [], None
        for _ in range(reps):
            xt.zero_()
            info = dev.krylov_dev(bt.data_ptr(), xt.data_ptr(), method, M=m, tol=0.0, maxit=iters, stream=st)
            per.append(info.solve_ms / max(info.iterations, 1))
        d = dev.describe()["krylov"]
        out[str(every)] = {"ms_per_iteration": spread(per), "polls": d["polls"], "iterations": info.iterations,
                           "reason": info.reason, "stopped_early": info.reason != 1}
    return out


def python_loop_ms(dev, f, method, bt, iters, st):
    """The same loops driven from Python: spmv_dev / trsv_dev for the operators, torch for vectors and dots (each dot
    comes back to the host, as a caller without device scalars has it)."""
    import torch

    def mul(v, out):
        dev.spmv_dev(v.data_ptr(), out.data_ptr(), st)
        return out

    def prec(v, out):
        f.trsv_dev(v.data_ptr(), out.data_ptr(), True, True, st)
        f.trsv_dev(out.data_ptr(), out.data_ptr(), False, False, st)
        return out

    x = torch.zeros_like(bt)
    q, z, t, sh, ph = (torch.empty_like(bt) for _ in range(5))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(st)
    r = bt - mul(x, q)
    if method == "cg":
        p = r.clone()
        rz = torch.dot(r, r).item()
        for _ in range(iters):
            mul(p, q)
            alpha = rz / torch.dot(p, q).item()
            x.add_(p, alpha=alpha)
            r.sub_(q, alpha=alpha)
            rz1 = torch.dot(r, r).item()
            p.mul_(rz1 / rz).add_(r)
            rz = rz1
    else:
        rhat, v, p = r.clone(), torch.zeros_like(bt), torch.zeros_like(bt)
        rho = alpha = omega = 1.0
        for _ in range(iters):
            rho1 = torch.dot(rhat, r).item()
            beta = (rho1 / rho) * (alpha / omega)
            rho = rho1
            p.sub_(v, alpha=omega).mul_(beta).add_(r)
            mul(prec(p, ph), v)
            alpha = rho / torch.dot(rhat, v).item()
            s = r.sub_(v, alpha=alpha)
            torch.dot(s, s).item()
            mul(prec(s, sh), t)
            omega = torch.dot(t, s).item() / torch.dot(t, t).item()
            x.add_(ph, alpha=alpha).add_(sh, alpha=omega)
            r = s.sub_(t, alpha=omega)
            torch.dot(r, r).item()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def child(name, out_dir, every_list, cg_iters, bicg_iters, reps):
    import numpy as np
    import torch
    import spalinalg_amd as sp
    n, rp, ci, va = make_case(name)
    es = va.dtype.itemsize
    nnz = int(rp[-1])
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    st = torch.cuda.current_stream()
    tdt = torch.float64 if es == 8 else torch.float32
    bt = torch.rand(n, dtype=tdt, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) * 2 - 1
    xt = torch.empty_like(bt)
    big = torch.empty(32 * 1024 * 1024, dtype=torch.float64, device="cuda")
    big2 = torch.empty_like(big)
    torch.cuda.synchronize()
    copy = timed(lambda: big2.copy_(big), 10, 3)
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": nnz,
           "copy_ceiling_gbs": 2 * big.numel() * 8 / (copy["median"] * 1e-3) / 1e9,
           "spmv_ms": timed(lambda: dev.spmv_dev(bt.data_ptr(), xt.data_ptr(), st), 20, 5)}
    del big, big2
    f = dev.ilu0()
    f.trsv_analyse(True, True)
    f.trsv_analyse(False, False)
    rec["trsv_lower_ms"] = timed(lambda: f.trsv_dev(bt.data_ptr(), xt.data_ptr(), True, True, st), 5, 1)
    rec["trsv_upper_ms"] = timed(lambda: f.trsv_dev(bt.data_ptr(), xt.data_ptr(), False, False, st), 5, 1)
    rec["parts_ms"] = rec["spmv_ms"]["median"] + rec["trsv_lower_ms"]["median"] + rec["trsv_upper_ms"]["median"]
    rec["cg"] = solve_sweep(dev, "cg", None, bt, xt, cg_iters, every_list, reps, st)
    rec["bicgstab_ilu0"] = solve_sweep(dev, "bicgstab", f, bt, xt, bicg_iters, every_list, reps, st)
    best = min(rec["cg"].values(), key=lambda r: r["ms_per_iteration"]["median"])["ms_per_iteration"]["median"]
    vec_ms = best - rec["spmv_ms"]["median"]
    rec["cg_vector_kernels"] = {"bytes_per_iteration": 11 * n * es, "ms_per_iteration": vec_ms,
                                "gbs": 11 * n * es / (vec_ms * 1e-3) / 1e9 if vec_ms > 0 else None}
    rec["python_loop_ms_per_iteration"] = {"cg": python_loop_ms(dev, f, "cg", bt, cg_iters, st),
                                           "bicgstab_ilu0": python_loop_ms(dev, f, "bicgstab", bt, bicg_iters, st)}
    assert np.isfinite(xt.cpu().numpy()).all()
    with open(os.path.join(out_dir, f"krylov_{name}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--every", default="1,2,4,8,16,32")
    ap.add_argument("--cg-iters", type=int, default=64)
    ap.add_argument("--bicg-iters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    every = [int(x) for x in args.every.split(",") if x]
    if args.child:
        child(args.child, args.out, every, args.cg_iters, args.bicg_iters, args.reps)
        return
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, "--every", args.every,
               "--cg-iters", str(args.cg_iters), "--bicg-iters", str(args.bicg_iters), "--reps", str(args.reps)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
