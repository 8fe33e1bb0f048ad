#!/usr/bin/env python3
"""Measures eigsh on the device (spal_csr_eigsh_*): ms per Lanczos step as a function of j, ms per restart
rotation V <- V Y for both kernel forms against (m + keep) n sizeof(T) bytes at the copy ceiling, and ms and restarts to
k = 6 LA at tol = 1e-8.  One JSON record per case under --out DIR.  Development tool, not part of the package, the tests
or bench.py.

    python tools/bench_eigsh.py --out DIR [--cases banded_1m_f64,...] [--ncv 30] [--reps 3]

cases:
    banded_{1m,10m}_{f64,f32} the matrix of tools/bench_krylov.py: 14 draws per row in a window of 4096, plus the diagonal.
                              It is NOT symmetric (eigsh does not check): its step and rotation times are what they would
                              be on a symmetric matrix of that pattern, its Ritz values are those of nothing in particular.
    poisson2d_1000_{f64,f32}  the five-point Laplacian on a 1000 x 1000 grid (tools/bench_amg.py), n = 1M
How a step is timed: the library reports one device time per call, so the call is run with k = 1, maxit = 0 and no
vectors for ncv = 2 .. --ncv + 1 (one phase of exactly ncv steps, no rotation); step j is t(j + 2) - t(j + 1), and
t(2) holds the start vector and steps 0 and 1.  How a rotation is timed: a call with a tolerance nothing meets and maxit
= 5 restarts, "eigsh_rotate" = 1 (batched passes) and = 2 (LDS row tiles); describe()["eigsh"]["rotate_ms"] / 5.  Every
case runs in a child process of its own under a time limit; the parent stops at the first child that does not end normally.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("banded_1m_f64", "banded_1m_f32", "poisson2d_1000_f64", "poisson2d_1000_f32", "banded_10m_f64", "banded_10m_f32")
RESTARTS = 5


def make(name):
    import numpy as np
    if name.startswith("banded"):
        from tools.bench_krylov import make_case
        return make_case(name)
    from tools.bench_amg import stencil
    return stencil((1000, 1000), np.float64 if name.endswith("f64") else np.float32)


def child(name, out_dir, ncv, reps):
    import numpy as np
    import torch
    import spalinalg_amd as sp
    from tools.bench_trsv import timed
    n, rp, ci, va = make(name)
    es = va.dtype.itemsize
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    st = torch.cuda.current_stream()
    tdt = torch.float64 if es == 8 else torch.float32
    bt = torch.rand(n, dtype=tdt, device="cuda")
    xt = torch.empty_like(bt)
    big = torch.empty(32 * 1024 * 1024, dtype=torch.float64, device="cuda")
    big2 = torch.empty_like(big)
    torch.cuda.synchronize()
    copy = timed(lambda: big2.copy_(big), 10, 3)
    ceiling = 2 * big.numel() * 8 / (copy["median"] * 1e-3) / 1e9
    del big, big2
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": int(rp[-1]), "ncv": ncv, "copy_ceiling_gbs": ceiling,
           "spmv_ms": timed(lambda: dev.spmv_dev(bt.data_ptr(), xt.data_ptr(), st), 20, 5)}
    dev.eigsh(1, "LA", ncv, tol=1e-300, maxit=0, return_eigenvectors=False)      # warm-up: the plan, the allocator's blocks
    total = []
    for m in range(2, ncv + 2):
        ms = []
        for _ in range(reps):
            _, _, info = dev.eigsh(1, "LA", m, tol=1e-300, maxit=0, return_eigenvectors=False)
            assert info.products == m and info.restarts == 0, info
            ms.append(info.solve_ms)
        total.append(float(np.median(ms)))
    rec["call_ms_by_ncv"] = {str(m): t for m, t in zip(range(2, ncv + 2), total)}
    rec["step_ms_by_j"] = {str(j): total[j - 1] - total[j - 2] for j in range(2, ncv + 1)}
    k = 6
    rec["rotation"] = {}
    for form, label in ((1, "batch"), (2, "lds")):
        dev.set_option("eigsh_rotate", form)
        ms = []
        for _ in range(reps + 1):
            _, _, info = dev.eigsh(k, "LA", ncv, tol=1e-300, maxit=RESTARTS, return_eigenvectors=False)
            d = dev.describe()["eigsh"]
            assert info.restarts == RESTARTS and d["rotate"] == label, (info, d)
            ms.append(d["rotate_ms"] / RESTARTS)
        keep = d["keep"]
        byts = (ncv + keep) * n * es
        med = float(np.median(ms[1:]))
        rec["rotation"][label] = {"ms": med, "all_ms": ms[1:], "m": ncv, "keep": keep, "tile_rows": d["rotate_tile_rows"],
                                  "bytes": byts, "gbs": byts / (med * 1e-3) / 1e9, "ms_at_copy_ceiling": byts / ceiling / 1e6,
                                  "basis_bytes": d["basis_bytes"]}
    dev.set_option("eigsh_rotate", 0)
    theta, _, info = dev.eigsh(k, "LA", ncv, tol=1e-8, maxit=300)
    rec["solve_k6_la_tol1e-8"] = {"solve_ms": info.solve_ms, "restarts": info.restarts, "products": info.products,
                                  "converged": info.converged, "reason": info.reason, "theta": [float(t) for t in theta],
                                  "rotate_ms": dev.describe()["eigsh"]["rotate_ms"]}
    with open(os.path.join(out_dir, f"eigsh_{name}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES[:4]), help="default: the four 1M cases")
    ap.add_argument("--ncv", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        child(args.child, args.out, args.ncv, args.reps)
        return
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, "--ncv", str(args.ncv),
               "--reps", str(args.reps)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
