#!/usr/bin/env python3
"""Measures restarted GMRES on the device (spal_csr_gmres_dev_*): ms per inner iteration as a function of j
inside one cycle of restart 30, without a preconditioner and with the ILU(0) factor applied by three sweeps per triangle,
beside what a caller could write before -- the same Arnoldi step (two passes of classical Gram-Schmidt) driven from Python
with spmv_dev, dot_dev (one launch pair per basis vector) and torch vector updates, no host round trip in it -- and the
orthogonalisation kernels' bytes over their time against the copy ceiling.  One JSON record per case under --out DIR.
Development tool, not part of the package, the tests or bench.py.

    python tools/bench_gmres.py --out DIR [--cases banded_1m_f64,...] [--restart 30] [--reps 3]

cases (the matrices of tools/bench_krylov.py):
    banded_{1m,10m}_{f64,f32}   14 draws per row in a window of 4096 around the diagonal, plus the diagonal
    anywhere_1m_{f64,f32}       1M x 1M, 7 draws per row anywhere in the row's 1M columns, plus the diagonal
How a step is timed: the library reports one device time per call, so the call is run with tol = 0 and maxit = k for
k = 1 .. restart (one cycle that ends after exactly k steps, then the cycle's end and the head that stops the call);
step j is t(j + 1) - t(j), which also holds the growth of the cycle's end (one more basis vector in u = V y).  "krylov_
check_every" is set to the restart, so a call polls once per cycle.  The orthogonalisation's share of a step without a
preconditioner is the step minus spmv_ms; its bytes are (4 j + 12) n elements: two multi-dots (w and j + 1 basis vectors
each), two multi-updates (the same, and w written), the scale (w read, v_{j+1} written).  Every case runs in a child
process of its own under a time limit; the parent stops at the first child that does not end normally.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_krylov import CASES, make_case  # noqa: E402
from tools.bench_trsv import timed  # noqa: E402

SWEEPS = 3


def cycle_ms(dev, m, bt, xt, restart, reps, st):
    """[median device ms of a call that runs exactly k steps of one cycle, k = 1 .. restart], and the last describe()"""
    import numpy as np
    out = []
    for k in range(1, restart + 1):
        ms = []
        for _ in range(reps):
            xt.zero_()
            info = dev.gmres_dev(bt.data_ptr(), xt.data_ptr(), M=m, restart=restart, tol=0.0, maxit=k, stream=st)
            assert info.iterations == k and info.reason == 1, info
            ms.append(info.solve_ms)
        out.append(float(np.median(ms)))
    return out, dev.describe()["gmres"]


def steps_of(total):
    return [total[0]] + [total[k] - total[k - 1] for k in range(1, len(total))]


def python_arnoldi_ms(dev, bt, restart, st):
    """ms of step j = 0 .. restart - 1 of the same CGS2 Arnoldi step written with the library's exported operations and
    torch: everything stays on the device (h as 1-element tensors), one dot_dev per basis vector and pass."""
    import numpy as np
    import torch
    import spalinalg_amd as sp
    n = bt.numel()
    dt = np.float64 if bt.dtype == torch.float64 else np.float32
    V = torch.empty(restart + 1, n, dtype=bt.dtype, device="cuda")
    w = torch.empty_like(bt)
    h = torch.zeros(restart + 1, dtype=bt.dtype, device="cuda")
    nrm = torch.zeros(1, dtype=bt.dtype, device="cuda")
    V[0] = bt / bt.norm()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(restart + 1)]
    torch.cuda.synchronize()
    ev[0].record(st)
    for j in range(restart):
        dev.spmv_dev(V[j].data_ptr(), w.data_ptr(), st)
        for _ in range(2):
            for k in range(j + 1):
                sp.dot_dev(dt, V[k].data_ptr(), w.data_ptr(), n, h[k:].data_ptr(), 0, st)
            for k in range(j + 1):
                w.addcmul_(V[k], h[k:k + 1], value=-1)
        sp.dot_dev(dt, w.data_ptr(), w.data_ptr(), n, nrm.data_ptr(), 0, st)
        torch.div(w, nrm.sqrt(), out=V[j + 1])
        ev[j + 1].record(st)
    torch.cuda.synchronize()
    return [ev[j].elapsed_time(ev[j + 1]) for j in range(restart)]


def child(name, out_dir, restart, reps):
    import torch
    import spalinalg_amd as sp
    n, rp, ci, va = make_case(name)
    es = va.dtype.itemsize
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    st = torch.cuda.current_stream()
    tdt = torch.float64 if es == 8 else torch.float32
    bt = torch.rand(n, dtype=tdt, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) * 2 - 1
    xt = torch.empty_like(bt)
    big = torch.empty(32 * 1024 * 1024, dtype=torch.float64, device="cuda")
    big2 = torch.empty_like(big)
    torch.cuda.synchronize()
    copy = timed(lambda: big2.copy_(big), 10, 3)
    ceiling = 2 * big.numel() * 8 / (copy["median"] * 1e-3) / 1e9
    del big, big2
    dev.set_option("krylov_check_every", restart)
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": int(rp[-1]), "restart": restart, "copy_ceiling_gbs": ceiling,
           "spmv_ms": timed(lambda: dev.spmv_dev(bt.data_ptr(), xt.data_ptr(), st), 20, 5)}
    dev.gmres_dev(bt.data_ptr(), xt.data_ptr(), restart=restart, tol=0.0, maxit=restart, stream=st)     # warm-up
    total, d = cycle_ms(dev, None, bt, xt, restart, reps, st)
    step = steps_of(total)
    orth = [s - rec["spmv_ms"]["median"] for s in step]
    rec["plain"] = {"call_ms_by_steps": total, "step_ms_by_j": step, "dot_batch": d["dot_batch"], "basis_bytes": d["basis_bytes"],
                    "orthogonalisation": [{"j": j, "ms": orth[j], "bytes": (4 * j + 12) * n * es,
                                           "gbs": (4 * j + 12) * n * es / (orth[j] * 1e-3) / 1e9 if orth[j] > 0 else None}
                                          for j in range(restart)]}
    f = dev.ilu0()
    f.set_option("trsv_sweeps", SWEEPS)
    dev.gmres_dev(bt.data_ptr(), xt.data_ptr(), M=f, restart=restart, tol=0.0, maxit=restart, stream=st)
    total, d = cycle_ms(dev, f, bt, xt, restart, reps, st)
    rec[f"ilu0_sweeps{SWEEPS}"] = {"call_ms_by_steps": total, "step_ms_by_j": steps_of(total), "basis_bytes": d["basis_bytes"]}
    python_arnoldi_ms(dev, bt, restart, st)                                                             # warm-up
    rec["python_arnoldi_step_ms_by_j"] = python_arnoldi_ms(dev, bt, restart, st)
    with open(os.path.join(out_dir, f"gmres_{name}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        child(args.child, args.out, args.restart, args.reps)
        return
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, "--restart", str(args.restart),
               "--reps", str(args.reps)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
