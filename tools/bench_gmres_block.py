#!/usr/bin/env python3
"""Measures restarted GMRES on a block of k right-hand sides (spal_csr_gmres_block_dev_*) against k vector
calls (spal_csr_gmres_dev_*) on the same handle, in the same process.  One JSON record per case under --out DIR.
Development tool, not part of the package, the tests or bench.py; no time in it is a pass criterion.

    python tools/bench_gmres_block.py --out profiles/gmres_block [--cases banded_1m_f64] [--widths 1,2,4,8,16,32]
                                      [--restart 30] [--reps 3]

cases (the input of tools/bench_colour.py, tools/bench_trsm.py and tools/bench_krylov_block.py):
    banded_1m_{f64,f32}      1M x 1M, 14 draws per row in a window of 4096 around the diagonal, plus the diagonal
Every case runs in a child process of its own under a time limit; the parent stops at the first child that does not end
normally.  A record holds three configurations and, per width k, ms per inner step of either form:
    plain        no preconditioner
    sweeps3      M = ilu0(sweeps=3) applied by 3 Jacobi sweeps per triangle ("trsv_sweeps" = 3)
    exact_mc     on the multicolour() ordering, M = its ilu0(), applied by the exact solves
tol = 0 and maxit = restart, so every call runs exactly one full cycle of `restart` inner steps and the head that stops
it.  A call's time is its own solve_ms (device events from its first to its last launch, polls included); the vector
form is the sum over its k calls.  --reps repetitions after one untimed call: median, min, max.  Column 0 of the block
result is compared bit for bit with the vector call's where the handle's SpMV sums rows in sequence.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("banded_1m_f64", "banded_1m_f32")


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def config(a, m, n, widths, tdt, st, restart, reps):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(7)
    out = {}
    for k in widths:
        B = torch.rand((n, k), dtype=tdt, device="cuda", generator=gen) * 2 - 1
        X = torch.empty_like(B)
        cols = B.t().contiguous()                      # the k right-hand sides as vectors
        xs = torch.empty_like(cols)
        torch.cuda.synchronize()

        def block():
            X.zero_()
            infos = a.gmres_block_dev(k, B.data_ptr(), k, X.data_ptr(), k, m, restart, 0.0, restart, st)
            return infos[0].solve_ms / max(max(i.iterations for i in infos), 1), infos

        def vectors():
            xs.zero_()
            ms, its = 0.0, 1
            for j in range(k):
                info = a.gmres_dev(cols[j].data_ptr(), xs[j].data_ptr(), m, restart, 0.0, restart, st)
                ms, its = ms + info.solve_ms, max(its, info.iterations)
            return ms / its

        block()
        tb = [block() for _ in range(reps)]
        d = a.describe()["gmres_block"]
        rec = {"block": {"ms_per_step": stats([t[0] for t in tb]), "tile": d["tile"], "polls": d["polls"], "steps": d["steps"],
                         "cycles": d["cycles"], "dot_batch": d["dot_batch"], "basis_bytes": d["basis_bytes"],
                         "iterations": [i.iterations for i in tb[-1][1]], "reasons": [i.reason for i in tb[-1][1]]}}
        vectors()
        tv = stats([vectors() for _ in range(reps)])
        torch.cuda.synchronize()
        rec["vector_calls_ms_per_step"] = tv
        rec["block_over_vectors"] = rec["block"]["ms_per_step"]["median"] / tv["median"]
        rec["column_0_bit_identical"] = bool(torch.equal(X[:, 0].contiguous().view(torch.uint8), xs[0].view(torch.uint8)))
        out[str(k)] = rec
    return out


def child(name, out_dir, widths, restart, reps):
    import torch
    import spalinalg_amd as sp
    from tools.bench_colour import make_case
    n, rp, ci, va = make_case(name)
    a = sp.CsrMatrix(n, n, rp, ci, va).device()
    st = torch.cuda.current_stream()
    tdt = torch.float64 if va.dtype.itemsize == 8 else torch.float32
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": int(rp[-1]), "restart": restart, "maxit": restart, "reps": reps,
           "widths": widths, "spmv_kernel": a.describe()["kernel"]}
    rec["plain"] = config(a, None, n, widths, tdt, st, restart, reps)
    f = a.ilu0(st, sweeps=3)
    f.set_option("trsv_sweeps", 3)
    rec["sweeps3"] = config(a, f, n, widths, tdt, st, restart, reps)
    p = a.multicolour(0, st)
    rec["colours"] = p.describe()["ordering"]["colours"]
    rec["exact_mc"] = config(p, p.ilu0(st), n, widths, tdt, st, restart, reps)
    with open(os.path.join(out_dir, f"gmres_block_{name}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    for key in ("plain", "sweeps3", "exact_mc"):
        print(key, {k: round(v["block_over_vectors"], 3) for k, v in rec[key].items()}, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default="banded_1m_f64")
    ap.add_argument("--widths", default="1,2,4,8,16,32")
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    widths = [int(w) for w in args.widths.split(",")]
    if args.child:
        child(args.child, args.out, widths, args.restart, args.reps)
        return
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, "--widths", args.widths,
               "--restart", str(args.restart), "--reps", str(args.reps)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
