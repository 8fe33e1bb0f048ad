#!/usr/bin/env python3
"""Measures ILU(0) by row sweeps (spal_csr_ilu0_sweep): what a pass costs and what a factor of s passes is
worth as a preconditioner, beside the exact factorisation of the same handle.  One JSON record per case under --out DIR.
Development tool, not part of the package, the tests or bench.py; no time in it is a pass criterion.

    python tools/bench_ilu_sweep.py --out profiles/ilu_sweep [--cases banded_1m_f64,...] [--sweeps 1,2,3,5] [--reps 3]
    python tools/bench_ilu_sweep.py --out DIR --cost-only --lib PATH --tag b128_s2048      (a geometry variant)

cases (the matrices of tools/bench_ilu.py):
    banded_1m_{f64,f32}     1M x 1M, 14 draws per row in a window of 4096 around the diagonal, plus the diagonal
    anywhere_1m_{f64,f32}   1M x 1M, 7 draws per row anywhere in the row's 1M columns, plus the diagonal
Every case runs in a child process of its own under a time limit; the parent stops at the first child that does not end
normally.  A record holds
  cost:    one SpMV on the handle (device events); for every s the kernel_ms and call_ms of describe()["ilu0_sweep"]
           (--reps calls: median, min, max) and kernel_ms / s as ms per pass -- kernel_ms holds the one classification
           launch too; the first swept call of the fresh handle (it pays the preparation); then, from the same run, the
           exact ilu0(): its first call, the host analysis it paid (describe()["trsv"]["lower"]["analysis_ms"]) and its
           kernel_ms over --reps further calls.  The swept calls come first, and the record says what the operand's
           describe() showed after them ("analyses_after_sweeps": 0, no "trsv" object).
  quality: BiCGStab from x0 = 0 at one tolerance (1e-8 for f64, 1e-5 for f32, at most 500 iterations; the median of three
           solves) with M = ilu0(sweeps=s) for every s, M = the exact ilu0(), both applied by three Jacobi sweeps per
           triangle, and the multicolour route of tools/bench_colour.py (P A P^T, its exact ilu0 applied by exact
           solves): iterations, reason, total ms, and the largest |swept - exact| entry of the factor.
  bits:    where the lower triangle has at most 64 levels, whether ilu0(sweeps=levels - 1) is the exact factor bit for bit.
The geometry (block_rows, stage_entries) is fixed when the library is built (-DSPAL_ILU_SWEEP_ROWS, -DSPAL_ILU_SWEEP_STAGE).
--lib runs the children on another build of the library (the SPAL_HIP_LIB override of spalinalg_amd/_ffi.py), --tag
names it in the record and its file, and --cost-only stops after the swept calls: a sweep over the geometry is one such
run per build, and `--table DIR` prints the records of a directory side by side.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_ilu import CASES, make_case, spread  # noqa: E402
from tools.bench_trsv import timed  # noqa: E402

MAXIT = 500
APPLY_SWEEPS = 3


def swept(dev, s, reps):
    """--reps swept factorisations: the describe() figures, and the last factor."""
    kernel, call, f = [], [], None
    for _ in range(reps):
        f = None                       # the previous factor's memory goes back before the next is allocated
        f = dev.ilu0(sweeps=s)
        d = f.describe()["ilu0_sweep"]
        kernel.append(d["kernel_ms"])
        call.append(d["call_ms"])
    rec = {"kernel_ms": spread(kernel), "call_ms": spread(call), "ms_per_pass": spread([k / d["sweeps"] for k in kernel]),
           "sweeps": d["sweeps"], "launches": d["launches"], "rows_wide_form": d["rows_wide_form"],
           "rows_row_form": d["rows_row_form"]}
    return rec, f


def bicgstab(dev, factor, apply_sweeps, bt, xt, tol, st):
    """iterations, reason and total ms (median of three solves from x0 = 0) with `factor` applied exactly (-1) or by sweeps"""
    import numpy as np
    factor.set_option("trsv_sweeps", apply_sweeps)
    ms, info = [], None
    for _ in range(3):
        xt.zero_()
        info = dev.krylov_dev(bt.data_ptr(), xt.data_ptr(), "bicgstab", factor, tol, MAXIT, st)
        ms.append(info.solve_ms)
    factor.set_option("trsv_sweeps", -1)
    return {"iterations": info.iterations, "reason": info.reason, "precond_sweeps": apply_sweeps,
            "total_ms": {"median": float(np.median(ms)), "min": min(ms), "max": max(ms), "reps": 3},
            "relative_residual": float(np.sqrt(info.residual_sq / info.rhs_sq)) if info.rhs_sq else None}


def child(name, out_dir, sweeps, reps, tag, cost_only):
    import numpy as np
    import torch
    import spalinalg_amd as sp
    n, rp, ci, va = make_case(name)
    es = va.dtype.itemsize
    nnz = int(rp[-1])
    tol = 1e-8 if es == 8 else 1e-5
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    st = torch.cuda.current_stream()
    tdt = torch.float64 if es == 8 else torch.float32
    bt = torch.rand(n, dtype=tdt, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) * 2 - 1
    xt, bp = torch.empty_like(bt), torch.empty_like(bt)
    torch.cuda.synchronize()
    rec = {"case": name, "tag": tag, "dtype": str(va.dtype), "n": n, "nnz": nnz,
           "matrix_bytes": nnz * (es + 4) + 4 * (n + 1), "tol": tol, "maxit": MAXIT,
           "spmv_ms": timed(lambda: dev.spmv_dev(bt.data_ptr(), xt.data_ptr(), st), 20, 5)}
    # ---- cost: the sweeps first, on a handle nothing has analysed
    t0 = time.perf_counter()
    f = dev.ilu0(sweeps=1)
    rec["first_swept_call_ms"] = (time.perf_counter() - t0) * 1e3
    d = f.describe()["ilu0_sweep"]
    rec["geometry"] = {k: d[k] for k in ("block_rows", "stage_entries", "wide_stage_entries", "wide_work")}
    f = None
    factors, rec["swept"] = {}, {}
    for s in sweeps:
        rec["swept"][str(s)], factors[s] = swept(dev, s, reps)
    after = dev.describe()
    rec["analyses_after_sweeps"] = after.get("trsv", {}).get("analyses", 0)
    rec["trsv_object_after_sweeps"] = "trsv" in after
    rec["preparation_ms"] = after["trsv_sweep"]["prepare_ms"]
    path = os.path.join(out_dir, f"ilu_sweep_{name}{'_' + tag if tag else ''}.json")
    if cost_only:
        with open(path, "w") as fh:
            json.dump(rec, fh, indent=1)
        print(json.dumps(rec))
        return
    # ---- ... then the exact factorisation of the same handle
    t0 = time.perf_counter()
    exact = dev.ilu0()
    rec["exact_first_call_ms"] = (time.perf_counter() - t0) * 1e3
    lower = dev.describe()["trsv"]["lower"]
    rec["exact_lower_plan"] = lower
    kernel, call = [exact.describe()["ilu0"]["kernel_ms"]], [exact.describe()["ilu0"]["call_ms"]]
    for _ in range(reps):
        exact = None
        exact = dev.ilu0()
        kernel.append(exact.describe()["ilu0"]["kernel_ms"])
        call.append(exact.describe()["ilu0"]["call_ms"])
    rec["exact"] = {"kernel_ms": spread(kernel[1:]), "call_ms": spread(call[1:]), "first_kernel_ms": kernel[0],
                    "analysis_ms": lower["analysis_ms"], "levels": lower["levels"], "launches": lower["launches"]}
    # ---- quality
    exact_bits = exact.download()[2]
    rec["solve"] = {}
    for s in sweeps:
        r = bicgstab(dev, factors[s], APPLY_SWEEPS, bt, xt, tol, st)
        r["max_abs_error_of_the_factor"] = float(np.abs(factors[s].download()[2].astype(np.float64) - exact_bits).max())
        r["factor_kernel_ms"] = rec["swept"][str(s)]["kernel_ms"]["median"]
        rec["solve"][f"swept_{s}"] = r
        factors[s] = None
    rec["solve"]["exact"] = bicgstab(dev, exact, APPLY_SWEEPS, bt, xt, tol, st)
    rec["solve"]["exact"]["factor_kernel_ms"] = rec["exact"]["kernel_ms"]["median"]
    rec["solve"]["exact"]["factor_analysis_ms"] = lower["analysis_ms"]
    if lower["levels"] <= 64:
        same = dev.ilu0(sweeps=lower["levels"] - 1).download()[2]
        bits = np.uint64 if es == 8 else np.uint32
        rec["levels_minus_one_sweeps_bit_identical_to_exact"] = bool(np.array_equal(same.view(bits), exact_bits.view(bits)))
    exact = None
    # ---- the multicolour route: reorder, factorise exactly, apply by exact solves
    t0 = time.perf_counter()
    p = dev.multicolour(0, st)
    mc_ms = (time.perf_counter() - t0) * 1e3
    fm = p.ilu0(st)
    p.permute_vec_dev(bt.data_ptr(), bp.data_ptr(), False, st)
    r = bicgstab(p, fm, -1, bp, xt, tol, st)
    r.update(multicolour_call_ms=mc_ms, colours=p.describe()["ordering"]["colours"],
             factor_kernel_ms=fm.describe()["ilu0"]["kernel_ms"],
             factor_analysis_ms=p.describe()["trsv"]["lower"]["analysis_ms"],
             spmv_ms=timed(lambda: p.spmv_dev(bp.data_ptr(), xt.data_ptr(), st), 20, 5))
    rec["solve"]["multicolour_exact"] = r
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


def table(directory):
    """The records of a directory side by side: geometry, ms per pass by s, beside one SpMV."""
    print("| case | build | block_rows | stage_entries | SpMV ms | " + " | ".join(f"s = {s}: ms per pass" for s in (1, 2, 3, 5)) + " |")
    print("|---|---|---|---|---|---|---|---|---|")
    for fn in sorted(os.listdir(directory)):
        if not (fn.startswith("ilu_sweep_") and fn.endswith(".json")):
            continue
        with open(os.path.join(directory, fn)) as fh:
            r = json.load(fh)
        g = r["geometry"]
        per = [r["swept"].get(str(s), {}).get("ms_per_pass", {}).get("median") for s in (1, 2, 3, 5)]
        print(f"| {r['case']} | {r.get('tag') or 'default'} | {g['block_rows']} | {g['stage_entries']} | "
              f"{r['spmv_ms']['median']:.4f} | " + " | ".join("-" if v is None else f"{v:.4f}" for v in per) + " |")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out")
    ap.add_argument("--table", metavar="DIR", help="print the records of DIR side by side and stop")
    ap.add_argument("--lib", help="run the children on this build of libspal_hip.so")
    ap.add_argument("--tag", default="", help="names the build in the record and its file")
    ap.add_argument("--cost-only", action="store_true", help="stop after the swept calls")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--sweeps", default="1,2,3,5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.table:
        table(args.table)
        return
    if not args.out:
        sys.exit("--out DIR is required")
    os.makedirs(args.out, exist_ok=True)
    sweeps = [int(x) for x in args.sweeps.split(",") if x]
    if any(s < 1 for s in sweeps):
        sys.exit("--sweeps: every count must be >= 1")
    if args.child:
        child(args.child, args.out, sweeps, args.reps, args.tag, args.cost_only)
        return
    env = dict(os.environ, SPAL_HIP_LIB=os.path.abspath(args.lib)) if args.lib else None
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, "--sweeps", args.sweeps,
               "--reps", str(args.reps), "--tag", args.tag] + (["--cost-only"] if args.cost_only else [])
        try:
            rc = subprocess.run(cmd, timeout=args.timeout, env=env).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
