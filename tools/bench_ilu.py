#!/usr/bin/env python3
"""Measures ILU(0) on the device (spal_csr_ilu0) over sweeps of its two options, "ilu_wide_work" and "trsv_chain_rows",
beside its yardsticks: one lower solve on the factor (the same launch list: the latency floor of the schedule), one SpMV
on the operand (the same bytes with no dependencies), and what a caller had before -- the sequential loop on one host
core (tools/micro/ilu0_host.cpp, g++ -O3 -ffp-contract=off) plus creating a handle from the host arrays again.  One
JSON record per case under --out DIR.  Development tool, not part of the package, the tests or bench.py.

    python tools/bench_ilu.py --out DIR [--cases banded_1m_f64,...] [--wide 0,256,1024,4096,16384,65536,huge]
                              [--chain 0,64,256,1024,4096,huge] [--reps 3] [--no-host]

cases:
    banded_1m_{f64,f32}     1M x 1M, 14 draws per row in a window of 4096 around the diagonal, plus the diagonal
    anywhere_1m_{f64,f32}   1M x 1M, 7 draws per row anywhere in the row's 1M columns, plus the diagonal
Every case runs in a child process of its own under a time limit; the parent stops at the first child that does not end
normally.  Off-diagonal values are uniform in (-1/16, 1/16) and the diagonal is 1: rows are strictly diagonally dominant,
which ILU(0) preserves.  A record holds the lower triangle's levels, launches and analysis time as the operand reports
them, the first call (it pays the analysis) and per point of either sweep kernel_ms and call_ms of describe()["ilu0"]
(--reps calls: median, min, max) with the rows in each form; the device factor is compared bit for bit with the host
program's.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_trsv import csr_from_rows, timed  # noqa: E402

CASES = ("banded_1m_f64", "banded_1m_f32", "anywhere_1m_f64", "anywhere_1m_f32")
HUGE = 1 << 40
HOST_SRC = os.path.join(ROOT, "tools", "micro", "ilu0_host.cpp")
HOST_EXE = os.path.join(ROOT, "tools", "micro", "ilu0_host")


def make_case(name):
    import numpy as np
    kind, t = name.rsplit("_", 1)
    dt = np.float64 if t == "f64" else np.float32
    rng = np.random.default_rng(59)
    n = 1_000_000
    if kind == "banded_1m":
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


def factorise(dev, reps):
    """--reps factorisations of a handle whose plan exists: the describe() figures, and the last factor."""
    kernel, call, f = [], [], None
    for _ in range(reps):
        f = None                       # the previous factor's memory goes back before the next is allocated
        f = dev.ilu0()
        d = f.describe()["ilu0"]
        kernel.append(d["kernel_ms"])
        call.append(d["call_ms"])
    return {"kernel_ms": spread(kernel), "call_ms": spread(call), "rows_wide_form": d["rows_wide_form"],
            "rows_row_form": d["rows_row_form"], "launches": d["launches"], "chain_launches": d["chain_launches"]}, f


def host_alternative(n, rp, ci, va):
    """The sequential loop on one core, and a handle created from the host arrays again; the host factor."""
    import numpy as np
    import spalinalg_amd as sp
    if not os.path.exists(HOST_EXE) or os.path.getmtime(HOST_EXE) < os.path.getmtime(HOST_SRC):
        subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++17", HOST_SRC, "-o", HOST_EXE])
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, p) for p in ("rowptr", "colind", "values", "factor")]
        rp.tofile(paths[0]), ci.tofile(paths[1]), va.tofile(paths[2])
        out = subprocess.run([HOST_EXE, "f64" if va.dtype == np.float64 else "f32", str(n)] + paths, check=True,
                             capture_output=True, text=True)
        factor = np.fromfile(paths[3], dtype=va.dtype)
    t0 = time.perf_counter()
    again = sp.CsrMatrix(n, n, rp, ci, factor).device()
    create_ms = (time.perf_counter() - t0) * 1e3
    del again
    return {"loop_ms": float(out.stdout.strip()), "create_handle_ms": create_ms}, factor


def child(name, out_dir, wide, chain, reps, use_host):
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
    torch.cuda.synchronize()
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": nnz, "matrix_bytes": nnz * (es + 4) + 4 * (n + 1),
           "spmv_ms": timed(lambda: dev.spmv_dev(bt.data_ptr(), xt.data_ptr(), st), 20, 5)}
    t0 = time.perf_counter()
    f = dev.ilu0()                                        # the first call: analysis included
    rec["first_call_ms"] = (time.perf_counter() - t0) * 1e3
    lower = dev.describe()["trsv"]["lower"]
    rec["lower_plan"] = lower
    rec["defaults"] = {k: f.describe()["ilu0"][k] for k in ("wide_work", "chain_rows", "lds_stage_entries")}
    rec["default"], f = factorise(dev, reps)
    rec["trsv_lower_on_factor_ms"] = timed(lambda: f.trsv_dev(bt.data_ptr(), xt.data_ptr(), True, True, st), 10, 2)
    default_bits = f.download()[2]
    if use_host:
        rec["host"], host_factor = host_alternative(n, rp, ci, va)
        bits = np.uint64 if es == 8 else np.uint32
        rec["bit_identical_to_host"] = bool(np.array_equal(default_bits.view(bits), host_factor.view(bits)))
    f = None
    rec["sweep_wide_work"], rec["sweep_chain_rows"] = {}, {}
    for thr in wide:
        dev.set_option("ilu_wide_work", thr)
        rec["sweep_wide_work"]["huge" if thr == HUGE else str(thr)], f = factorise(dev, reps)
        f = None
    dev.set_option("ilu_wide_work", rec["defaults"]["wide_work"])
    for thr in chain:
        dev.set_option("trsv_chain_rows", thr)
        rec["sweep_chain_rows"]["huge" if thr == HUGE else str(thr)], f = factorise(dev, reps)
        f = None
    with open(os.path.join(out_dir, f"ilu_{name}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--wide", default="0,256,1024,4096,16384,65536,huge")
    ap.add_argument("--chain", default="0,64,256,1024,4096,huge")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the sequential host loop")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    parse = lambda s: [HUGE if x == "huge" else int(x) for x in s.split(",") if x]   # noqa: E731
    if args.child:
        child(args.child, args.out, parse(args.wide), parse(args.chain), args.reps, not args.no_host)
        return
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, "--wide", args.wide,
               "--chain", args.chain, "--reps", str(args.reps)] + (["--no-host"] if args.no_host else [])
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
