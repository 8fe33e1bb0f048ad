#!/usr/bin/env python3
"""Measures C = A * B on the device (spal_csr_mul) over four generated inputs and writes one JSON record per case under
--out DIR.  Development tool, not part of the package, the tests or bench.py.

    python tools/bench_spgemm.py --out DIR [--cases a_f64,a_f32,b,c,d] [--iters 10] [--warmup 2]

cases (spal_synth inputs, every product A * A):
    a_f64 / a_f32   banded 1M x 1M, 14 per row (window 4096)
    b               ragged 1M x 1M (1 ... 27 per row, window 4096)
    c               uniform columns 1M x 1M, 14 per row: little compression, hash-heavy
    d               power-law rows with columns near the rows, 300k rows: the large-row tier
Every case runs in a child process of its own under a time limit; the parent stops at the first child that does not
end normally.  A record holds products (sum of ub) and nnz(C), ms per call (device events over --iters calls after
--warmup, the result's eager plan included), the plan's share (describe()["spgemm"]["plan_ms"], a host clock) and the
time without it, GFLOP/s (2 * products / t), the single-core oracle's time, and torch.sparse.mm of two sparse_csr
tensors on the GPU (rocSPARSE) with a tolerance check of its values against ours, or "unavailable" if it raises.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("a_f64", "a_f32", "b", "c", "d")


def make_case(name):
    import numpy as np
    import spal_synth as synth
    n = 1_000_000
    if name in ("a_f64", "a_f32"):
        dt = np.float64 if name == "a_f64" else np.float32
        return n, synth.banded_csr(n, n, 14, 4096, synth.matrix_seed(3), dtype=dt)
    if name == "b":
        return n, synth.ragged_csr(n, n, 4096, synth.matrix_seed(3))
    if name == "c":
        return n, synth.banded_csr(n, n, 14, n, synth.matrix_seed(3))
    n = 300_000
    rng = np.random.default_rng(31)
    lens = np.minimum((rng.pareto(1.6, n) * 6 + 1).astype(np.int64), 5000)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = np.clip(rows - 5000 + rng.integers(0, 10000, rows.size), 0, n - 1)
    key = np.unique(rows * n + cols)
    r2, c2 = key // n, key % n
    rp = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=n))]).astype(np.uint64)
    return n, (rp, c2.astype(np.uint64), rng.uniform(-1, 1, c2.size))


def rocsparse_leg(n, a, ours, iters, warmup):
    """torch.sparse.mm of two sparse_csr tensors on the GPU: its time and how far its values are from ours."""
    import numpy as np
    import torch
    rp, ci, va = a
    try:
        t = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)), torch.from_numpy(ci.astype(np.int64)),
                                    torch.from_numpy(va), size=(n, n), device="cuda")
        for _ in range(warmup):
            r = torch.sparse.mm(t, t)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            r = torch.sparse.mm(t, t)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        r = r.to_sparse_csr() if r.layout != torch.sparse_csr else r
        trp, tci, tva = (r.crow_indices().cpu().numpy(), r.col_indices().cpu().numpy(), r.values().cpu().numpy())
        orp, oci, ova = ours
        out = {"ms": ms, "nnz": int(tva.size)}
        if np.array_equal(trp, orp.astype(np.int64)) and np.array_equal(tci, oci.astype(np.int64)):
            scale = float(np.abs(ova).max()) if ova.size else 0.0
            err = float(np.abs(tva.astype(np.float64) - ova.astype(np.float64)).max()) if ova.size else 0.0
            tol = 1e-12 if ova.dtype == np.float64 else 1e-5
            out.update(pattern="equal", max_abs_diff=err, rel_to_max=err / scale if scale else 0.0,
                       within_tolerance=bool(err <= tol * max(scale, 1.0)))
        else:
            out.update(pattern="differs")   # (rocSPARSE may drop or keep other entries; values not compared)
        return out
    except Exception as e:  # noqa: BLE001 -- recorded, not fatal
        return {"status": "unavailable", "error": f"{type(e).__name__}: {e}"[:300]}


def child(name, out_dir, iters, warmup):
    import importlib
    import numpy as np
    import torch
    import spalinalg_amd as sp
    # the single-core CPU baseline leg only, as in bench.py: the checker is loaded here and nowhere on the product path
    oracle = importlib.import_module("oracle")
    n, a = make_case(name)
    A = sp.CsrMatrix(n, n, *a)
    dev = A.device()
    stream = torch.cuda.current_stream()
    for _ in range(warmup):
        dev.mul(dev, stream).close()
    torch.cuda.synchronize()
    results = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        results.append(dev.mul(dev, stream))
    e1.record(stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    infos = [r.describe()["spgemm"] for r in results]
    plan_ms = float(np.mean([i["plan_ms"] for i in infos]))
    ours = results[0].download()
    for r in results:
        r.close()
    info = infos[0]
    t0 = time.perf_counter()
    ref = oracle.csr_mul((n, n), a, (n, n), a)
    oracle_s = time.perf_counter() - t0
    bits = np.uint64 if ours[2].dtype == np.float64 else np.uint32
    same = (np.array_equal(ours[0], ref[0]) and np.array_equal(ours[1], ref[1])
            and np.array_equal(ours[2].view(bits), ref[2].view(bits)))
    products = info["products"]
    rec = {
        "case": name, "dtype": str(a[2].dtype), "n": n, "nnz_a": int(a[0][-1]), "products": products,
        "nnz_c": info["nnz"], "tier_rows": info["tier_rows"], "large_products": info["large_products"],
        "iters": iters, "warmup": warmup, "ms_per_call": ms, "plan_ms": plan_ms,
        "ms_per_call_without_plan": ms - plan_ms,
        "gflops": 2.0 * products / (ms * 1e6), "gflops_without_plan": 2.0 * products / ((ms - plan_ms) * 1e6),
        "bit_identical_to_oracle": bool(same), "oracle_single_core_s": oracle_s,
        "rocsparse": rocsparse_leg(n, a, ours, iters, warmup),
    }
    with open(os.path.join(out_dir, f"spgemm_{name}.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        child(args.child, args.out, max(args.iters, 10), max(args.warmup, 2))
        return
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out,
               "--iters", str(args.iters), "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
