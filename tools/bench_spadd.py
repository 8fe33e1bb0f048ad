#!/usr/bin/env python3
"""Measures C = A + B and C = A - B on the device (spal_csr_add / spal_csr_sub) over four generated inputs and writes
one JSON record per case under --out DIR.  Development tool, not part of the package, the tests or bench.py.

    python tools/bench_spadd.py --out DIR [--cases a_f64,a_f32,b,c,d] [--iters 10] [--warmup 2]

cases (spal_synth inputs):
    a_f64 / a_f32   banded 1M x 1M, 14 per row (window 4096), A + A' with A' of A's structure and other values:
                    every position matched
    b               banded 1M x 1M, seeds 3 and 4: almost disjoint
    c               power-law rows with columns near the rows, 300k rows, two seeds
    d               config-3 size: banded 10M x 10M, 140M + 140M entries (seeds 3 and 4), f64
Every case runs in a child process of its own under a time limit; the parent stops at the first child that does not
end normally.  A record holds nnz(A), nnz(B), the matched pairs and nnz(C); ms per call for Add and for Sub (device
events over --iters calls through DeviceCsr.add / .sub after --warmup: no download inside the timed region), the
result's plan (describe()["spadd"]["plan_ms"], a host clock) and the kernels' device time (kernel_ms); the one-pass
bytes (4 + es) * (nnz(A) + nnz(B) + nnz(C)) + 12 * (n + 1) and their share of the 8 TB/s peak over kernel_ms; parity
with the CPU restatement (tests/spadd_ref.py: every row, or 4096 sampled rows in case d); and torch.add of two
sparse_csr tensors on the GPU (rocSPARSE), its time and whether its arrays equal ours, or "unavailable" if it raises.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("a_f64", "a_f32", "b", "c", "d")
PEAK_BYTES_PER_S = 8e12


def power_law(n, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    lens = np.minimum((rng.pareto(1.6, n) * 6 + 1).astype(np.int64), 5000)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = np.clip(rows - 5000 + rng.integers(0, 10000, rows.size), 0, n - 1)
    key = np.unique(rows * n + cols)
    r2, c2 = key // n, key % n
    rp = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=n))]).astype(np.uint64)
    return rp, c2.astype(np.uint64), rng.uniform(-1, 1, c2.size)


def make_case(name):
    import numpy as np
    import spal_synth as synth
    n = 1_000_000
    if name in ("a_f64", "a_f32"):
        dt = np.float64 if name == "a_f64" else np.float32
        a = synth.banded_csr(n, n, 14, 4096, synth.matrix_seed(3), dtype=dt)
        vals = np.random.default_rng(4).uniform(-1, 1, a[2].size).astype(dt)
        return n, a, (a[0], a[1], vals)
    if name == "b":
        return n, synth.banded_csr(n, n, 14, 4096, synth.matrix_seed(3)), synth.banded_csr(n, n, 14, 4096, synth.matrix_seed(4))
    if name == "c":
        n = 300_000
        return n, power_law(n, 31), power_law(n, 32)
    n = 10_000_000
    return n, synth.banded_csr(n, n, 14, 4096, synth.matrix_seed(3)), synth.banded_csr(n, n, 14, 4096, synth.matrix_seed(4))


def rows_of(arr, rows):
    """the CSR arrays of the listed rows of `arr` (a smaller matrix with len(rows) rows)"""
    import numpy as np
    rp, ci, va = arr
    rp = rp.astype(np.int64)
    lens = rp[rows + 1] - rp[rows]
    idx = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), ci[idx], va[idx]


def same_bits(x, y):
    import numpy as np
    bits = np.uint64 if x[2].dtype == np.float64 else np.uint32
    return bool(np.array_equal(np.asarray(x[0], np.uint64), np.asarray(y[0], np.uint64))
                and np.array_equal(np.asarray(x[1], np.uint64), np.asarray(y[1], np.uint64))
                and np.array_equal(x[2].view(bits), y[2].view(bits)))


def rocsparse_leg(n, a, b, ours, iters, warmup):
    """torch.add of two sparse_csr tensors on the GPU: its time and whether its arrays equal ours."""
    import numpy as np
    import torch
    try:
        ts = [torch.sparse_csr_tensor(torch.from_numpy(m[0].astype(np.int64)), torch.from_numpy(m[1].astype(np.int64)),
                                      torch.from_numpy(m[2]), size=(n, n), device="cuda") for m in (a, b)]
        for _ in range(warmup):
            r = torch.add(ts[0], ts[1])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            r = torch.add(ts[0], ts[1])
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        r = r.to_sparse_csr() if r.layout != torch.sparse_csr else r
        theirs = (r.crow_indices().cpu().numpy().astype(np.uint64), r.col_indices().cpu().numpy().astype(np.uint64),
                  r.values().cpu().numpy())
        return {"ms": ms, "nnz": int(theirs[2].size), "arrays_equal_ours": same_bits(theirs, ours)}
    except Exception as e:  # noqa: BLE001 -- recorded, not fatal
        return {"status": "unavailable", "error": f"{type(e).__name__}: {e}"[:300]}


def time_op(dev_a, dev_b, op, stream, iters, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        getattr(dev_a, op)(dev_b, stream).close()
    torch.cuda.synchronize()
    results = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        results.append(getattr(dev_a, op)(dev_b, stream))
    e1.record(stream)
    torch.cuda.synchronize()
    infos = [r.describe()["spadd"] for r in results]
    out = {"ms_per_call": e0.elapsed_time(e1) / iters,
           "plan_ms": float(np.mean([i["plan_ms"] for i in infos])),
           "kernel_ms": float(np.median([i["kernel_ms"] for i in infos])),
           "kernel_ms_min": float(np.min([i["kernel_ms"] for i in infos]))}
    for r in results[1:]:
        r.close()
    return out, results[0], infos[0]


def child(name, out_dir, iters, warmup):
    import numpy as np
    import torch
    import spalinalg_amd as sp
    from tests import spadd_ref
    n, a, b = make_case(name)
    A, B = sp.CsrMatrix(n, n, *a), sp.CsrMatrix(n, n, *b)
    da, db = A.device(), B.device()
    stream = torch.cuda.current_stream()
    es = a[2].dtype.itemsize
    rec = {"case": name, "dtype": str(a[2].dtype), "n": n, "nnz_a": int(a[0][-1]), "nnz_b": int(b[0][-1]),
           "iters": iters, "warmup": warmup}
    rng = np.random.default_rng(12)
    for op in ("add", "sub"):
        t, res, info = time_op(da, db, op, stream, iters, warmup)
        ours = res.download()
        res.close()
        nnz_c = info["nnz"]
        one_pass = (4 + es) * (rec["nnz_a"] + rec["nnz_b"] + nnz_c) + 12 * (n + 1)
        if name == "d":   # parity on 4096 sampled rows
            rows = np.sort(rng.choice(n, size=4096, replace=False))
            ref = spadd_ref.add_sub_fast(len(rows), n, rows_of(a, rows), rows_of(b, rows), op == "sub")
            parity = {"rows": 4096, "bit_identical": same_bits(rows_of(ours, rows), ref)}
        else:
            ref = spadd_ref.add_sub_fast(n, n, a, b, op == "sub")
            parity = {"rows": n, "bit_identical": same_bits(ours, ref)}
        rec[op] = dict(t, matched=info["matched"], nnz_c=nnz_c, tile=info["tile"], tiles=info["tiles"],
                       one_pass_bytes=one_pass,
                       share_of_peak_over_kernel_ms=one_pass / (t["kernel_ms"] * 1e-3) / PEAK_BYTES_PER_S,
                       parity=parity)
        if op == "add":
            rec["rocsparse_add"] = rocsparse_leg(n, a, b, ours, min(iters, 5), 1) if name != "d" else \
                rocsparse_leg(n, a, b, ours, 2, 1)
        del ours
    with open(os.path.join(out_dir, f"spadd_{name}.json"), "w") as f:
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
        child(args.child, args.out, args.iters, args.warmup)
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
