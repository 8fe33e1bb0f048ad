#!/usr/bin/env python3
"""Measures Y = A * X for a dense block of k vectors (spal_csr_spmm_dev_*) against what a caller had before it: k
back-to-back spal_csr_spmv_dev_* launches on the same handle with its default plan.  One JSON record per case under
--out DIR.  Development tool, not part of the package, the tests or bench.py.

    python tools/bench_spmm.py --out DIR [--cases banded_1m_f64,...] [--ks 1,2,4,8,16,32] [--iters 100] [--warmup 10]
                               [--tile 0]

cases (each as _f64 and _f32):
    banded_1m    banded 1M x 1M, 14 per row, window 4096 (spal_synth)
    banded_10m   banded 10M x 10M, 140M entries: the config-3 size
    uniform_1m   1M x 1M, 14 draws per row with columns anywhere
    power_law    300k rows, power-law row lengths up to 5000, columns near the rows
Every case runs in a child process of its own under a time limit; the parent stops at the first child that does not
end normally.  Per k a record holds: ms per SpMM (device events around --iters launches after --warmup, three
repetitions: median, min, max); ms for the k SpMV launches, measured the same way in the same process (five
repetitions: median, min, max -- their spread is the noise the comparison has to clear); the ratio of the medians; the
algorithmic bytes nnz * (es + 4) + 4 * (nrows + 1) + es * k * (ncols + nrows) and their share of the 8 TB/s peak over
the SpMM time.  A matrix under 256 MB is rotated over several device copies, and X / Y (and the vectors of the
baseline) over two sets, so the Infinity Cache does not serve them.  Column 0 of one SpMM result is compared bit for
bit with the same sums done on the CPU (every row; numpy, one stored position of all rows at a time).  --tile forces a
column tile ("spmm_tile") to compare variants.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("banded_1m", "banded_10m", "uniform_1m", "power_law")
CASES = tuple(f"{k}_{t}" for k in KINDS for t in ("f64", "f32"))
PEAK_BYTES_PER_S = 8e12
CACHE_BYTES = 256 << 20


def from_keys(n, rows, cols, rng, dtype):
    import numpy as np
    key = np.unique(rows * n + cols)
    r2, c2 = key // n, key % n
    rp = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=n))]).astype(np.uint64)
    return rp, c2.astype(np.uint64), rng.uniform(-1, 1, c2.size).astype(dtype)


def make_case(name):
    import numpy as np
    import spal_synth as synth
    kind, t = name.rsplit("_", 1)
    dt = np.float64 if t == "f64" else np.float32
    if kind in ("banded_1m", "banded_10m"):
        n = 1_000_000 if kind == "banded_1m" else 10_000_000
        return n, synth.banded_csr(n, n, 14, 4096, synth.matrix_seed(3), dtype=dt)
    if kind == "uniform_1m":
        n = 1_000_000
        rng = np.random.default_rng(41)
        rows = np.repeat(np.arange(n, dtype=np.int64), 14)
        return n, from_keys(n, rows, rng.integers(0, n, rows.size), rng, dt)
    n = 300_000
    rng = np.random.default_rng(31)
    lens = np.minimum((rng.pareto(1.6, n) * 6 + 1).astype(np.int64), 5000)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = np.clip(rows - 5000 + rng.integers(0, 10000, rows.size), 0, n - 1)
    return n, from_keys(n, rows, cols, rng, dt)


def reference_column(rp, ci, va, x):
    """y = A * x with every row summed in stored order, the first product assigned (numpy multiplies and adds
    separately, like the kernels)"""
    import numpy as np
    rp = rp.astype(np.int64)
    lens = np.diff(rp)
    y = np.zeros(lens.size, dtype=va.dtype)
    rows = np.flatnonzero(lens > 0)
    t = 0
    while rows.size:
        idx = rp[rows] + t
        prod = va[idx] * x[ci[idx].astype(np.int64)]
        y[rows] = prod if t == 0 else y[rows] + prod
        t += 1
        rows = rows[lens[rows] > t]
    return y


def timed(launch, iters, warmup, reps):
    """ms per launch() over `iters` calls, `reps` times: [median, min, max]"""
    import numpy as np
    import torch
    st = torch.cuda.current_stream()
    for i in range(warmup):
        launch(i)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for i in range(iters):
            launch(i)
        e1.record(st)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "reps": reps}


def child(name, out_dir, ks, iters, warmup, tile):
    import numpy as np
    import torch
    import spalinalg_amd as sp
    n, (rp, ci, va) = make_case(name)
    es = va.dtype.itemsize
    tdt = torch.float64 if es == 8 else torch.float32
    nnz = int(rp[-1])
    matrix_bytes = nnz * (es + 4) + 4 * (n + 1)
    copies = 1 if matrix_bytes >= CACHE_BYTES else min(4, max(2, -(-3 * CACHE_BYTES // matrix_bytes)))
    A = sp.CsrMatrix(n, n, rp, ci, va)
    handles = [A.device_copy() for _ in range(copies)]
    for h in handles:
        h.set_option("spmm_tile", tile)
    st = torch.cuda.current_stream()
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": nnz, "matrix_bytes": matrix_bytes,
           "device_copies": copies, "vector_sets": 2, "iters": iters, "warmup": warmup, "forced_tile": tile,
           "spmv_plan": handles[0].describe().get("kernel"), "k": {}}
    gen = torch.Generator(device="cuda").manual_seed(7)
    for k in ks:
        Xs = [torch.rand((n, k), dtype=tdt, device="cuda", generator=gen) * 2 - 1 for _ in range(2)]
        Ys = [torch.empty((n, k), dtype=tdt, device="cuda") for _ in range(2)]
        xv = [torch.rand((k, n), dtype=tdt, device="cuda", generator=gen) * 2 - 1 for _ in range(2)]   # k vectors
        yv = [torch.empty((k, n), dtype=tdt, device="cuda") for _ in range(2)]
        xp = [[int(x[j].data_ptr()) for j in range(k)] for x in xv]
        yp = [[int(y[j].data_ptr()) for j in range(k)] for y in yv]
        Xp, Yp = [int(x.data_ptr()) for x in Xs], [int(y.data_ptr()) for y in Ys]

        def spmm(i):
            handles[i % copies].spmm_dev(k, Xp[i % 2], k, Yp[i % 2], k, st)

        def spmv_k(i):
            h, s = handles[i % copies], i % 2
            for j in range(k):
                h.spmv_dev(xp[s][j], yp[s][j], st)

        t_mm = timed(spmm, iters, warmup, 3)
        t_mv = timed(spmv_k, iters, warmup, 5)
        if k == ks[0]:     # column 0 of set 0 against the sequential sums on the CPU, every row, raw bits
            handles[0].spmm_dev(k, Xp[0], k, Yp[0], k, st)
            torch.cuda.synchronize()
            ref = reference_column(rp, ci, va, Xs[0][:, 0].contiguous().cpu().numpy())
            bits = np.uint64 if es == 8 else np.uint32
            rec["column0_bit_identical_to_cpu"] = bool(
                np.array_equal(Ys[0][:, 0].contiguous().cpu().numpy().view(bits), ref.view(bits)))
        alg = matrix_bytes + es * k * (n + n)
        rec["k"][str(k)] = {
            "spmm_ms": t_mm, "k_spmv_ms": t_mv, "ratio_k_spmv_over_spmm": t_mv["median"] / t_mm["median"],
            "spmm_faster_by_more_than_baseline_spread": bool(t_mv["median"] - t_mm["median"] > t_mv["max"] - t_mv["min"]),
            "algorithmic_bytes": alg, "share_of_peak": alg / (t_mm["median"] * 1e-3) / PEAK_BYTES_PER_S,
            "spmm": handles[0].describe()["spmm"]}
        del Xs, Ys, xv, yv
        torch.cuda.empty_cache()
    with open(os.path.join(out_dir, f"spmm_{name}.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tile", type=int, default=0, help="force the column tile (option spmm_tile); 0 = automatic")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    ks = [int(k) for k in args.ks.split(",")]
    if args.child:
        child(args.child, args.out, ks, args.iters, args.warmup, args.tile)
        return
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, "--ks", args.ks,
               "--iters", str(args.iters), "--warmup", str(args.warmup), "--tile", str(args.tile)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
