#!/usr/bin/env python3
"""Measures the sparse triangular solve (spal_csr_trsv_dev_*) over a sweep of its one option, "trsv_chain_rows", against
two yardsticks: one SpMV on the same handle (the same bytes with no dependencies: the floor) and torch's sparse-CSR
triangular solve where this torch build has one.  One JSON record per case under --out DIR.  Development tool, not part
of the package, the tests or bench.py.

    python tools/bench_trsv.py --out DIR [--cases banded_1m_f64,...] [--sweep 0,64,256,1024,4096,16384,huge]
                               [--iters 10] [--warmup 2] [--no-torch]

cases:
    banded_1m_{f64,f32}    1M x 1M, 14 draws per row in a window of 4096 around the diagonal, plus the diagonal
    banded_10m_{f64,f32}   10M x 10M, the same band: the config-3 size
    power_law_f64          300k rows, power-law row lengths up to 5000, columns near the rows
    bidiagonal_f64         100k rows, one sub- or super-diagonal: a chain of 100k one-row levels
Every case runs in a child process of its own under a time limit; the parent stops at the first child that does not end
normally.  Per triangle (lower, upper) a record holds the level statistics (spal_trsv_levels on the host arrays: levels,
rows per level min / mean / max, how many levels are at most 64 / 1024 / 4096 rows wide), the analysis time the handle
reports, and per threshold of the sweep: launches, chain launches and ms per solve (device events around --iters
solves after --warmup, three repetitions: median, min, max).  Off-diagonal values are uniform in (-1/16, 1/16) and the
diagonal is 1, so every row's off-diagonal sum is below 1 and x stays bounded.  Up to 1M rows one solve per triangle
is compared bit for bit with the sequential definition on the CPU (tests/trsv_ref.py, its level form).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("banded_1m_f64", "banded_1m_f32", "banded_10m_f64", "banded_10m_f32", "power_law_f64", "bidiagonal_f64")
HUGE = 1 << 40


def csr_from_rows(n, cols):
    """CSR pattern from an (n, m) array of column draws: sorted inside a row, duplicates dropped."""
    import numpy as np
    cols = np.sort(np.clip(cols, 0, n - 1), axis=1)
    keep = np.ones(cols.shape, dtype=bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.uint64)
    return rp, cols[keep].astype(np.uint64)


def make_case(name):
    import numpy as np
    kind, t = name.rsplit("_", 1)
    dt = np.float64 if t == "f64" else np.float32
    rng = np.random.default_rng(53)
    if kind in ("banded_1m", "banded_10m"):
        n = 1_000_000 if kind == "banded_1m" else 10_000_000
        draws = rng.integers(-2048, 2048, size=(n, 15), dtype=np.int32)
        draws[:, 0] = 0                                            # the diagonal
        draws += np.arange(n, dtype=np.int32)[:, None]
        rp, ci = csr_from_rows(n, draws)
    elif kind == "bidiagonal":
        n = 100_000
        i = np.arange(n, dtype=np.int64)
        rp, ci = csr_from_rows(n, np.stack([i - 1, i, i + 1], axis=1))
    else:
        n = 300_000
        lens = np.minimum((rng.pareto(1.6, n) * 6 + 1).astype(np.int64), 5000)
        rows = np.concatenate([np.repeat(np.arange(n, dtype=np.int64), lens), np.arange(n, dtype=np.int64)])
        cols = np.clip(rows - 5000 + rng.integers(0, 10000, rows.size), 0, n - 1)
        cols[-n:] = np.arange(n)                                   # the diagonal
        key = np.unique(rows * n + cols)
        rp = np.concatenate([[0], np.cumsum(np.bincount(key // n, minlength=n))]).astype(np.uint64)
        ci = (key % n).astype(np.uint64)
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rp.astype(np.int64)))
    scale = 16.0 if kind != "power_law" else 8192.0                # rows of up to 5000 entries: the sum stays below 1
    va = (rng.uniform(-1, 1, ci.size) / scale).astype(dt)
    va[rows == ci] = 1
    return n, rp, ci, va


def level_stats(n, rp, ci, uplo):
    import numpy as np
    from spalinalg_amd import _ffi
    level_of, nl = np.zeros(n, dtype=np.uint64), C.c_uint64()
    _ffi.check(_ffi.lib().spal_trsv_levels(C.c_uint64(n), rp.ctypes.data_as(_ffi.u64p), ci.ctypes.data_as(_ffi.u64p),
                                           uplo, 0, level_of.ctypes.data_as(_ffi.u64p), C.byref(nl)))
    w = np.bincount(level_of.astype(np.int64), minlength=nl.value)
    return {"levels": int(nl.value), "rows_per_level": {"min": int(w.min()), "mean": float(w.mean()), "max": int(w.max())},
            "levels_at_most": {str(t): int((w <= t).sum()) for t in (64, 1024, 4096)},
            "rows_in_levels_at_most": {str(t): int(w[w <= t].sum()) for t in (64, 1024, 4096)}}


def timed(launch, iters, warmup, reps=3):
    import numpy as np
    import torch
    st = torch.cuda.current_stream()
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(iters):
            launch()
        e1.record(st)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "reps": reps}


def torch_solve_ms(n, rp, ci, va, bt, upper, iters, warmup):
    """torch.triangular_solve with a sparse CSR matrix, or why it is not there."""
    import torch
    try:
        A = torch.sparse_csr_tensor(torch.from_numpy(rp.astype("int64")), torch.from_numpy(ci.astype("int64")),
                                    torch.from_numpy(va), size=(n, n)).cuda()
        B = bt.reshape(n, 1).contiguous()
        torch.triangular_solve(B, A, upper=upper)
        torch.cuda.synchronize()
        return timed(lambda: torch.triangular_solve(B, A, upper=upper), iters, warmup)
    except Exception as e:          # not built for this backend, or not for this layout
        return f"unavailable: {type(e).__name__}: {str(e).splitlines()[0][:160]}"


def child(name, out_dir, sweep, iters, warmup, use_torch):
    import numpy as np
    import torch
    import spalinalg_amd as sp
    n, rp, ci, va = make_case(name)
    es = va.dtype.itemsize
    nnz = int(rp[-1])
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    st = torch.cuda.current_stream()
    tdt = torch.float64 if es == 8 else torch.float32
    gen = torch.Generator(device="cuda").manual_seed(7)
    bt = torch.rand(n, dtype=tdt, device="cuda", generator=gen) * 2 - 1
    xt, yt = torch.empty_like(bt), torch.empty_like(bt)
    torch.cuda.synchronize()
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": nnz, "iters": iters, "warmup": warmup,
           "matrix_bytes": nnz * (es + 4) + 4 * (n + 1),
           "spmv_ms": timed(lambda: dev.spmv_dev(bt.data_ptr(), yt.data_ptr(), st), max(iters, 20), warmup + 3),
           "spmv_plan": dev.describe().get("kernel"), "triangles": {}}
    for uplo, key in ((0, "lower"), (1, "upper")):
        lower = uplo == 0
        tri = {"level_stats": level_stats(n, rp, ci, uplo), "sweep": {}}
        for thr in sweep:
            dev.set_option("trsv_chain_rows", thr)
            t = timed(lambda: dev.trsv_dev(bt.data_ptr(), xt.data_ptr(), lower, False, st), iters, warmup)
            d = dev.describe()["trsv"][key]
            tri["sweep"]["huge" if thr == HUGE else str(thr)] = {
                "ms": t, "launches": d["launches"], "chain_launches": d["chain_launches"],
                "over_spmv": t["median"] / rec["spmv_ms"]["median"]}
            tri["analysis_ms"] = d["analysis_ms"]
        if n <= 1_000_000:
            from tests import trsv_ref
            ref = trsv_ref.solve_by_levels(n, rp, ci, va, bt.cpu().numpy(), lower=lower)
            bits = np.uint64 if es == 8 else np.uint32
            tri["bit_identical_to_cpu"] = bool(np.array_equal(xt.cpu().numpy().view(bits), ref.view(bits)))
        else:
            tri["bit_identical_to_cpu"] = None
        tri["torch_triangular_solve_ms"] = (torch_solve_ms(n, rp, ci, va, bt, not lower, max(2, iters // 3), 1)
                                            if use_torch else "not run")
        rec["triangles"][key] = tri
    with open(os.path.join(out_dir, f"trsv_{name}.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--sweep", default="0,64,256,1024,4096,16384,huge")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true", help="skip torch.triangular_solve")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    sweep = [HUGE if s == "huge" else int(s) for s in args.sweep.split(",")]
    if args.child:
        child(args.child, args.out, sweep, args.iters, args.warmup, not args.no_torch)
        return
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, "--sweep", args.sweep,
               "--iters", str(args.iters), "--warmup", str(args.warmup)] + (["--no-torch"] if args.no_torch else [])
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
