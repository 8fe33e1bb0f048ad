#!/usr/bin/env python3
"""Measures the triangular solves for a block of k right-hand sides (spal_csr_trsm_dev_*, spal_csr_trsm_sweep_dev_*,
DESIGN 3.20) against k single-vector calls on the same handle, in the same process.  One JSON record per case under
--out DIR.  Development tool, not part of the package, the tests or bench.py; no time in it is a pass criterion.

    python tools/bench_trsm.py --out profiles/trsm [--cases banded_1m_f64,banded_1m_f32] [--widths 1,2,4,8,16,32]
                               [--iters 5] [--warmup 1]

cases (the input of tools/bench_colour.py):
    banded_1m_{f64,f32}      1M x 1M, 14 draws per row in a window of 4096 around the diagonal, plus the diagonal
Every case runs in a child process of its own under a time limit; the parent stops at the first child that does not end
normally.  A record holds, for the matrix in its natural order (thousands of narrow levels: the solve is bound by the
latency of a level) and after multicolour() (a handful of wide levels), the levels and launches of the lower triangle and
per width k:
    exact   ms of one block solve of the lower triangle, ms of k vector solves (spal_csr_trsv_dev_*), their ratio
    sweep   the same for one Jacobi pass (sweeps = 1: the scaling and one pass; spal_csr_trsv_sweep_dev_* k times)
Device events around --iters calls after --warmup, three repetitions: median, min, max.  The vector calls' code is the
single-vector solve as it was before the block solves existed.  Column 0 of every block result is compared bit for bit
with the vector call's.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_trsv import timed  # noqa: E402

CASES = ("banded_1m_f64", "banded_1m_f32")


def side(dev, n, widths, tdt, st, iters, warmup):
    """Both forms on one handle, per width: block call against k vector calls, exact and one sweep pass."""
    import torch
    plan = dev.trsv_analyse(lower=True, stream=st)["lower"]
    rec = {"levels": plan["levels"], "launches": plan["launches"], "max_level_rows": plan["max_level_rows"],
           "analysis_ms": plan["analysis_ms"], "exact": {}, "sweep": {}}
    gen = torch.Generator(device="cuda").manual_seed(7)
    for k in widths:
        B = torch.rand((n, k), dtype=tdt, device="cuda", generator=gen) * 2 - 1
        X = torch.empty_like(B)
        cols = B.t().contiguous()                      # the k right-hand sides as vectors
        xs = torch.empty_like(cols)
        torch.cuda.synchronize()
        bp, xp = B.data_ptr(), X.data_ptr()
        vec = [(cols[j].data_ptr(), xs[j].data_ptr()) for j in range(k)]

        def exact_vectors():
            for b, x in vec:
                dev.trsv_dev(b, x, True, False, st)

        def sweep_vectors():
            for b, x in vec:
                dev.trsv_sweep_dev(b, x, 1, True, False, st)

        for key, block, vectors in (("exact", lambda: dev.trsm_dev(k, bp, k, xp, k, True, False, st), exact_vectors),
                                    ("sweep", lambda: dev.trsm_sweep_dev(k, bp, k, xp, k, 1, True, False, st), sweep_vectors)):
            it = iters if key == "exact" else max(iters, 20)
            tb, tv = timed(block, it, warmup), timed(vectors, it, warmup)
            same = bool(torch.equal(X[:, 0].contiguous().view(torch.uint8), xs[0].view(torch.uint8)))
            d = dev.describe()["trsm"]
            rec[key][str(k)] = {"block_ms": tb, "vector_calls_ms": tv, "block_over_vectors": tb["median"] / tv["median"],
                                "tile": d["tile"], "launches": d["launches"], "column_0_bit_identical": same}
    return rec


def child(name, out_dir, widths, iters, warmup):
    import torch
    import spalinalg_amd as sp
    from tools.bench_colour import make_case
    n, rp, ci, va = make_case(name)
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    st = torch.cuda.current_stream()
    tdt = torch.float64 if va.dtype.itemsize == 8 else torch.float32
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": int(rp[-1]), "iters": iters, "warmup": warmup,
           "widths": widths, "natural": side(dev, n, widths, tdt, st, iters, warmup)}
    p = dev.multicolour(0, st)
    rec["colours"] = p.describe()["ordering"]["colours"]
    rec["multicolour"] = side(p, n, widths, tdt, st, max(iters, 20), warmup)
    with open(os.path.join(out_dir, f"trsm_{name}.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--widths", default="1,2,4,8,16,32")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    widths = [int(w) for w in args.widths.split(",")]
    if args.child:
        child(args.child, args.out, widths, args.iters, args.warmup)
        return
    for name in args.cases.split(","):
        if name not in CASES:
            sys.exit(f"unknown case {name!r} (one of {', '.join(CASES)})")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, "--widths", args.widths,
               "--iters", str(args.iters), "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
        if rc != 0:
            sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
