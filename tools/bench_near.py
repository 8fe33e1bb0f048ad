#!/usr/bin/env python3
"""Measures the Chebyshev series step and eigsh near sigma on the device (spal_*_cheb_series_*, spal_*_eigsh_near_*,
DESIGN 3.28).  One JSON record per case under --out DIR.  Development tool, not part of the package, the tests or bench.py.

    python tools/bench_near.py --out DIR [--cases poisson2d_1000_f64,...] [--part step|solve|all]

step:  cases banded_1m_{f64,f32} and poisson2d_1000_{f64,f32}, the handles of tools/bench_eigsh_filter.py.  t(d) = device
       time (HIP events) of one call at degree d; a step is (t(17) - t(1)) / 16.  Three forms in the same run, alternated
       round by round so that a drift of the machine meets all of them alike:
         fused     cheb_series_dev with "cheb_series_form" 1: the accumulation in the step kernel's epilogue;
         unfused   the same call with "cheb_series_form" 2: the recurrence step and a separate accumulation launch;
         apply     cheb_apply_dev, the filter's recurrence step: the yardstick (it moves two vector streams fewer).
       Bytes a step must move: nnz * (sizeof(T) + 4) + 4 n for the matrix, then per vector of n values: apply 3 (y
       gathered, x, out), fused 5 (y, x, t, s read, s written), unfused 6 (apply's 3, then t, s read, s written).
solve: eigsh(k=6, sigma = the middle of Gershgorin's interval + 0.1 of its width, filter_degree=256, ncv=30, tol=1e-8,
       maxit=50) in f64 on poisson2d_1000 (the eigenvalue spacing mid-spectrum is far below the resolution of degree
       256: expected NOT to converge) and on laplace1d_1m (the 1-D Laplacian of 1M rows; its spacing mid-spectrum is
       6e-6, so the same holds); then the same call at filter_degree=4096 on laplace1d_16k (16 384 rows: spacing 3.8e-4
       against a resolution of 9.8e-4, the size this method resolves); restarts, products, ms, converged, reason, the
       residuals.
Every case runs in a child process of its own under a time limit; the parent stops at the first child that does not end
normally.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_CASES = ("banded_1m_f64", "banded_1m_f32", "poisson2d_1000_f64", "poisson2d_1000_f32")
SOLVE_CASES = ("poisson2d_1000_f64", "laplace1d_1m_f64", "laplace1d_16k_f64")
SOLVE_DEGREE = {"laplace1d_16k_f64": 4096}     # 256 elsewhere
ROUNDS = 5


def make(name):
    import numpy as np
    if name.startswith("laplace1d"):
        n = 16_384 if "16k" in name else 1_000_000
        i = np.arange(n, dtype=np.int64)
        rows = np.concatenate([i[1:], i, i[:-1]])
        cols = np.concatenate([i[1:] - 1, i, i[:-1] + 1])
        vals = np.concatenate([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)])
        order = np.lexsort((cols, rows))
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.uint64)
        return n, rowptr, cols[order].astype(np.uint64), vals[order]
    from tools.bench_eigsh import make as make_eigsh
    return make_eigsh(name)


def once(launch, iters):
    """device ms per call over `iters` calls between two events"""
    import torch
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters):
        launch()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def step_part(dev, n, nnz, es, rec):
    import numpy as np
    import torch
    import spalinalg_amd as sp
    st = torch.cuda.current_stream()
    tdt = torch.float64 if es == 8 else torch.float32
    xt = torch.rand(n, dtype=tdt, device="cuda")
    ot = torch.empty_like(xt)
    glo, ghi = dev.gershgorin()
    m = (ghi - glo) / 1024
    lo, hi = glo - m, ghi + m
    coef = {d: sp.cheb_delta_coefficients(d, 0.2) for d in (1, 17)}
    a0 = hi + 0.1 * (hi - lo)

    def series(form, d):
        def run():
            dev.cheb_series_dev(xt.data_ptr(), ot.data_ptr(), coef[d], lo, hi, st)
        return form, run

    forms = {"fused": 1, "unfused": 2}
    calls = {}
    for name, form in forms.items():
        for d in (1, 17):
            calls[name, d] = series(form, d)
    for d in (1, 17):
        calls["apply", d] = (None, (lambda d=d: dev.cheb_apply_dev(xt.data_ptr(), ot.data_ptr(), d, lo, hi, a0, st)))
    ms = {key: [] for key in calls}
    for rnd in range(ROUNDS + 1):                # round 0 warms every shape up and is dropped
        for key, (form, run) in calls.items():
            if form is not None:
                dev.set_option("cheb_series_form", form)
            t = once(run, 40 if key[1] == 1 else 10)
            if rnd:
                ms[key].append(t)
    dev.set_option("cheb_series_form", 0)
    matrix = nnz * (es + 4) + 4 * n
    vectors = {"apply": 3, "fused": 5, "unfused": 6}
    out = {"gershgorin": [glo, ghi], "interval": [lo, hi], "rounds": ROUNDS}
    for name in ("fused", "unfused", "apply"):
        t1, t17 = float(np.median(ms[name, 1])), float(np.median(ms[name, 17]))
        steps = [(b - a) / 16 for a, b in zip(ms[name, 1], ms[name, 17])]
        byts = matrix + vectors[name] * n * es
        step = (t17 - t1) / 16
        out[name] = {"first_step_ms": t1, "degree17_ms": t17, "step_ms": step, "step_ms_min": min(steps), "step_ms_max": max(steps),
                     "bytes": byts, "gbs": byts / (step * 1e-3) / 1e9}
    out["fused_over_unfused"] = out["fused"]["step_ms"] / out["unfused"]["step_ms"]
    out["fused_over_apply"] = out["fused"]["step_ms"] / out["apply"]["step_ms"]
    out["bytes_fused_over_apply"] = out["fused"]["bytes"] / out["apply"]["bytes"]
    rec["step"] = out


def solve_part(dev, rec, degree):
    import numpy as np
    glo, ghi = dev.gershgorin()
    sigma = (glo + ghi) / 2 + 0.1 * (ghi - glo)
    theta, _, info = dev.eigsh(6, ncv=30, tol=1e-8, maxit=50, return_eigenvectors=False, sigma=sigma, filter_degree=degree)
    rec["solve"] = {"k": 6, "sigma": sigma, "degree": degree, "ncv": 30, "tol": 1e-8, "maxit": 50, "gershgorin": [glo, ghi],
                    "lo": info.lo, "hi": info.hi, "gamma": info.gamma, "restarts": info.restarts, "products": info.products,
                    "solve_ms": info.solve_ms, "converged": info.converged, "reason": info.reason,
                    "theta": [float(t) for t in theta], "resid": [float(r) for r in info.resid],
                    "largest_resid": float(np.max(info.resid)) if len(info.resid) else None,
                    "tol_times_scale": 1e-8 * max(abs(glo), abs(ghi)),
                    "resolution": (info.hi - info.lo) / degree}


def child(name, out_dir, part):
    import spalinalg_amd as sp
    n, rp, ci, va = make(name)
    es = va.dtype.itemsize
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": int(rp[-1])}
    if part == "step":
        step_part(dev, n, int(rp[-1]), es, rec)
    else:
        solve_part(dev, rec, SOLVE_DEGREE.get(name, 256))
    print(json.dumps(rec[part]), flush=True)
    with open(os.path.join(out_dir, f"eigsh_near_{part}_{name}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default="")
    ap.add_argument("--part", default="all", choices=("step", "solve", "all"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        child(args.child, args.out, args.part)
        return
    for part, cases in (("step", STEP_CASES), ("solve", SOLVE_CASES)):
        if args.part not in (part, "all"):
            continue
        for name in (args.cases.split(",") if args.cases else cases):
            if name not in cases:
                if args.part == "all":
                    continue
                sys.exit(f"unknown case {name!r} of part {part} (one of {', '.join(cases)})")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", args.out, "--part", part]
            try:
                rc = subprocess.run(cmd, timeout=args.timeout).returncode
            except subprocess.TimeoutExpired:
                sys.exit(f"case {name}: no result within {args.timeout} s; stopping")
            if rc != 0:
                sys.exit(f"case {name}: exit status {rc}; stopping")


if __name__ == "__main__":
    main()
