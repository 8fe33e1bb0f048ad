#!/usr/bin/env python3
"""Measures the KPM block step and eig_count on the device (spal_*_kpm_moments_*).  One JSON record per case
under --out DIR.  Development tool, not part of the package, the tests or bench.py.

    python tools/bench_kpm.py --out DIR [--cases poisson2d_1000_f64,...] [--part step|count|all]

step:  cases banded_1m_{f64,f32} and poisson2d_1000_{f64,f32}, the handles of tools/bench_eigsh_filter.py, at k = 1, 4, 8,
       16, 32 hashed probes.  t(d) = the call's device time (HIP events around its launches: info.solve_ms); a step is
       (t(34) - t(2)) / 16: 17 steps minus 1.  Three things in the same process, alternated round by round so that a
       drift of the machine meets all of them alike (round 0 warms up and is dropped; median, min and max of the rest):
         fused     "kpm_form" 1: the recurrence and the first level of both dots in the step kernel;
         unfused   "kpm_form" 2: the same block step, then a block dot launch;
         today     what the library offered before for the same work: k x (one cheb_series step + two spal_dot_dev
                   calls).  The series step is (t(17) - t(1)) / 16 of cheb_series_dev, the dots are timed on their own.
       Bytes a step must move: per pass over the matrix nnz * (sizeof(T) + 4) + 4 n, ceil(k / tile) passes; per column 4
       vectors of n values (t_{i-1} gathered and read by row, t_{i-2}, t_i written).  The copy ceiling is a device-to-
       device copy of 512 MiB timed in the same process.
count: a.eig_count on laplace1d_16k and poisson2d_1000 (f64) inside the main lobe of the delta filter of
       eigsh(sigma=...) at degree 256 and 4096, sigma = the middle of Gershgorin's interval + 0.1 of its width (DESIGN
       3.28's): the lobe is |theta - theta_sigma| < 2 pi / (D + 1), theta = arccos((x - c) / e).  The KPM degree is 4 D
       (at most 4096), 32 probes.  Both spectra are known in closed form, so the exact count stands beside the estimate.
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

STEP_CASES = ("poisson2d_1000_f64", "poisson2d_1000_f32", "banded_1m_f64", "banded_1m_f32")
COUNT_CASES = ("laplace1d_16k_f64", "poisson2d_1000_f64")
WIDTHS = (1, 4, 8, 16, 32)
ROUNDS = 5
COPY_BYTES = 512 << 20


def events(launch, iters):
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


def spread(values):
    import numpy as np
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def step_part(dev, n, nnz, es, rec):
    import numpy as np
    import torch
    import spalinalg_amd as sp
    st = torch.cuda.current_stream()
    tdt = torch.float64 if es == 8 else torch.float32
    glo, ghi = dev.gershgorin()
    m = (ghi - glo) / 1024
    lo, hi = glo - m, ghi + m
    xt = torch.rand(n, dtype=tdt, device="cuda")
    ot = torch.empty_like(xt)
    dt = torch.empty(1, dtype=tdt, device="cuda")
    coef = {d: sp.cheb_delta_coefficients(d, 0.2) for d in (1, 17)}
    src = torch.empty(COPY_BYTES, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    np_dt = np.float64 if es == 8 else np.float32

    def kpm(form, k, degree):
        dev.set_option("kpm_form", form)
        return dev.kpm_moments_dev(degree, k, seed=1, interval=(lo, hi), stream=st)[1].solve_ms

    def series_step():
        t1 = events(lambda: dev.cheb_series_dev(xt.data_ptr(), ot.data_ptr(), coef[1], lo, hi, st), 20)
        t17 = events(lambda: dev.cheb_series_dev(xt.data_ptr(), ot.data_ptr(), coef[17], lo, hi, st), 5)
        return (t17 - t1) / 16

    def two_dots():
        def run():
            sp.dot_dev(np_dt, xt.data_ptr(), ot.data_ptr(), n, dt.data_ptr(), stream=st)
            sp.dot_dev(np_dt, ot.data_ptr(), ot.data_ptr(), n, dt.data_ptr(), stream=st)
        return events(run, 20)

    steps = {(form, k): [] for form in (1, 2) for k in WIDTHS}
    series, dots, copy = [], [], []
    for rnd in range(ROUNDS + 1):                # round 0 warms every shape up and is dropped
        got = {}
        for k in WIDTHS:
            for form in (1, 2):
                got[form, k] = (kpm(form, k, 34) - kpm(form, k, 2)) / 16
        s, d2 = series_step(), two_dots()
        c = events(lambda: dst.copy_(src), 5)
        if rnd:
            for key, v in got.items():
                steps[key].append(v)
            series.append(s)
            dots.append(d2)
            copy.append(c)
    dev.set_option("kpm_form", 0)
    ceiling = 2 * COPY_BYTES / (float(np.median(copy)) * 1e-3) / 1e9
    today_step = float(np.median(series)) + float(np.median(dots))
    out = {"gershgorin": [glo, ghi], "interval": [lo, hi], "rounds": ROUNDS, "copy_ceiling_gbs": ceiling,
           "copy_ms": spread(copy), "series_step_ms": spread(series), "two_dots_ms": spread(dots), "widths": {}}
    matrix = nnz * (es + 4) + 4 * n
    for k in WIDTHS:
        tile = min(8, 1 << (k - 1).bit_length())
        passes = -(-k // tile)
        byts = passes * matrix + 4 * k * n * es
        fused, unfused = spread(steps[1, k]), spread(steps[2, k])
        today = k * today_step
        out["widths"][str(k)] = {
            "tile": tile, "passes": passes, "bytes": byts, "fused_step_ms": fused, "unfused_step_ms": unfused, "today_step_ms": today,
            "fused_gbs": byts / (fused["median"] * 1e-3) / 1e9, "fraction_of_copy_ceiling": byts / (fused["median"] * 1e-3) / 1e9 / ceiling,
            "fused_over_unfused": fused["median"] / unfused["median"], "fused_over_today": fused["median"] / today,
            "ms_per_column_step": fused["median"] / k}
    rec["step"] = out


def exact_spectrum(name):
    import numpy as np
    if name.startswith("laplace1d"):
        n = 16_384
        return 2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))
    one = 2.0 - 2.0 * np.cos(np.arange(1, 1001) * np.pi / 1001)
    return np.add.outer(one, one).ravel()


def count_part(a, name, rec):
    import numpy as np
    glo, ghi = a.gershgorin()
    m = (ghi - glo) / 1024
    lo, hi = glo - m, ghi + m
    c, e = (lo + hi) / 2, (hi - lo) / 2
    sigma = (glo + ghi) / 2 + 0.1 * (ghi - glo)
    th = np.arccos((sigma - c) / e)
    lam = exact_spectrum(name)
    out = {"gershgorin": [glo, ghi], "interval": [lo, hi], "sigma": sigma, "probes": 32, "lobes": {}}
    for D in (256, 4096):
        half = 2 * np.pi / (D + 1)
        lo_x, hi_x = c + e * np.cos(th + half), c + e * np.cos(th - half)
        degree = min(4 * D, 4096)
        est, se = a.eig_count(lo_x, hi_x, degree=degree, probes=32, seed=0, interval=(lo, hi))
        d = a.device().describe()["kpm"]
        out["lobes"][str(D)] = {"lobe": [float(lo_x), float(hi_x)], "kpm_degree": degree, "estimate": est, "standard_error": se,
                                "exact": int(((lam >= lo_x) & (lam <= hi_x)).sum()), "solve_ms": d["solve_ms"], "launches": d["launches"]}
    rec["count"] = out


def child(name, out_dir, part):
    import spalinalg_amd as sp
    from tools.bench_near import make
    n, rp, ci, va = make(name)
    es = va.dtype.itemsize
    a = sp.CsrMatrix(n, n, rp, ci, va)
    rec = {"case": name, "dtype": str(va.dtype), "n": n, "nnz": int(rp[-1])}
    if part == "step":
        step_part(a.device(), n, int(rp[-1]), es, rec)
    else:
        count_part(a, name, rec)
    print(json.dumps(rec[part]), flush=True)
    with open(os.path.join(out_dir, f"kpm_{part}_{name}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default="")
    ap.add_argument("--part", default="all", choices=("step", "count", "all"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case (its child process)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        child(args.child, args.out, args.part)
        return
    for part, cases in (("step", STEP_CASES), ("count", COUNT_CASES)):
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
