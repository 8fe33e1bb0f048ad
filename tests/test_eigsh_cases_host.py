"""CPU tests that keep tests/test_gpu_eigsh_fuzz.py honest: the text (tests/eigsh_ref.py) alone, with a host product, does
on the directed cases of tests/eigsh_cases.py what they were built for -- exhaustion at step L, stop 2 in the middle of a
phase and after restarts, rotation tiles of 512 and 1024 rows and more tiles than workgroups; the default seeds of the
fuzz reach both reasons, every batch position, all value classes; and on the small seeds the text's values are the
eigenvalues numpy.linalg.eigvalsh finds."""
import os
import re

import numpy as np
import pytest

from tests import eigsh_cases as ec
from tests import eigsh_ref as er
from tests.test_eigsh_host import lib_jacobi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spalinalg_amd", "csrc")
SEEDS = range(ec.DEFAULT_SEEDS)
DTYPES = [np.float64, np.float32]


def run(mat, dtype, k, which, ncv, tol, maxit, v0=None, seed=0):
    return er.eigsh(ec.host_mul(mat), mat[0], dtype, k, which, ncv, tol, maxit, v0, seed, lib_jacobi)


# ---- the kernel's constants and the tiles they give ------------------------------------------------------------------

def test_rotation_constants_are_the_kernels():
    text = open(os.path.join(CSRC, "spal_eigsh.hip")).read()
    assert int(re.search(r"kRotMinRows = (\d+);", text).group(1)) == ec.ROT_MIN_ROWS
    m = re.search(r"kRotLdsTarget = (\d+) \* (\d+);", text)
    assert int(m.group(1)) * int(m.group(2)) == ec.ROT_LDS_TARGET
    assert int(re.search(r"kRotMaxGrid = (\d+);", text).group(1)) == ec.ROT_MAX_GRID
    assert re.search(r"while \(r < kTile && \(size_t\)2 \* r \* m \* sizeof\(T\) <= kRotLdsTarget\) r \*= 2;", text)
    tile = re.search(r"constexpr uint64_t kTile = (\d+);", open(os.path.join(CSRC, "krylov_kernels.hpp")).read())
    assert int(tile.group(1)) == ec.ROT_MAX_ROWS


def test_rotation_cases_have_the_tiles_they_are_there_for():
    seen = set()
    for n, ncv in ec.ROTATION_TILES:
        for dtype in DTYPES:
            rows = ec.rot_tile_rows(ncv, np.dtype(dtype).itemsize)
            seen.add(rows)
            assert rows in (512, 1024) and -(-n // rows) >= 2 and n % rows != 0, (n, ncv, rows)
    assert seen == {512, 1024}
    assert [ec.rot_tile_rows(m, 8) for m in (2, 3, 4)] == [1024, 512, 512]
    assert [ec.rot_tile_rows(m, 4) for m in (2, 3, 4)] == [1024, 1024, 1024]
    assert [ec.rot_tile_rows(m, 8) for m in (8, 16, 17, 256)] == [256, 128, 64, 64]
    # more tiles than the rotation's grid has workgroups, by one: the smallest such size
    mt = ec.MANY_TILES
    assert ec.rot_tile_rows(mt["ncv"], 8) == 64 and ec.rot_tile_rows(mt["ncv_f32"], 4) == 64
    assert ec.rot_tile_rows(mt["ncv"], 4) == 128                    # (f32 at ncv = 17: 4097 tiles, one per workgroup)
    assert -(-mt["n"] // 64) == ec.ROT_MAX_GRID + 1 and -(-(mt["n"] - 1) // 64) == ec.ROT_MAX_GRID


# ---- exhaustion ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("L", ec.EXHAUSTION_L)
def test_exhaustion_falls_at_step_L(L, dtype):
    mat = ec.exhaustion(L, dtype)
    n, ncv = ec.EXHAUSTION_N, ec.EXHAUSTION_NCV
    v0 = ec.e0(n, dtype)
    r = run(mat, dtype, 3, "LA", ncv, 1e-6, 5, v0)
    assert (r["products"], r["restarts"]) == (L, 0)
    assert (r["reason"], r["pairs"]) == ((0, 3) if L >= 3 else (3, L))
    r = run(mat, dtype, L + 1, "SA", ncv, 1e-6, 5, v0)
    assert (r["products"], r["restarts"], r["reason"], r["pairs"]) == (L, 0, 3, L)
    # all arithmetic is exact: the vectors found span e_0 .. e_{L-1}, and the values are those of the leading block
    assert not r["X"][L:].any()
    lam = np.linalg.eigvalsh(ec.dense(mat)[:L, :L])
    assert np.allclose(r["theta"], lam, rtol=1e-5 if dtype == np.float32 else 1e-12)


# ---- stop 2 ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_overflow_stops_in_the_middle_of_a_phase_and_after_restarts(dtype):
    n, k = ec.OVERFLOW_N, ec.OVERFLOW_K
    v0 = ec.e0(n, dtype)
    for p in ec.OVERFLOW_P:
        mat = ec.overflow(p, dtype)
        assert np.isfinite(mat[3]).all()
        r = run(mat, dtype, k, "LA", ec.OVERFLOW_NCV, 1e-6, 5, v0)
        assert (r["reason"], r["products"], r["restarts"], r["pairs"], r["converged"]) == (2, p + 1, 0, 0, 0), (p, r)
    o = ec.OVERFLOW_RESTARTED
    r = run(ec.overflow(o["p"], dtype), dtype, k, "LA", o["ncv"], 1e-6, 5, v0)
    assert (r["reason"], r["products"], r["restarts"]) == (2, o["products"], o["restarts"])
    # the call that follows on the device is a good one: the same path without the large coupling
    r = run(ec.exhaustion(n, dtype), dtype, k, "LA", ec.OVERFLOW_NCV, 1e-6, 5, v0)
    assert r["reason"] in (0, 1) and r["pairs"] == k


# ---- ncv == n --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,k", ec.FULL_BASIS)
def test_a_basis_of_the_whole_space(n, k, dtype):
    mat = ec.banded(n, dtype)
    r = run(mat, dtype, k, "LA", n, ec.default_tol(dtype) * 100, 1)
    assert r["reason"] in (0, 1, 3) and r["pairs"] == k and r["products"] >= n
    if r["reason"] == 0:
        lam = np.linalg.eigvalsh(ec.dense(mat))[::-1][:k]
        assert np.allclose(r["theta"], lam, rtol=1e-4 if dtype == np.float32 else 1e-10)


# ---- the fuzz --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_seed_is_a_valid_symmetric_input(seed):
    mat, k = ec.case(seed)
    n, rowptr, colind, values = mat
    assert n == ec.N_TABLE[seed % len(ec.N_TABLE)] == k["n"] and values.dtype == k["dtype"] and np.isfinite(values).all()
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    cols = colind.astype(np.int64)
    same_row = rows[1:] == rows[:-1]
    assert np.all(cols[1:][same_row] > cols[:-1][same_row])
    order = np.lexsort((rows, cols))                                # the transpose, entry by entry
    assert np.array_equal(rows[order], cols) and np.array_equal(cols[order], rows)
    assert values[order].tobytes() == values.tobytes(), "the matrix must be symmetric"
    assert 0 < k["k"] < k["ncv"] <= min(n, 256) and k["ncv"] == min(ec.NCV_TABLE[(5 * seed + seed // 12) % len(ec.NCV_TABLE)], n)
    assert k["k"] in (1, max(k["ncv"] // 2, 1), k["ncv"] - 1) and k["which"] in ("LA", "SA") and k["rotate"] in (1, 2)
    assert k["tol"] in (0.0, ec.TOL[k["dtype"]], 1e-2) and k["maxit"] in ec.MAXIT + (ec.SMALL_MAXIT,)
    assert k["v0"] is None or (k["v0"].dtype == k["dtype"] and k["v0"].shape == (n,) and not k["v0"].flags.writeable)
    assert k["seed"] in ec.SEEDS and (k["jacobi"] == "lib") == (k["ncv"] > 24)
    assert not any(a.flags.writeable for a in mat[1:])
    diag = values[rows == cols].astype(np.float64)
    big = float(np.abs(values).max())
    if k["cls"] == "indefinite" and n > 2:
        assert diag.min() < 0 < diag.max() and abs(diag.mean()) < 1e-5 * np.abs(diag).max()
    if k["cls"] == "scaled_down":
        assert big < 1e-10
    if k["cls"] == "scaled_up":
        assert big > 1e10
    if k["cls"] == "clustered":
        assert np.unique(diag).size <= 4 and (n == 1 or np.abs(values[rows != cols]).max() <= 1e-6)


def test_default_seeds_reach_what_the_device_test_is_there_for():
    """Over the default seeds: reasons 0 and 1, keep and ncv below, at and above the batch of 8, the five value classes,
    both kinds, dtypes, rotation forms and start vectors; and on the seeds with n <= 300 the text's values are
    numpy.linalg.eigvalsh's, unless the text did not converge -- which at most a third of them may."""
    reasons, keeps, ncvs, classes = set(), set(), set(), set()
    kinds, dtypes, forms, starts, seeds, jacobis, whiches = set(), set(), set(), set(), set(), set(), set()
    eligible = compared = 0
    for seed in SEEDS:
        mat, k = ec.case(seed)
        dtype = k["dtype"].type
        tol = k["tol"] or ec.default_tol(dtype)
        r = ec.text(mat, k, jacobi_fn=lib_jacobi)
        reasons.add(r["reason"]), keeps.add(er.keep_of(k["k"], k["ncv"])), ncvs.add(k["ncv"]), classes.add(k["cls"])
        kinds.add(k["kind"]), dtypes.add(k["dtype"].name), forms.add(k["rotate"]), starts.add(k["v0"] is None)
        seeds.add(k["seed"] >= 2**32), jacobis.add(k["jacobi"]), whiches.add(k["which"])
        line = (f"eigsh seed {seed}: n {k['n']} {k['cls']} {k['dtype'].name} ncv {k['ncv']} k {k['k']} {k['which']} tol {tol:.1e} "
                f"maxit {k['maxit']} -> reason {r['reason']} restarts {r['restarts']} products {r['products']}")
        if k["n"] > ec.SMALL:
            print(line)
            continue
        eligible += 1
        if r["reason"] != 0:
            print(line, "(not converged: not compared)")
            continue
        compared += 1
        a = ec.dense(mat)
        lam = np.linalg.eigvalsh(a)
        scale = np.abs(lam).max()
        by_which = lam[::-1] if k["which"] == "LA" else lam
        nk = r["pairs"]
        x64, t64 = r["X"].astype(np.float64), r["theta"].astype(np.float64)
        res = np.linalg.norm(a @ x64 - x64 * t64, axis=0) / np.linalg.norm(x64, axis=0)
        slack = res + (1e-12 + np.finfo(dtype).eps) * scale
        nearest = np.abs(t64[:, None] - lam[None, :]).min(axis=1)
        err = np.abs(t64 - by_which[:nk])
        print(line, f"residual {res.max() / scale:.1e} |theta - lambda| {err.max() / scale:.1e} of max|lambda|")
        assert np.all(res <= 2 * tol * scale), (seed, res / scale)
        assert np.all(nearest <= slack), (seed, nearest, slack)     # a residual r puts an eigenvalue within r of theta
        if k["cls"] != "clustered":
            assert np.all(err <= slack), (seed, err, slack)
            continue
        # A cluster (one diagonal value, spread by the 1e-6 coupling) may come back once or member by member
        # (consequence 4 of the header).  Either way the j-th value is no more extreme than the j-th eigenvalue (Ritz
        # values interlace) and no less extreme than the j-th DISTINCT value.
        distinct = by_which[np.concatenate([[True], np.abs(np.diff(by_which)) > 1e-3])]
        sign = 1.0 if k["which"] == "LA" else -1.0
        assert np.all(sign * (t64 - by_which[:nk]) <= slack), (seed, t64, by_which[:nk])
        m = min(nk, distinct.size)
        assert np.all(sign * (distinct[:m] - t64[:m]) <= slack[:m] + 1e-4), (seed, t64, distinct[:m])   # (1e-4: a cluster's width)
    print(f"compared {compared} of {eligible} seeds with n <= {ec.SMALL}; reasons {sorted(reasons)}; keep {sorted(keeps)}; ncv {sorted(ncvs)}")
    assert reasons == {0, 1}
    for sizes in (keeps, ncvs):
        assert min(sizes) < 8 and 8 in sizes and max(sizes) > 8
    assert any(s > 16 for s in keeps) and any(s > 64 for s in ncvs)
    assert classes == set(ec.CLASSES) and kinds == {"csr", "csc"} and dtypes == {"float64", "float32"} and forms == {1, 2}
    assert starts == {True, False} and seeds == {True, False} and jacobis == {"lib", "numpy"} and whiches == {"LA", "SA"}
    assert eligible >= 12 and 3 * (eligible - compared) <= eligible, (compared, eligible)
