"""FSAI without a device: spal_fsai_row_* (the library's host text) against tests/fsai_ref.py bit for bit, the reference
itself against what FSAI promises (unit diagonal of G A Gt, no rejection on SPD matrices, fewer CG iterations with a
denser pattern), the fuzz generator's share of wholly rejected cases, and the new symbols of the ABI."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import fsai_ref as fr
from tests import krylov_ref as kr
from tests import trsv_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float64, np.float32]
SIZES = [1, 2, 3, 7, 13, 33, 64]
FUZZ_SEED, FUZZ_CASES = 20261021, 40


def same_row(B, dtype):
    g, rejected = sp.fsai_row(fr.pack_lower(np.asarray(B, dtype=dtype)))
    g_ref, rejected_ref = fr.row(B, dtype)
    assert g.dtype == dtype and rejected == rejected_ref
    tr.assert_same_bits(g, g_ref)
    return g, rejected


def spd_dominant(m, dtype, seed):
    return fr.dense(fr.dense_spd(m, dtype, seed)).astype(dtype)


def spd_random(m, dtype, seed):
    X = np.random.default_rng(seed).standard_normal((m, m + 3))
    return (X @ X.T + 0.5 * np.eye(m)).astype(dtype)


def poisson_block(m, dtype):
    """the leading m x m principal submatrix of Poisson 8 x 8"""
    return fr.dense(fr.poisson2d(8, dtype))[:m, :m].astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("build", [spd_dominant, spd_random], ids=["dominant", "random"])
def test_row_is_the_text_on_spd_systems(build, m, dtype):
    B = build(m, dtype, m)
    g, rejected = same_row(B, dtype)
    assert rejected == 0
    # g solves the row's system up to rounding: (B g)[m - 1] = g[m - 1], the others 0 (g = C^-T e_m / C[m-1, m-1])
    full = np.tril(B.astype(np.float64)) + np.tril(B.astype(np.float64), -1).T
    res = full @ g.astype(np.float64)
    res[m - 1] -= 1.0 / g.astype(np.float64)[m - 1]
    assert np.abs(res).max() <= 64 * m * np.finfo(dtype).eps * np.linalg.cond(full) * np.abs(g).max() * np.abs(full).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("m", SIZES)
def test_row_is_the_text_on_poisson_blocks(m, dtype):
    _, rejected = same_row(poisson_block(m, dtype), dtype)
    assert rejected == 0


def rejected_cases(dtype):
    P = poisson_block(7, dtype)
    first = P.copy()
    first[0, 0] = -4
    zero_first = P.copy()
    zero_first[0, 0] = 0
    last = P.copy()
    last[6, 6] = -4
    cancel = np.array([[1, 0, 0], [1, 1, 0], [0, 0, 3]], dtype=dtype)        # d_1 = 1 - 1 * 1 = 0
    cancel_neg = np.array([[1, 0, 0], [2, 1, 0], [0, 0, 3]], dtype=dtype)    # d_1 = 1 - 4 < 0
    nan = P.copy()
    nan[3, 1] = np.nan
    inf = P.copy()
    inf[6, 6] = np.inf
    inf_first = P.copy()
    inf_first[0, 0] = np.inf
    zero = np.array([[0.0]], dtype=dtype)
    cases = {"first": first, "zero_first": zero_first, "last": last, "cancel": cancel, "cancel_neg": cancel_neg,
             "nan": nan, "inf": inf, "inf_first": inf_first, "zero": zero}
    if dtype == np.float32:
        cases["overflow"] = overflow_ladder()
    return cases


def overflow_ladder(m=13):
    """f32: B = 2^-146 L Lt with L unit lower bidiagonal, -32 below the diagonal.  Every value of the factorisation is a
    power of two (C = 2^-73 L, exactly, through subnormal numbers), every pivot is positive, and g[t] = 2^(73 + 5 (m -
    1 - t)): 1 / C times the ladder passes 2^128 from t = 1 down, so g is not finite and the row is rejected AFTER a
    complete factorisation.  (1 / C[m-1, m-1] alone cannot overflow: the smallest positive f32 has the root 3.7e-23.)"""
    L = np.eye(m) - 32.0 * np.eye(m, k=-1)
    B = (L @ L.T) * 2.0 ** -146
    assert np.array_equal(B.astype(np.float32).astype(np.float64), B)
    return B.astype(np.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_row_rejections_are_the_text(dtype):
    for name, B in rejected_cases(dtype).items():
        g, rejected = same_row(B, dtype)
        assert rejected == 1, name
        assert np.all(g[:-1] == 0) and np.isfinite(g[-1]) and g[-1] > 0, name
        aii = B[-1, -1]
        if aii > 0 and np.isfinite(aii):
            tr.assert_same_bits(g[-1:], (dtype(1) / np.sqrt(aii.astype(dtype))).reshape(1))
        else:
            assert g[-1] == 1, name
    if dtype == np.float32:
        # the ladder one step shorter than the overflow is a valid row: the rejection above is the overflow's
        g, rejected = same_row(overflow_ladder(11), dtype)
        assert rejected == 0 and g[0] == np.float32(2.0 ** 123)


def test_row_refusals():
    lib = _ffi.lib()
    g = np.zeros(4)
    b = np.ones(10)
    rej = C.c_int(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                              # noqa: E731
    assert lib.spal_fsai_row_f64(_ffi.u64(0), p(b), p(g), C.byref(rej)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert "m = 0" in lib.spal_last_error().decode()
    assert lib.spal_fsai_row_f64(_ffi.u64(65), p(b), p(g), C.byref(rej)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert lib.spal_fsai_row_f64(_ffi.u64(4), None, p(g), C.byref(rej)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert lib.spal_fsai_row_f64(_ffi.u64(4), p(b), None, C.byref(rej)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert lib.spal_fsai_row_f32(_ffi.u64(4), p(b), p(g), None) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    with pytest.raises(sp.Panic):
        sp.fsai_row(np.ones(4))                     # 4 values are no packed triangle
    with pytest.raises(sp.Panic):
        sp.fsai_row(np.ones((2, 3)))
    # handles: null arguments are refused before any device is looked for
    out = C.c_void_p()
    assert lib.spal_csr_fsai_setup(None, None, None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert lib.spal_csc_fsai_setup(None, None, None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert lib.spal_fsai_destroy(None) == _ffi.SPAL_OK
    buf = C.create_string_buffer(64)
    assert lib.spal_fsai_describe(None, buf, C.c_size_t(64)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert lib.spal_fsai_factor_csr(None, C.c_int(0), C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    x = np.zeros(4)
    assert lib.spal_fsai_apply_f64(None, p(x), _ffi.u64(4), p(g), _ffi.u64(4)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert lib.spal_fsai_apply_dev_f32(None, p(x), p(g), None) == _ffi.SPAL_ERR_INVALID_ARGUMENT


def test_every_new_symbol_is_exported_and_the_rust_ffi_is_current():
    names, lib = _ffi.exported_names(), _ffi.lib()
    new = ["spal_csr_fsai_setup", "spal_csc_fsai_setup", "spal_fsai_destroy", "spal_fsai_describe", "spal_fsai_factor_csr"]
    for sfx in ("f64", "f32"):
        new += [f"spal_fsai_apply_{sfx}", f"spal_fsai_apply_dev_{sfx}", f"spal_fsai_row_{sfx}"]
        for kind in ("csr", "csc"):
            for solver in ("krylov", "minres"):
                new += [f"spal_{kind}_{solver}_fsai_{sfx}", f"spal_{kind}_{solver}_fsai_dev_{sfx}"]
    assert len(new) == 27
    for name in new:
        assert name in names and hasattr(lib, name), name
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"]).returncode == 0


# ---- the reference is FSAI ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def poisson32():
    a = fr.readonly(fr.poisson2d(32, np.float64))
    a2 = fr.product_pattern(a, a)
    a3 = fr.product_pattern(a2, a)
    return a, {"A": None, "A2": a2, "A3": a3}


@functools.lru_cache(maxsize=None)
def poisson32_factor(name):
    a, patterns = poisson32()
    return fr.fsai(a, patterns[name])


@pytest.mark.parametrize("name,largest", [("A", 3), ("A2", 7), ("A3", 13)])
def test_reference_has_a_unit_diagonal_and_rejects_nothing(name, largest):
    a, _ = poisson32()
    G, rejected, max_row = poisson32_factor(name)
    assert rejected == 0 and max_row == largest
    Gd, Ad = fr.dense(G), fr.dense(a)
    assert np.all(np.triu(Gd, 1) == 0)
    d = np.diag(Gd @ Ad @ Gd.T)
    print(name, "max |diag(G A Gt) - 1|", np.abs(d - 1).max())
    assert np.abs(d - 1).max() <= 8 * max_row * np.finfo(np.float64).eps
    M = Gd.T @ Gd
    assert np.array_equal(M, M.T) or np.abs(M - M.T).max() <= 1e-15
    assert np.linalg.eigvalsh((M + M.T) / 2).min() > 0


def test_reference_pcg_iteration_counts():
    """Poisson 32 x 32, tol = 1e-8, random b (seed 1): 100 iterations plain, 58 / 42 / 32 with the three patterns.  The
    reference is deterministic, so +-2 only guards the transcription."""
    a, _ = poisson32()
    n = a[0]
    b = np.random.default_rng(1).standard_normal(n)
    mul = lambda v: fr.spmv_seq(a, v)                                                       # noqa: E731
    _, plain = kr.cg(mul, None, b, np.zeros(n), 1e-8, 1000)
    counts = {}
    for name in ("A", "A2", "A3"):
        G = poisson32_factor(name)[0]
        Gt = fr.transpose(G)
        _, info = kr.cg(mul, lambda v: fr.apply(G, Gt, v), b, np.zeros(n), 1e-8, 1000)
        assert info["reason"] == 0
        counts[name] = info["iterations"]
    print("plain", plain["iterations"], counts)
    assert abs(plain["iterations"] - 100) <= 2
    assert abs(counts["A"] - 58) <= 2 and abs(counts["A2"] - 42) <= 2 and abs(counts["A3"] - 32) <= 2


def test_transpose_moves_bits():
    G = poisson32_factor("A2")[0]
    Gt = fr.transpose(G)
    assert np.array_equal(fr.dense(Gt), fr.dense(G).T)
    assert np.all(np.diff(Gt[2][int(Gt[1][5]):int(Gt[1][6])].astype(np.int64)) > 0)


def test_fuzz_generator_rarely_rejects_every_row():
    """The GPU fuzz (tests/test_gpu_zz_fsai.py) draws these very cases: fewer than one in ten may be wholly rejected, or
    it would compare little but Jacobi."""
    rng = np.random.default_rng(FUZZ_SEED)
    wholly = some = 0
    for _ in range(FUZZ_CASES):
        mat, cap = fr.fuzz_case(rng)
        _, rejected, _ = fr.fsai(mat, None, cap)
        wholly += rejected == mat[0]
        some += rejected > 0
    print("cases with a rejection", some, "wholly rejected", wholly, "of", FUZZ_CASES)
    assert wholly * 10 < FUZZ_CASES
    assert some >= 3            # ... and the rejected row is exercised
