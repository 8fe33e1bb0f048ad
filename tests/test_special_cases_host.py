"""The inputs and the comparison rule of tests/test_gpu_special_values.py, checked with the oracle alone (no GPU).

For every structure the GPU file uses: most rows stay finite, every class of row occurs, the leak check poisons enough
columns and leaves the reference's rows of R alone.  The rule itself must reject each kind of damage, one change at a time.
The block-window kernel's one-thread row sums, restated in tests/cpp/blockwin_rows.hpp, equal the oracle on the planted
rows -- and seeded with +0.0, as the kernel once was, they miss exactly the rows of -0.0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import special_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float64, np.float32]


def reference(oracle, name, dtype):
    n, nc, rp, ci, s = sc.case(name, dtype)
    return n, nc, rp, ci, s, oracle.csr_spmv(rp, ci, s["values"], s["x"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(sc.STRUCTURES))
def test_every_structure_carries_every_class(oracle, name, dtype):
    n, nc, rp, ci, s, y_ref = reference(oracle, name, dtype)
    tiny = np.finfo(dtype).tiny
    b = sc.bits(y_ref)
    neg_zero, pos_zero = sc.bits(np.array([-0.0], dtype=dtype))[0], sc.bits(np.array([0.0], dtype=dtype))[0]
    assert np.isfinite(y_ref).mean() >= 0.75
    rows = s["rows"]
    for cls in sc.CLASSES:
        assert rows[cls].size >= sc.PER_CLASS, (cls, rows[cls].size)
    assert np.all(b[rows["neg_zero"]] == neg_zero)
    assert np.all(b[rows["plus_minus_zero"]] == pos_zero)
    assert np.all(np.isnan(y_ref[rows["inf_minus_inf"]]))
    for cls in ("subnormal_product", "subnormal_sum"):
        v = np.abs(y_ref[rows[cls]])
        assert np.all((v > 0) & (v < tiny)), (cls, y_ref[rows[cls]])
    lens = np.diff(rp.astype(np.int64))
    assert np.array_equal(rows["empty"], np.flatnonzero(lens == 0)) and np.all(b[rows["empty"]] == pos_zero)
    if sc.STRUCTURES[name][1]:
        assert rows["empty"].size >= sc.PER_CLASS
    else:
        assert rows["empty"].size == 0       # (rows of one length throughout: the structure cannot hold an empty one)
    # the classes are in the random part too: -0.0, NaN from 0 * inf, +-inf, subnormal results
    assert (b == neg_zero).sum() >= sc.PER_CLASS
    x, va = s["x"], s["values"]
    assert np.any((va[np.isinf(x[ci.astype(np.int64)])]) == 0)
    assert np.isnan(y_ref).sum() >= sc.PER_CLASS and np.isposinf(y_ref).any() and np.isneginf(y_ref).any()
    assert ((np.abs(y_ref) > 0) & (np.abs(y_ref) < tiny)).sum() >= 2 * sc.PER_CLASS
    # x carries every special at the window boundaries
    for special in sc.x_specials(dtype):
        assert np.isnan(x).any() if np.isnan(special) else (sc.bits(x) == sc.bits(np.array([special]))[0]).any(), special
    edges = [0, nc - 1] + [c for m in range(256, 4097, 256) for c in (m - 1, m) if c < nc]
    assert np.all(~np.isfinite(x[edges]) | (np.abs(x[edges]) < tiny))
    assert 0.001 <= (~np.isfinite(x) | (np.abs(x) < tiny)).mean() - len(set(edges)) / nc <= 0.003 or nc < 2000


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(sc.STRUCTURES))
def test_leak_check_inputs(oracle, name, dtype):
    """poison_complement poisons at least a tenth of the columns, and the reference's rows of R do not see it."""
    n, nc, rp, ci, s = sc.case(name, dtype)
    R = sc.leak_rows(n)
    x = sc.ordinary(np.random.default_rng(9), nc, dtype)
    xp = sc.poison_complement(rp, ci, nc, R, x)
    poisoned = ~np.isfinite(xp)
    assert poisoned.mean() >= 0.10, poisoned.mean()
    assert np.array_equal(xp[~poisoned], x[~poisoned])
    assert np.isnan(xp).any() and np.isposinf(xp).any() and np.isneginf(xp).any()
    m = sc.rows_mask(n, R)
    y0, y1 = oracle.csr_spmv(rp, ci, s["values"], x), oracle.csr_spmv(rp, ci, s["values"], xp)
    sc.assert_special_parity(y1[m], y0[m], True, None, None)
    assert not np.array_equal(np.isfinite(y1[~m]), np.isfinite(y0[~m]))      # (the poison is seen outside R)


def test_cut_rows_are_planted(oracle):
    """The pareto structure: in every block of 4096 rows a pass boundary falls inside a row of ten entries, after its second
    entry; that row's first segment is all -0.0, its neighbours are dedicated rows."""
    for dtype in DTYPES:
        n, nc, rp, ci, s, y_ref = reference(oracle, "pareto", dtype)
        rp64 = rp.astype(np.int64)
        assert s["cut"].size == -(-n // sc.BW_TALLEST) >= 5
        planted = np.concatenate([s["rows"][c] for c in sc.CLASSES])
        for r in s["cut"]:
            r0 = r // sc.BW_TALLEST * sc.BW_TALLEST
            e = rp64[r0] + sc.BW_PASS
            assert r - r0 < sc.BW_UNIT and rp64[r] + 2 == e and rp64[r + 1] == e + 8
            prod = s["values"][rp64[r]:e] * s["x"][ci[rp64[r]:e].astype(np.int64)]
            assert np.all(prod == 0) and np.all(np.signbit(prod))
            assert r - 1 in planted and r + 1 in planted
        cut_totals = y_ref[s["cut"]]
        assert (sc.bits(cut_totals) == sc.bits(np.array([-0.0], dtype=dtype))[0]).sum() >= 2      # the carry is the result
        assert (np.abs(cut_totals) > 0.1).sum() >= 2                                                # ordinary numbers follow


def _damaged(y_ref, where, value):
    y = y_ref.copy()
    y[where] = value
    return y


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_rule_rejects_each_kind_of_damage(oracle, dtype):
    n, nc, rp, ci, s, y_ref = reference(oracle, "ragged_lds", dtype)
    bound = sc.spmv_bound(rp, ci, s["values"], s["x"], oracle)
    tol = sc.TOL[np.dtype(dtype)]
    rows = s["rows"]
    everywhere, nowhere = True, False
    short = np.diff(rp.astype(np.int64)) <= 12                      # a row mask
    sc.assert_special_parity(y_ref.copy(), y_ref, everywhere, bound, tol)
    sc.assert_special_parity(y_ref.copy(), y_ref, nowhere, bound, tol)
    sc.assert_special_parity(y_ref.copy(), y_ref, short, bound, tol)
    # the tolerance-based rows may lose the sign of a zero, the exact ones may not
    lost = _damaged(y_ref, rows["neg_zero"][0], 0.0)
    sc.assert_special_parity(lost, y_ref, nowhere, bound, tol)
    finite_row = int(np.flatnonzero(np.isfinite(y_ref) & (np.abs(y_ref) > 0.1))[0])
    nan_row = int(rows["inf_minus_inf"][0])
    inf_row = int(np.flatnonzero(np.isinf(y_ref))[0])
    sub_row = int(rows["subnormal_sum"][0])
    damage = {
        "a -0.0 turned into +0.0 in an exact row": (lost, everywhere),
        "a NaN written into a finite row": (_damaged(y_ref, finite_row, np.nan), nowhere),
        "an inf with its sign flipped": (_damaged(y_ref, inf_row, -y_ref[inf_row]), nowhere),
        "a NaN replaced by a number": (_damaged(y_ref, nan_row, 1.0), nowhere),
        "a NaN replaced by an inf": (_damaged(y_ref, nan_row, np.inf), nowhere),
        "a subnormal flushed to zero in an exact row": (_damaged(y_ref, sub_row, 0.0), everywhere),
        "a finite row beyond the tolerance": (_damaged(y_ref, finite_row, y_ref[finite_row] * (1 + 1000 * tol)), nowhere),
        "an inf written into a finite row": (_damaged(y_ref, finite_row, np.inf), nowhere),
    }
    for what, (y, exact) in damage.items():
        with pytest.raises(AssertionError):
            sc.assert_special_parity(y, y_ref, exact, bound, tol)
            pytest.fail(f"the rule accepted {what}")
    # a flushed subnormal is rejected in a tolerance row too, in f64 as in f32 (no absolute slack hides it)
    with pytest.raises(AssertionError):
        sc.assert_special_parity(_damaged(y_ref, sub_row, 0.0), y_ref, nowhere, bound, tol)
    with pytest.raises(AssertionError):
        sc.assert_special_parity(_damaged(y_ref, int(rows["subnormal_product"][0]), 0.0), y_ref, nowhere, bound, tol)
    # a row mask: the damage counts where the mask is set
    mask = np.zeros(n, dtype=bool)
    mask[rows["neg_zero"][0]] = True
    with pytest.raises(AssertionError):
        sc.assert_special_parity(lost, y_ref, mask, bound, tol)
    sc.assert_special_parity(lost, y_ref, ~mask & short, bound, tol)


@pytest.fixture(scope="module")
def mirror_lib(tmp_path_factory):
    """tests/cpp/blockwin_rows_lib.cpp, compiled once into a temporary directory"""
    so = str(tmp_path_factory.mktemp("blockwin_rows") / "libblockwin_rows.so")
    src = os.path.join(ROOT, "tests", "cpp", "blockwin_rows_lib.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    return C.CDLL(so)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["pareto", "bw_a", "bw_b", "bw_c"])
def test_block_window_thread_rows_mirror_against_the_oracle(oracle, mirror_lib, name, dtype):
    """The kernel's one-thread row sum with its carry (tests/cpp/blockwin_rows.hpp), at every block height: the oracle's
    bits on every row of at most 32 entries.  Seeded with +0.0 the same sum differs from the oracle exactly where the
    reference returns -0.0."""
    lib = mirror_lib
    n, nc, rp, ci, s, y_ref = reference(oracle, name, dtype)
    fn = getattr(lib, "bw_thread_rows_f64" if dtype == np.float64 else "bw_thread_rows_f32")
    fn.restype = None
    rp64, ci64 = np.ascontiguousarray(rp, dtype=np.uint64), np.ascontiguousarray(ci, dtype=np.uint64)
    thread_rows = np.diff(rp64.astype(np.int64)) <= 32
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    neg_zero = sc.bits(np.array([-0.0], dtype=dtype))[0]
    for block_rows in (512, 1024, 2048, 4096):
        for seed_neg in (1, 0):
            y = np.full(n, 77, dtype=dtype)
            fn(C.c_uint64(n), p(rp64), p(ci64), p(s["values"]), p(s["x"]), C.c_uint64(block_rows), C.c_uint64(sc.BW_PASS),
               C.c_int(seed_neg), p(y))
            assert np.all(y[~thread_rows] == 77)
            if seed_neg:
                sc.assert_special_parity(y[thread_rows], y_ref[thread_rows], True, None, None)
            else:
                differ = (sc.bits(y) != sc.bits(y_ref)) & thread_rows & ~np.isnan(y_ref)
                assert np.array_equal(differ, thread_rows & (sc.bits(y_ref) == neg_zero)) and differ.sum() >= sc.PER_CLASS
