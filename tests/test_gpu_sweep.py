"""Jacobi sweeps on a triangle on the device against their sequential definition (tests/sweep_ref.py): raw bits equal, NaN
by position, f64 and f32, lower and upper, CSR and CSC -- and CG / BiCGStab preconditioned through them against
tests/krylov_ref.py run with the sweep reference as preconditioner.

Matrices come from trsv_ref.fill (values and b in (-1, 1), a dominant diagonal), a few hundred rows each; the sizes that
matter to the kernel -- the rows of a workgroup and the entries it stages at a time -- are read from describe(), and
the geometry cases are built around them."""
import functools
import threading
import zlib

import numpy as np
import pytest

import spalinalg_amd as sp
from tests import ilu_ref as ir
from tests import krylov_ref as kr
from tests import sweep_ref as sw
from tests import trsv_ref as tr
from tests.test_trsv_host import HAND_L, dense_to_csr

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
SWEEPS = (0, 1, 2, 5)


def csr(pattern, values):
    n, rowptr, colind = pattern
    return sp.CsrMatrix(n, n, rowptr, colind, values)


def csc(pattern, values):
    n, _, _ = pattern
    colptr, rowind, vals, _ = ir.to_csc(pattern, values)
    return sp.CscMatrix(n, n, colptr, rowind, vals)


MAKERS = {"csr": csr, "csc": csc}


def _lower_pattern(name):
    rng = np.random.default_rng(20261018)
    if name == "diagonal":
        return tr.diagonal(300)
    if name == "bidiagonal":
        return tr.bidiagonal(300)
    if name == "dense":
        return tr.dense_triangle(200)                 # row lengths 0 .. 199
    if name == "banded":
        return tr.banded(701, 6, 64, rng)
    if name == "arrow":
        return tr.arrow(400)                          # one row of 400 entries, a first column read by every row
    if name == "chains":
        return tr.chains(np.concatenate([rng.integers(1, 12, size=90), [40]]))
    if name == "prescribed":
        return tr.prescribed((1, 255, 256, 257, 1, 513, 3, 1), rng)
    if name == "one":
        return tr.diagonal(1)
    raise KeyError(name)


STRUCTURES = ["diagonal", "bidiagonal", "dense", "banded", "arrow", "chains", "prescribed", "one"]


@functools.lru_cache(maxsize=None)
def case(name, lower, dtype):
    """(pattern, values, b) -- made once per session, shared, never written to."""
    pattern = _lower_pattern(name)
    if not lower:
        pattern = tr.mirror(pattern)
    values, b = tr.fill(pattern, dtype, np.random.default_rng(zlib.crc32(f"sweep/{name}/{lower}".encode())))
    for a in (*pattern[1:], values, b):
        a.setflags(write=False)
    return pattern, values, b


@functools.lru_cache(maxsize=None)
def geometry():
    """(rows of a workgroup, entries of a chunk), as describe() reports them after a first sweep."""
    pattern, values, b = case("bidiagonal", True, np.float64)
    dev = csr(pattern, values).device()
    dev.trsv_sweep(b, 1)
    d = dev.describe()["trsv_sweep"]
    assert d["prepared"] == 1 and d["calls"] == 1 and d["prepare_ms"] >= 0
    assert d["block_rows"] >= 1 and d["chunk_entries"] >= 1
    return d["block_rows"], d["chunk_entries"]


def check_all(a, pattern, values, b, lower, units=(False, True), sweeps=SWEEPS):
    for unit in units:
        for s in sweeps:
            got = a.solve_triangular(b, lower=lower, unit_diagonal=unit, sweeps=s)
            sw.assert_same_bits(got, sw.sweep_vec(*pattern, values, b, s, lower, unit))


# ---- the hand example -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_hand_example(kind, dtype):
    bl, bu = np.array([2, 3, 10, 9], dtype=dtype), np.array([7, 5, 10, 6], dtype=dtype)
    for dense, b, lower in ((HAND_L, bl, True), (HAND_L.T, bu, False)):
        n, rp, ci, v = dense_to_csr(dense, dtype)
        a = MAKERS[kind]((n, rp, ci), v)
        for unit in (False, True):
            for s in range(4):
                got = a.solve_triangular(b, lower=lower, unit_diagonal=unit, sweeps=s)
                assert got.dtype == dtype
                sw.assert_same_bits(got, sw.sweep_loop(n, rp, ci, v, b, s, lower, unit))
        # four levels: three passes are the substitution, two are not yet
        assert a.solve_triangular(b, lower=lower, sweeps=3).tolist() == [1, 2, 1, 3]
        assert a.solve_triangular(b, lower=lower, sweeps=2).tolist() != [1, 2, 1, 3]
        assert a.solve_triangular(b, lower=lower, sweeps=0).tolist() == (b / np.diag(dense).astype(dtype)).tolist()


# ---- structures ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("name", STRUCTURES)
def test_structure_csr(name, lower, dtype):
    pattern, values, b = case(name, lower, dtype)
    check_all(csr(pattern, values), pattern, values, b, lower)


@pytest.mark.parametrize("name", STRUCTURES)
def test_structure_csc(name):
    lower = STRUCTURES.index(name) % 2 == 0
    pattern, values, b = case(name, lower, np.float64)
    check_all(csc(pattern, values), pattern, values, b, lower)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("name", STRUCTURES)
def test_enough_sweeps_are_the_device_s_own_exact_solve(name, lower, dtype):
    pattern, values, b = case(name, lower, dtype)
    nl = tr.levels(*pattern, lower=lower)[1]
    a = csr(pattern, values)
    for unit in (False, True):
        exact = a.solve_triangular(b, lower=lower, unit_diagonal=unit)
        sw.assert_same_bits(a.solve_triangular(b, lower=lower, unit_diagonal=unit, sweeps=nl - 1), exact)
        sw.assert_same_bits(a.solve_triangular(b, lower=lower, unit_diagonal=unit, sweeps=10 ** 9), exact)   # clamped to n - 1
    if name == "bidiagonal":
        short = a.solve_triangular(b, lower=lower, sweeps=5)
        assert short.tobytes() != a.solve_triangular(b, lower=lower).tobytes()


# ---- geometry ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("rows", ["R-1", "R", "R+1", "2R+1"])
def test_row_counts_around_a_workgroup(rows, lower):
    R, _ = geometry()
    n = {"R-1": R - 1, "R": R, "R+1": R + 1, "2R+1": 2 * R + 1}[rows]
    pattern = tr.banded(n, 4, 48, np.random.default_rng(n))
    if not lower:
        pattern = tr.mirror(pattern)
    for dtype in DTYPES:
        values, b = tr.fill(pattern, dtype, np.random.default_rng(n + 1))
        check_all(csr(pattern, values), pattern, values, b, lower, sweeps=(1, 3))


def _long_rows_pattern(R, K):
    """Lower triangle: rows of 2K + 3, K + 1 and 2K + 3 triangle entries as the first, a middle and the last row of one
    block of R rows, and of K + 1, 2K + 3 and K + 1 in the block after it; every other row holds its diagonal and up to
    two entries below it."""
    first = ((2 * K + 3) // R + 1) * R              # the first block boundary with enough columns to the left
    n = first + 2 * R
    rng = np.random.default_rng(K)
    i = np.repeat(np.arange(1, n, dtype=np.int64), 2)
    j = np.maximum(i - rng.integers(1, 40, size=i.size), 0)
    rows, cols = [i], [j]
    long_rows = ((first, 2 * K + 3), (first + R // 2, K + 1), (first + R - 1, 2 * K + 3),
                 (first + R, K + 1), (first + R + R // 2, 2 * K + 3), (n - 1, K + 1))
    for r, cnt in long_rows:
        rows.append(np.full(cnt, r, dtype=np.int64))
        cols.append(np.arange(cnt, dtype=np.int64) * (r // cnt))            # spread over [0, r)
    return tr._with_diag(n, np.concatenate(rows), np.concatenate(cols)), long_rows


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_rows_longer_than_one_and_two_chunks(lower):
    R, K = geometry()
    pattern, long_rows = _long_rows_pattern(R, K)
    n, rowptr, colind = pattern
    lens = np.diff(rowptr.astype(np.int64))
    assert all(lens[r] >= cnt + 1 for r, cnt in long_rows)
    assert [r % R for r, _ in long_rows] == [0, R // 2, R - 1] * 2
    if not lower:
        pattern = tr.mirror(pattern)
    for dtype in DTYPES:
        values, b = tr.fill(pattern, dtype, np.random.default_rng(23))
        check_all(csr(pattern, values), pattern, values, b, lower, units=(False,), sweeps=(1, 2))


def test_chunk_boundary_inside_a_row():
    R, K = geometry()
    per_row = K // R + 3                           # entries per row, so that a block holds more than one chunk
    pattern = tr.banded(3 * R + 7, per_row - 1, 4 * per_row, np.random.default_rng(29))
    n, rowptr, colind = pattern
    rp = rowptr.astype(np.int64)
    cuts = [rp[r0] + K for r0 in range(0, n, R) if rp[min(r0 + R, n)] - rp[r0] > K]
    assert cuts and any(c not in set(rp.tolist()) for c in cuts), "no chunk boundary falls inside a row"
    for lower, pat in ((True, pattern), (False, tr.mirror(pattern))):
        for dtype in DTYPES:
            values, b = tr.fill(pat, dtype, np.random.default_rng(31))
            check_all(csr(pat, values), pat, values, b, lower, sweeps=(1, 2))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_empty_rows_and_rows_of_their_diagonal_alone(dtype):
    R, _ = geometry()
    n = 2 * R + 5
    rng = np.random.default_rng(37)
    kind = rng.integers(0, 3, size=n)              # 0: empty, 1: the diagonal alone, 2: the diagonal and entries on both sides
    kind[[0, R - 1, R, n - 1]] = [0, 0, 1, 0]
    r2 = np.flatnonzero(kind == 2)
    i = np.repeat(r2, 4)
    j = np.clip(i + rng.integers(-30, 31, size=i.size), 0, n - 1)
    d = np.flatnonzero(kind >= 1)
    ragged = tr.from_coo(n, np.concatenate([i, d]), np.concatenate([j, d]))
    values, b = tr.fill(ragged, dtype, np.random.default_rng(41))
    a = csr(ragged, values)
    for lower in (True, False):
        check_all(a, ragged, values, b, lower, units=(True,))
        with pytest.raises(sp.Panic, match="row 0 stores no diagonal entry"):
            a.solve_triangular(b, lower=lower, sweeps=1)
    # ... and with every diagonal stored, the rows of kind 0 holding it alone
    d = np.arange(n)
    stored = tr.from_coo(n, np.concatenate([i, d]), np.concatenate([j, d]))
    values, b = tr.fill(stored, dtype, np.random.default_rng(43))
    a = csr(stored, values)
    for lower in (True, False):
        check_all(a, stored, values, b, lower)


# ---- IEEE --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_other_triangle_full_of_nan_is_never_read_into_the_arithmetic(kind, dtype):
    pattern = tr.full(600, 6, np.random.default_rng(47))
    values, b = tr.fill(pattern, dtype, np.random.default_rng(53))
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    for lower in (True, False):
        poisoned = values.copy()
        poisoned[(colind.astype(np.int64) > rows) if lower else (colind.astype(np.int64) < rows)] = np.nan
        a = MAKERS[kind](pattern, poisoned)
        for s in (1, 3):
            ref = sw.sweep_vec(*pattern, values, b, s, lower)
            assert np.isfinite(ref).all()
            sw.assert_same_bits(a.solve_triangular(b, lower=lower, sweeps=s), ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_zero_diagonal_gives_the_reference_inf_and_nan(lower, dtype):
    n = 601
    pattern = tr.banded(n, 6, 64, np.random.default_rng(13))
    if not lower:
        pattern = tr.mirror(pattern)
    values, b = tr.fill(pattern, dtype, np.random.default_rng(14))
    _, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    values[(rows == colind.astype(np.int64)) & (rows == n // 2)] = 0
    a = csr(pattern, values)
    ref = sw.sweep_vec(*pattern, values, b, 3, lower)
    assert np.isinf(ref[n // 2]) and np.isnan(ref).any() and np.isfinite(ref).any()
    check_all(a, pattern, values, b, lower, units=(False,), sweeps=(0, 1, 3, n - 1))
    sw.assert_same_bits(a.solve_triangular(b, lower=lower, sweeps=n), a.solve_triangular(b, lower=lower))


# ---- device pointers -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_device_forms_in_place_out_of_place_stream_and_back_to_back(kind, dtype):
    import torch
    pattern = tr.full(900, 5, np.random.default_rng(11))
    values, b = tr.fill(pattern, dtype, np.random.default_rng(12))
    b2 = np.ascontiguousarray(b[::-1])
    dev = MAKERS[kind](pattern, values).device()
    bt, b2t = torch.from_numpy(b).cuda(), torch.from_numpy(b2).cuda()
    torch.cuda.synchronize()
    # out of place on the default stream, every scratch count: b stays as it was
    for s in (0, 1, 2, 3):
        out = torch.full_like(bt, float("nan"))
        torch.cuda.synchronize()
        dev.trsv_sweep_dev(bt.data_ptr(), out.data_ptr(), s, True, False)
        torch.cuda.synchronize()
        sw.assert_same_bits(out.cpu().numpy(), sw.sweep_vec(*pattern, values, b, s, True))
        sw.assert_same_bits(bt.cpu().numpy(), b)
    # in place on a stream of the caller's: the lower sweep, the upper one behind it, and the same on another right-hand
    # side behind that -- nothing synchronised in between
    st = torch.cuda.Stream()
    w1, w2 = bt.clone(), b2t.clone()
    torch.cuda.synchronize()
    for w in (w1, w2):
        dev.trsv_sweep_dev(w.data_ptr(), w.data_ptr(), 2, True, True, st)
        dev.trsv_sweep_dev(w.data_ptr(), w.data_ptr(), 3, False, False, st)
    st.synchronize()
    for w, rhs in ((w1, b), (w2, b2)):
        ref = sw.sweep_vec(*pattern, values, sw.sweep_vec(*pattern, values, rhs, 2, True, True), 3, False)
        sw.assert_same_bits(w.cpu().numpy(), ref)
    # out of place, two right-hand sides back to back on that stream
    o1, o2 = torch.empty_like(bt), torch.empty_like(bt)
    torch.cuda.synchronize()
    dev.trsv_sweep_dev(bt.data_ptr(), o1.data_ptr(), 2, False, False, st)
    dev.trsv_sweep_dev(b2t.data_ptr(), o2.data_ptr(), 2, False, False, st)
    st.synchronize()
    sw.assert_same_bits(o1.cpu().numpy(), sw.sweep_vec(*pattern, values, b, 2, False))
    sw.assert_same_bits(o2.cpu().numpy(), sw.sweep_vec(*pattern, values, b2, 2, False))


# ---- handle kinds, threads, describe ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_handles_built_on_the_device_sweep_like_uploaded_ones(dtype):
    pattern = tr.full(800, 5, np.random.default_rng(15))
    values, b = tr.fill(pattern, dtype, np.random.default_rng(16))
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rowptr.astype(np.int64)))
    perm = np.random.default_rng(17).permutation(colind.size)
    assembled = sp.CsrMatrix.from_coo(sp.CooMatrix.with_triplets(n, n, rows[perm], colind[perm], values[perm]))
    assert np.array_equal(assembled.rowptr(), rowptr) and np.array_equal(assembled.colind(), colind)
    for lower in (True, False):
        check_all(assembled, pattern, values, b, lower, sweeps=(0, 2))
    f = ir.ilu0_rows(*pattern, values)
    for make in (csr, csc):
        factor = make(pattern, values).ilu0()
        sw.assert_same_bits(factor.solve_triangular(b, True, True, sweeps=2), sw.sweep_vec(*pattern, f, b, 2, True, True))
        sw.assert_same_bits(factor.solve_triangular(b, False, False, sweeps=2), sw.sweep_vec(*pattern, f, b, 2, False))


@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_two_threads_take_the_first_sweep_of_a_fresh_handle(kind):
    pattern, values, b = case("banded", True, np.float64)
    b2 = np.ascontiguousarray(b[::-1])
    dev = MAKERS[kind](pattern, values).device()
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i, rhs):
        try:
            gate.wait(timeout=30)
            results[i] = dev.trsv_sweep(rhs, 3)
        except Exception as e:          # reported below, from the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(0, b), daemon=True),
               threading.Thread(target=work, args=(1, b2), daemon=True)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "a thread did not return from its first sweep"
    assert not errors, errors
    sw.assert_same_bits(results[0], sw.sweep_vec(*pattern, values, b, 3))
    sw.assert_same_bits(results[1], sw.sweep_vec(*pattern, values, b2, 3))
    assert dev.describe()["trsv_sweep"]["calls"] == 2


@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_sweeps_analyse_nothing(kind):
    pattern, values, b = case("banded", True, np.float64)
    dev = MAKERS[kind](pattern, values).device()
    assert "trsv_sweep" not in dev.describe() and "trsv" not in dev.describe()
    dev.trsv_sweep(b, 2, lower=True)
    dev.trsv_sweep(b, 0, lower=False, unit_diagonal=True)
    d = dev.describe()
    assert "trsv" not in d
    R, K = geometry()
    assert d["trsv_sweep"]["calls"] == 2 and (d["trsv_sweep"]["block_rows"], d["trsv_sweep"]["chunk_entries"]) == (R, K)
    # the exact solve does not look at the option
    dev.set_option("trsv_sweeps", 0)
    tr.assert_same_bits(dev.trsv(b), tr.solve_loop(*pattern, values, b))
    assert dev.describe()["trsv"]["analyses"] == 1


# ---- errors ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_errors_through_the_binding_leave_the_handle_usable(kind):
    make = MAKERS[kind]
    cls = sp.CsrMatrix if kind == "csr" else sp.CscMatrix
    rect = cls(2, 3, [0, 1, 2] if kind == "csr" else [0, 1, 2, 2], [0, 1], np.array([1.0, 2.0])).device()
    with pytest.raises(sp.Panic, match=r"not square \(2 x 3\)"):
        rect.trsv_sweep(np.ones(2), 1)
    pattern = tr.drop_diagonal(tr.drop_diagonal(tr.full(900, 4, np.random.default_rng(18)), 700), 333)
    values, b = tr.fill(pattern, np.float64, np.random.default_rng(19))
    dev = make(pattern, values).device()
    for lower in (True, False):
        for s in (0, 2):
            with pytest.raises(sp.Panic, match=rf"spal_{kind}_trsv_sweep: row 333 stores no diagonal entry"):
                dev.trsv_sweep(b, s, lower)
        sw.assert_same_bits(dev.trsv_sweep(b, 2, lower, unit_diagonal=True), sw.sweep_vec(*pattern, values, b, 2, lower, True))
    pattern, values, b = case("dense", True, np.float64)
    dev = make(pattern, values).device()
    with pytest.raises(sp.Panic, match=r"b.len\(\) = 199"):
        dev.trsv_sweep(b[:-1], 1)
    with pytest.raises(sp.Panic, match="handle holds f64 values"):
        dev.trsv_sweep(b.astype(np.float32), 1)
    with pytest.raises(sp.Panic, match="null vector"):
        dev.trsv_sweep_dev(0, 0, 1)
    with pytest.raises(sp.Panic, match="trsv_sweeps must be >= -1"):
        dev.set_option("trsv_sweeps", -2)
    dev.set_option("trsv_sweeps", -1)
    sw.assert_same_bits(dev.trsv_sweep(b, 2), sw.sweep_vec(*pattern, values, b, 2))


# ---- CG and BiCGStab through the sweeps --------------------------------------------------------------------------------

TOL = {np.float64: 1e-10, np.float32: 1e-5}
MAXIT = 120


@functools.lru_cache(maxsize=None)
def krylov_case(method, dtype):
    """(pattern, values, b, the ILU(0) factor's values by the host reference): CG on an SPD banded matrix, BiCGStab on an
    unsymmetric one.  Shared, read-only."""
    rng = np.random.default_rng(zlib.crc32(method.encode()))
    if method == "cg":
        pattern = ir.sym(tr.banded(351, 4, 40, rng))
        values, b = kr.spd_fill(pattern, dtype, rng)
    else:
        pattern = ir.full(383, 5, rng)
        values, b = tr.fill(pattern, dtype, rng)
    f = ir.ilu0_rows(*pattern, values)
    for a in (*pattern[1:], values, b, f):
        a.setflags(write=False)
    return pattern, values, b, f


def same_result(got, ref):
    x, info = got
    xr, ir_ = ref
    sw.assert_same_bits(x, xr)
    assert info.iterations == ir_["iterations"] and info.reason == ir_["reason"]
    sw.assert_same_bits(np.array([info.residual_sq]), np.array([ir_["residual_sq"]]))
    assert info.rhs_sq == ir_["rhs_sq"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("sweeps", [0, 2])
@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_preconditioned_solve_is_the_reference_loop_with_the_sweep_reference(method, kind, sweeps, dtype):
    pattern, values, b, f = krylov_case(method, dtype)
    a = MAKERS[kind](pattern, values)
    m = a.ilu0()
    x, info = a.solve(b, method, M=m, tol=TOL[dtype], maxit=MAXIT, precond_sweeps=sweeps)
    ref = kr.METHODS[method](lambda v: a.device().spmv(v), sw.preconditioner(pattern, f, sweeps), b, np.zeros_like(b),
                             TOL[dtype], MAXIT)
    same_result((x, info), ref)
    assert info.reason == 0 and 0 < info.iterations < MAXIT
    # no triangle was analysed for it (the factor came with a copy of a's lower plan: that is no analysis of its own)
    d = m.device().describe()
    assert d["trsv_sweep"]["prepared"] == 1 and d.get("trsv", {}).get("analyses", 0) == 0 and "upper" not in d.get("trsv", {})
    k = a.device().describe()["krylov"]
    assert k["precond_sweeps"] == sweeps and k["preconditioned"] == 1 and k["iterations"] == info.iterations


@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_poll_interval_does_not_change_a_bit(method):
    pattern, values, b, f = krylov_case(method, np.float64)
    a = csr(pattern, values)
    m = a.ilu0()
    runs = []
    for every in (1, 3, 8):
        a.device().set_option("krylov_check_every", every)
        runs.append(a.solve(b, method, M=m, tol=1e-10, maxit=MAXIT, precond_sweeps=2))
        assert a.device().describe()["krylov"]["check_every"] == every
    for x, info in runs[1:]:
        sw.assert_same_bits(x, runs[0][0])
        assert (info.iterations, info.reason, info.residual_sq) == (runs[0][1].iterations, runs[0][1].reason, runs[0][1].residual_sq)


@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_default_option_is_the_exact_solves_of_an_untouched_factor(kind):
    pattern, values, b, f = krylov_case("cg", np.float64)
    a = MAKERS[kind](pattern, values)
    untouched, back = a.ilu0(), a.ilu0()
    x0, i0 = a.solve(b, "cg", M=untouched, tol=1e-10, maxit=MAXIT)
    assert a.device().describe()["krylov"]["precond_sweeps"] == -1
    a.solve(b, "cg", M=back, tol=1e-10, maxit=MAXIT, precond_sweeps=2)
    x1, i1 = a.solve(b, "cg", M=back, tol=1e-10, maxit=MAXIT, precond_sweeps=-1)
    sw.assert_same_bits(x1, x0)
    assert (i1.iterations, i1.reason, i1.residual_sq) == (i0.iterations, i0.reason, i0.residual_sq)
    assert a.device().describe()["krylov"]["precond_sweeps"] == -1
    assert "upper" in back.device().describe()["trsv"]              # the exact solves analysed it


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["csr", "csc"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_the_matrix_itself_with_no_sweeps_is_jacobi(method, kind, dtype):
    pattern, values, b, _ = krylov_case(method, dtype)
    n, rowptr, colind = pattern
    a = MAKERS[kind](pattern, values)
    diag = values[ir.diag_positions(n, rowptr, colind)]
    x, info = a.solve(b, method, M=a, tol=TOL[dtype], maxit=MAXIT, precond_sweeps=0)
    with np.errstate(all="ignore"):
        ref = kr.METHODS[method](lambda v: a.device().spmv(v), lambda v: v / diag, b, np.zeros_like(b), TOL[dtype], MAXIT)
    same_result((x, info), ref)
    assert info.reason == 0
    d = a.device().describe()
    assert "trsv" not in d and d["krylov"]["precond_sweeps"] == 0


@pytest.mark.parametrize("kind", ["csr", "csc"])
def test_option_validation(kind):
    pattern, values, b, _ = krylov_case("cg", np.float64)
    a = MAKERS[kind](pattern, values)
    for bad in (-2, -100):
        with pytest.raises(sp.Panic, match="trsv_sweeps must be >= -1"):
            a.device().set_option("trsv_sweeps", bad)
        with pytest.raises(sp.Panic, match="trsv_sweeps must be >= -1"):
            a.solve(b, "cg", M=a, precond_sweeps=bad)
    for good in (-1, 0, 7, 10 ** 12):
        a.device().set_option("trsv_sweeps", good)
