"""FSAI on the device against its sequential text (tests/fsai_ref.py): the raw bits of G and Gt, f64 and f32, CSR and
CSC, on both sides of every switch of the factor kernel (the thread form, the wave form, the cap, a workgroup's rows),
the rejected rows, the refusals, apply() as two products, CG / BiCGStab / MINRES with M = f against their texts, a
fuzz over random symmetric patterns, and two threads on one factor.

(The file's name sorts it behind every other GPU test file on purpose: tests/test_gpu_stream_contract.py holds a control
that depends on which streams the process created and used before it, and this file creates streams of its own.)

The geometry is read once from describe(): Bk = block_rows, Mt = thread_form_max, and the default cap.  The reference
costs milliseconds per row, so every reference factor is computed once per (case, dtype) and shared."""
import functools
import threading

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import fsai_ref as fr
from tests import krylov_ref as kr
from tests import minres_ref as mr
from tests import trsv_ref as tr
from tests.test_fsai_host import FUZZ_CASES, FUZZ_SEED
from tests.util import assert_spmv_close

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
KINDS = ["csr", "csc"]
IDS = dict(ids=["f64", "f32"])
SPMV_TOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-4}     # tests/test_gpu_csr_spmv.py's


def make(kind, mat):
    n = mat[0]
    if kind == "csr":
        return sp.CsrMatrix(n, n, mat[1], mat[2], mat[3])
    t = fr.transpose(mat)                              # the CSR arrays of the transpose are the CSC arrays
    return sp.CscMatrix(n, n, t[1], t[2], t[3])


@functools.lru_cache(maxsize=None)
def geometry():
    d = make("csr", fr.diagonal_pattern(1)).fsai().describe()
    return d["block_rows"], d["thread_form_max"], d["cap"]


def lower_lengths(pattern):
    n, rowptr, colind = pattern[:3]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    return np.bincount(rows[colind.astype(np.int64) <= rows], minlength=n)


def check_factor(f, mat, pattern, cap, ref):
    """f against the reference (G, rejected, max_row): structure, bits, counts."""
    G, rejected, max_row = ref
    Gt = fr.transpose(G)
    for got, want in ((f.G, G), (f.Gt, Gt)):
        assert np.array_equal(got.rowptr(), want[1]) and np.array_equal(got.colind(), want[2])
        tr.assert_same_bits(got.values(), want[3])
    _, Mt, _ = geometry()
    q = lower_lengths(mat if pattern is None else pattern)
    d = f.describe()
    assert f.rejected == rejected == d["rejected"]
    assert (d["rows"], d["nnz"], d["cap"], d["max_row"]) == (mat[0], int(G[1][-1]), cap, max_row)
    assert d["capped_rows"] == int(np.sum(q > cap))
    assert d["rows_wave_form"] == int(np.sum(np.minimum(q, cap) > Mt))
    assert d["rows_thread_form"] + d["rows_wave_form"] == mat[0]
    assert d["dtype"] == ("f64" if mat[3].dtype == np.float64 else "f32")
    assert d["setup_ms"] > 0 and d["kernel_ms"] > 0 and d["transpose_ms"] > 0


# ---- 1. the bits of G and Gt ------------------------------------------------------------------------------------------
def double_arrow(n, dtype):
    """A dense first column and a dense last row beside the diagonal: the last row is capped, and Gt's first row has n
    entries."""
    k = np.arange(1, n - 1, dtype=np.int64)
    i = np.concatenate([k, np.full(n - 1, n - 1)])
    j = np.concatenate([np.zeros(n - 2, dtype=np.int64), np.arange(n - 1, dtype=np.int64)])
    return fr.symmetric(n, i, j, np.random.default_rng(3100).uniform(-1, 1, size=i.size), dtype)


def upper_differs(dtype):
    """Stored entries above the diagonal that are NOT those below it: only the lower triangle may be read."""
    n, rowptr, colind, values = fr.band(90, 5, dtype, 7)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    values = values.copy()
    values[colind.astype(np.int64) > rows] *= 3
    return n, rowptr, colind, values


def rejecting(name, dtype):
    base = fr.band(80, 4, dtype, 11)
    if name == "negative_diagonal":
        return fr.with_values(base, [(17, 17)], -2.0)
    if name == "zero_diagonal":
        return fr.with_values(base, [(0, 0), (40, 40)], 0.0)
    if name == "nan":
        return fr.with_values(base, [(33, 31)], np.nan)
    if name == "indefinite_block":                       # rows 50, 51: [[1, 5], [5, 1]] inside the band
        return fr.with_values(fr.with_values(base, [(50, 50), (51, 51)], 1.0), [(51, 50), (50, 51)], 5.0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def fixed_case(name, dtype):
    """(matrix, pattern or None, cap, reference).  Shared, read-only."""
    Bk, Mt, cap = geometry()
    pattern = None
    if name.startswith("n="):
        n = {"1": 1, "Bk-1": Bk - 1, "Bk": Bk, "Bk+1": Bk + 1, "2Bk+1": 2 * Bk + 1}[name[2:]]
        mat = fr.band(n, 4, dtype, n)
    elif name == "band_Mt":
        mat = fr.band(3 * Mt, Mt, dtype, 1)
    elif name == "band_Mt+1":
        mat = fr.band(3 * Mt, Mt + 1, dtype, 2)
    elif name.startswith("dense70/"):
        mat = fr.dense_spd(70, dtype, 3)
        cap = {"1": 1, "Mt": Mt, "32": 32, "64": 64}[name[8:]]
    elif name == "arrow":
        mat = double_arrow(150, dtype)
    elif name == "fill_in_pattern":                      # the pattern has entries where A stores none: zeros in B
        mat, pattern = fr.band(60, 3, dtype, 4), fr.band(60, 6, dtype, 5)
    elif name == "diagonal_pattern":
        mat, pattern = fr.band(60, 5, dtype, 6), fr.diagonal_pattern(60, dtype)
    elif name == "upper_differs":
        mat = upper_differs(dtype)
    elif name.startswith("reject/"):
        mat = rejecting(name[7:], dtype)
    else:
        raise KeyError(name)
    fr.readonly(mat)
    return mat, pattern, cap, fr.fsai(mat, pattern, cap)


FIXED = ["n=1", "n=Bk-1", "n=Bk", "n=Bk+1", "n=2Bk+1", "band_Mt", "band_Mt+1", "dense70/1", "dense70/Mt", "dense70/32",
         "dense70/64", "arrow", "fill_in_pattern", "diagonal_pattern", "upper_differs", "reject/negative_diagonal",
         "reject/zero_diagonal", "reject/nan", "reject/indefinite_block"]


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FIXED)
def test_factor_is_the_text(name, kind, dtype):
    mat, pattern, cap, ref = fixed_case(name, dtype)
    a = make(kind, mat)
    _, Mt, default_cap = geometry()
    f = a.fsai(None if pattern is None else make(kind, pattern), max_row=None if cap == default_cap else cap)
    check_factor(f, mat, pattern, cap, ref)
    G, rejected, max_row = ref
    if name == "band_Mt":
        assert max_row == Mt and f.describe()["rows_wave_form"] == 0
    if name == "band_Mt+1":
        assert max_row == Mt + 1 and f.describe()["rows_wave_form"] == mat[0] - Mt
    if name == "dense70/64":
        assert f.describe()["capped_rows"] == 6 and max_row == 64
    if name == "arrow":
        assert f.describe()["capped_rows"] == 1 and int(np.diff(f.Gt.rowptr().astype(np.int64))[0]) == mat[0]
    if name == "diagonal_pattern":                       # Jacobi: G = diag(1 / sqrt(a_ii))
        d = fr.dense(mat).diagonal().astype(dtype)
        tr.assert_same_bits(f.G.values(), dtype(1) / np.sqrt(d))
    if name.startswith("reject/"):
        assert rejected >= 1 and rejected < mat[0]
        clean = fr.fsai(fr.band(80, 4, dtype, 11), None, cap)[0]
        untouched = np.flatnonzero(G[3] == clean[3])
        assert untouched.size >= G[3].size - 40, "a rejection disturbed rows it does not reach"
    elif name != "upper_differs":
        assert rejected == 0
    # max_row was an option of this call only: the next one has the default again
    if cap != default_cap:
        assert a.fsai().describe()["cap"] == default_cap
    f.close()
    f.close()                                            # twice is fine


@functools.lru_cache(maxsize=None)
def poisson_case(m, dtype):
    """(matrix, {A, A2, A3: (pattern, reference)}): the patterns come from the library's own products."""
    mat = fr.readonly(fr.poisson2d(m, dtype))
    a = make("csr", mat)
    a2 = a @ a
    a3 = a2 @ a
    out = {"A": (None, fr.fsai(mat, None))}
    for name, p in (("A2", a2), ("A3", a3)):
        pattern = fr.readonly((mat[0], p.rowptr().copy(), p.colind().copy(), np.ones(p.nnz(), dtype=dtype)))
        out[name] = (pattern, fr.fsai(mat, pattern))
    return mat, out


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,largest", [("A", 3), ("A2", 7), ("A3", 13)])
def test_poisson_with_the_three_patterns(name, largest, kind, dtype):
    mat, cases = poisson_case(20, dtype)
    pattern, ref = cases[name]
    f = make(kind, mat).fsai(None if pattern is None else make(kind, pattern))
    check_factor(f, mat, pattern, geometry()[2], ref)
    assert ref[1] == 0 and ref[2] == largest
    Gd = fr.dense(ref[0])
    d = np.diag(Gd @ fr.dense(mat) @ Gd.T)
    assert np.abs(d - 1).max() <= 8 * largest * np.finfo(dtype).eps


# ---- 2. refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    mat = fr.band(40, 3, np.float64)
    a = make(kind, mat)
    n, rowptr, colind, values = mat
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    keep = ~((rows == 23) & (colind.astype(np.int64) == 23)) & ~((rows == 31) & (colind.astype(np.int64) == 31))
    hole = fr.from_triplets(n, rows[keep], colind.astype(np.int64)[keep], values[keep], np.float64)
    with pytest.raises(sp.Panic, match="row 23 of the pattern stores no diagonal") as e:
        a.fsai(make(kind, hole))
    assert e.value.status == _ffi.SPAL_ERR_INVALID_ARGUMENT
    with pytest.raises(sp.Panic, match="row 23"):
        make(kind, hole).fsai()                          # the matrix is its own pattern
    # not square, and another shape: through the C entry points
    rect = sp.CsrMatrix(2, 3, np.array([0, 1, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint64), np.ones(2)) \
        if kind == "csr" else sp.CscMatrix(2, 3, np.array([0, 1, 2, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint64), np.ones(2))
    with pytest.raises(sp.Panic, match="not square"):
        rect.fsai()
    with pytest.raises(sp.Panic, match="not square"):
        rect.device().fsai()
    other = make(kind, fr.band(41, 3, np.float64))
    with pytest.raises(sp.Panic, match="the pattern is 41 x 41"):
        a.fsai(other)
    with pytest.raises(sp.Panic, match="the pattern is 41 x 41"):
        a.device().fsai(other.device())
    with pytest.raises(sp.Panic, match="element sizes"):
        a.device().fsai(make(kind, fr.band(40, 3, np.float32)).device())
    for bad in (0, 65, -1):
        with pytest.raises(sp.Panic, match="1 .. 64"):
            a.fsai(max_row=bad)
        with pytest.raises(sp.Panic, match="fsai_max_row must be 1 .. 64"):
            a.device().set_option("fsai_max_row", bad)
    with pytest.raises(TypeError):
        a.fsai(make("csc" if kind == "csr" else "csr", mat))
    f = a.fsai()
    assert f.describe()["cap"] == geometry()[2]          # the refused values left the option alone
    b = np.ones(n)
    with pytest.raises(sp.Panic, match="rows"):
        f.apply(np.ones(n + 1))
    with pytest.raises(sp.Panic, match="handle holds"):
        f.apply(b.astype(np.float32))
    with pytest.raises(sp.Panic, match="41 rows|40 rows"):
        other.solve(np.ones(41), M=f)
    for call in (lambda: a.gmres(b, M=f), lambda: a.solve_block(np.ones((n, 2)), M=f),
                 lambda: a.minres_block(np.ones((n, 2)), M=f), lambda: a.gmres_block(np.ones((n, 2)), M=f),
                 lambda: a.solve(b, M=f, precond_sweeps=1)):
        with pytest.raises(TypeError):
            call()


# ---- 3. apply ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("name", ["n=2Bk+1", "dense70/64", "arrow"])
def test_apply_is_two_products(name, dtype, oracle):
    import torch
    mat, pattern, cap, ref = fixed_case(name, dtype)
    f = make("csr", mat).fsai(max_row=None if cap == geometry()[2] else cap)
    n = mat[0]
    v = np.random.default_rng(5).uniform(-1, 1, size=n).astype(dtype)
    x = f.apply(v)
    G, Gt = f.G, f.Gt
    tr.assert_same_bits(x, Gt.device().spmv(G.device().spmv(v)))
    u_ref = oracle.csr_spmv(G.rowptr(), G.colind(), G.values(), v)
    x_ref = oracle.csr_spmv(Gt.rowptr(), Gt.colind(), Gt.values(), u_ref)
    longest = max(int(np.diff(m.rowptr().astype(np.int64)).max()) for m in (G, Gt))
    if longest <= 32:
        tr.assert_same_bits(x, x_ref)
        tr.assert_same_bits(x, fr.apply(ref[0], fr.transpose(ref[0]), v))
    else:
        assert name != "n=2Bk+1"
        u = G.device().spmv(v)
        assert_spmv_close(u, u_ref, oracle.csr_abs_bound(G.rowptr(), G.colind(), G.values(), v), SPMV_TOL[np.dtype(dtype)])
        assert_spmv_close(x, oracle.csr_spmv(Gt.rowptr(), Gt.colind(), Gt.values(), u),
                          oracle.csr_abs_bound(Gt.rowptr(), Gt.colind(), Gt.values(), u), SPMV_TOL[np.dtype(dtype)])
    # the device-pointer form on two streams of its own, and what it refuses
    t = torch.tensor(v).cuda()
    outs = [torch.empty_like(t), torch.empty_like(t)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(2):
        for o, s in zip(outs, streams):
            f.apply_dev(t.data_ptr(), o.data_ptr(), s)
    for o, s in zip(outs, streams):
        s.synchronize()
        tr.assert_same_bits(o.cpu().numpy(), x)
    with pytest.raises(sp.Panic, match="x == b"):
        f.apply_dev(t.data_ptr(), t.data_ptr(), streams[0])
    with pytest.raises(sp.Panic, match="handle holds"):
        f.apply_dev(t.data_ptr(), outs[0].data_ptr(), streams[0], dtype=np.float32 if dtype == np.float64 else np.float64)
    # u is the stream's scratch block: like every call that takes it, refused on a capturing stream; the capture lives on
    graph = torch.cuda.CUDAGraph()
    y = torch.zeros_like(t)
    with torch.cuda.graph(graph, stream=streams[0]):
        with pytest.raises(sp.Panic, match="cannot be captured"):
            f.apply_dev(t.data_ptr(), outs[0].data_ptr(), torch.cuda.current_stream())
        y.add_(t)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, t)


# ---- 4. the solvers ---------------------------------------------------------------------------------------------------
SOLVE_TOL = {np.float64: 1e-10, np.float32: 1e-5}


def device_ops(a, f):
    G, Gt = f.G.device(), f.Gt.device()
    return (lambda v: a.device().spmv(v)), (lambda v: Gt.spmv(G.spmv(v)))


def same_result(got, ref):
    x, info = got
    xr, ir_ = ref
    tr.assert_same_bits(x, xr)
    assert (info.iterations, info.reason) == (ir_["iterations"], ir_["reason"])
    tr.assert_same_bits(np.array([info.residual_sq]), np.array([ir_["residual_sq"]]))


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("check_every", [1, 8])
@pytest.mark.parametrize("solver", ["cg", "bicgstab", "minres0", "minres_shifted"])
def test_solvers_with_fsai_are_their_texts(solver, check_every, kind, dtype):
    mat, cases = poisson_case(20, dtype)
    pattern, _ = cases["A2"]
    a = make(kind, mat)
    f = a.fsai(make(kind, pattern))
    a.device().set_option("krylov_check_every", check_every)
    b = np.random.default_rng(9).uniform(-1, 1, size=mat[0]).astype(dtype)
    tol, maxit = SOLVE_TOL[dtype], 300
    mul, prec = device_ops(a, f)
    if solver in ("cg", "bicgstab"):
        got = a.solve(b, method=solver, M=f, tol=tol, maxit=maxit)
        ref = kr.METHODS[solver](mul, prec, b, np.zeros_like(b), tol, maxit)
    else:
        shift = 0.0 if solver == "minres0" else 2.5       # inside the spectrum (0, 8) of the 5-point Laplacian
        got = a.minres(b, M=f, shift=shift, tol=tol, maxit=maxit)
        ref = mr.minres(mul, prec, b, np.zeros_like(b), shift, tol, maxit)
    same_result(got, ref)
    assert got[1].iterations >= 3 and (got[1].reason == 0 or solver == "minres_shifted")
    d = a.device().describe()["krylov"]
    assert d["precond"] == "fsai" and d["preconditioned"] == 1 and d["check_every"] == check_every
    assert d["method"] == ("minres" if solver.startswith("minres") else solver) and d["precond_sweeps"] == -1
    # without the factor the record is what it was
    a.solve(b, tol=tol, maxit=5)
    assert "precond" not in a.device().describe()["krylov"]


@pytest.mark.parametrize("name", ["A", "A2", "A3"])
def test_fsai_takes_strictly_fewer_cg_iterations_on_poisson_32(name):
    mat = fr.readonly(fr.poisson2d(32, np.float64))
    a = make("csr", mat)
    pattern = {"A": None, "A2": a @ a, "A3": (a @ a) @ a}[name]
    f = a.fsai(pattern)
    b = np.random.default_rng(1).standard_normal(mat[0])
    _, plain = a.solve(b, tol=1e-8, maxit=1000)
    x, info = a.solve(b, M=f, tol=1e-8, maxit=1000)
    print(name, "plain", plain.iterations, "fsai", info.iterations, "max_row", f.describe()["max_row"])
    assert info.reason == 0 and plain.reason == 0 and info.iterations < plain.iterations
    assert kr.true_relative_residual(mat[:3], mat[3], x, b) <= 2e-8


# ---- 5. fuzz ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fuzz_cases():
    rng = np.random.default_rng(FUZZ_SEED)               # the host test's generator and seed: its share of wholly
    return [fr.fuzz_case(rng) for _ in range(FUZZ_CASES)]  # rejected cases is asserted there


@pytest.mark.parametrize("block", range(4))
def test_fuzz_against_the_text(block):
    wholly = 0
    for k in range(block * 10, block * 10 + 10):
        mat, cap = fuzz_cases()[k]
        kind = KINDS[k % 2]
        ref = fr.fsai(mat, None, cap)
        f = make(kind, mat).fsai(max_row=cap)
        check_factor(f, mat, None, cap, ref)
        wholly += ref[1] == mat[0]
    assert wholly <= 1


# ---- 6. two threads, one factor ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_threads_solve_on_one_factor(kind):
    mat, cases = poisson_case(20, np.float64)
    a = make(kind, mat)
    f = a.fsai(make(kind, cases["A2"][0]))
    bs = [np.random.default_rng(s).uniform(-1, 1, size=mat[0]) for s in (77, 78)]
    expect = [a.solve(v, M=f, tol=1e-10, maxit=300) for v in bs]
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i):
        try:
            gate.wait(timeout=30)
            results[i] = a.solve(bs[i], M=f, tol=1e-10, maxit=300)
        except Exception as e:          # reported below, from the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a thread did not return from its solve"
    assert not errors, errors
    for got, want in zip(results, expect):
        tr.assert_same_bits(got[0], want[0])
        assert (got[1].iterations, got[1].reason, got[1].residual_sq) == (want[1].iterations, 0, want[1].residual_sq)
