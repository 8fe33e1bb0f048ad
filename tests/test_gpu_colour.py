"""The multicolour ordering on the device against its sequential text (tests/colour_ref.py): colours and rounds exactly,
P A P^T with A's value bits, the ordering kept on the result handle, the vector gather / scatter, and one solve of a
permuted system taken back to the original numbering.  CSR and CSC handles, f64 and f32.

Sizes are the smallest that cross a boundary of the code: 64 / 65 / 130 colours (the 64-colour windows), rows of
thousands of neighbours, a chain of 3000 rounds (every batch size between two polls, 8 .. 512, is crossed), more rows
than one workgroup, and 4096 * 1024 + 1 rows."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import colour_ref as cr
from tests import ilu_ref as ir
from tests import krylov_ref as kr
from tests import ordering_cases as oc
from tests import trsv_ref as tr

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
KINDS = ["csr", "csc"]
TOL = {np.float64: 1e-10, np.float32: 1e-5}
u64 = C.c_uint64


def make(kind, pattern, values):
    n, rowptr, colind = pattern
    if kind == "csr":
        return sp.CsrMatrix(n, n, rowptr, colind, values)
    colptr, rowind, vals, _ = ir.to_csc(pattern, values)
    return sp.CscMatrix(n, n, colptr, rowind, vals)


def arrays(m):
    """(ptr, ind, values) of a CsrMatrix / CscMatrix."""
    return (m.rowptr(), m.colind(), m.values()) if isinstance(m, sp.CsrMatrix) else (m.colptr(), m.rowind(), m.values())


def expected_arrays(kind, pattern, values):
    if kind == "csr":
        return pattern[1], pattern[2], values
    return ir.to_csc(pattern, values)[:3]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_same_matrix(m, kind, pattern, values):
    """Structure equal, value BITS equal (NaN payloads and the sign of zero included)."""
    ptr, ind, val = arrays(m)
    eptr, eind, eval_ = expected_arrays(kind, pattern, values)
    assert np.array_equal(ptr, eptr) and np.array_equal(ind, eind)
    assert val.dtype == eval_.dtype and np.array_equal(bits(val), bits(eval_))


@functools.lru_cache(maxsize=None)
def matrix(name, kind, dtype=np.float32):
    """A named pattern of colour_ref with values of trsv_ref.fill on the device: made once per session and shared."""
    pattern = cr.patterns_cached()[name]
    values, _ = tr.fill(pattern, dtype, np.random.default_rng(len(name)))
    return make(kind, pattern, values), pattern, values


# ---- 1. colours and rounds -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(cr.patterns_cached()))
def test_colours_and_rounds_are_the_text(name, kind):
    a, pattern, _ = matrix(name, kind)
    for seed in cr.SEEDS:
        ref, ref_nc, ref_rounds = cr.reference(name, seed)
        colours, nc, rounds = a.device().colour(seed)
        assert nc == ref_nc and rounds == ref_rounds, (seed, nc, ref_nc, rounds, ref_rounds)
        assert np.array_equal(colours, ref), seed
    got, nc = a.colour()                                  # the matrix-level call, seed 0
    assert nc == cr.reference(name, 0)[1] and np.array_equal(got, cr.reference(name, 0)[0])
    if name == "hand":
        assert got.tolist() == cr.HAND_COLOURS


@pytest.mark.parametrize("kind", KINDS)
def test_chain_of_3000_rounds(kind):
    pattern = cr.key_chain(3000)
    ref, ref_nc, ref_rounds = cr.greedy(pattern, 0)
    assert ref_nc == 2 and ref_rounds == 3000
    a = make(kind, pattern, np.ones(pattern[2].size, dtype=np.float32))
    colours, nc, rounds = a.device().colour(0)
    assert (nc, rounds) == (2, 3000)
    assert np.array_equal(colours, ref)
    # with another seed the same edges are no chain of keys any more: far fewer rounds, the text's colours again
    ref7, nc7, rounds7 = cr.greedy(pattern, 7)
    colours, nc, rounds = a.device().colour(7)
    assert (nc, rounds) == (nc7, rounds7) and rounds7 < 100 and np.array_equal(colours, ref7)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rounds", oc.CHAIN_ROUNDS)
def test_chain_at_batch_boundaries(rounds, kind):
    """The host enqueues batches of 8, 16, 32, 64, ... rounds between two polls.  A chain of exactly 8, 24, 56 or 120
    rounds ends with a batch: the last poll reads the count a round past the end would start with.  One round more,
    and a whole batch runs for one row."""
    pattern = oc.chain(rounds)
    ref, ref_nc, ref_rounds = cr.greedy(pattern, 0)
    assert (ref_nc, ref_rounds) == (2, rounds)
    a = make(kind, pattern, np.ones(pattern[2].size, dtype=np.float32))
    colours, nc, got = a.device().colour(0)
    assert (nc, got) == (2, rounds)
    assert np.array_equal(colours, ref)
    m = a.multicolour(0)                                  # ... and the whole call on the same boundary
    assert m.ncolours == 2 and np.array_equal(m.perm, cr.perm_from_colours(ref))
    assert m.device().describe()["ordering"]["rounds"] == rounds


def test_one_row_past_one_grid_trip():
    n = 4096 * 1024 + 1
    rowptr = np.empty(n + 1, dtype=np.uint64)
    rowptr[0] = 0
    rowptr[1:] = np.arange(1, 2 * n, 2, dtype=np.uint64)        # row 0: the diagonal; row i: (i, i - 1), (i, i)
    colind = np.empty(2 * n - 1, dtype=np.uint64)
    colind[0] = 0
    colind[1::2] = np.arange(n - 1, dtype=np.uint64)
    colind[2::2] = np.arange(1, n, dtype=np.uint64)
    a = sp.CsrMatrix._trusted(n, n, rowptr, colind, np.ones(2 * n - 1, dtype=np.float32))
    ref = np.empty(n, dtype=np.uint64)
    ref_nc = u64()
    assert _ffi.lib().spal_colour_greedy(u64(n), rowptr.ctypes.data_as(_ffi.u64p), colind.ctypes.data_as(_ffi.u64p), u64(0),
                                         ref.ctypes.data_as(_ffi.u64p), C.byref(ref_nc)) == _ffi.SPAL_OK
    colours, nc, rounds = a.device().colour(0)
    assert nc == ref_nc.value and nc <= 3
    assert np.array_equal(colours, ref)
    assert 1 < rounds < 64                                      # the longest run of descending keys along a path


# ---- 2. permute ------------------------------------------------------------------------------------------------------

def _special_values(pattern, dtype):
    """NaNs with distinct payloads, both zeros, infinities and subnormals among ordinary values."""
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, size=pattern[2].size).astype(dtype)
    b = bits(v).copy()
    nan = np.uint64(0x7FF0000000000000) if dtype == np.float64 else np.uint32(0x7F800000)
    sign = np.uint64(1 << 63) if dtype == np.float64 else np.uint32(1 << 31)
    k = np.arange(b.size)
    b[k % 7 == 0] = nan | (k[k % 7 == 0] + 1).astype(b.dtype)                  # NaN, payload = position + 1
    b[k % 7 == 1] = sign | nan | (k[k % 7 == 1] + 1).astype(b.dtype)           # ... with the sign set
    b[k % 7 == 2] = sign                                                       # -0.0
    b[k % 7 == 3] = 0                                                          # +0.0
    b[k % 7 == 4] = (k[k % 7 == 4] + 1).astype(b.dtype)                        # subnormals
    b[k % 49 == 5] = nan                                                       # +inf
    return b.view(dtype)


PERMUTE_CASES = {"full": "full", "banded": "sym_banded", "arrow": "arrow", "fan": "fan", "special": "full"}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", sorted(PERMUTE_CASES))
def test_permute_moves_structure_and_value_bits(case, kind, dtype):
    name = PERMUTE_CASES[case]
    pattern = cr.patterns_cached()[name]
    n = pattern[0]
    if case == "special":
        values = _special_values(pattern, dtype)
        assert np.isnan(values).any() and np.signbit(values[values == 0]).any()
    else:
        values, _ = tr.fill(pattern, dtype, np.random.default_rng(11))
    a = make(kind, pattern, values)
    perms = {"identity": np.arange(n, dtype=np.uint64), "reversal": np.arange(n, dtype=np.uint64)[::-1].copy(),
             "random": np.random.default_rng(77).permutation(n).astype(np.uint64),
             "multicolour": cr.perm_from_colours(cr.reference(name, 0)[0])}
    for label, perm in perms.items():
        p = a.permute(perm)
        want_pattern, want_values = cr.permute(pattern, values, perm)
        assert_same_matrix(p, kind, want_pattern, want_values)
        assert type(p) is type(a) and p.ncolours == 0 and np.array_equal(p.perm, perm), label
        if label == "identity":
            assert_same_matrix(p, kind, pattern, values)
        assert p.device().describe()["ordering"]["colours"] == 0


# ---- 3. multicolour --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["sym_banded", "full", "bidiagonal", "sym_bidiagonal", "arrow", "dense_65", "diagonal_1"])
def test_multicolour_is_colour_then_order_then_permute(name, kind):
    a, pattern, values = matrix(name, kind)
    for seed in (0, 7):
        ref, ref_nc, ref_rounds = cr.reference(name, seed)
        perm = cr.perm_from_colours(ref)
        m = a.multicolour(seed)
        assert type(m) is type(a) and m.ncolours == ref_nc and np.array_equal(m.perm, perm)
        want_pattern, want_values = cr.permute(pattern, values, perm)
        assert_same_matrix(m, kind, want_pattern, want_values)
        # ... which is what the three calls give one after the other
        colours, nc, _ = a.device().colour(seed)
        st_perm = np.empty(pattern[0], dtype=np.uint64)
        assert _ffi.lib().spal_perm_from_colours(u64(colours.size), colours.ctypes.data_as(_ffi.u64p),
                                                 st_perm.ctypes.data_as(_ffi.u64p)) == _ffi.SPAL_OK
        assert_same_matrix(a.permute(st_perm), kind, want_pattern, want_values)
        dev = m.device()
        got_perm, got_nc = dev.ordering()
        assert got_nc == ref_nc and np.array_equal(got_perm, perm)
        info = dev.describe()["ordering"]
        assert set(info) == {"colours", "rounds", "seed", "colour_ms", "permute_ms"}
        assert (info["colours"], info["rounds"], info["seed"]) == (ref_nc, ref_rounds, seed)
        dev.trsv_analyse(lower=True)
        plans = dev.trsv_analyse(lower=False)
        assert plans["lower"]["levels"] <= ref_nc and plans["upper"]["levels"] <= ref_nc
        n, rp, ci = want_pattern
        assert plans["lower"]["levels"] == tr.levels(n, rp, ci, lower=True)[1]
    assert "ordering" not in a.device().describe()        # the operand is left as it was


@pytest.mark.parametrize("kind", KINDS)
def test_two_threads_multicolour_one_fresh_handle(kind):
    """Two callers, one handle nothing has been called on yet: both results are the text.  A hang fails the test at the
    joins."""
    pattern = cr.patterns_cached()["sym_banded"]
    values, _ = tr.fill(pattern, np.float64, np.random.default_rng(41))
    ref, ref_nc, ref_rounds = cr.reference("sym_banded", 7)
    perm = cr.perm_from_colours(ref)
    want_pattern, want_values = cr.permute(pattern, values, perm)
    dev = make(kind, pattern, values).device()
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i):
        try:
            gate.wait(timeout=30)
            out = dev.multicolour(7)
            results[i] = (out.download(), out.ordering(), out.describe()["ordering"])
        except Exception as e:          # reported below, from the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "a thread did not return from multicolour"
    assert not errors, errors
    eptr, eind, eval_ = expected_arrays(kind, want_pattern, want_values)
    for (ptr, ind, val), (got_perm, got_nc), info in results:
        assert np.array_equal(ptr, eptr) and np.array_equal(ind, eind) and np.array_equal(bits(val), bits(eval_))
        assert got_nc == ref_nc and np.array_equal(got_perm, perm)
        assert (info["colours"], info["rounds"], info["seed"]) == (ref_nc, ref_rounds, 7)
    assert "ordering" not in dev.describe()


# ---- 4. vectors ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_vector_permute_both_directions(kind, dtype):
    import torch
    pattern = cr.patterns_cached()["sym_banded"]
    n = pattern[0]
    values, _ = tr.fill(pattern, dtype, np.random.default_rng(3))
    a = make(kind, pattern, values)
    m = a.multicolour()
    perm = m.perm.astype(np.int64)
    v = _special_values((n, None, np.empty(n)), dtype)
    inverse = np.empty_like(v)
    inverse[perm] = v
    dev = m.device()
    x = torch.tensor(v).cuda()
    y = torch.zeros_like(x)
    torch.cuda.synchronize()
    dev.permute_vec_dev(x.data_ptr(), y.data_ptr(), back=False)
    torch.cuda.synchronize()
    assert np.array_equal(bits(y.cpu().numpy()), bits(v[perm]))
    z = torch.zeros_like(x)
    dev.permute_vec_dev(y.data_ptr(), z.data_ptr(), back=True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(z.cpu().numpy()), bits(v))                      # the round trip is the identity
    dev.permute_vec_dev(x.data_ptr(), y.data_ptr(), back=True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(y.cpu().numpy()), bits(inverse))
    # the host twins and the matrix's own helpers
    assert np.array_equal(bits(dev.permute_vec(v)), bits(v[perm]))
    assert np.array_equal(bits(dev.permute_vec(v, back=True)), bits(inverse))
    assert np.array_equal(bits(m.to_order(v)), bits(v[perm])) and np.array_equal(bits(m.from_order(m.to_order(v))), bits(v))
    with pytest.raises(sp.Panic, match="x == y"):
        dev.permute_vec_dev(x.data_ptr(), x.data_ptr())
    with pytest.raises(sp.Panic, match="direction = 2"):
        _ffi.check(getattr(_ffi.lib(), f"spal_{kind}_permute_vec_dev_{'f64' if dtype == np.float64 else 'f32'}")(
            dev._h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_int(2), None))
    with pytest.raises(sp.Panic, match="has no ordering"):
        a.device().permute_vec_dev(x.data_ptr(), y.data_ptr())
    with pytest.raises(sp.Panic, match="has no ordering"):
        a.device().ordering()
    with pytest.raises(sp.Panic, match="handle holds"):
        dev.permute_vec(np.ones(n, dtype=np.float32 if dtype == np.float64 else np.float64))
    with pytest.raises(TypeError, match="no ordering"):
        a.to_order(v)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_solve_in_multicolour_order_and_back(kind, dtype):
    """Residual bound: the solve stops at dot(r, r) <= tol^2 dot(b, b) of the PERMUTED system, whose residual is the
    original one permuted; recomputed in float64 on the original A it may differ by the rounding of the recurrence,
    which for f32 is given a factor of 4."""
    pattern = cr.patterns_cached()["sym_banded"]
    n, rowptr, colind = pattern
    values, b = tr.fill(pattern, dtype, np.random.default_rng(2026))
    tol = TOL[dtype]
    a = make(kind, pattern, values)
    p = a.multicolour()
    assert p.ncolours == cr.reference("sym_banded", 0)[1]
    want_pattern, want_values = cr.permute(pattern, values, p.perm)
    assert_same_matrix(p, kind, want_pattern, want_values)
    f = p.ilu0()
    assert_same_matrix(f, kind, want_pattern, ir.ilu0_rows(*want_pattern, want_values))
    assert f.device().describe()["trsv"]["lower"]["levels"] <= p.ncolours
    bp = p.to_order(b)
    xp, info = p.solve(bp, method="bicgstab", M=f, tol=tol, maxit=200)
    mul = lambda v: p.device().spmv(v)                                                       # noqa: E731
    prec = lambda v: f.solve_triangular(f.solve_triangular(v, True, True), False)           # noqa: E731
    xr, ref = kr.bicgstab(mul, prec, bp, np.zeros_like(bp), tol, 200)
    tr.assert_same_bits(xp, xr)
    assert info.reason == 0 and info.iterations == ref["iterations"] and ref["reason"] == 0
    assert info.residual_sq == ref["residual_sq"]
    x = p.from_order(xp)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    ax = np.bincount(rows, weights=values.astype(np.float64) * x.astype(np.float64)[colind.astype(np.int64)], minlength=n)
    r = b.astype(np.float64) - ax
    slack = 4.0 if dtype == np.float32 else 1.0
    res_sq, rhs_sq = float(r @ r), float(b.astype(np.float64) @ b.astype(np.float64))
    print(f"{kind} {np.dtype(dtype).name}: iterations {info.iterations}, |b - A x|^2 / |b|^2 = {res_sq / rhs_sq:.3e}, "
          f"tol^2 = {tol * tol:.3e}")
    assert res_sq <= slack * tol * tol * rhs_sq


# ---- 6. refusals -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    lib = _ffi.lib()
    cls = sp.CsrMatrix if kind == "csr" else sp.CscMatrix
    wide = cls(2, 3, [0, 1, 2] if kind == "csr" else [0, 1, 2, 2], [0, 1], np.array([1.0, 2.0]))
    for call in (lambda: wide.colour(), lambda: wide.multicolour(), lambda: wide.permute([0, 1])):
        with pytest.raises(sp.Panic, match=r"not square \(2 x 3\)"):
            call()
    assert not wide._dev                                  # refused before a device copy was made
    h = wide.device()
    for call in (lambda: h.colour(), lambda: h.multicolour(), lambda: h.permute([0, 1])):
        with pytest.raises(sp.Panic, match=r"not square \(2 x 3\)"):
            call()
    a, pattern, _ = matrix("hand", kind)
    dev = a.device()
    with pytest.raises(sp.Panic, match=r"perm\[3\] = 1 repeats"):
        dev.permute([0, 1, 2, 1, 4])
    with pytest.raises(sp.Panic, match=r"perm\[1\] = 5 is out of range"):
        dev.permute([0, 5, 2, 5, 4])
    with pytest.raises(sp.Panic, match="perm has 4 entries but the matrix 5 rows"):
        dev.permute([0, 1, 2, 3])
    perm = np.arange(5, dtype=np.uint64)
    out, nc = C.c_void_p(), u64()
    bad = _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert getattr(lib, f"spal_{kind}_permute")(dev._h, perm.ctypes.data_as(_ffi.u64p), u64(5), None, None) == bad
    assert getattr(lib, f"spal_{kind}_permute")(dev._h, None, u64(5), None, C.byref(out)) == bad
    assert getattr(lib, f"spal_{kind}_multicolour")(dev._h, u64(0), None, None, C.byref(nc)) == bad
    assert getattr(lib, f"spal_{kind}_multicolour")(dev._h, u64(0), None, C.byref(out), None) == bad
    assert getattr(lib, f"spal_{kind}_colour")(dev._h, u64(0), None, None, None, C.byref(nc)) == bad
    assert b"null argument" in lib.spal_last_error() and not out.value
    # colours may be left on the device: NULL is allowed there
    rounds = u64()
    assert getattr(lib, f"spal_{kind}_colour")(dev._h, u64(0), None, None, C.byref(nc), C.byref(rounds)) == _ffi.SPAL_OK
    assert (nc.value, rounds.value) == (3, cr.HAND_ROUNDS)


def test_row_block_handle_is_refused(monkeypatch):
    """A CSR handle held as row blocks (more entries than one set of 32-bit offsets addresses; the limit lowered for the
    test) has no ordering calls: refused by name (SPAL_ERR_UNSUPPORTED) before anything is launched."""
    monkeypatch.setenv("SPAL_CSR_PART_ENTRIES", "4000")
    pattern = cr.patterns_cached()["sym_bidiagonal"]
    n = pattern[0]
    a = sp.CsrMatrix(n, n, pattern[1], pattern[2], np.ones(pattern[2].size))
    dev = a.device()
    d = dev.describe()
    assert d["kernel"] == "row_blocks" and d["parts"] >= 3, d
    refused = r"spal_csr_{}: an operand of more than 2\^32 - 65537 entries \(row blocks\)"
    with pytest.raises(sp.SpalError, match=refused.format("colour")):
        dev.colour(0)
    with pytest.raises(sp.SpalError, match=refused.format("permute")):
        dev.permute(np.arange(n, dtype=np.uint64))
    with pytest.raises(sp.SpalError, match=refused.format("multicolour")):
        dev.multicolour(0)
    with pytest.raises(sp.SpalError, match=refused.format("colour")):
        a.colour()
    with pytest.raises(sp.SpalError, match=refused.format("multicolour")):
        a.multicolour()
    x = np.arange(n, dtype=np.float64)
    assert np.array_equal(dev.spmv(x), np.convolve(x, [1, 1, 1], mode="same"))      # the handle is as it was
