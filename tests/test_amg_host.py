"""The aggregation AMG without a device: spal_amg_aggregate against the text (tests/amg_ref.py) and the known answers
of include/spal.h, its refusals, the parameter validation, and the effectiveness of the TEXT itself as a preconditioner
of CG on the 32 x 32 five-point matrix (reference only)."""
import ctypes as C

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from spalinalg_amd.matrix import _AmgParamsC
from tests import amg_ref as ar
from tests import colour_ref as cr
from tests import trsv_ref as tr

U = np.uint64


def _host(pattern, seed=0):
    return sp.amg_aggregate(pattern[1], pattern[2], seed)


def _same(pattern, seed=0):
    agg, nagg = _host(pattern, seed)
    ref, nref = ar.aggregate(pattern, seed)
    assert nagg == nref and np.array_equal(agg, ref)
    return agg, nagg


def test_known_answers():
    agg, nagg = _same(ar.path(8)[0])
    assert agg.tolist() == [0, 1, 1, 2, 2, 2, 3, 3] and nagg == 4
    agg, nagg = _same(ar.stencil((3, 3))[0])
    assert agg.tolist() == [0, 2, 1, 2, 2, 2, 3, 2, 4] and nagg == 5
    (pattern, values) = ar.stencil((3, 3))
    (_, p, i), v = ar.coarse(pattern, values, agg, nagg)
    dense = np.zeros((5, 5))
    dense[np.repeat(np.arange(5), np.diff(p.astype(np.int64))), i.astype(np.int64)] = v
    assert dense.tolist() == [[4, 0, -2, 0, 0], [0, 4, -2, 0, 0], [-2, -2, 12, -2, -2], [0, 0, -2, 4, 0], [0, 0, -2, 0, 4]]
    agg, nagg = _same(ar.star(9, two_sided=False)[0])
    assert nagg == 1 and not agg.any()


@pytest.mark.parametrize("seed", cr.SEEDS)
@pytest.mark.parametrize("name", sorted(cr.patterns()))
def test_colouring_patterns(name, seed):
    agg, nagg = _same(cr.patterns_cached()[name], seed)
    assert agg.size == 0 or int(agg.max()) + 1 == nagg


def test_small_and_special_graphs():
    agg, nagg = _host((0, np.zeros(1, dtype=U), np.zeros(0, dtype=U)))
    assert agg.size == 0 and nagg == 0
    agg, nagg = _same(tr.diagonal(1))
    assert agg.tolist() == [0] and nagg == 1
    agg, nagg = _same(tr.diagonal(50))                       # isolated vertices: aggregates of one
    assert nagg == 50 and agg.tolist() == list(range(50))
    n = 70                                                   # the complete graph: one aggregate
    full = tr.from_coo(n, np.repeat(np.arange(n), n), np.tile(np.arange(n), n))
    agg, nagg = _same(full)
    assert nagg == 1
    two = tr.from_coo(6, [0, 1, 1, 2, 3, 4, 4, 5], [1, 0, 2, 1, 4, 3, 5, 4])   # two paths of three
    agg, nagg = _same(two)
    assert set(agg[:3].tolist()).isdisjoint(agg[3:].tolist())


def test_direction_of_storage_and_degree():
    one = tr.from_coo(5, [0, 1, 2, 3], [1, 2, 3, 4])                      # a path stored upwards only
    both = tr.from_coo(5, [0, 1, 2, 3, 1, 2, 3, 4], [1, 2, 3, 4, 0, 1, 2, 3])
    a1, n1 = _same(one)
    a2, n2 = _same(both)
    assert n1 == n2 and np.array_equal(a1, a2)                            # stored twice counts once: the same degrees
    assert np.array_equal(ar.priorities(one), ar.priorities(both))
    assert (ar.priorities(both) >> U(32)).tolist() == [1, 2, 2, 2, 1]


def test_seed_is_taken_mod_2_32():
    pattern = cr.patterns_cached()["sym_banded"]
    a7, n7 = _host(pattern, 7)
    a, n = _host(pattern, 2**32 + 7)
    assert n == n7 and np.array_equal(a, a7)
    a0, _ = _host(pattern, 0)
    assert not np.array_equal(a0, a7)


def test_refusals():
    lib = _ffi.lib()
    inv = _ffi.SPAL_ERR_INVALID_ARGUMENT
    rp, ci = np.array([0, 1, 2], dtype=U), np.array([0, 1], dtype=U)
    agg, nagg = np.zeros(2, dtype=U), C.c_uint64()
    p = lambda a: a.ctypes.data_as(_ffi.u64p)                             # noqa: E731

    def refused(status, text):
        assert status == inv and text in lib.spal_last_error().decode()

    refused(lib.spal_amg_aggregate(C.c_uint64(2), None, p(ci), C.c_uint64(0), p(agg), C.byref(nagg)), "spal_amg_aggregate: null array")
    refused(lib.spal_amg_aggregate(C.c_uint64(2), p(rp), p(ci), C.c_uint64(0), None, C.byref(nagg)), "null array")
    refused(lib.spal_amg_aggregate(C.c_uint64(2), p(rp), p(ci), C.c_uint64(0), p(agg), None), "null array")
    refused(lib.spal_amg_aggregate(C.c_uint64(2), p(np.array([1, 1, 2], dtype=U)), p(ci), C.c_uint64(0), p(agg), C.byref(nagg)), "rowptr[0] = 1")
    refused(lib.spal_amg_aggregate(C.c_uint64(2), p(np.array([0, 2, 1], dtype=U)), p(ci), C.c_uint64(0), p(agg), C.byref(nagg)), "rowptr is not sorted")
    refused(lib.spal_amg_aggregate(C.c_uint64(2), p(rp), p(np.array([0, 2], dtype=U)), C.c_uint64(0), p(agg), C.byref(nagg)), "column 2")
    refused(lib.spal_amg_aggregate(C.c_uint64(2), p(rp), None, C.c_uint64(0), p(agg), C.byref(nagg)), "null array")


def test_parameter_validation_needs_no_device():
    lib = _ffi.lib()
    d = _AmgParamsC()
    assert lib.spal_amg_default_params(C.byref(d)) == 0
    assert [d.seed, d.max_levels, d.coarse_rows, d.nu, d.coarse_sweeps, d.gamma] == [0, 16, 64, 2, 16, 1]
    assert d.omega == 2.0 / 3.0 and d.alpha == 1.0
    assert lib.spal_amg_default_params(None) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    fake = C.create_string_buffer(1 << 16)                                # params are checked before the handle is read
    out = C.c_void_p()
    bad = [("max_levels", 0), ("max_levels", 33), ("nu", 0), ("nu", 17), ("coarse_sweeps", 0), ("coarse_sweeps", 1025),
           ("gamma", 0), ("gamma", 3), ("omega", 0.0), ("omega", -1.0), ("omega", float("nan")), ("omega", float("inf")),
           ("alpha", 0.0), ("alpha", float("nan")), ("alpha", float("inf"))]
    for entry in (lib.spal_csr_amg_setup, lib.spal_csc_amg_setup):
        for field, value in bad:
            p = _AmgParamsC()
            lib.spal_amg_default_params(C.byref(p))
            setattr(p, field, value)
            assert entry(fake, C.byref(p), None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT, (field, value)
            assert field in lib.spal_last_error().decode() and out.value is None
        assert entry(None, C.byref(d), None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
        assert entry(fake, None, None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
        assert entry(fake, C.byref(d), None, None) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert lib.spal_amg_destroy(None) == 0
    with pytest.raises(sp.Panic, match="cycle"):
        sp.CsrMatrix.eye(4).amg(cycle="k")
    a = sp.CsrMatrix(2, 3, [0, 1, 2], [0, 1], [1.0, 1.0])
    with pytest.raises(sp.Panic, match="not square"):
        a.amg()


def _grid_solves():
    pattern, values = ar.stencil((32, 32))
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))
    cols = colind.astype(np.int64)

    def mul(v):
        return np.bincount(rows, weights=values * v[cols], minlength=n)
    b = np.random.default_rng(0).standard_normal(n)
    plain = ar.solve(None, mul, b, "cg", 1e-8, 1000)[1]
    return pattern, values, mul, b, plain


@pytest.mark.parametrize("kw", [dict(), dict(gamma=2, alpha=1.5)], ids=["defaults", "w_alpha_1.5"])
def test_the_text_halves_cg_iterations_on_the_grid(kw):
    """32 x 32 five-point Poisson, f64, tol 1e-8, rng(0) right-hand side: unpreconditioned CG needs about 100
    iterations, with the default V cycle about 21 (levels 1024 / 391 / 95 / 23)."""
    pattern, values, mul, b, plain = _grid_solves()
    h = ar.Hierarchy(pattern, values, **kw)
    assert h.rows == [1024, 391, 95, 23]
    x, info = ar.solve(h, mul, b, "cg", 1e-8, 1000)
    print("cg iterations: plain", plain["iterations"], "amg", info["iterations"])
    assert plain["reason"] == 0 and info["reason"] == 0
    assert 2 * info["iterations"] <= plain["iterations"]
    assert np.linalg.norm(b - mul(x)) <= 1e-7 * np.linalg.norm(b)
