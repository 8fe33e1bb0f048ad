"""CPU-side tests of A + B, A - B and -A (spal_csr_add / _sub / _neg and the CSC twins): the ABI, the two CPU
restatements against each other and against the reference's known-answer tests, the host-side panics and type errors
of the Python binding, and the kernels' ISA (Neg is an fneg, not 0 - x)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi
from tests import spadd_ref
from tests.util import random_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "spalinalg_amd", "csrc", "spal_spadd.hip")
NAMES = [f"spal_{f}_{op}" for f in ("csr", "csc") for op in ("add", "sub", "neg")]


@pytest.fixture(scope="module")
def ops_kats():
    with open(os.path.join(ROOT, "tests", "golden", "reference_ops_kats.json")) as f:
        return json.load(f)


def kat_operand(m):
    """(nmajor, nminor, (ptr, ind, values)) of a fixture matrix, compressed by its major index"""
    if "rowptr" in m:
        return m["nrows"], m["ncols"], (np.array(m["rowptr"], np.uint64), np.array(m["colind"], np.uint64),
                                        np.array(m["values"]))
    return m["ncols"], m["nrows"], (np.array(m["colptr"], np.uint64), np.array(m["rowind"], np.uint64),
                                    np.array(m["values"]))


def test_entry_points_declared_and_exported():
    names = _ffi.exported_names()
    lib = _ffi.lib()
    for n in NAMES:
        assert n in names
        assert hasattr(lib, n)


@pytest.mark.parametrize("name", NAMES)
def test_null_arguments(name):
    fn = getattr(_ffi.lib(), name)
    out = C.c_void_p()
    if name.endswith("neg"):
        assert fn(None, None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
        assert fn(None, None, None) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    else:
        assert fn(None, None, None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
        assert fn(None, None, None, None) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert b"null" in _ffi.lib().spal_last_error()


# ---- the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["csr_add", "csr_sub", "csr_neg", "csc_add", "csc_sub", "csc_neg"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_reproduces_the_kats(ops_kats, name, dtype):
    k = ops_kats[name]
    nmaj, nmin, a = kat_operand(k["lhs"])
    a = (a[0], a[1], a[2].astype(dtype))
    _, _, o = kat_operand(k["out"])
    if k["op"] == "neg":
        forms = [spadd_ref.neg(a)]
    else:
        _, _, b = kat_operand(k["rhs"])
        b = (b[0], b[1], b[2].astype(dtype))
        sub = k["op"] == "sub"
        forms = [spadd_ref.add_sub_loop(nmaj, nmin, a, b, sub), spadd_ref.add_sub_fast(nmaj, nmin, a, b, sub)]
    for p, i, v in forms:
        assert p.tolist() == o[0].tolist() and i.tolist() == o[1].tolist()
        assert v.dtype == dtype and v.tolist() == o[2].tolist()


def same_bits(x, y):
    (xp, xi, xv), (yp, yi, yv) = x, y
    assert np.array_equal(np.asarray(xp, np.uint64), np.asarray(yp, np.uint64))
    assert np.array_equal(np.asarray(xi, np.uint64), np.asarray(yi, np.uint64))
    assert xv.dtype == yv.dtype
    bits = np.uint64 if xv.dtype == np.float64 else np.uint32
    assert np.array_equal(xv.view(bits), yv.view(bits))


@pytest.mark.parametrize("shape", [(40, 40), (13, 29), (29, 13), (1, 17), (17, 1)])
@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_loop_and_vectorised_forms_agree(shape, sub, dtype):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    m, n = shape
    a = random_csr(rng, m, n, density=0.3, dtype=dtype, empty_rows=0.2)
    b = random_csr(rng, m, n, density=0.3, dtype=dtype, empty_rows=0.2)
    # signed zeros and a few exact cancellations
    b[2][: b[2].size // 4] = 0.0
    loop = spadd_ref.add_sub_loop(m, n, a, b, sub)
    fast = spadd_ref.add_sub_fast(m, n, a, b, sub)
    same_bits(loop, fast)
    # the union, nothing dropped: nnz(C) = nnz(A) + nnz(B) - matched
    assert int(fast[0][-1]) == int(a[0][-1]) + int(b[0][-1]) - spadd_ref.matched(m, a, b)
    # A - A keeps every position with +0.0
    p, i, v = spadd_ref.add_sub_fast(m, n, a, a, True)
    assert np.array_equal(p, a[0]) and np.array_equal(i, a[1])
    assert np.all(v == 0) and not np.signbit(v).any()


# ---- the Python binding: host-side checks ------------------------------------------------------------------------
def test_shape_mismatch_panics_before_the_device():
    a = sp.CsrMatrix(2, 3, [0, 1, 2], [0, 2], np.array([1.0, 2.0]))
    b = sp.CsrMatrix(3, 3, [0, 1, 1, 2], [0, 1], np.array([1.0, 2.0]))
    c = sp.CsrMatrix(2, 4, [0, 1, 2], [0, 3], np.array([1.0, 2.0]))
    d = sp.CsrMatrix(3, 4, [0, 1, 1, 2], [0, 3], np.array([1.0, 2.0]))
    with pytest.raises(sp.Panic, match=r"assertion failed: nrows == rhs.nrows \(left: 2, right: 3\)"):
        a + b
    with pytest.raises(sp.Panic, match=r"assertion failed: ncols == rhs.ncols \(left: 3, right: 4\)"):
        a - c
    with pytest.raises(sp.Panic, match=r"nrows == rhs.nrows \(left: 2, right: 3\)"):   # nrows is asserted first
        a + d
    assert not a._dev and not b._dev and not c._dev and not d._dev       # no device copy was made
    e = sp.CscMatrix(2, 3, [0, 1, 1, 2], [0, 1], np.array([1.0, 2.0]))
    f = sp.CscMatrix(4, 3, [0, 1, 2, 2], [0, 3], np.array([1.0, 2.0]))
    with pytest.raises(sp.Panic, match=r"nrows == rhs.nrows \(left: 2, right: 4\)"):
        e - f
    assert not e._dev and not f._dev


def test_mixed_formats_and_non_matrices_are_type_errors():
    a = sp.CsrMatrix(2, 2, [0, 1, 2], [0, 1], np.array([1.0, 2.0]))
    b = sp.CscMatrix(2, 2, [0, 1, 2], [0, 1], np.array([1.0, 2.0]))
    for x, y in ((a, b), (b, a)):
        with pytest.raises(TypeError):
            x + y
        with pytest.raises(TypeError):
            x - y
    for other in (1.0, np.ones(2), "a"):
        with pytest.raises(TypeError):
            a + other
        with pytest.raises(TypeError):
            b - other
    assert not a._dev and not b._dev


# ---- ISA ---------------------------------------------------------------------------------------------------------
def _kernel_bodies(asm: str) -> dict:
    bodies = {}
    for m in re.finditer(r"^(\S*spadd_\S*):[^\n]*$(.*?)^\.Lfunc_end", asm, flags=re.M | re.S):
        bodies[m.group(1)] = m.group(2)
    return bodies


def test_neg_is_a_sign_flip_and_the_sums_are_plain_adds(tmp_path):
    out = tmp_path / "spadd.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only",
                           "-S", SRC, "-o", str(out)])
    bodies = _kernel_bodies(out.read_text())
    neg = [b for k, b in bodies.items() if "spadd_neg" in k]
    assert len(neg) == 2, sorted(bodies)
    for body in neg:   # -x flips the sign bit (NaN included); 0 - x would be an arithmetic op
        assert "v_xor_b32" in body
        assert not re.search(r"\bv_(add|sub|subrev|mul)_f(32|64)", body)
    fills = [b for k, b in bodies.items() if "spadd_tile" in k]
    assert len(fills) == 8, sorted(bodies)
    for body in fills:
        assert not re.search(r"\bv_(fma|fmac|mad|mac|pk_fma)_", body)
