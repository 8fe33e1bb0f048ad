"""The host layer the sparse operations share (spal_ops.hpp), through the C ABI: a refused call nulls its out, for every
result-producing operation of either handle type, and the objects the operations add to a describe() line compose in
their fixed order.  These paths are host code: the matrices (2 x 3, 3 x 3, 4 x 4) only have to reach them."""
import ctypes as C
import json

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi

pytestmark = pytest.mark.gpu

KINDS = ["csr", "csc"]
SENTINEL = 0x1234       # never dereferenced


def rect(kind, dtype=np.float64):
    """2 x 3 with entries (0, 0) and (1, 1)."""
    v = np.array([1, 2], dtype=dtype)
    if kind == "csr":
        return sp.CsrMatrix(2, 3, [0, 1, 2], [0, 1], v).device()
    return sp.CscMatrix(2, 3, [0, 1, 2, 2], [0, 1], v).device()


def no_middle_diagonal(kind):
    """3 x 3 with entries (0, 0), (1, 0) and (2, 2): the middle row stores no diagonal."""
    v = np.array([1.0, 2.0, 3.0])
    if kind == "csr":
        return sp.CsrMatrix(3, 3, [0, 1, 2, 3], [0, 0, 2], v).device()
    return sp.CscMatrix(3, 3, [0, 2, 2, 3], [0, 1, 2], v).device()


def bidiagonal(kind):
    """4 x 4 lower bidiagonal with a full diagonal, f64."""
    v = np.array([2.0, 1.0, 2.0, 1.0, 2.0, 1.0, 2.0])
    if kind == "csr":
        return sp.CsrMatrix(4, 4, [0, 1, 3, 5, 7], [0, 0, 1, 1, 2, 2, 3], v).device()
    return sp.CscMatrix(4, 4, [0, 2, 4, 6, 7], [0, 1, 1, 2, 2, 3, 3], v).device()


@pytest.mark.parametrize("kind", KINDS)
def test_a_refused_call_nulls_its_out(kind):
    lib = _ffi.lib()
    a, a32, hole = rect(kind), rect(kind, np.float32), no_middle_diagonal(kind)

    def refused(name, message, *handles):
        out = C.c_void_p(SENTINEL)
        status = getattr(lib, f"spal_{kind}_{name}")(*[h._h for h in handles], None, C.byref(out))
        text = lib.spal_last_error().decode()
        assert status != _ffi.SPAL_OK and message in text, (name, status, text)
        assert out.value is None, name

    # the messages are those tests/test_gpu_spgemm.py, test_gpu_spadd.py and test_gpu_ilu.py match
    refused("mul", "assertion failed: ncols == rhs.nrows (left: 3, right: 2)", a, a)
    for name in ("add", "sub"):
        refused(name, "assertion failed: nrows == rhs.nrows (left: 2, right: 3)", a, hole)
    refused("add", f"spal_{kind}_add: operands of element sizes 8 and 4", a, a32)
    refused("ilu0", "not square (2 x 3)", a)
    refused("ilu0", f"spal_{kind}_ilu0: row 1 stores no diagonal entry", hole)


def raw_describe(dev):
    buf = C.create_string_buffer(16384)
    _ffi.check(dev._fn("describe")(dev._h, buf, C.c_size_t(len(buf))))
    text = buf.value.decode()
    json.loads(text)        # one valid JSON line, whatever was appended
    return text


def assert_objects(text, present, absent):
    """`present` appear as keys in that order, `absent` not at all."""
    at = [text.index(f'"{key}": {{') for key in present]
    assert at == sorted(at), (present, at)
    for key in absent:
        assert f'"{key}"' not in text, key


@pytest.mark.parametrize("kind", KINDS)
def test_the_objects_compose(kind):
    a = bidiagonal(kind)
    c = a.mul(a)
    assert c.spmm(np.ones((4, 2))).shape == (4, 2)
    c.trsv_analyse(lower=True)
    assert_objects(raw_describe(c), ["spgemm", "spmm", "trsv"], ["spadd", "ilu0"])
    assert_objects(raw_describe(c.add(c)), ["spadd"], ["spgemm"])
    assert_objects(raw_describe(c.ilu0()), ["trsv", "ilu0"], [])
