"""Host side of Y = A * X (SpMM): the entry points exist, argument checks answer before any device work, nothing falls
back to the CPU, and the device code multiplies and adds separately with no float atomics.  None of this needs a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "spalinalg_amd", "csrc", "spal_spmm.hip")
FUSED = ("v_fma_f64", "v_fmac_f64", "v_fma_f32", "v_fmac_f32", "v_mad_f32", "v_mac_f32", "v_pk_fma_f32", "v_fma_mix")
NAMES = [f"spal_{fmt}_spmm_{form}{sfx}" for fmt in ("csr", "csc") for form in ("", "dev_") for sfx in ("f64", "f32")]


def test_the_eight_entry_points_are_declared_and_exported():
    names = _ffi.exported_names()
    lib = _ffi.lib()
    assert len(NAMES) == 8
    for n in NAMES:
        assert n in names
        assert hasattr(lib, n)


@pytest.mark.parametrize("name", NAMES)
def test_null_handle_is_an_invalid_argument(name):
    fn = getattr(_ffi.lib(), name)
    u, buf = C.c_uint64, (C.c_double * 4)()
    if "_dev_" in name:
        st = fn(None, u(1), buf, u(1), buf, u(1), None)
    else:
        st = fn(None, u(1), buf, u(1), u(1), buf, u(1), u(1))
    assert st == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert b"handle is NULL" in _ffi.lib().spal_last_error()


@pytest.mark.parametrize("cls", [sp.CsrMatrix, sp.CscMatrix])
def test_wrong_first_dimension_panics_before_the_device(cls):
    ptr = [0, 1, 2] if cls is sp.CsrMatrix else [0, 1, 1, 2]
    a = cls(2, 3, ptr, [0, 1] if cls is sp.CscMatrix else [0, 2], np.array([1.0, 2.0]))
    with pytest.raises(sp.Panic, match=r"assertion failed: ncols == rhs.nrows \(left: 3, right: 4\)"):
        a @ np.ones((4, 2))
    with pytest.raises(sp.Panic, match=r"ncols == rhs.nrows \(left: 3, right: 2\)"):
        a * np.ones((2, 5))
    with pytest.raises(TypeError):
        a @ np.ones((3, 2, 2))
    with pytest.raises(TypeError):
        a @ np.float64(2.0)
    assert not a._dev              # no device copy was made


def test_no_cpu_fallback_for_a_block():
    if sp.device_count() > 0:
        pytest.skip("a GPU is present: the no-device error path cannot be exercised")
    a = sp.CsrMatrix(2, 3, [0, 1, 2], [0, 2], np.array([1.0, 2.0]))
    with pytest.raises(sp.SpalError) as e:
        a @ np.ones((3, 3))
    assert e.value.status == _ffi.SPAL_ERR_NO_DEVICE


def _kernel_bodies(asm: str) -> dict:
    """{kernel symbol: its instructions} for the spmm kernels of a device assembly listing."""
    bodies = {}
    for m in re.finditer(r"^(\S*spmm_\S*):[^\n]*$(.*?)^\s*s_endpgm", asm, flags=re.M | re.S):
        bodies[m.group(1)] = m.group(2)
    return bodies


def test_spmm_kernels_multiply_and_add_separately_without_float_atomics(tmp_path):
    out = tmp_path / "spmm.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only",
                           "-S", SRC, "-o", str(out)])
    bodies = _kernel_bodies(out.read_text())
    tiles = [k for k in bodies if "spmm_csr_tile" in k]
    assert len(tiles) == 12, sorted(bodies)          # 6 column tiles x 2 types
    for name in tiles:
        body = bodies[name]
        for f in FUSED:
            assert f not in body, (name, f)
        assert len(re.findall(r"\bv_mul_f(32|64)", body)) > 0, name     # the products are there, as separate multiplies
        assert len(re.findall(r"\bv_add_f(32|64)", body)) > 0, name
    for name, body in bodies.items():
        # no float atomic of any kind (global, flat, buffer or LDS); the integer ones that list long rows are fine
        assert not re.search(r"atomic\w*_(pk_)?(add|min|max|fmin|fmax)\w*_(f16|bf16|f32|f64)", body), name
        assert not re.search(r"\bds_\w*_(rtn_)?(f32|f64|f16|bf16)\b", body), name
        assert not re.search(r"\bds_(add|min|max|pk_add)\w*f(32|64)", body), name
    f64 = [bodies[k] for k in tiles if "IdLi" in k]
    f32 = [bodies[k] for k in tiles if "IfLi" in k]
    assert len(f64) == 6 and all("v_mul_f64" in b for b in f64)
    assert len(f32) == 6 and all("v_mul_f32" in b for b in f32)
