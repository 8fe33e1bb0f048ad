"""CPU-side tests of the sparse x sparse product (spal_csr_mul / spal_csc_mul): the ABI, the host-side panics of the
Python binding, and the kernels' ISA (products are rounded before they are added: no fused multiply-add)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import spalinalg_amd as sp
from spalinalg_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "spalinalg_amd", "csrc", "spal_spgemm.hip")
FUSED = ("v_fma_f64", "v_fmac_f64", "v_fma_f32", "v_fmac_f32", "v_mad_f32", "v_mac_f32", "v_pk_fma_f32", "v_fma_mix")


def test_mul_entry_points_declared_and_exported():
    names = _ffi.exported_names()
    lib = _ffi.lib()
    for n in ("spal_csr_mul", "spal_csc_mul"):
        assert n in names
        assert hasattr(lib, n)


@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_mul_null_arguments(fmt):
    fn = getattr(_ffi.lib(), f"spal_{fmt}_mul")
    out = C.c_void_p()
    assert fn(None, None, None, C.byref(out)) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert fn(None, None, None, None) == _ffi.SPAL_ERR_INVALID_ARGUMENT
    assert b"null" in _ffi.lib().spal_last_error()


def test_csr_mul_dimension_mismatch_panics_before_the_device():
    a = sp.CsrMatrix(2, 3, [0, 1, 2], [0, 2], np.array([1.0, 2.0]))
    b = sp.CsrMatrix(4, 2, [0, 1, 1, 1, 2], [0, 1], np.array([1.0, 2.0]))
    with pytest.raises(sp.Panic, match=r"assertion failed: ncols == rhs.nrows \(left: 3, right: 4\)"):
        a * b
    with pytest.raises(sp.Panic, match="ncols == rhs.nrows"):
        a @ b
    assert not a._dev and not b._dev       # no device copy was made


def test_csc_mul_dimension_mismatch_panics():
    a = sp.CscMatrix(2, 3, [0, 1, 1, 2], [0, 1], np.array([1.0, 2.0]))
    b = sp.CscMatrix(4, 2, [0, 1, 2], [0, 3], np.array([1.0, 2.0]))
    with pytest.raises(sp.Panic, match=r"left: 3, right: 4"):
        a * b


def test_mixed_csr_csc_is_a_type_error():
    a = sp.CsrMatrix(2, 2, [0, 1, 2], [0, 1], np.array([1.0, 2.0]))
    b = sp.CscMatrix(2, 2, [0, 1, 2], [0, 1], np.array([1.0, 2.0]))
    with pytest.raises(TypeError):
        a * b
    with pytest.raises(TypeError):
        b * a


def _kernel_bodies(asm: str) -> dict:
    """{kernel symbol: its instructions} for the spgemm_* kernels of a device assembly listing."""
    bodies = {}
    for m in re.finditer(r"^(\S*spgemm_\S*):[^\n]*$(.*?)^\s*s_endpgm", asm, flags=re.M | re.S):
        bodies[m.group(1)] = m.group(2)
    return bodies


def test_spgemm_kernels_have_no_fused_multiply_add(tmp_path):
    out = tmp_path / "spgemm.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only",
                           "-S", SRC, "-o", str(out)])
    bodies = _kernel_bodies(out.read_text())
    # the LDS tiers (symbolic + numeric, 5 geometries, 2 types), the expand and run-sum kernels of the large tier
    assert sum("spgemm_lds" in k for k in bodies) == 20, sorted(bodies)
    assert any("spgemm_expand" in k for k in bodies) and any("spgemm_run_fill" in k for k in bodies)
    mults = 0
    for name, body in bodies.items():
        for f in FUSED:
            assert f not in body, (name, f)
        mults += len(re.findall(r"\bv_mul_f(32|64)", body))
    assert mults > 0          # (the products are there, as separate multiplies)


def test_contract_off_toy_kernel_emits_separate_mul_and_add(tmp_path):
    """The check above can see an FMA: without the pragma the same toy kernel contracts."""
    src = tmp_path / "toy.hip"
    body = ("#include <hip/hip_runtime.h>\n%s\n__global__ void toy(double *a, const double *b, const double *c)"
            " { a[threadIdx.x] = a[threadIdx.x] + b[threadIdx.x] * c[threadIdx.x]; }\n")
    for pragma, fused in (("#pragma clang fp contract(off)", False), ("", True)):
        src.write_text(body % pragma)
        out = tmp_path / "toy.s"
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                               str(src), "-o", str(out)])
        asm = out.read_text()
        assert any(f in asm for f in FUSED) == fused
        if not fused:
            assert "v_mul_f64" in asm and "v_add_f64" in asm
