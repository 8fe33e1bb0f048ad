"""Packed values (spalinalg_amd/csrc/csr_valpack.hpp) without a product: the codec as a stand-alone host program under
-fsanitize=address,undefined (tests/cpp/test_valpack_codec.cpp), the packed-value sliding kernels' register footprint
and arithmetic in the device assembly, and the two options."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spalinalg_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_codec_round_trips_and_refuses_at_the_bounds(tmp_path):
    exe = str(tmp_path / "test_valpack_codec")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "test_valpack_codec.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    status, cases = out.stdout.split()
    assert status == "ok" and int(cases) > 50_000


def test_packed_kernels_use_no_scratch_and_no_more_registers(tmp_path):
    """Every field of a block sits at a compile-time place: the decode indexes no register dynamically, so the
    packed-value kernels (L = 12, 14, 16) keep everything in registers -- at most the 165 of the record form, which
    keeps two workgroups per CU -- and every product and sum is rounded on its own (no fused multiply-add)."""
    out = tmp_path / "slide.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics",
                           "--cuda-device-only", "-S", os.path.join(CSRC, "spal_csr_slide.hip"), "-o", str(out)])
    asm = out.read_text()
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, flags=re.S):
        k = re.search(r"csr_spmv_slide_valpackILi(12|14|16)ELi2EE", m.group(1))
        if k:
            body = asm[asm.index("\n" + m.group(1) + ":"):]
            body = body[:body.index(".Lfunc_end")]
            found[int(k.group(1))] = (int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(2)).group(1)),
                                      int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", m.group(2)).group(1)),
                                      len(re.findall(r"\bv_fma(c|ak|mk)?_f64", body)))
    assert sorted(found) == [12, 14, 16], sorted(found)
    assert all(scratch == 0 and vgprs <= 165 and fused == 0 for scratch, vgprs, fused in found.values()), found


@pytest.mark.gpu
def test_options_are_checked_and_valpack_0_keeps_the_values():
    import spalinalg_amd as sp
    import spal_synth as synth
    n = 4096
    rp, ci, va = synth.banded_csr(n, n, 14, 4096, 3)
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    for key, bad in (("valpack", -2), ("valpack", 2), ("valpack_on", -1), ("valpack_on", 2)):
        with pytest.raises(sp.Panic):
            dev.set_option(key, bad)
    d = dev.describe()
    assert d["slide"] == 1 and d["rowrec"] == 1 and d["valpack"] == 1 and d["valpack_on"] == 1, d
    assert d["valpack_bytes_per_row"] == 96 and d["valpack_failed"] == 0, d
    x = synth.vector(n)
    y1 = dev.spmv(x)
    dev.set_option("valpack", 0)
    d = dev.describe()
    assert d["valpack"] == 0 and d["valpack_on"] == 0 and d["valpack_bytes_per_row"] == 0 and d["rowrec_on"] == 1, d
    assert np.array_equal(dev.spmv(x).view(np.uint64), y1.view(np.uint64))
    dev.set_option("valpack", 1)
    assert dev.describe()["valpack"] == 1
    dev.set_option("valpack_on", 0)
    d = dev.describe()
    assert d["valpack"] == 1 and d["valpack_on"] == 0, d
    assert np.array_equal(dev.spmv(x).view(np.uint64), y1.view(np.uint64))
    dev.set_option("rowrec_on", 0)          # no records, no packed values: they ride on the record form
    dev.set_option("valpack_on", 1)
    d = dev.describe()
    assert d["rowrec_on"] == 0 and d["valpack_on"] == 0, d
    assert np.array_equal(dev.spmv(x).view(np.uint64), y1.view(np.uint64))
