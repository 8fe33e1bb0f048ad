"""Row records (spalinalg_amd/csrc/csr_rowrec.hpp) without a product: the codec as a stand-alone host program under
-fsanitize=address,undefined (tests/cpp/test_rowrec_codec.cpp), the record-form sliding kernels' register footprint in
the device assembly, and the two options."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spalinalg_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_codec_round_trips_and_refuses_at_the_bounds(tmp_path):
    exe = str(tmp_path / "test_rowrec_codec")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "test_rowrec_codec.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    status, cases = out.stdout.split()
    assert status == "ok" and int(cases) > 50_000


def test_record_kernels_use_no_scratch(tmp_path):
    """Every field of a record sits at a compile-time place: the decode indexes no register dynamically, so the
    record-form kernels (template argument REC = 12, 14, 16; f64 and f32) keep everything in registers."""
    out = tmp_path / "slide.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics",
                           "--cuda-device-only", "-S", os.path.join(CSRC, "spal_csr_slide.hip"), "-o", str(out)])
    asm = out.read_text()
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, flags=re.S):
        k = re.search(r"csr_spmv_slideI([df])Li64ELi([678])ELb1ELi2ELi(12|14|16)EE", m.group(1))
        if k:
            found[(k.group(1), int(k.group(2)), int(k.group(3)))] = int(
                re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(2)).group(1))
    assert sorted(found) == [(t, rec // 2, rec) for t in "df" for rec in (12, 14, 16)], sorted(found)
    assert all(v == 0 for v in found.values()), found


@pytest.mark.gpu
def test_options_are_checked_and_rowrec_0_keeps_col16():
    import spalinalg_amd as sp
    import spal_synth as synth
    n = 4096
    rp, ci, va = synth.banded_csr(n, n, 14, 4096, 3)
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    for key, bad in (("rowrec", -2), ("rowrec", 2), ("rowrec_on", -1), ("rowrec_on", 2)):
        with pytest.raises(sp.Panic):
            dev.set_option(key, bad)
    d = dev.describe()
    assert d["slide"] == 1 and d["rowrec"] == 1 and d["rowrec_on"] == 1 and d["rowrec_bytes_per_row"] == 20, d
    assert d["rowrec_failed"] == 0 and d["index_bits"] == 16
    dev.set_option("rowrec", 0)
    d = dev.describe()
    assert d["rowrec"] == 0 and d["rowrec_on"] == 0 and d["rowrec_bytes_per_row"] == 0, d
    dev.set_option("rowrec", 1)
    assert dev.describe()["rowrec"] == 1
    dev.set_option("rowrec_on", 0)
    d = dev.describe()
    assert d["rowrec"] == 1 and d["rowrec_on"] == 0, d
    x = synth.vector(n)
    y0 = dev.spmv(x)
    dev.set_option("rowrec_on", 1)
    assert np.array_equal(dev.spmv(x).view(np.uint64), y0.view(np.uint64))
