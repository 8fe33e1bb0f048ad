"""Builds tests/cpp/test_fsai_asan.cpp -- a stand-alone host program, not Python -- with spalinalg_amd/csrc/fsai_host.hpp
under -fsanitize=address,undefined and runs it on the CPU: the text's Cholesky and back-substitution on exact-size
buffers for m = 1 .. 64, in place and out of place, and every kind of rejected row.  The header is plain C++ and needs
neither the library nor a device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]


def test_fsai_host_header_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_fsai_asan")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", *SAN, "-I", os.path.join(ROOT, "spalinalg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_fsai_asan.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fsai sanitize ok" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
