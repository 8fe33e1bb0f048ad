"""Builds tests/cpp/test_eigsh_asan.cpp -- a stand-alone host program, not Python -- with the host side of spal_eigsh.hip
and spal_host.cpp under -fsanitize=address,undefined and runs it on the CPU: the Jacobi text (spal_eigsh_jacobi) on
buffers of exactly the claimed size, and the refusals of every eigsh entry point that need no device.  No GPU is touched:
every call ends before any device work, and the device code of spal_eigsh.hip is compiled unoptimised only because its
host object refers to it.  The iteration needs a device; tests/test_gpu_eigsh.py covers it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spalinalg_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]


def test_eigsh_host_text_and_refusals_under_asan_ubsan(tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "test_eigsh_asan")
    lib = os.path.join(ROOT, "spalinalg_amd", "lib")
    host_san = [f for s in SAN for f in ("-Xarch_host", s)]
    objs, procs = [], []
    for src in ("spal_eigsh.hip", "spal_host.cpp"):
        obj = str(tmp_path / (src + ".o"))
        objs.append(obj)
        lang = ["-x", "hip"] if src.endswith(".cpp") else []
        procs.append(subprocess.Popen(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
                                       "-Xarch_device", "-O0", *host_san, *lang, "-c", os.path.join(CSRC, src), "-o", obj]))
    assert [p.wait(timeout=600) for p in procs] == [0, 0]
    # the program's own copies of the entry points come first; everything else they refer to is the built library's
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", *SAN, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_eigsh_asan.cpp"), *objs, "-o", exe,
                           "-L", lib, "-lspal_hip", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "eigsh sanitize ok" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
