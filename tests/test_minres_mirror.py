"""Builds and runs the C++ mirror test of MINRES (include/spalinalg.hpp minres, minres_block) against the C ABI."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("minres_mirror") / "test_minres_mirror")
    src = os.path.join(ROOT, "tests", "cpp", "test_minres_mirror.cpp")
    lib = os.path.join(ROOT, "spalinalg_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src,
                           "-o", out, "-L", lib, "-lspal_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_minres_mirror_host(exe):
    out = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "minres mirror host ok" in out.stdout


@pytest.mark.gpu
def test_minres_mirror_gpu(exe):
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "minres mirror gpu ok" in out.stdout
