"""Builds tests/cpp/test_krylov_loops.cpp -- a stand-alone host program that includes nothing of the library but
spalinalg_amd/csrc/krylov_loops.hpp -- under -fsanitize=address,undefined and runs it on the CPU: the CG and BiCGStab
loops enqueue, on a recording driver, exactly the launch sequences written out below, and poll on the
schedule "krylov_check_every" promises.  The expected sequences are this file's text, not the header's output."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

N = "-,-,-,-"   # an update that names only a and b
START = ["mul(X,q)", "V_INIT(B,q,-,-,-,r)", "F_INIT(0)"]
CG_PROLOGUE = {False: ["V_COPY_DOT(r,r,-,-,-,p)", "F_RZ(0)"],
               True: ["prec(r,z)", "V_COPY_DOT(r,z,-,-,-,p)", "F_RZ(0)"]}
CG_ITERATION = {False: ["mul(p,q)", f"V_DOT(p,q,{N})", "F_ALPHA_CG(0)", "V_CG_XR(p,q,-,-,X,r)", "F_TEST_CG(1)",
                        "V_CG_P(r,-,-,-,-,p)"],
                True: ["mul(p,q)", f"V_DOT(p,q,{N})", "F_ALPHA_CG(0)", "V_CG_XR(p,q,-,-,X,r)", "F_TEST_CG(0)",
                       "prec(r,z)", f"V_DOT(r,z,{N})", "F_BETA(0)", "V_CG_P(z,-,-,-,-,p)"]}
BI_PROLOGUE = ["copy(rhat,r)", "zero(v)", "zero(p)"]
# s lives in q; ph / sh are p / s (that is, q) without a preconditioner
BI_ITERATION = {False: [f"V_DOT(rhat,r,{N})", "F_RHO(0)", "V_BI_P(r,v,-,-,-,p)", "mul(p,v)", f"V_DOT(rhat,v,{N})",
                        "F_ALPHA_BI(0)", "V_BI_S(r,v,-,-,-,q)", "F_HALF(0)", "V_BI_HALF(p,q,-,-,X,r)", "mul(q,t)",
                        f"V_DOT2(t,q,{N})", "F_OMEGA(0)", "V_BI_XR(p,q,q,t,X,r)", "F_TEST_BI(0)"],
                True: [f"V_DOT(rhat,r,{N})", "F_RHO(0)", "V_BI_P(r,v,-,-,-,p)", "prec(p,ph)", "mul(ph,v)",
                       f"V_DOT(rhat,v,{N})", "F_ALPHA_BI(0)", "V_BI_S(r,v,-,-,-,q)", "F_HALF(0)",
                       "V_BI_HALF(ph,q,-,-,X,r)", "prec(q,sh)", "mul(sh,t)", f"V_DOT2(t,q,{N})", "F_OMEGA(0)",
                       "V_BI_XR(ph,sh,q,t,X,r)", "F_TEST_BI(0)"]}
PROLOGUE = {"cg": CG_PROLOGUE, "bicgstab": {False: BI_PROLOGUE, True: BI_PROLOGUE}}
ITERATION = {"cg": CG_ITERATION, "bicgstab": BI_ITERATION}


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("krylov_loops") / "test_krylov_loops")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "spalinalg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_krylov_loops.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    found = {}
    for line in out.stdout.splitlines():
        name, rest = line.split(": ", 1)
        status, trace = rest.split(" |", 1)
        found[name] = (int(status), trace.split())
    return found


def test_the_header_needs_no_hip():
    text = open(os.path.join(ROOT, "spalinalg_amd", "csrc", "krylov_loops.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<cstdint>"]


def test_start_is_the_product_the_residual_and_its_scalars(traces):
    assert traces["start"] == (0, START)


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "pre"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_loop_enqueues_the_sequence_of_the_contract(traces, method, pre):
    expected = PROLOGUE[method][pre] + 2 * ITERATION[method][pre] + ["poll"]
    assert traces[f"{method}_{'pre' if pre else 'plain'}"] == (0, expected)


@pytest.mark.parametrize("method", ["cg", "bicgstab"])
@pytest.mark.parametrize("case, batches", [("0_8", []), ("5_2", [2, 2, 1]), ("5_8", [5]), ("40_1_stop3", [1, 1, 1])])
def test_poll_schedule(traces, method, case, batches):
    """min(check_every, maxit - enqueued) iterations, then a poll; no iteration after the poll that reports the stop; one
    poll when maxit = 0."""
    expected = list(PROLOGUE[method][False])
    for b in batches:
        expected += b * ITERATION[method][False] + ["poll"]
    if not batches:
        expected += ["poll"]
    status, trace = traces[f"{method}_{case}"]
    assert status == 0
    assert trace == expected
    assert trace.count("poll") == max(1, len(batches))
    assert trace.count(ITERATION[method][False][0]) == sum(batches)


@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_a_failed_call_ends_the_loop_at_once(traces, method):
    status, trace = traces[f"{method}_fail6"]
    assert status == 7
    assert trace == (PROLOGUE[method][False] + ITERATION[method][False])[:5]
