"""Builds tests/cpp/test_minres_loops.cpp -- a stand-alone host program that includes nothing of the library but
spalinalg_amd/csrc/krylov_loops.hpp -- under -fsanitize=address,undefined and runs it on the CPU: minres_start and
minres_loop enqueue, on a recording driver, exactly the launch sequences written out below, rotate their
buffers by exchanging operands, and poll on the schedule "krylov_check_every" promises.  The expected sequences are this
file's text, not the header's output."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

N = "-,-,-,-"
# buffers: v; the ring ra, rb, rc (r1 = ra is zeroed, the first residual r2 lives in rb); the ring wa, wb; y with M
START = {False: ["mul(X,rb)", "V_MR_R0(B,rb,X,-,-,rb)", "F_MR_INIT(1)", "zero(ra)", "zero(wa)", "zero(wb)",
                 f"V_MR_V(rb,{N},v)"],
         True: ["prec(B,y)", f"V_DOT(B,y,{N})", "F_MR_BB(0)", "mul(X,rb)", "V_MR_R0(B,rb,X,-,-,rb)", "prec(rb,y)",
                f"V_DOT(rb,y,{N})", "F_MR_INIT(0)", "zero(ra)", "zero(wa)", "zero(wb)", f"V_MR_V(y,{N},v)"]}
R = ["ra", "rb", "rc"]
W = ["wa", "wb"]


def iteration(j, pre):
    """Iteration j (from 0): r1, r2, t are ring buffers j, j + 1, j + 2 (mod 3) -- the product writes the next t into
    the buffer r1 left an iteration ago --, w1, w2 are j, j + 1 (mod 2) and w goes over w1; six launches without M."""
    r1, r2, t = R[j % 3], R[(j + 1) % 3], R[(j + 2) % 3]
    w1, w2 = W[j % 2], W[(j + 1) % 2]
    if pre:
        return [f"mul(v,{t})", f"V_MR_T1(v,{r1},-,-,-,{t})", "F_MR_ALFA(0)", f"V_MR_T2_PRE({r2},{N},{t})", f"prec({t},y)",
                f"V_DOT({t},y,{N})", "F_MR_ROT(0)", f"V_MR_WX(y,{w2},-,-,X,{w1},v)"]
    return [f"mul(v,{t})", f"V_MR_T1(v,{r1},-,-,-,{t})", "F_MR_ALFA(0)", f"V_MR_T2({r2},{N},{t})", "F_MR_ROT(0)",
            f"V_MR_WX({t},{w2},-,-,X,{w1},v)"]


def iterations(count, pre=False, first=0):
    out = []
    for j in range(first, first + count):
        out += iteration(j, pre)
    return out


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("minres_loops") / "test_minres_loops")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "spalinalg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_minres_loops.cpp"), "-o", exe])
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


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "pre"])
def test_start(traces, pre):
    assert traces[f"start_{'pre' if pre else 'plain'}"] == (0, START[pre])


def test_an_unpreconditioned_iteration_is_six_launches():
    assert len(iteration(0, False)) == 6 and len(iteration(0, True)) == 8


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "pre"])
def test_loop_enqueues_the_sequence_and_rotates_operands(traces, pre):
    """Seven iterations: the ring of three comes round twice, the ring of two three times; nothing is copied."""
    status, trace = traces["pre" if pre else "plain"]
    assert status == 0 and trace == iterations(7, pre) + ["poll"]
    assert not any(t.startswith("copy") or t.startswith("zero") for t in trace)
    # the buffer the product fills is the one r1 left in the iteration before
    for j in range(1, 7):
        assert iteration(j, pre)[0] == f"mul(v,{R[(j - 1) % 3]})"


@pytest.mark.parametrize("case, batches", [("0_8", []), ("5_2", [2, 2, 1]), ("5_8", [5]), ("40_1_stop3", [1, 1, 1])])
def test_poll_schedule(traces, case, batches):
    """min(check_every, maxit - enqueued) iterations, then a poll; no iteration after the poll that reports the stop; one
    poll when maxit = 0."""
    expected, j = [], 0
    for b in batches:
        expected += iterations(b, False, j) + ["poll"]
        j += b
    if not batches:
        expected += ["poll"]
    status, trace = traces[case]
    assert status == 0
    assert trace == expected
    assert trace.count("poll") == max(1, len(batches))
    assert sum(t.startswith("mul(") for t in trace) == sum(batches)


def test_a_failed_call_ends_the_loop_at_once(traces):
    status, trace = traces["fail4"]
    assert status == 7
    assert trace == iteration(0, False)[:3]
