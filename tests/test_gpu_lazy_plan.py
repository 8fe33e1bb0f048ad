"""Device-assembled CSR handles on every path of the planner.

A handle that comes out of the COO assembly is the only kind whose product plan is built lazily, by whoever first needs
it (csr_ensure_plan, under the handle's lock).  Every other test of the planner uploads host arrays, which plan inside
the create call.  Here every case of tests/lazy_cases.py -- one per planner path, the skewed ones among them, whose
plan is decided by a timed race of two product forms -- is assembled from shuffled triplets and then touched for the
FIRST time in every way the library offers; nothing else touches the handle before.  The twin of a case is the same
matrix uploaded from the host.

Reference: oracle.csr_spmv / oracle.csr_abs_bound through assert_spmv_close at the tolerances of the block-window and
row-split tests (1e-10 f64, 1e-4 f32); rows of at most 32 entries of the skewed cases and every row of the stream cases
bit for bit.  Outputs are prefilled with NaN.

The skewed cases used to hang in their first touch (the planner's timed launches re-entered csr_ensure_plan on the
thread that held its lock).  `canary` runs that touch once in a child process with a time limit; every in-process
test of a skewed case depends on it and ERRORS -- neither hangs nor skips -- should the deadlock return.
"""
import functools
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import spalinalg_amd as sp
from tests import lazy_cases as zoo
from tests import spadd_ref, trsv_ref
from tests.util import assert_spmv_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_CASES = ("banded", "ragged")                   # the stream kernels: the reference's order in every row
HOST_PATH = {"banded": "stream", "ragged": "stream", "long_rows": "vector"}   # what the uploaded twin must plan


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def tol_of(dtype):
    return 1e-10 if np.dtype(dtype) == np.float64 else 1e-4


def assemble(c):
    """The handle under test: COO triplets in shuffled order -> CSR on the device; its plan is pending."""
    return sp.CooMatrix.with_triplets(c.nrows, c.ncols, c.rows, c.cols, c.vals).upload().assemble_csr()


def twin(c):
    return sp.CsrMatrix(c.nrows, c.ncols, c.rowptr, c.colind, c.values).device_copy()


@functools.lru_cache(maxsize=None)
def _reference(name, dtype_name, diag):
    """(case, x, y_ref, bound, row lengths), computed once and shared (nobody writes to them)."""
    import oracle
    c = zoo.case(name, dtype_name)
    if diag:   # the same triplets and, appended, a one on every diagonal position (summed into a stored diagonal entry)
        d = np.arange(c.nrows, dtype=np.uint64)
        rows, cols = np.concatenate([c.rows, d]), np.concatenate([c.cols, d])
        vals = np.concatenate([c.vals, np.ones(c.nrows, dtype=c.vals.dtype)])
        rp, ci, va = oracle.coo_to_csr(c.nrows, c.ncols, rows, cols, vals)
        c = zoo.Case(name + "+I", c.nrows, c.ncols, rp, ci, va, rows, cols, vals)
    x = zoo.x_for(c)
    y_ref = oracle.csr_spmv(c.rowptr, c.colind, c.values, x)
    bound = oracle.csr_abs_bound(c.rowptr, c.colind, c.values.astype(np.float64), x.astype(np.float64))
    out = (c, x, y_ref, bound, np.diff(c.rowptr.astype(np.int64)))
    for a in out[1:]:
        a.setflags(write=False)
    return out


def reference(name, dtype=np.float64, diag=False):
    return _reference(name, np.dtype(dtype).name, diag)


def check_product(name, dtype, y, diag=False, skew_kernel=True):
    """y = A * x of case `name` against the oracle.  `skew_kernel`: a skewed case ran the row split or the block-window
    kernel, which sum a row of at most 32 entries in the reference's order.  With the row split
    switched off such a matrix streams as rounds 1-3 had it: the tiles that hold a long row go to the overflow kernel,
    eight lanes to a short row, and those rows are held to the tolerance alone."""
    c, x, y_ref, bound, lens = reference(name, dtype, diag)
    y = np.asarray(y)
    assert y.dtype == y_ref.dtype and y.shape == y_ref.shape
    assert not np.isnan(y).any(), f"{int(np.isnan(y).sum())} rows were not written"
    assert_spmv_close(y, y_ref, bound, tol_of(dtype))
    if name in STREAM_CASES:
        assert np.array_equal(bits(y), bits(y_ref))
    elif name in zoo.SKEWED and skew_kernel:
        short = lens <= 32          # one thread of the block-window kernel / a lane of the short part's stream kernel
        assert short.any() and np.array_equal(bits(y[short]), bits(y_ref[short]))
    assert np.all(y[lens == 0] == 0)
    if name == "empty":
        assert not bits(y).any()    # +0.0 in every row


def product(dev, name, dtype, diag=False, skew_kernel=True):
    """One product through the device entry point into an output prefilled with NaN, checked."""
    import torch
    c, x = reference(name, dtype, diag)[:2]
    xt = torch.tensor(x).cuda()
    yt = torch.full((c.nrows,), float("nan"), dtype=xt.dtype, device="cuda")
    dev.spmv_torch(xt, out=yt)
    torch.cuda.synchronize()
    y = yt.cpu().numpy()
    if name in zoo.SKEWED and skew_kernel:
        assert dev.describe()["kernel"] in ("split", "blockwin")
    check_product(name, dtype, y, diag, skew_kernel)
    return y


# ---- a. the canary -----------------------------------------------------------------------------------------------------
_CANARY = """
import sys, time
sys.path.insert(0, {root!r})
import numpy as np
import spalinalg_amd as sp
from tests import lazy_cases as zoo
c = zoo.case("skew_det")
t0 = time.perf_counter()
dev = sp.CooMatrix.with_triplets(c.nrows, c.ncols, c.rows, c.cols, c.vals).upload().assemble_csr()
y = dev.spmv(zoo.x_for(c))
print("canary", float(np.abs(y).sum()).hex(), "%.3f" % (time.perf_counter() - t0))
"""


@pytest.fixture(scope="module")
def canary(oracle):
    """The first product of an assembled, skewed matrix in a fresh child process: 600 s is the backstop the project's
    other GPU child processes use, not a measurement (the child needs a few seconds, most of them imports)."""
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, "-c", _CANARY.format(root=ROOT)], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("canary ")]
    assert len(line) == 1, out.stdout[-2000:]
    _, checksum, inner = line[0].split()
    print(f"[lazy plan canary] wall {wall:.2f} s, assembly + first product {inner} s")
    y_ref, bound = reference("skew_det")[2:4]
    assert abs(float.fromhex(checksum) - float(np.abs(y_ref.astype(np.float64)).sum())) <= 1e-10 * float(bound.sum())
    return wall


@pytest.fixture
def guarded(request):
    """Case name -> the same name; a skewed case first asks for the canary."""
    def guard(name):
        if name in zoo.SKEWED:
            request.getfixturevalue("canary")
        return name
    return guard


def test_canary_finishes_well_inside_its_cap(canary):
    assert canary < 300.0, canary


# ---- b. first touch x case ---------------------------------------------------------------------------------------------
def _torch_vectors(name, dtype):
    import torch
    c, x = reference(name, dtype)[:2]
    xt = torch.tensor(x).cuda()
    yt = torch.full((c.nrows,), float("nan"), dtype=xt.dtype, device="cuda")
    torch.cuda.synchronize()
    return torch, xt, yt


def touch_spmv(dev, name, dtype):
    check_product(name, dtype, dev.spmv(reference(name, dtype)[1]))


def touch_spmv_dev(dev, name, dtype):
    torch, xt, yt = _torch_vectors(name, dtype)
    s = torch.cuda.Stream()
    dev.spmv_dev(xt.data_ptr(), yt.data_ptr(), s)
    s.synchronize()
    check_product(name, dtype, yt.cpu().numpy())


def touch_plan(dev, name, dtype):
    dev.plan()
    dev.plan()                                   # (a second call finds it built)


def touch_describe(dev, name, dtype):
    d = dev.describe()
    c = zoo.case(name, dtype)
    assert (d["nrows"], d["ncols"], d["nnz"]) == (c.nrows, c.ncols, c.values.size), d
    if name in zoo.SKEWED:
        assert d["kernel"] in (("split",) if name == "skew_511" else ("blockwin", "split")), d


def touch_blockwin_0(dev, name, dtype):
    dev.set_option("blockwin", 0)
    if name in zoo.SKEWED:
        assert dev.describe()["kernel"] == "split"


def touch_row_split_0(dev, name, dtype):
    dev.set_option("row_split", 0)
    assert dev.describe()["kernel"] not in ("split", "blockwin")


def touch_autotune(dev, name, dtype):
    torch, xt, yt = _torch_vectors(name, dtype)
    dev.autotune(xt, yt, iters=3)
    torch.cuda.synchronize()


def touch_alloc_vectors(dev, name, dtype):
    import torch
    c, x = reference(name, dtype)[:2]
    xv, yv = dev.vectors_torch()                 # spal_csr_alloc_vectors, as torch views of the handle's block
    assert xv.numel() == c.ncols and yv.numel() == c.nrows
    xv.copy_(torch.tensor(x))
    yv.fill_(float("nan"))
    dev.spmv_torch(xv, out=yv)
    torch.cuda.synchronize()
    check_product(name, dtype, yv.cpu().numpy())


PLANNING = {"spmv": touch_spmv, "spmv_dev": touch_spmv_dev, "plan": touch_plan, "describe": touch_describe,
            "blockwin_0": touch_blockwin_0, "row_split_0": touch_row_split_0, "autotune": touch_autotune,
            "alloc_vectors": touch_alloc_vectors}


@pytest.mark.parametrize("touch", list(PLANNING))
@pytest.mark.parametrize("name", zoo.NAMES)
def test_first_touch_that_plans(oracle, guarded, name, touch):
    name = guarded(name)
    dev = assemble(zoo.case(name))
    PLANNING[touch](dev, name, np.float64)
    product(dev, name, np.float64, skew_kernel=touch != "row_split_0")
    dev.close()


@pytest.mark.parametrize("touch", ["spmv", "spmv_dev"])
@pytest.mark.parametrize("name", zoo.NAMES)
def test_first_touch_that_plans_f32(oracle, guarded, name, touch):
    name = guarded(name)
    dev = assemble(zoo.case(name, np.float32))
    PLANNING[touch](dev, name, np.float32)
    product(dev, name, np.float32)
    dev.close()


def same_arrays(got, ref):
    (gp, gi, gv), (rp, ri, rv) = got, ref
    assert np.array_equal(gp, rp) and np.array_equal(gi, ri)
    assert gv.dtype == rv.dtype and np.array_equal(bits(gv), bits(rv))


def touch_spmm(oracle, dev, c):
    X = np.random.default_rng(3).uniform(-1, 1, (c.ncols, 3))
    Y = dev.spmm(X)
    assert Y.shape == (c.nrows, 3)
    for j in range(3):
        assert np.array_equal(bits(Y[:, j]), bits(oracle.csr_spmv(c.rowptr, c.colind, c.values, X[:, j]))), j


def touch_trsv(oracle, dev, c):
    b = np.random.default_rng(4).uniform(-1, 1, c.nrows)
    trsv_ref.assert_same_bits(dev.trsv(b, lower=True),
                              trsv_ref.solve_by_levels(c.nrows, c.rowptr, c.colind, c.values, b, lower=True))


def touch_to_csc(oracle, dev, c):
    same_arrays(dev.to_csc().download(), oracle.transpose(c.nrows, c.ncols, c.rowptr, c.colind, c.values))


def touch_mul(oracle, dev, c):
    a = (c.rowptr, c.colind, c.values)
    same_arrays(dev.mul(dev).download(), oracle.csr_mul((c.nrows, c.ncols), a, (c.nrows, c.ncols), a))


def touch_add(oracle, dev, c):
    a = (c.rowptr, c.colind, c.values)
    same_arrays(dev.add(dev).download(), spadd_ref.add_sub_fast(c.nrows, c.ncols, a, a, False))


def touch_neg(oracle, dev, c):
    same_arrays(dev.neg().download(), spadd_ref.neg((c.rowptr, c.colind, c.values)))


def touch_download(oracle, dev, c):
    same_arrays(dev.download(), (c.rowptr, c.colind, c.values))


NOT_PLANNING = {"spmm": touch_spmm, "trsv": touch_trsv, "to_csc": touch_to_csc, "mul": touch_mul, "add": touch_add,
                "neg": touch_neg, "download": touch_download}
SQUARE_ONLY = ("trsv", "mul")                # (a triangle, A * A: the square cases)


@pytest.mark.parametrize("name,touch", [(n, t) for n in zoo.NAMES for t in NOT_PLANNING
                                        if t not in SQUARE_ONLY or n in zoo.SQUARE])
def test_first_touch_that_needs_no_plan(oracle, guarded, name, touch):
    """Download, conversion, SpGEMM, sums, SpMM and the triangular solve work on the assembled arrays; the product that
    follows is then the handle's first and builds the plan."""
    name = guarded(name)
    diag = touch == "trsv"                       # (every row needs a diagonal entry: ones appended to the triplets)
    c = reference(name, np.float64, diag)[0]
    dev = assemble(c)
    NOT_PLANNING[touch](oracle, dev, c)
    product(dev, name, np.float64, diag)
    dev.close()


# ---- c. the plan of the uploaded twin -----------------------------------------------------------------------------------
PLAN_KEYS = ("kernel", "rows_per_tile", "blocks", "lds_x", "lds_window_bytes", "lds_row_fraction", "stream_row_fraction",
             "index_bits", "block_rows", "window_columns", "split_threshold", "split_long_rows", "split_long_entries")


def plan_of(d):
    out = {k: d[k] for k in PLAN_KEYS if k in d}
    if "short_part" in d:
        out["short_part"] = plan_of(d["short_part"])
    return out


@pytest.mark.parametrize("name", zoo.NAMES)
def test_assembled_handle_plans_like_its_uploaded_twin(oracle, guarded, name):
    name = guarded(name)
    c, x = reference(name)[:2]
    got, ref = assemble(c), twin(c)
    if name in HOST_PATH:
        assert ref.describe()["kernel"] == HOST_PATH[name], ref.describe()
    for blockwin in (0, 1):                      # (-1 is decided by a timer: two handles may differ)
        got.set_option("blockwin", blockwin)
        ref.set_option("blockwin", blockwin)
        dg, dr = got.describe(), ref.describe()
        assert plan_of(dg) == plan_of(dr), (blockwin, dg, dr)
        if name in zoo.SKEWED and blockwin == 0:
            assert dg["kernel"] == "split", dg
        if name == "skew_far" and blockwin == 1:
            assert dg["kernel"] == "blockwin" and dg["window_columns"] == 0, dg
        yg = product(got, name, np.float64)
        assert np.array_equal(bits(yg), bits(ref.spmv(x))), (blockwin, dg)
    if name in zoo.SKEWED:
        for dev in (got, ref):
            dev.set_option("blockwin", -1)
            d = dev.describe()
            assert d["kernel"] in (("split",) if name == "skew_511" else ("blockwin", "split")), d
            product(dev, name, np.float64)
    got.close()
    ref.close()


# ---- d. two threads, first product -------------------------------------------------------------------------------------
@pytest.mark.parametrize("attempt", range(2))
def test_first_product_from_two_threads(oracle, canary, attempt):
    """Two threads issue the FIRST product of an untouched handle together, each on its own stream: the plan -- here one
    with a timed race in it -- is built once under the handle's lock, the other thread waits for it, and both results
    carry the bits of a later single-threaded product."""
    import torch
    name = "skew_pareto"
    c, x = reference(name)[:2]
    dev = assemble(c)
    xt = torch.tensor(x).cuda()
    ys = [torch.full((c.nrows,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    torch.cuda.synchronize()
    gate, errors = threading.Barrier(2), []

    def work(k):
        try:
            gate.wait()
            for _ in range(3):
                dev.spmv_dev(xt.data_ptr(), ys[k].data_ptr(), streams[k])
            streams[k].synchronize()
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    y = product(dev, name, np.float64)
    for k in range(2):
        assert np.array_equal(bits(ys[k].cpu().numpy()), bits(y)), k
    dev.close()


# ---- e. graph capture --------------------------------------------------------------------------------------------------
def _capture_after_plan(dev, name):
    """plan(), then the product captured into a graph and replayed twice."""
    import torch
    c, x = reference(name)[:2]
    xt = torch.tensor(x).cuda()
    yt = torch.empty(c.nrows, dtype=torch.float64, device="cuda")
    dev.plan()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dev.spmv_torch(xt, out=yt)               # warm-up outside the capture (module load, LDS attribute)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dev.spmv_torch(xt, out=yt)
    for _ in range(2):
        yt.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        check_product(name, np.float64, yt.cpu().numpy())


def test_first_product_refuses_a_capture_then_plans_and_captures(oracle):
    """The first product of a pending handle would build its plan (allocations, copies, host round trips): inside a stream
    capture the library refuses it by name and the handle stays pending.  spal_csr_plan before the capture is the way."""
    import torch
    name = "banded"
    c, x = reference(name)[:2]
    dev = assemble(c)
    xt = torch.tensor(x).cuda()
    yt = torch.empty(c.nrows, dtype=torch.float64, device="cuda")
    yt.fill_(0.0)                                # (the fill kernel is loaded before the capture)
    torch.cuda.synchronize()
    refused = torch.cuda.CUDAGraph()             # never replayed
    message = None
    with torch.cuda.graph(refused):
        yt.fill_(float("nan"))                   # (so that the graph is not empty)
        try:
            dev.spmv_torch(xt, out=yt)
        except sp.Panic as exc:
            message = str(exc)
    torch.cuda.synchronize()
    assert message is not None and "cannot be captured" in message, message
    del refused
    _capture_after_plan(dev, name)
    dev.close()


def test_planned_skewed_handle_captures(oracle, canary):
    dev = assemble(zoo.case("skew_det"))
    _capture_after_plan(dev, "skew_det")
    dev.close()


# ---- g. CSC from the same triplets -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["skew_pareto", "skew_far"])
def test_csc_assembled_from_the_same_triplets(oracle, canary, name, dtype):
    """`CscMatrix::from(&coo)` of a skewed matrix, then csc * x (by default through the handle's CSR form, which is planned
    eagerly): test_csc_random's criterion."""
    c, x, _, bound, _ = reference(name, dtype)
    csc = sp.CscMatrix.from_coo(sp.CooMatrix.with_triplets(c.nrows, c.ncols, c.rows, c.cols, c.vals))
    same_arrays((csc.colptr(), csc.rowind(), csc.values()), oracle.coo_to_csc(c.nrows, c.ncols, c.rows, c.cols, c.vals))
    y_ref = oracle.csc_spmv(c.nrows, csc.colptr(), csc.rowind(), csc.values(), x)
    for kernel in (2, 1):
        csc.device().set_option("kernel", kernel)
        assert_spmv_close(csc * x, y_ref, bound, tol_of(dtype))
