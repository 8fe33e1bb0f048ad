"""Colouring, permutation and the multicolour solve path on seeded random matrices against their sequential texts
(tests/colour_ref.py, ilu_ref.py, trsv_ref.py, krylov_ref.py, gmres_ref.py), one handle per seed through the whole chain:
colour -> multicolour -> permute -> vectors -> the result as a full handle -> ILU(0) exactly and by ncolours - 1 row
sweeps -> the triangular solves by ncolours - 1 sweeps -> a Krylov solve with either factor.

Every comparison is of raw bits or integers: there is no tolerance anywhere in this file.  tests/ordering_cases.py draws
the matrices (dense random blocks that need more than 64 and more than 128 colours and leave holes in the 64-colour
windows, edges stored in one direction, runs of empty rows, missing diagonals, nnz = 0, n = 1) and the knobs (colouring
seeds at and above 2^32, the stream, a device-assembled or a computed operand, which ordering call comes first);
tests/test_ordering_cases_host.py proves on the CPU that the default seeds reach those conditions.

The composite invariant (DESIGN 3.18 + 3.19 + 3.15): after p = a.multicolour(seed) both triangles have at most
p.ncolours levels, so p.ilu0(sweeps=p.ncolours - 1) IS p.ilu0(), trsv_sweep(b, p.ncolours - 1) IS the exact solve, and a
Krylov solve that applies the swept factor by p.ncolours - 1 sweeps is bit for bit the solve with the exact factor and
the two exact triangular solves.

The Krylov reference runs with the device's own spmv as its product and a preconditioner computed on the host alone
(trsv_ref.solve_by_levels on ilu_ref.ilu0_rows), as tests/test_gpu_solver_fuzz.py does."""
import os
import time

import numpy as np
import pytest

import spalinalg_amd as sp
from tests import colour_ref as cr
from tests import gmres_ref as gr
from tests import ilu_ref as ir
from tests import krylov_ref as kr
from tests import ordering_cases as oc
from tests import solver_cases as sc
from tests import test_gpu_colour as tc
from tests import trsv_ref as tr

pytestmark = pytest.mark.gpu

same = tr.assert_same_bits
same_matrix = tc.assert_same_matrix


def upload(kind, pattern, values):
    return tc.make(kind, pattern, values)


def assemble(kind, pattern, values, rng):
    """The matrix assembled on the device from its triplets in a shuffled order (no duplicates: the values' bits)."""
    n, rowptr, colind = pattern
    rows = np.repeat(np.arange(n, dtype=np.uint64), np.diff(rowptr.astype(np.int64)))
    order = rng.permutation(colind.size)
    coo = sp.CooMatrix.with_triplets(n, n, rows[order], colind[order], values[order])
    return (sp.CsrMatrix if kind == "csr" else sp.CscMatrix).from_coo(coo)


def the_stream(k):
    if k["stream"] is None:
        return None
    import torch
    return torch.cuda.Stream()


def multicolour(a, cseed, stream):
    """a.multicolour(cseed); on a stream of the caller's through the device handle, which is where the argument is."""
    if stream is None:
        return a.multicolour(cseed)
    return a._adopt_ordered(a.device().multicolour(cseed, stream), 0)


def permute(a, perm, stream):
    if stream is None:
        return a.permute(perm)
    return a._adopt_ordered(a.device().permute(perm, stream), 0)


def check_colour(dev, pattern, cseed, stream, ref=None):
    ref = cr.greedy(pattern, cseed) if ref is None else ref
    colours, nc, rounds = dev.colour(cseed, stream)
    assert (nc, rounds) == ref[1:], (cseed, nc, rounds, ref[1:])
    assert np.array_equal(colours, ref[0])
    again = dev.colour(cseed % 2**32, stream)                   # the seed is read mod 2^32
    assert again[1:] == ref[1:] and np.array_equal(again[0], ref[0])
    return ref


def check_permute(a, kind, pattern, values, perm, stream):
    p = permute(a, perm, stream)
    want_pattern, want_values = cr.permute(pattern, values, perm)
    same_matrix(p, kind, want_pattern, want_values)
    assert type(p) is type(a) and p.ncolours == 0 and np.array_equal(p.perm, perm)
    info = p.device().describe()["ordering"]
    assert (info["colours"], info["rounds"], info["seed"]) == (0, 0, 0)
    return p


def krylov(m, f, b, x0, k, sweeps):
    if k["method"] == "gmres":
        return m.gmres(b, M=f, x0=x0, restart=oc.GMRES_RESTART, tol=k["tol"], maxit=k["maxit"], precond_sweeps=sweeps)
    return m.solve(b, k["method"], M=f, x0=x0, tol=k["tol"], maxit=k["maxit"], precond_sweeps=sweeps)


@pytest.mark.parametrize("seed", range(int(os.environ.get("SPAL_FUZZ_SEEDS", "24"))))   # (more seeds: a longer soak)
def test_ordering_chain_is_its_sequential_text(seed):
    t_start = time.perf_counter()
    pattern, values, b, x0, k = oc.case(seed)
    n, kind, cseed, cseed2 = pattern[0], k["kind"], k["cseed"], k["cseed2"]
    rng = np.random.default_rng(seed)
    stream = the_stream(k)
    ref = oc.reference(seed)

    # ---- the operand: uploaded, assembled on the device, or itself a result of the device (coloured as its first call) ----
    a = assemble(kind, pattern, values, rng) if k["origin"] == "assembled" else upload(kind, pattern, values)
    if k["operand"] == "spadd":
        a = a + a                                               # the same structure, every value doubled exactly
        values = values + values
    elif k["operand"] == "spgemm":
        a = a @ a
        pattern, values = oc.csr_view(kind, n, *tc.arrays(a))
        assert sc.first_row_without_diagonal(pattern) is None
        ref = cr.greedy(pattern, cseed)
    same_matrix(a, kind, pattern, values)
    dev = a.device()
    before = [x.copy() for x in dev.download()]

    # ---- colour, multicolour and permute; the dealt one is the handle's first call ----
    steps = {"colour": lambda: check_colour(dev, pattern, cseed, stream, ref),
             "multicolour": lambda: multicolour(a, cseed, stream),
             "permute": lambda: check_permute(a, kind, pattern, values, k["perm"], stream)}
    first = steps[k["first_call"]]()
    if k["first_call"] != "colour":
        check_colour(dev, pattern, cseed, stream, ref)
    m = first if k["first_call"] == "multicolour" else multicolour(a, cseed, stream)
    perm = cr.perm_from_colours(ref[0])
    ppattern, pvalues = cr.permute(pattern, values, perm)
    assert type(m) is type(a) and m.ncolours == ref[1] and np.array_equal(m.perm, perm)
    same_matrix(m, kind, ppattern, pvalues)
    mdev = m.device()
    got_perm, got_nc = mdev.ordering()
    assert got_nc == ref[1] and np.array_equal(got_perm, perm)
    info = mdev.describe()["ordering"]
    assert (info["colours"], info["rounds"], info["seed"]) == (ref[1], ref[2], cseed)     # the seed as it was given
    if k["first_call"] != "permute":
        check_permute(a, kind, pattern, values, k["perm"], stream)
    if k["special"]:                                            # NaN payloads, both zeros, infinities, subnormals
        special = tc._special_values(pattern, k["dtype"].type)
        check_permute(upload(kind, pattern, special), kind, pattern, special, k["perm"], stream)
    assert "ordering" not in dev.describe()                     # the operand is left as it was
    after = dev.download()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    assert np.array_equal(tc.bits(after[2]), tc.bits(before[2]))

    # ---- vectors ----
    import torch
    v = tc._special_values((n, None, np.empty(n)), k["dtype"].type)
    pi = perm.astype(np.int64)
    inverse = np.empty_like(v)
    inverse[pi] = v
    assert np.array_equal(tc.bits(mdev.permute_vec(v)), tc.bits(v[pi]))
    assert np.array_equal(tc.bits(mdev.permute_vec(v, back=True)), tc.bits(inverse))
    x_t = torch.tensor(v).cuda()
    y_t, z_t = torch.zeros_like(x_t), torch.zeros_like(x_t)
    torch.cuda.synchronize()
    mdev.permute_vec_dev(x_t.data_ptr(), y_t.data_ptr(), back=False, stream=stream)
    mdev.permute_vec_dev(x_t.data_ptr(), z_t.data_ptr(), back=True, stream=stream)
    (stream.synchronize if stream is not None else torch.cuda.synchronize)()
    assert np.array_equal(tc.bits(y_t.cpu().numpy()), tc.bits(v[pi]))
    assert np.array_equal(tc.bits(z_t.cpu().numpy()), tc.bits(inverse))

    # ---- the result as a full handle ----
    # An adopted handle builds its tiled second copy with its first product and an uploaded one at creation; the plan
    # is the same one, so the product's bits are (unlike a sum's in tests/test_gpu_spadd.py, no rounding is allowed for).
    fresh = upload(kind, ppattern, pvalues)
    xs = rng.uniform(-1, 1, size=n).astype(k["dtype"])
    y = mdev.spmv(xs)
    same(y, fresh.device().spmv(xs))
    assert mdev.describe().get("kernel") == fresh.device().describe().get("kernel")
    m2 = multicolour(m, cseed2, stream)
    ref2 = cr.greedy(ppattern, cseed2)
    perm2 = cr.perm_from_colours(ref2[0])
    same_matrix(m2, kind, *cr.permute(ppattern, pvalues, perm2))
    got_perm, got_nc = m2.device().ordering()                   # of the last call only, not composed with the first
    assert got_nc == ref2[1] == m2.ncolours and np.array_equal(got_perm, perm2)
    info = m2.device().describe()["ordering"]
    assert (info["colours"], info["rounds"], info["seed"]) == (ref2[1], ref2[2], cseed2)
    del m2

    levels = outcome = None
    nc = ref[1]
    sweeps = max(nc - 1, 0)
    if not k["dropped"]:
        # ---- ILU(0): by ncolours - 1 row sweeps first (it must not analyse the operand), then exactly ----
        fv = ir.ilu0_rows(*ppattern, pvalues)
        fs = m.ilu0(sweeps=sweeps)
        assert "trsv" not in mdev.describe()
        f = m.ilu0()
        same_matrix(f, kind, ppattern, fv)
        same_matrix(fs, kind, ppattern, fv)
        fdev = f.device()
        fdev.trsv_analyse(lower=True)
        plans = fdev.trsv_analyse(lower=False)
        levels = {lower: tr.levels(*ppattern, lower=lower)[1] for lower in (True, False)}
        assert (plans["lower"]["levels"], plans["upper"]["levels"]) == (levels[True], levels[False])
        assert levels[True] <= nc and levels[False] <= nc
        bp = m.to_order(b)
        for lower, unit in ((True, True), (False, False)):
            exact = tr.solve_by_levels(*ppattern, fv, bp, lower, unit)
            same(f.solve_triangular(bp, lower, unit), exact)
            same(fdev.trsv_sweep(bp, sweeps, lower, unit), exact)
            same(fs.device().trsv_sweep(bp, sweeps, lower, unit), exact)

        # ---- the solve on the permuted system: (i) the exact factor by exact solves against the reference loop, ----
        # ---- (ii) the swept factor by ncolours - 1 sweeps, bit for bit (i)                                      ----
        x0p = m.to_order(x0)
        x, info = krylov(m, f, bp, x0p, k, None)
        prec = lambda w: tr.solve_by_levels(*ppattern, fv, tr.solve_by_levels(*ppattern, fv, w, True, True), False, False)  # noqa: E731
        mul = lambda w: mdev.spmv(w)                                                                                        # noqa: E731
        if k["method"] == "gmres":
            xr, want = gr.gmres(mul, prec, bp, x0p, oc.GMRES_RESTART, k["tol"], k["maxit"])
        else:
            xr, want = kr.METHODS[k["method"]](mul, prec, bp, x0p, k["tol"], k["maxit"])
        same(x, xr)
        assert (info.iterations, info.reason) == (want["iterations"], want["reason"])
        same(np.array([info.residual_sq]), np.array([want["residual_sq"]]))
        assert info.rhs_sq == want["rhs_sq"]
        x2, info2 = krylov(m, fs, bp, x0p, k, sweeps)
        same(x2, x)
        assert (info2.iterations, info2.reason) == (info.iterations, info.reason)
        same(np.array([info2.residual_sq]), np.array([info.residual_sq]))
        d = mdev.describe()["gmres" if k["method"] == "gmres" else "krylov"]
        assert d["preconditioned"] == 1 and d["precond_sweeps"] == sweeps
        inv = np.argsort(pi)
        same(m.from_order(x), x[inv])
        outcome = (info.reason, info.iterations)
    else:
        # ---- a missing diagonal: refused by the name of the first such row IN THE NEW NUMBERING; the handle goes on ----
        inv = np.empty(n, dtype=np.int64)
        inv[pi] = np.arange(n)
        first_missing = int(inv[list(k["dropped"])].min())
        assert first_missing == sc.first_row_without_diagonal(ppattern)
        with pytest.raises(sp.Panic, match=rf"spal_{kind}_ilu0: row {first_missing} stores no diagonal entry"):
            m.ilu0()
        with pytest.raises(sp.Panic, match=rf"spal_{kind}_ilu0_sweep: row {first_missing} stores no diagonal entry"):
            m.ilu0(sweeps=1)
        check_colour(mdev, ppattern, cseed2, stream)
        check_permute(m, kind, ppattern, pvalues, k["perm"], stream)

    print(f"ordering fuzz seed {seed}: n {n} nnz {pattern[2].size} {kind} {k['dtype'].name} {k['origin']} {k['operand']} "
          f"first {k['first_call']} stream {k['stream']} colours {ref[1]} rounds {ref[2]} levels "
          f"{None if levels is None else (levels[True], levels[False])} {k['method']} maxit {k['maxit']} "
          f"(reason, iterations) {outcome} {time.perf_counter() - t_start:.2f} s")
