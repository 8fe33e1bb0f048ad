"""The three forms of the sliding CSR kernel on one handle -- col16, row records (csr_rowrec.hpp), packed values
(csr_valpack.hpp) -- forced one after the other by run_forms on the inputs of tests/slide_cases.py: every structural
edge under every form and row length, special operands under packed values, the plan's accept / reject bounds as the
device derives them, re-plans into kept allocations, the state the autotune leaves, and a randomised sweep.

The three forms compute the same products in the same order as the CPU oracle: every comparison is bit for bit (NaN
against NaN by place: special_cases.assert_special_parity with exact=True); there is no tolerance in this file except for
the randomised test's matrices of scattered columns, which no sliding form takes."""
import os

import numpy as np
import pytest

import spalinalg_amd as sp
import spal_synth as synth
from tests import slide_cases as cases
from tests import special_cases as sc

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
FORMS = ("col16", "records", "packed")
ALL, TWO = frozenset(FORMS), frozenset(FORMS[:2])
_SWITCHES = {"col16": (0, 0), "records": (1, 0), "packed": (1, 1)}      # "rowrec_on", "valpack_on"
_FORM_KEYS = ("slide", "rowrec", "rowrec_on", "rowrec_bytes_per_row", "valpack", "valpack_on", "valpack_bytes_per_row",
              "valpack_exp", "valpack_bits", "ring_pages")
W = 4096


def form_of(d):
    """the form describe() says a product launches; None where it is not the sliding kernel"""
    if d.get("slide") != 1:
        return None
    return "packed" if d.get("valpack_on") == 1 else "records" if d.get("rowrec_on") == 1 else "col16"


def built_forms(d):
    """the forms the plan holds arrays for"""
    if "rowrec" not in d:
        return set()
    return {"col16"} | ({"records"} if d["rowrec"] == 1 else set()) | ({"packed"} if d.get("valpack") == 1 else set())


def coherent(d, L):
    """valpack_on => rowrec_on => slide, valpack => rowrec, and the sizes that go with the row length"""
    if "rowrec" not in d:                          # no sliding plan: nothing of the forms is reported
        assert d["slide"] == 0 and not [k for k in d if k.startswith(("rowrec", "valpack"))], d
        return
    f64 = d["dtype"] == "f64"
    assert ("valpack" in d) == f64, d
    vp, vp_on = (d["valpack"], d["valpack_on"]) if f64 else (0, 0)
    assert vp_on <= d["rowrec_on"] <= d["slide"] and vp <= d["rowrec"] and vp_on <= vp and d["rowrec_on"] <= d["rowrec"], d
    assert d["rowrec_failed"] == 0 and d["rowrec_bytes_per_row"] == ((20 if L <= 14 else 24) if d["rowrec"] else 0), d
    if f64:
        assert d["valpack_failed"] == 0 and d["valpack_bytes_per_row"] == ({12: 80, 14: 96, 16: 112}[L] if vp else 0), d


def product(dev, x):
    return dev.spmv(x) if isinstance(x, np.ndarray) else dev.spmv_torch(x).cpu().numpy()


def run_forms(dev, x, expect, y_ref=None):
    """Forces every form in `expect` in turn on the handle -- "rowrec_on" / "valpack_on" -- asserts through describe()
    that this very form launches, takes the product, and restores the two switches.  `expect` is the EXACT set of
    forms the handle must hold: a form it names that the plan did not build fails here, and so does a form the plan
    built that it does not name.  The empty set: the sliding kernel must not run at all.  The products agree bit for
    bit with each other and, where y_ref is given, with it (NaN by place).  Returns {form: y}."""
    expect = set(expect)
    assert expect <= set(FORMS)
    d0 = dev.describe()
    if not expect:
        assert form_of(d0) is None, d0
        y = product(dev, x)
        if y_ref is not None:
            sc.assert_special_parity(y, y_ref, True, None, None)
        return {}
    assert d0["slide"] == 1, d0
    assert built_forms(d0) == expect, (sorted(expect), d0)
    f64 = d0["dtype"] == "f64"
    assert f64 or "packed" not in expect
    out = {}
    for form in FORMS:
        if form not in expect:
            continue
        rowrec_on, valpack_on = _SWITCHES[form]
        dev.set_option("rowrec_on", rowrec_on)
        if f64:
            dev.set_option("valpack_on", valpack_on)
        d = dev.describe()
        assert d["slide"] == 1 and d["rowrec_on"] == rowrec_on and d["rowrec_failed"] == 0, (form, d)
        if f64:
            assert d["valpack_on"] == valpack_on and d["valpack_failed"] == 0, (form, d)
        assert form_of(d) == form and built_forms(d) == expect, (form, d)
        out[form] = product(dev, x)
    # back to where the switches stood (a switch describe() cannot show, its form not being built, goes back to its default)
    dev.set_option("rowrec_on", d0["rowrec_on"] if d0["rowrec"] else 1)
    if f64:
        dev.set_option("valpack_on", d0["valpack_on"] if d0["valpack"] and d0["rowrec_on"] else 1)
    d1 = dev.describe()
    assert [d1.get(k) for k in _FORM_KEYS] == [d0.get(k) for k in _FORM_KEYS], (d0, d1)
    first = out[next(f for f in FORMS if f in out)]
    for form, y in out.items():
        assert np.array_equal(sc.bits(y), sc.bits(first)), form
        if y_ref is not None:
            sc.assert_special_parity(y, y_ref, True, None, None)
            if not np.isnan(y_ref).any():
                assert np.array_equal(sc.bits(y), sc.bits(y_ref)), form
    return out


def forms_of(dtype, packable=True):
    return ALL if np.dtype(dtype) == np.float64 and packable else TWO


def draws(rng, size, dtype):
    """rng.uniform(-1, 1): m * 2^-52 in f64 (they pack: slide_cases.packs gives (True, -52, 53)), rounded for f32"""
    return rng.uniform(-1, 1, size).astype(dtype)


def handle(n, nc, rp, ci, va, L):
    """the device handle; rows of 128 bytes get skewed strips and no sliding plan by default: "skew" 0"""
    dev = sp.CsrMatrix(n, nc, rp, ci, va).device()
    if L * va.dtype.itemsize == 128:
        d = dev.describe()
        assert d["skew"] == 1 and d["slide"] == 0 and "rowrec" not in d, d
        dev.set_option("skew", 0)
    return dev


def under_options(dev, x, expect, y_ref):
    """the forms under runs of 3 and 5 steps dealt round-robin, a grid of 64 workgroups, and non-temporal stores"""
    for key, value, back in (("slide_run", 3, 0), ("slide_run", 5, 0), ("persistent_blocks", 64, 0), ("nt_store", 1, 0)):
        dev.set_option(key, value)
        run_forms(dev, x, expect, y_ref)
        dev.set_option(key, back)


# ---- structure x form x L ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", cases.LENGTHS)
def test_hand_built_rows(oracle, L, dtype):
    """n = 40 037 (last tile and last step partial), rows that wrap the ring, rows inside one page, and the widest row a
    record holds -- and one column wider, which leaves the matrix on col16 alone"""
    rng = np.random.default_rng(14)
    n = 40_000 + 37
    top = cases.max_span(L)
    for span, on in ((top, 1), (top + 1, 0)):
        rp, ci = cases.hand_built(n, 20_000, span, L)
        va, x = draws(rng, ci.size, dtype), draws(rng, n, dtype)
        y_ref = oracle.csr_spmv(rp, ci, va, x)
        dev = handle(n, n, rp, ci, va, L)
        dev.set_option("window_pages", 40)      # (the step of the widest row needs up to 32 pages)
        d = dev.describe()
        coherent(d, L)
        assert d["slide"] == 1 and d["rowrec_failed"] == 0, d
        # (the ring is wider than the record's reach: the bits decide)
        assert d["rowrec_max_span"] == top == cases.max_span(L, d["ring_pages"]), d
        assert d["rowrec"] == on and d["rowrec_on"] == on, d
        if on:
            R = d["ring_pages"] * 256
            wraps = cases.wrapping_rows(ci, L, R)
            assert np.any(wraps % cases.SPREAD_EVERY == 0), d       # a row of 600 columns whose positions wrap the ring
            run_forms(dev, x, forms_of(dtype), y_ref)
            under_options(dev, x, forms_of(dtype), y_ref)
        else:
            assert np.array_equal(dev.spmv(x), y_ref)
            run_forms(dev, x, {"col16"}, y_ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", cases.LENGTHS)
def test_block_jumps(oracle, L, dtype):
    """column ranges that jump forwards and backwards between steps: entering pages on both sides, disjoint windows,
    synchronous page loads; ncols odd and reached (x ends inside a 16-byte vector)"""
    rng = np.random.default_rng(5)
    n, nc = 40_000, 50_001
    rp, ci = cases.block_jumps(rng, n, nc, L)
    va, x = draws(rng, ci.size, dtype), draws(rng, nc, dtype)
    y_ref = oracle.csr_spmv(rp, ci, va, x)
    dev = handle(n, nc, rp, ci, va, L)
    coherent(dev.describe(), L)
    run_forms(dev, x, forms_of(dtype), y_ref)
    under_options(dev, x, forms_of(dtype), y_ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", cases.LENGTHS)
def test_non_square(oracle, L, dtype):
    """10 037 x 6000: below row 1904 every row draws from the same window, the matrix's last 4096 columns"""
    rng = np.random.default_rng(6)
    n, nc = 10_000 + 37, 6000
    rp, ci = cases.band(rng, n, nc, L, W)
    va, x = draws(rng, ci.size, dtype), draws(rng, nc, dtype)
    dev = handle(n, nc, rp, ci, va, L)
    coherent(dev.describe(), L)
    run_forms(dev, x, forms_of(dtype), oracle.csr_spmv(rp, ci, va, x))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", cases.LENGTHS)
@pytest.mark.parametrize("n", [64, 65, 257])
def test_small_matrices(oracle, n, L, dtype):
    """one tile (slide_cases.MIN_ROWS: the fewest rows with records); one row in the last tile; one row in the last step"""
    rng = np.random.default_rng(7)
    nc = 6000
    rp, ci = cases.band(rng, n, nc, L, W)
    va, x = draws(rng, ci.size, dtype), draws(rng, nc, dtype)
    dev = handle(n, nc, rp, ci, va, L)
    d = dev.describe()
    assert d["rowrec"] == 1 and d["slide"] == 0 and d["rowrec_on"] == 0, d   # (so few tiles are mostly re-reads: not by default)
    dev.set_option("slide_on", 1)                                             # ... but by name
    coherent(dev.describe(), L)
    run_forms(dev, x, forms_of(dtype), oracle.csr_spmv(rp, ci, va, x))


# ---- special operands ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", cases.LENGTHS)
def test_special_x_under_every_form(oracle, L):
    """Packed values hold no NaN, Inf or -0.0, but x does: rows of stored +0.0 over negative x give -0.0 (the first
    product is assigned, not added to +0.0), +0.0 * Inf gives NaN, and the pad rows past the last row leak nothing."""
    s = cases.special_layout(L)
    n, rp, ci, va, x = s["n"], s["rowptr"], s["colind"], s["values"], s["x"]
    y_ref = oracle.csr_spmv(rp, ci, va, x)
    dev = handle(n, n, rp, ci, va, L)
    d = dev.describe()
    assert d["valpack"] == 1 and (d["valpack_exp"], d["valpack_bits"]) == cases.packs(va, L)[1:] == (0, 11), d
    out = run_forms(dev, x, ALL, y_ref)
    assert set(out) == ALL
    neg = s["neg_zero_rows"]
    last_tile = (n // 64) * 64
    assert n - 1 in neg and {64, 320, last_tile} <= set(neg.tolist())     # the last row; rows after a tile's end
    for form, y in out.items():
        sc.assert_special_parity(y, y_ref, True, None, None)
        assert np.all(y[neg] == 0) and np.all(np.signbit(y[neg])), (form, neg[~np.signbit(y[neg])][:8])
        assert np.signbit(y[n - 1]) and y[n - 1] == 0, form
        for r in (64, 320, last_tile):
            assert np.signbit(y[r]) and y[r] == 0, (form, r)
        assert np.isnan(y[s["zero_rows"]]).any() and np.isinf(y).any(), form


# ---- the plan's bounds, as the device derives them --------------------------------------------------------------------------
@pytest.mark.parametrize("L", cases.LENGTHS)
@pytest.mark.parametrize("name", sorted(cases.VALUE_CLASSES))
def test_plan_bounds_on_the_device(oracle, name, L):
    """valpack_scan / valpack_plan derive e and bits themselves: on every value class they decide as the rule restated in
    slide_cases.packs does, one step to each side of e = -1022, e = 970 and k = -+2^(W-1).  x in +-[0.5, 1): under
    "quantum_min" and "quantum_max" (|k| >= 2^20) every product is normal and every sum finite; under
    "quantum_min_units" (k = +-1 at e = -1022, x / 32) every product and every sum is subnormal, and held to the oracle's bits like
    everything else."""
    rng = np.random.default_rng(100 + L)
    n = 1000 + 37
    rp, ci = cases.band(rng, n, n, L, 1024)
    va, stated = cases.VALUE_CLASSES[name](rng, ci.size, L)
    assert cases.packs(va, L) == stated
    x = cases.half_to_one(rng, n)
    if name == "quantum_min_units":
        x /= 32                                  # (products below 2^-1027: a sum of 16 stays below the smallest normal)
    y_ref = oracle.csr_spmv(rp, ci, va, x)
    if name == "quantum_min_units":
        assert np.all((y_ref != 0) & (np.abs(y_ref) < np.finfo(np.float64).tiny))
    elif stated[0]:
        assert np.all(np.isfinite(y_ref))
    dev = handle(n, n, rp, ci, va, L)
    dev.set_option("slide_on", 1)
    d = dev.describe()
    coherent(d, L)
    assert d["rowrec"] == 1 and d["valpack"] == int(stated[0]) and d["valpack_failed"] == 0, d
    if stated[0]:
        assert (d["valpack_exp"], d["valpack_bits"]) == stated[1:], d
    else:
        assert d["valpack_on"] == 0 and d["valpack_bytes_per_row"] == 0, d
    run_forms(dev, x, ALL if stated[0] else TWO, y_ref)


# ---- x off a 16-byte boundary -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [12, 14])
def test_unaligned_x_falls_back(oracle, L):
    """x off a 16-byte boundary: the one-super-tile kernels run on col16 and the plain values, which stay resident beside
    the records and the row blocks; the handle's forms are what they were afterwards"""
    import torch
    n = 40_000 + 37
    rp, ci, va = synth.banded_csr(n, n, L, W, 100 + L)
    x = synth.vector(n)
    y_ref = oracle.csr_spmv(rp, ci, va, x)
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    d0 = dev.describe()
    assert form_of(d0) == "packed" and built_forms(d0) == ALL, d0
    big = torch.zeros(n + 8, dtype=torch.float64, device="cuda")
    xs = big[1:n + 1]
    xs.copy_(torch.from_numpy(x))
    assert xs.data_ptr() % 16 == 8
    assert np.array_equal(sc.bits(dev.spmv_torch(xs).cpu().numpy()), sc.bits(y_ref))
    d1 = dev.describe()
    assert [d1.get(k) for k in _FORM_KEYS] == [d0.get(k) for k in _FORM_KEYS], (d0, d1)
    xa = big[2:n + 2]
    xa.copy_(torch.from_numpy(x))
    assert xa.data_ptr() % 16 == 0
    run_forms(dev, xa, ALL, y_ref)
    xs.copy_(torch.from_numpy(x))                # (xa lay over it) ... and off the boundary again
    assert np.array_equal(sc.bits(dev.spmv_torch(xs).cpu().numpy()), sc.bits(y_ref))


# ---- re-plans ---------------------------------------------------------------------------------------------------------------
def _implied(state, f64=True):
    """(forms built, forms a product can launch) under the options of `state`"""
    if state["tiles_per_wave"] != 4 or state["skew"]:
        return None, set()                       # no sliding plan
    built = {"col16"}
    if state["rowrec"] and state["rows_per_tile"] in (0, 64):
        built.add("records")
        if state["valpack"] and f64:
            built.add("packed")
    return built, (built if state["slide_on"] else set())


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("L", cases.LENGTHS)
def test_replans_keep_every_form(oracle, L, seed):
    """Every option that re-plans, in a shuffled order: a re-plan that changes the ring ("window_pages") re-encodes every
    record into the allocation it kept, "valpack" / "rowrec" 0 free and 1 rebuild, tiles of 32 rows and 8 tiles per
    wave have no records, "slide_on" 0 keeps the arrays and launches none of the forms.  After each one describe() is
    coherent, reports exactly the forms the options imply, and every one of them returns the oracle's bits."""
    rng = np.random.default_rng(50 + seed)
    n = 10_000 + 37
    rp, ci, va = synth.banded_csr(n, n, L, W, 60 + L)
    x = synth.vector(n)
    y_ref = oracle.csr_spmv(rp, ci, va, x)
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    state = {"valpack": 1, "rowrec": 1, "window_pages": 0, "rows_per_tile": 0, "tiles_per_wave": 4, "slide_on": 1,
             "skew": 1 if L == 16 else 0}
    steps = [("valpack", 0), ("valpack", 1), ("rowrec", 0), ("rowrec", 1), ("window_pages", 0), ("window_pages", 24),
             ("window_pages", 40), ("rows_per_tile", 32), ("tiles_per_wave", 8), ("slide_on", 0), ("slide_on", 1)]
    if L == 16:
        steps += [("skew", 1), ("skew", 0), ("skew", 0)]
    steps = [steps[i] for i in rng.permutation(len(steps))]
    # ... and at the end everything on again
    steps += [("skew", 0), ("slide_on", 1), ("rowrec", 1), ("valpack", 1), ("window_pages", 40), ("window_pages", 24)]
    back = {"rows_per_tile": 0, "tiles_per_wave": 4}      # "32 -> 0", "8 -> 4": set, checked, and set back, checked

    def check():
        d = dev.describe()
        coherent(d, L)
        built, reach = _implied(state)
        assert (built_forms(d) or None) == built, (state, d)
        assert form_of(d) == (None if not reach else "packed" if "packed" in reach else "records" if "records" in reach else "col16"), (state, d)
        run_forms(dev, x, reach, y_ref)
        return d

    check()
    for key, value in steps:
        for v in (value, back[key]) if key in back else (value,):
            dev.set_option(key, v)
            state[key] = v
            check()
    assert _implied(state) == (set(ALL), set(ALL))


# ---- after the autotune -----------------------------------------------------------------------------------------------------
def test_forms_after_the_autotune(oracle):
    """Stages 1b and 1c of the autotune flip "rowrec_on" and "valpack_on" while they time and leave what won.  Whatever
    that is: describe() is coherent, both stages have timed where the sliding kernel was kept, the default product is
    the oracle's, and all three forms still are -- also after a re-plan onto another ring.  Nothing is asserted about
    which form won.  (The placement stage moves the records only where they take 64 MiB: that stays with the full-size
    runs of the benchmark.)"""
    import torch
    n, L = 40_000 + 37, 14
    rp, ci, va = synth.banded_csr(n, n, L, W, 9)
    x = synth.vector(n)
    y_ref = oracle.csr_spmv(rp, ci, va, x)
    dev = sp.CsrMatrix(n, n, rp, ci, va).device()
    assert built_forms(dev.describe()) == ALL
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty_like(xd)
    d = dev.autotune(xd, yd, iters=3)
    coherent(d, L)
    assert built_forms(d) == ALL and all(t > 0 for t in d["autotune_us"]), d
    if d["slide"] == 1:
        assert all(t > 0 for t in d["rowrec_us"]) and all(t > 0 for t in d["valpack_us"]), d
    assert d["placement_tries"] == 0, d
    assert np.array_equal(sc.bits(dev.spmv_torch(xd).cpu().numpy()), sc.bits(y_ref))
    assert np.array_equal(sc.bits(dev.spmv(x)), sc.bits(y_ref))
    dev.set_option("slide_on", 1)                # (by name, should the one-super-tile form have won)
    run_forms(dev, x, ALL, y_ref)
    dev.set_option("window_pages", 40)
    coherent(dev.describe(), L)
    run_forms(dev, x, ALL, y_ref)
    run_forms(dev, xd, ALL, y_ref)


# ---- randomised ---------------------------------------------------------------------------------------------------------------
def check_fuzz_case(oracle, c):
    L, dtype, x = c["L"], c["dtype"], c["x"]
    n, nc, rp, ci, va = c["n"], c["ncols"], c["rowptr"], c["colind"], c["values"]
    y_ref = oracle.csr_spmv(rp, ci, va, x)
    dev = sp.CsrMatrix(n, nc, rp, ci, va).device()
    what = {k: c[k] for k in ("seed", "L", "n", "ncols", "pattern", "width", "value_class", "special_x")}
    if c["pattern"] in cases.SLIDING:
        if L * dtype.itemsize == 128:
            dev.set_option("skew", 0)
        if c["window_pages"]:
            dev.set_option("window_pages", c["window_pages"])
        dev.set_option("slide_on", 1)
        d = dev.describe()
        coherent(d, L)
        assert d["slide"] == 1 and d["rowrec"] == 1 and d["rowrec_on"] == 1, (what, d)
        packable = c["expected"][0]
        if dtype == np.float64:
            assert d["valpack"] == int(packable), (what, d)
            if packable:
                assert (d["valpack_exp"], d["valpack_bits"]) == c["expected"][1:], (what, d)
        run_forms(dev, x, forms_of(dtype, packable), y_ref)
    else:
        d = dev.describe()
        coherent(d, L)
        assert "rowrec" not in d and "valpack" not in d and d["slide"] == 0, (what, d)
        exact = d["kernel"] in ("stream", "cblock")
        bound = None if exact else sc.spmv_bound(rp, ci, va, x, oracle)
        sc.assert_special_parity(dev.spmv(x), y_ref, exact, bound, sc.TOL[dtype])


@pytest.mark.parametrize("seed", range(int(os.environ.get("SPAL_FUZZ_SEEDS", "24"))))   # (more seeds: a longer soak)
def test_random_uniform_rows_every_form(oracle, seed):
    """slide_cases.fuzz_case: L, n, ncols, a column pattern (band, clusters, block jumps, anywhere), a value class and
    ordinary or special x.  The three sliding patterns MUST have records, packed values exactly where the rule says,
    and every form the oracle's bits; columns anywhere must have no sliding plan at all."""
    check_fuzz_case(oracle, cases.fuzz_case(seed))
