"""CPU tests that keep tests/test_gpu_ordering_fuzz.py honest: every default seed of tests/ordering_cases.py is a valid
input, and the default seeds between them reach what the device test is there for -- more than 64 and more than 128
colours with holes in the 64-colour windows, round counts in several batches of rounds, empty rows at the front, at
the back and in the middle, missing diagonals, every knob's values -- and the composite invariant is not trivially
true: the levels of a multicolour-ordered pattern reach ncolours, and one sweep fewer than levels - 1 does not give the
exact factor."""
import numpy as np
import pytest

from tests import colour_ref as cr
from tests import ilu_ref as ir
from tests import ilu_sweep_ref as isr
from tests import ordering_cases as oc
from tests import solver_cases as sc
from tests import trsv_ref as tr

SEEDS = range(oc.DEFAULT_SEEDS)
_FACTS = {}


def facts(seed):
    """What one seed brings: its colouring at its own seed and the levels of the permuted pattern (once per process)."""
    if seed not in _FACTS:
        pattern, values, _, _, k = oc.case(seed)
        colours, ncolours, rounds = oc.reference(seed)
        permuted, pvalues = cr.permute(pattern, values, cr.perm_from_colours(colours))
        levels = None
        if not k["dropped"]:
            levels = {lower: tr.levels(*permuted, lower=lower)[1] for lower in (True, False)}
        _FACTS[seed] = dict(ncolours=ncolours, rounds=rounds, holes=oc.holes(pattern, colours, k["cseed"]),
                            levels=levels, permuted=permuted, pvalues=pvalues)
    return _FACTS[seed]


# ---- every seed is a valid input ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_seed_is_valid(seed):
    pattern, values, b, x0, k = oc.case(seed)
    base, _, _, _, k0 = sc.case(seed)
    n, rowptr, colind = pattern
    assert n == base[0] == k["n"] and n <= 8000 and rowptr.dtype == colind.dtype == np.uint64 and rowptr.shape == (n + 1,)
    rp = rowptr.astype(np.int64)
    assert rp[0] == 0 and rp[-1] == colind.size and np.all(np.diff(rp) >= 0)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = colind.astype(np.int64)
    assert cols.size == 0 or (cols.min() >= 0 and cols.max() < n)
    same_row = rows[1:] == rows[:-1]
    assert np.all(cols[1:][same_row] > cols[:-1][same_row]), "columns must ascend strictly inside a row"
    assert values.dtype == b.dtype == x0.dtype == k["dtype"] == k0["dtype"] and k["kind"] == k0["kind"]
    assert values.shape == colind.shape and b.shape == x0.shape == (n,)
    assert np.isfinite(values).all() and np.isfinite(b).all() and np.isfinite(x0).all()
    # the diagonal: missing where solver_cases dropped it and in the empty runs, nowhere else
    stored = np.zeros(n, dtype=bool)
    stored[rows[rows == cols]] = True
    cleared = np.zeros(n, dtype=bool)
    for place, a, e in k["empty_runs"]:
        assert 0 <= a < e <= n and place in ("front", "middle", "back")
        assert (a == 0) == (place == "front") or n <= 2
        assert (e == n) == (place == "back") or n <= 2
        cleared[a:e] = True
    assert [p for p, _, _ in k["empty_runs"]] == list(oc.EMPTY.get(seed % 24, ()))
    expected_missing = cleared.copy()
    expected_missing[list(k0["dropped"])] = True
    assert tuple(np.flatnonzero(~stored).tolist()) == k["dropped"] == tuple(np.flatnonzero(expected_missing).tolist())
    # an empty run is empty: no entry in its rows or in its columns
    assert not cleared[rows].any() and not cleared[cols].any()
    # the block: m members, each edge of the block stored in one direction only (unless the base matrix had the other)
    if k["block"]:
        m, density, members = k["block"]
        assert m in oc.BLOCK_M and density in oc.BLOCK_DENSITY and members.size == m <= 400 and np.all(np.diff(members) > 0)
        inside = np.zeros(n, dtype=bool)
        inside[members] = True
        be = inside[rows] & inside[cols] & (rows != cols) & ~cleared[rows]
        pairs = np.unique(np.minimum(rows[be], cols[be]) * n + np.maximum(rows[be], cols[be])).size
        live = int((~cleared[members]).sum())
        assert pairs >= 0.8 * density * live * (live - 1) / 2
        assert int(be.sum()) < 1.2 * pairs, "most edges of the block must be stored in one direction only"
        up = int((cols[be] > rows[be]).sum())
        assert 0.35 * be.sum() < up < 0.65 * be.sum(), "... in either direction about as often"
    else:
        assert seed % 2 == 0 or n < oc.BLOCK_MIN_N
    # strictly dominant rows where the diagonal is stored: ILU(0) and the solves stay finite
    off = np.bincount(rows[rows != cols], weights=np.abs(values[rows != cols]).astype(np.float64), minlength=n)
    diag = np.zeros(n)
    diag[rows[rows == cols]] = values[rows == cols]
    assert np.all(diag[stored] > off[stored])
    if k["symmetric"]:
        t = tr.from_coo(n, cols, rows)
        assert np.array_equal(t[1], rowptr) and np.array_equal(t[2], colind), "a CG seed must be structurally symmetric"
        dense_key = dict(zip(zip(rows.tolist(), cols.tolist()), values.tolist()))
        probe = list(dense_key.items())[:: max(1, len(dense_key) // 500)]
        assert all(dense_key[(j, i)] == v for (i, j), v in probe), "a CG seed must be symmetric"
    # the knobs
    assert k["method"] in oc.METHODS and (k["method"] != "cg" or k["symmetric"]) and k["maxit"] in oc.MAXIT
    assert k["stream"] in oc.STREAMS and k["origin"] in oc.ORIGINS and k["first_call"] in oc.FIRST_CALLS
    assert k["operand"] in ("plain", "spadd", "spgemm") and (k["operand"] != "spgemm" or n <= 257)
    assert k["operand"] == "plain" or not k["dropped"]
    assert k["origin"] == "uploaded" or colind.size > 0         # (a COO matrix without triplets assembles nothing)
    for s in (k["cseed"], k["cseed2"]):
        assert 0 <= s < 2**64 and (s in oc.CSEEDS or s >= 2**32)
    perm = k["perm"]
    assert perm.dtype == np.uint64 and np.array_equal(np.sort(perm), np.arange(n, dtype=np.uint64))
    assert k["perm_kind"] in oc.PERM_KINDS
    if k["perm_kind"] == "identity":
        assert np.array_equal(perm, np.arange(n, dtype=np.uint64))
    if k["perm_kind"] == "rotation" and k["empty_runs"]:
        # the rotation moves the first run off its end of the matrix, into the middle
        _, a, e = k["empty_runs"][0]
        inv = np.empty(n, dtype=np.int64)
        inv[perm.astype(np.int64)] = np.arange(n)
        assert inv[a] > 0 and inv[e - 1] < n - 1 and np.array_equal(inv[a:e], np.arange(inv[a], inv[a] + e - a))
    # the references are finite where the device test runs them
    f = facts(seed)
    assert cr.is_proper(pattern, oc.reference(seed)[0])
    if not k["dropped"]:
        fv = ir.ilu0_rows(*f["permuted"], f["pvalues"])
        assert np.isfinite(fv).all()
        y = tr.solve_by_levels(*f["permuted"], fv, b, True, True)
        assert np.isfinite(tr.solve_by_levels(*f["permuted"], fv, y, False, False)).all()


def test_case_is_deterministic_in_its_seed():
    for seed in (1, 5, 14):
        a = oc.case(seed)
        b = oc.case.__wrapped__(seed)
        assert all(np.array_equal(x, y) for x, y in zip((*a[0][1:], *a[1:4]), (*b[0][1:], *b[1:4])))
        for key, v in a[4].items():
            w = b[4][key]
            if key == "block":
                assert (v is None and w is None) or (v[:2] == w[:2] and np.array_equal(v[2], w[2]))
            elif key == "perm":
                assert np.array_equal(v, w)
            else:
                assert v == w, key


def test_batch_of_is_the_batches_of_the_rounds():
    # batches of 8, 16, 32, 64, ... rounds: the first four end at 8, 24, 56, 120
    assert [oc.batch_of(r) for r in (1, 8, 9, 24, 25, 56, 57, 120, 121, 248, 249)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5]
    assert [r for r in range(1, 130) if oc.batch_of(r) != oc.batch_of(r + 1)] == [8, 24, 56, 120]
    assert oc.CHAIN_ROUNDS == (8, 9, 24, 25, 56, 57, 120, 121)


# ---- what the default seeds cover --------------------------------------------------------------------------------------

def test_the_windows_of_64_colours_are_crossed_with_holes():
    nc = {s: facts(s)["ncolours"] for s in SEEDS}
    assert sum(c > 64 for c in nc.values()) >= 2, nc
    with_holes = [s for s in SEEDS if facts(s)["holes"] > 0]
    assert with_holes, "no seed has a non-prefix mask in a window past the first"
    # more than 128 colours: the third window, on a seed that has holes (a clique would reach it without any)
    assert any(nc[s] > 128 and facts(s)["holes"] > 0 for s in SEEDS), nc
    # a clique has none: the condition does say something
    clique = tr.dense_triangle(130)
    assert oc.holes(clique, cr.greedy(clique, 0)[0], 0) == 0


def test_round_counts_fall_in_several_batches():
    batches = {s: oc.batch_of(facts(s)["rounds"]) for s in SEEDS}
    assert len(set(batches.values())) >= 3, batches
    assert {0, 1, 2} <= set(batches.values()), batches          # <= 8, 9 - 24 and 25 - 56 rounds are all there
    assert max(batches.values()) >= 3, batches                  # ... and beyond


@pytest.mark.parametrize("rounds", oc.CHAIN_ROUNDS)
def test_chain_has_its_rounds_and_two_colours(rounds):
    pattern = oc.chain(rounds)
    assert pattern[0] == rounds
    colours, ncolours, got = cr.greedy(pattern, 0)
    assert (ncolours, got) == (2, rounds)
    assert cr.is_proper(pattern, colours)


def test_empty_runs_and_missing_diagonals_appear():
    places = {p for s in SEEDS for p, _, _ in oc.case(s)[4]["empty_runs"]}
    assert places == {"front", "middle", "back"}
    assert any(oc.case(s)[4]["dropped"] for s in SEEDS)
    # a missing diagonal without an empty row (solver_cases' own), and an empty row in front of stored ones
    assert any(oc.case(s)[4]["dropped"] and len(oc.case(s)[4]["dropped"]) > sum(e - a for _, a, e in oc.case(s)[4]["empty_runs"])
               for s in SEEDS)
    # runs of more than one row, a single empty row, and a matrix without entries
    lengths = {e - a for s in SEEDS for _, a, e in oc.case(s)[4]["empty_runs"]}
    assert 1 in lengths and max(lengths) >= 64
    assert any(oc.case(s)[0][2].size == 0 for s in SEEDS) and any(oc.case(s)[0][0] == 1 for s in SEEDS)
    # a rotation falls on a seed with empty runs
    assert any(oc.case(s)[4]["perm_kind"] == "rotation" and oc.case(s)[4]["empty_runs"] for s in SEEDS)
    # most seeds still run the ILU and solve stages
    assert sum(not oc.case(s)[4]["dropped"] for s in SEEDS) >= 18


def test_every_knob_value_occurs():
    knobs = [oc.case(s)[4] for s in SEEDS]
    solving = [k for k in knobs if not k["dropped"]]
    assert {k["kind"] for k in knobs} == {"csr", "csc"} == {k["kind"] for k in solving}
    assert {k["dtype"] for k in knobs} == {np.dtype(np.float64), np.dtype(np.float32)} == {k["dtype"] for k in solving}
    assert {k["stream"] for k in knobs} == set(oc.STREAMS) == {k["stream"] for k in solving}
    assert {k["origin"] for k in knobs} == set(oc.ORIGINS)
    assert {k["method"] for k in solving} == set(oc.METHODS)
    assert {k["maxit"] for k in solving} == set(oc.MAXIT)
    assert {k["perm_kind"] for k in knobs} == set(oc.PERM_KINDS)
    assert {k["operand"] for k in knobs} == {"plain", "spadd", "spgemm"}
    # every ordering call is the first call on some device-assembled handle
    assert {k["first_call"] for k in knobs if k["origin"] == "assembled" and k["operand"] == "plain"} == set(oc.FIRST_CALLS)
    # the colouring seeds: the table's four values and a drawn one at or above 2^32
    cseeds = {k["cseed"] for k in knobs}
    assert {0, 7, 2**32 - 1, 2**32 + 7} <= cseeds and any(s > 2**32 + 7 for s in cseeds)
    assert any(k["special"] for k in knobs)
    # blocks on about half the seeds, at every size of the table
    blocks = [k["block"] for k in knobs if k["block"]]
    assert 8 <= len(blocks) <= 14 and {b[0] for b in blocks} == set(oc.BLOCK_M)


def test_seed_is_read_mod_2_to_the_32():
    for seed in (1, 8):                                         # a seed with a block, and one without
        pattern = oc.case(seed)[0]
        a, b = cr.greedy(pattern, 2**32 + 7), cr.greedy(pattern, 7)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
        c = cr.greedy(pattern, 8)
        assert not np.array_equal(a[0], c[0])                   # (another seed is another colouring)


# ---- the composite invariant is not trivially true -----------------------------------------------------------------------

def test_levels_of_the_multicolour_order_reach_ncolours():
    exact = []
    for s in SEEDS:
        f = facts(s)
        if f["levels"] is None:
            continue
        assert f["levels"][True] <= f["ncolours"] and f["levels"][False] <= f["ncolours"], (s, f["levels"], f["ncolours"])
        if f["levels"][True] == f["ncolours"]:
            exact.append(s)
    assert exact, "no seed whose lower triangle has exactly ncolours levels"
    # ... and one of them past the first window of colours would be a clique; with a block the bound is not reached
    assert any(facts(s)["levels"] is not None and facts(s)["levels"][True] < facts(s)["ncolours"] for s in SEEDS)


def test_one_sweep_fewer_is_not_the_exact_factor():
    """ncolours - 1 sweeps give the exact factor because levels - 1 do; levels - 2 do not, on a seed without a block
    and with a handful of levels (the sweep reference costs a pass over the matrix per sweep)."""
    candidates = sorted((s for s in SEEDS if facts(s)["levels"] is not None and oc.case(s)[4]["block"] is None
                         and 3 <= facts(s)["levels"][True] <= 8 and oc.case(s)[4]["n"] <= 5000),
                        key=lambda s: facts(s)["levels"][True] * oc.case(s)[0][2].size)
    assert candidates
    s = candidates[0]
    f = facts(s)
    levels = f["levels"][True]
    exact = ir.ilu0_rows(*f["permuted"], f["pvalues"])
    tr.assert_same_bits(isr.ilu0_sweep_rows(*f["permuted"], f["pvalues"], levels - 1), exact)
    fewer = isr.ilu0_sweep_rows(*f["permuted"], f["pvalues"], levels - 2)
    assert not np.array_equal(fewer.view(np.uint8), exact.view(np.uint8)), (s, levels)
