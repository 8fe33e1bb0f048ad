"""CPU tests that keep tests/test_gpu_solver_fuzz.py honest: every default seed of tests/solver_cases.py is a valid,
finite input of the four references, the vector references it is compared with equal the sequential loops on the small
seeds, the two schedule restatements say what the header says on hand cases, and the default seeds between them meet
the schedule conditions the device test is there for."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import ilu_ref as ir
from tests import solver_cases as sc
from tests import sweep_ref as sw
from tests import trsv_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(sc.DEFAULT_SEEDS)
HUGE = 1 << 40


def triangles(knobs):
    """(lower, unit) pairs the matrix allows: a missing diagonal leaves the unit-diagonal ones."""
    return [(lower, unit) for lower in (True, False) for unit in ((True,) if knobs["dropped"] else (False, True))]


# ---- every seed is a valid, finite input -----------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_seed_is_valid_and_finite(seed):
    pattern, values, b, x0, k = sc.case(seed)
    n, rowptr, colind = pattern
    assert n in sc.SIZES and rowptr.dtype == colind.dtype == np.uint64 and rowptr.shape == (n + 1,)
    rp = rowptr.astype(np.int64)
    assert rp[0] == 0 and rp[-1] == colind.size and np.all(np.diff(rp) >= 0)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = colind.astype(np.int64)
    assert cols.size == 0 or (cols.min() >= 0 and cols.max() < n)
    same_row = rows[1:] == rows[:-1]
    assert np.all(cols[1:][same_row] > cols[:-1][same_row]), "columns must ascend strictly inside a row"
    assert values.dtype == b.dtype == x0.dtype == k["dtype"] and values.shape == colind.shape and b.shape == x0.shape == (n,)
    assert np.isfinite(values).all() and np.isfinite(b).all() and np.isfinite(x0).all()
    # the diagonal: stored everywhere, or missing exactly where the knobs say
    stored = np.zeros(n, dtype=bool)
    stored[rows[rows == cols]] = True
    assert tuple(np.flatnonzero(~stored).tolist()) == k["dropped"]
    assert sc.first_row_without_diagonal(pattern) == (k["dropped"][0] if k["dropped"] else None)
    assert bool(k["dropped"]) == (seed % 6 == 5)
    # strictly dominant rows where the diagonal is stored
    off = np.bincount(rows[rows != cols], weights=np.abs(values[rows != cols]).astype(np.float64), minlength=n)
    diag = np.zeros(n)
    diag[rows[rows == cols]] = values[rows == cols]
    assert np.all(diag[stored] > off[stored])
    if k["method"] == "cg":
        t = tr.from_coo(n, cols, rows)
        assert np.array_equal(t[1], rowptr) and np.array_equal(t[2], colind), "a CG seed must be structurally symmetric"
        dense_key = dict(zip(zip(rows.tolist(), cols.tolist()), values.tolist()))
        probe = list(dense_key.items())[:: max(1, len(dense_key) // 500)]
        assert all(dense_key[(j, i)] == v for (i, j), v in probe), "a CG seed must be symmetric"
    # the knobs
    assert k["chain_rows"] in sc.CHAIN_ROWS and k["chain_rows_2"] in sc.CHAIN_ROWS and k["chain_rows"] != k["chain_rows_2"]
    assert k["wide_work"] in sc.WIDE_WORK and k["method"] in sc.METHODS and k["prec"] in sc.PRECS
    assert k["check_every"] in sc.CHECK_EVERY and k["check_every_2"] in sc.CHECK_EVERY and k["check_every"] != k["check_every_2"]
    assert k["maxit"] in sc.MAXIT
    for lower in (True, False):
        nl = tr.levels(*pattern, lower=lower)[1]
        assert k["levels"][lower] == nl
        counts = k["sweeps"][lower]
        assert {0, 1, 2, nl - 1, nl + 3} <= set(counts) and all(s >= 0 for s in counts)
        drawn = set(counts) - {0, 1, 2, nl - 1, nl + 3}
        assert len(drawn) <= 1 and all(3 <= s < nl for s in drawn)
    # the references
    for lower, unit in triangles(k):
        assert np.isfinite(tr.solve_by_levels(*pattern, values, b, lower, unit)).all()
        for s in k["sweeps"][lower]:
            if s < k["levels"][lower] - 1:          # (from there on the device test compares with the exact solve)
                assert np.isfinite(sw.sweep_vec(*pattern, values, b, s, lower, unit)).all()
    if not k["dropped"]:
        assert np.isfinite(ir.ilu0_rows(*pattern, values)).all()


def test_case_is_deterministic_in_its_seed():
    for seed in (0, 5, 13):
        a = sc.case(seed)
        b = sc.case.__wrapped__(seed)
        assert all(np.array_equal(x, y) for x, y in zip((*a[0][1:], *a[1:4]), (*b[0][1:], *b[1:4])))
        assert {key: v for key, v in a[4].items()} == {key: v for key, v in b[4].items()}


# ---- the vector references are the loops -----------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [s for s in SEEDS if sc.case(s)[4]["n"] <= 257])
def test_vector_references_equal_the_loops_on_the_small_seeds(seed):
    pattern, values, b, x0, k = sc.case(seed)
    if not k["dropped"]:
        tr.assert_same_bits(ir.ilu0_rows(*pattern, values), ir.ilu0_loop(*pattern, values))
    for lower, unit in triangles(k):
        exact = tr.solve_loop(*pattern, values, b, lower, unit)
        tr.assert_same_bits(tr.solve_by_levels(*pattern, values, b, lower, unit), exact)
        for s in k["sweeps"][lower]:
            loop = sw.sweep_loop(*pattern, values, b, s, lower, unit)
            tr.assert_same_bits(sw.sweep_vec(*pattern, values, b, s, lower, unit), loop)
            if s >= k["levels"][lower] - 1:         # what lets the device test take the exact solve as reference there
                tr.assert_same_bits(loop, exact)


# ---- the two restatements on hand cases --------------------------------------------------------------------------------

def test_expected_launches_on_the_prescribed_widths():
    w = tr.PRESCRIBED_WIDTHS
    # [1, 1023, 1024] one chain, 1025 a level, [1] a chain, 2049 a level, [3, 1] a chain: five launches, three of them
    # chains (what tests/test_gpu_trsv.py has the device report for this matrix)
    assert sc.expected_launches(w, 1024) == (5, 3)
    assert sc.expected_launches(w, 0) == (len(w), 0)
    assert sc.expected_launches(w, HUGE) == (1, 1)
    assert sc.expected_launches(w, 1) == (8, 3)             # [1] 1023 1024 1025 [1] 2049 3 [1]: no two narrow ones meet
    assert sc.expected_launches(w, 1025) == (3, 2)
    assert sc.expected_launches([], 64) == (0, 0)
    assert sc.expected_launches([65, 65], 64) == (2, 0) and sc.expected_launches([64, 64], 64) == (1, 1)


def test_expected_wide_rows_on_a_hand_matrix():
    # rows: 0 {0,1,3}; 1 {1,2,3}; 2 {0,1,2}; 3 {3}; 4 {0,2,4}
    dense = np.array([[1, 1, 0, 1, 0], [0, 1, 1, 1, 0], [1, 1, 1, 0, 0], [0, 0, 0, 1, 0], [1, 0, 1, 0, 1]])
    pattern, _ = ir.dense_to_csr(dense.astype(np.float64), np.float64)
    work, has_lower = sc.row_work(pattern)
    # entries past the diagonal: row 0 two, row 1 two, others none; row 2 reads rows 0 and 1, row 4 rows 0 and 2
    assert work.tolist() == [0, 0, 4, 0, 2] and has_lower.tolist() == [False, False, True, False, True]
    assert [sc.expected_wide_rows(pattern, t) for t in (0, 1, 2, 3, 4, 5, HUGE)] == [2, 2, 2, 1, 1, 0, 0]
    assert sc.expected_wide_rows(pattern, 0) == ir.rows_with_lower_entries(pattern)
    # a row with entries below the diagonal and no work is wide at 0 only
    pattern = tr.bidiagonal(4)
    assert [sc.expected_wide_rows(pattern, t) for t in (0, 1)] == [3, 0]


def test_default_wide_work_is_the_library_s():
    with open(os.path.join(ROOT, "spalinalg_amd", "csrc", "spal_internal.hpp")) as f:
        m = re.search(r"constexpr\s+int64_t\s+kIluWideWorkDefault\s*=\s*(\d+)\s*;", f.read())
    assert m and int(m.group(1)) == sc.WIDE_WORK_DEFAULT


# ---- what the default seeds cover --------------------------------------------------------------------------------------

def _longest_run(flags):
    best = cur = 0
    for f in flags:
        cur = cur + 1 if f else 0
        best = max(best, cur)
    return best


def _facts(seed):
    """What one seed brings, from its pattern and knobs alone."""
    pattern, _, _, _, k = sc.case(seed)
    n, rowptr, colind = pattern
    level_of, nl = tr.levels(*pattern, lower=True)
    w = np.array(tr.level_widths(level_of, nl), dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    cols = colind.astype(np.int64)
    total = np.diff(rowptr.astype(np.int64))
    low, up = np.bincount(rows[cols < rows], minlength=n), np.bincount(rows[cols > rows], minlength=n)
    facts = {
        "a lower level wider than 1024 rows": bool((w > 1024).any()),
        "a lower level of 257 to 1024 rows": bool(((w >= 257) & (w <= 1024)).any()),
        "100 consecutive levels of at most 64 rows": _longest_run(w <= 64) >= 100,
        "a level above 256 rows directly between two of at most 64": bool(
            w.size >= 3 and ((w[1:-1] > 256) & (w[:-2] <= 64) & (w[2:] <= 64)).any()),
        "a row of more than 256 entries with one below the diagonal": bool(((total > 256) & (low > 0)).any()),
        "a lower part above 2048 entries": bool((low > 2048).any()),
        "an upper part above 2048 entries": bool((up > 2048).any()),
        "256 consecutive diagonal-only rows": _longest_run((total == 1) & (low == 0) & (up == 0)) >= 256,
        "n no multiple of 256": n % 256 != 0,
        "other triangle: " + k["other"]: True,
        "dtype: " + k["dtype"].name: True,
        "kind: " + k["kind"]: True,
        "trsv_chain_rows = %d" % k["chain_rows"]: True,
    }
    if not k["dropped"]:                                    # the others run neither ILU(0) nor a Krylov method
        facts["%s with %s" % (k["method"], k["prec"])] = True
        facts["ilu_wide_work = %s" % k["wide_work"]] = True
        if k["maxit"] >= 1 and n > 2:                       # ... where the preconditioner decides bits of x
            facts["%s with %s iterates" % (k["method"], k["prec"])] = True
    return facts


CONDITIONS_TWICE = (
    ["a lower level wider than 1024 rows", "a lower level of 257 to 1024 rows", "100 consecutive levels of at most 64 rows",
     "a level above 256 rows directly between two of at most 64", "a row of more than 256 entries with one below the diagonal",
     "a lower part above 2048 entries", "an upper part above 2048 entries", "256 consecutive diagonal-only rows",
     "n no multiple of 256"]
    + ["other triangle: " + o for o in sc.OTHER] + ["dtype: float64", "dtype: float32", "kind: csr", "kind: csc"]
    + ["%s with %s" % mp for mp in itertools.product(sc.METHODS, sc.PRECS)])
CONDITIONS_ONCE = (["trsv_chain_rows = %d" % c for c in sc.CHAIN_ROWS] + ["ilu_wide_work = %s" % w for w in sc.WIDE_WORK]
                   + ["%s with %s iterates" % mp for mp in itertools.product(sc.METHODS, sc.PRECS)])


def test_default_seeds_cover_the_schedule_conditions():
    counts = {}
    for seed in SEEDS:
        for name, holds in _facts(seed).items():
            counts[name] = counts.get(name, 0) + int(holds)
    missing = [(c, counts.get(c, 0)) for c in CONDITIONS_TWICE if counts.get(c, 0) < 2]
    missing += [(c, 0) for c in CONDITIONS_ONCE if counts.get(c, 0) < 1]
    assert not missing, missing


def test_the_restatements_are_not_vacuous_on_the_default_seeds():
    """Some seed's launch count is neither its level count nor one, at its drawn trsv_chain_rows; some seed's wide rows
    are neither none nor every row with an entry below the diagonal, at a threshold other than 0 and 1 << 40."""
    mixed_launches, mixed_forms = [], []
    for seed in SEEDS:
        pattern, _, _, _, k = sc.case(seed)
        for lower in (True, False):
            w = tr.level_widths(*tr.levels(*pattern, lower=lower))
            for c in (k["chain_rows"], k["chain_rows_2"]):
                launches, chains = sc.expected_launches(w, c)
                if launches not in (1, len(w)) and 0 < chains < launches:
                    mixed_launches.append((seed, lower, c))
        if k["dropped"] or k["wide_work"] in (0, HUGE):
            continue
        t = sc.WIDE_WORK_DEFAULT if k["wide_work"] is None else k["wide_work"]
        if 0 < sc.expected_wide_rows(pattern, t) < ir.rows_with_lower_entries(pattern):
            mixed_forms.append((seed, t))
    assert len(mixed_launches) >= 2, mixed_launches
    assert len({t for _, t in mixed_forms}) >= 2, mixed_forms       # at two different thresholds at least
