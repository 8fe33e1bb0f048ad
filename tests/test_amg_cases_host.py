"""CPU tests that keep tests/test_gpu_amg_fuzz.py honest: every default seed of tests/amg_cases.py is a valid, finite
input; between them the seeds reach every stop rule, the poll batches of the rounds, hubs and large aggregates on wide and
on tail levels and the W-cycle with nothing between two visits; `expected_rounds` says what the header says on hand
cases; the text (tests/amg_ref.py) has the structure it claims on every seed; and on the small seeds the text is compared
with the MATHEMATICS it claims -- P^T A P, damped Jacobi, x += alpha P e as dense linear algebra -- not with itself."""
import os
import re

import numpy as np
import pytest

from tests import amg_cases as ac
from tests import amg_ref as ar
from tests import colour_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(ac.DEFAULT_SEEDS)
DENSE_ROWS = 1100
DESCENDING_PATH_3000_ROUNDS = 2999       # what describe()["rounds"][0] of tests/test_gpu_amg.py's descending_path_3000 is


def _rows_of(pattern):
    return np.repeat(np.arange(pattern[0], dtype=np.int64), np.diff(pattern[1].astype(np.int64)))


# ---- every seed is a valid, finite input -----------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_seed_is_valid_and_finite(seed):
    pattern, values, b, k = ac.case(seed)
    n, rowptr, colind = pattern
    assert n == ac.N_TABLE[seed % 12] == k["n"] and rowptr.dtype == colind.dtype == np.uint64 and rowptr.shape == (n + 1,)
    rp = rowptr.astype(np.int64)
    assert rp[0] == 0 and rp[-1] == colind.size == values.size and np.all(np.diff(rp) >= 1)
    rows, cols = _rows_of(pattern), colind.astype(np.int64)
    assert cols.min() >= 0 and cols.max() < n
    same_row = rows[1:] == rows[:-1]
    assert np.all(cols[1:][same_row] > cols[:-1][same_row]), "columns must ascend strictly inside a row"
    assert values.dtype == b.dtype == k["dtype"] and b.shape == (n,)
    assert np.isfinite(values).all() and np.isfinite(b).all()
    assert not any(a.flags.writeable for a in (rowptr, colind, values, b))
    # every row stores its diagonal, positive and at least the sum of the row's other entries
    assert np.all(ar.diagonal_positions(pattern) >= 0)
    off = rows != cols
    weight = np.bincount(rows[off], weights=np.abs(values[off]).astype(np.float64), minlength=n)
    diag = values[ar.diagonal_positions(pattern)].astype(np.float64)
    assert np.all(diag > 0) and np.all(diag >= weight * (1 - 1e-6))
    assert k["what"]["integers"] == bool(np.all(values == np.rint(values))) or n <= 2
    assert k["what"]["integers"] or np.all(values[off] < 0)
    if off.sum() > 40:                                              # values differ from entry to entry
        assert np.unique(values[off]).size >= (2 if k["what"]["integers"] else off.sum() // 2)
    # the pattern is symmetric on the seeds that say so, and not on the others (where there is room for an edge)
    mirrored = set(zip(cols[off].tolist(), rows[off].tolist())) == set(zip(rows[off].tolist(), cols[off].tolist()))
    hub_one_sided = any(one for _, _, one in k["what"]["hubs"])
    assert mirrored == (k["what"]["symmetric"] and not hub_one_sided) or n <= 2
    # isolated vertices: about 5 %
    if n >= 255:
        lonely = n - np.unique(np.concatenate([rows[off], cols[off]])).size
        assert 0.04 * n <= lonely <= 0.12 * n, lonely
    # hubs: the row of a hub holds the drawn number of entries
    for hub, length, _ in k["what"]["hubs"]:
        assert length in ac.HUB_LENGTHS and int(rp[hub + 1] - rp[hub]) == length
    # the knobs
    p = k["params"]
    assert set(p) == set(ar.DEFAULTS) and p["seed"] in ac.SEEDS and p["max_levels"] in ac.MAX_LEVELS
    assert p["coarse_rows"] in ac.COARSE_ROWS and p["nu"] in ac.NU and p["coarse_sweeps"] in ac.COARSE_SWEEPS
    assert p["gamma"] in (1, 2) and p["omega"] in ac.OMEGA and p["alpha"] in ac.ALPHA
    assert k["kind"] in ("csr", "csc") and k["method"] in ac.METHODS and k["maxit"] in ac.MAXIT
    h = ac.reference(seed)
    assert {0, ac.TAIL_DEFAULT, ac.TAIL_CLAMP} <= set(k["tails"])
    assert any(t in h.rows and max(t - 1, 0) in k["tails"] for t in k["tails"])
    x = h.cycle(b)
    assert x.dtype == k["dtype"] and np.isfinite(x).all()


def test_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "spalinalg_amd", "csrc", "spal_amg.hip")).read()
    m = re.search(r"kTailRowsDefault = (\d+), kTailRowsMax = (\d+)", text)
    assert (int(m.group(1)), int(m.group(2))) == (ac.TAIL_DEFAULT, ac.TAIL_CLAMP)
    assert re.search(r"kThreads = 256, kTailThreads = 1024", text)
    assert re.search(r"kFirstBatch = 8, kMaxBatch = 512", text) and re.search(r"kLong = 32;", text)


# ---- the rounds ------------------------------------------------------------------------------------------------------

def test_expected_rounds_on_hand_cases():
    assert ac.expected_rounds(ar.diagonal(300)[0]) == 1
    # a descending path: the second vertex of the order is the first root (the ends have degree 1), then one vertex per
    # round: n - 1 rounds
    for n in (3, 9, 10, 25, 26):
        assert ac.expected_rounds(ar.descending_path(n)[0]) == n - 1
    assert ac.expected_rounds(ar.descending_path(3000)[0]) == DESCENDING_PATH_3000_ROUNDS
    assert ac.expected_rounds(ar.descending_path(57, 2**32 + 7)[0], 7) == 56          # only seed mod 2^32 enters
    # a star: the hub in round 0, every leaf in round 1; a path of 2: both have degree 1, the keys decide
    assert ac.expected_rounds(ar.star(50, True)[0]) == 2 and ac.expected_rounds(ar.star(50, False)[0]) == 2
    assert ac.expected_rounds(ar.path(2)[0]) == 2


def test_expected_rounds_is_the_rule_played_round_by_round():
    """The closed form against a simulation of the kernel's rule: all vertices of a round decide from the state BEFORE it."""
    for seed in (3, 4, 7, 15, 16):
        pattern, _, _, k = ac.case(seed)
        for lv in ac.reference(seed).levels[:-1]:
            n = lv.n
            ptr, nbr = cr.adjacency(lv.pattern)
            prio = ar.priorities(lv.pattern, k["params"]["seed"])
            src = np.repeat(np.arange(n), np.diff(ptr))
            higher = prio[nbr] > prio[src]
            state = np.zeros(n, dtype=np.int64)                         # 0 undecided, 1 non-root, 2 root
            r = 0
            while (state == 0).any():
                beside_root = np.bincount(src[higher], weights=(state[nbr[higher]] == 2), minlength=n) > 0
                pending = np.bincount(src[higher], weights=(state[nbr[higher]] == 0), minlength=n) > 0
                new = state.copy()
                new[(state == 0) & beside_root] = 1
                new[(state == 0) & ~beside_root & ~pending] = 2
                assert (new != state).any()
                state, r = new, r + 1
            assert r == ac.expected_rounds(lv.pattern, k["params"]["seed"])
            assert np.array_equal(state == 2, _roots(lv.agg, prio))


def _roots(agg, prio):
    """The root flags from the aggregates alone: a non-root joins a root that was decided before it, so the root is its
    aggregate's member of highest priority."""
    order = np.lexsort((prio, agg))
    last = np.ones(agg.size, dtype=bool)
    last[:-1] = agg[order][1:] != agg[order][:-1]
    root = np.zeros(agg.size, dtype=bool)
    root[order[last]] = True
    return root


# ---- what the default seeds reach ------------------------------------------------------------------------------------

def _level_facts(seed):
    """[(rows, longest row, largest aggregate or 0, rounds or 0)] per level of the reference"""
    _, _, _, k = ac.case(seed)
    h = ac.reference(seed)
    out = []
    for lv in h.levels:
        longest = int(np.diff(lv.pattern[1].astype(np.int64)).max())
        coarser = lv.agg is not None
        out.append((lv.n, longest, int(np.bincount(lv.agg).max()) if coarser else 0,
                    ac.expected_rounds(lv.pattern, k["params"]["seed"]) if coarser else 0))
    return out


def test_default_seeds_reach_what_the_device_test_is_there_for():
    stops, rounds = {}, []
    hub_wide = hub_tail = agg_wide = agg_tail = 0
    bare = tail0_w = w_deep = 0
    dtypes, kinds, gammas, sided = set(), set(), set(), set()
    level0, coarse = set(), set()
    for seed in SEEDS:
        _, _, _, k = ac.case(seed)
        h, p = ac.reference(seed), k["params"]
        facts = _level_facts(seed)
        stops.setdefault(h.stopped_by, []).append(seed)
        rounds += [f[3] for f in facts if f[3]]
        hub_wide += any(n > ac.TAIL_CLAMP and row > 32 for n, row, _, _ in facts)
        hub_tail += any(n <= ac.TAIL_DEFAULT and row > 32 for n, row, _, _ in facts)
        agg_wide += any(n > ac.TAIL_CLAMP and agg > 32 for n, _, agg, _ in facts)
        agg_tail += any(n <= ac.TAIL_DEFAULT and agg > 32 for n, _, agg, _ in facts)
        dtypes.add(k["dtype"].name), kinds.add(k["kind"]), gammas.add(p["gamma"]), sided.add(k["what"]["symmetric"])
        bare += p["nu"] == 1 and p["coarse_sweeps"] == 1
        starts_at_0 = any(ac.tail_from_level(h.rows, t) == 0 for t in k["tails"])
        tail0_w += starts_at_0 and p["gamma"] == 2 and len(h.levels) >= 3
        w_deep += starts_at_0 and p["gamma"] == 2 and len(h.levels) >= 3 and p["nu"] == 1 and p["coarse_sweeps"] == 1
        level0.add(h.rows[0])
        coarse.update(h.rows[1:])
    print("stop rules:", {s: len(v) for s, v in stops.items()}, "rounds:", sorted(rounds),
          f"hub rows > 32 on > 4096 / <= 1024 rows: {hub_wide} / {hub_tail}, aggregates > 32: {agg_wide} / {agg_tail};",
          f"nu = coarse_sweeps = 1: {bare}; W-cycle in a tail from level 0 over >= 3 levels: {tail0_w} (with nu = cs = 1: {w_deep})")
    for rule in ("coarse_rows", "max_levels", "no_coarsening", "diagonal"):
        assert len(stops.get(rule, [])) >= 2, (rule, stops)
    for batch in (8, 24, 56):                                      # the polls after 8, 8 + 16 and 8 + 16 + 32 rounds
        assert any(r > batch for r in rounds) and any(r <= batch for r in rounds)
    assert 8 in rounds or 24 in rounds or 56 in rounds             # the last round of a batch
    assert hub_wide >= 1 and hub_tail >= 1 and agg_wide >= 1 and agg_tail >= 1
    assert dtypes == {"float64", "float32"} and kinds == {"csr", "csc"} and gammas == {1, 2} and sided == {True, False}
    assert bare >= 1 and tail0_w >= 1 and w_deep >= 1
    # level 0 and the coarse levels on both sides of a workgroup, of the tail's default and of its clamp
    for edge in (256, 1024, 4096):
        assert {edge - 1, edge, edge + 1} <= level0
        assert any(n < edge for n in coarse) and any(n > edge for n in coarse)
    assert any(len(ac.reference(s).levels) >= 6 for s in SEEDS)


# ---- the structure of the text ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_text_has_the_structure_it_claims(seed):
    pattern, values, _, k = ac.case(seed)
    h = ac.reference(seed)
    dt = k["dtype"].type
    for lv, nxt in zip(h.levels[:-1], h.levels[1:]):
        n, agg, nagg = lv.n, lv.agg, lv.nagg
        # a partition: every vertex in one aggregate, no aggregate empty
        assert agg.shape == (n,) and agg.min() == 0 and agg.max() == nagg - 1 and np.unique(agg).size == nagg == nxt.n
        ptr, nbr = cr.adjacency(lv.pattern)
        prio = ar.priorities(lv.pattern, k["params"]["seed"])
        assert np.unique(prio).size == n
        src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
        # the roots are a maximal independent set of the symmetrised graph, numbered by ascending row
        root = _roots(agg, prio)
        assert root.sum() == nagg and np.array_equal(agg[root], np.arange(nagg))  # numbered by ascending row
        assert _is_mis(root, src, nbr, n)
        # every non-root lies beside its root, which is its neighbouring root of highest priority
        rootof = np.flatnonzero(root)[agg]
        beside = set(zip(src.tolist(), nbr.tolist()))
        nonroot = np.flatnonzero(~root)
        assert all((v, rootof[v]) in beside for v in nonroot.tolist())
        best = np.zeros(n, dtype=np.uint64)
        np.maximum.at(best, src[root[nbr]], prio[nbr[root[nbr]]])
        assert np.array_equal(best[nonroot], prio[rootof[nonroot]])
        # the coarse level: the triplets (agg[i], agg[j], v) in storage order, summed one after the other per entry;
        # an entry is stored unless that sum is an exact zero
        ci, cj = agg[_rows_of(lv.pattern)], agg[lv.pattern[2].astype(np.int64)]
        key = ci * nagg + cj
        order = np.argsort(key, kind="stable")
        uniq, start, count = np.unique(key[order], return_index=True, return_counts=True)
        sums = np.zeros(uniq.size, dtype=dt)
        vals = lv.values[order]
        for t in range(int(count.max())):
            live = count > t
            sums[live] = sums[live] + vals[start[live] + t]
        kept = sums != 0
        got_key = _rows_of(nxt.pattern) * nagg + nxt.pattern[2].astype(np.int64)
        assert np.array_equal(got_key, uniq[kept])
        assert nxt.values.tobytes() == sums[kept].tobytes()
        assert (~kept).sum() == 0 or k["what"]["integers"]
    if h.stopped_by == "diagonal":
        assert k["what"]["integers"] and k["what"]["zero_sum"]


def _is_mis(root, src, nbr, n):
    """independent (no two roots adjacent) and maximal (every other vertex beside a root)"""
    independent = not np.any(root[src] & root[nbr])
    covered = root.copy()
    covered[src[root[nbr]]] = True
    return independent and bool(covered.all())


# ---- the text against the mathematics --------------------------------------------------------------------------------

def _dense(pattern, values, dtype):
    a = np.zeros((pattern[0], pattern[0]), dtype=dtype)
    a[_rows_of(pattern), pattern[2].astype(np.int64)] = values
    return a


def _ptap_by_sums(a, agg, nagg):
    """P^T A P with P[i, agg[i]] = 1, in a's dtype: columns, then rows, added aggregate by aggregate"""
    order = np.argsort(agg, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(agg, minlength=nagg))[:-1]])
    ap = np.add.reduceat(a[:, order], starts, axis=1)
    return np.add.reduceat(ap[order, :], starts, axis=0)


def _dense_cycle(levels, aggs, b, p, l=0):
    """The cycle as dense linear algebra in b's dtype: x = W b, x += W (b - A x), r, P^T r, gamma recursions, x += alpha P e"""
    a, dt = levels[l], b.dtype.type
    w = dt(p["omega"]) / np.diag(a)
    last = l == len(levels) - 1
    x = w * b
    for _ in range((p["coarse_sweeps"] if last else p["nu"]) - 1):
        x = x + w * (b - a @ x)
    if last:
        return x
    agg, nagg = aggs[l]
    for _ in range(p["gamma"]):
        r = b - a @ x
        rc = np.zeros(nagg, dtype=b.dtype)
        np.add.at(rc, agg, r)                                       # P^T r
        x = x + dt(p["alpha"]) * _dense_cycle(levels, aggs, rc, p, l + 1)[agg]
    for _ in range(p["nu"]):
        x = x + w * (b - a @ x)
    return x


def test_text_is_the_mathematics_on_the_small_seeds():
    """The text in float64 against P^T A P and the cycle evaluated densely in numpy.longdouble.

    Level values: a sequential sum of t terms differs from the exact sum by at most (t - 1) eps sum|term|; the text's
    level l + 1 is held to that bound against P^T A_l P of the text's own level l in long double.

    The cycle has no derived bound, so one is measured per case: the difference between the dense float64 and the dense
    long-double evaluation relative to max|x|, times 16, plus one ulp.  Both are independent of the text; a float64
    evaluation in another summation order has the same first-order bound, and one order of magnitude covers the
    constants.  Measured over the 16 default seeds with n <= 1100: dense f64 against long double, largest 1.2e-15,
    median 5.9e-17; text f64 against long double, largest 5.8e-15 (seed 18, where the dense f64 differs by 1.1e-15),
    median 5.9e-17 (all relative to max|x|)."""
    eps, eps_ld = np.finfo(np.float64).eps, np.finfo(np.longdouble).eps
    assert eps_ld < eps / 1000, "numpy.longdouble is no wider than float64 here"
    measured, text_err, checked = [], [], 0
    for seed in SEEDS:
        pattern, values, b, k = ac.case(seed)
        if pattern[0] > DENSE_ROWS:
            continue
        checked += 1
        p = k["params"]
        h = ac.reference(seed) if k["dtype"] == np.float64 else ar.Hierarchy(pattern, values.astype(np.float64), **p)
        assert h.rows == ac.reference(seed).rows
        aggs = [(lv.agg, lv.nagg) for lv in h.levels[:-1]]
        # the levels: the text's A_{l+1} against P^T A_l P of the text's A_l
        for lv, nxt in zip(h.levels[:-1], h.levels[1:]):
            exact = _ptap_by_sums(_dense(lv.pattern, lv.values, np.longdouble), lv.agg, lv.nagg)
            terms = _ptap_by_sums(_dense(lv.pattern, np.ones(lv.values.size), np.float64), lv.agg, lv.nagg)
            mass = _ptap_by_sums(_dense(lv.pattern, np.abs(lv.values), np.longdouble), lv.agg, lv.nagg)
            bound = np.maximum(terms - 1, 0) * eps * mass + terms * eps_ld * mass
            assert np.all(np.abs(_dense(nxt.pattern, nxt.values, np.longdouble) - exact) <= bound)
        # the cycle, on levels formed from level 0 by P^T A P alone
        b64 = b.astype(np.float64)
        out = {}
        for dt in (np.float64, np.longdouble):
            levels = [_dense(pattern, values.astype(dt), dt)]
            for agg, nagg in aggs:
                if dt == np.float64:
                    pm = np.zeros((levels[-1].shape[0], nagg))
                    pm[np.arange(agg.size), agg] = 1.0
                    levels.append(pm.T @ levels[-1] @ pm)
                else:
                    levels.append(_ptap_by_sums(levels[-1], agg, nagg))
            out[dt] = _dense_cycle(levels, aggs, b64.astype(dt), p)
        scale = np.abs(out[np.longdouble]).max()
        diff = float(np.abs(out[np.float64] - out[np.longdouble]).max() / scale)
        got = float(np.abs(h.cycle(b64) - out[np.longdouble]).max() / scale)
        measured.append(diff), text_err.append(got)
        print(f"amg seed {seed}: n {pattern[0]} levels {len(h.levels)} dense f64 - long double {diff:.2e}, text - long double {got:.2e}")
        assert got <= 16 * diff + eps, (seed, got, diff)
    print(f"dense f64 against long double: largest {max(measured):.2e}, median {np.median(measured):.2e}; "
          f"text against long double: largest {max(text_err):.2e}, median {np.median(text_err):.2e}; {checked} seeds")
    assert checked >= 12
