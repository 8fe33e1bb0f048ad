"""CPU tests that keep tests/test_gpu_spgemm_tiers.py honest: the host mirror of the SpGEMM binning
(tests/spgemm_cases.py) against the text of spal_spgemm.hip, every generator against what it promises, the inputs'
order sensitivity, and the tier coverage of the power-law fixture and of the fuzz seeds."""
import os
import re

import numpy as np
import pytest

from tests import spgemm_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "spalinalg_amd", "csrc", "spal_spgemm.hip")
DTYPES = [np.float64, np.float32]


# ---- 1. drift: the mirror against the source ---------------------------------------------------------------------
def check_drift(text):
    """asserts that spal_spgemm.hip's constants are the mirror's (also run on altered copies below)"""
    def const(name):
        m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\w+)\s*;" % name, text)
        assert m, name
        return int(m.group(1).rstrip("u"), 0)

    assert const("kDefaultCap") == sc.DEFAULT_CAP
    assert const("kMaxCap") == sc.MAX_CAP
    m = re.search(r"kTierNames\[kTiers\]\s*=\s*\{([^}]*)\}", text)
    assert tuple(re.findall(r'"(\w+)"', m.group(1))) == sc.TIER_NAMES
    m = re.search(r"return ub <= (\d+) \? 1 : ub <= (\d+) \? 2 : ub <= (\d+) \? 3 : ub <= (\d+) \? 4 : 5;", text)
    assert m and tuple(int(x) for x in m.groups()) == sc.CUTS
    assert re.search(r"if \(route == 2 \|\| ub > cap\) return 6;", text)
    m = re.search(r"slot_of\(uint32_t j, int bits\) \{ return \(j \* (0x[0-9A-Fa-f]+)u\) >> \(32 - bits\); \}", text)
    assert m and int(m.group(1), 16) == sc.HASH_MULT
    launches = re.findall(r"launch_tier<T, (\d+), (\d+), (\d+)>\(numeric, list \+ tier_start\[(\d)\]", text)
    assert len(launches) == 5
    for g, ts, gpb, t in launches:
        assert (int(g), int(ts), int(gpb)) == sc.GEOMETRY[sc.TIER_NAMES[int(t)]], t
    # every table is twice its tier's largest ub (half full at the cut), the route-1 cap is the largest table's half
    for tier, (_, ts, _) in sc.GEOMETRY.items():
        assert ts == 2 * sc.TIER_UB[tier]
    assert re.search(r"route == 1 \? kMaxCap : lds_cap > 0 \? \(uint32_t\)std::min<int64_t>\(lds_cap, kMaxCap\) : kDefaultCap", text)
    assert re.search(r"for \(uint32_t x0 = b; x0 < e; x0 \+= %d\)" % sc.CHUNK, text)     # spgemm_run_fill's chunk


def test_mirror_matches_the_source():
    with open(SRC) as f:
        check_drift(f.read())


@pytest.mark.parametrize("old,new", [
    ("kDefaultCap = 2048", "kDefaultCap = 1024"),
    ("launch_tier<T, 256, 8192, 1>", "launch_tier<T, 256, 16384, 1>"),
    ("ub <= 1024 ? 3", "ub <= 1000 ? 3"),
    ("0x9E3779B1u", "0x9E3779B9u"),
])
def test_drift_check_sees_a_change(old, new):
    with open(SRC) as f:
        text = f.read()
    assert old in text
    with pytest.raises(AssertionError):
        check_drift(text.replace(old, new))


def test_mirror_functions_agree():
    assert [sc.effective_cap(r, c) for r, c in ((0, 0), (0, 1), (0, 5000), (1, 7), (2, 0), (0, 4096))] == \
        [2048, 1, 4096, 4096, 2048, 4096]
    for cap, route in ((2048, 0), (4096, 1), (63, 0), (2048, 2)):
        for ub in range(0, 4200):
            want = "empty" if ub == 0 else "large" if (route == 2 or ub > cap) else \
                sc.LDS_TIERS[sum(ub > c for c in sc.CUTS)]
            assert sc.tier_of(ub, cap, route) == want
    assert sc.slot_of(1, 7) == 0x9E3779B1 >> 25 and sc.slot_of(3, 13) == ((3 * 0x9E3779B1) & 0xFFFFFFFF) >> 19


def brute_expected(a, b, route, lds_cap):
    """expected() by a plain loop over rows and entries"""
    (arp, aci, _), (brp, _, _) = a, b
    cap = 4096 if route == 1 else (min(lds_cap, 4096) if lds_cap > 0 else 2048)
    tiers = dict.fromkeys(sc.TIER_NAMES, 0)
    products = large = 0
    for i in range(len(arp) - 1):
        ub = 0
        for q in range(int(arp[i]), int(arp[i + 1])):
            k = int(aci[q])
            ub += int(brp[k + 1]) - int(brp[k])
        if ub == 0:
            name = "empty"
        elif route == 2 or ub > cap:
            name = "large"
        elif ub <= 64:
            name = "g16"
        elif ub <= 256:
            name = "g32"
        elif ub <= 1024:
            name = "wave"
        elif ub <= 2048:
            name = "block4k"
        else:
            name = "block8k"
        tiers[name] += 1
        products += ub
        large += ub if name == "large" else 0
    return {"tier_rows": tiers, "products": products, "large_products": large}


def check_case(case, oracle, configs):
    """the generator's per-row claims against the arrays and the oracle's product; expected() against brute force"""
    (arp, aci, av), (brp, bci, bv) = case.a, case.b
    assert len(arp) == case.m + 1 and len(brp) == case.n + 1 and av.dtype == bv.dtype
    assert aci.size == 0 or int(aci.max()) < case.n
    assert bci.size == 0 or int(bci.max()) < case.p
    for ptr, ind in ((arp, aci), (brp, bci)):        # valid CSR: columns increase strictly inside a row
        inner = np.ones(ind.size, dtype=bool)
        inner[np.asarray(ptr[:-1], dtype=np.int64)[np.diff(ptr.astype(np.int64)) > 0]] = False
        assert np.all(np.diff(ind.astype(np.int64))[inner[1:]] > 0)
    ref = oracle.csr_mul(*case.shapes[:1], case.a, case.shapes[1], case.b)
    ub = sc.row_ub(case.a, case.b)
    if case.rows is not None:
        assert [r["ub"] for r in case.rows] == ub.tolist()
        assert [r["distinct"] for r in case.rows] == np.diff(ref[0].astype(np.int64)).tolist()
    for route, cap in configs:
        assert sc.expected(case.a, case.b, route, cap) == brute_expected(case.a, case.b, route, cap)
    return ref, ub


# ---- 2. generator claims ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_boundaries_claims(oracle, dtype):
    case = sc.boundaries(1, dtype)
    configs = [(0, 0), (1, 0), (2, 0)] + [(0, c) for c in sc.BOUNDARY_CAPS]
    check_case(case, oracle, configs)
    rows = [r for r in case.rows if r["kind"] == "boundary"]
    assert len(case.rows) == 2 * len(rows)                       # as many empty rows
    for r in rows:
        assert r["ub"] == r["want_ub"]
        if r["shape"] == "distinct":
            assert r["distinct"] == r["ub"]                      # the table half full at the cut, no padding to sort
        elif r["way"] == "ubx1" and r["shape"] == "one":
            assert r["distinct"] == 1
        elif r["shape"] == "half":
            assert abs(r["distinct"] - (r["ub"] + 1) // 2) <= max(1, int(r["ub"] ** 0.5))
    for ub in sc.BOUNDARY_UBS:
        got = {(r["way"], r["shape"]) for r in rows if r["ub"] == ub}
        assert got == {("1xub", "distinct")} | {(w, s) for w in ("ubx1", "square") for s in ("distinct", "one", "half")}
    for cut in sc.CUTS + (sc.MAX_CAP,):
        assert {cut - 1, cut, cut + 1} <= set(sc.BOUNDARY_UBS)
    # ub = cap is an LDS row, ub = cap + 1 a large one, for every cap the GPU test sets
    for cap in sc.BOUNDARY_CAPS:
        assert cap in sc.BOUNDARY_UBS and cap + 1 in sc.BOUNDARY_UBS
        assert sc.tier_of(cap, sc.effective_cap(0, cap), 0) in sc.LDS_TIERS
        assert sc.tier_of(cap + 1, sc.effective_cap(0, cap), 0) == "large"
    # the rows of one tier are not neighbours: the shuffle mixed them
    kinds = [sc.tier_of(r["ub"], sc.MAX_CAP, 1) for r in case.rows]
    assert sum(kinds[i] != kinds[i + 1] for i in range(len(kinds) - 1)) > len(kinds) // 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tier", sorted(sc.WITNESS))
def test_order_witness_claims(oracle, tier, dtype):
    case = sc.order_witness(tier, dtype)
    _, opts = sc.WITNESS[tier]
    route = opts.get("spgemm_route", 0)
    ref, ub = check_case(case, oracle, [(route, 0)])
    e = sc.expected(case.a, case.b, route, 0)["tier_rows"]
    assert e[tier] == case.m - 1 and e["empty"] == 1             # every row is in the tier the case is named for
    rp, ci, va = ref
    lanes = sc.GEOMETRY.get(tier, (256,))[0]
    for i, r in enumerate(case.rows):
        row = dict(zip(ci[int(rp[i]):int(rp[i + 1])].tolist(), va[int(rp[i]):int(rp[i + 1])].tolist()))
        if r["kind"] == "three":
            assert row[r["witness"]] == 1.0                      # ((1e16 - 1e16) + 1)
            idx = r["index_in_b_row"]
            assert len({x % lanes for x in idx}) == 3            # another lane at every k
            if sc.WITNESS[tier][0] > lanes:
                assert len({x // lanes for x in idx}) >= 2       # ... and another step
            if tier == "large":
                k0 = int(case.a[1][int(case.a[0][i])])
                below = sum(int((case.b[1][int(case.b[0][k]):int(case.b[0][k + 1])] < r["witness"]).sum())
                            for k in range(k0, k0 + 3))
                assert below % sc.CHUNK == sc.CHUNK - 1          # the run of 3 spans two chunks
        elif r["kind"] == "many":
            assert r["ub"] == 2 * r["terms"] and r["distinct"] == r["terms"] + 1
            if tier != "large":
                assert r["ub"] == sc.TIER_UB[tier]
            else:
                assert r["terms"] > 4 * sc.CHUNK                 # the witness run covers several chunks
        elif r["kind"] == "dense":
            assert r["ub"] == (sc.TIER_UB[tier] if tier != "large" else 2200) // r["terms"] * r["terms"] - 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_hash_worst_claims(oracle, dtype):
    case = sc.hash_worst(dtype)
    check_case(case, oracle, [(0, 0), (1, 0)])
    seen = set()
    for r in case.rows:
        if r["kind"] == "empty":
            continue
        tier, kind = r["tier"], r["kind"]
        seen.add((tier, kind))
        bits, ts = sc.table_bits(tier), sc.GEOMETRY[tier][1]
        assert r["ub"] == sc.TIER_UB[tier] == ts // 2
        keys = np.asarray(r["keys"])
        assert np.unique(keys).size == keys.size
        assert r["distinct"] == keys.size == (r["ub"] if kind in ("top", "same") else r["ub"] // 2)
        homes = sc.slot_of(keys, bits)
        own = keys[keys != case.p - 1]                            # (column ncols - 1 replaces one key)
        if kind.startswith("top"):
            assert sc.slot_of(own, bits).min() >= ts - min(64, ts // 8)
        else:
            assert np.all(sc.slot_of(own, bits) == ts - 1)
        if kind in ("top", "same"):
            assert r["last_column"] and case.p - 1 in keys
        lengths, wrapped = sc.probe_lengths(keys, bits)
        # the keys pile up behind the table's end: nearly all of them wrap, the longest chain is about the key count
        room = min(64, ts // 8) if kind.startswith("top") else 1
        assert wrapped >= keys.size - room - 1 and wrapped >= 1
        assert lengths.max() >= keys.size - room - 1
        if kind.endswith("_adv"):
            assert np.all(np.diff(homes) <= 0) and not np.all(np.diff(keys) > 0)
        if kind.endswith("_asc"):
            assert np.all(np.diff(keys) > 0)
    want = {(t, k + s) for t in sc.LDS_TIERS for k in ("top",) for s in ("", "_asc", "_adv")}
    want |= {(t, "same" + s) for t in ("g16", "g32") for s in ("", "_asc", "_adv")}
    assert seen == want
    assert case.p == 1 << 20


def test_collision_sets_exist_in_2_20_columns():
    counts = []
    for tier in sc.LDS_TIERS:
        ts = sc.GEOMETRY[tier][1]
        home = sc.slot_of(np.arange(1 << 20), sc.table_bits(tier))
        counts.append(int((home >= ts - min(64, ts // 8)).sum()))
        assert counts[-1] >= sc.TIER_UB[tier]
    assert counts[-1] == 8191
    for tier in ("g16", "g32"):
        ts = sc.GEOMETRY[tier][1]
        assert int((sc.slot_of(np.arange(1 << 20), sc.table_bits(tier)) == ts - 1).sum()) >= sc.TIER_UB[tier]


@pytest.mark.parametrize("p", [1, 1 << 20])
def test_large_runs_claims(oracle, p):
    case = sc.large_runs(np.float64, p)
    ref, ub = check_case(case, oracle, [(0, 0), (2, 0), (0, 48)])
    e = sc.expected(case.a, case.b, 0, 48)["tier_rows"]
    assert e["large"] == len(sc.RUN_ROWS) and e["g16"] == 3 * len(sc.RUN_ROWS) and e["empty"] == len(sc.RUN_ROWS)
    rp, ci, _ = ref
    heads, lengths, totals = set(), set(), set()
    for i, r in enumerate(case.rows):
        if r["kind"] != "runs":
            continue
        runs = np.asarray(r["runs"])
        assert r["ub"] == runs.sum() and r["distinct"] == runs.size
        # the oracle's row and the products per column say the same
        k0, k1 = int(case.a[1][int(case.a[0][i])]), int(case.a[1][int(case.a[0][i + 1]) - 1])
        cols = case.b[1][int(case.b[0][k0]):int(case.b[0][k1 + 1])].astype(np.int64)
        uniq, cnt = np.unique(cols, return_counts=True)
        assert np.array_equal(uniq, ci[int(rp[i]):int(rp[i + 1])].astype(np.int64)) and np.array_equal(cnt, runs)
        h = sc.run_heads(runs)
        heads |= set((h[runs > 1] % sc.CHUNK).tolist())
        lengths |= set(runs.tolist())
        totals.add(int(runs.sum()))
    if p == 1:
        assert all(len(r["runs"]) == 1 for r in case.rows if r["kind"] == "runs")     # a single run = the whole row
        assert {t % sc.CHUNK for t in totals} >= {0, 1, sc.CHUNK - 1}
    else:
        assert {0, 63, 64, 255} <= heads                       # a run head on lane 63 / thread 255 among them
        assert {2, 255, 256, 257, 1025, 5000} <= lengths
        assert {sc.CHUNK * 9 - 1, sc.CHUNK * 9, sc.CHUNK * 9 + 1} <= totals
        assert any(len(r["runs"]) == 1 for r in case.rows if r["kind"] == "runs")
        assert any(set(r["runs"]) == {1} for r in case.rows if r["kind"] == "runs")   # all-distinct rows
        assert int(case.b[1].max()) == p - 1
        spans = [r for r in case.rows if r["kind"] == "runs" and r["name"] == "run1025_at255"][0]
        h = sc.run_heads(spans["runs"])
        assert h[255] == 255 and spans["runs"][255] == 1025      # one run over five chunks, its head on thread 255


# ---- 3. order sensitivity of the inputs ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tier", sorted(sc.WITNESS))
def test_order_witness_inputs_are_order_sensitive(tier, dtype):
    case = sc.order_witness(tier, dtype)
    n, desc, pair = sc.reorder_sensitivity(case.a, case.b)
    assert n > 50 and 2 * desc >= n and 2 * pair >= n, (n, desc, pair)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fuzz_inputs_are_order_sensitive(dtype):
    """over the default seeds, at least half of C's entries with several products change bits in either other order"""
    n = desc = pair = 0
    for seed in range(16):
        case = sc.fuzz(seed, dtype=dtype)[0]
        r = sc.reorder_sensitivity(case.a, case.b)
        n, desc, pair = n + r[0], desc + r[1], pair + r[2]
    assert n > 10_000 and 2 * desc >= n and 2 * pair >= n, (n, desc, pair)


def test_reorder_sensitivity_counts_what_it_says():
    # one entry, three products: ((1e16 - 1e16) + 1) = 1, backwards 0; pairwise (a + b) + c is the forward sum
    a = (np.array([0, 3]), np.array([0, 1, 2]), np.array([1e16, -1e16, 1.0]))
    b = (np.array([0, 1, 2, 3]), np.array([0, 0, 0]), np.array([1.0, 1.0, 1.0]))
    assert sc.reorder_sensitivity(a, b) == (1, 1, 0)
    a4 = (np.array([0, 4]), np.array([0, 1, 2, 3]), np.array([1.0, 1e16, -1e16, 1.0]))
    b4 = (np.array([0, 1, 2, 3, 4]), np.array([0, 0, 0, 0]), np.ones(4))
    assert sc.reorder_sensitivity(a4, b4) == (1, 0, 1)          # forward 1, backward 1, (1 + 1e16) + (-1e16 + 1) = 0


# ---- 4. tier coverage ------------------------------------------------------------------------------------------
def test_fuzz_seeds_cover_every_tier(oracle):
    total = dict.fromkeys(sc.TIER_NAMES, 0)
    shapes, dtypes, fmts = set(), set(), set()
    for seed in range(16):
        case, dt, fm, opts = sc.fuzz(seed)
        check_case(case, oracle, [(opts["spgemm_route"], opts["spgemm_lds_cap"])])
        e = sc.expected(case.a, case.b, opts["spgemm_route"], opts["spgemm_lds_cap"])
        for k, v in e["tier_rows"].items():
            total[k] += v
        shapes |= {("m", case.m == 1), ("n", case.n == 1), ("p", case.p)}
        dtypes.add(dt.name)
        fmts.add(fm)
        for arr in (case.a[2], case.b[2]):
            if arr.size >= 256:
                assert np.isnan(arr).any() and np.isinf(arr).any() and (arr == 0).any()
                assert ((arr != 0) & (np.abs(arr) < np.finfo(arr.dtype).tiny)).any()          # subnormals
    assert all(v > 0 for v in total.values()), total
    assert {("m", True), ("n", True), ("p", 1), ("p", 1 << 20)} <= shapes
    assert dtypes == {"float64", "float32"} and fmts == {"csr", "csc"}


def test_power_law_fixture_fills_every_lds_tier():
    """the operands of test_gpu_spgemm.py::test_every_route_bit_for_bit: under route 1 every LDS tier holds a row"""
    import spal_synth as synth
    from tests.test_gpu_spgemm import power_law_operand_arrays
    n, a, banded = power_law_operand_arrays(synth)
    for b in (a, banded):
        t = sc.expected(a, b, 1, 0)["tier_rows"]
        assert all(t[name] > 0 for name in sc.LDS_TIERS), t
