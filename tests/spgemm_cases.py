"""Constructed inputs for the sparse x sparse product and a host mirror of its row binning (test infrastructure, plain
numpy, no GPU).

The mirror restates the constants of spalinalg_amd/csrc/spal_spgemm.hip (tests/test_spgemm_cases_host.py reads that
file and fails when they drift apart): the tier cuts, the default and largest LDS cap, the five table geometries and
the multiplicative hash.  `expected()` is what `describe()["spgemm"]` of a product must report.

Every generator returns a `Case`: valid CSR arrays of A (m x n) and B (n x p) (strictly increasing columns inside a
row) and, per row of A, the properties it promises (`ub` = products of the row, `distinct` = its distinct columns,
and whatever else the generator states).  The CSC form of a case feeds the same arrays as B^T * A^T.
"""
import numpy as np

# ---- the mirror ------------------------------------------------------------------------------------------------
TIER_NAMES = ("empty", "g16", "g32", "wave", "block4k", "block8k", "large")
LDS_TIERS = TIER_NAMES[1:6]
CUTS = (64, 256, 1024, 2048)           # ub <= cut -> g16 / g32 / wave / block4k, above (up to the cap) block8k
DEFAULT_CAP = 2048                     # kDefaultCap
MAX_CAP = 4096                         # kMaxCap
HASH_MULT = 0x9E3779B1
# tier -> (G lanes per row, TS table slots, GPB rows per workgroup): the launch_tier<T, G, TS, GPB> lines
GEOMETRY = {"g16": (16, 128, 16), "g32": (32, 512, 4), "wave": (64, 2048, 1), "block4k": (256, 4096, 1),
            "block8k": (256, 8192, 1)}
TIER_UB = {"g16": 64, "g32": 256, "wave": 1024, "block4k": 2048, "block8k": 4096}   # the largest ub of each LDS tier
CHUNK = 256                            # spgemm_run_fill numbers run heads in chunks of 256 entries (4 waves of 64)


def table_bits(tier):
    return GEOMETRY[tier][1].bit_length() - 1


def effective_cap(route, lds_cap):
    if route == 1:
        return MAX_CAP
    return min(int(lds_cap), MAX_CAP) if lds_cap and lds_cap > 0 else DEFAULT_CAP


def tier_of(ub, cap, route):
    if ub == 0:
        return "empty"
    if route == 2 or ub > cap:
        return "large"
    for cut, name in zip(CUTS, LDS_TIERS):
        if ub <= cut:
            return name
    return "block8k"


def slot_of(j, bits):
    """home slot of column j in a table of 2^bits slots (vectorised)"""
    j = np.asarray(j, dtype=np.uint64)
    return (((j * np.uint64(HASH_MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)).astype(np.int64)


def row_ub(a, b):
    """products per row of A: the sum over its entries of the length of B's row"""
    arp, aci = np.asarray(a[0], dtype=np.int64), np.asarray(a[1], dtype=np.int64)
    blen = np.diff(np.asarray(b[0], dtype=np.int64))
    c = np.concatenate([[0], np.cumsum(blen[aci])])
    return c[arp[1:]] - c[arp[:-1]]


def expected(a, b, route=0, lds_cap=0, nnz=None):
    """what describe()["spgemm"] must report for A * B with these options on the left operand; `nnz` = the oracle's"""
    ub = row_ub(a, b)
    cap = effective_cap(route, lds_cap)
    bounds = np.array((0,) + CUTS, dtype=np.int64)
    t = np.searchsorted(bounds, ub, side="left")          # 0 empty, 1..4 by the cuts, 5 above 2048
    if route == 2:
        t = np.where(ub > 0, 6, 0)
    else:
        t = np.where(ub > cap, 6, t)
    counts = np.bincount(t, minlength=7)
    out = {"tier_rows": {name: int(counts[k]) for k, name in enumerate(TIER_NAMES)}, "products": int(ub.sum()),
           "large_products": int(ub[t == 6].sum())}
    if nnz is not None:
        out["nnz"] = int(nnz)
    return out


def reported(d):
    """the part of describe()["spgemm"] that `expected` pins"""
    return {k: d[k] for k in ("tier_rows", "products", "large_products", "nnz")}


def probe_lengths(cols, bits):
    """Linear probing of `cols` (distinct, in insertion order) into 2^bits slots: (slots examined per key, how many
    keys went past the last slot to slot 0)."""
    size = 1 << bits
    used = np.zeros(size, dtype=bool)
    lengths, wrapped = [], 0
    for h in slot_of(cols, bits).tolist():
        n, w = 1, False
        while used[h]:
            h += 1
            if h == size:
                h, w = 0, True
            n += 1
        used[h] = True
        lengths.append(n)
        wrapped += w
    return np.array(lengths, dtype=np.int64), wrapped


def order_sensitive_values(rng, n, dtype, spread=3):
    """sign x mantissa in [1, 2) x 2^e, e uniform over +-spread binades.  The terms of a sum must OVERLAP for its order
    to show: with full random mantissas every add rounds, and terms a few binades apart leave different roundings
    behind in different orders.  (Measured on the CPU for sums of 8 products: +-3 binades per factor changes the bits of
    60 % of the sums when folded backwards, +-30 binades of 22 % in f32 and 46 % in f64 -- terms far below the
    largest one vanish in any order.  tests/test_spgemm_cases_host.py holds the generators to one half.)"""
    e = rng.integers(-spread, spread + 1, n)
    v = rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * np.exp2(e)
    return v.astype(np.dtype(dtype))


# ---- assembling a case -----------------------------------------------------------------------------------------
class Case:
    def __init__(self, m, n, p, a, b, rows):
        self.m, self.n, self.p, self.a, self.b, self.rows = m, n, p, a, b, rows

    @property
    def shapes(self):
        return (self.m, self.n), (self.n, self.p)


class _Build:
    """Rows of A with rows of B of their own: A's row = the consecutive k of the B rows it was given."""

    def __init__(self):
        self.arows, self.avals, self.brows, self.bvals, self.meta = [], [], [], [], []

    def row(self, brows, avals=None, bvals=None, **meta):
        k0 = len(self.brows)
        brows = [np.asarray(c, dtype=np.int64) for c in brows]
        for c in brows:
            assert c.size == 0 or np.all(np.diff(c) > 0), "columns of a B row must increase strictly"
        self.brows += brows
        self.bvals += list(bvals) if bvals is not None else [None] * len(brows)
        self.arows.append(np.arange(k0, k0 + len(brows), dtype=np.int64))
        self.avals.append(avals)
        distinct = int(np.unique(np.concatenate(brows)).size) if brows else 0
        self.meta.append(dict(meta, ub=int(sum(c.size for c in brows)), distinct=distinct))

    def empty(self):
        self.row([], kind="empty")

    def finish(self, rng, dtype, p, shuffle=True):
        order = rng.permutation(len(self.arows)) if shuffle else np.arange(len(self.arows))
        arows = [self.arows[i] for i in order]
        rows = [self.meta[i] for i in order]
        n = max(len(self.brows), 1)
        ap = np.concatenate([[0], np.cumsum([r.size for r in arows])]).astype(np.uint64)
        ac = (np.concatenate(arows) if arows else np.empty(0)).astype(np.uint64)
        av = order_sensitive_values(rng, ac.size, dtype)
        for pos, i in enumerate(order):
            if self.avals[i] is not None:
                av[int(ap[pos]):int(ap[pos + 1])] = np.asarray(self.avals[i], dtype=dtype)
        bp = np.concatenate([[0], np.cumsum([c.size for c in self.brows])]).astype(np.uint64)
        if len(self.brows) == 0:
            bp = np.zeros(2, dtype=np.uint64)
        bc = (np.concatenate(self.brows) if self.brows else np.empty(0)).astype(np.uint64)
        assert bc.size == 0 or int(bc.max()) < p
        bv = order_sensitive_values(rng, bc.size, dtype)
        for k, vals in enumerate(self.bvals):
            if vals is not None:
                bv[int(bp[k]):int(bp[k + 1])] = np.asarray(vals, dtype=dtype)
        return Case(len(arows), n, p, (ap, ac, av), (bp, bc, bv), rows)


def _split(total, parts):
    """`parts` lengths summing to `total`, as even as possible"""
    q, r = divmod(total, parts)
    return [q + (1 if i < r else 0) for i in range(parts)]


# ---- a. tier boundaries ----------------------------------------------------------------------------------------
BOUNDARY_UBS = (1, 2, 63, 64, 65, 66, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
BOUNDARY_CAPS = (1, 63, 64, 65, 2048, 4096)


def _columns_for(rng, lens, shape, p):
    """B rows of the given lengths whose union has as many distinct columns as `shape` asks: "distinct" = the sum of the
    lengths, "one" = as few as valid rows allow (the longest row: 1 where every row holds one entry), "half" = about
    half of the sum."""
    total, longest = sum(lens), max(lens)
    want = {"distinct": total, "one": longest, "half": max(longest, (total + 1) // 2)}[shape]
    pool = np.sort(rng.choice(p, size=want, replace=False))
    if want == total:
        perm = rng.permutation(total)
        cuts = np.concatenate([[0], np.cumsum(lens)])
        return [np.sort(pool[perm[cuts[i]:cuts[i + 1]]]) for i in range(len(lens))]
    rows, uncovered = [], list(rng.permutation(want))
    for ln in lens:                                  # every pool column is used by some row, the rest drawn at random
        take = [uncovered.pop() for _ in range(min(ln, len(uncovered)))]
        rest = np.setdiff1d(np.arange(want), take)
        more = rng.choice(rest, size=ln - len(take), replace=False) if ln > len(take) else []
        rows.append(np.sort(pool[np.concatenate([take, more]).astype(np.int64)]))
    return rows


def boundaries(seed, dtype, p=100_003):
    """Every ub of BOUNDARY_UBS built three ways (1 x ub: one A entry times one B row of ub entries; ub x 1: ub A entries
    times B rows of one entry; square: about sqrt(ub) A entries times B rows of about sqrt(ub)), each with the column
    shapes it admits (a single B row has distinct columns only), between empty rows, in shuffled order."""
    rng = np.random.default_rng(seed)
    bld = _Build()
    for ub in BOUNDARY_UBS:
        side = max(1, int(round(ub ** 0.5)))
        for way, lens in (("1xub", [ub]), ("ubx1", [1] * ub), ("square", _split(ub, side))):
            for shape in ("distinct", "one", "half"):
                if way == "1xub" and shape != "distinct":
                    continue
                cols = _columns_for(rng, lens, shape, p)
                bld.row(cols, kind="boundary", way=way, shape=shape, want_ub=ub)
                bld.empty()
    return bld.finish(rng, dtype, p)


# ---- b. order witnesses ----------------------------------------------------------------------------------------
# tier -> (blen of the three-term witness, options that send it there)
WITNESS = {
    "g16": (20, {}),
    "g32": (80, {}),
    "wave": (300, {}),
    "block4k": (600, {}),
    "block8k": (1300, {"spgemm_route": 1}),
    "large": (300, {"spgemm_route": 2}),
}


def order_witness(tier, dtype, seed=0):
    """Rows of A that all land in `tier` (one empty row among them).

    Row "three": [1e16, -1e16, 1] at three consecutive k whose B rows hold `blen` columns each and 1.0 at the witness
    column j; C[., j] = ((1e16 - 1e16) + 1) = 1 in k order only.  j sits at index 1, blen / 2 and blen - 2 of the three
    B rows (another lane each time, another step where a B row is longer than the group); in the sorted product stream
    of the large tier its run of 3 starts at offset 255 of a 256-entry chunk.
    Row "many": K = ub / 2 entries of A times B rows of two columns, the witness column w and a neighbour below or
    above it (w is at index 0 or 1), all valued by order_sensitive_values: C[., w] is a sum of K products.
    Rows "dense": 32 entries of A (16 in g16) times B rows that share ub / 32 - 1 columns behind 0, 1 or 2 columns of
    their own (so a shared column moves by a lane from k to k): every shared entry of C is a sum of 32 order-sensitive
    products; ub = the tier's largest - 1."""
    blen, _ = WITNESS[tier]
    rng = np.random.default_rng(1000 + blen + seed)
    bld = _Build()
    j = blen + 8
    idx = [1, blen // 2, blen - 2]
    if tier == "large":
        idx[1] += (CHUNK - 1 - sum(idx)) % CHUNK             # the run of j starts at offset 255 of a chunk
        assert idx[1] < blen - 1
    rows, vals = [], []
    for r in range(3):
        lo = j - idx[r] - 4 + np.sort(rng.choice(idx[r] + 4, size=idx[r], replace=False))
        up = blen - 1 - idx[r]
        hi = j + 1 + np.sort(rng.choice(up + 4, size=up, replace=False))
        cols = np.concatenate([lo, [j], hi])
        v = rng.uniform(-1, 1, cols.size)
        v[idx[r]] = 1.0
        rows.append(cols)
        vals.append(v)
    bld.row(rows, avals=[1e16, -1e16, 1.0], bvals=vals, kind="three", witness=j, index_in_b_row=list(idx))
    top = TIER_UB[tier] if tier != "large" else 2200
    K = top // 2
    w = 2 * blen + 16 + 2 * K
    rows = []
    for t in range(K):
        other = w - 1 - t if t % 3 else w + 1 + t            # below w (w at index 1) or above it (w at index 0)
        rows.append(np.sort(np.array([w, other])))
    bld.row(rows, kind="many", witness=w, terms=K)
    bld.empty()
    terms = 32 if top >= 256 else 16
    shared_n = top // terms - 1
    base = w + K + 8
    for d in range(-(-5 * blen // shared_n)):
        shared = base + 128 + np.sort(rng.choice(2 * shared_n, size=shared_n, replace=False))
        rows = [np.concatenate([base + 3 * t + np.arange(t % 3), shared]) for t in range(terms)]
        bld.row(rows, kind="dense", shared=shared, terms=terms)
    return bld.finish(rng, dtype, base + 128 + 2 * shared_n + 8, shuffle=False)


# ---- c. hash worst cases ---------------------------------------------------------------------------------------
HASH_NCOLS = 1 << 20


def _home_slots(bits, ncols=HASH_NCOLS):
    return slot_of(np.arange(ncols, dtype=np.uint64), bits)


def top_slot_columns(tier, count, ncols=HASH_NCOLS):
    """`count` columns below ncols whose home slots all lie in the top min(64, TS / 8) slots of the tier's table"""
    _, ts, _ = GEOMETRY[tier]
    home = _home_slots(table_bits(tier), ncols)
    cols = np.nonzero(home >= ts - min(64, ts // 8))[0]
    assert cols.size >= count, (tier, cols.size)
    return cols[np.linspace(0, cols.size - 1, count).astype(np.int64)]


def same_slot_columns(tier, count, ncols=HASH_NCOLS):
    """`count` columns whose home slot is the table's last one"""
    _, ts, _ = GEOMETRY[tier]
    cols = np.nonzero(_home_slots(table_bits(tier), ncols) == ts - 1)[0]
    assert cols.size >= count, (tier, cols.size)
    return cols[np.linspace(0, cols.size - 1, count).astype(np.int64)]


def _overlapping_rows(keys):
    """four B rows over `keys` (in the order given), every key in exactly two of them: r_t = chunk t + chunk t+1"""
    chunks = np.array_split(np.asarray(keys), 4)
    return [np.sort(np.concatenate([chunks[t], chunks[(t + 1) % 4]])) for t in range(4)]


def hash_worst(dtype, seed=0, ncols=HASH_NCOLS, tiers=LDS_TIERS):
    """Per LDS tier (ub = TS / 2 in every row, so the row stays in its tier and the table ends half full or less):
    * "top": one B row of ub distinct columns homed in the table's top slots -- the chains wrap and grow to ~ub slots;
      one of the columns is ncols - 1 (it replaces a key: its own home slot is wherever the hash puts it);
    * "top_asc" / "top_adv": ub / 2 such keys through four B rows, every key in two of them (claimed at one step, added
      at a later one), dealt to the rows in ascending column order / in descending (home slot, column) order;
    * g16, g32 only: "same", "same_asc", "same_adv": the same with keys that all share the home slot TS - 1."""
    rng = np.random.default_rng(2000 + seed)
    bld = _Build()
    for tier in tiers:
        ub = TIER_UB[tier]
        bits = table_bits(tier)
        sets = [("top", top_slot_columns(tier, ub, min(ncols, HASH_NCOLS)))]
        if tier in ("g16", "g32"):
            sets.append(("same", same_slot_columns(tier, ub, min(ncols, HASH_NCOLS))))
        for name, keys in sets:
            full = keys.copy()
            if ncols - 1 not in full:
                full[-1] = ncols - 1
            full = np.sort(full)
            bld.row([full], kind=name, tier=tier, keys=full, last_column=True)
            half = np.sort(keys[::2])
            adv = half[np.lexsort((-half, -slot_of(half, bits)))]        # (descending home slot, then column)
            bld.row(_overlapping_rows(half), kind=name + "_asc", tier=tier, keys=half)
            bld.row(_overlapping_rows(adv), kind=name + "_adv", tier=tier, keys=adv)
            bld.empty()
    return bld.finish(rng, dtype, ncols)


# ---- d. run shapes of the large tier ---------------------------------------------------------------------------
# sorted product stream of a row as run lengths (1 = a column with one product)
RUN_ROWS = {
    "run2_at0": [2] + [1] * 2200,
    "run255_at63": [1] * 63 + [255] + [1] * 2000,
    "run256_at64": [1] * 64 + [256] + [1] * 2000,
    "run257_at255": [1] * 255 + [257] + [1] * 2048,
    "run1025_at255": [1] * 255 + [1025] + [1] * 1024 + [2],
    "run5000_mid": [1] * 300 + [5000] + [1] * 211 + [3],
    "len_256k": [1] * (CHUNK * 9),
    "len_256k_minus1": [1] * (CHUNK * 9 - 1),
    "len_256k_plus1": [1] * (CHUNK * 9 + 1),
    "whole_row_run": [2560],
    "whole_row_run_odd": [2303],
    "mixed": [3, 1, 1, 64, 1, 190, 2, 255, 1, 256, 1, 257, 1, 1025] + [1] * 100,
}


def run_heads(runs):
    """offset of every run's head in the row's sorted stream"""
    return np.concatenate([[0], np.cumsum(runs)[:-1]])


def _rows_for_runs(cols, runs):
    """B rows t = 0 .. max(runs) - 1: row t holds every column whose run is longer than t (so column c gets runs[c]
    products, one per k, and the stream sorted by column has exactly these runs)"""
    cols, runs = np.asarray(cols), np.asarray(runs)
    return [cols[runs > t] for t in range(int(runs.max()))]


def large_runs(dtype, p, seed=0):
    """Rows whose sorted product stream has the runs of RUN_ROWS, between short rows for the LDS tiers and empty rows.
    p = 1: every B row holds column 0 at most, so every row is ONE run (its length = the sum of the runs above)."""
    rng = np.random.default_rng(3000 + seed + p % 7)
    bld = _Build()
    for name, runs in sorted(RUN_ROWS.items()):
        if p == 1:
            total = int(np.sum(runs))
            bld.row([np.zeros(1, dtype=np.int64)] * total, kind="runs", name=name, runs=[total])
        else:
            cols = np.sort(rng.choice(p - 1, size=len(runs), replace=False))
            if name == "mixed":
                cols[-1] = p - 1
            bld.row(_rows_for_runs(cols, runs), kind="runs", name=name, runs=list(runs))
        for ln in (1, 7, 40):                          # LDS-tier company (ub <= 48)
            width = min(ln, p)
            bld.row([np.sort(rng.choice(p, size=width, replace=False))] * (ln // width), kind="short")
        bld.empty()
    return bld.finish(rng, dtype, p)


# ---- h. fuzz ---------------------------------------------------------------------------------------------------
def _lengths(rng, law, count, hi):
    hi = max(int(hi), 1)
    if law == "constant":
        ln = np.full(count, hi)
    elif law == "uniform":
        ln = rng.integers(hi // 2, hi + 1, count)
    elif law == "pareto":
        ln = np.minimum((rng.pareto(1.2, count) * 3 + 1).astype(np.int64), hi)
    elif law == "two_regions":
        ln = np.where(np.arange(count) < count // 2, rng.integers(1, 4, count), rng.integers(hi // 2, hi + 1, count))
    else:                                              # stretches of empty rows
        ln = rng.integers(hi // 2 + 1, hi + 1, count)
        for _ in range(3):
            s = rng.integers(0, count)
            ln[s:s + max(1, count // 6)] = 0
    return np.asarray(ln, dtype=np.int64)


LAWS = ("constant", "uniform", "pareto", "two_regions", "empty_stretches")
FUZZ_SHAPES = ("general", "m1", "n1", "p1", "p2^20")
# (route, lds_cap) and the longest rows of (A, B), dealt by seed so that the default 16 seeds visit every tier
FUZZ_OPTIONS = ((0, 0), (1, 0), (2, 0), (0, 48), (0, 4096), (1, 63), (0, 300), (0, 1))
FUZZ_SIZES = ((64, 1), (64, 4), (64, 16), (64, 32), (90, 45), (48, 40), (80, 3))
BLOCK = 32                             # B's rows come in blocks of 32: even blocks share a column window


def fuzz(seed, dtype=None, fmt=None):
    """One fuzz draw: shapes (m = 1, n = 1, p = 1 and p = 2^20 among them), row-length laws for A and B, values from
    order_sensitive_values with a few +-0, +-inf, NaN and subnormals, dtype, format, route and cap.

    So that a wrong order shows, most entries of C that have several products must have many (a sum of two is the same
    in either order): the rows of every even block of 32 rows of B draw their columns from one window a quarter wider
    than the block's longest row, the rows of odd blocks from all p columns; a row of A with 8 entries or more takes its
    k from neighbouring window rows, a shorter one from the scattered rows.  Returns (case, dtype, fmt, options)."""
    rng = np.random.default_rng(7000 + seed)
    shape = FUZZ_SHAPES[seed % len(FUZZ_SHAPES)]
    route, cap = FUZZ_OPTIONS[seed % len(FUZZ_OPTIONS)]
    big_a, big_b = FUZZ_SIZES[seed % len(FUZZ_SIZES)]
    law_a, law_b = LAWS[rng.integers(len(LAWS))], LAWS[rng.integers(len(LAWS))]
    if big_a * big_b > DEFAULT_CAP:                    # (the block8k draw: every row of the same, full length)
        law_a = law_b = "constant"
    dt = np.dtype(dtype) if dtype is not None else np.dtype((np.float64, np.float32)[(seed // 2) % 2])
    fm = fmt if fmt is not None else ("csr", "csc")[(seed // 3) % 2]
    m = 1 if shape == "m1" else int(rng.integers(30, 300))
    n = 1 if shape == "n1" else int(rng.integers(100, 500))
    p = {"p1": 1, "p2^20": 1 << 20}.get(shape, int(rng.integers(3000, 60000)))
    la = np.minimum(_lengths(rng, law_a, m, big_a), n)
    lb = np.minimum(_lengths(rng, law_b, n, big_b), p)
    if shape == "m1":
        la[:] = min(n, big_a)
    block = np.arange(n) // BLOCK
    window_row = (block % 2 == 0) | (n < 2 * BLOCK)
    brows = []
    for g in range(int(block[-1]) + 1):
        ks = np.nonzero(block == g)[0]
        width = min(p, int(lb[ks].max()) * 5 // 4 + 1)
        c0 = p - width if g % 4 == 0 else int(rng.integers(0, p - width + 1))      # (column p - 1 is in reach)
        for k in ks:
            if window_row[k]:
                brows.append(c0 + np.sort(rng.choice(width, size=int(lb[k]), replace=False)))
            else:
                brows.append(np.sort(rng.choice(p, size=int(lb[k]), replace=False)))
    win, sca = np.nonzero(window_row)[0], np.nonzero(~window_row)[0]
    if sca.size == 0:
        sca = win
    arows = []
    for i in range(m):
        pool = win if la[i] >= 8 else sca
        ln = min(int(la[i]), pool.size)
        la[i] = ln
        span = min(pool.size, ln * 5 // 4 + 1)
        s0 = int(rng.integers(0, pool.size - span + 1))
        arows.append(np.sort(pool[s0 + rng.choice(span, size=ln, replace=False)]))
    ap = np.concatenate([[0], np.cumsum(la)]).astype(np.uint64)
    bp = np.concatenate([[0], np.cumsum(lb)]).astype(np.uint64)
    ac = np.concatenate(arows).astype(np.uint64)
    bc = np.concatenate(brows).astype(np.uint64)
    av, bv = order_sensitive_values(rng, ac.size, dt), order_sensitive_values(rng, bc.size, dt)
    tiny = np.finfo(dt).smallest_subnormal
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -3 * tiny, np.finfo(dt).tiny / 2], dtype=dt)
    for arr in (av, bv):
        if arr.size >= 256:
            idx = rng.choice(arr.size, size=8, replace=False)
            arr[idx] = special
    case = Case(m, n, p, (ap, ac, av), (bp, bc, bv), None)
    return case, dt, fm, {"spgemm_route": route, "spgemm_lds_cap": cap}


# ---- CPU folds in other orders (the inputs' order sensitivity) -------------------------------------------------
def products_by_entry(a, b):
    """every product of A * B as (row, column, value), sorted by (row, column) with k ascending inside an entry"""
    arp, aci, av = np.asarray(a[0], dtype=np.int64), np.asarray(a[1], dtype=np.int64), np.asarray(a[2])
    brp, bci, bv = np.asarray(b[0], dtype=np.int64), np.asarray(b[1], dtype=np.int64), np.asarray(b[2])
    arow = np.repeat(np.arange(arp.size - 1), np.diff(arp))
    blen = (brp[1:] - brp[:-1])[aci]
    src = np.repeat(np.arange(aci.size), blen)                       # the A entry of every product
    start = np.concatenate([[0], np.cumsum(blen)])[:-1]
    q = brp[aci][src] + (np.arange(src.size) - start[src])           # the B entry
    with np.errstate(all="ignore"):
        val = av[src] * bv[q]
    row, col = arow[src], bci[q]
    order = np.lexsort((np.arange(src.size), col, row))              # (stable: k ascending inside an entry)
    return row[order], col[order], val[order]


def _folds(v, ln):
    """rows of `v` (padded; `ln` terms each) folded left to right, right to left and pairwise (neighbours first)"""
    width = v.shape[1]
    rows = np.arange(v.shape[0])
    fwd, bwd = v[:, 0].copy(), v[rows, ln - 1].copy()
    for t in range(1, width):
        live = t < ln
        fwd = np.where(live, fwd + v[:, t], fwd)
        bwd = np.where(live, bwd + v[rows, np.maximum(ln - 1 - t, 0)], bwd)
    cur, n = v, ln.copy()
    while cur.shape[1] > 1:
        if cur.shape[1] % 2:
            cur = np.concatenate([cur, np.zeros((cur.shape[0], 1), dtype=cur.dtype)], axis=1)
        left, right = cur[:, 0::2], cur[:, 1::2]
        has_right = (2 * np.arange(left.shape[1]) + 1)[None, :] < n[:, None]
        cur = np.where(has_right, left + right, left)
        n = (n + 1) // 2
    return fwd, bwd, cur[:, 0]


def reorder_sensitivity(a, b):
    """Of the entries of C with two or more products (NaN results aside): how many there are, and the share whose value
    changes bits when the products are folded in descending k / pairwise (neighbours first, as a tree)."""
    row, col, val = products_by_entry(a, b)
    head = np.ones(row.size, dtype=bool)
    head[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
    starts = np.nonzero(head)[0]
    lens = np.diff(np.concatenate([starts, [row.size]]))
    bits = np.uint64 if val.dtype == np.float64 else np.uint32
    n = desc = pair = 0
    with np.errstate(all="ignore"):
        width = 2
        while lens.size and width < 2 * int(lens.max()):
            pick = (lens > max(width // 2, 1)) & (lens <= width)
            if pick.any():
                st, ln = starts[pick], lens[pick]
                idx = st[:, None] + np.minimum(np.arange(width)[None, :], ln[:, None] - 1)
                fwd, bwd, tree = _folds(val[idx], ln)
                ok = ~np.isnan(fwd)
                n += int(ok.sum())
                desc += int((fwd.view(bits) != bwd.view(bits))[ok].sum())
                pair += int((fwd.view(bits) != tree.view(bits))[ok].sum())
            width *= 2
    return n, desc, pair
