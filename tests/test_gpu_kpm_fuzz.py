"""Random small symmetric patterns through the KPM moments against the text (tests/kpm_ref.py), seeded: n <= 3000,
k <= 12, degree <= 12, random column tile, chunk, form, seed, leading dimension and interval; CSR and CSC, f32 and f64.
Bits, not tolerances."""
import numpy as np
import pytest

import spalinalg_amd as sp
from tests import kpm_ref as K
from tests import trsv_ref as tr
from tests.test_gpu_cheb import make

pytestmark = pytest.mark.gpu

CASES = 120                                    # per element type


def symmetric_pattern(rng, n, dtype):
    """a random symmetric matrix with |row sums| <= 1: a few off-diagonal pairs per row, some rows empty, one long row"""
    per_row = int(rng.integers(0, 5))
    r = rng.integers(0, n, size=per_row * n)
    c = rng.integers(0, n, size=per_row * n)
    if n > 200 and rng.random() < 0.3:          # a long row (and column)
        hub = int(rng.integers(0, n))
        far = rng.choice(n, size=int(rng.integers(100, min(n, 1500))), replace=False)
        r, c = np.concatenate([r, np.full(far.size, hub)]), np.concatenate([c, far])
    keep = rng.random(r.size) < 0.8
    r, c = r[keep], c[keep]
    empty = rng.choice(n, size=n // 10, replace=False)
    keep = ~np.isin(r, empty) & ~np.isin(c, empty)
    r, c = r[keep], c[keep]
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    pairs = np.unique(np.stack([lo, hi], axis=1), axis=0) if r.size else np.zeros((0, 2), dtype=np.int64)
    v = rng.uniform(-1, 1, pairs.shape[0])
    off = pairs[:, 0] != pairs[:, 1]
    rr = np.concatenate([pairs[:, 0], pairs[off, 1]])
    cc = np.concatenate([pairs[:, 1], pairs[off, 0]])
    vv = np.concatenate([v, v[off]])
    scale = np.bincount(rr, weights=np.abs(vv), minlength=n).max() if rr.size else 1.0
    return K.from_triplets(n, rr, cc, vv / max(scale, 1e-30), dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_random_symmetric_patterns_against_the_text(dtype):
    rng = np.random.default_rng(20240607 + np.dtype(dtype).itemsize)
    for case in range(CASES):
        n = int(rng.choice([rng.integers(1, 40), rng.integers(40, 400), rng.integers(900, 1200), rng.integers(1200, 3001)],
                           p=[0.3, 0.4, 0.2, 0.1]))
        k, degree, seed = int(rng.integers(1, 13)), int(rng.integers(1, 13)), int(rng.integers(0, 2**40))
        csr = symmetric_pattern(rng, n, dtype)
        kind = "csr" if case % 2 == 0 else "csc"
        a = make(kind, (n, *csr))
        dev = a.device()
        options = dict(cheb_chunk=int(rng.choice([0, 256, 512, 1024, 2048, 4096])), kpm_tile=int(rng.choice([0, 1, 2, 4, 8])),
                       kpm_form=int(rng.choice([0, 1, 2])))
        for key, value in options.items():
            dev.set_option(key, value)
        interval = (-1.0 - float(rng.random()), 1.0 + float(rng.random())) if rng.random() < 0.7 or csr[2].size == 0 else None
        what = f"case {case}: n = {n}, k = {k}, degree = {degree}, seed = {seed}, {kind}, {options}, interval = {interval}"
        if rng.random() < 0.5:                  # hashed probes
            Z = sp.kpm_probes(n, k, seed, dtype)
            mu, info = a.kpm_moments(degree, probes=k, seed=seed, interval=interval)
        else:                                   # a given block inside a wider one
            big = rng.uniform(-1, 1, (n, k + int(rng.integers(0, 4)))).astype(dtype)
            Z = big[:, :k]
            mu, info = a.kpm_moments(degree, interval=interval, Z=Z)
        ref = K.moments(csr, Z, degree, interval)
        try:
            tr.assert_same_bits(mu, ref)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None
        assert (info.products, info.probes, info.degree) == ((degree + 1) // 2, k, degree), what
