"""Seeded fuzz of eigsh near sigma against its text (tests/near_ref.py), bit for bit: random symmetric graphs from the
generators of tests/eigsh_cases.py with n on both sides of 256 and 1024, sigma drawn uniformly inside Gershgorin's interval,
degree in {2, 5, 16, 48}, k in 1 .. 4, ncv in k + 2 .. 24, maxit <= 6, both dtypes and both handle kinds.

THE CAP: at most a quarter of the seeds may end with stop 2 or 3 (values that are not finite, a space exhausted below k):
such a seed compares little.  test_the_text_alone_stays_within_the_cap proves it for SEEDS on the CPU, with the text
alone."""
import functools

import numpy as np
import pytest

from tests import eigsh_cases as ec
from tests import near_ref as nr
from tests import cheb_ref as cr
from tests import trsv_ref as tr
from tests.test_eigsh_host import lib_jacobi

SEEDS = tuple(range(20))
BASE_SEED = 20283000
N_TABLE = (9, 255, 256, 257, 1023, 1024, 1025, 300)
DEGREES = (2, 5, 16, 48)
CAP = len(SEEDS) // 4


@functools.lru_cache(maxsize=None)
def case(seed):
    """(mat, knobs) of one seed; built once per process, shared, read-only"""
    rng = np.random.default_rng(BASE_SEED + seed)
    n = N_TABLE[seed % len(N_TABLE)]
    dtype = np.dtype((np.float64, np.float32)[(seed // 2) % 2])
    cls = ec.CLASSES[(seed + seed // 5) % len(ec.CLASSES)]
    pattern = ec._pattern(rng, n, seed)
    values = ec._values(rng, pattern, dtype, cls)
    mat = ec.readonly((*pattern, values))
    glo, ghi = cr.gershgorin(*mat[1:])
    k = 1 + int(rng.integers(4))
    ncv = min(int(rng.integers(k + 2, 25)), n)
    knobs = dict(n=n, cls=cls, dtype=dtype, kind=("csr", "csc")[(seed + seed // 3) % 2], k=k, ncv=ncv,
                 sigma=float(rng.uniform(glo, ghi)), degree=DEGREES[int(rng.integers(len(DEGREES)))],
                 tol=(0.0, ec.TOL[dtype], 1e-2)[int(rng.integers(3))], maxit=int(rng.integers(7)),
                 v0=rng.uniform(-1, 1, size=n).astype(dtype) if rng.random() < 0.4 else None,
                 seed=ec.SEEDS[int(rng.integers(len(ec.SEEDS)))], rotate=int(rng.integers(3)), chunk=(0, 256, 1024)[int(rng.integers(3))],
                 form=int(rng.integers(3)))
    return mat, knobs


@functools.lru_cache(maxsize=None)
def text(seed):
    mat, k = case(seed)
    return nr.eigsh_near(mat[1:], k["dtype"].type, k["k"], k["sigma"], k["ncv"], k["tol"], k["maxit"], k["degree"], None, k["v0"],
                         k["seed"], lib_jacobi)


def test_the_text_alone_stays_within_the_cap():
    """No GPU: the text on every seed.  Also what the seeds reach: sizes on both sides of 256 and 1024, every degree,
    both dtypes and kinds, restarts, and no refusal (sigma is strictly inside Gershgorin's interval, which the automatic
    interval contains)."""
    runs = [(case(s)[1], text(s)) for s in SEEDS]
    assert all(isinstance(r, dict) for _, r in runs)
    reasons = [r["reason"] for _, r in runs]
    print("reasons", reasons, "restarts", [r["restarts"] for _, r in runs])
    assert sum(x in (2, 3) for x in reasons) <= CAP
    assert {k["n"] for k, _ in runs} >= {255, 257, 1023, 1025}
    assert {k["degree"] for k, _ in runs} == set(DEGREES)
    assert {k["dtype"] for k, _ in runs} == {np.dtype(np.float64), np.dtype(np.float32)} and {k["kind"] for k, _ in runs} == {"csr", "csc"}
    assert max(r["restarts"] for _, r in runs) >= 2 and all(1 <= k["k"] <= 4 and k["k"] + 2 <= k["ncv"] <= 24 for k, _ in runs)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_the_device_is_the_text(seed):
    from tests.test_gpu_cheb import make
    mat, k = case(seed)
    ref = text(seed)
    a = make(k["kind"], mat)
    dev = a.device()
    dev.set_option("eigsh_rotate", k["rotate"])
    dev.set_option("cheb_chunk", k["chunk"])
    dev.set_option("cheb_series_form", k["form"])
    theta, X, info = a.eigsh(k["k"], "LA", k["ncv"], k["v0"], k["seed"], k["tol"], k["maxit"], sigma=k["sigma"], filter_degree=k["degree"])
    assert (info.restarts, info.products, info.converged, info.reason) == (ref["restarts"], ref["products"], ref["converged"], ref["reason"])
    assert (info.lo, info.hi, info.gamma) == (ref["lo"], ref["hi"], ref["gamma"])
    tr.assert_same_bits(theta, ref["theta"])
    tr.assert_same_bits(info.resid, ref["resid"])
    tr.assert_same_bits(X, ref["X"])
