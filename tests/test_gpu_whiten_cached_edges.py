"""The cached whitening (whiten_kfu_d2x2, k_dist.hip) at its edges, through gpar_fit with the
distance cache engaged (D >= 17): chunk tails that are and are not a multiple of the kernel's
8-row blocks, padding columns, lanes past the last column, a second column block, every time and
output kernel (the r cache of the Matern kernels, the d^2 cache of EQ) and compact gains records.

Each case fits for 3 evaluations and compares the returned -nlml with gpar_dtc_objective of the same
problem at the returned theta, which never reads the cache (the fused whitening, D <= 64).  Both
build the centred Gram-form distances in a different summation order, so they agree to rounding:
rel 1e-12, the bound tests/test_gpu_dist_cache.py puts on the cached against the uncached fit."""
import functools

import numpy as np
import pytest

from oracle import gpar_oracle as O

pytestmark = pytest.mark.gpu
G = pytest.importorskip("gparatscale")

X0 = np.array([0.0, 0.0, 0.5, 0.0, -1.5])
D = 17
NMAX = 1000


@functools.lru_cache(maxsize=None)
def _series():
    return O.synthetic_gpar(NMAX, D + 2, seed=61, noise=0.3)


@functools.lru_cache(maxsize=None)
def _data(n, m, d=D):
    """The first n steps of the series; the pseudo-inputs are drawn from all NMAX rows (m > n)."""
    t, Y = _series()
    Vall = np.ascontiguousarray(Y[:, :d].T)
    Z = O.pick_pseudo_inputs(Vall, m, 300 + m + d)
    return np.ascontiguousarray(t[:n]), np.ascontiguousarray(Vall[:, :n]), Z, np.ascontiguousarray(Y[:n, d])


def _check(n, m, out_kernel, time_kernel):
    t, V, Z, y = _data(n, m)
    pr, keep = G.make_problem(V, Z, t, y, out_kernel, time_kernel)
    ctx = G.context(0)
    fit = G.fit_batch([pr], X0[None, :], max_evals=3, g_tol=-1.0)
    assert ctx.dist_cache_stats()[0] == 1            # the fit whitened from the cache
    ref = G.compute_gpar_dtc_objective(V, Z, t, y, fit.theta[0], out_kernel, time_kernel)
    got = -fit.nlml[0]
    print(f"n={n} m={m} {out_kernel}/{time_kernel}: fit {got!r} objective {ref!r} "
          f"rel {abs(got - ref) / abs(ref):.2e}")
    assert np.isfinite(got)
    np.testing.assert_allclose(got, ref, rtol=1e-12)


# N: 3 full chunks + 232 rows (a multiple of 8) / a last block of 773 - 768 = 5 rows / one chunk
# M: Mp = 128 with padding columns and idle lanes / no padding / Mp = 640, a second column block
@pytest.mark.parametrize("m", [100, 128, 600])
@pytest.mark.parametrize("n", [1000, 773, 256])
def test_cached_whitening_shapes(n, m):
    _check(n, m, "matern52", "matern52")


@pytest.mark.parametrize("time_kernel", ["matern12", "matern32", "matern52"])
@pytest.mark.parametrize("out_kernel", ["matern12", "matern32", "matern52", "eq"])
def test_cached_whitening_kernels(out_kernel, time_kernel):
    _check(773, 100, out_kernel, time_kernel)


def test_cached_whitening_compact_records():
    """compact_rec = 1 on the forced CU split: the whitening recomputes each step's transition from
    t (the CR instantiation), two outputs on one grid."""
    n, m = 773, 100
    probs, keep, data = [], [], []
    for d in (D, D + 1):
        t, V, Z, y = _data(n, m, d)
        pr, k = G.make_problem(V, Z, _data(n, m, D)[0], y, "matern52", "matern52")
        probs.append(pr)
        keep.append(k)
        data.append((V, Z, y))
    t = _data(n, m, D)[0]
    ctx = G.context(0)
    try:
        ctx.set_cu_split(8)
        ctx.set_schedule("compact_rec", 1)
        fit = G.fit_batch(probs, np.tile(X0, (2, 1)), max_evals=3, g_tol=-1.0)
        assert ctx.dist_cache_stats()[0] == 2
    finally:
        ctx.set_schedule("compact_rec", -1)
        ctx.set_cu_split(-1)
    for i, (V, Z, y) in enumerate(data):
        ref = G.compute_gpar_dtc_objective(V, Z, t, y, fit.theta[i], "matern52", "matern52")
        got = -fit.nlml[i]
        print(f"compact_rec output {i}: fit {got!r} objective {ref!r} rel {abs(got - ref) / abs(ref):.2e}")
        np.testing.assert_allclose(got, ref, rtol=1e-12)
