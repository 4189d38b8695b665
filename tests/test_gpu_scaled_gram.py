"""The rescaled Gram (schedule knob "scaled_gram", host_objective.cpp ScaledGram): a batched fit
keeps each output's first Gram of the call and serves the evaluation that differs from it only in
sv_o -- the fifth, the sv_o vertex of the initial simplex -- as G' = c^2 G, r' = c r instead of a
whitening and a Gram.  Every check compares scaled_gram 1 against 0: the same fit to rounding (theta
and nlml at rtol 1e-9, the bound tests/test_gpu_headline.py puts on two schedules of one fit), one
Gram and one whitening fewer per output, and bit for bit the serialized twin."""
import functools

import numpy as np
import pytest

from oracle import gpar_oracle as O

pytestmark = pytest.mark.gpu
G = pytest.importorskip("gparatscale")

X0 = np.array([0.0, 0.0, 0.5, 0.0, -1.5])


@functools.lru_cache(maxsize=None)
def _series(n):
    return O.synthetic_gpar(n, 28, seed=71, noise=0.3)


def _batch(n=2000, m=96, dims=(3, 20, 3, 20), out_kernel="matern52", kuu_noise=True):
    """Outputs with D = 3 (fused whitening) and D = 20 (cached distances) on one time grid."""
    t, Y = _series(n)
    probs, keep = [], []
    for i, d in enumerate(dims):
        V = np.ascontiguousarray(Y[:, :d].T)
        Z = O.pick_pseudo_inputs(V, m, 400 + i)
        pr, k = G.make_problem(V, Z, t, Y[:, 20 + i], out_kernel, "matern52", kuu_noise=kuu_noise)
        probs.append(pr)
        keep.append(k)
    return probs, keep


def _fit(probs, x0, max_evals, knobs=None, split=None, stats=False):
    """One gpar_fit under the knobs; with stats also the (gram, whiten) launch counts."""
    ctx = G.context(0)
    knobs = dict(knobs or {})
    old = {k: ctx.schedule(k) for k in knobs}
    try:
        for k, v in knobs.items():
            ctx.set_schedule(k, v)
        if split is not None:
            ctx.set_cu_split(split)
        if stats:
            ctx.set_profiling(True)
            ctx.reset_stats()
        fit = G.fit_batch(probs, x0, max_evals=max_evals, g_tol=-1.0)
        counts = (ctx.kernel_stats("gram")[0], ctx.kernel_stats("whiten")[0]) if stats else None
    finally:
        if stats:
            ctx.set_profiling(False)
        if split is not None:
            ctx.set_cu_split(-1)
        for k, v in old.items():
            ctx.set_schedule(k, v)
    return fit, counts


def _same_fit(a, b):
    print("theta max rel", np.abs(a.theta / b.theta - 1).max(), "nlml", a.nlml, b.nlml)
    np.testing.assert_array_equal(a.evals, b.evals)
    np.testing.assert_allclose(a.theta, b.theta, rtol=1e-9)
    np.testing.assert_allclose(a.nlml, b.nlml, rtol=1e-9)


def _bitwise(a, b):
    np.testing.assert_array_equal(a.theta, b.theta)
    np.testing.assert_array_equal(a.nlml, b.nlml)
    np.testing.assert_array_equal(a.evals, b.evals)


def test_scaled_gram_same_fit_fewer_launches_and_serialized_twin():
    probs, keep = _batch()
    x0 = np.tile(X0, (len(probs), 1))
    per_output = {"gram_group": 0}              # one timed Gram per output, not per group
    on, c_on = _fit(probs, x0, 12, {**per_output, "scaled_gram": 1}, stats=True)
    off, c_off = _fit(probs, x0, 12, {**per_output, "scaled_gram": 0}, stats=True)
    _same_fit(on, off)
    assert np.all(on.evals >= 5)
    assert c_off[0] - c_on[0] == len(probs), (c_on, c_off)      # Gram launches
    assert c_off[1] - c_on[1] == len(probs), (c_on, c_off)      # whitenings
    twin, _ = _fit(probs, x0, 12, {**per_output, "scaled_gram": 1, "serialize": 1})
    _bitwise(on, twin)


def test_scaled_gram_each_output_its_own_slot():
    probs, keep = _batch()
    rng = np.random.default_rng(5)
    x0 = X0 + rng.uniform(-0.3, 0.3, size=(len(probs), 5))
    on, _ = _fit(probs, x0, 12, {"scaled_gram": 1})
    off, _ = _fit(probs, x0, 12, {"scaled_gram": 0})
    _same_fit(on, off)


def test_scaled_gram_after_a_failed_first_evaluation():
    """The first evaluation's Cholesky fails by its parameters (EQ pseudo-inputs at a length scale
    of e^5 without Kuu noise: Kuu is numerically singular); its Gram is still the reference."""
    probs, keep = _batch(out_kernel="eq", kuu_noise=False)
    x0 = np.tile(np.array([0.0, 0.0, 5.0, 0.0, -1.5]), (len(probs), 1))
    theta0 = np.exp(x0) + 1e-3
    with pytest.raises(G.PosDefException):
        G.dtc_objective_batch(probs, theta0)
    on, _ = _fit(probs, x0, 12, {"scaled_gram": 1})
    off, _ = _fit(probs, x0, 12, {"scaled_gram": 0})
    np.testing.assert_array_equal(on.evals, off.evals)
    np.testing.assert_allclose(on.theta, off.theta, rtol=1e-9)
    np.testing.assert_allclose(on.nlml, off.nlml, rtol=1e-9)


def test_scaled_gram_budget_ends_before_the_fifth_evaluation():
    probs, keep = _batch()
    x0 = np.tile(X0, (len(probs), 1))
    on, c_on = _fit(probs, x0, 4, {"gram_group": 0, "scaled_gram": 1}, stats=True)
    off, c_off = _fit(probs, x0, 4, {"gram_group": 0, "scaled_gram": 0}, stats=True)
    _bitwise(on, off)
    assert c_on == c_off


@pytest.mark.parametrize("split", [None, 8], ids=["unsplit", "split"])
def test_scaled_gram_in_the_round_overlap(split):
    """8 outputs in two groups of 4: the unsplit round overlap (eval_dtc per group) and, on the
    forced CU split, fit_overlapped's pipeline."""
    probs, keep = _batch(dims=(3, 20, 3, 20, 20, 3, 20, 3))
    x0 = np.tile(X0, (len(probs), 1))
    knobs = {"overlap": 1, "overlap_group": 4}
    on, c_on = _fit(probs, x0, 12, {**knobs, "scaled_gram": 1}, split=split, stats=True)
    off, c_off = _fit(probs, x0, 12, {**knobs, "scaled_gram": 0}, split=split, stats=True)
    _same_fit(on, off)
    assert c_off[1] - c_on[1] == len(probs), (c_on, c_off)
    twin, _ = _fit(probs, x0, 12, {**knobs, "scaled_gram": 1, "serialize": 1}, split=split)
    _bitwise(on, twin)


def test_scaled_gram_with_the_grouped_gram():
    probs, keep = _batch(n=4000, m=64)          # the dtc-like shape: one grouped Gram per round
    x0 = np.tile(X0, (len(probs), 1))
    on, c_on = _fit(probs, x0, 12, {"scaled_gram": 1}, stats=True)
    off, c_off = _fit(probs, x0, 12, {"scaled_gram": 0}, stats=True)
    _same_fit(on, off)
    assert c_off[0] - c_on[0] == 1, (c_on, c_off)               # one grouped Gram launch set
    assert c_off[1] - c_on[1] == len(probs), (c_on, c_off)
