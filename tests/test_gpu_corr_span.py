"""The plan knob "corr_span" (include/gpar_hip.h): the batched fit's cached whitening
(whiten_kfu_d2x2) filters S consecutive 256-step chunks from one zero state, so the Gram's chunk
correction, the carry of beta's columns and vec_fix's E_j / q_j run over ceil(nch / S) spans.

Through gpar_fit on the forced CU split with D = 18..20 (the distance cache engaged, three outputs
on one grid: the split pipeline of eval_dtc).  A fit of 3 evaluations returns the best of three
known simplex points, so its -nlml is the objective at the returned theta:
  * every S against S = 1 and against the oracle at rel 1e-10, the bound the project puts on a plan
    (test_grouped_gram_is_a_plan_not_a_schedule, test_gpu_dtc.py);
  * S > 1 bit for bit its serialized twin;
  * S = 1 bit for bit the values the parent build returned for the same inputs
    (tests/golden/corr_span_parent.npz, recorded with the library of the commit before the knob);
  * a 12-evaluation fit reaches the same theta as S = 1 (rtol 1e-9, tests/test_gpu_scaled_gram.py).

At X0 the time scale is about 1 on a grid of step 1/30, so a chunk's closed-loop transition is
numerically zero and with it every Psi_i, i >= 1: those cases cannot see the re-basing of the
fix-up rows.  test_slow_decay_* runs the same comparisons at l_t about 200 with a large noise,
where the transition over a chunk is O(1) (asserted from the oracle's Riccati recursion), so a
wrong Psi shows at the first digits.

tests/golden/corr_span_parent.npz comes from tests/golden/make_corr_span_parent.py, run with
GPAR_HIP_LIB pointing at a library built from the commit before the knob.
"""
import functools
import os

import numpy as np
import pytest

from oracle import gpar_oracle as O

pytestmark = pytest.mark.gpu
G = pytest.importorskip("gparatscale")
from gparatscale import data as D  # noqa: E402

X0 = np.array([0.0, 0.0, 0.5, 0.0, -1.5])
# a slowly decaying closed loop: l_t = 200 (a 256-step chunk is 0.04 time scales), sigma = 3
X0_SLOW = np.array([np.log(200.0), 0.0, 0.5, 0.0, np.log(3.0)])
DIMS = (18, 19, 20)
SPANS = (1, 2, 4)
NMAX = 3200
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corr_span_parent.npz")


def size_of(kind, s):
    """The issue's sizes for span s: a partial last span with a partial last chunk / exactly one
    span / shorter than one span (s > 1) / one step into the second span."""
    return {"tail": 3 * s * 256 + 37, "exact": s * 256, "short": 300, "plus1": 256 * s + 1}[kind]


KINDS = ("tail", "exact", "short", "plus1")
# (kind, span the size is built for, M); M = 192 pads to Mp = 256: padding columns
CASES = [(k, s, 128) for s in SPANS for k in KINDS] + [("gaps", 0, 128), ("tail", 4, 192)]


@functools.lru_cache(maxsize=None)
def _series():
    return O.synthetic_gpar(NMAX, max(DIMS) + 1, seed=83, noise=0.3)


@functools.lru_cache(maxsize=None)
def _gaps():
    # 2100 grid points less two gaps of 150: N = 1800 (7 chunks + 8 steps), two long time steps
    ds = D.gpar_dataset(2100, max(DIMS) + 1, seed=5, observation_noise=0.8, gaps=2, gap_len=150)
    return ds["t"], ds["Y"]


@functools.lru_cache(maxsize=None)
def batch(kind, s, m, dims=DIMS):
    """(problems, keep-alive, [(V, Z, t, y)]) of the case: outputs with D = 18, 19, 20 on one grid."""
    if kind == "gaps":
        t, Y = _gaps()
    else:
        t, Y = _series()
    n = len(t) if kind == "gaps" else size_of(kind, s)
    tn = np.ascontiguousarray(t[:n])
    probs, keep, data = [], [], []
    for i, d in enumerate(dims):
        Vall = np.ascontiguousarray(Y[:, :d].T)
        Z = O.pick_pseudo_inputs(Vall, m, 500 + m + d)
        V = np.ascontiguousarray(Vall[:, :n])
        y = np.ascontiguousarray(Y[:n, d])
        pr, k = G.make_problem(V, Z, tn, y, "matern52", "matern52")
        probs.append(pr)
        keep.append(k)
        data.append((V, Z, tn, y))
    return probs, keep, data


def fit(probs, span=None, serialize=0, evals=3, overlap=None, dg_rows_w=None, x0=X0):
    """One gpar_fit on the forced CU split; span None leaves the knob alone (the run of
    tests/golden/make_corr_span_parent.py on a library from before the knob)."""
    ctx = G.context(0)
    try:
        ctx.set_cu_split(8)
        ctx.set_schedule("serialize", serialize)
        if span is not None:
            ctx.set_schedule("corr_span", span)
        if overlap is not None:
            ctx.set_schedule("overlap", overlap)
        if dg_rows_w is not None:
            ctx.set_schedule("dg_rows_w", dg_rows_w)
        fr = G.fit_batch(probs, np.tile(x0, (len(probs), 1)), max_evals=evals, g_tol=-1.0)
        assert ctx.dist_cache_stats()[0] == len(probs)   # every output whitened from the cache
    finally:
        ctx.set_schedule("overlap", 1)
        ctx.set_schedule("dg_rows_w", -100)
        ctx.set_schedule("serialize", 0)
        if span is not None:
            ctx.set_schedule("corr_span", -1)
        ctx.set_cu_split(-1)
    return fr


def golden_key(kind, s, m):
    return f"{kind}_{s}_{m}"


@functools.lru_cache(maxsize=None)
def _base(kind, s, m):
    """The case at corr_span = 1, shared by its tests."""
    return fit(batch(kind, s, m)[0], span=1)


@functools.lru_cache(maxsize=None)
def _oracle(kind, s, m):
    base = _base(kind, s, m)
    return np.array([O.compute_gpar_dtc_objective(V, Z, t, y, base.theta[i])[0]
                     for i, (V, Z, t, y) in enumerate(batch(kind, s, m)[2])])


def test_knob_round_trip():
    ctx = G.context(0)
    assert ctx.schedule("corr_span") == -1
    for v in (1, 2, 4, 8, -1):
        ctx.set_schedule("corr_span", v)
        assert ctx.schedule("corr_span") == v
    for v in (0, 3, 16, -2):
        with pytest.raises(G.DomainError):
            ctx.set_schedule("corr_span", v)
    assert ctx.schedule("corr_span") == -1


@pytest.mark.parametrize("kind,s,m", CASES, ids=[golden_key(*c) for c in CASES])
def test_span_one_is_the_parent_bit_for_bit(kind, s, m):
    base = _base(kind, s, m)
    with np.load(GOLDEN) as gold:
        key = golden_key(kind, s, m)
        np.testing.assert_array_equal(base.nlml, gold[key + "_nlml"])
        np.testing.assert_array_equal(base.theta, gold[key + "_theta"])


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("kind,s,m", CASES, ids=[golden_key(*c) for c in CASES])
def test_objective_matches_span_one_and_the_oracle(kind, s, m, span):
    probs = batch(kind, s, m)[0]
    base = _base(kind, s, m)
    got = base if span == 1 else fit(probs, span=span)
    ref = _oracle(kind, s, m)
    print(f"{golden_key(kind, s, m)} S={span}: -nlml {-got.nlml!r} S=1 {-base.nlml!r} oracle {ref!r} "
          f"rel S=1 {np.abs(got.nlml / base.nlml - 1).max():.2e} "
          f"rel oracle {np.abs(-got.nlml / ref - 1).max():.2e}")
    np.testing.assert_array_equal(got.theta, base.theta)      # the same simplex point
    np.testing.assert_allclose(got.nlml, base.nlml, rtol=1e-10)
    np.testing.assert_allclose(-got.nlml, ref, rtol=1e-10)


@pytest.mark.parametrize("span", [2, 4])
@pytest.mark.parametrize("kind,s,m", CASES, ids=[golden_key(*c) for c in CASES])
def test_span_is_bit_identical_to_its_serialized_twin(kind, s, m, span):
    probs = batch(kind, s, m)[0]
    a = fit(probs, span=span)
    b = fit(probs, span=span, serialize=1)
    np.testing.assert_array_equal(a.theta, b.theta)
    np.testing.assert_array_equal(a.nlml, b.nlml)
    np.testing.assert_array_equal(a.evals, b.evals)


@pytest.mark.parametrize("span", [2, 4])
def test_twelve_evaluation_fit_reaches_the_same_theta(span):
    probs = batch("tail", span, 128)[0]
    a = fit(probs, span=span, evals=12)
    b = fit(probs, span=1, evals=12)
    print("theta max rel", np.abs(a.theta / b.theta - 1).max(), "nlml", a.nlml, b.nlml)
    np.testing.assert_array_equal(a.evals, b.evals)
    np.testing.assert_allclose(a.theta, b.theta, rtol=1e-9)
    np.testing.assert_allclose(a.nlml, b.nlml, rtol=1e-9)


@pytest.mark.parametrize("span", [2, 4])
def test_span_in_the_round_overlap_equals_round_by_round(span):
    """Four outputs on the forced split take the round overlap (two groups whose rounds take
    turns, fit_overlapped), which builds its own stage jobs: the same span rule, so bit for bit
    the round-by-round fit (overlap 0) and its serialized twin, as every schedule must be.
    dg_rows_w, a plan of its own, is pinned as tests/test_gpu_schedule.py pins it: its auto value
    differs between the two schedules (N = 1573 has 8 DG splits, two of them on the whitening CUs,
    so it applies here)."""
    probs = batch("tail", span, 128, (17, 18, 19, 20))[0]
    a = fit(probs, span=span, evals=12, overlap=1, dg_rows_w=10)
    b = fit(probs, span=span, evals=12, overlap=0, dg_rows_w=10)
    c = fit(probs, span=span, evals=12, overlap=1, serialize=1, dg_rows_w=10)
    for o in (b, c):
        np.testing.assert_array_equal(a.theta, o.theta)
        np.testing.assert_array_equal(a.nlml, o.nlml)
        np.testing.assert_array_equal(a.evals, o.evals)


def chunk_transition(t, theta, j):
    """The closed-loop transition over chunk j, prod_k (I - K_k h) A_k, from the oracle's Riccati
    recursion: the Phi_j that span_psi composes (Psi_1 of a span that starts at chunk j)."""
    lg = O.build_lgssm(t, "matern52", theta[0], theta[1] ** 2, theta[4] ** 2)
    K = O.riccati(lg)[3]
    phi = np.eye(3)
    for k in range(256 * j, min(len(t), 256 * (j + 1))):
        a = lg.A[k].copy()
        phi = (a - np.outer(K[k], a[0])) @ phi
    return phi


@functools.lru_cache(maxsize=None)
def _slow(s):
    """The tail size of span s at X0_SLOW, corr_span = 1, and the oracle at the returned theta."""
    probs, _, data = batch("tail", s, 128)
    base = fit(probs, span=1, x0=X0_SLOW)
    ref = np.array([O.compute_gpar_dtc_objective(V, Z, t, y, base.theta[i])[0]
                    for i, (V, Z, t, y) in enumerate(data)])
    return base, ref


@pytest.mark.parametrize("s", [2, 4])
def test_slow_decay_inputs_have_a_live_transition(s):
    """What makes the slow-decay cases a check of Psi: at the theta they evaluate, the transition
    over every chunk of the first span is far from zero (at X0 it is below 1e-12)."""
    base, _ = _slow(s)
    t = batch("tail", s, 128)[2][0][2]
    for i in range(len(DIMS)):
        for j in range(s):
            nrm = np.linalg.norm(chunk_transition(t, base.theta[i], j), 2)
            print(f"S={s} output {i} chunk {j}: |Phi| = {nrm:.3e}")
            assert nrm > 1e-3
    fast = np.linalg.norm(chunk_transition(t, np.exp(X0) + 1e-3, 1), 2)
    print(f"at X0: |Phi_1| = {fast:.3e}")
    assert fast < 1e-6


@pytest.mark.parametrize("span", [2, 4])
@pytest.mark.parametrize("s", [2, 4])
def test_slow_decay_objective_matches_span_one_and_the_oracle(s, span):
    probs = batch("tail", s, 128)[0]
    base, ref = _slow(s)
    got = fit(probs, span=span, x0=X0_SLOW)
    twin = fit(probs, span=span, x0=X0_SLOW, serialize=1)
    print(f"slow tail_{s} S={span}: -nlml {-got.nlml!r} S=1 {-base.nlml!r} oracle {ref!r} "
          f"rel S=1 {np.abs(got.nlml / base.nlml - 1).max():.2e} "
          f"rel oracle {np.abs(-got.nlml / ref - 1).max():.2e} "
          f"S=1 rel oracle {np.abs(-base.nlml / ref - 1).max():.2e}")
    np.testing.assert_array_equal(got.theta, base.theta)
    np.testing.assert_allclose(got.nlml, base.nlml, rtol=1e-10)
    np.testing.assert_allclose(-got.nlml, ref, rtol=1e-10)
    np.testing.assert_array_equal(got.nlml, twin.nlml)
