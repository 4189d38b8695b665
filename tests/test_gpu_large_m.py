"""Pseudo-point counts in (600, 2048] at small N.  check_problem accepts m <= 2048 and the dense
tail is sized for it (finish2_kernel's b[2048], w[2048]; kMaxMTrsv = kMaxM = 2048), but the other
tests stop at M = 600 except for the full-size M = 1024 runs.  Here Mp / 128 = 8..16 blocks of the
Gram (36..120 off-diagonal groups), 16..32 blocks of 64 in the blocked Cholesky, its inverse and
finish2_kernel's solves, 4..8 centre groups of 256 columns in the distance, whitening and
Kfu-vector kernels, the unfused prediction at Mp up to 2048, and the m > 2048 rejection -- each
against the oracle at the tolerance the suite already uses for that quantity:

  objective   1e-10 max(1, |ref|)                           test_dtc_objective_matches_oracle
  A           rtol 1e-9, atol 1e-11 max|ref|                test_dtc_with_gaps_and_A
  distances   r^2 to 32 eps scale, r rel 1e-12 where r^2 >= 1e-3 scale; Matern-1/2 rtol 1e-14
                                                            test_cached_distances_match_direct_differences
  q(u)        U_u rtol 1e-9, atol 1e-10 max|U|; m_e, cov rtol 1e-7, atol 1e-9 max|ref|, granted
              while cond(Cuu) <= 1e7                        test_q_u_matches_oracle
  prediction  mean rtol 1e-8, atol 1e-9 max|ref|; std rtol 1e-7, atol 1e-9 max|ref|
                                                            test_predict_analytic_matches_oracle
  mean-only   rtol 1e-8, atol 1e-9 max|ref|                 test_gpu_predict_mean.py's _check
  batches     rtol 1e-10                                    test_mixed_batch_sizes

The objective and the predictions use Kuu + sigma^2 I (kuu_noise, qu_kuu_noise), which keeps
cond(Kuu) at a few thousand.  Each case's oracle values are computed once and shared.
Measured on an MI355X: DESIGN.md §7.
"""
import functools

import numpy as np
import pytest

from oracle import gpar_oracle as O

pytestmark = pytest.mark.gpu
G = pytest.importorskip("gparatscale")


def _theta(D, l_o=None):
    return (1.2, 0.9, 1.0 + 0.1 * D ** 0.5 if l_o is None else l_o, 1.1, 0.3)


# name: (n, D, M, (output kernel, time kernel), theta)
SHAPES = {
    # Mp / 128 = 8, exactly the full-size M, at small N
    "M1024": (1100, 3, 1024, ("matern52", "matern52"), _theta(3)),
    # one column into a ninth 128-block, 127 padded columns
    "M1025": (1300, 2, 1025, ("matern52", "matern32"), _theta(2)),
    "M1100_eq": (1400, 2, 1100, ("eq", "matern32"), _theta(2)),
    # an odd number of 128-blocks (13), state dimension 1
    "M1537": (1800, 5, 1537, ("matern32", "matern12"), _theta(5)),
    # ragged in the last 64-block of finish2_kernel's b[2048]
    "M1999": (2100, 3, 1999, ("matern52", "matern52"), _theta(3)),
    # the limit, no padding
    "M2048": (2304, 3, 2048, ("matern52", "matern52"), _theta(3)),
    # D > 64: the distance pass feeds the whitening
    "M1100_D70": (1300, 70, 1100, ("matern52", "matern52"), _theta(70, 6.0)),
    # Matern-1/2 output kernel: direct differences (whiten_kfu, kfu_gemv_direct)
    "M1100_m12": (1400, 2, 1100, ("matern12", "matern32"), _theta(2)),
}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _inputs(name):
    n, D, M, _, _ = SHAPES[name]
    t, Y = O.synthetic_gpar(n, D + 1, seed=M + D, noise=0.3)
    V = np.ascontiguousarray(Y[:, :D].T)
    y = Y[:, D].copy()
    Z = O.pick_pseudo_inputs(V, M, M + D + 7)
    return _frozen(t, V, Z, y)


@functools.lru_cache(maxsize=None)
def _oracle_objective(name):
    _, _, _, (ok, tk), theta = SHAPES[name]
    t, V, Z, y = _inputs(name)
    return O.compute_gpar_dtc_objective(V, Z, t, y, theta, ok, tk)      # (dtc, A)


def _close(got, ref, rtol, atol_rel, what):
    """assert_allclose(rtol, atol = atol_rel max|ref|), printing the measured maximum first."""
    got, ref = np.asarray(got), np.asarray(ref)
    scale = np.abs(ref).max()
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    used = (np.abs(got - ref) / (atol_rel * scale + rtol * np.abs(ref))).max()
    print(f"{what}: max|diff| / max|ref| = {np.abs(got - ref).max() / scale:.3e}, "
          f"{used:.3f} of the tolerance")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol_rel * scale, err_msg=what)


# ---------------------------------------------------------------------------- objective, A
@pytest.mark.parametrize("name", list(SHAPES))
def test_objective_matches_oracle(name):
    _, _, _, (ok, tk), theta = SHAPES[name]
    t, V, Z, y = _inputs(name)
    ref, _ = _oracle_objective(name)
    got = G.compute_gpar_dtc_objective(V, Z, t, y, theta, ok, tk)
    print(f"{name}: |got - ref| / max(1, |ref|) = {abs(got - ref) / max(1.0, abs(ref)):.3e}")
    assert abs(got - ref) <= 1e-10 * max(1.0, abs(ref)), (got, ref)


@pytest.mark.parametrize("name", ["M1025", "M2048"])
def test_A_matches_oracle(name):
    """A = L_u^-1 beta^T (M x N): an error confined to a few columns moves the scalar objective
    too little to see, A shows it."""
    _, _, _, (ok, tk), theta = SHAPES[name]
    t, V, Z, y = _inputs(name)
    ref, A_ref = _oracle_objective(name)
    got, A = G.compute_gpar_dtc_objective(V, Z, t, y, theta, ok, tk, return_A=True)
    assert abs(got - ref) <= 1e-10 * max(1.0, abs(ref)), (got, ref)
    _close(A, A_ref, 1e-9, 1e-11, f"{name} A")


# ---------------------------------------------------------------------------- distances
@functools.lru_cache(maxsize=None)
def _distance_points(D):
    """700 points (five 128-row tiles and 60 rows) and up to 2048 centres in D dimensions."""
    _, Y = O.synthetic_gpar(2304, D, seed=57 + D, noise=0.3)
    Vall = np.ascontiguousarray(Y.T)
    return _frozen(np.ascontiguousarray(Vall[:, :700]), O.pick_pseudo_inputs(Vall, 2048, 200 + D))


@pytest.mark.parametrize("kernel", ["matern52", "eq", "matern12"])
@pytest.mark.parametrize("D", [3, 16])
@pytest.mark.parametrize("M", [1100, 2048])
def test_pairwise_distances_match_direct_differences(M, D, kernel):
    V, Zall = _distance_points(D)
    Z = np.ascontiguousarray(Zall[:, :M])
    got = G.pairwise_distances(V, Z, kernel)
    r2 = np.zeros((V.shape[1], M))
    for q in range(D):
        diff = V[q][:, None] - Z[q][None, :]
        r2 += diff * diff
    if kernel == "matern12":                                # direct differences on the device too
        np.testing.assert_allclose(got, np.sqrt(r2), rtol=1e-14, atol=2e-100)
        return
    eps = np.finfo(np.float64).eps
    g2 = got if kernel == "eq" else got * got
    scale = np.einsum("dk,dk->k", V, V).max() + np.einsum("dc,dc->c", Z, Z).max()
    print(f"M={M} D={D} {kernel}: max|r^2 diff| / (eps scale) = {np.abs(g2 - r2).max() / (eps * scale):.2f}")
    assert np.abs(g2 - r2).max() <= 32 * eps * scale, (np.abs(g2 - r2).max(), scale)
    big = r2 >= 1e-3 * scale
    assert big.mean() > 0.5
    np.testing.assert_allclose(np.sqrt(g2[big]), np.sqrt(r2[big]), rtol=1e-12)


# ---------------------------------------------------------------------------- q(u)
# (shape, output kernel, l_o): l_o chosen so that the oracle's noise-free Cuu has cond <= 1e7, the
# range in which test_q_u_matches_oracle's tolerances hold.  The build forms D = T_u (beta^T beta)
# T_u^T + I where the reference forms B B^T + I with B = L_u^-1 beta^T; the two associations differ
# by ~cond(Cuu) eps in D (test_dtc_small_noise_ill_conditioned_kuu), which reaches the small
# entries of inv(D), held to atol = 1e-9 max|cov| alone, once 1e-14 cond approaches 1e-9.  So the
# conds here are a few 1e5 (on the CPU: 5.7e5 and 2.3e5), not 1e7: at l_o = 0.25 (cond 3.2e6) the
# M = 2048 cov measured 0.97 of its tolerance on an MI355X, m_e 0.05, U_u 0.02.
QU = {"M1100": ("M1100_m12", "matern12", 1.5), "M2048": ("M2048", "matern52", 0.15)}


@functools.lru_cache(maxsize=None)
def _oracle_q_u(key):
    name, ok, l_o = QU[key]
    n, D, M, (_, tk), _ = SHAPES[name]
    t, V, Z, y = _inputs(name)
    theta = _theta(D, l_o)
    me, cov, U, _ = O.compute_q_u(V, Z, t, y, theta, ok, tk)
    w = np.linalg.eigvalsh(U.T @ U)
    return theta, me, cov, U, w[-1] / w[0]


@pytest.mark.parametrize("key", list(QU))
def test_q_u_noise_free_matches_oracle(key):
    name, ok, _ = QU[key]
    tk = SHAPES[name][3][1]
    t, V, Z, y = _inputs(name)
    theta, me_r, cov_r, U_r, cond = _oracle_q_u(key)
    print(f"{key}: cond(Cuu) = {cond:.3e}")
    assert cond <= 1e7, cond
    me, cov, U = G.compute_q_u(V, Z, t, y, theta, ok, tk)
    _close(U, U_r, 1e-9, 1e-10, f"{key} U_u")
    _close(me, me_r, 1e-7, 1e-9, f"{key} m_e")
    _close(cov, cov_r, 1e-7, 1e-9, f"{key} cov")


# ---------------------------------------------------------------------------- predictions
PRED = [(name, ns) for name in ("M1025", "M1537", "M2048") for ns in (129, 333)]
MEAN_ONLY = PRED + [("M1100_m12", 129), ("M1100_D70", 129)]
_pid = lambda c: f"{c[0]}_N{c[1]}"     # noqa: E731


@functools.lru_cache(maxsize=None)
def _test_points(name, n_star):
    """N* test times beyond both ends of the training grid, the inputs interpolated to them."""
    t, V, _, _ = _inputs(name)
    rng = np.random.default_rng(n_star + V.shape[1])
    ts = np.sort(rng.uniform(t[0] - 1.0, t[-1] + 2.0, n_star))
    Vs = np.vstack([np.interp(ts, t, V[q]) for q in range(V.shape[0])])
    assert ts[0] < t[0] and ts[-1] > t[-1]
    return _frozen(ts, Vs)


@functools.lru_cache(maxsize=None)
def _oracle_prediction(name, n_star):
    _, _, _, (ok, tk), theta = SHAPES[name]
    t, V, Z, y = _inputs(name)
    ts, Vs = _test_points(name, n_star)
    return O.get_gpar_scaled_predictions_fixed(V, Z, t, y, ts, Vs, theta, ok, tk, "analytic",
                                               qu_kuu_noise=True)


@functools.lru_cache(maxsize=None)
def _device_prediction(name, n_star):
    _, _, _, (ok, tk), theta = SHAPES[name]
    t, V, Z, y = _inputs(name)
    ts, Vs = _test_points(name, n_star)
    return G.predict_scaled(V, Z, t, y, theta, ts, Vs, ok, tk, mode="analytic", qu_kuu_noise=True)


@pytest.mark.parametrize("case", PRED, ids=_pid)
def test_prediction_matches_oracle(case):
    rm, rs = _oracle_prediction(*case)
    mean, std = _device_prediction(*case)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std > 0)
    _close(mean, rm, 1e-8, 1e-9, f"{_pid(case)} mean")
    _close(std, rs, 1e-7, 1e-9, f"{_pid(case)} std")


@pytest.mark.parametrize("case", MEAN_ONLY, ids=_pid)
def test_mean_only_prediction_matches_oracle_and_full(case):
    name, n_star = case
    _, _, _, (ok, tk), theta = SHAPES[name]
    t, V, Z, y = _inputs(name)
    ts, Vs = _test_points(name, n_star)
    rm, _ = _oracle_prediction(name, n_star)
    full, _ = _device_prediction(name, n_star)
    mean = G.predict_mean_scaled(V, Z, t, y, theta, ts, Vs, ok, tk, qu_kuu_noise=True)
    _close(mean, rm, 1e-8, 1e-9, f"{_pid(case)} mean-only vs oracle")
    _close(mean, full, 1e-8, 1e-9, f"{_pid(case)} mean-only vs full path")


# ---------------------------------------------------------------------------- batches
BATCH_M = (40, 2048, 1100, 600)
X0 = np.array([0.0, 0.0, 0.5, 0.0, -1.5])


@functools.lru_cache(maxsize=None)
def _batch_data():
    """Four outputs of one draw on one time grid, D = 1..4, M = BATCH_M: the batch's G is padded
    to the widest output."""
    t, Y = O.synthetic_gpar(2304, 5, seed=91, noise=0.3)
    data = []
    for p, M in zip(range(2, 6), BATCH_M):
        V = np.ascontiguousarray(Y[:, : p - 1].T)
        data.append(_frozen(V, O.pick_pseudo_inputs(V, M, p), Y[:, p - 1].copy()))
    t.setflags(write=False)
    return t, data


@functools.lru_cache(maxsize=None)
def _oracle_batch_objective(i, theta):
    t, data = _batch_data()
    V, Z, y = data[i]
    return O.compute_gpar_dtc_objective(V, Z, t, y, theta)[0]


@pytest.mark.parametrize("split", [None, 8], ids=["default", "cu_split8"])
def test_batched_objective_and_fit_padded_to_widest(split):
    """dtc_objective_batch and fit_batch over M = (40, 2048, 1100, 600): every output against the
    oracle, and the fit's reported value against the device objective and the oracle's at the
    fitted theta (one oracle evaluation per output).  With the CU split, the split Gram plans 120
    off-diagonal groups on 192 CUs."""
    t, data = _batch_data()
    probs, keep, thetas = [], [], []
    for p, (V, Z, y) in zip(range(2, 6), data):
        pr, k = G.make_problem(V, Z, t, y)
        probs.append(pr); keep.append(k)
        thetas.append((1.0, 0.9, 1.0 + 0.2 * p, 1.1, 0.25))
    ctx = G.context(0)
    try:
        if split is not None:
            ctx.set_cu_split(split)
        got = G.dtc_objective_batch(probs, thetas)
        fit = G.fit_batch(probs, np.tile(X0, (len(probs), 1)), max_evals=8, g_tol=-1.0)
    finally:
        ctx.set_cu_split(-1)
    refs = [_oracle_batch_objective(i, thetas[i]) for i in range(len(probs))]
    print("batch objective rel:", np.abs((got - refs) / refs))
    np.testing.assert_allclose(got, refs, rtol=1e-10)
    for i, (V, Z, y) in enumerate(data):
        th = tuple(float(v) for v in fit.theta[i])
        assert np.all(np.isfinite(th)) and np.isfinite(fit.nlml[i])
        dev = G.compute_gpar_dtc_objective(V, Z, t, y, th)
        ref = _oracle_batch_objective(i, th)
        print(f"fit output {i} (M = {BATCH_M[i]}): vs device {abs(-fit.nlml[i] - dev) / abs(dev):.3e}, "
              f"vs oracle {abs(-fit.nlml[i] - ref) / abs(ref):.3e}")
        assert abs(-fit.nlml[i] - dev) <= 1e-10 * abs(dev), (i, fit.nlml[i], dev)
        assert abs(-fit.nlml[i] - ref) <= 1e-10 * abs(ref), (i, fit.nlml[i], ref)


# ---------------------------------------------------------------------------- rejection
def test_m_2049_is_rejected_everywhere():
    """m > 2048 raises Unsupported (GPAR_ERR_UNSUPPORTED) from every entry point before any
    launch, also when only the last problem of a batch is too wide; the context works afterwards."""
    t, Y = O.synthetic_gpar(300, 3, seed=4, noise=0.3)
    V, y = np.ascontiguousarray(Y[:, :2].T), Y[:, 2].copy()
    rng = np.random.default_rng(4)
    Zw = rng.normal(size=(2, 2049)) + V.mean(axis=1, keepdims=True)
    Z = O.pick_pseudo_inputs(V, 20, 3)
    theta = _theta(2)
    ts, Vs = t[::7] + 0.01, V[:, ::7] + 0.01
    with pytest.raises(G.Unsupported):
        G.compute_gpar_dtc_objective(V, Zw, t, y, theta)
    with pytest.raises(G.Unsupported):
        G.compute_q_u(V, Zw, t, y, theta)
    with pytest.raises(G.Unsupported):
        G.predict_scaled(V, Zw, t, y, theta, ts, Vs)
    with pytest.raises(G.Unsupported):
        G.predict_mean_scaled(V, Zw, t, y, theta, ts, Vs)
    probs, keep = [], []
    for z in (Z, Z, Zw):
        pr, k = G.make_problem(V, z, t, y)
        probs.append(pr); keep.append(k)
    with pytest.raises(G.Unsupported):
        G.dtc_objective_batch(probs, [theta] * 3)
    with pytest.raises(G.Unsupported):
        G.fit_batch(probs, np.tile(X0, (3, 1)), max_evals=8, g_tol=-1.0)
    # exactly 2048 is not rejected by the check (run in the tests above); the context still works
    ref, _ = O.compute_gpar_dtc_objective(V, Z, t, y, theta)
    got = G.compute_gpar_dtc_objective(V, Z, t, y, theta)
    assert abs(got - ref) <= 1e-10 * max(1.0, abs(ref)), (got, ref)
    np.testing.assert_allclose(G.dtc_objective_batch(probs[:2], [theta] * 2), [ref, ref], rtol=1e-10)
