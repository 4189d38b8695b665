"""The gains' phase 1 by lanes per chunk.  launch_gains takes gains_phase1<D, 4> (four lanes per
chunk, combined through lane shuffles) below 262144 chunk-chains and gains_phase1<D, 1> (one lane
per chunk: early return, no shuffles, k1 = c1, another combine order) above, a size only the
production shards reach.  GPAR_GAINS_P1_LANES = 1 / 4 forces one kernel at any size, and
gpar_debug_counter("gains_p1_lane1" / "gains_p1_lane4") shows which one ran.  Every later phase
reads the aggregates phase 1 writes, so each kernel is checked through the chains' logpdf,
the smoother, a DTC objective and an analytic prediction against the oracle, at the tolerances of
the tests that cover the default path:

  logpdf rel 1e-10                                    test_lgssm_logpdf_matches_oracle
  smoothed mean rtol 1e-9, atol 1e-10 max|ref|;
  variance rtol 1e-8, atol 1e-12                      test_lgssm_smooth_matches_oracle
  objective 1e-10 max(1, |ref|)                       test_dtc_objective_matches_oracle
  prediction mean rtol 1e-8, atol 1e-9 max|ref|;
  std rtol 1e-7, atol 1e-9 max|ref|                   test_predict_analytic_matches_oracle

Measured on an MI355X: see DESIGN.md §4.1 and §7.
"""
import functools

import numpy as np
import pytest

from oracle import gpar_oracle as O

pytestmark = pytest.mark.gpu
G = pytest.importorskip("gparatscale")

KINDS = ["matern12", "matern32", "matern52"]          # state dimensions 1, 2, 3
TH = np.array([[0.05, 1.3, 0.2], [0.5, 0.7, 0.6], [4.0, 2.0, 0.05]])
N_SHORT = 1300                  # 6 chunks of 256, the last one short
N_MID = 256 * 40 + 8
N_LONG = 256 * 300 + 8          # run_len = 2, several phase-1 workgroups per chain


class _Lanes:
    """GPAR_GAINS_P1_LANES = lanes for the block; on exit asserts through the counters that the
    forced kernel ran and the other one did not."""

    def __init__(self, monkeypatch, lanes):
        self.mp, self.lanes = monkeypatch, lanes

    def __enter__(self):
        self.mp.setenv("GPAR_GAINS_P1_LANES", str(self.lanes))
        self.c1, self.c4 = G.debug_counter("gains_p1_lane1"), G.debug_counter("gains_p1_lane4")
        return self

    def __exit__(self, *exc):
        d1 = G.debug_counter("gains_p1_lane1") - self.c1
        d4 = G.debug_counter("gains_p1_lane4") - self.c4
        self.mp.delenv("GPAR_GAINS_P1_LANES")
        if exc[0] is None:
            took, other = (d1, d4) if self.lanes == 1 else (d4, d1)
            assert took >= 1 and other == 0, (self.lanes, d1, d4)
        return False


@functools.lru_cache(maxsize=None)
def _chains(n):
    """An irregular grid with a few large gaps and repeated stamps, three chains' data, and a
    noise vector (every fifth point a 'test' point of variance 1e10, the rest the chain's own)."""
    rng = np.random.default_rng(17 + n)
    dt = rng.exponential(0.05, n) + np.where(rng.random(n) < 0.01, 3.0, 0.0)
    dt[rng.choice(np.arange(1, n), size=7, replace=False)] = 0.0       # repeated stamps
    dt[[255, 256, 257]] = (0.0, 3.0, 0.0)                              # at a chunk boundary too
    t = np.cumsum(dt)
    Y = np.ascontiguousarray(rng.normal(size=(3, n)))
    noise = np.where(np.arange(n) % 5 == 0, 1e10, -1.0)
    for a in (t, Y, noise):
        a.setflags(write=False)
    return t, Y, noise


@functools.lru_cache(maxsize=None)
def _oracle_chains(n, kind):
    """(logpdfs, smoothed means, variances) of the three chains, computed once per (n, kind)."""
    t, Y, noise = _chains(n)
    lml, mean, var = [], [], []
    for c in range(3):
        lml.append(O.lgssm_logpdf(O.create_lgssm(t, *TH[c], kind=kind), Y[c]))
        R = np.where(noise < 0, TH[c][2] ** 2, noise)
        ms, Ps = O.rts_smooth(O.create_lgssm(t, *TH[c], kind=kind, noise_vector=R), Y[c])
        mean.append(ms[:, 0])
        var.append(Ps[:, 0, 0])
    return np.array(lml), np.array(mean), np.array(var)


def _run_chains(n, kind):
    t, Y, noise = _chains(n)
    lml = np.asarray(G.lgssm_logpdf_batch(t, Y, TH, kind))
    m, v = G.lgssm_smooth_batch(t, Y, TH, kind, noise=noise)
    return lml, np.asarray(m), np.asarray(v)


def _report(what, got, ref):
    print(f"{what}: max|diff| / max|ref| = {np.abs(got - ref).max() / np.abs(ref).max():.3e}")


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("n", [N_SHORT, N_MID])
@pytest.mark.parametrize("kind", KINDS)
def test_chains_match_oracle(kind, n, lanes, monkeypatch):
    r_lml, r_mean, r_var = _oracle_chains(n, kind)
    with _Lanes(monkeypatch, lanes):
        lml, mean, var = _run_chains(n, kind)
    for what, g, r in (("logpdf", lml, r_lml), ("mean", mean, r_mean), ("var", var, r_var)):
        assert np.all(np.isfinite(g))
        _report(f"{kind} n={n} lanes={lanes} {what}", g, r)
    for c in range(3):
        assert abs(lml[c] - r_lml[c]) <= 1e-10 * max(1.0, abs(r_lml[c])), (c, lml[c], r_lml[c])
        np.testing.assert_allclose(mean[c], r_mean[c], rtol=1e-9,
                                   atol=1e-10 * np.abs(r_mean[c]).max())
        np.testing.assert_allclose(var[c], r_var[c], rtol=1e-8, atol=1e-12)


@functools.lru_cache(maxsize=None)
def _gpar(kind):
    """n = 1300, D = 3, M = 40 with N* = 129 test points beyond both ends of the training grid,
    and the oracle's objective and analytic prediction there."""
    n, D, M, n_star = N_SHORT, 3, 40, 129
    t, Y = O.synthetic_gpar(n, D + 1, seed=3, noise=0.3, gaps=2, gap_len=n // 20)
    V, y = np.ascontiguousarray(Y[:, :D].T), Y[:, D].copy()
    Z = O.pick_pseudo_inputs(V, M, 10)
    ts = np.sort(np.random.default_rng(14).uniform(t[0] - 1.0, t[-1] + 2.0, n_star))
    Vs = np.vstack([np.interp(ts, t, V[q]) for q in range(D)])
    theta = (1.2, 0.9, 1.0 + 0.1 * D ** 0.5, 1.1, 0.3)
    dtc, _ = O.compute_gpar_dtc_objective(V, Z, t, y, theta, "matern52", kind)
    rm, rs = O.get_gpar_scaled_predictions_fixed(V, Z, t, y, ts, Vs, theta, "matern52", kind,
                                                 "analytic", qu_kuu_noise=True)
    return (t, V, Z, y, ts, Vs, theta), dtc, rm, rs


@pytest.mark.parametrize("kind", KINDS)
def test_objective_and_prediction_one_lane(kind, monkeypatch):
    """The shared gains with data (the objective) and over the merged grid with a noise vector and
    filtered covariances (the prediction), from the one-lane aggregates."""
    (t, V, Z, y, ts, Vs, theta), dtc, rm, rs = _gpar(kind)
    with _Lanes(monkeypatch, 1):
        got = G.compute_gpar_dtc_objective(V, Z, t, y, theta, "matern52", kind)
    assert abs(got - dtc) <= 1e-10 * max(1.0, abs(dtc)), (got, dtc)
    with _Lanes(monkeypatch, 1):
        mean, std = G.predict_scaled(V, Z, t, y, theta, ts, Vs, "matern52", kind, mode="analytic",
                                     qu_kuu_noise=True)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std > 0)
    _report(f"{kind} one-lane prediction mean", mean, rm)
    _report(f"{kind} one-lane prediction std", std, rs)
    np.testing.assert_allclose(mean, rm, rtol=1e-8, atol=1e-9 * np.abs(rm).max())
    np.testing.assert_allclose(std, rs, rtol=1e-7, atol=1e-9 * np.abs(rs).max())


@pytest.mark.parametrize("kind", KINDS)
def test_one_lane_against_four_lanes_many_workgroups(kind, monkeypatch):
    """n = 256 * 300 + 8: 301 chunks, so each scan thread owns two aggregates and phase 1 runs
    two (one lane) or five (four lanes) workgroups per chain.  The two kernels fold the same steps
    in another order and are not bit-identical; each is within the oracle bounds of
    test_chains_match_oracle, so they differ by at most twice those.  One chain's logpdf is
    checked against the C port of the reference's filter (the numpy oracle's step loop would take
    most of a minute at this n)."""
    from oracle import cpu_ref as CR
    CR.load()
    t, Y, _ = _chains(N_LONG)
    out = {}
    for lanes in (1, 4):
        with _Lanes(monkeypatch, lanes):
            out[lanes] = _run_chains(N_LONG, kind)
    (l1, m1, v1), (l4, m4, v4) = out[1], out[4]
    for a in out[1] + out[4]:
        assert np.all(np.isfinite(a))
    print(f"{kind} lanes 1 vs 4: logpdf rel {np.abs((l1 - l4) / l4).max():.3e}, "
          f"mean {np.abs(m1 - m4).max() / np.abs(m4).max():.3e} of max, "
          f"var rel {np.abs((v1 - v4) / v4).max():.3e}")
    assert np.all(np.abs(l1 - l4) <= 2e-10 * np.maximum(1.0, np.abs(l4))), (l1, l4)
    for c in range(3):
        np.testing.assert_allclose(m1[c], m4[c], rtol=2e-9, atol=2e-10 * np.abs(m4[c]).max())
        np.testing.assert_allclose(v1[c], v4[c], rtol=2e-8, atol=2e-12)
    c = 1
    ref = CR.lgssm_logpdf(kind, t, Y[c], TH[c][0], TH[c][1] ** 2, TH[c][2] ** 2)
    for lml in (l1, l4):
        assert abs(lml[c] - ref) <= 1e-10 * max(1.0, abs(ref)), (lml[c], ref)


@pytest.mark.parametrize("kind", KINDS)
def test_offset_data_one_lane(kind, monkeypatch):
    """test_lgssm_logpdf_offset_data_matches_oracle's case (y + 1e3, small noise sd: per-chunk
    moments of ~1e6 that cancel) from the one-lane aggregates, at its rel 1e-10."""
    t, Y = O.synthetic_gpar(N_MID, 3, seed=5, noise=0.05)
    Y = Y + 1e3
    th = [(0.5, 1.3, 0.05), (2.0, 0.7, 0.05), (10.0, 2.0, 0.02)]
    with _Lanes(monkeypatch, 1):
        got = G.lgssm_logpdf_batch(t, np.ascontiguousarray(Y.T), th, kind)
    for c in range(3):
        ref = O.lgssm_logpdf(O.create_lgssm(t, *th[c], kind=kind), Y[:, c])
        assert abs(got[c] - ref) <= 1e-10 * abs(ref), (c, got[c], ref)


def test_size_rule_when_unset(monkeypatch):
    """Unset, or set to anything but 1 or 4, the size rule holds: four lanes at these sizes."""
    t, Y, _ = _chains(N_SHORT)
    for val in (None, "2", "14", ""):
        if val is None:
            monkeypatch.delenv("GPAR_GAINS_P1_LANES", raising=False)
        else:
            monkeypatch.setenv("GPAR_GAINS_P1_LANES", val)
        c1, c4 = G.debug_counter("gains_p1_lane1"), G.debug_counter("gains_p1_lane4")
        G.lgssm_logpdf_batch(t, Y, TH, "matern32")
        assert G.debug_counter("gains_p1_lane1") == c1, val
        assert G.debug_counter("gains_p1_lane4") > c4, val
