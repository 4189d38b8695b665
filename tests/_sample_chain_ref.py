"""numpy restatement of the sample-chained prediction (gpar_predict_samples), the yardstick of
tests/test_gpu_sample_chain.py, built only from oracle.gpar_oracle's compute_q_u, merge_grid,
pairwise, build_lgssm and lgssm_posterior_rand.

get_gpar_scaled_predictions_path_fixed (the estimator of src/gp/tmp.jl:119-167) with one change:
sample s's Cf*u is taken at its own test inputs [shared | sample_s], so
  FX[:, s] = Kstar_s U_u^{-1} e_s,   e_s = m_e + chol(inv(D)) xi_u[:, s],
and everything after FX is the path estimator's."""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import gpar_oracle as O


def _ref_samples(V, Z, t, y, t_star, shared, samp, theta, xi_u, xi_path, out_kernel="matern52",
                 time_kernel="matern52", qu_kuu_noise=False):
    """V D x n, Z D x M (ColVecs); shared d_sh x N* (or None); samp S x N* x d_sa (or None);
    xi_u M x S; xi_path S x (n + N*) x (d + 1), the merged grid in time order.
    Returns (F S x N*, mean, std) at the test points in input order."""
    l_t, sv_t, l_o, sv_o, sigma = (float(v) for v in theta)
    s_t, s_o, s2 = sv_t * sv_t, sv_o * sv_o, sigma * sigma
    V, Z = O.to_colvecs(V), O.to_colvecs(Z)
    n, ns = len(t), len(t_star)
    S = np.asarray(xi_u).shape[1]
    m_e, cov, U_u, _ = O.compute_q_u(V, Z, t, y, theta, out_kernel, time_kernel, qu_kuu_noise)
    tc, perm = O.merge_grid(t, t_star)
    yc = np.concatenate([np.asarray(y, float), np.zeros(ns)])[perm]
    Rc = np.concatenate([np.full(n, s2), np.full(ns, 1e10)])[perm]
    lg = O.build_lgssm(tc[perm], time_kernel, l_t, s_t, Rc)
    E = m_e[:, None] + np.linalg.cholesky(cov) @ np.asarray(xi_u, dtype=np.float64)
    B = solve_triangular(U_u, E, lower=False)                     # M x S: U_u^{-1} e_s
    sh = np.zeros((0, ns)) if shared is None else np.atleast_2d(np.asarray(shared, float))
    FX = np.empty((n + ns, S))
    for s in range(S):
        sa = np.zeros((0, ns)) if samp is None else np.asarray(samp, float)[s].T
        Vc = np.hstack([V, np.vstack([sh, sa])])[:, perm]
        Kstar_s = O.pairwise(out_kernel, Vc, Z, l_o, s_o)
        FX[:, s] = Kstar_s @ B[:, s]
    Ft = O.lgssm_posterior_rand(lg, yc[:, None] - FX, xi_path)    # S x (n + N*)
    F = FX + Ft.T
    inv = np.argsort(perm, kind="stable")
    Fs = F[inv][n:]                                               # N* x S, input order
    with np.errstate(invalid="ignore", divide="ignore"):
        std = Fs.std(axis=1, ddof=1) if S > 1 else np.full(ns, np.nan)
    return Fs.T.copy(), Fs.mean(axis=1), std
