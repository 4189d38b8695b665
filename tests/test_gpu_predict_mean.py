"""Mean-only prediction (gpar_predict_mean, gpar_posterior_predict_mean / _prepare_mean): the
ANALYTIC mean of get_gpar_scaled_predictions (gpar_scaled_inference.jl:91-97 with e = m_e) from one
Kfu-vector product with the kernel evaluated on the fly (k_kfu_gemv.hip) and a one-column smoother,
against the oracle and against the full prediction's mean at the full prediction's own mean
tolerance (tests/test_gpu_predict.py: rtol 1e-8, atol 1e-9 max|ref|).

Measured on an MI355X (largest |mean-only - ref| / max|ref| over the cases below): see DESIGN.md
§4.6.
"""
import functools

import numpy as np
import pytest

from oracle import gpar_oracle as O

pytestmark = pytest.mark.gpu
G = pytest.importorskip("gparatscale")

X0 = np.array([0.0, 0.0, 0.0, 0.0, -2.0])


def _data(n, P, M, seed, n_star, gaps=0):
    """tests/test_gpu_predict.py's helper: gaps in the training grid, test times beyond both of
    its ends."""
    t, Y = O.synthetic_gpar(n, P, seed=seed, noise=0.3, gaps=gaps, gap_len=max(1, n // 25))
    V = Y[:, : P - 1].T
    y = Y[:, P - 1]
    Z = O.pick_pseudo_inputs(V, M, seed + 3)
    rng = np.random.default_rng(seed + 11)
    ts = np.sort(rng.uniform(t[0] - 1.0, t[-1] + 2.0, n_star))
    Vs = np.vstack([np.interp(ts, t, V[q]) for q in range(P - 1)])
    return t, V, Z, y, ts, Vs


def _wide(n, D, M, seed, n_star):
    """tests/test_gpu_wide.py's inputs: D columns of one synthetic GPAR draw, test points beside
    training points."""
    t, Y = O.synthetic_gpar(n, D + 1, seed=seed, noise=0.3)
    V = np.ascontiguousarray(Y[:, :D].T)
    y = Y[:, D].copy()
    Z = O.pick_pseudo_inputs(V, M, seed + 7)
    idx = (np.arange(n_star) * (n // n_star)).astype(int)
    return t, V, Z, y, t[idx] + 0.013, V[:, idx] + 0.01


# name: (data, (out kernel, time kernel), theta, qu_kuu_noise).  The first three are
# test_predict_analytic_matches_oracle's cases.  The others sit on the new kernel's edges, with
# n + N* >= 3 * 256 so that both carries of the one-column smoother cross chunks; the wider M take
# the regularised q(u) (Cuu + sigma^2 I) so that cond(Cuu) does not limit the comparison.
CASES = {
    "base_m52": (lambda: _data(400, 3, 30, 5, 150, gaps=2), ("matern52", "matern52"),
                 (1.4, 0.9, 1.2, 1.1, 0.3), False),
    "base_eq": (lambda: _data(700, 4, 140, 5, 150, gaps=2), ("eq", "matern32"),
                (1.4, 0.9, 0.25, 1.1, 0.3), False),
    "base_m32": (lambda: _data(300, 2, 20, 5, 150, gaps=2), ("matern32", "matern12"),
                 (1.4, 0.9, 0.3, 1.1, 0.3), False),
    # M = 300 crosses a 256-column centre group and a column tile; N* = 129: one row past a tile
    "M300_D2_N129": (lambda: _data(700, 3, 300, 7, 129, gaps=1), ("matern52", "matern52"),
                     (1.3, 0.9, 0.9, 1.2, 0.3), True),
    # D = 1, one test point
    "M140_D1_N1": (lambda: _data(800, 2, 140, 8, 1), ("matern32", "matern32"),
                   (1.2, 1.0, 0.6, 1.1, 0.3), True),
    # D = 17: one K-step and one dimension of the next
    "M140_D17_N150": (lambda: _wide(650, 17, 140, 9, 150), ("matern52", "matern32"),
                      (1.1, 0.9, 3.0, 1.1, 0.25), True),
    # D = 70: wider than the fused whitening takes
    "M40_D70_N129": (lambda: _wide(700, 70, 40, 1, 129), ("matern52", "matern52"),
                     (1.3, 0.9, 6.0, 1.1, 0.2), True),
    # Matern-1/2 output kernel: the direct-difference kernel, across one 16-dimension slice
    "M64_D17_m12": (lambda: _wide(650, 17, 64, 10, 150), ("matern12", "matern32"),
                    (2.0, 0.7, 3.0, 1.0, 0.35), True),
    "M300_D2_eq": (lambda: _data(700, 3, 300, 11, 150), ("eq", "matern52"),
                   (1.2, 1.0, 0.4, 1.1, 0.3), True),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, oracle mean, full-path mean, mean-only mean) of a case, computed once."""
    make, (ok, tk), theta, qn = CASES[name]
    t, V, Z, y, ts, Vs = make()
    ref, _ = O.get_gpar_scaled_predictions_fixed(V, Z, t, y, ts, Vs, theta, ok, tk, "analytic",
                                                 qu_kuu_noise=qn)
    full, _ = G.predict_scaled(V, Z, t, y, theta, ts, Vs, ok, tk, mode="analytic", qu_kuu_noise=qn)
    mean = G.predict_mean_scaled(V, Z, t, y, theta, ts, Vs, ok, tk, qu_kuu_noise=qn)
    return ref, full, mean


def _check(got, ref, what):
    print(f"{what}: max|diff| / max|ref| = {np.abs(got - ref).max() / np.abs(ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=1e-8, atol=1e-9 * np.abs(ref).max())


@pytest.mark.parametrize("name", list(CASES))
def test_predict_mean_matches_oracle(name):
    ref, _, mean = _case(name)
    assert mean.shape == ref.shape and np.all(np.isfinite(mean))
    _check(mean, ref, f"{name} vs oracle")


@pytest.mark.parametrize("name", list(CASES))
def test_predict_mean_matches_full_prediction(name):
    _, full, mean = _case(name)
    _check(mean, full, f"{name} vs full path")


def test_predict_mean_unsorted_and_coincident_test_points():
    t, V, Z, y, ts, Vs = _data(350, 3, 25, 9, 120)
    ts = np.concatenate([ts, t[::37]])            # test times coinciding with train times
    Vs = np.hstack([Vs, V[:, ::37]])
    perm = np.random.default_rng(1).permutation(len(ts))
    ts, Vs = ts[perm], Vs[:, perm]
    theta = (0.9, 1.1, 0.8, 1.3, 0.25)
    ref, _ = O.get_gpar_scaled_predictions_fixed(V, Z, t, y, ts, Vs, theta, mode="analytic")
    _check(G.predict_mean_scaled(V, Z, t, y, theta, ts, Vs), ref, "unsorted, coincident")


@pytest.mark.parametrize("side", ["before", "after"])
def test_predict_mean_all_test_times_outside_the_training_grid(side):
    t, V, Z, y, _, _ = _data(600, 3, 30, 13, 1)
    rng = np.random.default_rng(3)
    ts = np.sort(rng.uniform(0.05, 1.5, 200))
    ts = t[0] - ts[::-1] if side == "before" else t[-1] + ts
    Vs = np.vstack([np.interp(ts, t, V[q]) for q in range(2)]) + 0.05 * rng.standard_normal((2, 200))
    theta = (1.2, 1.0, 0.9, 1.2, 0.3)
    ref, _ = O.get_gpar_scaled_predictions_fixed(V, Z, t, y, ts, Vs, theta, mode="analytic")
    _check(G.predict_mean_scaled(V, Z, t, y, theta, ts, Vs), ref, f"all {side}")


def test_predict_mean_device_inputs_equal_host_inputs():
    """Device tensors (V* a strided column slice) through the same kernels: the same bits."""
    import torch
    dev = torch.device("cuda", 0)
    t, V, Z, y, ts, Vs = _data(500, 4, 40, 15, 300)
    theta = (1.2, 1.0, 0.9, 1.2, 0.3)
    host = G.predict_mean_scaled(V, Z, t, y, theta, ts, Vs)
    F = torch.from_numpy(np.ascontiguousarray(np.vstack([Vs, Vs[:1]]).T)).to(dev)   # N* x 4
    got = G.predict_mean_scaled(torch.from_numpy(np.ascontiguousarray(V.T)).to(dev),
                                torch.from_numpy(np.ascontiguousarray(Z.T)).to(dev),
                                torch.from_numpy(t).to(dev), torch.from_numpy(y.copy()).to(dev),
                                theta, torch.from_numpy(ts).to(dev), F[:, :3])
    np.testing.assert_array_equal(got.cpu().numpy(), host)


def _posterior(qu_noise, seed=31, n=800, P=5, n_star=170, M=40, evals=15):
    import torch
    dev = torch.device("cuda", 0)
    t, Y = O.synthetic_gpar(n, P, seed=seed, noise=0.3)
    ts = np.sort(np.random.default_rng(seed + 1).uniform(t[0], t[-1], n_star))
    F = np.column_stack([np.interp(ts, t, Y[:, q]) for q in range(P)])
    t_d, Y_d, ts_d, F_d = (torch.from_numpy(a).to(dev) for a in (t, Y, ts, F))
    outs = [2, 3, 4, 5]
    probs, keep = [], []
    for p in outs:
        Z = torch.from_numpy(O.pick_pseudo_inputs(Y[:, : p - 1].T, M, p).T.copy()).to(dev)
        pr, k = G.make_problem(Y_d[:, : p - 1], Z, t_d, Y_d[:, p - 1].contiguous(),
                               qu_kuu_noise=qu_noise)
        probs.append(pr)
        keep.append((k, Z))
    post = G.fit_posterior(probs, np.tile(X0, (len(outs), 1)), max_evals=evals, g_tol=-1.0,
                           keep=keep)
    return post, ts_d, [F_d[:, : p - 1] for p in outs]


@pytest.mark.parametrize("qu_noise", [True, False])
def test_posterior_predict_mean_matches_predict_and_repeats(qu_noise):
    post, ts_d, Vs = _posterior(qu_noise)
    for i in range(len(Vs)):
        full = post.predict(i, ts_d, Vs[i])[0].cpu().numpy()
        first = post.predict_mean(i, ts_d, Vs[i]).cpu().numpy()    # computes the training rows
        second = post.predict_mean(i, ts_d, Vs[i]).cpu().numpy()   # finds them
        _check(first, full, f"posterior output {i} (qu_noise={qu_noise}) vs predict")
        np.testing.assert_array_equal(first, second)
    post.close()


def test_posterior_prepared_means_equal_in_line():
    """prepare_mean, and a slot left by plain prepare, give the in-line bits; a slot for another
    t_star tensor is not used; the training rows filled on the side stream by prepare_mean are the
    bits the in-line call computes."""
    post, ts_d, Vs = _posterior(True)
    ts2_d = ts_d.clone()   # same values, another pointer: not the prepared slot
    ref = [post.predict_mean(i, ts_d, Vs[i]).cpu().numpy() for i in range(len(Vs))]
    post.prepare_mean(0, ts_d)
    for i in range(len(Vs)):
        if i + 1 < len(Vs):
            post.prepare_mean(i + 1, ts_d)
        np.testing.assert_array_equal(post.predict_mean(i, ts_d, Vs[i]).cpu().numpy(), ref[i])
    post.prepare(1, ts_d)     # plain prepare's slot serves predict_mean
    np.testing.assert_array_equal(post.predict_mean(1, ts_d, Vs[1]).cpu().numpy(), ref[1])
    post.prepare_mean(2, ts_d)   # prepare_mean's slot serves predict
    full = post.predict(2, ts_d, Vs[2])
    full2 = post.predict(2, ts_d, Vs[2])
    np.testing.assert_array_equal(full[0].cpu().numpy(), full2[0].cpu().numpy())
    np.testing.assert_array_equal(full[1].cpu().numpy(), full2[1].cpu().numpy())
    post.prepare_mean(3, ts2_d)
    np.testing.assert_array_equal(post.predict_mean(3, ts_d, Vs[3]).cpu().numpy(), ref[3])
    post.close()
    # a fresh posterior whose training rows are first filled by prepare_mean, on the side stream
    post2, ts_b, Vs_b = _posterior(True)
    post2.prepare_mean(2, ts_b)
    np.testing.assert_array_equal(post2.predict_mean(2, ts_b, Vs_b[2]).cpu().numpy(), ref[2])
    post2.close()


def test_posterior_mean_argument_errors():
    import torch
    post, ts_d, Vs = _posterior(True, n=300, n_star=40, M=16, evals=8)
    with pytest.raises(G.DomainError):
        post.predict_mean(4, ts_d, Vs[0])                 # output index out of range
    with pytest.raises(G.DomainError):
        post.predict_mean(-1, ts_d, Vs[0])
    with pytest.raises(G.DomainError):
        post.predict_mean(2, ts_d, Vs[0])                 # wrong input width
    with pytest.raises(G.DomainError):
        post.predict_mean(0, ts_d[:10], Vs[0])            # N* disagrees
    with pytest.raises(G.DomainError):
        post.prepare_mean(7, ts_d)
    with pytest.raises(G.DomainError):
        post.prepare_mean(0, ts_d[::2])                   # not contiguous
    # the C entry points' own checks
    import ctypes as C
    lib, ctx = G.load(), G.context(0)
    mean = torch.empty(40, dtype=torch.float64, device=ts_d.device)
    v = Vs[0].contiguous()
    args = (ts_d.data_ptr(), v.data_ptr(), v.stride(0), mean.data_ptr())
    assert lib.gpar_posterior_predict_mean(ctx.h, post.h, 0, 0, *args) == 1          # n_star < 1
    assert lib.gpar_posterior_predict_mean(ctx.h, post.h, 9, 40, *args) == 1         # i
    assert lib.gpar_posterior_predict_mean(ctx.h, post.h, 1, 40, args[0], args[1], 1, args[3]) == 1
    assert lib.gpar_posterior_predict_mean(ctx.h, post.h, 0, 40, None, args[1], 1, args[3]) == 1
    assert lib.gpar_posterior_predict_mean(ctx.h, None, 0, 40, *args) == 1
    assert lib.gpar_posterior_prepare_mean(ctx.h, post.h, 0, 0, args[0]) == 1
    assert lib.gpar_posterior_prepare_mean(ctx.h, post.h, 0, 40, None) == 1
    assert lib.gpar_posterior_prepare_mean(ctx.h, post.h, -1, 40, args[0]) == 1
    post.close()
    # host-memory posteriors cannot prepare
    t, V, Z, y, ts, Vsh = _data(300, 3, 16, 5, 30)
    pr, k = G.make_problem(V, Z, t, y, qu_kuu_noise=True)
    hp = G.fit_posterior([pr], X0[None, :], max_evals=8, g_tol=-1.0, keep=[k])
    with pytest.raises(G.DomainError):
        hp.prepare_mean(0, torch.from_numpy(ts).to(ts_d.device))
    full = hp.predict(0, ts, Vsh)[0]
    _check(hp.predict_mean(0, ts, Vsh), full, "host posterior vs predict")
    th = np.ascontiguousarray(hp.theta[0])
    with pytest.raises(G.DomainError):
        G.predict_mean_scaled(V, Z, t, y, th, ts, Vsh[:1])     # wrong dimension
    assert lib.gpar_predict_mean(ctx.h, C.byref(pr), th.ctypes.data, 0, ts.ctypes.data,
                                 ts.ctypes.data, 2, ts.ctypes.data) == 1
    assert lib.gpar_predict_mean(ctx.h, C.byref(pr), th.ctypes.data, 30, ts.ctypes.data,
                                 ts.ctypes.data, 1, ts.ctypes.data) == 1             # ldvs < d
    assert lib.gpar_predict_mean(ctx.h, None, th.ctypes.data, 30, ts.ctypes.data,
                                 ts.ctypes.data, 2, ts.ctypes.data) == 1
    hp.close()
