"""The chained driver's mean-first schedule (knob "chain_mean_first"): gpar_fit_predict_chain runs
only each output's mean-only prediction in chain order and the full predictions, which supply the
stds, on the side lane.  Data of tests/test_gpu_driver.py's chained test (n = 400, P = 5, N* = 90,
M = 20, 25 evaluations); predictions against the serial oracle chain at its tolerance
(_close(1e-7)); the schedule against its serialized twin, and the cases the knob must not touch
(MC mode, host memory), bit for bit; and a one-process chained_sweep_blocks over posterior objects
with mean_fn against the one-call driver, bit for bit."""
import numpy as np
import pytest

from oracle import gpar_oracle as O

pytestmark = pytest.mark.gpu
G = pytest.importorskip("gparatscale")

X0 = np.array([0.0, 0.0, 0.0, 0.0, -2.0])
OUTS, M, EV = [2, 3, 4, 5], 20, 25


def _close(got, ref, rtol):
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=rtol * 1e-2 * np.abs(ref).max())


@pytest.fixture(scope="module")
def data():
    t, Y = O.synthetic_gpar(400, 5, seed=43, noise=0.3)
    ts = np.sort(np.random.default_rng(44).uniform(t[0], t[-1], 90))
    F = np.column_stack([np.interp(ts, t, Y[:, q]) for q in range(5)])
    return t, Y, ts, F


@pytest.fixture(scope="module")
def oracle_chain(data):
    """Serial reference chain: output p's inference inputs are [test_y1, pred_y2 .. pred_y(p-1)]."""
    t, Y, ts, F = data
    chain = F[:, :1].copy()
    res = {}
    for p in OUTS:
        V = np.ascontiguousarray(Y[:, : p - 1].T)
        Z = O.pick_pseudo_inputs(V, M, p)
        Vs = np.ascontiguousarray(chain[:, : p - 1].T)
        m, s, th = O.get_gpar_scaled_predictions(V, Z, t, Y[:, p - 1], ts, Vs, log_theta0=X0,
                                                 max_evals=EV, g_tol=-1.0, qu_kuu_noise=True)
        chain = np.column_stack([chain, m])
        res[p] = (th, m, s)
    return res


def _device_problems(data):
    import torch
    dev = torch.device("cuda", 0)
    t, Y, ts, F = data
    t_d, Y_d, ts_d = (torch.from_numpy(a).to(dev) for a in (t, Y, ts))
    probs, keep = [], []
    for p in OUTS:
        Z = torch.from_numpy(O.pick_pseudo_inputs(Y[:, : p - 1].T, M, p).T.copy()).to(dev)
        pr, k = G.make_problem(Y_d[:, : p - 1], Z, t_d, Y_d[:, p - 1].contiguous(), qu_kuu_noise=True)
        probs.append(pr)
        keep.append((k, Z))
    chain = torch.zeros((len(ts), 5), dtype=torch.float64, device=dev)
    chain[:, 0] = torch.from_numpy(F[:, 0]).to(dev)
    return probs, keep, ts_d, chain


def _run(data, knobs, device=True, **kw):
    """One chained gpar_fit_predict_chain under the knobs -> (theta, means, stds, chain) as numpy."""
    ctx = G.context(0)
    old = {k: ctx.schedule(k) for k in knobs}
    try:
        for k, v in knobs.items():
            ctx.set_schedule(k, v)
        if device:
            probs, keep, ts_in, chain = _device_problems(data)
        else:
            t, Y, ts_in, F = data
            probs, keep = [], []
            for p in OUTS:
                V = np.ascontiguousarray(Y[:, : p - 1].T)
                pr, k = G.make_problem(V, O.pick_pseudo_inputs(V, M, p), t, Y[:, p - 1],
                                       qu_kuu_noise=True)
                probs.append(pr)
                keep.append(k)
            chain = np.zeros((len(ts_in), 5))
            chain[:, 0] = F[:, 0]
        fr, means, stds = G.fit_predict_batch(probs, np.tile(X0, (len(OUTS), 1)), ts_in,
                                              [None] * len(OUTS), max_evals=EV, g_tol=-1.0,
                                              chain=chain, chain_cols=[p - 1 for p in OUTS], **kw)
    finally:
        for k, v in old.items():
            ctx.set_schedule(k, v)
    tonp = (lambda a: a.cpu().numpy()) if device else (lambda a: a)
    return fr.theta, [tonp(m) for m in means], [tonp(s) for s in stds], tonp(chain)


@pytest.fixture(scope="module")
def runs(data):
    return {k: _run(data, {"chain_mean_first": k}) for k in (0, 1)}


def test_knob_round_trips_and_defaults_off():
    ctx = G.context(0)
    assert ctx.schedule("chain_mean_first") == 0
    ctx.set_schedule("chain_mean_first", 5)   # a flag: any non-zero value is on
    try:
        assert ctx.schedule("chain_mean_first") == 1
    finally:
        ctx.set_schedule("chain_mean_first", 0)


def test_mean_first_chain_matches_oracle_and_knob_off(data, oracle_chain, runs):
    t, Y, ts, F = data
    th0, m0, s0, c0 = runs[0]
    th1, m1, s1, c1 = runs[1]
    np.testing.assert_array_equal(th1, th0)   # the fit does not see the knob
    for i, p in enumerate(OUTS):
        th, m, s = oracle_chain[p]
        np.testing.assert_allclose(th1[i], th, rtol=1e-6)
        np.testing.assert_array_equal(c1[:, p - 1], m1[i])   # chain column == returned mean
        for what, got, ref in (("mean vs oracle", m1[i], m), ("std vs oracle", s1[i], s),
                               ("mean vs knob 0", m1[i], m0[i]), ("std vs knob 0", s1[i], s0[i])):
            print(f"output {p} {what}: {np.abs(got - ref).max() / np.abs(ref).max():.3e}")
            _close(got, ref, 1e-7)
        assert np.all(s1[i] > 0)
    np.testing.assert_array_equal(c1[:, 0], F[:, 0])


def test_mean_first_equals_its_serialized_twin(data, runs):
    twin = _run(data, {"chain_mean_first": 1, "serialize": 1})
    for a, b in zip(runs[1], twin):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


def test_mean_first_without_batched_q_u_matches(data, runs):
    """qu_batch 0: each lane runs q(u) for itself (the mean's w on the context stream): the same
    kernels on the same inputs as the batched q(u)'s per output."""
    got = _run(data, {"chain_mean_first": 1, "qu_batch": 0})
    for i in range(len(OUTS)):
        _close(got[1][i], runs[1][1][i], 1e-7)
        _close(got[2][i], runs[1][2][i], 1e-7)
        np.testing.assert_array_equal(got[3][:, OUTS[i] - 1], got[1][i])


def test_knob_has_no_effect_in_mc_mode(data):
    a = _run(data, {"chain_mean_first": 0}, mode="mc", samples=64, seed=9)
    b = _run(data, {"chain_mean_first": 1}, mode="mc", samples=64, seed=9)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def test_knob_has_no_effect_on_host_memory_chains(data):
    a = _run(data, {"chain_mean_first": 0}, device=False)
    b = _run(data, {"chain_mean_first": 1}, device=False)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def test_sweep_over_posteriors_with_mean_fn_equals_mean_first_driver(data, runs):
    """chained_sweep_blocks on one process, means by Posterior.predict_mean (prepared one output
    ahead by prepare_mean), stds by Posterior.predict afterwards: the knob-1 driver's means, stds
    and chain bit for bit -- the property tests/test_gpu_posterior.py holds for the full path."""
    from gparatscale import shard as S
    probs, keep, ts_d, chain = _device_problems(data)
    post = G.fit_posterior(probs, np.tile(X0, (len(OUTS), 1)), max_evals=EV, g_tol=-1.0, keep=keep)
    idx = {p: i for i, p in enumerate(OUTS)}
    mine = S.chained_sweep_blocks(
        [[1] + OUTS], lambda p, c: post.predict(idx[p], ts_d, c[:, : p - 1]), chain,
        prepare_fn=lambda p: post.prepare_mean(idx[p], ts_d),
        mean_fn=lambda p, c: post.predict_mean(idx[p], ts_d, c[:, : p - 1]))
    th1, m1, s1, c1 = runs[1]
    np.testing.assert_array_equal(post.theta, th1)
    for i, p in enumerate(OUTS):
        np.testing.assert_array_equal(mine[p][0].cpu().numpy(), m1[i])
        np.testing.assert_array_equal(mine[p][1].cpu().numpy(), s1[i])
    np.testing.assert_array_equal(chain.cpu().numpy(), c1)
    post.close()
