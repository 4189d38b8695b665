"""Sample-chained prediction on the GPU (gpar_predict_samples, k_kfu_samples.hip): path mode with
test inputs of each sample's own and the samples returned, so a joint draw of GPAR's outputs can
feed sample s of the earlier outputs into sample s of the later ones.

Checked here:
  * every sample replayed through the numpy restatement (tests/_sample_chain_ref.py) fed the
    device's own draws (mc_normals / path_normals), at test_gpu_path.py's prediction tolerances
    (rtol 1e-7, atol 1e-9 max|ref|; std rtol 1e-6), one variation at a time over the output kernel,
    the shared / per-sample column split, M, N* and S;
  * equal inputs for every sample give mode="path";
  * samples are independent of each other's inputs, calls are deterministic, host and device
    memory and in-place chain views give the same bits;
  * Posterior.predict_samples / sample_chain;
  * argument errors."""
import functools

import numpy as np
import pytest

from oracle import gpar_oracle as O
from _sample_chain_ref import _ref_samples

pytestmark = pytest.mark.gpu
G = pytest.importorskip("gparatscale")

THETA = (1.3, 0.9, 0.8, 1.1, 0.2)
SEED = 77


@functools.lru_cache(maxsize=None)
def _data(D=2, M=30, ns=150, unsorted=False):
    """test_gpu_path.py's _gpar_case shapes (n = 600: more than two 256-step chunks), for output
    D + 1 of a (D + 1)-output synthetic GPAR."""
    t, Y = O.synthetic_gpar(600, D + 1, seed=21, noise=0.3)
    V = np.ascontiguousarray(Y[:, :D].T)
    Z = O.pick_pseudo_inputs(V, M, 5)
    y = Y[:, D].copy()
    rng = np.random.default_rng(4)
    ts = np.sort(rng.uniform(t[0], t[-1], ns))
    if unsorted:   # some test times equal to training times, then out of order
        hit = rng.choice(ns, size=min(10, ns), replace=False)
        ts[hit] = t[rng.choice(len(t), size=len(hit), replace=False)]
        ts = ts[rng.permutation(ns)]
    Vs = np.vstack([np.interp(ts, t, V[q]) for q in range(D)])
    for a in (V, Z, t, y, ts, Vs):
        a.setflags(write=False)
    return V, Z, t, y, ts, Vs


def _split(Vs, d_sh, d_sa, S, jitter=0.1, seed=11):
    """shared d_sh x N* and per-sample S x N* x d_sa inputs: V* plus jitter * normals per sample"""
    ns = Vs.shape[1]
    shared = Vs[:d_sh].copy() if d_sh else None
    samp = None
    if d_sa:
        rng = np.random.default_rng(seed)
        samp = Vs[d_sh:].T[None] + jitter * rng.standard_normal((S, ns, d_sa))
    return shared, samp


def _draws(S, M, nt, seed, time_kernel="matern52"):
    sd = {"matern12": 1, "matern32": 2, "matern52": 3}[time_kernel]
    return G.mc_normals(S, M, seed).T, G.path_normals(S, nt, sd + 1, seed)


def _close(got, ref, rtol):
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=1e-9 * np.abs(ref).max())


# one variation of the base case at a time: (out_kernel, d_sh, d_sa, M, N*, S, qu_noise, unsorted)
BASE = ("matern52", 1, 1, 30, 150, 5, False, False)
CASES = {
    "base": BASE,
    # output kernel: matern12 takes the direct-difference kernel
    "matern12": ("matern12", 1, 1, 30, 150, 5, False, False),
    "matern32": ("matern32", 1, 1, 30, 150, 5, False, False),
    "eq": ("eq", 1, 1, 30, 150, 5, True, False),
    # the column split; (15, 3) crosses a 16-wide K-step, (35, 36) the 32-dimension staging chunk
    # of either part (the z tile is then restaged per sample)
    "d=2+0": ("matern52", 2, 0, 30, 150, 5, False, False),
    "d=0+2": ("matern52", 0, 2, 30, 150, 5, False, False),
    "d=15+3": ("matern52", 15, 3, 30, 150, 5, False, False),
    "d=35+36": ("matern52", 35, 36, 30, 150, 5, False, False),
    "matern12,d=2+0": ("matern12", 2, 0, 30, 150, 5, False, False),
    "matern12,d=0+2": ("matern12", 0, 2, 30, 150, 5, False, False),
    # two 16-dimension slices per part and two 256-column tiles of the direct kernel
    "matern12,d=18+17,M=300": ("matern12", 18, 17, 300, 150, 5, True, False),
    # a second column tile, and a 256-group centre boundary
    "M=130": ("matern52", 1, 1, 130, 150, 5, True, False),
    "M=300": ("matern52", 1, 1, 300, 150, 5, True, False),
    # the row-tile edge
    "N*=1": ("matern52", 1, 1, 30, 1, 5, False, False),
    "N*=129": ("matern52", 1, 1, 30, 129, 5, False, False),
    # S = 130: past one 128-column block of the training rows' GEMM
    "S=1": ("matern52", 1, 1, 30, 150, 1, False, False),
    "S=130": ("matern52", 1, 1, 30, 150, 130, False, False),
    # the perm gather and the caller-order delivery
    "unsorted": ("matern52", 1, 1, 30, 150, 5, False, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_samples_replay_through_the_oracle(case):
    ok, d_sh, d_sa, M, ns, S, qu_noise, unsorted = CASES[case]
    V, Z, t, y, ts, Vs = _data(d_sh + d_sa, M, ns, unsorted)
    shared, samp = _split(Vs, d_sh, d_sa, S)
    F, mean, std = G.predict_samples_scaled(V, Z, t, y, THETA, ts, shared, samp, samples=S,
                                            seed=SEED, out_kernel=ok, qu_kuu_noise=qu_noise)
    xi_u, xi_p = _draws(S, M, len(t) + ns, SEED)
    Fr, rm, rs = _ref_samples(V, Z, t, y, ts, shared, samp, THETA, xi_u, xi_p, out_kernel=ok,
                              qu_kuu_noise=qu_noise)
    assert F.shape == (S, ns)
    print(f"{case}: max|dF| = {np.abs(F - Fr).max():.3e} (max|F| = {np.abs(Fr).max():.3e}), "
          f"max|dmean| = {np.abs(mean - rm).max():.3e}")
    for s in range(S):
        _close(F[s], Fr[s], 1e-7)
    _close(mean, rm, 1e-7)
    if S == 1:   # the Bessel std of one sample is 0 / 0, as numpy's ddof = 1
        assert np.all(np.isnan(std)) and np.all(np.isnan(rs))
    else:
        _close(std, rs, 1e-6)


@pytest.mark.parametrize("d_sh", [1, 0])
def test_equal_inputs_give_path_mode(d_sh):
    V, Z, t, y, ts, Vs = _data()
    S = 8
    shared, samp = _split(Vs, d_sh, 2 - d_sh, S, jitter=0.0)
    F, mean, std = G.predict_samples_scaled(V, Z, t, y, THETA, ts, shared, samp, seed=SEED)
    pm, ps = G.predict_scaled(V, Z, t, y, THETA, ts, Vs, mode="path", samples=S, seed=SEED)
    _close(mean, pm, 1e-7)
    _close(std, ps, 1e-6)
    np.testing.assert_allclose(F.mean(0), mean, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(F.std(0, ddof=1), std, rtol=1e-12, atol=1e-14)


def test_samples_are_independent_and_calls_deterministic():
    V, Z, t, y, ts, Vs = _data()
    S = 5
    shared, samp = _split(Vs, 1, 1, S)
    call = lambda sa, **kw: G.predict_samples_scaled(V, Z, t, y, THETA, ts, shared, sa, seed=SEED, **kw)
    F0, m0, s0 = call(samp)
    F1, m1, s1 = call(samp)
    assert np.array_equal(F0, F1) and np.array_equal(m0, m1) and np.array_equal(s0, s1)
    samp2 = samp.copy()
    samp2[3] += 0.25
    F2, _, _ = call(samp2)
    others = [0, 1, 2, 4]
    assert np.array_equal(F2[others], F0[others])
    assert np.abs(F2[3] - F0[3]).max() > 1e-6
    # fewer samples: the first ones keep their values
    F3, _, _ = call(samp[:3])
    assert np.array_equal(F3, F0[:3])


def test_device_host_and_in_place_views_agree_bitwise():
    import torch
    V, Z, t, y, ts, Vs = _data()
    S = 5
    shared, samp = _split(Vs, 1, 1, S)
    Fh, mh, sh = G.predict_samples_scaled(V, Z, t, y, THETA, ts, shared, samp, seed=SEED)
    dev = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    Vd, Zd, td, yd, tsd = dev(V.T), dev(Z.T), dev(t), dev(y), dev(ts)
    shd, sad = dev(shared.T), dev(samp)
    Fd, md, sd = G.predict_samples_scaled(Vd, Zd, td, yd, THETA, tsd, shd, sad, seed=SEED)
    assert np.array_equal(Fd.cpu().numpy(), Fh)
    assert np.array_equal(md.cpu().numpy(), mh) and np.array_equal(sd.cpu().numpy(), sh)
    # a column-prefix view of a wider tensor, the output written to a column of that tensor
    wide = torch.full((S, len(ts), 3), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :, :1] = sad
    Fw, mw, sw = G.predict_samples_scaled(Vd, Zd, td, yd, THETA, tsd, shd, wide[:, :, :1],
                                          seed=SEED, out=wide[:, :, 1])
    assert Fw.data_ptr() == wide[:, :, 1].data_ptr()
    assert torch.equal(wide[:, :, 1], Fd) and torch.equal(mw, md) and torch.equal(sw, sd)
    assert torch.equal(wide[:, :, :1], sad) and bool(torch.isnan(wide[:, :, 2]).all())
    # the same on the host
    wh = np.full((S, len(ts), 3), np.nan)
    wh[:, :, :1] = samp
    Fv, mv, sv = G.predict_samples_scaled(V, Z, t, y, THETA, ts, shared, wh[:, :, :1], seed=SEED,
                                          out=wh[:, :, 1])
    assert np.array_equal(wh[:, :, 1], Fh) and np.array_equal(mv, mh) and np.array_equal(sv, sh)
    assert np.array_equal(wh[:, :, :1], samp) and np.all(np.isnan(wh[:, :, 2]))


@functools.lru_cache(maxsize=None)
def _posterior():
    """3 outputs in the GPAR ordering on the device: output i reads the given column and outputs
    0..i-1 (D_i = 1 + i)."""
    import torch
    t, Y = O.synthetic_gpar(600, 4, seed=21, noise=0.3)
    ts = np.sort(np.random.default_rng(4).uniform(t[0], t[-1], 150))
    Yd = torch.from_numpy(Y).cuda()
    td, tsd = torch.from_numpy(t).cuda(), torch.from_numpy(ts).cuda()
    given = torch.from_numpy(np.interp(ts, t, Y[:, 0])).cuda().reshape(-1, 1)
    probs, keep, Zs = [], G.api._Keep(), []
    for i in range(3):
        Z = torch.from_numpy(np.ascontiguousarray(O.pick_pseudo_inputs(Y[:, :1 + i].T, 30, 5 + i).T)).cuda()
        pr, k = G.make_problem(Yd[:, :1 + i], Z, td, Yd[:, 1 + i].contiguous())
        probs.append(pr)
        keep.append(k)
        Zs.append(Z)
    x0 = np.tile([0.0, 0.0, 0.0, 0.0, -2.0], (3, 1))
    post = G.fit_posterior(probs, x0, max_evals=12, g_tol=-1.0, keep=keep)
    return post, Yd, td, tsd, given, Zs


def test_posterior_predict_samples_equals_the_direct_call():
    import torch
    post, Yd, td, tsd, given, Zs = _posterior()
    S, i = 6, 1
    samp = (given + 0.3).reshape(1, -1, 1) + 0.1 * torch.randn(
        (S, given.shape[0], 1), dtype=torch.float64, device="cuda",
        generator=torch.Generator("cuda").manual_seed(3))
    ref = G.predict_samples_scaled(Yd[:, :2], Zs[i], td, Yd[:, 2].contiguous(), post.theta[i], tsd,
                                   given, samp, seed=9)
    got = post.predict_samples(i, tsd, given, samp, seed=9)
    post.prepare(i, tsd)
    prepared = post.predict_samples(i, tsd, given, samp, seed=9)
    for a, b, c in zip(got, ref, prepared):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-12, atol=1e-14)
        assert torch.equal(a, c)


def test_sample_chain_is_the_loop_of_predict_samples():
    import torch
    post, Yd, td, tsd, given, Zs = _posterior()
    S, seed = 6, 40
    chain, means, stds = post.sample_chain(tsd, given, S, seed=seed)
    assert tuple(chain.shape) == (S, tsd.numel(), 3) and len(means) == len(stds) == 3
    prev = None
    for i in range(3):
        F, m, s = post.predict_samples(i, tsd, given, prev, samples=S, seed=seed + i)
        assert torch.equal(chain[:, :, i], F) and torch.equal(means[i], m) and torch.equal(stds[i], s)
        prev = F.unsqueeze(2) if prev is None else torch.cat([prev, F.unsqueeze(2)], dim=2)
    # the first output has no sampled inputs: its samples are mode="path"'s
    pm, ps = post.predict(0, tsd, given, mode="path", samples=S, seed=seed)
    _close(means[0].cpu().numpy(), pm.cpu().numpy(), 1e-7)
    _close(stds[0].cpu().numpy(), ps.cpu().numpy(), 1e-6)
    # later outputs see different inputs per sample: their spread across samples is real
    assert float(chain[:, :, :2].std(0).min()) > 0.0


def test_arguments():
    import ctypes as C
    import torch
    V, Z, t, y, ts, Vs = _data()
    S = 4
    shared, samp = _split(Vs, 1, 1, S)
    call = lambda sh, sa, **kw: G.predict_samples_scaled(V, Z, t, y, THETA, ts, sh, sa, **kw)
    with pytest.raises(G.DomainError):      # d_shared > d
        call(np.vstack([Vs, Vs[:1]]), None, samples=S)
    with pytest.raises(G.DomainError):      # null v_samp with d_sa > 0
        call(shared, None, samples=S)
    with pytest.raises(G.DomainError):      # columns do not add up to D
        call(Vs, samp)
    with pytest.raises(G.DomainError):      # samples < 1
        call(Vs, None, samples=0)
    with pytest.raises(G.DomainError):      # N* mismatch
        call(shared[:, :-1], samp)
    with pytest.raises(G.DomainError):
        call(shared, samp[:, :-1])
    with pytest.raises(G.DomainError):      # out of another shape
        call(shared, samp, out=np.zeros((S, len(ts) + 1)))
    with pytest.raises(G.Unsupported):      # the time kernel needs a state-space form
        call(shared, samp, time_kernel="eq")
    # the C-ABI's own checks, with everything else valid: d_shared < 0 and strides too small
    lib, ctx = G.load(), G.context(0)
    p, keep = G.make_problem(V, Z, t, y)
    th = np.array(THETA)
    ns = len(ts)
    sh = np.ascontiguousarray(shared.T)
    F, mean, std = np.zeros((S, ns)), np.zeros(ns), np.zeros(ns)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def raw(d_sh=1, ldvs=1, ld_s=ns, ld_r=1, ldf_s=ns, ldf_r=1, samples=S):
        return lib.gpar_predict_samples(ctx.h, C.byref(p), ptr(th), ns, ptr(ts.copy()), ptr(sh), ldvs,
                                        d_sh, ptr(samp), ld_s, ld_r, samples, 1, ptr(F), ldf_s,
                                        ldf_r, ptr(mean), ptr(std))
    assert raw() == 0
    for bad in (dict(d_sh=-1), dict(d_sh=3), dict(ldvs=0), dict(ld_r=0), dict(ld_s=ns - 1),
                dict(ldf_r=0), dict(ldf_s=ns - 1), dict(samples=0), dict(samples=65537)):
        with pytest.raises(G.DomainError):
            ctx.check(raw(**bad))
    # device tensors: lengths are checked on the Python side (the C side cannot see them)
    dev = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()
    Vd, Zd, td, yd, tsd = dev(V.T), dev(Z.T), dev(t), dev(y), dev(ts)
    shd, sad = dev(shared.T), dev(samp)
    dcall = lambda sh_, sa_, **kw: G.predict_samples_scaled(Vd, Zd, td, yd, THETA, tsd, sh_, sa_, **kw)
    with pytest.raises(G.DomainError):
        dcall(shd[:-1], sad)
    with pytest.raises(G.DomainError):
        dcall(shd, sad[:, :-1])
    with pytest.raises(G.DomainError):
        dcall(shd, sad, samples=S + 1)
    with pytest.raises(G.DomainError):
        dcall(shd, sad, out=torch.empty((S, len(ts) - 1), dtype=torch.float64, device="cuda"))
    with pytest.raises(G.DomainError):
        dcall(shd, sad.float())
