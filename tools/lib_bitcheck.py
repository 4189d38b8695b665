"""Bit-identity check of two library builds on a workload that runs every gains variant.

    python tools/lib_bitcheck.py run out.npz [section ...]   (the library GPAR_HIP_LIB points at,
                                                       or the in-tree one; sections: headline,
                                                       small, predict; default all)
    python tools/lib_bitcheck.py compare a.npz b.npz  (exit 1 on any differing bit)

Workload (one MI355X): a headline-schedule fit_predict_batch at N = 4e5 + 57 (the auto CU split,
the distance cache, a partial last chunk) over five outputs (the round overlap: compact gains
records with the data filter) and over three outputs (round by round: full records), predictions
on the merged grid (the noise-vector gains), the temporal-only chains' fit + smoothing (gains
without data, with the filtered covariances, with and without a noise vector).  A kernel change
that claims the same arithmetic (r05: the gains' phase 3 fast path) must reproduce every value.

That workload's fits only reach the CU-split pipeline.  small_cases adds a few seconds each of the
other schedules of the batched Gram stage (run_gram_stage) and of the round overlaps, so a change
of the host code that orders the launches is on the path too: the grouped Gram with a full and a
ragged group, the unsplit pipelined stage, the unsplit round overlap with two and three groups,
the two-lane loop, per-output gains (outputs that do not share a time grid), a batch of two
widths (the padding memsets), and the fix_beta stage (q(u), the (dtc, A) entry point).

predict_cases runs every prediction entry point and mode at small sizes (merged grids of several
256-step chunks ending in a short one; M = 30, 70, 140 and one 520; one time kernel per state
dimension): the single-output predictions (analytic fused / unfused, MC on both statistics
branches, path, mean only; host unsorted with coincident and out-of-range test times, device),
q(u) under both Cuu conventions, fit_predict_batch on every route (lanes, staged host inputs,
chains, chain_mean_first, qu_batch off), posteriors predicted in line and prepared,
posterior_rand and the temporal-only predictions with unsorted host test times.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpar-at-scale_amd", "python"))


def small_cases(res, G, D, torch, dev):
    ctx = G.context(0)
    ctx.set_cu_split(-1)   # the auto split: off at these sizes

    def problems(n, ms, outs, seed, own_t=False):
        ds = D.gpar_dataset(n, max(outs), seed=seed, observation_noise=0.8, n_star=4_000)
        Y = torch.from_numpy(ds["Y"]).to(dev)
        t = torch.from_numpy(ds["t"]).to(dev)
        probs, keep = [], []
        for p, m in zip(outs, ms):
            Z = torch.from_numpy(D.pseudo_inputs(ds["Y"][:, : p - 1], m, seed=p)).to(dev)
            tp = t.clone() if own_t else t   # own_t: equal grids the library cannot know are equal
            pr, k = G.make_problem(Y[:, : p - 1], Z, tp, Y[:, p - 1].contiguous(), "eq", "matern52",
                                   qu_kuu_noise=True)
            probs.append(pr)
            keep.append((k, Z, tp))
        ts = torch.from_numpy(ds["t_star"]).to(dev)
        Fs = torch.from_numpy(ds["F_star"]).to(dev)
        return probs, keep, ts, [Fs[:, : p - 1] for p in outs], ds

    def case(tag, batch, max_evals, knobs=(), lanes=1):
        probs, _, ts, Vs, _ = batch
        th = np.tile([[1.1, 0.9, 1.3, 0.8, 0.3]], (len(probs), 1))
        x0 = np.tile([0.0, 0.0, 0.0, 0.0, -2.0], (len(probs), 1))
        old = {k: ctx.schedule(k) for k, _ in knobs}
        try:
            for k, v in knobs:
                ctx.set_schedule(k, v)
            ctx.set_lanes(lanes)
            res[tag + "_obj"] = np.asarray(G.dtc_objective_batch(probs, th))
            fr, means, stds = G.fit_predict_batch(probs, x0, ts, Vs, max_evals=max_evals, g_tol=-1.0)
        finally:
            ctx.set_lanes(1)
            for k, v in old.items():
                ctx.set_schedule(k, v)
        res[tag + "_theta"], res[tag + "_nlml"] = fr.theta, fr.nlml
        res[tag + "_mean"] = np.array([m.cpu().numpy() for m in means])
        res[tag + "_std"] = np.array([s.cpu().numpy() for s in stds])

    five = problems(30_000, [128] * 5, [2, 3, 5, 9, 17], seed=3)
    case("grp_auto", five, 8, [("gram_group", -1)])    # one grouped Gram of five
    case("grp_2", five, 8, [("gram_group", 2)])        # groups of 2 + 2 + 1
    case("grp_off", five, 8, [("gram_group", 0)])      # the unsplit pipelined stage
    case("lanes2", five, 8, lanes=2)                   # the two-lane loop
    six = problems(20_000, [512] * 6, [2, 3, 5, 9, 12, 17], seed=4)
    case("ovu_2grp", six, 12, [("overlap_group", 0)])  # unsplit round overlap, two groups of 3
    case("ovu_3grp", six, 12, [("overlap_group", 2)])  # three groups of 2
    own = problems(30_000, [128] * 2, [3, 9], seed=6, own_t=True)
    case("own_t_grp", own, 8)                          # per-output gains under the grouped Gram
    case("own_t_lane", own, 8, [("gram_group", 0)])    # ... and output by output on one lane
    case("mixed_m", problems(30_000, [128, 192, 128], [2, 5, 9], seed=7), 8)   # padded G / r slots
    # fix_beta: q(u) on the noise-free Cuu and the (dtc, A) entry point, one output
    ds = five[4]
    V, y, t = ds["Y"][:, :4].T.copy(), ds["Y"][:, 4].copy(), ds["t"]
    Z = D.pseudo_inputs(ds["Y"][:, :4], 128, seed=5).T.copy()
    th1 = [1.1, 0.9, 1.3, 0.8, 0.3]
    res["qu_me"], res["qu_cov"], res["qu_U"] = G.compute_q_u(V, Z, t, y, th1, "eq", "matern52")
    res["dtcA_val"], res["dtcA_A"] = G.compute_gpar_dtc_objective(V, Z, t, y, th1, "eq", "matern52",
                                                                  return_A=True)


def predict_cases(res, G, D, torch, dev):
    ctx = G.context(0)
    ctx.set_cu_split(-1)
    th = [1.1, 0.9, 1.3, 0.8, 0.3]

    def knobs(pairs):
        old = {k: ctx.schedule(k) for k, _ in pairs}
        for k, v in pairs:
            ctx.set_schedule(k, v)
        return old

    def restore(old):
        for k, v in old.items():
            ctx.set_schedule(k, v)

    def unsorted_times(ds, n_star, seed):
        """n_star host test times, shuffled: some equal to training times, some repeated, some
        before the first and after the last training time."""
        rng = np.random.default_rng(seed)
        t, ts = ds["t"], ds["t_star"][:n_star].copy()
        ts[5:25] = t[rng.choice(len(t), 20, replace=False)]      # coincident with training points
        ts[30:40] = ts[40:50]                                    # repeated test times
        ts[50:60] = t[0] - np.arange(1, 11) * (t[1] - t[0])      # before the training range
        ts[60:70] = t[-1] + np.arange(1, 11) * (t[1] - t[0])     # after it
        perm = rng.permutation(n_star)
        return ts[perm], perm

    # ---- single-output entries: one case per time kernel, n = 900 / 3000, n* = 200 / 333
    for tag, n, n_star, m, d, tk in (("p12", 900, 200, 30, 2, "matern12"),
                                     ("p32", 3000, 333, 70, 4, "matern32"),
                                     ("p52", 900, 333, 140, 3, "matern52")):
        ds = D.gpar_dataset(n, d + 1, seed=11, observation_noise=0.8, n_star=n_star)
        V, y, t = ds["Y"][:, :d].T.copy(), ds["Y"][:, d].copy(), ds["t"]
        Z = D.pseudo_inputs(ds["Y"][:, :d], m, seed=d).T.copy()
        ts, Vs = ds["t_star"], ds["F_star"][:, :d].T.copy()
        tu, perm = unsorted_times(ds, n_star, seed=n)
        Vu = Vs[:, perm].copy()
        kw = dict(out_kernel="matern52", time_kernel=tk, qu_kuu_noise=True)
        res[tag + "_an_mean"], res[tag + "_an_std"] = G.predict_scaled(V, Z, t, y, th, ts, Vs, **kw)
        old = knobs([("predict_fused", 0)])
        try:
            res[tag + "_unf_mean"], res[tag + "_unf_std"] = G.predict_scaled(V, Z, t, y, th, ts, Vs, **kw)
        finally:
            restore(old)
        for S in (8, 200):   # statistics in the GEMM epilogue / over column blocks
            res[f"{tag}_mc{S}_mean"], res[f"{tag}_mc{S}_std"] = G.predict_scaled(
                V, Z, t, y, th, ts, Vs, mode="mc", samples=S, seed=7, **kw)
        res[tag + "_path_mean"], res[tag + "_path_std"] = G.predict_scaled(
            V, Z, t, y, th, ts, Vs, mode="path", samples=8, seed=7, **kw)
        res[tag + "_uns_mean"], res[tag + "_uns_std"] = G.predict_scaled(V, Z, t, y, th, tu, Vu, **kw)
        res[tag + "_mean_uns"] = G.predict_mean_scaled(V, Z, t, y, th, tu, Vu, **kw)
        dV, dZ = torch.from_numpy(V.T.copy()).to(dev), torch.from_numpy(Z.T.copy()).to(dev)
        dt, dy = torch.from_numpy(t).to(dev), torch.from_numpy(y).to(dev)
        dts, dVs = torch.from_numpy(ts).to(dev), torch.from_numpy(Vs.T.copy()).to(dev)
        mn, sd = G.predict_scaled(dV, dZ, dt, dy, th, dts, dVs, **kw)
        res[tag + "_dev_mean"], res[tag + "_dev_std"] = mn.cpu().numpy(), sd.cpu().numpy()
        res[tag + "_mean_dev"] = G.predict_mean_scaled(dV, dZ, dt, dy, th, dts, dVs, **kw).cpu().numpy()
        for qn in (False, True):
            try:
                me, cov, U = G.compute_q_u(V, Z, t, y, th, "matern52", tk, qu_kuu_noise=qn)
            except G.PosDefException:   # the noise-free Cuu may fail: then under both libraries
                me = cov = U = np.zeros(0)
            res[f"{tag}_qu{int(qn)}_me"], res[f"{tag}_qu{int(qn)}_cov"], res[f"{tag}_qu{int(qn)}_U"] = me, cov, U
    # M = 520: no fused tiling, so the default knobs take the unfused tail
    ds = D.gpar_dataset(900, 4, seed=12, observation_noise=0.8, n_star=200)
    V, y, t = ds["Y"][:, :3].T.copy(), ds["Y"][:, 3].copy(), ds["t"]
    Z = D.pseudo_inputs(ds["Y"][:, :3], 520, seed=3).T.copy()
    res["m520_mean"], res["m520_std"] = G.predict_scaled(
        V, Z, t, y, th, ds["t_star"], ds["F_star"][:, :3].T.copy(), qu_kuu_noise=True)

    # ---- batched fit + predict and posteriors: three outputs of different D and M
    n, n_star, outs, ms = 3000, 333, [2, 4, 7], [30, 70, 140]
    ds = D.gpar_dataset(n, max(outs), seed=13, observation_noise=0.8, n_star=n_star)
    x0 = np.tile([0.0, 0.0, 0.0, 0.0, -2.0], (len(outs), 1))
    Zs = [D.pseudo_inputs(ds["Y"][:, : p - 1], m, seed=p) for p, m in zip(outs, ms)]
    fit = dict(max_evals=30, g_tol=-1.0)

    def put(tag, fr, means, stds):
        res[tag + "_theta"], res[tag + "_nlml"] = fr.theta, fr.nlml
        res[tag + "_mean"] = np.array([m.cpu().numpy() if torch.is_tensor(m) else m for m in means])
        res[tag + "_std"] = np.array([s.cpu().numpy() if torch.is_tensor(s) else s for s in stds])

    Y = torch.from_numpy(ds["Y"]).to(dev)
    t = torch.from_numpy(ds["t"]).to(dev)
    ts = torch.from_numpy(ds["t_star"]).to(dev)
    Fs = torch.from_numpy(ds["F_star"]).to(dev)
    dprobs, dkeep = [], G.api._Keep()
    for p, Z in zip(outs, Zs):
        pr, _ = G.make_problem(Y[:, : p - 1], torch.from_numpy(Z).to(dev), t, Y[:, p - 1].contiguous(),
                               "matern52", "matern52", qu_kuu_noise=True, keep=dkeep)
        dprobs.append(pr)
    dVs = [Fs[:, : p - 1] for p in outs]
    hprobs, hkeep = [], G.api._Keep()
    for p, Z in zip(outs, Zs):
        pr, _ = G.make_problem(ds["Y"][:, : p - 1].T.copy(), Z.T.copy(), ds["t"], ds["Y"][:, p - 1].copy(),
                               "matern52", "matern52", qu_kuu_noise=True, keep=hkeep)
        hprobs.append(pr)
    tu, perm = unsorted_times(ds, n_star, seed=5)
    hVs = [ds["F_star"][perm, : p - 1].T.copy() for p in outs]

    for tag, pairs in (("fp_lanes2", [("predict_lanes", 2)]), ("fp_lanes1", [("predict_lanes", 1)]),
                       ("fp_qub0", [("qu_batch", 0)])):
        old = knobs(pairs)
        try:
            put(tag, *G.fit_predict_batch(dprobs, x0, ts, dVs, **fit))
        finally:
            restore(old)
    put("fp_host", *G.fit_predict_batch(hprobs, x0, tu, hVs, **fit))
    cols = [p - 1 for p in outs]   # output p's mean into column p - 1, read by the later outputs
    chain = ds["F_star"][perm].copy()
    put("fp_hchain", *G.fit_predict_batch(hprobs, x0, tu, [None] * len(outs), chain=chain,
                                          chain_cols=cols, **fit))
    res["fp_hchain_chain"] = chain
    for k in (0, 1):
        old = knobs([("chain_mean_first", k)])
        try:
            dchain = Fs.clone()
            put(f"fp_dchain{k}", *G.fit_predict_batch(dprobs, x0, ts, [None] * len(outs), chain=dchain,
                                                      chain_cols=cols, **fit))
            res[f"fp_dchain{k}_chain"] = dchain.cpu().numpy()
        finally:
            restore(old)
    post = G.fit_posterior(dprobs, x0, keep=dkeep, **fit)
    res["post_theta"], res["post_nlml"] = post.fit.theta, post.fit.nlml
    for i in range(len(outs)):
        mn, sd = post.predict(i, ts, dVs[i])
        res[f"post{i}_mean"], res[f"post{i}_std"] = mn.cpu().numpy(), sd.cpu().numpy()
        res[f"post{i}_mean_only"] = post.predict_mean(i, ts, dVs[i]).cpu().numpy()
        post.prepare(i, ts)
        mn, sd = post.predict(i, ts, dVs[i])
        res[f"post{i}_prep_mean"], res[f"post{i}_prep_std"] = mn.cpu().numpy(), sd.cpu().numpy()
        post.prepare_mean(i, ts)
        res[f"post{i}_prep_mean_only"] = post.predict_mean(i, ts, dVs[i]).cpu().numpy()
    post.close()

    # ---- temporal-only: posterior_rand, and the chains' predictions at unsorted host test times
    res["prand"] = G.posterior_rand(ds["t"], ds["Y"][:, 0].copy(), [1.3, 0.8, 0.3], "matern32",
                                    samples=8, seed=3)
    th_s, m_s, v_s = G.get_sde_predictions(ds["t"], ds["Y"][:, :2].T.copy(), tu, "matern32",
                                           0.0, 0.0, -2.0, max_evals=30, g_tol=-1.0)
    res["sde_uns_theta"], res["sde_uns_mean"], res["sde_uns_var"] = th_s, m_s, v_s
    th_s, m_s, v_s = G.get_sde_predictions(ds["t"], ds["Y"][:, :2].T.copy(), ds["t_star"], "matern52",
                                           0.0, 0.0, -2.0, max_evals=30, g_tol=-1.0)
    res["sde_srt_theta"], res["sde_srt_mean"], res["sde_srt_var"] = th_s, m_s, v_s


def run(out, sections=("headline", "small", "predict")):
    import torch
    import gparatscale as G
    from gparatscale import data as D
    dev = torch.device("cuda", 0)
    res = {}
    if "headline" in sections:
        headline(res, G, D, torch, dev)
    if "small" in sections:
        small_cases(res, G, D, torch, dev)
    if "predict" in sections:
        predict_cases(res, G, D, torch, dev)
    np.savez(out, **res)
    print("saved", out, sorted(res))


def headline(res, G, D, torch, dev):
    N, M, NS = 400_057, 512, 30_011
    ds = D.gpar_dataset(N, 34, seed=5, observation_noise=0.8, n_star=NS)
    Y = torch.from_numpy(ds["Y"]).to(dev)
    t = torch.from_numpy(ds["t"]).to(dev)
    ts = torch.from_numpy(ds["t_star"]).to(dev)
    Fs = torch.from_numpy(ds["F_star"]).to(dev)
    for tag, outs in (("ov", [2, 3, 9, 17, 33]), ("rr", [4, 12, 25])):
        probs, keep = [], []
        for p in outs:
            Z = torch.from_numpy(D.pseudo_inputs(ds["Y"][:, : p - 1], M, seed=p)).to(dev)
            pr, k = G.make_problem(Y[:, : p - 1], Z, t, Y[:, p - 1].contiguous(), qu_kuu_noise=True)
            probs.append(pr)
            keep.append((k, Z))
        x0 = np.tile([0.0, 0.0, 0.0, 0.0, -2.0], (len(outs), 1))
        fr, means, stds = G.fit_predict_batch(probs, x0, ts, [Fs[:, : p - 1] for p in outs],
                                              max_evals=8, g_tol=-1.0)
        res[tag + "_theta"] = fr.theta
        res[tag + "_nlml"] = fr.nlml
        res[tag + "_mean"] = np.array([m.cpu().numpy() for m in means])
        res[tag + "_std"] = np.array([s.cpu().numpy() for s in stds])
    th, m1, v1 = G.get_sde_predictions_device(t, Y[:, :3].T.contiguous(), ts, "matern32",
                                              (0.0, 0.0, -2.0), max_evals=10)
    res["sde_theta"], res["sde_mean"], res["sde_var"] = th, m1.cpu().numpy(), v1.cpu().numpy()
    th5 = np.tile([[1.3, 0.8, 0.1]], (2, 1))
    th_h, y_h = ds["t"][:20_011], ds["Y"][:20_011, :2].T.copy()
    noise = np.where(np.arange(20_011) % 3 == 0, 1e10, -1.0)
    sm, sv = G.lgssm_smooth_batch(th_h, y_h, th5, "matern52", noise=noise)
    res["smooth_noise_mean"], res["smooth_noise_var"] = sm, sv
    sm, sv = G.lgssm_smooth_batch(th_h, y_h, th5, "matern52")
    res["smooth_mean"], res["smooth_var"] = sm, sv
    res["logpdf"] = G.lgssm_logpdf_batch(th_h, y_h, th5, "matern52")


def compare(a, b, tols):
    """tols: {key prefix: rtol} for outputs a change is allowed to move within rounding (a new
    summation order); every other output must be bit-identical."""
    A, B = np.load(a), np.load(b)
    bad = 0
    for k in sorted(set(A.files) ^ set(B.files)):
        print(f"{k:20s} in one file only  FAIL")
        bad += 1
    for k in sorted(set(A.files) & set(B.files)):
        same = np.array_equal(A[k], B[k])
        diff = np.max(np.abs(A[k] - B[k]) / np.maximum(np.abs(A[k]), 1e-300)) if not same else 0.0
        tol = next((v for p, v in tols.items() if k.startswith(p)), None)
        ok = same or (tol is not None and diff <= tol)
        verdict = "bit-identical" if same else f"max rel {diff:.3e} (allowed {tol})"
        print(f"{k:20s} {verdict}{'' if ok else '  FAIL'}")
        bad += not ok
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], tuple(sys.argv[3:]) or ("headline", "small", "predict"))
    else:
        tols = dict((kv.split("=")[0], float(kv.split("=")[1])) for kv in sys.argv[4:])
        compare(sys.argv[2], sys.argv[3], tols)
