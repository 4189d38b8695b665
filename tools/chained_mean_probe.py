"""Time the ordered part of the chained sweep with and without the mean-only path.

    python tools/chained_mean_probe.py --config eeg [--sweeps 20] [--warmup 2] [--commit SHA]

Builds every GPAR output's posterior with a short fit (as bench.py's one-rank chained measurement
does: the sweep's cost does not depend on theta), then runs shard.chained_predictions over all
outputs on one process, alternating a sweep whose ordered loop runs the full prediction
(Posterior.predict, prepared one output ahead with Posterior.prepare) with one whose ordered loop
runs the mean alone (Posterior.predict_mean / prepare_mean).  The ordered part is timed with a
synchronised wall clock: from the sweep's start to the end of its last ordered prediction; the
mean-first sweep's std calls come after that point and are skipped here.  Prints one JSON line
with the median ms per chained output of each, and their min / max over the sweeps.

The measurement runs in a child process under a time limit (--limit seconds), so a stuck GPU step
ends the tool instead of hanging it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpar-at-scale_amd", "python"))

CONFIGS = {"eeg": dict(N=100_000, M=512, P=64), "north": dict(N=1_000_000, M=512, P=64),
           "small": dict(N=4_000, M=64, P=6)}


def child(args):
    import numpy as np
    import torch
    import gparatscale as G
    from gparatscale import data as D, shard as S

    cfg = CONFIGS[args.config]
    N, M, P = cfg["N"], cfg["M"], args.outputs or cfg["P"]
    dev = torch.device("cuda", 0)
    ds = D.gpar_dataset(N, P, seed=0, observation_noise=0.8)
    t_d, Y_d, ts_d, Fs_d = (torch.from_numpy(ds[k]).to(dev) for k in ("t", "Y", "t_star", "F_star"))
    outs = list(range(2, P + 1))
    probs, keep = [], []
    for p in outs:
        Z = torch.from_numpy(D.pseudo_inputs(ds["Y"][:, : p - 1], M, seed=p)).to(dev)
        pr, k = G.make_problem(Y_d[:, : p - 1], Z, t_d, Y_d[:, p - 1].contiguous(), "matern52",
                               "matern52", qu_kuu_noise=True)
        probs.append(pr)
        keep.append((k, Z))
    x0 = np.tile([0.0, 0.0, 0.0, 0.0, -2.0], (len(outs), 1))
    post = G.fit_posterior(probs, x0, max_evals=6, g_tol=-1.0, keep=keep)
    idx = {p: i for i, p in enumerate(outs)}
    owners = {p: 0 for p in outs}

    def sweep(mean_first):
        chain = Fs_d.clone()
        mark = {}

        def predict(p, c):
            if mean_first:   # the first std call: the ordered part is over
                if "t" not in mark:
                    torch.cuda.synchronize()
                    mark["t"] = time.perf_counter()
                return None, None
            return post.predict(idx[p], ts_d, c[:, : p - 1])

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mean_first:
            S.chained_predictions(outs, owners, predict, chain,
                                  prepare_fn=lambda p: post.prepare_mean(idx[p], ts_d),
                                  mean_fn=lambda p, c: post.predict_mean(idx[p], ts_d, c[:, : p - 1]))
        else:
            S.chained_predictions(outs, owners, predict, chain,
                                  prepare_fn=lambda p: post.prepare(idx[p], ts_d))
            torch.cuda.synchronize()
            mark["t"] = time.perf_counter()
        return (mark["t"] - t0) * 1e3 / len(outs), chain

    for _ in range(args.warmup):
        _, c_full = sweep(False)
        _, c_mean = sweep(True)
    ms = {False: [], True: []}
    for _ in range(args.sweeps):   # alternating, so drift hits both alike
        for mf in (False, True):
            ms[mf].append(sweep(mf)[0])
    cf, cm = c_full.cpu().numpy(), c_mean.cpu().numpy()
    line = {"tool": "chained_mean_probe", "config": args.config, "N": len(ds["t"]),
            "N_star": len(ds["t_star"]), "M": M, "P": P, "sweeps": args.sweeps,
            "ordered_ms_per_output_full": statistics.median(ms[False]),
            "ordered_ms_per_output_mean": statistics.median(ms[True]),
            "full_min_max": [min(ms[False]), max(ms[False])],
            "mean_min_max": [min(ms[True]), max(ms[True])],
            "chain_max_rel_diff": float(np.abs(cf - cm).max() / np.abs(cf).max()),
            "device": torch.cuda.get_device_name(0), "commit": args.commit}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="eeg", choices=sorted(CONFIGS))
    ap.add_argument("--outputs", type=int, default=0, help="P (default: the config's)")
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=600, help="seconds the measurement may take")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.commit is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                           text=True)
        args.commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", args.config,
           "--outputs", str(args.outputs), "--sweeps", str(args.sweeps), "--warmup", str(args.warmup),
           "--commit", args.commit]
    try:
        return subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        print(f"chained_mean_probe: no result within {args.limit} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
