"""Timing of gpar_score_samples against gpar_sample_quantiles and a torch route (needs an MI355X;
not a test).

Sizes: S = 100 samples, levels (0.5, 0.9, 0.95), 10 bins, device memory, at N* = 1e5, P = 64 (eeg's
chain, 5.1 GB) and N* = 1e6, P = 8 (a north rank's block, 6.4 GB).  Per size, 2 warm-up rounds and
10 timed rounds, each round three calls on the same tensor in the same process:

  scorer     HIP-event time of the "score" family (the per-entry pass) and of "score_reduce"
             (gpar_ctx_kernel_stats), min and max over the rounds, the per-entry pass's fraction of
             the bytes bound 8 S N* P / 8 TB/s; gpar_ctx_workspace_bytes (asserted unchanged by a
             repeated call) and torch's peak allocation across the call;
  quantiles  gpar_sample_quantiles with the six band edges of the three levels: the yardstick, the
             same loads and the same sort ("quantile" family);
  torch      torch.sort(F, dim=0) and the same formulas in torch (rank counts, the centred CRPS, the
             band flags, per-output sums), timed with torch events; its peak allocation beyond F.
             When the sort's workspace does not fit beside F the route is reported as such.

Also timed: both scorer paths forced (GPAR_SCORE_PATH) at S = 64, the longest list both can hold,
on a tensor of the same number of entries.

  python tools/score_probe.py [--quick] > profiles/score_probe.txt"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpar-at-scale_amd", "python"))

HBM_BYTES_PER_S = 8.0e12
LEVELS = (0.5, 0.9, 0.95)
BINS = 10


def band_levels():
    q = []
    for l in LEVELS:
        q += [(1 - l) / 2, (1 + l) / 2]
    return tuple(q)


def torch_route(torch, F, y):
    """sort along the samples, then the scorer's definitions; returns (crps mean, inside counts)"""
    S = F.shape[0]
    x, _ = torch.sort(F, dim=0)
    ok = ~torch.isnan(y)
    below = (F < y).sum(0)
    equal = (F == y).sum(0)
    pbin = torch.clamp(((2 * below + equal) * BINS) // (2 * S), max=BINS - 1)
    d = x - y
    w = (2 * torch.arange(S, device=F.device, dtype=torch.float64) - S + 1).reshape(S, 1, 1)
    crps = d.abs().sum(0) / S - (w * d).sum(0) / (S * S)
    inside = []
    for qlo, qhi in zip(band_levels()[0::2], band_levels()[1::2]):
        edges = []
        for qj in (qlo, qhi):
            h = qj * (S - 1)
            lo = int(np.floor(h))
            g = h - lo
            a, b = x[lo], x[min(lo + 1, S - 1)]
            dd = b - a
            edges.append(a if g == 0.0 else (a + dd * g if g < 0.5 else b - dd * (1.0 - g)))
        inside.append(((edges[0] <= y) & (y <= edges[1]) & ok).sum(0))
    hist = torch.stack([((pbin == b) & ok).sum(0) for b in range(BINS)])
    mean = torch.where(ok, crps, torch.zeros_like(crps)).sum(0) / ok.sum(0)
    return mean, torch.stack(inside), hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a hundredth of the rows (a rehearsal)")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import gparatscale as G
    assert torch.cuda.is_available(), "score_probe needs an MI355X"
    ctx = G.context(0)
    S = 100
    failed = False
    print("tools/score_probe.py on one MI355X (S = 100, levels 0.5 / 0.9 / 0.95, 10 bins, device "
          "memory)")
    for ns, P in ((100_000, 64), (1_000_000, 8)):
        if args.quick:
            ns //= 100
        gen = torch.Generator("cuda").manual_seed(ns + P)
        F = torch.randn((S, ns, P), dtype=torch.float64, device="cuda", generator=gen)
        y = torch.randn((ns, P), dtype=torch.float64, device="cuda", generator=gen) * 1.2
        y[::97] = float("nan")
        nbytes = 8.0 * S * ns * P
        bound_ms = nbytes / HBM_BYTES_PER_S * 1e3
        print(f"== S={S} N*={ns} P={P}: chain {nbytes / 1e9:.2f} GB, bytes bound "
              f"{bound_ms:.3f} ms at 8 TB/s", flush=True)
        G.score_samples(F, y)                      # the workspace is sized by the first call
        ws0 = ctx.workspace_bytes()
        base_ok = True
        sc_ms, red_ms, q_ms, base_ms = [], [], [], []
        sc_peak = q_peak = base_peak = 0
        ctx.set_profiling(True)
        for it in range(args.warmup + args.rounds):
            timed = it >= args.warmup
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated()
            # the scorer
            torch.cuda.reset_peak_memory_stats()
            ctx.reset_stats()
            got = G.score_samples(F, y, levels=LEVELS, bins=BINS)
            assert ctx.workspace_bytes() == ws0, (ws0, ctx.workspace_bytes())
            launches, ms = ctx.kernel_stats("score")
            assert launches == 1 and ctx.kernel_work("score") == nbytes
            rms = ctx.kernel_stats("score_reduce")[1]
            sc_peak = max(sc_peak, torch.cuda.max_memory_allocated() - held)
            if timed:
                sc_ms.append(ms)
                red_ms.append(rms)
            # the quantile call with the six band edges
            torch.cuda.reset_peak_memory_stats()
            ctx.reset_stats()
            bands = G.sample_quantiles(F, band_levels())
            qms = ctx.kernel_stats("quantile")[1]
            q_peak = max(q_peak, torch.cuda.max_memory_allocated() - held)
            if timed:
                q_ms.append(qms)
            del bands
            # the torch route
            if base_ok:
                try:
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    mean, inside, hist = torch_route(torch, F, y)
                    e1.record()
                    torch.cuda.synchronize()
                    base_peak = max(base_peak, torch.cuda.max_memory_allocated() - held)
                    if timed:
                        base_ms.append(e0.elapsed_time(e1))
                    if it == 0:
                        err = float(np.abs(got.crps - mean.cpu().numpy()).max())
                        tol = 2 * (S + 4 + ns) * 2.0 ** -52 * float(got.crps.max())
                        cnt = np.rint(got.coverage * got.scored).astype(np.int64)
                        same = (np.array_equal(cnt, inside.cpu().numpy())
                                and np.array_equal(got.pit_hist, hist.cpu().numpy()))
                        print(f"   scorer vs torch route: max |crps diff| {err:.3e} (tolerance "
                              f"{tol:.3e}{'' if err <= tol else ': EXCEEDED'}), inside counts and "
                              f"PIT histogram {'equal' if same else 'DIFFER'}")
                        failed |= err > tol or not same
                    del mean, inside, hist
                except torch.cuda.OutOfMemoryError:
                    base_ok = False
                    torch.cuda.empty_cache()
                    print("   torch route: ran out of device memory beside the chain")
        ctx.set_profiling(False)
        print(f"   scorer   : per-entry pass min {min(sc_ms):.3f} ms  max {max(sc_ms):.3f} ms  "
              f"({bound_ms / min(sc_ms) * 100:.1f} % of the bytes bound at the min, "
              f"{nbytes / min(sc_ms) / 1e9:.2f} TB/s); reduction min {min(red_ms):.3f} ms  "
              f"max {max(red_ms):.3f} ms")
        print(f"              workspace {ws0} bytes ({ws0 / (ns * P):.2f} per entry, unchanged by "
              f"the calls); torch memory beyond the chain and y {sc_peak / 1e6:.1f} MB")
        print(f"   quantiles: 6 levels min {min(q_ms):.3f} ms  max {max(q_ms):.3f} ms  "
              f"(output {q_peak / 1e6:.1f} MB); scorer per-entry pass / quantiles "
              f"{min(sc_ms) / min(q_ms):.2f}")
        if base_ms:
            print(f"   torch    : min {min(base_ms):.3f} ms  max {max(base_ms):.3f} ms  "
                  f"device memory beyond the chain {base_peak / 1e9:.2f} GB "
                  f"({base_peak / nbytes:.2f} x the chain)")
            total = min(sc_ms) + min(red_ms)
            print(f"   ratio torch / scorer (pass + reduction, min over min): "
                  f"{min(base_ms) / total:.2f}")
            if not total < min(base_ms):
                print("   FAILED: the scorer must beat the torch route")
                failed = True
        del F, y
        torch.cuda.empty_cache()
        # the two scorer paths at S = 64, the same number of entries
        F = torch.randn((64, ns, P), dtype=torch.float64, device="cuda", generator=gen)
        y = torch.randn((ns, P), dtype=torch.float64, device="cuda", generator=gen)
        ctx.set_profiling(True)
        for path in ("reg", "lds"):
            os.environ["GPAR_SCORE_PATH"] = path
            ms_p = []
            for it in range(1 + 3):
                ctx.reset_stats()
                G.score_samples(F, y)
                ms_p.append(ctx.kernel_stats("score")[1])
            print(f"   S=64 forced {path} path: min {min(ms_p[1:]):.3f} ms  max {max(ms_p[1:]):.3f} ms"
                  f"  ({8.0 * 64 * ns * P / min(ms_p[1:]) / 1e9:.2f} TB/s)")
        del os.environ["GPAR_SCORE_PATH"]
        ctx.set_profiling(False)
        del F, y
        torch.cuda.empty_cache()
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
