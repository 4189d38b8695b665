"""Timing of gpar_sample_quantiles against the torch.sort route (needs an MI355X; not a test).

Sizes: S = 100 samples, q = (0.025, 0.5, 0.975), device memory, at N* = 1e5, P = 64 (eeg's chain,
5.1 GB) and N* = 1e6, P = 8 (a north rank's block, 6.4 GB).  Per size, 2 warm-up rounds and 10
timed rounds, each round one library call followed by one baseline call on the same tensor in the
same process:

  library   HIP-event time of the "quantile" family (gpar_ctx_kernel_stats), min and max over the
            rounds, and its fraction of the bytes bound 8 S N* P / 8 TB/s;
            gpar_ctx_workspace_bytes before and after (asserted equal) and torch's peak allocation
            across the call beyond the tensor (the nq x N* x P output);
  baseline  torch.sort(F, dim=0) and the same interpolation in torch, the only device route a
            Python user has otherwise, timed with torch events; its peak allocation beyond F.
            When the sort's workspace does not fit beside F the baseline is reported as such.

Also timed, for DESIGN 4.9: both kernel paths forced (GPAR_QUANTILE_PATH) at S = 100, and the
results of the two routes compared.

  python tools/quantile_probe.py [--quick] > profiles/quantile_probe.txt"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpar-at-scale_amd", "python"))

HBM_BYTES_PER_S = 8.0e12
Q = (0.025, 0.5, 0.975)


def torch_route(torch, F, q):
    """sort along the samples, then numpy's _lerp at the same positions"""
    S = F.shape[0]
    x, _ = torch.sort(F, dim=0)
    rows = []
    for qj in q:
        h = qj * (S - 1)
        lo = int(np.floor(h))
        g = h - lo
        a, b = x[lo], x[min(lo + 1, S - 1)]
        d = b - a
        rows.append(a if g == 0.0 else (a + d * g if g < 0.5 else b - d * (1.0 - g)))
    return torch.stack(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a hundredth of the rows (a rehearsal)")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import gparatscale as G
    assert torch.cuda.is_available(), "quantile_probe needs an MI355X"
    ctx = G.context(0)
    S = 100
    failed = False
    for ns, P in ((100_000, 64), (1_000_000, 8)):
        if args.quick:
            ns //= 100
        gen = torch.Generator("cuda").manual_seed(ns + P)
        F = torch.randn((S, ns, P), dtype=torch.float64, device="cuda", generator=gen)
        nbytes = 8.0 * S * ns * P
        bound_ms = nbytes / HBM_BYTES_PER_S * 1e3
        print(f"== S={S} N*={ns} P={P}: chain {nbytes / 1e9:.2f} GB, bytes bound "
              f"{bound_ms:.3f} ms at 8 TB/s", flush=True)
        base_ok = True
        lib_ms, base_ms = [], []
        lib_peak = base_peak = 0
        ws0 = ws1 = None
        ctx.set_profiling(True)
        for it in range(args.warmup + args.rounds):
            timed = it >= args.warmup
            # the library call
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ctx.reset_stats()
            ws0 = ctx.workspace_bytes()
            got = G.sample_quantiles(F, Q)
            ws1 = ctx.workspace_bytes()
            assert ws1 == ws0, (ws0, ws1)
            launches, ms = ctx.kernel_stats("quantile")
            assert launches == 1 and ctx.kernel_work("quantile") == nbytes
            lib_peak = max(lib_peak, torch.cuda.max_memory_allocated() - held)
            if timed:
                lib_ms.append(ms)
            # the baseline, alternating with it
            if base_ok:
                try:
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    ref = torch_route(torch, F, Q)
                    e1.record()
                    torch.cuda.synchronize()
                    base_peak = max(base_peak, torch.cuda.max_memory_allocated() - held)
                    if timed:
                        base_ms.append(e0.elapsed_time(e1))
                    if it == 0:
                        err = float((got - ref).abs().max())
                        tol = 6 * 2.0 ** -52 * float(F.abs().max())
                        print(f"   library vs torch route: max |diff| {err:.3e} (tolerance {tol:.3e}"
                              f"{'' if err <= tol else ': EXCEEDED'})")
                        failed |= err > tol
                    del ref
                except torch.cuda.OutOfMemoryError:
                    base_ok = False
                    torch.cuda.empty_cache()
                    print("   baseline: torch.sort ran out of device memory beside the chain")
            del got
        ctx.set_profiling(False)
        print(f"   library : min {min(lib_ms):.3f} ms  max {max(lib_ms):.3f} ms  "
              f"({bound_ms / min(lib_ms) * 100:.1f} % of the bytes bound at the min, "
              f"{nbytes / min(lib_ms) / 1e9:.2f} TB/s)")
        print(f"             workspace {ws0} -> {ws1} bytes (unchanged); device memory beyond the "
              f"chain {lib_peak / 1e6:.1f} MB (output {8.0 * len(Q) * ns * P / 1e6:.1f} MB)")
        if base_ms:
            print(f"   baseline: min {min(base_ms):.3f} ms  max {max(base_ms):.3f} ms  "
                  f"device memory beyond the chain {base_peak / 1e9:.2f} GB "
                  f"({base_peak / nbytes:.2f} x the chain)")
            print(f"   ratio baseline / library (min over min): {min(base_ms) / min(lib_ms):.2f}")
            if not min(lib_ms) < min(base_ms):
                print("   FAILED: the kernel must beat the torch.sort route")
                failed = True
        # the two kernel paths at this size
        ctx.set_profiling(True)
        for path in ("reg", "lds"):
            os.environ["GPAR_QUANTILE_PATH"] = path
            ms_p = []
            for it in range(1 + 3):
                ctx.reset_stats()
                G.sample_quantiles(F, Q)
                ms_p.append(ctx.kernel_stats("quantile")[1])
            print(f"   forced {path} path: min {min(ms_p[1:]):.3f} ms  max {max(ms_p[1:]):.3f} ms")
        del os.environ["GPAR_QUANTILE_PATH"]
        ctx.set_profiling(False)
        del F
        torch.cuda.empty_cache()
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
