#!/usr/bin/env python3
"""bigKRLS(kernel="stored") against bigKRLS(kernel="implicit"): wall time and peak device memory.

    python tools/implicit_fit_bench.py [--configs C4 C5 BIG] [--reps 2]

C4 and C5 are bench.py's shapes (N = 50 000, P = 20, Neig = 512; N = 100 000, P = 50, Neig = 1024 with
which.derivatives = 1, 3, 5), both fitted with vcov_form="factors" so that K is the only N x N buffer of the stored
fit. BIG is one fit that cannot be stored: N = 200 000, P = 20, Neig = 512, whose K alone would be 320 GB (implicit
only). Per fit: the best wall time of `reps` fits after one warm-up, the phases of that fit, and the peak device memory
= the library's workspace (hipMalloc) + the peak of torch's allocator (the outputs). One JSON line per fit."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "C4": dict(n=50000, p=20, seed=104, neig=512, which=None, forms=("stored", "implicit")),
    "C5": dict(n=100000, p=50, seed=105, neig=1024, which=[1, 3, 5], forms=("stored", "implicit")),
    "BIG": dict(n=200000, p=20, seed=106, neig=512, which=None, forms=("implicit",)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["C4", "C5", "BIG"], choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    import torch
    import bigkrls_amd as bk
    from bigkrls_amd.synth import synth
    ctx = bk.Context(0)
    for name in args.configs:
        c = CONFIGS[name]
        X, y = synth(c["n"], c["p"], c["seed"])
        for form in c["forms"]:
            ctx.release_workspace()
            torch.cuda.empty_cache()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            best, phases, keep = None, None, None
            for rep in range(args.reps + 1):                    # (the first fit allocates the workspace)
                t = {}
                t0 = time.perf_counter()
                out = bk.bigKRLS(y, X, Neig=c["neig"], which_derivatives=c["which"], vcov_form="factors", kernel=form,
                                 ctx=ctx, noisy=False, timings=t)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                keep = (out["lastkeeper"], out["lambda"])
                del out
                if rep > 0 and (best is None or wall < best):
                    best, phases = wall, {k: round(v, 4) for k, v in t.items()}
            peak = ctx.workspace_bytes() + torch.cuda.max_memory_allocated()
            print(json.dumps({"config": name, "n": c["n"], "p": c["p"], "neig": c["neig"], "kernel": form,
                              "wall_s": round(best, 4), "peak_device_GB": round(peak / 1e9, 2),
                              "workspace_GB": round(ctx.workspace_bytes() / 1e9, 2),
                              "K_GB": round(8.0 * c["n"] ** 2 / 1e9, 1), "lastkeeper": keep[0], "lambda": keep[1],
                              "phases_s": phases}), flush=True)


if __name__ == "__main__":
    main()
