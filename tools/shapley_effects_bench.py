"""Times shapley_effects() in one process at N = 20 000, P = 20, u = 1 000 explained rows, B = 100 background rows, on a
fit that carries the factors of vcov.est.c (kernel="implicit", Neig = 250, nothing truncated): wall time of the second
and later calls (the first pays for the workspace), median of --reps,

  - with one player per column (M = 20) and with the 20 columns grouped into 5 players of 4,
  - without and with standard errors (from the factors),

and, from one more call under the context's profile, the time inside the weights kernel
(bigkrls_dev_shapley_weights, all row blocks), its rate against the operation count the design quotes -- 4 M ceil(M/2)
fused multiply-adds = 8 M ceil(M/2) flops per (explained, training, background) triple -- and the share of the call
spent outside that kernel (host standardisation, upload, W c, W Q, the row sums of squares, read-back).

Prints one JSON line per measurement.

    python tools/shapley_effects_bench.py [--reps 7] [--n 20000] [--p 20] [--u 1000] [--background 100] [--k 250]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--u", type=int, default=1000)
    ap.add_argument("--background", type=int, default=100)
    ap.add_argument("--k", type=int, default=250)
    ap.add_argument("--players", type=int, default=5, help="players of the grouped run (columns dealt out in turn)")
    args = ap.parse_args()
    import bigkrls_amd as bk
    from bigkrls_amd.synth import synth

    ctx = bk.Context(0)
    n, p, u, B = args.n, args.p, args.u, args.background
    X, y = synth(n, p, 103)
    fit = bk.bigKRLS(y, X, Neig=args.k, eigtrunc=0.0, kernel="implicit", derivative=False, instructions=False, noisy=False,
                     ctx=ctx, vcov_form="factors")
    k = int(np.asarray(fit["vcov.est.w"]).size)
    Z = X[np.random.default_rng(7).choice(n, u, replace=False)] + 0.1
    grouped = [[c + 1 for c in range(p) if c % args.players == m] for m in range(args.players)]

    def wall(fn):
        fn()                                    # the first call grows the workspace
        ts = []
        for _ in range(args.reps):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), ts

    for name, groups in (("singletons", None), ("grouped", grouped)):
        M = p if groups is None else len(groups)
        for se in (False, True):
            call = lambda: bk.shapley_effects(fit, Z, background=B, groups=groups, se=se, vcov="factors", ctx=ctx)
            ms, all_ms = wall(call)
            ctx.set_profile(True)
            call()
            ctx.sync()
            k_ms, k_work, k_launches = ctx.get_profile("shapley_weights")
            ctx.set_profile(False)
            print(json.dumps({"players": name, "n": n, "p": p, "M": M, "nodes": (M + 1) // 2, "u": u, "B": B, "k": k, "se": se,
                              "call_ms_median": ms, "call_ms_all": all_ms, "reps": args.reps,
                              "weights_kernel_ms": k_ms, "weights_kernel_launches": k_launches,
                              "weights_kernel_counted_flops": k_work,
                              "weights_kernel_counted_tflops": k_work / (k_ms * 1e-3) / 1e12 if k_ms > 0 else None,
                              "counted_flops_are": "8 M ceil(M/2) u n B: 4 M ceil(M/2) fused multiply-adds per triple",
                              "share_outside_weights_kernel": 1.0 - k_ms / ms}), flush=True)
    ctx.release_workspace()


if __name__ == "__main__":
    main()
