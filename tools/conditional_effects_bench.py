"""Times conditional_effects() with HIP events, in one process (medians of --reps after --warmup warm-ups), at the C3
shape (N = u = 20 000, P = 20), for

  (a) one effect along one moderator, G = 25 grid values: pairs (2, 1);
  (b) all 19 other columns along one moderator: pairs (2, 1) .. (20, 1).

For each: the fused pass alone (bigkrls_dev_kernel_loo_moments on the standardised rows: 1 and 19 kind-1 entries on
c = 0), the end-to-end call from the factors of vcov.est.c, and the route they replace, timed on the same build: G
marginal_effects() calls on the training rows with the moderator's column rewritten (one call serves all effects of a
grid value). The largest difference between the two routes' values and variances is printed with the times.

Prints one JSON line per measurement.

    python tools/conditional_effects_bench.py [--reps 10] [--warmup 3] [--n 20000] [--p 20] [--grid 25]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--grid", type=int, default=25)
    args = ap.parse_args()
    import bigkrls_amd as bk
    from bigkrls_amd import _lib
    from bigkrls_amd.synth import synth

    ctx = bk.Context(0)
    n, p, G = args.n, args.p, args.grid

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ctx.sync()
        ts = []
        for _ in range(args.reps):
            e0 = ctx.event()
            fn()
            e1 = ctx.event()
            ctx.sync()
            ts.append(ctx.elapsed_ms(e0, e1))
            ctx.release_events([e0, e1])
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    X, y = synth(n, p, 103)
    Xs = (X - X.mean(axis=0)) / X.std(axis=0, ddof=1)
    sigma = float(p)
    fit = bk.bigKRLS(y, X, eigtrunc=0.001, derivative=False, instructions=False, noisy=False, ctx=ctx,
                     vcov_form="factors")
    k = fit["lastkeeper"]
    dX = ctx.from_numpy(Xs)
    grid = np.linspace(X[:, 0].min(), X[:, 0].max(), G)

    for part, effects in (("a", [2]), ("b", list(range(2, p + 1)))):
        ne = len(effects)
        entries = np.ascontiguousarray([(1, 0, j - 1) for j in effects], dtype=np.int64)
        M = ctx.empty(n, ne)

        def fused():
            _lib.call("bigkrls_dev_kernel_loo_moments", ctx.handle, dX.ptr, n, dX.ld, dX.ptr, n, dX.ld, p, sigma,
                      entries.ctypes.data, ne, M.ptr, M.ld)

        def call():
            return bk.conditional_effects(fit, effects, 1, grid=G, vcov="factors", ctx=ctx)

        def route():
            avg, var = np.empty((G, ne)), np.empty((G, ne))
            for g, v in enumerate(grid):
                Z = X.copy()
                Z[:, 0] = v
                me = bk.marginal_effects(fit, Z, which_derivatives=effects, vcov="factors", ctx=ctx)
                avg[g], var[g] = me["avgderivatives"][0], me["var.avgderivatives"][0]
            return avg, var

        t_f, t_c = timed(fused), timed(call)
        row = {"part": part, "n": n, "u": n, "p": p, "k": k, "grid": G, "effects": ne,
               "fused_pass_ms": t_f[0], "fused_pass_min_max_ms": t_f[1:],
               "fused_pass_gpairs_per_s": float(n) * n / (t_f[0] * 1e-3) / 1e9,
               "conditional_effects_ms": t_c[0], "conditional_effects_min_max_ms": t_c[1:]}
        t_r = timed(route)
        res = call()
        avg, var = route()
        ce = np.array(res["ce"]).T
        se2 = np.array(res["se.ce"]).T ** 2
        row.update({"marginal_effects_route_ms": t_r[0], "marginal_effects_route_min_max_ms": t_r[1:],
                    "call_over_route": t_c[0] / t_r[0],
                    "max_abs_diff_ce_over_max": float(np.max(np.abs(ce - avg)) / np.max(np.abs(avg))),
                    "max_rel_diff_var": float(np.max(np.abs(se2 - var) / var))})
        print(json.dumps(row), flush=True)
        del M
    ctx.release_workspace()


if __name__ == "__main__":
    main()
