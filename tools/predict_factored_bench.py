"""Times the post-fit path on the factors of vcov.est.c (Q diag(w) Q') against the N x N matrix, with HIP events after
warm-up, in one process (medians of --reps):

  (a) kernel        : T = A Q (bigkrls_dev_gemm) + sum_j w_j T_ij^2 (bigkrls_dev_rowsumsq_weighted) against
                      diag(A V A') (bigkrls_dev_quadform_diag) for A m x n, Q n x k, V = Q diag(w) Q'
  (b) predict       : predict(se_pred=True, matrices=False) with vcov="factors" against vcov="dense" on the same
                      vcov_form="both" fit
  (c) fit           : wall time and peak device memory (torch allocator peak + library workspace) of
                      bigKRLS(vcov_form="dense") against vcov_form="factors"

Prints one JSON line per measurement.

    python tools/predict_factored_bench.py [--reps 10] [--n 20000] [--p 20]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--m", type=int, nargs="*", default=[2048, 6656])
    ap.add_argument("--u", type=int, nargs="*", default=[5000, 20000, 50000, 200000])
    ap.add_argument("--fit-reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import bigkrls_amd as bk
    from bigkrls_amd import _lib
    from bigkrls_amd.synth import synth

    ctx = bk.Context(0)
    n, p = args.n, args.p

    def timed(fn, reps=args.reps, warmup=args.warmup):
        for _ in range(warmup):
            fn()
        ctx.sync()
        ts = []
        for _ in range(reps):
            e0 = ctx.event()
            fn()
            e1 = ctx.event()
            ctx.sync()
            ts.append(ctx.elapsed_ms(e0, e1))
            ctx.release_events([e0, e1])
        return float(np.median(ts))

    X, y = synth(n, p, 103)
    fit = bk.bigKRLS(y, X, eigtrunc=0.001, derivative=False, instructions=False, noisy=False, ctx=ctx,
                     vcov_form="both")
    Q, V, k = fit["vcov.est.Q"], fit["vcov.est.c"], fit["lastkeeper"]
    dw = ctx.from_numpy(fit["vcov.est.w"])

    # ---- (a) gemm + the new operator against quadform_diag -------------------------------------------------------
    rng = np.random.default_rng(n)
    for m in args.m:
        A = ctx.from_numpy(rng.random((m, n)))
        T, out_f, out_d = ctx.empty(m, k), ctx.empty(m, 1), ctx.empty(m, 1)

        def gm():
            _lib.call("bigkrls_dev_gemm", ctx.handle, 0, 0, m, k, n, 1.0, A.ptr, A.ld, Q.ptr, Q.ld, 0.0, T.ptr, T.ld)

        def rs():
            _lib.call("bigkrls_dev_rowsumsq_weighted", ctx.handle, m, k, T.ptr, T.ld, dw.ptr, out_f.ptr)

        def fact():
            gm()
            rs()

        def dense():
            _lib.call("bigkrls_dev_quadform_diag", ctx.handle, m, n, A.ptr, A.ld, V.ptr, V.ld, out_d.ptr)
        t_gm, t_rs, t_f, t_d = timed(gm), timed(rs), timed(fact), timed(dense)
        a, b = out_f.to_numpy().ravel(), out_d.to_numpy().ravel()
        print(json.dumps({"part": "a", "m": m, "n": n, "k": k, "gemm_ms": t_gm, "rowsumsq_weighted_ms": t_rs,
                          "gemm_plus_rowsumsq_ms": t_f, "quadform_diag_ms": t_d, "speedup": t_d / t_f,
                          "flop_ratio_n_over_k": n / k,
                          "max_abs_diff_over_max": float(np.max(np.abs(a - b)) / np.max(np.abs(b)))}), flush=True)
        del A, T, out_f, out_d
        ctx.release_workspace()

    # ---- (b) predict with SEs without the matrices, both forms ---------------------------------------------------
    for u in args.u:
        Zh = np.random.default_rng(u).standard_normal((u, p))
        res = {}

        def from_dense():
            res["d"] = bk.predict(fit, Zh, se_pred=True, ctx=ctx, matrices=False, vcov="dense")

        def from_factors():
            res["f"] = bk.predict(fit, Zh, se_pred=True, ctx=ctx, matrices=False, vcov="factors")
        reps = args.reps if u <= 50000 else max(3, args.reps // 3)
        t_d = timed(from_dense, reps=reps, warmup=1)
        ctx.release_workspace()
        t_f = timed(from_factors, reps=reps, warmup=1)
        dse = float(np.max(np.abs(res["f"]["se.pred"] - res["d"]["se.pred"])) / np.max(res["d"]["se.pred"]))
        print(json.dumps({"part": "b", "n": n, "p": p, "k": k, "u": u, "dense_ms": t_d, "factors_ms": t_f,
                          "speedup": t_d / t_f, "se_max_abs_diff_over_max_se": dse}), flush=True)
        del res
        ctx.release_workspace()
    del fit, Q, V, dw
    torch.cuda.empty_cache()

    # ---- (c) the fit: wall time and peak device memory -----------------------------------------------------------
    for form in ("dense", "factors"):
        walls, peak = [], 0
        for r in range(args.fit_reps + 1):
            ctx.release_workspace()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            out = bk.bigKRLS(y, X, eigtrunc=0.001, instructions=False, noisy=False, ctx=ctx, vcov_form=form)
            ctx.sync()
            wall = time.perf_counter() - t0
            if r > 0:                                          # the first repetition warms up
                walls.append(wall)
            peak = max(peak, torch.cuda.max_memory_allocated() - base + ctx.workspace_bytes())
            del out
        print(json.dumps({"part": "c", "n": n, "p": p, "vcov_form": form, "fit_wall_ms": 1e3 * float(np.median(walls)),
                          "peak_device_gb": peak / 1e9}), flush=True)
    ctx.release_workspace()


if __name__ == "__main__":
    main()
