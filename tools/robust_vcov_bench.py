"""Times the kernels behind robust_vcov() with HIP events after warm-up, in one fresh process (medians of --reps):

  (a) gram    : bigkrls_dev_gram_weighted against the route the library offered before it -- a row-scaled copy of Q
                (an elementwise kernel; here torch's, on the context's stream) plus bigkrls_dev_gemm(ta = 1) -- with the
                copy timed and not timed. Shapes (N, k) = (20 000, 250) and (100 000, 1 024), random operands.
  (b) scores  : bigkrls_dev_cluster_scores at G = 50 and G = N / 4, labels contiguous and shuffled, against the
                8 N k bytes it has to read at the card's copy bandwidth as measured here (a device-to-device copy of
                the same operand: 16 N k bytes moved).
  (c) call    : robust_vcov("HC1") and robust_vcov("CR1", G = 50) on the C3 fit (N = 20 000, P = 20, k = its
                lastkeeper) beside the fit's own vcov_c phase. Host clock around the call (it ends synchronised).

Prints one JSON line per measurement.

    python tools/robust_vcov_bench.py [--reps 10] [--warmup 3] [--skip-fit]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(20000, 250), (100000, 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-fit", action="store_true")
    args = ap.parse_args()
    import torch
    import bigkrls_amd as bk
    from bigkrls_amd import _lib

    ctx = bk.Context(0)

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
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    for n, k in SHAPES:
        rng = np.random.default_rng(n + k)
        Q = ctx.from_numpy(rng.standard_normal((n, k)))
        om = ctx.from_numpy(rng.random(n))
        M, M2, Qw = ctx.empty(k, k), ctx.empty(k, k), ctx.empty(n, k)

        # ---- (a) ------------------------------------------------------------------------------------------------------
        def fused():
            _lib.call("bigkrls_dev_gram_weighted", ctx.handle, n, k, Q.ptr, Q.ld, om.ptr, M.ptr, M.ld)

        def scale_copy():
            with ctx.on_stream():
                torch.mul(Q.t, om.t, out=Qw.t)            # (k, n) storage: row i of Q times omega[i]

        def gemm_only():
            _lib.call("bigkrls_dev_gemm", ctx.handle, 1, 0, k, k, n, 1.0, Qw.ptr, Qw.ld, Q.ptr, Q.ld, 0.0, M2.ptr, M2.ld)

        def copy_and_gemm():
            scale_copy()
            gemm_only()
        copy_and_gemm()
        fused()
        ctx.sync()
        a, b = M.to_numpy(), M2.to_numpy()
        agree = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
        t_f, t_c, t_g = timed(fused), timed(copy_and_gemm), timed(gemm_only)
        print(json.dumps({"part": "a", "n": n, "k": k, "gram_weighted_ms": t_f[0], "min_max_ms": t_f[1:],
                          "copy_plus_gemm_ms": t_c[0], "gemm_only_ms": t_g[0], "fused_over_copy_plus_gemm": t_f[0] / t_c[0],
                          "fused_over_gemm_only": t_f[0] / t_g[0],
                          "gram_tflops_of_nk(k+1)": n * k * (k + 1.0) / (t_f[0] * 1e-3) / 1e12,
                          "max_abs_diff_over_max": agree}), flush=True)

        # ---- (b) ------------------------------------------------------------------------------------------------------
        def d2d():
            _lib.call("bigkrls_d2d", ctx.handle, Qw.ptr, Q.ptr, 8 * n * k)
        t_copy = timed(d2d)
        copy_bw = 16.0 * n * k / (t_copy[0] * 1e-3)
        e = ctx.from_numpy(rng.standard_normal(n))
        for G in (50, n // 4):
            S = ctx.empty(k, G)
            base = (np.arange(n) * G) // n
            for what, lab in (("contiguous", base), ("shuffled", rng.permutation(base))):
                lab = np.ascontiguousarray(lab, dtype=np.int64)

                def scores():
                    _lib.call("bigkrls_dev_cluster_scores", ctx.handle, n, k, Q.ptr, Q.ld, e.ptr, lab.ctypes.data, G,
                              S.ptr, S.ld)
                ctx.set_profile(True)
                timed(scores)
                ms, _, launches = ctx.get_profile("cluster_scores")
                ctx.set_profile(False)
                t_call = timed(scores)
                print(json.dumps({"part": "b", "n": n, "k": k, "G": G, "labels": what, "kernels_ms": ms / launches,
                                  "call_with_host_sort_ms": t_call[0], "copy_bandwidth_TBps": copy_bw / 1e12,
                                  "read_8nk_at_copy_bandwidth_ms": 8.0 * n * k / copy_bw * 1e3,
                                  "kernels_over_that": (ms / launches) / (8.0 * n * k / copy_bw * 1e3)}), flush=True)
            del S
        del Q, om, M, M2, Qw, e
        ctx.release_workspace()

    # ---- (c) ----------------------------------------------------------------------------------------------------------
    if args.skip_fit:
        return
    from bigkrls_amd.synth import synth
    n, p = 20000, 20
    X, y = synth(n, p, 103)
    timings = {}
    fit = bk.bigKRLS(y, X, eigtrunc=0.001, instructions=False, noisy=False, ctx=ctx, vcov_form="both", timings=timings)
    fit = bk.bigKRLS(y, X, eigtrunc=0.001, instructions=False, noisy=False, ctx=ctx, vcov_form="both", timings=timings)
    lab = np.random.default_rng(1).permutation((np.arange(n) * 50) // n)
    for type, cluster in (("HC1", None), ("HC3", None), ("CR1", lab)):
        ts = []
        for i in range(args.warmup + args.reps):
            ctx.sync()
            t0 = time.perf_counter()
            r = bk.robust_vcov(fit, type=type, cluster=cluster, ctx=ctx)
            ctx.sync()
            if i >= args.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        # ... and without the recomputation of var.avgderivatives (one marginal_effects() at newdata = X)
        bare = bk.BigKRLS({key: v for key, v in fit.items() if key != "derivatives"})
        tb = []
        for i in range(args.warmup + args.reps):
            ctx.sync()
            t0 = time.perf_counter()
            bk.robust_vcov(bare, type=type, cluster=cluster, ctx=ctx)
            ctx.sync()
            if i >= args.warmup:
                tb.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"part": "c", "n": n, "p": p, "k": int(fit["lastkeeper"]), "type": type,
                          "robust_vcov_ms": float(np.median(ts)), "without_marginal_effects_ms": float(np.median(tb)),
                          "fit_vcov_c_phase_ms": timings["vcov_c"] * 1e3, "fit_native_ms": timings["native"] * 1e3,
                          "w0": float(r["vcov.est.w"][0])}), flush=True)


if __name__ == "__main__":
    main()
