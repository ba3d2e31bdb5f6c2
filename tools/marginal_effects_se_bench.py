"""Times the pointwise standard errors of the marginal effects (marginal_effects(se=True)) with HIP events after
warm-up, in one process (medians of --reps), on the C3 fit (n = 20 000, P = |J| = 20, k = its lastkeeper):

  (a) product  : per block of m new points and all |J| columns, the fused route -- bigkrls_dev_gemm_modulated +
                 bigkrls_dev_rowsumsq_weighted per column -- against the unfused chain built from entries that need no
                 modulated GEMM: T0 = Kn_b Q once, and per column T_j = Kn_b (diag(x_j) Q) as bigkrls_dev_multdiag on Q'
                 and a bigkrls_dev_gemm with B transposed. The chain's combination diag(r) T0 + diag(t) T_j and its row
                 sums are NOT timed (they would only add to the chain), so the comparison favours the chain.
  (b) call     : marginal_effects(se=True) from the factors against se=False, u new points
  (c) dense    : marginal_effects(se=True, vcov="dense") at the smallest u
  (d) memory   : peak device memory of the se=True call from the factors (torch allocator peak + library workspace)

Prints one JSON line per measurement.

    python tools/marginal_effects_se_bench.py [--reps 10] [--n 20000] [--p 20] [--u 5000 20000 200000]
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
    ap.add_argument("--u", type=int, nargs="*", default=[5000, 20000, 200000])
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
    Q, k = fit["vcov.est.Q"], fit["lastkeeper"]
    dw = ctx.from_numpy(fit["vcov.est.w"])
    Xs = (X - X.mean(axis=0)) / X.std(axis=0, ddof=1)
    b = max(128, ((1 << 30) // (8 * (n + k))) // 128 * 128)            # rows per block from the factors

    # ---- (a) the fused product against the unfused chain, one block, all columns ----------------------------------
    rng = np.random.default_rng(n)
    dS = ctx.from_numpy(Xs)                                             # s of column j: column j of Xs
    Qt = ctx.from_numpy(np.ascontiguousarray(Q.to_numpy().T))           # Q' (k x n), made once outside the timing
    for m in sorted({min(b, u) for u in args.u}):
        A = ctx.from_numpy(rng.random((m, n)))
        R, Tm = ctx.from_numpy(rng.standard_normal((m, p))), ctx.from_numpy(rng.standard_normal((m, p)))
        T, T0, QtS, out = ctx.empty(m, k), ctx.empty(m, k), ctx.empty(k, n), ctx.empty(m, p)

        def fused():
            for j in range(p):
                _lib.call("bigkrls_dev_gemm_modulated", ctx.handle, m, k, n, A.ptr, A.ld, R.col_ptr(j), Tm.col_ptr(j),
                          dS.col_ptr(j), Q.ptr, Q.ld, T.ptr, T.ld)
                _lib.call("bigkrls_dev_rowsumsq_weighted", ctx.handle, m, k, T.ptr, T.ld, dw.ptr, out.col_ptr(j))

        def chain():
            _lib.call("bigkrls_dev_gemm", ctx.handle, 0, 0, m, k, n, 1.0, A.ptr, A.ld, Q.ptr, Q.ld, 0.0, T0.ptr, T0.ld)
            for j in range(p):
                _lib.call("bigkrls_dev_multdiag", ctx.handle, Qt.ptr, k, n, Qt.ld, dS.col_ptr(j), QtS.ptr, QtS.ld)
                _lib.call("bigkrls_dev_gemm", ctx.handle, 0, 1, m, k, n, 1.0, A.ptr, A.ld, QtS.ptr, QtS.ld, 0.0, T.ptr,
                          T.ld)

        def plain():
            for j in range(p):
                _lib.call("bigkrls_dev_gemm", ctx.handle, 0, 0, m, k, n, 1.0, A.ptr, A.ld, Q.ptr, Q.ld, 0.0, T.ptr, T.ld)
        t_f, t_c, t_p = timed(fused), timed(chain), timed(plain)
        flops = 2.0 * m * n * k * p
        print(json.dumps({"part": "a", "m": m, "n": n, "k": k, "columns": p, "fused_ms": t_f, "unfused_chain_ms": t_c,
                          "plain_gemm_only_ms": t_p, "fused_over_chain": t_f / t_c,
                          "fused_tflops": flops / (t_f * 1e-3) / 1e12}), flush=True)
        del A, R, Tm, T, T0, QtS, out
        ctx.release_workspace()
    del Qt, dS

    # ---- (b), (d): the call from the factors with and without se; peak memory -------------------------------------
    for u in args.u:
        Zh = np.random.default_rng(u).standard_normal((u, p))
        reps = args.reps if u <= 50000 else max(3, args.reps // 3)
        t0 = timed(lambda: bk.marginal_effects(fit, Zh, ctx=ctx, vcov="factors"), reps=reps, warmup=1)
        ctx.release_workspace()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t1 = timed(lambda: bk.marginal_effects(fit, Zh, ctx=ctx, vcov="factors", se=True), reps=reps, warmup=1)
        peak = torch.cuda.max_memory_allocated() - base + ctx.workspace_bytes()
        print(json.dumps({"part": "b", "n": n, "p": p, "k": k, "u": u, "se_false_ms": t0, "se_true_ms": t1,
                          "se_only_ms": t1 - t0, "se_tflops": 2.0 * u * n * k * p / ((t1 - t0) * 1e-3) / 1e12}),
              flush=True)
        print(json.dumps({"part": "d", "u": u, "peak_device_gb": peak / 1e9}), flush=True)
        ctx.release_workspace()

    # ---- (c) the dense path ------------------------------------------------------------------------------------------
    u = min(args.u)
    Zh = np.random.default_rng(u).standard_normal((u, p))
    res = {}

    def dense():
        res["d"] = bk.marginal_effects(fit, Zh, ctx=ctx, vcov="dense", se=True)
    t_d = timed(dense, reps=max(3, args.reps // 3), warmup=1)
    f = bk.marginal_effects(fit, Zh, ctx=ctx, vcov="factors", se=True)["se.derivatives"]
    d = res["d"]["se.derivatives"]
    print(json.dumps({"part": "c", "n": n, "p": p, "u": u, "dense_se_true_ms": t_d,
                      "se_max_abs_diff_over_max_se": float(np.max(np.abs(f - d)) / np.max(d))}), flush=True)
    ctx.release_workspace()


if __name__ == "__main__":
    main()
