"""Times partial_dependence() with HIP events after warm-up, in one process (medians of --reps), at the C3 shape
(N = u = 20 000, P = 20, all 20 columns):

  (a) pass : M (n x 20) by the fused leave-one-column-out pass (bigkrls_dev_kernel_loo_colsums, one launch) against the
             same M made without it: one bigkrls_dev_kernel_contract(trans = 1, W = ones) per column on copies of the
             operands with that column removed. The chain is timed with its operand copies (two
             bigkrls_dev_copy_matrix per column) and without them (the 20 copies made beforehand). Both routes evaluate
             u n 20 exponentials; the largest difference between the two results is printed.
  (b) call : partial_dependence(grid = 25) from the factors of vcov.est.c, all columns, the training rows as the
             reference sample, beside ONE predict(se_pred=True, matrices=False) on 20 000 rewritten rows -- the route it
             replaces runs 20 x 25 = 500 of them, so "predict_route_x500_ms" is an EXTRAPOLATION, not a measurement.

Prints one JSON line per measurement.

    python tools/partial_dependence_bench.py [--reps 10] [--n 20000] [--p 20] [--grid 25]
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
    ap.add_argument("--skip-call", action="store_true", help="part (a) only")
    args = ap.parse_args()
    import bigkrls_amd as bk
    from bigkrls_amd import _lib, ops
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
    Xs = (X - X.mean(axis=0)) / X.std(axis=0, ddof=1)
    sigma = float(p)

    # ---- (a) the fused pass against the chain of the parent commit's entries ----------------------------------------
    dX = ctx.from_numpy(Xs)
    cols = np.arange(p, dtype=np.int64)
    M_f, M_c = ctx.empty(n, p), ctx.empty(n, p)
    ones = ctx.from_numpy(np.ones((n, 1)))
    Xd = ctx.empty(n, p - 1)
    pre = [ctx.from_numpy(np.asfortranarray(np.delete(Xs, c, axis=1))) for c in range(p)]

    def fused():
        _lib.call("bigkrls_dev_kernel_loo_colsums", ctx.handle, dX.ptr, n, dX.ld, dX.ptr, n, dX.ld, p, sigma,
                  cols.ctypes.data, p, M_f.ptr, M_f.ld)

    def contract(D, c):
        _lib.call("bigkrls_dev_kernel_contract", ctx.handle, D.ptr, n, D.ld, D.ptr, n, D.ld, p - 1, sigma, ones.ptr, 1,
                  ones.ld, 1, M_c.col_ptr(c), M_c.ld)

    def chain_with_copies():
        for c in range(p):
            if c > 0:
                _lib.call("bigkrls_dev_copy_matrix", ctx.handle, dX.ptr, n, c, dX.ld, Xd.ptr, Xd.ld)
            if c < p - 1:
                _lib.call("bigkrls_dev_copy_matrix", ctx.handle, dX.col_ptr(c + 1), n, p - 1 - c, dX.ld, Xd.col_ptr(c),
                          Xd.ld)
            contract(Xd, c)

    def chain_no_copies():
        for c in range(p):
            contract(pre[c], c)

    t_f, t_cc, t_c = timed(fused), timed(chain_with_copies), timed(chain_no_copies)
    Mf, Mc = M_f.to_numpy(), M_c.to_numpy()
    print(json.dumps({"part": "a", "n": n, "u": n, "p": p, "columns": p, "fused_ms": t_f,
                      "chain_with_copies_ms": t_cc, "chain_contractions_only_ms": t_c,
                      "fused_over_chain_with_copies": t_f / t_cc, "fused_over_chain_contractions_only": t_f / t_c,
                      "fused_gexp_per_s": float(n) * n * p / (t_f * 1e-3) / 1e9,
                      "max_abs_diff_over_max": float(np.max(np.abs(Mf - Mc)) / np.max(np.abs(Mc)))}), flush=True)
    del pre, Xd, M_f, M_c, ones, dX
    ctx.release_workspace()
    if args.skip_call:
        return

    # ---- (b) the call, and one predict() of the route it replaces ----------------------------------------------------
    fit = bk.bigKRLS(y, X, eigtrunc=0.001, derivative=False, instructions=False, noisy=False, ctx=ctx,
                     vcov_form="factors")
    k = fit["lastkeeper"]
    reps = max(3, args.reps // 3)
    t_pd = timed(lambda: bk.partial_dependence(fit, grid=args.grid, vcov="factors", ctx=ctx), reps=reps, warmup=1)
    t_pd_nose = timed(lambda: bk.partial_dependence(fit, grid=args.grid, se=False, ctx=ctx), reps=reps, warmup=1)
    Zmod = X.copy()
    Zmod[:, 0] = 0.5
    t_pr = timed(lambda: bk.predict(fit, Zmod, se_pred=True, matrices=False, ctx=ctx), reps=reps, warmup=1)
    print(json.dumps({"part": "b", "n": n, "u": n, "p": p, "k": k, "grid": args.grid,
                      "partial_dependence_ms": t_pd, "partial_dependence_se_false_ms": t_pd_nose,
                      "one_predict_pointwise_ms": t_pr, "predict_route_x500_ms": t_pr * p * args.grid,
                      "predict_route_is": "an extrapolation: one call's time x columns x grid"}), flush=True)
    ctx.release_workspace()


if __name__ == "__main__":
    main()
