"""Times accumulated_effects() with HIP events after warm-up, in one process (medians of --reps), at the C3 shape
(N = u = 20 000, P = 20, all 20 columns, 20 inverted-CDF bins each):

  (a) pass : M (n x 400) by the fused binned leave-one-column-out pass (bigkrls_dev_kernel_loo_binsums) against the
             same M made without it: one bigkrls_dev_kernel_loo_colsums per (column, bin) on that bin's rows, 400
             calls. The chain's entries take a row block of a matrix, so "gathered" means: per column one copy of the
             reference rows in that column's bin order (made on the host and uploaded); every bin is then a row block of
             it. The chain is timed with these 20 copies and without them (made beforehand). Both routes evaluate
             u n 20 exponentials; the largest difference between the two results is printed. From the pass's profile
             and the same launch with ONE bin per column (kernel_loo_colsums' work per column, chunk width 1) against
             bigkrls_dev_kernel_loo_colsums itself (chunk width 4: the Gram tile shared by 4 columns) comes the share
             of the Gram rebuild per column.
  (b) call : accumulated_effects(bins = 20) from the factors of vcov.est.c, with and without standard errors, beside
             ONE predict(se_pred=True, matrices=False) on 1 000 rewritten rows (a bin's rows at one edge) -- the route
             it replaces runs 2 x 400 of them, so "predict_route_x800_ms" is an EXTRAPOLATION, not a measurement.

Prints one JSON line per measurement.

    python tools/accumulated_effects_bench.py [--reps 10] [--n 20000] [--p 20] [--bins 20]
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
    ap.add_argument("--bins", type=int, default=20)
    ap.add_argument("--skip-call", action="store_true", help="part (a) only")
    args = ap.parse_args()
    import bigkrls_amd as bk
    from bigkrls_amd import _lib
    from bigkrls_amd.synth import synth

    ctx = bk.Context(0)
    n, p, nb = args.n, args.p, args.bins

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
    Xs = np.asfortranarray((X - X.mean(axis=0)) / X.std(axis=0, ddof=1))
    sigma = float(p)

    # ---- (a) the fused pass against the chain of the parent commit's entries ----------------------------------------
    cols = np.arange(p, dtype=np.int64)
    labels = np.empty((n, p), dtype=np.int64, order="F")
    nbins = np.empty(p, dtype=np.int64)
    orders, offsets = [], []
    for j in range(p):
        e = np.unique(np.quantile(Xs[:, j], np.arange(nb + 1) / nb, method="inverted_cdf"))
        labels[:, j] = np.maximum(np.searchsorted(e, Xs[:, j], side="left"), 1) - 1
        nbins[j] = e.size - 1
        orders.append(np.argsort(labels[:, j], kind="stable"))
        offsets.append(np.concatenate([[0], np.cumsum(np.bincount(labels[:, j], minlength=nbins[j]))]))
    total = int(nbins.sum())
    dX = ctx.from_numpy(Xs)
    M_f, M_c, M_1, M_l = ctx.empty(n, total), ctx.empty(n, total), ctx.empty(n, p), ctx.empty(n, p)
    zeros, ones_b = np.zeros((n, p), dtype=np.int64, order="F"), np.ones(p, dtype=np.int64)

    def fused():
        _lib.call("bigkrls_dev_kernel_loo_binsums", ctx.handle, dX.ptr, n, dX.ld, dX.ptr, n, dX.ld, p, sigma,
                  cols.ctypes.data, p, labels.ctypes.data, nbins.ctypes.data, M_f.ptr, M_f.ld)

    def fused_one_bin():
        _lib.call("bigkrls_dev_kernel_loo_binsums", ctx.handle, dX.ptr, n, dX.ld, dX.ptr, n, dX.ld, p, sigma,
                  cols.ctypes.data, p, zeros.ctypes.data, ones_b.ctypes.data, M_1.ptr, M_1.ld)

    def colsums():
        _lib.call("bigkrls_dev_kernel_loo_colsums", ctx.handle, dX.ptr, n, dX.ld, dX.ptr, n, dX.ld, p, sigma,
                  cols.ctypes.data, p, M_l.ptr, M_l.ld)

    def chain(gathered):
        at = 0
        for j in range(p):
            G = gathered[j] if gathered is not None else ctx.from_numpy(np.asfortranarray(Xs[orders[j]]))
            cj = cols[j:j + 1]
            for b in range(int(nbins[j])):
                r0, r1 = int(offsets[j][b]), int(offsets[j][b + 1])
                _lib.call("bigkrls_dev_kernel_loo_colsums", ctx.handle, G.col_ptr(0, r0), r1 - r0, G.ld, dX.ptr, n, dX.ld,
                          p, sigma, cj.ctypes.data, 1, M_c.col_ptr(at + b), M_c.ld)
            at += int(nbins[j])

    pre = [ctx.from_numpy(np.asfortranarray(Xs[orders[j]])) for j in range(p)]
    t_f = timed(fused)
    t_cg = timed(lambda: chain(None), reps=max(3, args.reps // 3), warmup=1)
    t_c = timed(lambda: chain(pre))
    t_1, t_l = timed(fused_one_bin), timed(colsums)
    ctx.set_profile(True)
    fused()
    ctx.sync()
    prof_ms, prof_work, prof_launches = ctx.get_profile("kernel_loo_binsums")
    ctx.set_profile(False)
    Mf, Mc = M_f.to_numpy(), M_c.to_numpy()
    print(json.dumps({"part": "a", "n": n, "u": n, "p": p, "columns": p, "bins": total, "fused_ms": t_f,
                      "chain_with_gathers_ms": t_cg, "chain_calls_only_ms": t_c,
                      "fused_over_chain_with_gathers": t_f / t_cg, "fused_over_chain_calls_only": t_f / t_c,
                      "fused_gexp_per_s": float(n) * n * p / (t_f * 1e-3) / 1e9,
                      "profile_kernel_loo_binsums_ms": prof_ms, "profile_launches": prof_launches,
                      "fused_one_bin_per_column_ms": t_1, "kernel_loo_colsums_ms": t_l,
                      "gram_rebuild_share_of_pass": (t_1 - t_l) / t_1,
                      "gram_rebuild_share_is": "(one bin per column, chunk width 1) minus (kernel_loo_colsums, chunk width "
                                               "4, same exponentials), over the former",
                      "max_abs_diff_over_max": float(np.max(np.abs(Mf - Mc)) / np.max(np.abs(Mc)))}), flush=True)
    del pre, M_f, M_c, M_1, M_l, dX
    ctx.release_workspace()
    if args.skip_call:
        return

    # ---- (b) the call, and one predict() of the route it replaces ----------------------------------------------------
    fit = bk.bigKRLS(y, X, eigtrunc=0.001, derivative=False, instructions=False, noisy=False, ctx=ctx,
                     vcov_form="factors")
    k = fit["lastkeeper"]
    reps = max(3, args.reps // 3)
    t_ale = timed(lambda: bk.accumulated_effects(fit, bins=nb, vcov="factors", ctx=ctx), reps=reps, warmup=1)
    t_ale_nose = timed(lambda: bk.accumulated_effects(fit, bins=nb, se=False, ctx=ctx), reps=reps, warmup=1)
    Zmod = X[: n // nb].copy()
    Zmod[:, 0] = 0.5
    t_pr = timed(lambda: bk.predict(fit, Zmod, se_pred=True, matrices=False, ctx=ctx), reps=reps, warmup=1)
    print(json.dumps({"part": "b", "n": n, "u": n, "p": p, "k": k, "bins": nb,
                      "accumulated_effects_ms": t_ale, "accumulated_effects_se_false_ms": t_ale_nose,
                      "one_predict_pointwise_ms": t_pr, "predict_rows": int(Zmod.shape[0]),
                      "predict_route_x800_ms": t_pr * 2 * p * nb,
                      "predict_route_is": "an extrapolation: one call's time x 2 edges x columns x bins; it gives no "
                                          "standard error of the accumulated curve"}), flush=True)
    ctx.release_workspace()


if __name__ == "__main__":
    main()
