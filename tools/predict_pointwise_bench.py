"""Times predict(..., matrices=False) and its kernel against what they replace, with HIP events after warm-up, in one
process (medians of --reps):

  (a) quadform_diag : diag(A V A') for A m x n, V n x n (bigkrls_dev_quadform_diag), against the plain gemm of the
                      same shape into a scratch T (bigkrls_dev_gemm) followed by diag_extract of T's leading m x m block;
                      share of the fp64 MFMA peak on 2 m n^2 flops
  (b) predict       : predict(se_pred=True) with matrices=True (u x n and u x u matrices) against matrices=False
  (c) predict, u = 200 000, matrices=False: time and peak extra device memory (library workspace and torch allocator)

Prints one JSON line per measurement. newdata is passed as a device matrix, so matrices=True keeps its outputs on the
device (no host copy of the u x u matrix inside the timed window).

    python tools/predict_pointwise_bench.py [--reps 10] [--n 20000] [--p 20]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_PEAK = 78.6e12   # MI355X fp64 MFMA peak, flop/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--m", type=int, nargs="*", default=[2048, 6656])
    ap.add_argument("--u", type=int, nargs="*", default=[5000, 20000, 50000])
    ap.add_argument("--u-big", type=int, default=200000)
    args = ap.parse_args()
    import torch
    import bigkrls_amd as bk
    from bigkrls_amd import _lib
    from bigkrls_amd.synth import synth

    ctx = bk.Context(0)
    n, p = args.n, args.p

    def timed(fn, reps=args.reps):
        for _ in range(args.warmup):
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

    # ---- (a) the kernel against the gemm of the same shape ------------------------------------------------------
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    V = ctx.from_numpy(G)
    del G
    for m in args.m:
        A = ctx.from_numpy(rng.standard_normal((m, n)))
        out, T, D = ctx.empty(m, 1), ctx.empty(m, n), ctx.empty(m, 1)

        def qf():
            _lib.call("bigkrls_dev_quadform_diag", ctx.handle, m, n, A.ptr, A.ld, V.ptr, V.ld, out.ptr)

        def gm():
            _lib.call("bigkrls_dev_gemm", ctx.handle, 0, 0, m, n, n, 1.0, A.ptr, A.ld, V.ptr, V.ld, 0.0, T.ptr, T.ld)

        def gd():
            gm()
            _lib.call("bigkrls_dev_diag", ctx.handle, T.ptr, m, T.ld, D.ptr)
        t_qf, t_gm, t_gd = timed(qf), timed(gm), timed(gd)
        # same result check: rowdot(T, A) on the host from the gemm's T
        ref = np.einsum("ij,ij->i", T.to_numpy(), A.to_numpy())
        err = float(np.max(np.abs(out.to_numpy().ravel() - ref)) / np.max(np.abs(ref)))
        flops = 2.0 * m * n * n
        print(json.dumps({"part": "a", "m": m, "n": n, "quadform_diag_ms": t_qf, "gemm_ms": t_gm,
                          "gemm_plus_diag_extract_ms": t_gd, "quadform_over_gemm": t_qf / t_gm,
                          "share_of_fp64_peak": {"quadform_diag": flops / (t_qf * 1e-3) / FP64_PEAK,
                                                 "gemm": flops / (t_gm * 1e-3) / FP64_PEAK},
                          "rel_err_vs_gemm_rowdot": err}), flush=True)
        del A, out, T, D
        ctx.release_workspace()
    del V
    torch.cuda.empty_cache()

    # ---- (b) predict with SEs, both modes --------------------------------------------------------------------------
    X, y = synth(n, p, 103)
    fit = bk.bigKRLS(y, X, eigtrunc=0.001, derivative=False, instructions=False, noisy=False, ctx=ctx)
    for u in args.u:
        Z = ctx.from_numpy(np.random.default_rng(u).standard_normal((u, p)))
        res = {}

        def full():
            res["full"] = bk.predict(fit, Z, se_pred=True, ctx=ctx)

        def pw():
            res["pw"] = bk.predict(fit, Z, se_pred=True, ctx=ctx, matrices=False)
        t_full = timed(full)
        fse = res["full"]["se.pred"]
        del res["full"]
        ctx.release_workspace()
        torch.cuda.empty_cache()
        t_pw = timed(pw)
        dse = float(np.max(np.abs(res["pw"]["se.pred"] - fse)) / np.max(fse))
        print(json.dumps({"part": "b", "n": n, "p": p, "u": u, "matrices_true_ms": t_full, "matrices_false_ms": t_pw,
                          "speedup": t_full / t_pw, "se_max_abs_diff_over_max_se": dse}), flush=True)
        del Z, res
        ctx.release_workspace()
        torch.cuda.empty_cache()

    # ---- (c) u = 200 000 without the matrices ----------------------------------------------------------------------
    u = args.u_big
    Zh = np.random.default_rng(u).standard_normal((u, p))
    ctx.release_workspace()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    res = {}

    def big():
        res["pw"] = bk.predict(fit, Zh, se_pred=True, ctx=ctx, matrices=False)
    t_big = timed(big)
    torch.cuda.synchronize()
    ws = ctx.workspace_bytes()
    torch_peak = torch.cuda.max_memory_allocated() - base
    print(json.dumps({"part": "c", "n": n, "p": p, "u": u, "matrices_false_ms": t_big,
                      "workspace_bytes": ws, "torch_peak_extra_bytes": torch_peak,
                      "peak_extra_gib": (ws + torch_peak) / 2 ** 30,
                      "finite": bool(np.all(np.isfinite(res["pw"]["se.pred"]))),
                      "matrices_true_would_need_gb": 8.0 * u * (2 * n + u) / 1e9}), flush=True)
    ctx.release_workspace()


if __name__ == "__main__":
    main()
