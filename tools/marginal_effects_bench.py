"""Times the two fused kernel contractions behind marginal_effects() against the unfused chain they replace, with HIP
events after warm-up, in one process:

  fused   : R = Kn B (u x q) and C = Kn' B* (n x q), q = 1 + |J|, Kn rebuilt in registers (bigkrls_dev_kernel_contract)
  unfused : Kn (u x n) = bigkrls_dev_kernel_block, then Kn B and Kn' B* with bigkrls_dev_gemm

Prints one JSON line per shape: median times, the flop model of the fused kernels and their share of the fp64 MFMA
peak. The unfused chain needs 8 u n bytes for Kn; it is skipped (reported as null) where that exceeds --max-kn-gb.

    python tools/marginal_effects_bench.py [--reps 10] [--max-kn-gb 8] [--shapes 20000,20000,20,20 ...]
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-kn-gb", type=float, default=8.0)
    ap.add_argument("--shapes", nargs="*", default=["20000,20000,20,20", "20000,200000,20,20"],
                    help="n,u,p,|J| per shape")
    args = ap.parse_args()
    import bigkrls_amd as bk
    from bigkrls_amd import _lib, ops

    ctx = bk.Context(0)
    for shape in args.shapes:
        n, u, p, nj = (int(x) for x in shape.split(","))
        q = 1 + nj
        rng = np.random.default_rng(n + u)
        Xs, Zs = ctx.from_numpy(rng.standard_normal((n, p))), ctx.from_numpy(rng.standard_normal((u, p)))
        B, Bs = ctx.from_numpy(rng.standard_normal((n, q))), ctx.from_numpy(rng.standard_normal((u, q)))
        sigma = float(p)

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
            return float(np.median(ts))

        R = ctx.empty(u, q)
        Cm = ctx.empty(n, q)

        def row():
            _lib.call("bigkrls_dev_kernel_contract", ctx.handle, Zs.ptr, u, Zs.ld, Xs.ptr, n, Xs.ld, p, sigma,
                      B.ptr, q, B.ld, 0, R.ptr, R.ld)

        def col():
            _lib.call("bigkrls_dev_kernel_contract", ctx.handle, Zs.ptr, u, Zs.ld, Xs.ptr, n, Xs.ld, p, sigma,
                      Bs.ptr, q, Bs.ld, 1, Cm.ptr, Cm.ld)
        t_row, t_col = timed(row), timed(col)
        ctx.release_workspace()

        unf = None
        kn_gb = 8.0 * u * n / 1e9
        if kn_gb <= args.max_kn_gb:
            Kn = ctx.empty(u, n)
            R2, C2 = ctx.empty(u, q), ctx.empty(n, q)

            def kb():
                _lib.call("bigkrls_dev_kernel_block", ctx.handle, Zs.ptr, u, Zs.ld, Xs.ptr, n, Xs.ld, p, sigma,
                          Kn.ptr, Kn.ld, -1)

            def gn():
                _lib.call("bigkrls_dev_gemm", ctx.handle, 0, 0, u, q, n, 1.0, Kn.ptr, Kn.ld, B.ptr, B.ld, 0.0,
                          R2.ptr, R2.ld)

            def gt():
                _lib.call("bigkrls_dev_gemm", ctx.handle, 1, 0, n, q, u, 1.0, Kn.ptr, Kn.ld, Bs.ptr, Bs.ld, 0.0,
                          C2.ptr, C2.ld)
            t_kb, t_gn, t_gt = timed(kb), timed(gn), timed(gt)
            err = max(float(np.max(np.abs(R.to_numpy() - R2.to_numpy())) / np.max(np.abs(R2.to_numpy()))),
                      float(np.max(np.abs(Cm.to_numpy() - C2.to_numpy())) / np.max(np.abs(C2.to_numpy()))))
            unf = {"kernel_block": t_kb, "gemm_KnB": t_gn, "gemm_KntBs": t_gt, "total": t_kb + t_gn + t_gt,
                   "fused_vs_unfused_rel_err": err}
            del Kn, R2, C2
            ctx.release_workspace()
        # flop model of one fused kernel per Kn entry: X Xs' over p padded to 4, contraction over q padded to 16 / 32 / 64
        ct = 1 if q <= 16 else (2 if q <= 32 else 4)
        qpad = -(-q // (16 * ct)) * 16 * ct
        per_entry = 2 * 4 * (-(-p // 4)) + 2 * qpad
        flops = float(per_entry) * u * n
        rec = {"n": n, "u": u, "p": p, "J": nj, "fused_ms": {"row": t_row, "col": t_col, "total": t_row + t_col},
               "unfused_ms": unf, "unfused_kn_gb": kn_gb,
               "mfma_flop_per_entry": per_entry,
               "fused_tflops": {"row": flops / t_row / 1e9, "col": flops / t_col / 1e9},
               "share_of_fp64_peak": {"row": flops / t_row / 1e-3 / FP64_PEAK, "col": flops / t_col / 1e-3 / FP64_PEAK},
               "speedup_vs_unfused": None if unf is None else unf["total"] / (t_row + t_col)}
        print(json.dumps(rec), flush=True)
        del Xs, Zs, B, Bs, R, Cm
        ctx.release_workspace()


if __name__ == "__main__":
    main()
