"""Times the interaction effects (interaction_effects) and their doubly modulated product with HIP events after warm-up,
in one process, on the C3 fit (n = 20 000, P = 20, k = its lastkeeper):

  (a) product : one bigkrls_dev_gemm_modulated2 call (m new points x k columns, contraction n) against one
                bigkrls_dev_gemm_modulated call at the same shape, and against the two-call chain it replaces --
                bigkrls_dev_gemm_modulated on Q plus bigkrls_dev_gemm_modulated on diag(s1) Q (that scaled copy is made
                once outside the timing). The chain's combination diag(r2) T_a + diag(t2) T_b is NOT timed, so the
                comparison favours the chain. The variants are alternated call by call inside every repetition, and the
                whole measurement (warm-up, --reps repetitions, medians) is repeated --rounds times: the spread of the
                rounds' medians is the run-to-run spread to judge the ratios against.
  (b) call    : interaction_effects over all P (P + 1) / 2 pairs from the factors, u new points, se=False and se=True
  (c) memory  : peak device memory of the calls of (b) (torch allocator peak + library workspace)

Prints one JSON line per measurement.

    python tools/interaction_effects_bench.py [--reps 10] [--rounds 3] [--n 20000] [--p 20] [--m 6656 2048] [--u 5000 20000]
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--m", type=int, nargs="*", default=[6656, 2048])
    ap.add_argument("--u", type=int, nargs="*", default=[5000, 20000])
    args = ap.parse_args()
    import torch
    import bigkrls_amd as bk
    from bigkrls_amd import _lib
    from bigkrls_amd.synth import synth

    ctx = bk.Context(0)
    n, p = args.n, args.p

    def timed_alternated(variants, reps=args.reps, warmup=args.warmup):
        """{name: median ms}: every repetition runs each variant once, in turn"""
        for _ in range(warmup):
            for fn in variants.values():
                fn()
        ctx.sync()
        ts = {name: [] for name in variants}
        for _ in range(reps):
            for name, fn in variants.items():
                e0 = ctx.event()
                fn()
                e1 = ctx.event()
                ctx.sync()
                ts[name].append(ctx.elapsed_ms(e0, e1))
                ctx.release_events([e0, e1])
        return {name: float(np.median(v)) for name, v in ts.items()}

    X, y = synth(n, p, 103)
    fit = bk.bigKRLS(y, X, eigtrunc=0.001, derivative=False, instructions=False, noisy=False, ctx=ctx,
                     vcov_form="factors")
    Q, k = fit["vcov.est.Q"], fit["lastkeeper"]
    Xs = (X - X.mean(axis=0)) / X.std(axis=0, ddof=1)

    # ---- (a) one product: modulated2 against modulated and against the two-call chain -------------------------------
    rng = np.random.default_rng(n)
    dS = ctx.from_numpy(Xs[:, :2])                                      # s1, s2: two columns of Xs
    QS = ctx.from_numpy(Q.to_numpy() * Xs[:, :1])                       # diag(s1) Q, made once outside the timing
    for m in args.m:
        A = ctx.from_numpy(rng.random((m, n)))
        R, Tm = ctx.from_numpy(rng.standard_normal((m, 2))), ctx.from_numpy(rng.standard_normal((m, 2)))
        T, Tb = ctx.empty(m, k), ctx.empty(m, k)

        def modulated2():
            _lib.call("bigkrls_dev_gemm_modulated2", ctx.handle, m, k, n, A.ptr, A.ld, R.col_ptr(0), Tm.col_ptr(0),
                      dS.col_ptr(0), R.col_ptr(1), Tm.col_ptr(1), dS.col_ptr(1), -0.1, Q.ptr, Q.ld, T.ptr, T.ld)

        def modulated():
            _lib.call("bigkrls_dev_gemm_modulated", ctx.handle, m, k, n, A.ptr, A.ld, R.col_ptr(0), Tm.col_ptr(0),
                      dS.col_ptr(0), Q.ptr, Q.ld, T.ptr, T.ld)

        def chain():
            _lib.call("bigkrls_dev_gemm_modulated", ctx.handle, m, k, n, A.ptr, A.ld, R.col_ptr(0), Tm.col_ptr(0),
                      dS.col_ptr(0), Q.ptr, Q.ld, T.ptr, T.ld)
            _lib.call("bigkrls_dev_gemm_modulated", ctx.handle, m, k, n, A.ptr, A.ld, R.col_ptr(0), Tm.col_ptr(0),
                      dS.col_ptr(0), QS.ptr, QS.ld, Tb.ptr, Tb.ld)

        def plain():
            _lib.call("bigkrls_dev_gemm", ctx.handle, 0, 0, m, k, n, 1.0, A.ptr, A.ld, Q.ptr, Q.ld, 0.0, T.ptr, T.ld)

        for rnd in range(args.rounds):
            t = timed_alternated({"modulated2": modulated2, "modulated": modulated, "chain": chain, "plain": plain})
            print(json.dumps({"part": "a", "round": rnd, "m": m, "n": n, "k": k, "modulated2_ms": t["modulated2"],
                              "modulated_ms": t["modulated"], "two_call_chain_ms": t["chain"], "plain_gemm_ms": t["plain"],
                              "modulated2_over_modulated": t["modulated2"] / t["modulated"],
                              "modulated2_over_chain": t["modulated2"] / t["chain"],
                              "modulated2_tflops": 2.0 * m * n * k / (t["modulated2"] * 1e-3) / 1e12}), flush=True)
        del A, R, Tm, T, Tb
        ctx.release_workspace()
    del QS, dS

    # ---- (b), (c): the call over all pairs with and without se; peak memory ------------------------------------------
    npairs = p * (p + 1) // 2
    for u in args.u:
        Zh = np.random.default_rng(u).standard_normal((u, p))
        for se in (False, True):
            reps = args.reps if not se else max(3, args.reps // 3)
            ctx.release_workspace()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t = timed_alternated({"call": lambda: bk.interaction_effects(fit, Zh, ctx=ctx, vcov="factors", se=se)},
                                 reps=reps, warmup=1)["call"]
            peak = torch.cuda.max_memory_allocated() - base + ctx.workspace_bytes()
            row = {"part": "b", "n": n, "p": p, "k": k, "pairs": npairs, "u": u, "se": se, "call_ms": t}
            print(json.dumps(row), flush=True)
            print(json.dumps({"part": "c", "u": u, "se": se, "peak_device_gb": peak / 1e9}), flush=True)
    ctx.release_workspace()


if __name__ == "__main__":
    main()
