"""Times the deletion residuals (bigkrls_dev_deletion_residuals) and influence() with HIP events, in one process: 3
warm-ups, the median of 10, at N = 20 000 rows and k = 250 factors.

  (a) primitive : Q with orthonormal columns, w in (0, 0.9); clusters of 2, 16, 64, MB = 128 rows and a mixed draw of
                  1 .. 250 rows. Route 0 (the fused kernel, one workgroup per unit: up to 128 rows with the matrix in LDS,
                  129 .. 256 with it in the workspace; only units above 256 rows go through the eigensolver, and no
                  shape below has one) against route 1 (EVERY unit through bigkrls_dev_gemm + bigkrls_dev_eigen + two gemv: what
                  a caller could assemble from the entries the library had before) on the same inputs. Route 1 makes one
                  eigensolver call per unit, so it is timed with fewer repetitions (--reps-general, default 3, 1 warm-up)
                  and, for the clusters of 2 and 16, on the first --general-units units only (default 500): its time per
                  unit is printed and the full time is that times the units, marked as an extrapolation.
  (b) call      : a fit at N = 20 000, P = 20 with 250 kept factors (Neig = 250); the whole influence(cluster=...) for the
                  same cluster shapes, and influence() for single rows.

Prints one JSON line per measurement.

    python tools/influence_bench.py [--n 20000] [--k 250] [--reps 10] [--skip-call]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MB = 128


def cluster_labels(n, kind, rng):
    if kind == "mixed":
        sizes = []
        while sum(sizes) < n:
            sizes.append(int(rng.integers(1, 251)))
        sizes[-1] -= sum(sizes) - n
        sizes = [s for s in sizes if s > 0]
    else:
        m = int(kind)
        sizes = [m] * (n // m) + ([n % m] if n % m else [])
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int64), len(sizes), sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--k", type=int, default=250)
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps-general", type=int, default=3)
    ap.add_argument("--general-units", type=int, default=500)
    ap.add_argument("--skip-call", action="store_true", help="part (a) only")
    args = ap.parse_args()
    import bigkrls_amd as bk
    from bigkrls_amd import _lib

    ctx = bk.Context(0)
    n, k = args.n, args.k
    rng = np.random.default_rng(11)

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

    # ---- (a) the primitive, route 0 against route 1 ------------------------------------------------------------------
    Q, _ = np.linalg.qr(rng.standard_normal((n, k)))
    w = np.ascontiguousarray(rng.uniform(0.0, 0.9, size=k))
    dQ = ctx.from_numpy(np.asfortranarray(Q))
    de = ctx.from_numpy(rng.standard_normal((n, 1)))
    det0, det1 = ctx.empty(n, 1), ctx.empty(n, 1)

    def call(labels, G, route, out, rows=n):
        _lib.call("bigkrls_dev_deletion_residuals", ctx.handle, rows, k, dQ.ptr, dQ.ld, w.ctypes.data, de.ptr,
                  labels.ctypes.data if labels is not None else None, G, route, out.ptr, None, None, 0)

    for kind in ("2", "16", "64", str(MB), "mixed"):
        labels, G, sizes = cluster_labels(n, kind, rng)
        perm = rng.permutation(n)
        shuffled = np.ascontiguousarray(labels[perm])
        t0 = timed(lambda: call(labels, G, 0, det0))
        t0s = timed(lambda: call(shuffled, G, 0, det0))
        ctx.set_profile(True)
        before = ctx.get_profile("deletion_residuals")
        call(labels, G, 0, det0)
        ctx.sync()
        after = ctx.get_profile("deletion_residuals")
        ctx.set_profile(False)
        # route 1 on the first units only where the units are many (grouped labels: the first rows)
        Gg = G if kind in ("64", str(MB), "mixed") else min(G, args.general_units)
        rows_g = int(np.sum(sizes[:Gg]))
        lab_g = np.ascontiguousarray(labels[:rows_g])
        t1 = timed(lambda: call(lab_g, Gg, 1, det1, rows=rows_g), reps=args.reps_general, warmup=1)
        call(lab_g, Gg, 0, det0, rows=rows_g)
        a, b = det0.to_numpy().ravel()[:rows_g], det1.to_numpy().ravel()[:rows_g]
        print(json.dumps({"part": "a", "n": n, "k": k, "clusters": kind, "units": G, "largest_unit": int(max(sizes)),
                          "route0_ms": t0, "route0_shuffled_labels_ms": t0s,
                          "route0_profile_ms": after[0] - before[0], "route0_profile_gflops": (after[1] - before[1]) / ((after[0] - before[0]) * 1e-3) / 1e9,
                          "route1_units_timed": Gg, "route1_ms": t1, "route1_ms_per_unit": t1 / Gg,
                          "route1_all_units_ms": t1 * G / Gg, "route1_all_units_is": "measured" if Gg == G else "an extrapolation: time per unit x units",
                          "route0_over_route1": t0 / (t1 * G / Gg),
                          "max_abs_diff_over_max": float(np.max(np.abs(a - b)) / np.max(np.abs(b)))}), flush=True)
    t_none = timed(lambda: call(None, 0, 0, det0))
    print(json.dumps({"part": "a", "n": n, "k": k, "clusters": "single rows (no labels)", "units": n, "route0_ms": t_none}), flush=True)
    del dQ, de, det0, det1
    ctx.release_workspace()
    if args.skip_call:
        return

    # ---- (b) the whole call ---------------------------------------------------------------------------------------------
    from bigkrls_amd.synth import synth
    X, y = synth(n, args.p, 103)
    fit = bk.bigKRLS(y, X, Neig=k, eigtrunc=0.0, instructions=False, noisy=False, ctx=ctx, vcov_form="factors")
    reps = max(3, args.reps // 3)
    for kind in ("2", "16", "64", str(MB), "mixed"):
        labels, G, sizes = cluster_labels(n, kind, rng)
        lab = labels[rng.permutation(n)]
        t = timed(lambda: bk.influence(fit, cluster=lab, ctx=ctx), reps=reps, warmup=1)
        print(json.dumps({"part": "b", "n": n, "p": args.p, "k": int(fit["lastkeeper"]), "clusters": kind, "units": G,
                          "influence_ms": t}), flush=True)
    t = timed(lambda: bk.influence(fit, ctx=ctx), reps=reps, warmup=1)
    t_fit = timed(lambda: bk.bigKRLS(y, X, Neig=k, eigtrunc=0.0, instructions=False, noisy=False, ctx=ctx, vcov_form="factors"),
                  reps=3, warmup=0)
    print(json.dumps({"part": "b", "n": n, "p": args.p, "k": int(fit["lastkeeper"]), "clusters": "single rows", "units": n,
                      "influence_ms": t, "one_fit_ms": t_fit, "refit_route_x_units_ms": t_fit * n,
                      "refit_route_is": "an extrapolation: one fit's time x N"}), flush=True)
    ctx.release_workspace()


if __name__ == "__main__":
    main()
