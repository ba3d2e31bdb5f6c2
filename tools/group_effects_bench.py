"""Times the grouped fused contraction behind group_effects() against what the library offered before it, with HIP
events after warm-up, in one process, at n = u, random labels, G groups:

  (a) grouped : ONE bigkrls_dev_kernel_contract_grouped (labels in random order: the gather of the rows is inside the time)
  (b) G calls : bigkrls_dev_kernel_contract(trans = 1) on each group's rows (the rows sorted beforehand and addressed in
                place, so that the baseline pays no copy)                                   -- the baseline
  (c) padded  : one bigkrls_dev_kernel_contract(trans = 1) with G q columns, block g zero outside the rows of group g
                (G <= --max-padded-groups only: G times the MFMA work)

and, with --e2e, group_effects() on a fit of that size against G calls of marginal_effects() (wall clock, the factors of
vcov.est.c). Prints one JSON line per G: median times in ms, the largest difference between (a) and (b) relative to the
largest entry, and (a) / (b).

    python tools/group_effects_bench.py [--n 20000] [--p 20] [--J 20] [--groups 1 4 50 400] [--reps 10] [--e2e]

--sorted: the labels in ascending order (no permutation, no gather: the host's plan is all that stands before the pass);
--grouped-only: (a) alone; --lib PATH: another build of libbigkrls_hip.so, to compare two builds on one machine.
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
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--J", type=int, default=20)
    ap.add_argument("--groups", type=int, nargs="*", default=[1, 4, 50, 400])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-padded-groups", type=int, default=50)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--sorted", action="store_true")
    ap.add_argument("--grouped-only", action="store_true")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    from bigkrls_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    import bigkrls_amd as bk

    ctx = bk.Context(0)
    n = u = args.n
    p, q = args.p, 1 + args.J
    sigma = float(p)
    rng = np.random.default_rng(n + p)
    Xh, Zh, Wh = rng.standard_normal((n, p)), rng.standard_normal((u, p)), rng.standard_normal((u, q))
    Xs, Zs, W = ctx.from_numpy(Xh), ctx.from_numpy(Zh), ctx.from_numpy(Wh)

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

    fit = None
    if args.e2e:
        y = Xh[:, 0] + np.sin(Xh[:, 1]) + 0.1 * rng.standard_normal(n)
        fit = bk.bigKRLS(y, Xh, Neig=min(n // 4, 400), vcov_form="factors", derivative=False, ctx=ctx, noisy=False)

    for G in args.groups:
        labels = np.ascontiguousarray(rng.integers(0, G, size=u), dtype=np.int64)
        if args.sorted:
            labels = np.sort(labels)
        order = np.argsort(labels, kind="stable")
        off = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=G))])
        out = ctx.empty(n, G * q)

        def grouped():
            _lib.call("bigkrls_dev_kernel_contract_grouped", ctx.handle, Zs.ptr, u, Zs.ld, Xs.ptr, n, Xs.ld, p, sigma,
                      W.ptr, q, W.ld, labels.ctypes.data, G, out.ptr, out.ld)
        t_a = timed(grouped)
        got = out.to_numpy()
        if args.grouped_only:
            print(json.dumps({"n": n, "u": u, "p": p, "q": q, "G": G, "sorted": args.sorted, "grouped_ms": t_a}), flush=True)
            del out
            ctx.release_workspace()
            continue

        Zsort, Wsort = ctx.from_numpy(np.asfortranarray(Zh[order])), ctx.from_numpy(np.asfortranarray(Wh[order]))
        out_b = ctx.empty(n, G * q)

        def per_group():
            for g in range(G):
                ug = int(off[g + 1] - off[g])
                if ug == 0:
                    continue
                _lib.call("bigkrls_dev_kernel_contract", ctx.handle, Zsort.col_ptr(0, off[g]), ug, Zsort.ld, Xs.ptr, n,
                          Xs.ld, p, sigma, Wsort.col_ptr(0, off[g]), q, Wsort.ld, 1, out_b.col_ptr(g * q), out_b.ld)
        t_b = timed(per_group)
        want = out_b.to_numpy()
        nonempty = np.repeat(np.diff(off) > 0, q)
        err = float(np.max(np.abs(got[:, nonempty] - want[:, nonempty])) / np.max(np.abs(want[:, nonempty])))
        del Zsort, Wsort, out_b

        t_c = None
        if G <= args.max_padded_groups:
            Wp = np.zeros((u, G * q), order="F")
            for g in range(G):
                rows = labels == g
                Wp[rows, g * q:(g + 1) * q] = Wh[rows]
            dWp = ctx.from_numpy(Wp)
            out_c = ctx.empty(n, G * q)

            def padded():
                _lib.call("bigkrls_dev_kernel_contract", ctx.handle, Zs.ptr, u, Zs.ld, Xs.ptr, n, Xs.ld, p, sigma,
                          dWp.ptr, G * q, dWp.ld, 1, out_c.ptr, out_c.ld)
            t_c = timed(padded)
            del dWp, out_c, Wp
        rec = {"n": n, "u": u, "p": p, "q": q, "G": G, "grouped_ms": t_a, "per_group_calls_ms": t_b, "padded_ms": t_c,
               "grouped_vs_calls_rel_diff": err, "grouped_over_calls": t_a / t_b}
        del out
        ctx.release_workspace()

        if fit is not None:
            def wall(fn):
                fn()
                ts = []
                for _ in range(args.e2e_reps):
                    ctx.sync()
                    t0 = time.perf_counter()
                    fn()
                    ctx.sync()
                    ts.append((time.perf_counter() - t0) * 1e3)
                return float(np.median(ts))
            which = list(range(1, min(args.J, 4096 // G) + 1))        # (group_effects() takes G |J| <= 4096)
            rec["e2e_J"] = len(which)
            groups_rows = [Xh[labels == g] for g in range(G)]
            rec["group_effects_ms"] = wall(lambda: bk.group_effects(fit, labels, which_derivatives=which, ctx=ctx))
            rec["marginal_effects_calls_ms"] = wall(lambda: [bk.marginal_effects(fit, r, which_derivatives=which, ctx=ctx)
                                                             for r in groups_rows if r.shape[0] > 0])
            ctx.release_workspace()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
