#!/usr/bin/env python3
"""Time bigkrls_dev_kernel_contract at q > 64 (the wide kernel's range), for same-box A/B runs of two builds.

    python tools/contract_wide_ab.py [--lib PATH/libbigkrls_hip.so] [--reps 15]

Shapes: K(X, X) W with n = 20 000, P = 20 and n = 50 000, P = 50, q = 128 (the Lanczos block) and q = 104 (the
marginal-effects operand of P = 50). Per shape: 3 warm-up calls, then the median and the spread of `reps` calls
timed with events on the launch stream. `--lib` loads another build of the library (e.g. the parent commit's) instead
of the tree's, so that both run in fresh processes on the same box, alternately. One JSON line per shape."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--label", default="tree")
    args = ap.parse_args()
    from bigkrls_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    import numpy as np
    import torch
    import bigkrls_amd as bk
    from bigkrls_amd import ops
    ctx = bk.Context(0)
    for n, p, q in [(20000, 20, 128), (50000, 50, 128), (50000, 50, 104)]:
        rng = np.random.default_rng(n + p + q)
        X = ctx.from_numpy(rng.standard_normal((n, p)))
        W = ctx.from_numpy(rng.standard_normal((n, q)))
        for _ in range(3):
            ops.bKernelContract(X, X, W, float(p))
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.bKernelContract(X, X, W, float(p))
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        flops = 2.0 * n * n * (p + q)
        print(json.dumps({"label": args.label, "n": n, "p": p, "q": q, "median_ms": round(ms[len(ms) // 2], 3),
                          "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
                          "tflops_at_median": round(flops / (ms[len(ms) // 2] * 1e-3) / 1e12, 2)}), flush=True)
        del X, W


if __name__ == "__main__":
    main()
