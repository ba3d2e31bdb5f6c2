"""The three products of one step of the stage-1 back-transform (back_transform_stage1_grouped, csrc/eigen_2stage.inc),
alone on the GPU, at every tile width gemm_thin can run them with (bigkrls_dev_gemm_thin, force_bn = 128, 64, 32) and
under its rule (0):

    p1  W1 = Vb' Zs     (w x m0)(m0 x nv), split over K, with its slab reduction
    p2  W2 = Tb W1      w x w x nv
    p3  Zs -= Vb W2     m0 x w x nv
    step                the three in order, as the back-transform issues them

Each figure is the median over --reps of a window of --inner launches between two HIP events, divided by --inner. Vb
rotates over --nbuf buffers from launch to launch, so that it is not simply found in the cache where the previous launch
left it (in the eigensolver every step has a Vb of its own). The constants of thin_plan's rule (csrc/splitplan.h) were
chosen from this table. Development tool; prints a table and one JSON line per shape.

    python tools/bt1_thin_bench.py [--shapes m0:nv:w ...] [--reps 15] [--inner 10] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTHS = (128, 64, 32, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["20000:250:512", "15000:250:512", "10000:250:512", "5000:250:512",
                                                    "2000:250:512", "5000:300:512", "2500:300:512", "1000:300:512"])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--nbuf", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bigkrls_amd as bk
    from bigkrls_amd import _lib

    ctx = bk.Context(0)
    lib = _lib.load()
    thin = lib.bigkrls_dev_gemm_thin
    i64, f64, vp = C.c_int64, C.c_double, C.c_void_p
    thin.argtypes = [vp, C.c_int, C.c_int, i64, i64, i64, f64, vp, i64, vp, i64, f64, vp, i64, C.c_int]
    thin.restype = C.c_int

    def timed(fn):
        for i in range(2 * args.nbuf):
            fn(i)
        ctx.sync()
        ts = []
        for _ in range(args.reps):
            e0 = ctx.event()
            for i in range(args.inner):
                fn(i)
            e1 = ctx.event()
            ctx.sync()
            ts.append(ctx.elapsed_ms(e0, e1) * 1e3 / args.inner)
            ctx.release_events([e0, e1])
        return float(np.median(ts))

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("us per launch (median of %d windows of %d launches); Vb rotates over %d buffers" % (args.reps, args.inner, args.nbuf))
    say("%-18s %-5s" % ("m0:nv:w", "what") + "".join("%10s" % (f"bn={w}" if w else "rule") for w in WIDTHS))
    for shape in args.shapes:
        m0, nv, w = (int(t) for t in shape.split(":"))
        rng = np.random.default_rng(m0 + nv)
        Vb = [ctx.from_numpy(rng.standard_normal((m0, w)) / np.sqrt(m0)) for _ in range(args.nbuf)]
        Tb = ctx.from_numpy(1e-4 * rng.standard_normal((w, w)) / np.sqrt(w))     # small: Zs stays bounded over the launches
        Zs = ctx.from_numpy(rng.standard_normal((m0, nv)))
        W1, W2 = ctx.from_numpy(np.zeros((w, nv))), ctx.from_numpy(np.zeros((w, nv)))
        rec = {"m0": m0, "nv": nv, "w": w, "us": {}}
        for what in ("p1", "p2", "p3", "step"):
            row = []
            for bn in WIDTHS:
                def p1(i):
                    V = Vb[i % args.nbuf]
                    _lib.check(thin(ctx.handle, 1, 0, w, nv, m0, 1.0, V.ptr, V.ld, Zs.ptr, Zs.ld, 0.0, W1.ptr, W1.ld, bn))

                def p2(i):
                    _lib.check(thin(ctx.handle, 0, 0, w, nv, w, 1.0, Tb.ptr, Tb.ld, W1.ptr, W1.ld, 0.0, W2.ptr, W2.ld, bn))

                def p3(i):
                    V = Vb[i % args.nbuf]
                    _lib.check(thin(ctx.handle, 0, 0, m0, nv, w, -1.0, V.ptr, V.ld, W2.ptr, W2.ld, 1.0, Zs.ptr, Zs.ld, bn))

                def step(i):
                    p1(i), p2(i), p3(i)
                row.append(timed({"p1": p1, "p2": p2, "p3": p3, "step": step}[what]))
            rec["us"][what] = dict(zip((str(x) for x in WIDTHS), row))
            say("%-18s %-5s" % (shape, what) + "".join("%10.1f" % t for t in row))
        assert np.isfinite(Zs.to_numpy()).all()
        say(json.dumps(rec))
        del Vb, Tb, Zs, W1, W2
        ctx.release_workspace()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
