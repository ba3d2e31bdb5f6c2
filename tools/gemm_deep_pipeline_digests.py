#!/usr/bin/env python3
"""Record (or check) the output digests of the k-tile sweep over gemm_tile's two-tiles-in-flight path (csrc/gemm.hip).

    python tools/gemm_deep_pipeline_digests.py --lib PATH/libbigkrls_hip.so --write   # record from another build
    python tools/gemm_deep_pipeline_digests.py                                        # compare the tree's build, exit 1 on a difference

The groups and inputs are tests/_gemm_deep_pipeline_cases.py; the file is tests/golden/gemm_deep_pipeline_digests.json,
which tests/test_gpu_gemm_deep_pipeline.py asserts against. It was recorded with --lib pointing at a build of the commit
before the interior loop of the two-tiles-in-flight path, on an MI355X. Each group's largest error against the numpy
reference, in units of its bound, is printed too. The compiler's version string is stored for information."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_deep_pipeline_digests.json")


def compiler_version():
    try:
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True)
        return " | ".join(line.strip() for line in r.stdout.splitlines()[:2])
    except OSError:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libbigkrls_hip.so (default: the tree's)")
    ap.add_argument("--write", action="store_true", help="write the golden file instead of comparing with it")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from bigkrls_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    import bigkrls_amd as bk
    import _gemm_deep_pipeline_cases as cases
    ctx = bk.Context(0)
    digests, outside = {}, 0
    for name in cases.group_names():
        digests[name], figures = cases.run_group(ctx, name)
        worst = max(figures, key=lambda f: f[1])
        outside += sum(1 for _, r, finite in figures if not (finite and r <= 1.0))
        print(f"{name}: {len(figures)} sub-cases, largest error / bound {worst[1]:.3g} at {worst[0]}")
    print(f"{outside} sub-cases outside the bound")
    if args.write:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"recorded_from": "a build of the parent of the commit that introduced the interior loop of gemm_tile's two-tiles-in-flight path",
                       "compiler": compiler_version(), "digests": digests}, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {len(digests)} digests to {args.out}")
        return 1 if outside else 0
    with open(args.out) as f:
        golden = json.load(f)["digests"]
    bad = [n for n in digests if golden.get(n) != digests[n]]
    for n in bad:
        print(f"DIFFERENT: {n}")
    print(f"{len(digests) - len(bad)} digests equal, {len(bad)} different")
    return 1 if bad or outside else 0


if __name__ == "__main__":
    sys.exit(main())
