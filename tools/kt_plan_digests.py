#!/usr/bin/env python3
"""Record (or check) the output digests of the kernel builds, the long grouped tables and the many-launch leave-out
moments.

    python tools/kt_plan_digests.py --lib PATH/libbigkrls_hip.so --write     # record from another build
    python tools/kt_plan_digests.py                                          # compare the tree's build, exit 1 on a difference

The cases and inputs are tests/_kt_plan_cases.py; the file is tests/golden/kt_plan_digests.json, which
tests/test_gpu_kt_plan_digests.py asserts against. It was recorded with --lib pointing at a build of the commit before
the host plans moved into csrc/ktplan.h, on an MI355X. The compiler's version string is stored for information."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kt_plan_digests.json")


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
    import _kt_plan_cases as cases
    ctx = bk.Context(0)
    digests = {name: cases.run_case(ctx, name) for name in cases.case_names()}
    if args.write:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"recorded_from": "a build of the parent of the commit that moved the host plans into csrc/ktplan.h",
                       "compiler": compiler_version(), "digests": digests}, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {sum(len(v) for v in digests.values())} digests of {len(digests)} cases to {args.out}")
        return 0
    with open(args.out) as f:
        golden = json.load(f)["digests"]
    bad = [(n, s) for n in digests for s in digests[n] if golden.get(n, {}).get(s) != digests[n][s]]
    for n, s in bad:
        print(f"DIFFERENT: {n} {s}")
    print(f"{sum(len(v) for v in digests.values()) - len(bad)} digests equal, {len(bad)} different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
