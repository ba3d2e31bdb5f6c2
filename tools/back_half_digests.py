#!/usr/bin/env python3
"""Record (or check) the output digests that pin the back half of the dense eigensolver: band to tridiagonal, the stage-2
back-transform and the stage-1 back-transform (csrc/eigen_2stage.inc, csrc/s2plan.h).

    python tools/back_half_digests.py --lib PATH/libbigkrls_hip.so --commit HASH --write    # record from another build
    python tools/back_half_digests.py                                 # compare the tree's build, exit 1 on a difference

The cases are tests/_back_half_cases.py; the file is tests/golden/back_half_digests.json, which
tests/test_gpu_back_half_digests.py asserts against. Beside the digests the golden file keeps each case's input digest,
its lastkeeper and the commit it was recorded from (--commit; default: the tree's HEAD). --write runs every case twice and
refuses to record a case whose two runs differ: an arm that does not reproduce pins nothing."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "back_half_digests.json")


def head_commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libbigkrls_hip.so (default: the tree's)")
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: HEAD)")
    ap.add_argument("--write", action="store_true", help="write the golden file instead of comparing with it")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from bigkrls_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    import bigkrls_amd as bk
    import _back_half_cases as cases
    ctx = bk.Context(0)
    lib_path = _lib.LIB_PATH if args.lib else None
    recorded, unstable = {}, []
    for name in cases.case_names():
        res = cases.run_case(ctx, name, lib_path=lib_path)
        if args.write and cases.run_case(ctx, name, lib_path=lib_path) != res:
            unstable.append(name)
        recorded[name] = res
        print(f"{name}: info {res['info']} values {res['digests']['values'][:12]} vectors {res['digests']['vectors'][:12]}"
              f"{' NOT REPRODUCED' if name in unstable else ''}", flush=True)
    if args.write:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"recorded_from": args.commit or head_commit(),
                       "cases": {n: r for n, r in recorded.items() if n not in unstable}}, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {len(recorded) - len(unstable)} cases to {args.out}; two runs differed for: {unstable or 'none'}")
        return 1 if unstable else 0
    with open(args.out) as f:
        golden = json.load(f)["cases"]
    bad = [n for n in recorded if golden.get(n) != recorded[n]]
    for n in bad:
        print(f"DIFFERENT: {n}")
    print(f"{len(recorded) - len(bad)} cases equal, {len(bad)} different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
