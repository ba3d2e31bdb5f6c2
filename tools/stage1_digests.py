#!/usr/bin/env python3
"""Record (or check) the output digests that pin stage 1 of the dense eigensolver (Stage1 of csrc/eigen_2stage.inc, dist_s1_*
of csrc/eigen.hip).

    python tools/stage1_digests.py --lib PATH/libbigkrls_hip.so --commit HASH --write    # record from another build
    python tools/stage1_digests.py                                   # compare the tree's build, exit 1 on a difference

The cases are tests/_stage1_cases.py; the file is tests/golden/stage1_digests.json, which
tests/test_gpu_stage1_digests.py asserts against. Beside the digests the golden file keeps each case's plain figures
(lastkeeper; the panels pq_chol left to the Householder kernel) and the commit it was recorded from (--commit; default:
the tree's HEAD). It was recorded on an MI355X, twice with equal results, from a build of the commit before stage 1 was
split into the phases of one struct. When comparing, the "stage 1 schedule" line of each run must also show the counts
csrc/s1sched.h gives (COUNTS of the cases file)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stage1_digests.json")


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
    import _stage1_cases as cases
    ctx = bk.Context(0)
    recorded = {}
    for name in cases.case_names():
        res = cases.run_case(ctx, name, lib_path=_lib.LIB_PATH if args.lib else None)
        recorded[name] = res
        print(f"{name}: info {res['info']} counts {res['counts']}", flush=True)
    if args.write:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"recorded_from": args.commit or head_commit(),
                       "cases": {n: {"digests": r["digests"], "info": r["info"]} for n, r in recorded.items()}},
                      f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {len(recorded)} cases to {args.out}")
        return 0
    with open(args.out) as f:
        golden = json.load(f)["cases"]
    bad = [n for n in recorded if golden.get(n, {}).get("digests") != recorded[n]["digests"]]
    bad += [n for n in recorded if n not in bad and cases.COUNTS[n] is not None and recorded[n]["counts"] != list(cases.COUNTS[n])]
    for n in bad:
        print(f"DIFFERENT: {n}")
    print(f"{len(recorded) - len(bad)} cases equal, {len(bad)} different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
