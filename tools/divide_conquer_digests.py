#!/usr/bin/env python3
"""Record (or check) the output digests and per-level figures that pin the divide & conquer of the dense eigensolver
(DivideConquer of csrc/eigen.hip, csrc/dcplan.h).

    python tools/divide_conquer_digests.py --lib PATH/libbigkrls_hip.so --commit HASH --write   # record from another build
    python tools/divide_conquer_digests.py                           # compare the tree's build, exit 1 on a difference

The cases are tests/_divide_conquer_cases.py; the file is tests/golden/divide_conquer_digests.json, which
tests/test_gpu_divide_conquer_digests.py asserts against. Per case the golden file keeps the digest of the input, the
digests of the outputs, lastkeeper, and the path: the figures of every "d&c depth" line and whether the "redoing" /
"factored levels applied" lines appeared. It also keeps the commit it was recorded from (--commit; default: the tree's
HEAD). --write runs every case twice and refuses to write unless the two recordings are equal. The file was recorded on
an MI355X from a build of the commit before the divide & conquer was split into the phases of one struct."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "divide_conquer_digests.json")


def head_commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def record(ctx, cases):
    recorded = {}
    for name in cases.case_names():
        res = cases.run_case(ctx, name)
        recorded[name] = res
        print(f"{name}: info {res['info']} redo {res['path']['redo']} applied {res['path']['applied']} "
              f"levels {res['path']['levels']}", flush=True)
    return recorded


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
    import _divide_conquer_cases as cases
    ctx = bk.Context(0)
    recorded = record(ctx, cases)
    if args.write:
        again = record(ctx, cases)
        differ = [n for n in recorded if recorded[n] != again[n]]
        if differ:
            print(f"the two recordings differ: {differ}")
            return 1
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"recorded_from": args.commit or head_commit(), "cases": recorded}, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {len(recorded)} cases to {args.out} (two equal recordings)")
        return 0
    with open(args.out) as f:
        golden = json.load(f)["cases"]
    bad = []
    for n, r in recorded.items():
        g = golden.get(n, {})
        what = [k for k in ("input", "digests", "info", "path") if g.get(k) != r[k]]
        if what:
            bad.append(n)
            print(f"DIFFERENT: {n}: {', '.join(what)}")
    print(f"{len(recorded) - len(bad)} cases equal, {len(bad)} different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
