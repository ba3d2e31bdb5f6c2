#!/usr/bin/env python3
"""Record (or check) the output digests of the block Lanczos eigensolver (eigen_krylov of csrc/eigen.hip).

    python tools/block_lanczos_digests.py --lib PATH/libbigkrls_hip.so --fault-lib PATH/libbigkrls_hip_fault.so \
        --commit HASH --write                                                    # record from another build
    python tools/block_lanczos_digests.py                                        # compare the tree's build, exit 1 on a difference

The cases are tests/_block_lanczos_cases.py; the file is tests/golden/block_lanczos_digests.json, which
tests/test_gpu_block_lanczos_digests.py asserts against. Every case runs under BIGKRLS_VERBOSE=1 with the process's
stderr (the library's, and that of the child process of the test-build case) collected in a file: beside the digests the
golden file keeps which path markers (MARKERS of the cases file) each case showed, and the commit it was recorded from
(--commit; default: the tree's HEAD). It was recorded on an MI355X from a build of the commit before the iteration was
split into the phases of one struct."""
import argparse
import contextlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "block_lanczos_digests.json")


@contextlib.contextmanager
def stderr_to(path):
    """File descriptor 2 of this process (and of what it starts) appended to `path` for the duration."""
    sys.stderr.flush()
    saved = os.dup(2)
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_APPEND, 0o644)
    os.dup2(fd, 2)
    os.close(fd)
    try:
        yield
    finally:
        sys.stderr.flush()
        os.dup2(saved, 2)
        os.close(saved)


def run_with_markers(ctx, cases, name):
    """run_case under BIGKRLS_VERBOSE=1: (result, sorted names of the markers its stderr showed, the stderr text)."""
    with tempfile.TemporaryDirectory() as tmp:
        log = os.path.join(tmp, "stderr.log")
        had = os.environ.get("BIGKRLS_VERBOSE")
        os.environ["BIGKRLS_VERBOSE"] = "1"
        try:
            with stderr_to(log):
                res = cases.run_case(ctx, name)
        finally:
            if had is None:
                del os.environ["BIGKRLS_VERBOSE"]
        with open(log) as f:
            text = f.read()
    return res, sorted(m for m, needle in cases.MARKERS.items() if needle in text), text


def head_commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libbigkrls_hip.so (default: the tree's)")
    ap.add_argument("--fault-lib", default=None, help="the test build (libbigkrls_hip_fault.so) that goes with --lib")
    ap.add_argument("--commit", default=None, help="the commit the library was built from (default: HEAD)")
    ap.add_argument("--write", action="store_true", help="write the golden file instead of comparing with it")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--show-stderr", action="store_true", help="print each case's verbose lines")
    args = ap.parse_args()
    from bigkrls_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    if args.fault_lib:
        os.environ["BIGKRLS_FAULT_LIB"] = os.path.abspath(args.fault_lib)
    import bigkrls_amd as bk
    import _block_lanczos_cases as cases
    ctx = bk.Context(0)
    recorded = {}
    for name in cases.case_names():
        res, markers, text = run_with_markers(ctx, cases, name)
        recorded[name] = {"digests": res["digests"], "info": res["info"], "markers": markers}
        print(f"{name}: markers {markers} info {res['info']}", flush=True)
        if args.show_stderr:
            print("".join("    " + line + "\n" for line in text.splitlines() if "block Lanczos" in line), end="", flush=True)
    if args.write:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"recorded_from": args.commit or head_commit(), "cases": recorded}, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {len(recorded)} cases to {args.out}")
        return 0
    with open(args.out) as f:
        golden = json.load(f)["cases"]
    bad = [n for n in recorded if golden.get(n, {}).get("digests") != recorded[n]["digests"]]
    bad += [n for n in recorded if n not in bad and golden[n]["markers"] != recorded[n]["markers"]]
    for n in bad:
        print(f"DIFFERENT: {n}")
    print(f"{len(recorded) - len(bad)} cases equal, {len(bad)} different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
