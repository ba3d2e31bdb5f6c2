"""The host plan of the dense eigensolver's back half (bigkrls_amd/csrc/s2plan.h: the bulge-chasing wavefronts, arm and
grid; the stage-2 back-transform's task geometry, anti-diagonals, flag layout and arm; the merged groups of the stage-1
back-transform; the regions of the two-stage workspace) is plain C++: a stand-alone host program (tests/s2plan_check.cpp,
with its own main) enumerates it over n = 1 .. 2 600 and five large sizes, checks by brute force what the kernels rely on
(every task once, no invalid task, predecessors on earlier wavefronts, offsets that count the valid steps, groups that
tile the panels, regions that tile their slots, a ticket clear of the flags) and requires every plan to equal
tests/golden/s2_plans.txt row for row. That file was recorded once from the statements csrc/eigen.hip and
csrc/eigen_2stage.inc held before they moved. Built with -fsanitize=address,undefined. No GPU, no HIP, nothing loaded
into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_s2plan_check_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "s2plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bigkrls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "s2plan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "s2_plans.txt")], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "s2plan_check: ok" in run.stdout
