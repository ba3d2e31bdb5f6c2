"""The host plans of the kernel builds and the fused kernel-tile entry points (bigkrls_amd/csrc/ktplan.h: the stable
group order, the segments of the grouped pass, the launches of the leave-out moments, the arm and grid of a kernel build)
are plain C++: a stand-alone host program (tests/ktplan_check.cpp, with its own main) enumerates them over grids of
sizes, labels, slot counts and switches, checks what the kernels rely on against brute force (stable permutations,
segments that tile their groups at 16-row cuts, chunks of one column, a band table that decodes to every lower tile
once), and requires every plan to equal tests/golden/kt_plans.txt row for row. That file was recorded once from the
statements csrc/gemm.hip held before they moved. Built with -fsanitize=address,undefined. No GPU, no HIP, nothing
loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ktplan_check_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "ktplan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bigkrls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "ktplan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "kt_plans.txt")], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "ktplan_check: ok" in run.stdout
