"""The split-K plan of the plain GEMM family (bigkrls_amd/csrc/splitplan.h: one search, three models -- plain GEMM,
quadform, skinny48) is pure arithmetic: a stand-alone host program (tests/splitplan_check.cpp, with its own main)
evaluates the three models over a grid of tile counts, contraction lengths and result sizes, with the development
override off and on, and requires (splits, k_chunk) to equal tests/golden/split_plans.txt row for row. That file was
recorded once from the three separate searches csrc/gemm.hip had before, so the constants in which they differed (step
cost, slab cost and its second rule, the gate, the override, the clamp) are pinned. Built with
-fsanitize=address,undefined. No GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_splitplan_check_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "splitplan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bigkrls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "splitplan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "split_plans.txt")], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "splitplan_check: ok" in run.stdout
