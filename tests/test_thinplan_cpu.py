"""thin_plan (bigkrls_amd/csrc/splitplan.h), the plan of gemm_thin, is pure arithmetic: a stand-alone host program
(tests/thinplan_check.cpp, with its own main) evaluates it over M in 64 ... 512, N in 1 ... 300 and K up to 24 000 and
requires the slabs (splits, k_chunk) to be split_plan()'s on the 128-wide tiling whatever width executes, the width to be
32, 64 or 128, a function of the shape alone and never wider than gemm()'s own tile, and the rule's own conditions for a
narrower tile. Built with -fsanitize=address,undefined. No GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_thinplan_check_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "thinplan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bigkrls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "thinplan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "thinplan_check: ok" in run.stdout
