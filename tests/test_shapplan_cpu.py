"""The host plan of the Shapley weights (bigkrls_amd/csrc/shapplan.h: the Gauss-Legendre rules on [0,1], the player
table and the column order the kernel walks, the kernel shapes, the background chunks in LDS and the row blocks) is plain
C++: a stand-alone host program (tests/shapplan_check.cpp, with its own main) checks every rule G = 1..64 against the
monomial moments 1/(k+1), k = 0..2G-1, to 1e-14 in long double, the nodes' order and symmetry, the table against brute
force and its refusals, and the caps. Built with -fsanitize=address,undefined. No GPU, no HIP, nothing loaded into
Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shapplan_check_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "shapplan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bigkrls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "shapplan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "shapplan_check: ok" in run.stdout
