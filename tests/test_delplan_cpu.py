"""The host plan of the deletion residuals (plan_deletion, bigkrls_amd/csrc/delplan.h: the stable order of the units'
rows, every unit's size and size class, the per-class lists the kernels walk, the workspace counts) is plain C++: a
stand-alone host program (tests/delplan_check.cpp, with its own main) plans sizes 1 .. 2 MB + 1, empty units, all rows in
one unit, G = n, grouped and shuffled labels, units over the general route's cap and labels out of range, and checks
every plan against brute force. Built with -fsanitize=address,undefined. No GPU, no HIP, nothing loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_delplan_check_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "delplan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bigkrls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "delplan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "delplan_check: ok" in run.stdout
    # the grid really holds what it is there for: empty units, refused labels and units over the cap
    m = re.search(r"plans (\d+), units (\d+) \((\d+) empty\), refused for a label (\d+), over the cap (\d+)", run.stdout)
    assert m and int(m.group(1)) >= 60 and int(m.group(3)) >= 10 and int(m.group(4)) == 4 and int(m.group(5)) == 2
