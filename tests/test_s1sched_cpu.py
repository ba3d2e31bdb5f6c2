"""The schedule of stage 1 of the dense eigensolver (bigkrls_amd/csrc/s1sched.h: which arm of the panel loop takes panel
k, where a pair group's update is cut) is pure arithmetic: a stand-alone host program (tests/s1sched_check.cpp, with its
own main) carries a literal transcription of the predicates the loop held while it was one function -- has_panel,
resident_qr, agg_ok, quad_ok, the pair loop's condition, the swap condition, the J1 / c1 arithmetic, the distributed
group size -- and requires the header to agree for every panel of every n from 257 to 24 000 under every switch setting
that reaches them. It also prints the arm counts of the GPU cases of tests/_stage1_cases.py, which must equal that file's
table (the GPU test holds the library's "stage 1 schedule" line to the same table), and checks that each case reaches
the arms it is there for. Built with -fsanitize=address,undefined. No GPU, no HIP, nothing loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

import _stage1_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_s1sched_check_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "s1sched_check")
    build = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bigkrls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "s1sched_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "s1sched_check: ok" in run.stdout
    printed = {m[0]: tuple(int(v) for v in m[1:]) for m in re.findall(r"^case (\w+): (\d+) (\d+) (\d+) (\d+)$", run.stdout, re.M)}
    expected = {name: counts for name, counts in cases.COUNTS.items() if counts is not None}
    assert printed == expected
    assert sorted(cases.COUNTS) == sorted(cases.CASES)
