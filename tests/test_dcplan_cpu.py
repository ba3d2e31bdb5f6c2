"""The host arithmetic of the divide & conquer of the dense eigensolver (bigkrls_amd/csrc/dcplan.h: the tree, the deflation
scan of one merge, which levels stay factored, where the secular vectors go, the root's ordering and truncation) is
plain C++: a stand-alone host program (tests/dcplan_check.cpp, with its own main) checks the tree for every n from 1 to
6000, host_merge on designed pairs of children against what the algorithm guarantees (counts, permutations, ascending
poles, orthogonal rotations, trace and norm, no kept pole below the threshold) -- the "squares that underflow" form of
the deflation test included, which no GPU run has reached --, the root's selection against a brute-force stable sort
(the full-sort fallback included), and the lazy predicate and stash offsets against a literal transcription of the
expressions the one long function held. Built with -fsanitize=address,undefined. No GPU, no HIP, nothing loaded into
Python. The input digests of the GPU cases (tests/_divide_conquer_cases.py) are held to the golden file here as well."""
import json
import os
import shutil
import subprocess

import pytest

import _divide_conquer_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dcplan_check_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "dcplan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bigkrls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "dcplan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("dcplan_check: ok")


def test_small_inputs_of_the_gpu_cases_are_the_recorded_ones():
    """The prescribed spectra go through one Householder similarity written elementwise (no BLAS, no LAPACK): the same
    bits as when the golden file was recorded. (The n x n inputs up to n = 777; the GPU test compares all of them.)"""
    with open(os.path.join(ROOT, "tests", "golden", "divide_conquer_digests.json")) as f:
        golden = json.load(f)["cases"]
    assert sorted(golden) == sorted(cases.case_names())
    for name, case in cases.CASES.items():
        if case["kind"] != "kernel" and case["n"] <= 777:
            assert cases.input_digest(name) == golden[name]["input"], name
