"""The packed layout of the post-estimation entries (bigkrls_amd/csrc/layout.h) is pure pointer arithmetic: a stand-alone
host program (tests/layout_check.cpp, with its own main) checks the offsets of the marginal_effects and the
interaction_effects layouts against hand-written tables, that host and device offsets agree for every staged region, the
rounding of record regions, zero-length and aliased regions and the read-back range, built with
-fsanitize=address,undefined. No GPU, no HIP, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_check_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bigkrls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "layout_check: ok" in run.stdout
