"""The host plan of the binned leave-out sums (plan_loo_binsums, bigkrls_amd/csrc/ktplan.h: every selected column's
stable bin order as an index list, the bins' counts, the launches, their segments and the slots of the cut bins) is
plain C++: a stand-alone host program (tests/binplan_check.cpp, with its own main) enumerates it over grids of sizes,
columns, bin counts, label patterns and slot counts and checks what kernel_loo_binsums_kernel relies on against brute
force. Built with -fsanitize=address,undefined. No GPU, no HIP, nothing loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binplan_check_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "binplan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bigkrls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "binplan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "binplan_check: ok" in run.stdout
    # the long-bin shape of tests/test_gpu_accumulated_effects.py: at least one bin is cut into several segments. The
    # program plans it with 2048 and 3072 wave slots, not with the count a device reports, and that does not matter:
    # the shape has 10 tasks per split (one stationary tile x 10 bins of about 2050 rows = 129 loop tiles, at most 8
    # parts each), so with any slot count of 80 or more every candidate split fits one round of waves and
    # plan_grouped_segments takes the largest, 8 parts per bin.
    m = re.search(r"u=4099 v=17 cols=5 bins=2: (\d+) bins cut into several segments", run.stdout)
    assert m and int(m.group(1)) >= 1
