"""The tile map of the mirrored rank-k update (bigkrls_amd/csrc/syrkmap.h: SyrkMap, its builder, the decode that
syrk_mirror_kernel runs, xcd_remap) is pure index arithmetic: a stand-alone host program (tests/syrkmap_check.cpp, with
its own main) decodes every block id of a launch for both tile widths and requires exactly the tiles of the requested
columns of the lower tile triangle, each once, and the builder's count: 1 to 13 row tiles with every column range; 40,
157, 318, 319, 330 and 700 row tiles, where the band table fills up and the rows per band are raised; every k that changes
the rows per band; the rows-per-band override; the column order with its offset; empty ranges. The walk of the whole lower
tile triangle (lower_tile_of: gram_weighted_kernel, gram_reduce_kernel, syrk_lower_kernel), a closed form with fix-ups, is
compared with the plain loop for every tile of every grid of 1 to 1024 tile rows. Built with
-fsanitize=address,undefined, so a band table that outgrows its array is seen. No GPU, no HIP, nothing loaded into
Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_syrkmap_check_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "syrkmap_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "bigkrls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "syrkmap_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "syrkmap_check: ok" in run.stdout
