"""The three statements of "a column with exactly two distinct values" (R/bigKRLS.R:242, src/bigderiv_v3.cpp:28-31) that
decide which finalise formula a column of the marginal-effects pass takes -- ops.binary_columns, two_valued() of
csrc/hostprep.h (the fit and marginal_effects) and the oracle's is_binary_column -- on the same columns, and
ops.deriv_scales against its two closed forms (src/bigderiv_v3.cpp:85, :105). No GPU: two_valued() is compiled into a
small host program of its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from bigkrls_amd import ops
from oracle import krls_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COLUMNS = {
    "constant": [2.5] * 6,
    "two_values": [1.0, 3.0, 3.0, 1.0, 1.0, 3.0],
    "two_values_one_lonely_high": [0.0, 0.0, 0.0, 7.0, 0.0, 0.0],
    "two_values_one_lonely_low": [4.0, 4.0, -4.0, 4.0, 4.0, 4.0],
    "three_values": [0.0, 1.0, 2.0, 1.0, 0.0, 1.0],
    "three_values_extremes_first": [0.0, 2.0, 0.0, 2.0, 1.0, 2.0],
    "single_row": [1.0],
    "signed_zeros_and_one": [-0.0, 0.0, 1.0, 0.0, -0.0, 1.0],
    "signed_zeros_only": [-0.0, 0.0, 0.0, -0.0],
    "negative_coding": [-1.5, 2.25, -1.5, -1.5, 2.25],
    "both_negative": [-3.0, -1.0, -1.0, -3.0],
    "continuous": [0.1, -0.7, 1.3, 0.1, 2.9, -0.2],
}
EXPECTED = {"constant": False, "two_values": True, "two_values_one_lonely_high": True, "two_values_one_lonely_low": True,
            "three_values": False, "three_values_extremes_first": False, "single_row": False, "signed_zeros_and_one": True,
            "signed_zeros_only": False, "negative_coding": True, "both_negative": True, "continuous": False}


def col(name):
    return np.array(COLUMNS[name], dtype=np.float64)


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_binary_columns_matches_the_oracle(name):
    x = col(name)
    assert bool(ops.binary_columns(x[:, None])[0]) == bool(orc.is_binary_column(x)) == EXPECTED[name]


def test_binary_columns_of_a_matrix():
    names = [k for k in sorted(COLUMNS) if len(COLUMNS[k]) == 6]
    X = np.column_stack([col(k) for k in names])
    assert ops.binary_columns(X).tolist() == [EXPECTED[k] for k in names]
    assert ops.binary_columns(np.zeros((0, 3))).tolist() == [False] * 3


def test_deriv_scales_closed_forms():
    names = [k for k in sorted(COLUMNS) if len(COLUMNS[k]) == 6]
    X = np.column_stack([col(k) for k in names])
    n, sigma = 6, 3.5
    isb = ops.binary_columns(X)
    got = ops.deriv_scales(X, isb, sigma)
    for j, k in enumerate(names):
        if EXPECTED[k]:
            sd = 1.0 / (X[:, j].max() - X[:, j].min())
            assert got[j] == 2.0 * sd * sd / 36.0, k                       # src/bigderiv_v3.cpp:85
        else:
            assert got[j] == 4.0 / (sigma * sigma * 36.0), k               # :105
    # the flags are the caller's: a binary column flagged continuous takes the continuous scale
    assert (ops.deriv_scales(X, np.zeros(len(names), dtype=bool), sigma) == 4.0 / (sigma * sigma * n * n)).all()


def _compile_two_valued(tmp_path):
    """A host program around two_valued() of csrc/hostprep.h. The header includes the HIP runtime's declarations
    (common.h), so a plain C++ compiler needs the ROCm include directory; without it, hipcc compiles the same
    host-only source."""
    body = []
    for name in sorted(COLUMNS):
        vals = ", ".join(float(v).hex() for v in COLUMNS[name])
        body.append(f'  {{ const double x[] = {{{vals}}}; double lo, hi; const bool b = bk::two_valued(x, {len(COLUMNS[name])}, &lo, &hi);\n'
                    f'    std::printf("{name} %d %a %a\\n", b ? 1 : 0, lo, hi); }}\n')
    src = tmp_path / "two_valued_main.cpp"
    src.write_text('#include <cstdio>\n#include "hostprep.h"\n'
                   'namespace bk { void set_error(const std::string&) {} }\n'
                   'int main() {\n' + "".join(body) + '  return 0;\n}\n')
    exe = tmp_path / "two_valued_main"
    csrc = os.path.join(ROOT, "bigkrls_amd", "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc = os.environ.get("HIPCC", os.path.join(rocm, "bin", "hipcc"))
    tried = []
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx and os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        tried.append([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", csrc,
                      str(src), "-o", str(exe), "-pthread"])
    if os.path.exists(hipcc):
        tried.append([hipcc, "-std=c++17", "-O1", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", csrc, str(src), "-o", str(exe),
                      "-pthread"])
    if not tried:
        pytest.skip("no C++ compiler with the HIP headers found")
    log = ""
    for cmd in tried:
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        log += " ".join(cmd) + "\n" + r.stderr[-2000:] + "\n"
    raise AssertionError("the host program around two_valued() does not compile:\n" + log)


def test_two_valued_of_hostprep_agrees(tmp_path):
    exe = _compile_two_valued(tmp_path)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = {}
    for line in out:
        if line.strip():
            name, b, lo, hi = line.split()
            seen[name] = (bool(int(b)), float.fromhex(lo), float.fromhex(hi))
    assert sorted(seen) == sorted(COLUMNS)
    for name, (b, lo, hi) in seen.items():
        x = col(name)
        assert b == EXPECTED[name] == bool(ops.binary_columns(x[:, None])[0]) == bool(orc.is_binary_column(x)), name
        assert lo == x.min() and hi == x.max(), name      # (== : the sign of a zero is not part of the contract)
