"""The divide & conquer on the tridiagonal matrix (DivideConquer of csrc/eigen.hip, csrc/dcplan.h) returns, bit for bit,
what it returned before its one long function was split into the phases of one struct, and takes the same path:
tests/golden/divide_conquer_digests.json holds, for the seeded runs of tests/_divide_conquer_cases.py, SHA-256 digests of
all returned eigenvalues, the kept eigenvectors and lastkeeper, and the figures of every "d&c depth" line the library
prints under BIGKRLS_VERBOSE (depth, factored or not, merges, largest, non-deflated, rotations; whether the "redoing the
top levels explicitly" and "factored levels applied to" lines appeared), recorded by tools/divide_conquer_digests.py from
a build of the commit before that change (twice, with equal results). No kernel, launch, operand, upload, read-back or
their order changed, so every bit and every figure must stand.

The golden file also keeps a digest of each case's input, compared first: a difference there is a different numpy, not a
different solver."""
import json
import os

import pytest

import _divide_conquer_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "divide_conquer_digests.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_golden_file_covers_every_case_and_its_path(golden):
    assert sorted(golden) == sorted(cases.case_names())
    for name, rec in golden.items():
        levels = rec["path"]["levels"]
        assert levels, name
        if "clusters" in name or "wilkinson" in name:
            assert any(lv[5] > 0 for lv in levels), name                    # rotations on some level
        if "identity" in name:
            assert all(lv[4] == 0 for lv in levels), name                   # everything deflates
        if name.startswith("factored_"):
            assert sorted(lv[0] for lv in levels if lv[1]) == [0, 1, 2, 3], name
            assert all(lv[1] == (lv[0] <= 3) for lv in levels), name
            assert rec["path"]["applied"], name
        if name.startswith("explicit_") or name.startswith("n"):
            assert not any(lv[1] for lv in levels) and not rec["path"]["applied"], name
        assert rec["path"]["redo"] == (name in cases.REDO_CASES), name
    for name in cases.REDO_CASES:
        # the first pass stops at the root, the second forms every level: no level of it is factored
        levels = golden[name]["path"]["levels"]
        first_root = [i for i, lv in enumerate(levels) if lv[0] == 0]
        assert len(first_root) == 1 and not golden[name]["path"]["applied"], name
        assert any(lv[1] for lv in levels) and not levels[-1][1], name
    # the two kernel cases go factored by the default switches, each through its own condition
    assert cases.CASES["kernel_4300_neig200"]["neig"] * 8 <= 4300 and cases.CASES["kernel_4300_neig200"]["trunc"] < 0
    assert cases.CASES["kernel_4300_trunc"]["neig"] is None and cases.CASES["kernel_4300_trunc"]["trunc"] > 0
    for name in ("kernel_4300_neig200", "kernel_4300_trunc"):
        assert golden[name]["path"]["applied"] and not cases.CASES[name]["env"], name
    assert golden["redo_natural"]["info"]["lastkeeper"] * 8 > cases.CASES["redo_natural"]["n"] > 4096
    assert not cases.CASES["redo_natural"]["env"]


@pytest.mark.parametrize("name", cases.case_names())
def test_outputs_and_path_match_the_recording(ctx, golden, name):
    A = cases.make_input(name)
    assert cases._sha(A) == golden[name]["input"], \
        f"the INPUT of {name} is not the recorded one (another numpy?): nothing is known about the solver"
    got = cases.run_case(ctx, name, A)
    print(f"{name}: {got}")
    assert got["path"] == golden[name]["path"]
    assert got["info"] == golden[name]["info"]
    assert got["digests"] == golden[name]["digests"]
