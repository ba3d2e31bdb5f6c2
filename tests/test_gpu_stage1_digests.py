"""Stage 1 of the dense eigensolver (full matrix to band: Stage1 of csrc/eigen_2stage.inc; the row-block distributed form,
dist_s1_* of csrc/eigen.hip) returns, bit for bit, what it returned before its one long function was split into the
phases of one struct: tests/golden/stage1_digests.json holds SHA-256 digests of the outputs of the seeded runs of
tests/_stage1_cases.py -- all n eigenvalues, the kept eigenvectors and lastkeeper; coeffs, lambda and lastkeeper of the
distributed fit -- recorded by tools/stage1_digests.py from a build of the commit before that change (twice, with equal
results). No kernel, launch, operand, stream, event or summation order changed, so every bit must stand.

Each run must also print, under BIGKRLS_VERBOSE, the "stage 1 schedule" line with the counts csrc/s1sched.h gives for
the case (COUNTS of the cases file, which tests/test_s1sched_cpu.py holds the header to): groups of four, pair groups,
two-stream panels, one-stream panels."""
import json
import os

import pytest

import _stage1_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage1_digests.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_golden_file_covers_every_case_and_its_path(golden):
    assert sorted(golden) == sorted(cases.case_names())
    # the P = 2 kernel is numerically singular: pq_chol leaves panels to the Householder kernel; no other case does
    for name, rec in golden.items():
        if "fallback_panels" in rec["info"]:
            assert (rec["info"]["fallback_panels"] > 0) == name.startswith("n2100_p2"), name
    assert all("fallback_panels" in golden[n]["info"] for n in ("n2100_p2", "n2100_p2_tpq0"))
    # every case that runs the loop reaches the arms it is named for (and n is never a multiple of 64)
    for name, (n, _p, _seed, _switches) in cases.CASES.items():
        assert n % 64 != 0, name
    quads, pairs, two, one = cases.COUNTS["n13150"]
    assert quads == 1 and pairs == 16 and two > 0 and one > 0
    assert cases.COUNTS["n11300_low_thresholds"][0] > 1
    assert cases.COUNTS["n11300"][0] == 0 and cases.COUNTS["n11300"][1] > 0 and cases.COUNTS["n11300_agg0"][:2] == (0, 0)


@pytest.mark.parametrize("name", cases.case_names())
def test_outputs_match_the_recorded_digests(ctx, golden, name):
    got = cases.run_case(ctx, name)
    print(f"{name}: {got}")
    assert got["digests"] == golden[name]["digests"]
    assert got["counts"] == (None if cases.COUNTS[name] is None else list(cases.COUNTS[name]))
