"""The plain GEMM family of csrc/gemm.hip (gemm, gemm_modulated, gemm_modulated2, gram_weighted, quadform_diag,
gemm_nn_skinny48, the five symmetric rank-2k forms, gemm_batched_nn) gives, bit for bit, what it gave before its kernels
were rebuilt from one tile frame and its three split-K searches from one plan: tests/golden/gemm_family_digests.json
holds SHA-256 digests of the outputs on the seeded inputs of tests/_gemm_family_cases.py, recorded by
tools/gemm_family_digests.py from a build of the commit before that change. A digest covers the whole parent array of
the output, its sentinel surroundings included; the inputs are standard normal, so another split count or summation
order shows. (The second cost rule of the plain split model, ntile >= 256 and K >= 16384, is covered by
tests/test_splitplan_cpu.py: its smallest case here would need two 268 MB operands.)"""
import json
import os

import pytest

import _gemm_family_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_family_digests.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


def test_golden_file_covers_every_case(golden):
    assert sorted(golden) == sorted(cases.case_names())


@pytest.mark.parametrize("name", cases.case_names())
def test_outputs_match_the_recorded_digests(ctx, golden, name):
    got = cases.run_case(ctx, name)
    for sub, d in got.items():
        print(f"{name} {sub}: {d}")
    assert got == golden[name]
