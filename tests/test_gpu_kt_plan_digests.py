"""The kernel builds, the grouped pass and the leave-out moments give, bit for bit, what they gave before their host
plans moved into csrc/ktplan.h: tests/golden/kt_plan_digests.json holds SHA-256 digests of their outputs on the seeded
inputs of tests/_kt_plan_cases.py, recorded by tools/kt_plan_digests.py from a build of the commit before that change.
The cases are the ones tests/_fused_tile_cases.py does not reach: every arm of the kernel build, a grouped table past
the inline limit (the pinned upload behind an event, twice in a row), leave-out moments in three launches."""
import json
import os

import numpy as np
import pytest

import _kt_plan_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kt_plan_digests.json")


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


@pytest.mark.parametrize("name", cases.GROUPED_CASES)
def test_long_grouped_tables_against_the_direct_sum(ctx, name):
    """Two calls in a row are bit-equal (the second waits on the event behind the first one's upload), and both are the
    direct sum in extended precision to 1e-13 of the scale max sum_i |W| e, test_grouped_contract_three_ways' bound."""
    A, B, W, sigma = cases.grouped_inputs()
    lab, G = cases.grouped_labels(name)
    q = cases.GRP_Q
    first, second = cases.grouped_outputs(ctx, name)
    assert first.shape == (cases.GRP_V, G * q) and np.array_equal(first, second)
    Al, Bl, Wl = (x.astype(np.longdouble) for x in (A, B, W))
    K = np.exp(-((Al[:, None, :] - Bl[None, :, :]) ** 2).sum(axis=2) / np.longdouble(sigma))   # u x v
    ref = np.zeros((cases.GRP_V, G * q), dtype=np.longdouble)
    scale = np.zeros_like(ref)
    for g in range(G):
        rows = lab == g
        ref[:, g * q:(g + 1) * q] = K[rows].T @ Wl[rows]
        scale[:, g * q:(g + 1) * q] = K[rows].T @ np.abs(Wl[rows])
        if not rows.any():
            assert np.array_equal(first[:, g * q:(g + 1) * q], np.zeros((cases.GRP_V, q)))
    err = float(np.max(np.abs(first.astype(np.longdouble) - ref)) / float(scale.max()))
    print(f"{name}: error {err:.3e} of the scale")
    assert err < 1e-13
