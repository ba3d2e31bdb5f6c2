"""The post-estimation entries (marginal_effects, interaction_effects, their pointwise standard errors, group_effects,
partial_dependence, conditional_effects) give, bit for bit, what they gave before their host bodies were rebuilt on one
shared frame (csrc/layout.h, hostprep.h, margeff.h, curvetail.h), leave the same workspace behind and raise the same
messages: tests/golden/effects_digests.json holds SHA-256 digests of every returned array, workspace_bytes() after every call and
the message of every error case on the seeded inputs of tests/_effects_cases.py, recorded by tools/effects_digests.py
from a build of the commit before that change."""
import json
import os

import pytest

import _effects_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "effects_digests.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.fixture(scope="module")
def own_ctx():
    """One context owned by the module (the cases release its workspace; the session's is left alone)."""
    import bigkrls_amd as bk
    own = bk.Context(0)
    yield own
    own.close()


def test_golden_file_covers_every_case(golden):
    assert sorted(golden) == sorted(cases.case_names())


@pytest.mark.parametrize("name", cases.case_names())
def test_outputs_match_the_recorded_digests(own_ctx, golden, name):
    got = cases.run_case(own_ctx, name)
    for sub, d in got.items():
        print(f"{name} {sub}: {d}")
    assert got == golden[name]


def test_every_error_case_raises(golden):
    for name, rec in golden.items():
        if name.startswith("err_"):
            assert isinstance(rec["message"], str) and rec["message"], name
