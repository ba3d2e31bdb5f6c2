"""The block Lanczos eigensolver (eigen_krylov of csrc/eigen.hip: stored, implicit and row-sharded products, fixed and
auto rank) returns, bit for bit, what it returned before its one long function was split into the phases of one struct:
tests/golden/block_lanczos_digests.json holds SHA-256 digests of the outputs of the seeded runs of
tests/_block_lanczos_cases.py, recorded by tools/block_lanczos_digests.py from a build of the commit before that change
(twice, with equal results). No kernel, product, collective or summation order changed, so every bit must stand.

The golden file also keeps which BIGKRLS_VERBOSE lines each recorded run showed. Its first test asserts that every case
is there and showed the path it is there for, so a re-recording at another shape cannot silently lose a path."""
import json
import os

import pytest

import _block_lanczos_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_lanczos_digests.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_golden_file_covers_every_case_and_its_path(golden):
    assert sorted(golden) == sorted(cases.case_names())
    for name, required in cases.REQUIRED.items():
        seen = golden[name]["markers"]
        for m in required:
            assert (m[1:] not in seen) if m.startswith("!") else (m in seen), (name, m, seen)
    for name, text in cases.ERROR_TEXT.items():
        assert text in golden[name]["info"]["error"], name
    # the eigtrunc count keeps fewer vectors than values; the auto rank returns one value more than it keeps vectors
    assert golden["stored_trunc"]["info"]["lastkeeper"] < golden["stored_trunc"]["info"]["rank"] == 300
    assert golden["auto_rank"]["info"]["rank"] == golden["auto_rank"]["info"]["lastkeeper"] + 1


@pytest.mark.parametrize("name", cases.case_names())
def test_outputs_match_the_recorded_digests(ctx, golden, name):
    got = cases.run_case(ctx, name)
    print(f"{name}: {got}")
    assert got["digests"] == golden[name]["digests"]
