"""The back half of the dense eigensolver -- band to tridiagonal, the stage-2 back-transform and the stage-1
back-transform (csrc/eigen_2stage.inc; their host arithmetic in csrc/s2plan.h) -- returns, bit for bit, what it returned
before that host arithmetic moved into one plan: tests/golden/back_half_digests.json holds, for the seeded runs of
tests/_back_half_cases.py, SHA-256 digests of all returned eigenvalues, the kept eigenvectors and lastkeeper, recorded by
tools/back_half_digests.py from a build of the commit before that change (twice, with equal results). No kernel, launch,
operand, stream, event or allocation size changed, so every bit must stand, on every arm of every switch.

The golden file also keeps a digest of each case's input, compared first: a difference there is a different numpy, not a
different solver."""
import json
import os

import pytest

import _back_half_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "back_half_digests.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_golden_file_covers_every_case_and_its_shape(golden):
    assert sorted(golden) == sorted(cases.case_names())
    c = cases.CASES
    # the smallest two-stage size; sizes that are no multiple of the panel width; the size rule of the chain kernel
    assert c["n259"]["n"] == 4 * 64 + 3 and c["n8100_trunc"]["n"] > 8000 and not c["n8100_trunc"]["env"]
    assert all(case["n"] % 64 != 0 for case in c.values())
    # all vectors kept: 18 slabs, the last one 12 columns wide; the truncated run: one slab
    assert golden["n1100"]["info"]["lastkeeper"] == 1100 and 1100 % 64 == 12
    assert 0 < golden["n1100_trunc"]["info"]["lastkeeper"] <= 64
    assert 0 < golden["n8100_trunc"]["info"]["lastkeeper"] < 8100
    # the column split returns the whole count, whichever part is computed
    assert all(golden[f"n1100_part{r}of2"]["info"]["lastkeeper"] == 1100 for r in (0, 1))
    # every arm of the three variant switches is there, on the all-vectors shape
    arms = [tuple(sorted(case["env"].items())) for case in c.values() if case["n"] == 1100 and case["trunc"] == cases.ALL]
    for bc in ((), (("BIGKRLS_BC", "lds"),), (("BIGKRLS_BC", "lds"), ("BIGKRLS_BC_T", "256")),
               (("BIGKRLS_BC", "persistent"),), (("BIGKRLS_BC", "wavefront"),)):
        assert bc in arms, bc
    for bt2 in ((("BIGKRLS_BT2", "chain"),), (("BIGKRLS_BT2", "chain"), ("BIGKRLS_BT2_SEG", "3")),
                (("BIGKRLS_BT2", "wavefront"),), (("BIGKRLS_BT2", "seq"),), (("BIGKRLS_BT1", "panel"),)):
        assert bt2 in arms, bt2
    assert sorted(case["own_process"]["BIGKRLS_BT1_GRP"] for case in c.values() if case["own_process"]) == ["2", "4"]
    # the arms that may not differ in a single bit (test_gpu_level1.py asserts the same on its own shapes)
    for name in ("n1100_bt2_chain", "n1100_bt2_chain_seg3", "n1100_bt2_wavefront"):
        assert golden[name]["digests"] == golden["n1100"]["digests"], name
    assert golden["n1100_bc_persistent"]["digests"] == golden["n1100_bc_wavefront"]["digests"]


@pytest.mark.parametrize("name", cases.case_names())
def test_outputs_match_the_recorded_digests(ctx, golden, name):
    Xs = cases.make_input(name)
    assert cases._sha(Xs) == golden[name]["input"], \
        f"the INPUT of {name} is not the recorded one (another numpy?): nothing is known about the solver"
    got = cases.run_case(ctx, name, Xs)
    print(f"{name}: {got}")
    assert got["input"] == golden[name]["input"]
    assert got["info"] == golden[name]["info"]
    assert got["digests"] == golden[name]["digests"]
