"""The five fused kernel-tile entry points (bKernelContract narrow and wide, bKernelContractGrouped, bKernelLooColsums,
bKernelLooMoments) give, bit for bit, what they gave before their kernels were rebuilt from one shared frame:
tests/golden/fused_tile_digests.json holds SHA-256 digests of their outputs on the seeded inputs of
tests/_fused_tile_cases.py, recorded by tools/fused_tile_digests.py from a build of the commit before that change.
The outputs depend on the loop splits, and those on the kernels' occupancy, so this also pins the register allocation."""
import json
import os

import pytest

import _fused_tile_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_tile_digests.json")


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


def test_both_split_regimes_are_covered():
    """trans = 1 (70 stationary rows, 69 loop tiles) cuts the loop: its partial sums take a workspace slot; trans = 0
    (5 loop tiles, below the 32 a cut needs) runs as one split and takes none. Same operands, so the rest of the
    workspace is the same. (A context of its own: the workspace of the session's is left alone.)"""
    import bigkrls_amd as bk
    from bigkrls_amd import ops
    own = bk.Context(0)
    try:
        p, q = 20, 20
        dA, dB, dWA, dWB = cases.operands(own, p, q)
        ops.bKernelContract(dA, dB, dWB, float(p), trans=0)
        own.sync()
        one_split = own.workspace_bytes()
        own.release_workspace()
        ops.bKernelContract(dA, dB, dWA, float(p), trans=1)
        own.sync()
        several = own.workspace_bytes()
        print(f"workspace: {one_split} bytes with one split, {several} with several")
        # at least two partial sums of 70 x 20 doubles
        assert several - one_split >= 2 * cases.V * q * 8
    finally:
        own.close()
