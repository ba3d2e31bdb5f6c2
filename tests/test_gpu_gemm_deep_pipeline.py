"""The two-tiles-in-flight k loop of gemm_tile (csrc/gemm.hip: every tile up to GEMM_DEEP_BN wide) over one to eight
k-tiles, with and without a partial last tile, through bigkrls_dev_gemm (all four transposes, two betas, row and column
tiles full and ragged, one split-K case each) and through its other users (gemm_modulated, gemm_modulated2,
gram_weighted): cases, inputs, reference and bound are tests/_gemm_deep_pipeline_cases.py, which also says which groups
run the interior loop (gemm at full tiles of its not-contiguous operands, gemm_modulated at n = 32 and 64) and which
only the general loop around it (gemm_modulated at n = 50, gemm_modulated2, gram_weighted).

Two assertions per group:
  (i)  every output, its sentinel surroundings included, is bit for bit what a build of the commit before the interior
       loop gave (tests/golden/gemm_deep_pipeline_digests.json, recorded by tools/gemm_deep_pipeline_digests.py);
  (ii) every entry is within (k + 4) 2^-53 (|alpha| |op(A)| |op(B)| + |beta| |C0|) of a numpy float64 reference that
       no recording enters."""
import json
import os

import pytest

import _gemm_deep_pipeline_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_deep_pipeline_digests.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


def test_golden_file_covers_every_group(golden):
    assert sorted(golden) == sorted(cases.group_names())


@pytest.mark.parametrize("name", cases.group_names())
def test_k_tile_sweep(ctx, golden, name):
    digest, figures = cases.run_group(ctx, name)
    worst = max(figures, key=lambda f: f[1])
    print(f"{name}: {len(figures)} sub-cases, largest |C - C_ref| / bound = {worst[1]:.3g} at {worst[0]}; digest {digest}")
    bad = [(sub, r) for sub, r, finite in figures if not (finite and r <= 1.0)]
    assert not bad, f"{name}: outside the bound (sub-case, error / bound): {bad[:8]}"
    assert digest == golden[name], f"{name}: not the bits of the recorded build"
