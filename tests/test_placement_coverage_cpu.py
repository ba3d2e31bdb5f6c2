"""Every device entry of include/bigkrls.h that takes a leading dimension is called by some test with that leading
dimension larger than the row count (operands placed inside larger parents, tests/_placement.py or the test's own
parent). COVERED maps every `bigkrls_dev_*` declaration with an `int64_t ld...` parameter to the test file that makes such
a call; NOT_YET holds, with a reason, the entries no test calls that way yet. A new entry in the header fails this test until
it is put into one of the two."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COVERED = {
    "bigkrls_dev_kernel_block": "test_gpu_kernel_tile_placement.py",
    "bigkrls_dev_kernel_contract": "test_gpu_kernel_tile_placement.py",
    "bigkrls_dev_kernel_contract_grouped": "test_gpu_kernel_tile_placement.py",
    "bigkrls_dev_kernel_loo_colsums": "test_gpu_kernel_tile_placement.py",
    "bigkrls_dev_kernel_loo_binsums": "test_gpu_kernel_tile_placement.py",
    "bigkrls_dev_kernel_loo_moments": "test_gpu_kernel_tile_placement.py",
    "bigkrls_dev_quadform_diag": "_gemm_family_cases.py",              # (run by test_gpu_gemm_family_digests.py)
    "bigkrls_dev_rowsumsq_weighted": "test_gpu_vcov_factors.py",
    "bigkrls_dev_gemm": "test_gpu_gemm_core.py",
    "bigkrls_dev_gemm_modulated": "test_gpu_gemm_modulated.py",
    "bigkrls_dev_gemm_modulated2": "test_gpu_gemm_modulated2.py",
    "bigkrls_dev_gram_weighted": "test_gpu_gram_weighted.py",
    "bigkrls_dev_cluster_scores": "test_gpu_cluster_scores.py",
    "bigkrls_dev_deletion_residuals": "test_gpu_deletion_placement.py",
    "bigkrls_dev_multdiag": "test_gpu_level2_helpers.py",
    "bigkrls_dev_eigen": "test_gpu_eigen_placement.py",
    "bigkrls_dev_eigen_part": "test_gpu_eigen_placement.py",
    "bigkrls_dev_eigen_implicit": "test_gpu_eigen_placement.py",
    "bigkrls_dev_eigen_auto": "test_gpu_eigen_placement.py",
    "bigkrls_dev_syr2k": "test_gpu_syr2k.py",
    "bigkrls_dev_gemm_skinny48": "test_gpu_gemm_skinny48.py",
    "bigkrls_dev_copy_matrix": "test_gpu_level2_helpers.py",
    "bigkrls_dev_qty": "test_gpu_level2_helpers.py",
    "bigkrls_dev_solveforc": "test_gpu_lambda_search.py",
    "bigkrls_dev_lambda_search": "test_gpu_lambda_search.py",
    "bigkrls_dev_deriv_rows": "test_gpu_deriv_pass.py",
    "bigkrls_dev_deriv_var": "test_gpu_deriv_pass.py",
    "bigkrls_dev_gemv": "test_gpu_level2_helpers.py",
    "bigkrls_dev_diag": "test_gpu_level2_helpers.py",
    "bigkrls_dev_neffective": "test_gpu_neffective_exact.py",
    "bigkrls_dev_panel_factor": "test_gpu_panel_routes.py",
}

NOT_YET = {
}

MUST_BE_COVERED = [name for name in COVERED if name.startswith("bigkrls_dev_kernel_")] + ["bigkrls_dev_deletion_residuals"]


def entries_with_a_leading_dimension():
    """{name: [ld parameters]} of the bigkrls_dev_* declarations of the public header"""
    with open(os.path.join(ROOT, "include", "bigkrls.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for m in re.finditer(r"\b(bigkrls_dev_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        lds = re.findall(r"\bint64_t\s+(ld\w*)", m.group(2))
        if lds:
            out[m.group(1)] = lds
    return out


def test_the_parser_sees_the_header():
    found = entries_with_a_leading_dimension()
    assert found["bigkrls_dev_kernel_contract"] == ["lda", "ldb", "ldw", "ldo"]
    assert found["bigkrls_dev_deletion_residuals"] == ["ldq", "lds"]
    assert found["bigkrls_dev_gemm"] == ["lda", "ldb", "ldc"]
    assert "bigkrls_dev_alloc" not in found and len(found) >= 30


def test_every_entry_with_a_leading_dimension_is_in_the_table():
    found = set(entries_with_a_leading_dimension())
    assert not (set(COVERED) & set(NOT_YET)), "an entry is in both tables"
    missing = sorted(found - set(COVERED) - set(NOT_YET))
    assert not missing, f"no test is named for {missing}: place its operands in a test and add it to COVERED (or to NOT_YET, with a reason)"
    stale = sorted((set(COVERED) | set(NOT_YET)) - found)
    assert not stale, f"{stale} are not declarations with a leading dimension in include/bigkrls.h any more"
    assert all(reason.strip() for reason in NOT_YET.values())
    assert len(MUST_BE_COVERED) == 7 and not (set(MUST_BE_COVERED) & set(NOT_YET))


def test_the_named_files_call_their_entries():
    for name, file in sorted(COVERED.items()):
        path = os.path.join(ROOT, "tests", file)
        assert os.path.exists(path), (name, file)
        with open(path) as f:
            assert re.search(rf"\b{name}\b", f.read()), f"tests/{file} does not mention {name}"
