"""The gate of stage 1's CholeskyQR2 panel factorisation (pq_chol, csrc/eigen_2stage.inc), restated in float64 numpy
(tests/_panel_cases.gate_restated: the two passes, the pivot test, the diagonal ratio of the first factor, the second Gram
matrix), on the panels tests/test_gpu_panel_routes.py sweeps on the device. It fixes what that sweep may demand: which
panels CholeskyQR2 must keep and which it must leave to the Householder kernel.

Kahan panels P = Q0 diag(s^j)(I - c triu(1, 1)): the diagonal of R falls to 0.004 only while cond(R) rises from 1e6 to
1.5e12. From c = 0.29 the first Gram matrix is numerically singular (cond^2 eps > 1) and what its factorisation does is
decided by the rounding of its last pivots: a pivot that is not positive (most panels), or a factor that goes through with
a diagonal ratio of 0.006 ... 0.07 -- nowhere near PQC_RATIO -- and a second factor with its diagonal in [0.65, 1.41].
With the pivot, ratio and diagonal tests alone the gate kept such panels, and Q after the second pass was orthonormal
only to cond(Q1)^2 eps (in this restatement 3e-14 ... 4e-13 at c = 0.35 and 1e-10 ... 8e-10 at c = 0.40; on the device up
to 1e-9). The bound on the second Gram matrix, max |Q1'Q1 - I| < 2^-7 (PQC_E2MAX: cond(Q1) < sqrt(3)), closes that: the
restatement keeps every panel up to c = 0.26 (cond 6.5e7) at every size and scale and none from c = 0.28 (cond 2.6e8).
Mixed panels Q0 diag(logspace(0, -e, 64)) Q1: kept up to e = 6, left by the ratio for e = 6.5, 7, 8, by a pivot for e = 9, 10."""
import numpy as np
import pytest

import _panel_cases as pc

SCALES = (1.0, 1e-20, 1e20)


@pytest.mark.parametrize("m", [300, 4097])
def test_restated_gate_on_kahan_panels(m):
    for scale in SCALES:
        for c in pc.KAHAN_C:
            why = pc.gate_restated(pc.kahan_panel(m, c) * scale)
            if c <= 0.26:
                assert why is None, (c, scale, why)
            elif c >= 0.28:     # never the ratio: the diagonal of a Kahan factor does not show its condition number
                assert why in ("breakdown", "far"), (c, scale, why)
            else:
                assert why in (None, "far"), (c, scale, why)


def test_without_the_bound_on_the_second_gram_matrix_singular_kahan_panels_pass(monkeypatch):
    """c >= 0.30, both sizes, three scales: 30 panels. The pivot, ratio and diagonal tests alone keep some of them (a first
    factor that happens to go through), never by the ratio; with the bound none is kept."""
    panels = [pc.kahan_panel(m, c) * scale for m in (300, 4097) for scale in SCALES for c in pc.KAHAN_C if c >= 0.30]
    assert len(panels) == 30 and not [P0 for P0 in panels if pc.gate_restated(P0) is None]
    monkeypatch.setattr(pc, "PQC_E2MAX", np.inf)
    whys = [pc.gate_restated(P0) for P0 in panels]
    assert whys.count(None) >= 5 and whys.count("breakdown") >= 5 and "ratio" not in whys


@pytest.mark.parametrize("m", [300, 4097])
def test_restated_gate_on_mixed_panels(m):
    for scale in SCALES:
        for e in pc.MIXED_E + [9]:
            why = pc.gate_restated(pc.mixed_panel(m, e) * scale)
            assert why == (None if e <= 6 else "ratio" if e <= 8 else "breakdown"), (e, scale, why)


def test_kahan_factor_hides_its_condition_number():
    for c, lo, hi in ((0.20, 1e6, 1.1e6), (0.24, 1.6e7, 1.7e7), (0.40, 1.5e12, 1.6e12)):
        R = pc.kahan_r(c)
        assert lo <= np.linalg.cond(R) <= hi and np.abs(np.diag(R)).min() >= 0.004
    assert np.abs(np.diag(pc.kahan_r(0.32))).min() >= 0.03


def test_lapack_reference_meets_the_checks_it_sets_the_bars_with():
    """numpy.linalg.qr(mode='raw') + dlarft, through the same error functions and the same structure check"""
    for m in (2, 3, 12, 63, 64, 65, 127, 300):
        P0 = pc.normal_panel(m)
        ref = pc.lapack_factor(P0)
        pc.check_structure(ref, m, scaled_in_place=True)
        orth, fact, fold = pc.errors(P0, ref)
        assert orth <= 1e-14 and fact <= 1e-14 and fold == 0.0


def test_structure_check_sees_a_wrong_scale():
    m = 100
    ref = pc.lapack_factor(pc.normal_panel(m))
    low = np.tril(np.ones((m, pc.B), dtype=bool), -1)
    unscaled = dict(ref, P=np.where(low, ref["P"] / 3.0, ref["P"]))
    unscaled["V"] = np.where(low, unscaled["P"] * 3.0, ref["V"])
    pc.check_structure(unscaled, m, scaled_in_place=False)
    with pytest.raises(AssertionError):
        pc.check_structure(unscaled, m, scaled_in_place=True)
    broken = dict(unscaled, V=unscaled["V"].copy())
    broken["V"][70, 5] = np.nextafter(broken["V"][70, 5], 2.0)
    with pytest.raises(AssertionError):
        pc.check_structure(broken, m, scaled_in_place=False)
