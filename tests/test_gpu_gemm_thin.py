"""gemm_thin (csrc/gemm.hip; its plan: thin_plan, csrc/splitplan.h), the entry of the three thin products of a step of the
stage-1 back-transform: gemm()'s kernels over gemm()'s k slabs, with a tile width chosen apart from the column count.
Through the test entry bigkrls_dev_gemm_thin(bigkrls_dev_gemm's arguments, force_bn), which is exported but not declared
in include/bigkrls.h (development only), so its arguments are declared here.

(i)   At every forced width (32, 64, 128) and under the rule (0) the output -- its whole parent, sentinel surroundings
      included -- is bit for bit bigkrls_dev_gemm's on the same operands:
        M in {64, 192, 512}: half a row tile, one and a half, four;
        N in {1, 31, 33, 65, 250}: around the widths 32 and 64, and the back-transform's ragged 250;
        K in {15, 64, 1023, 1024, 2600}: below one k-tile, no split, the last length without a split, the first with
          one, several slabs with a ragged last one;
        forms: T,N with beta = 0; N,N with beta = 0; N,N with alpha = -1, beta = 1 (the three products of a step).
      Every operand is a sub-block of a larger parent (tests/_placement.py), so lda, ldb and ldc exceed the row counts.
(ii)  Independently of (i), every entry of bigkrls_dev_gemm_thin's result under the rule is within
      (k + 4) 2^-53 (|alpha| |op(A)| |op(B)| + |beta| |C0|) of a numpy float64 reference, the bound of
      tests/test_gpu_gemm_deep_pipeline.py.
(iii) ops.bEigen of the n259 and n1100 inputs of tests/_back_half_cases.py under BIGKRLS_BT1_TILE = 32, 64 and 128 gives
      the digests recorded in tests/golden/back_half_digests.json (the file is read, never written)."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

import _back_half_cases as back_half
from _placement import SENT, place, take

pytestmark = pytest.mark.gpu

MS = (64, 192, 512)
NS = (1, 31, 33, 65, 250)
KS = (15, 64, 1023, 1024, 2600)
WIDTHS = (32, 64, 128, 0)          # 0: the rule
FORMS = {"tn_beta0": (1, 0, 1.0, 0.0), "nn_beta0": (0, 0, 1.0, 0.0), "nn_update": (0, 0, -1.0, 1.0)}   # ta, tb, alpha, beta
U = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "back_half_digests.json")


@pytest.fixture(scope="module")
def thin(lib):
    fn = lib.bigkrls_dev_gemm_thin
    i64, f64, vp = C.c_int64, C.c_double, C.c_void_p
    fn.argtypes = [vp, C.c_int, C.c_int, i64, i64, i64, f64, vp, i64, vp, i64, f64, vp, i64, C.c_int]
    fn.restype = C.c_int
    return fn


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_width_gives_gemms_bits_and_the_numpy_bound(ctx, thin, form, k):
    from bigkrls_amd import _lib
    ta, tb, alpha, beta = FORMS[form]
    rng = np.random.default_rng([20262, sorted(FORMS).index(form), k])
    opA = rng.standard_normal((max(MS), k))
    opB = rng.standard_normal((k, max(NS)))
    C0 = rng.standard_normal((max(MS), max(NS)))
    placedA = {m: place(ctx, np.ascontiguousarray(opA[:m].T) if ta else opA[:m]) for m in MS}
    placedB = {n: place(ctx, opB[:, :n]) for n in NS}
    worst, differ = (0.0, None), []
    for m, n in itertools.product(MS, NS):
        _, pA, lda, _, _ = placedA[m]
        _, pB, ldb, _, _ = placedB[n]
        c0 = C0[:m, :n] if beta != 0.0 else np.full((m, n), np.nan)      # (beta = 0 must not read C)

        def run(width):
            dC, pC, ldc, r0, cc0 = place(ctx, c0, fill=SENT)
            assert lda > (k if ta else m) and ldb > k and ldc > m
            if width is None:
                _lib.call("bigkrls_dev_gemm", ctx.handle, ta, tb, m, n, k, alpha, pA, lda, pB, ldb, beta, pC, ldc)
            else:
                _lib.check(thin(ctx.handle, ta, tb, m, n, k, alpha, pA, lda, pB, ldb, beta, pC, ldc, width))
            return dC, r0, cc0

        want = np.ascontiguousarray(run(None)[0].to_numpy()).tobytes()
        for width in WIDTHS:
            dC, r0, cc0 = run(width)
            if np.ascontiguousarray(dC.to_numpy()).tobytes() != want:
                differ.append((m, n, width))
        blk = take(dC, r0, cc0, m, n, (form, m, n, k))                  # the rule's result
        ref = alpha * (opA[:m] @ opB[:, :n]) + (beta * C0[:m, :n] if beta != 0.0 else 0.0)
        bound = (k + 4) * U * (abs(alpha) * (np.abs(opA[:m]) @ np.abs(opB[:, :n]))
                               + (abs(beta) * np.abs(C0[:m, :n]) if beta != 0.0 else 0.0))
        assert np.isfinite(blk).all(), (form, m, n, k)
        ratio = float(np.max(np.abs(blk - ref) / bound))
        worst = max(worst, (ratio, (m, n)))
    print(f"{form} k={k}: {len(MS) * len(NS)} shapes x {len(WIDTHS)} widths; largest |C - C_ref| / bound = {worst[0]:.3g} "
          f"at (m, n) = {worst[1]}; not gemm()'s bits at (m, n, width): {differ}")
    assert not differ, f"{form} k={k}: (m, n, width) whose output is not bigkrls_dev_gemm's bit for bit: {differ}"
    assert worst[0] <= 1.0, f"{form} k={k}: outside the bound at (m, n) = {worst[1]}: error / bound = {worst[0]}"


def test_zero_sizes_and_bad_arguments(ctx, thin):
    from bigkrls_amd import _lib
    d = ctx.from_numpy(np.asfortranarray(np.full((8, 8), SENT)))
    for width in WIDTHS:
        assert thin(ctx.handle, 0, 0, 0, 5, 4, 1.0, d.ptr, 8, d.ptr, 8, 0.0, d.ptr, 8, width) == _lib.OK
        assert thin(ctx.handle, 0, 0, 5, 0, 4, 1.0, d.ptr, 8, d.ptr, 8, 0.0, d.ptr, 8, width) == _lib.OK
        assert thin(ctx.handle, 0, 0, 5, 5, 0, 1.0, d.ptr, 8, d.ptr, 8, 1.0, d.ptr, 8, width) == _lib.OK
    assert (d.to_numpy() == SENT).all()
    assert thin(ctx.handle, 0, 0, -1, 5, 4, 1.0, d.ptr, 8, d.ptr, 8, 0.0, d.ptr, 8, 0) == _lib.EINVAL
    assert thin(ctx.handle, 0, 0, 5, 5, 4, 1.0, None, 8, d.ptr, 8, 0.0, d.ptr, 8, 0) == _lib.EINVAL


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("width", ("32", "64", "128"))
@pytest.mark.parametrize("name", ("n259", "n1100"))
def test_back_transform_digests_at_every_width(ctx, golden, monkeypatch, name, width):
    Xs = back_half.make_input(name)
    assert back_half._sha(Xs) == golden[name]["input"], f"the INPUT of {name} is not the recorded one (another numpy?)"
    monkeypatch.setenv("BIGKRLS_BT1_TILE", width)
    got = back_half.run_case(ctx, name, Xs)
    print(f"{name} BIGKRLS_BT1_TILE={width}: {got}")
    assert got["info"] == golden[name]["info"]
    assert got["digests"] == golden[name]["digests"]
