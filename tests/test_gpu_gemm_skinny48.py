"""bigkrls_dev_gemm_skinny48 (csrc/gemm.hip: gemm_nn_skinny48, gemm_nn48_kernel, splitk_reduce_kernel): C = A B with at
most 48 columns, the 128 x 48 tile of the marginal-effects pass, by the method of test_gpu_gemm_core.py. A and B sit
inside NaN-filled parents with odd leading dimensions; C starts as NaN (nothing of it may be read) inside a
sentinel-filled parent with ldc > m.

Exact reference: integer entries in [-64, 64]; every partial sum is an integer below 2^53, so the result does not depend
on the summation order, the split count or FMA contraction and must equal the numpy fp64 product bit for bit.
Rounding reference: standard normal inputs, the product in np.longdouble and test_gpu_gemm_core's bound
    |C - ref| <= (k + 70) 2^-53 |A||B|
(a k-term inner product summed in any order; the 70 covers at most 64 split-K slabs and their reduction). Derived, not
measured.

Production calls this kernel with 33 <= n <= 48 and m = k >= 4096 only (csrc/deriv.hip); the shapes here leave that
domain on purpose: m around the 128-row tile, n = 48 (the strided B loader) and n < 48 (the clamped one), k from one
partial k-tile through the two-in-flight pipeline's prologue, even and odd halves and early exits, and 1, 2, 4 and 57
split-K slabs by the host's cost model (k = 255, 512, 1100, 16 389 at m = 129) with a partial last slab."""
import numpy as np
import pytest

from bigkrls_amd import _lib

from _placement import SENT, place, take

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
MS = (1, 127, 128, 129, 300)
NS = (1, 16, 33, 42, 47, 48)
KS = (1, 15, 16, 17, 31, 32, 33, 48, 64, 80, 255, 512, 513, 1100, 16389)


def skinny_call(ctx, A, B):
    m, k = A.shape
    n = B.shape[1]
    dA, pA, lda, _, _ = place(ctx, A)
    dB, pB, ldb, _, _ = place(ctx, B)
    dC, pC, ldc, r0, c0 = place(ctx, np.full((m, n), np.nan), fill=SENT)
    assert ldc > m
    _lib.call("bigkrls_dev_gemm_skinny48", ctx.handle, m, n, k, pA, lda, pB, ldb, pC, ldc)
    return take(dC, r0, c0, m, n, ("gemm_skinny48", m, n, k))


def check_exact(ctx, rng, m, n, k):
    A = rng.integers(-64, 65, size=(m, k)).astype(np.float64)
    B = rng.integers(-64, 65, size=(k, n)).astype(np.float64)
    got, ref = skinny_call(ctx, A, B), A @ B
    if not np.array_equal(got, ref):
        bad = np.argwhere(~(got == ref))
        raise AssertionError(f"gemm_skinny48 m={m} n={n} k={k}: {len(bad)} wrong entries, first at {tuple(bad[0])}: "
                             f"got {got[tuple(bad[0])]}, expected {ref[tuple(bad[0])]}")


@pytest.mark.parametrize("n", NS)
def test_k_tiles_and_slabs(ctx, n):
    """Every k of the list at m = 129 (a full row tile and a one-row one), for every n."""
    rng = np.random.default_rng(2000 + n)
    for k in KS:
        check_exact(ctx, rng, 129, n, k)


@pytest.mark.parametrize("m", MS)
def test_row_counts(ctx, m):
    """Every m with every n; k cycles through the list so that every (m, k mod 3 class) pairing occurs."""
    rng = np.random.default_rng(2100 + m)
    for i, n in enumerate(NS):
        for k in KS[(i + m) % 3::3]:
            check_exact(ctx, rng, m, n, k)


def test_rounding_bound_and_determinism(ctx):
    rng = np.random.default_rng(22)
    m, n, k = 300, 42, 1100
    A, B = rng.standard_normal((m, k)), rng.standard_normal((k, n))
    L = np.longdouble
    ref = A.astype(L) @ B.astype(L)
    bound = (k + 70) * EPS * (np.abs(A) @ np.abs(B))
    got = skinny_call(ctx, A, B)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(L) - ref).astype(np.float64)
    worst = float(np.max(err / bound))
    print(f"gemm_skinny48 m={m} n={n} k={k}: error / bound = {worst:.3g}")
    assert worst <= 1.0, (worst, np.unravel_index(np.argmax(err / bound), err.shape))
    assert np.array_equal(got, skinny_call(ctx, A, B)), "two calls differ"


def test_many_slabs_are_deterministic(ctx):
    """k = 16 389: 57 slabs of 288 (the last one partial), summed in slab order: two calls are bitwise equal."""
    rng = np.random.default_rng(23)
    A, B = rng.standard_normal((129, 16389)), rng.standard_normal((16389, 47))
    got = skinny_call(ctx, A, B)
    assert np.isfinite(got).all() and np.array_equal(got, skinny_call(ctx, A, B))
