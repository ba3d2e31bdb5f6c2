"""Neffective (csrc/neff.hip) on data whose answer is exact.

Every row of X is a random permutation of p/2 ones and p/2 minus-ones, p in {4, 16, 64}: the row mean is 0, the norm of
the de-meaned row is 2, 4 or 8, so every z is exactly +-1/2, +-1/4 or +-1/8, every |z_i . z_j| is a multiple of 1/p and
r = sum_{i > j} |z_i . z_j| is exact in any order: on the device (MFMA accumulation, the per-wave fold, the fixed-order
sum of the partials) and on the host, where it comes from block-wise integer Gram products. The expected value is
N (1 - 2 r / N^2) + 1 in fp64, and the result must lie within 2 np.spacing(expected) of it: the margin allows for a
contracted multiply-add in the host formula, nothing else. One pair counted wrongly -- a wave mapped to the wrong tile,
a diagonal tile's mask, the clamped last tile, the masked k tail -- moves the result by at least 2 / (64 N), about
5e-6 at N = 6000, ten orders above the margin."""
import numpy as np
import pytest

from bigkrls_amd import _lib, ops

from _placement import place

pytestmark = pytest.mark.gpu


def pm_rows(n, p, seed):
    base = np.tile(np.r_[np.ones(p // 2), -np.ones(p // 2)], (n, 1))
    return np.random.default_rng(seed).permuted(base, axis=1)


def expected_neff(X):
    """r from integer Gram blocks: sum over all pairs of |x_i . x_j|, minus the diagonal (n p), halved, over p."""
    n, p = X.shape
    total = 0
    for i0 in range(0, n, 1024):
        total += int(np.abs(X[i0:i0 + 1024] @ X.T).sum())
    lower = (total - n * p) // 2
    assert (total - n * p) % 2 == 0
    r = lower / p                                         # p is a power of two: exact
    assert r * p == lower
    N = float(n)
    return N * (1.0 - 2.0 * r / (N * N)) + 1.0


def close_enough(got, want):
    assert abs(got - want) <= 2.0 * np.spacing(want), (got, want, (got - want) / np.spacing(want))


@pytest.mark.parametrize("p", [4, 16, 64])
@pytest.mark.parametrize("n", [31, 32, 33, 64, 65, 1025, 6000])
def test_neffective_exact(ctx, n, p):
    """n around the 32 x 32 wave tile (a single diagonal tile, exactly full, one row past; two tiles per side and one
    row past), 33 tiles per side, and 188 tiles per side = 17 766 waves through the float sqrt of the tile map.
    p = 4: one partly masked chunk of the k loop; p = 16: exactly one chunk; p = 64: four."""
    X = pm_rows(n, p, 100 * n + p)
    close_enough(ops.bNeffective(ctx.from_numpy(X)), expected_neff(X))


def test_dev_neffective_on_a_sub_block(ctx):
    """X as an odd-offset block of a NaN-filled parent (ldx > n); ldx < n is rejected and the output left alone."""
    n, p = 97, 16
    X = pm_rows(n, p, 5)
    dX, pX, ldx, _, _ = place(ctx, X)
    assert ldx > n
    out = np.full(3, -7.0)
    _lib.call("bigkrls_dev_neffective", ctx.handle, pX, n, ldx, p, out[1:].ctypes.data)
    assert out[0] == -7.0 and out[2] == -7.0
    close_enough(float(out[1]), expected_neff(X))
    out[:] = -7.0
    with pytest.raises(_lib.BigKRLSError) as e:
        _lib.call("bigkrls_dev_neffective", ctx.handle, pX, n, n - 1, p, out[1:].ctypes.data)
    assert e.value.code == _lib.EINVAL and (out == -7.0).all()
    close_enough(ops.bNeffective(ctx.from_numpy(X)), expected_neff(X))


def test_constant_row_gives_nan(ctx):
    """A constant row has norm 0 after de-meaning: 0/0, NaN in its correlations and in the result, as in the
    reference (src/Neffective.cpp:29-44; documented at neff_rowstd_kernel)."""
    X = pm_rows(70, 16, 6)
    X[41] = 3.0
    assert np.isnan(ops.bNeffective(ctx.from_numpy(X)))
