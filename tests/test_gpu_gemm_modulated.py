"""bigkrls_dev_gemm_modulated (csrc/gemm.hip: gemm_modulated, gemm_modulated_kernel, gemm_tile<.., MOD>):
C = (A o (r 1' + t s')) B, called through the C ABI so that leading dimensions exceed the row counts.

Exact reference: A and B hold integers with |value| <= 8, r, t and s integers with |value| <= 3. The factor
r_i + t_i s_l (|.| <= 12) and every modulated entry (|.| <= 96) are integers, and every partial sum is an integer below
96 * 8 * k < 2^53, so the result does not depend on the summation order, the split count or FMA contraction and must
equal the numpy product bit for bit: every indexing, tail and split-K error shows.

The shapes cover the three tile widths (n <= 32, n <= 64, else), one and several row tiles, rows and columns that are
no multiple of the tile, k below, at and above one k-tile of 16 with a partial last tile, and one shape at which
launch_gemm's rule takes many k splits. Operand padding holds NaN and the result's padding a sentinel: a read of the
padding that reaches the result, or a write outside the m x n block, shows."""
import numpy as np
import pytest

from bigkrls_amd import _lib

pytestmark = pytest.mark.gpu

SENT = -98765.4321          # finite and non-zero: `==` on it is a bitwise comparison
EPS = 2.0 ** -53
SPLIT_SHAPE = (130, 70, 20000)   # 2 tiles of 128 x 128, k >= 1024: the cost model takes the most splits it allows (64)


def place(ctx, block, fill=np.nan):
    """Upload `block` (r x c) inside a parent with a larger, odd leading dimension, starting at row 2 of column 1; the
    rest of the parent holds `fill`. Returns (parent, pointer, ld, r0, c0)."""
    r, c = block.shape
    ld = r + 3 if (r + 3) % 2 else r + 4
    host = np.full((ld, c + 2), fill, order="F")
    host[2:2 + r, 1:1 + c] = block
    d = ctx.from_numpy(host)
    return d, d.col_ptr(1, 2), ld, 2, 1


def vec(ctx, v):
    """a vector inside a longer one: one NaN in front, NaN behind"""
    host = np.full((v.size + 9, 1), np.nan, order="F")
    host[1:1 + v.size, 0] = v
    d = ctx.from_numpy(host)
    return d, d.col_ptr(0, 1)


def modulated(ctx, A, r, t, s, B, plain=False):
    m, k = A.shape
    n = B.shape[1]
    dA, pA, lda, _, _ = place(ctx, A)
    dB, pB, ldb, _, _ = place(ctx, B)
    dC, pC, ldc, r0, c0 = place(ctx, np.full((m, n), np.nan), fill=SENT)     # C is overwritten, never read
    if plain:
        _lib.call("bigkrls_dev_gemm", ctx.handle, 0, 0, m, n, k, 1.0, pA, lda, pB, ldb, 0.0, pC, ldc)
    else:
        (dr, pr), (dt, pt), (ds, ps) = vec(ctx, r), vec(ctx, t), vec(ctx, s)
        _lib.call("bigkrls_dev_gemm_modulated", ctx.handle, m, n, k, pA, lda, pr, pt, ps, pB, ldb, pC, ldc)
    out = np.array(dC.to_numpy())
    blk = out[r0:r0 + m, c0:c0 + n].copy()
    out[r0:r0 + m, c0:c0 + n] = SENT
    assert (out == SENT).all(), ("wrote outside the m x n block", m, n, k)
    return blk


def int_case(rng, m, n, k):
    A = rng.integers(-8, 9, size=(m, k)).astype(np.float64)
    B = rng.integers(-8, 9, size=(k, n)).astype(np.float64)
    r, t = (rng.integers(-3, 4, size=m).astype(np.float64) for _ in range(2))
    s = rng.integers(-3, 4, size=k).astype(np.float64)
    return A, r, t, s, B


def reference(A, r, t, s, B):
    return (A * (r[:, None] + t[:, None] * s[None, :])) @ B


def check_exact(ctx, rng, m, n, k):
    A, r, t, s, B = int_case(rng, m, n, k)
    got = modulated(ctx, A, r, t, s, B)
    ref = reference(A, r, t, s, B)
    assert np.isfinite(got).all(), (m, n, k, "NaN / Inf in the result")
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError(f"gemm_modulated m={m} n={n} k={k}: {len(bad)} wrong entries, first at {tuple(bad[0])}: "
                             f"got {got[tuple(bad[0])]}, expected {ref[tuple(bad[0])]}")


@pytest.mark.parametrize("m", [1, 127, 129, 300])
def test_exact_integer_product(ctx, m):
    rng = np.random.default_rng(1000 + m)
    for n in (1, 33, 64, 65, 129, 250):
        for k in (1, 15, 16, 17, 100):
            check_exact(ctx, rng, m, n, k)


def test_exact_integer_product_with_k_splits(ctx):
    m, n, k = SPLIT_SHAPE
    check_exact(ctx, np.random.default_rng(7), m, n, k)


@pytest.mark.parametrize("m,n,k", [(129, 20, 100), (300, 33, 117), (127, 250, 47), SPLIT_SHAPE, (200, 40, 3000)])
def test_repeatable_and_plain_product_at_unit_factor(ctx, m, n, k):
    """Real-valued operands: the same call twice is bitwise equal, and with r = 1, t = 0 the factor is exactly 1 and
    the result is bitwise bigkrls_dev_gemm's -- same tiles, same pipeline, same splits, same order."""
    rng = np.random.default_rng(m * 31 + n)
    A, B = rng.standard_normal((m, k)), rng.standard_normal((k, n))
    r, t, s = rng.standard_normal(m), rng.standard_normal(m), rng.standard_normal(k)
    a = modulated(ctx, A, r, t, s, B)
    b = modulated(ctx, A, r, t, s, B)
    assert np.array_equal(a, b)
    # forward bound of a k-term inner product in any order, over at most 64 slabs, plus the factor's two roundings
    F = r[:, None] + t[:, None] * s[None, :]
    ref = (A.astype(np.longdouble) * F.astype(np.longdouble)) @ B.astype(np.longdouble)
    bound = (k + 72) * EPS * ((np.abs(A) * (np.abs(r)[:, None] + np.abs(t)[:, None] * np.abs(s)[None, :])) @ np.abs(B))
    assert (np.abs(a - ref.astype(np.float64)) <= bound + 1e-300).all()
    unit = modulated(ctx, A, np.ones(m), np.zeros(m), s, B)
    plain = modulated(ctx, A, None, None, None, B, plain=True)
    assert np.array_equal(unit, plain)


def test_empty_sum_and_empty_result(ctx):
    rng = np.random.default_rng(3)
    A, r, t, s, B = int_case(rng, 5, 7, 4)
    dA, dB, dC = ctx.from_numpy(A), ctx.from_numpy(B), ctx.from_numpy(np.full((5, 7), SENT))
    (dr, pr), (dt, pt), (ds, ps) = vec(ctx, r), vec(ctx, t), vec(ctx, s)
    _lib.call("bigkrls_dev_gemm_modulated", ctx.handle, 0, 7, 4, dA.ptr, 5, pr, pt, ps, dB.ptr, 4, dC.ptr, 5)
    _lib.call("bigkrls_dev_gemm_modulated", ctx.handle, 5, 0, 4, dA.ptr, 5, pr, pt, ps, dB.ptr, 4, dC.ptr, 5)
    assert (dC.to_numpy() == SENT).all()
    _lib.call("bigkrls_dev_gemm_modulated", ctx.handle, 5, 7, 0, dA.ptr, 5, pr, pt, ps, dB.ptr, 4, dC.ptr, 5)
    assert (dC.to_numpy() == 0.0).all()
    with pytest.raises(_lib.BigKRLSError, match="leading dimension"):
        _lib.call("bigkrls_dev_gemm_modulated", ctx.handle, 5, 7, 4, dA.ptr, 4, pr, pt, ps, dB.ptr, 4, dC.ptr, 5)


def test_ops_wrapper(ctx):
    from bigkrls_amd import ops
    rng = np.random.default_rng(11)
    A, r, t, s, B = int_case(rng, 70, 9, 37)
    got = ops.bGemmModulated(ctx.from_numpy(A), r, t, ctx.from_numpy(s), ctx.from_numpy(B)).to_numpy()
    assert np.array_equal(got, reference(A, r, t, s, B))
    with pytest.raises(ValueError, match="r must be"):
        ops.bGemmModulated(ctx.from_numpy(A), r[:-1], t, s, ctx.from_numpy(B))
