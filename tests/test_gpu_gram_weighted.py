"""bigkrls_dev_gram_weighted (csrc/gemm.hip: gram_weighted, gram_weighted_kernel, gram_reduce_kernel, gemm_tile<.., WK>):
M = A' diag(omega) A, called through the C ABI so that leading dimensions exceed the row counts.

Exact reference: A holds integers with |value| <= 8 and omega integers with |value| <= 3, so every weighted entry
(|.| <= 24), every product (|.| <= 192) and every partial sum (< 192 n < 2^53) is an integer: the result does not depend
on the summation order, the split count or FMA contraction and must equal the numpy product bit for bit -- every
indexing, tail, mirroring and split-K error shows.

k covers the three tile widths (k <= 32, k <= 64, else), one tile, a partial tile, two and three tile rows (so that
diagonal and off-diagonal tiles both occur); n lies below, at and above one k-tile of 16 with a partial last tile, and
one shape makes the split plan take many slabs. Operand padding holds NaN and the result's parent a sentinel: a read
of the padding that reaches the result, or a write outside the k x k block, shows."""
import numpy as np
import pytest

from bigkrls_amd import _lib

pytestmark = pytest.mark.gpu

SENT = -98765.4321          # finite and non-zero: `==` on it is a bitwise comparison
EPS = 2.0 ** -53
SPLIT_SHAPE = (20000, 130)  # 3 computed tiles, n >= 1024: the cost model takes the most slabs it allows


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


def gram(ctx, A, omega, plain=False):
    n, k = A.shape
    dA, pA, lda, _, _ = place(ctx, A)
    dM, pM, ldm, r0, c0 = place(ctx, np.full((k, k), np.nan), fill=SENT)      # M is overwritten, never read
    if plain:
        _lib.call("bigkrls_dev_gemm", ctx.handle, 1, 0, k, k, n, 1.0, pA, lda, pA, lda, 0.0, pM, ldm)
    else:
        dw, pw = vec(ctx, omega)
        _lib.call("bigkrls_dev_gram_weighted", ctx.handle, n, k, pA, lda, pw, pM, ldm)
    out = np.array(dM.to_numpy())
    blk = out[r0:r0 + k, c0:c0 + k].copy()
    out[r0:r0 + k, c0:c0 + k] = SENT
    assert (out == SENT).all(), ("wrote outside the k x k block", n, k)
    return blk


def check_exact(ctx, rng, n, k):
    A = rng.integers(-8, 9, size=(n, k)).astype(np.float64)
    omega = rng.integers(-3, 4, size=n).astype(np.float64)
    got = gram(ctx, A, omega)
    ref = A.T @ (omega[:, None] * A)
    assert np.isfinite(got).all(), (n, k, "NaN / Inf in the result")
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError(f"gram_weighted n={n} k={k}: {len(bad)} wrong entries, first at {tuple(bad[0])}: "
                             f"got {got[tuple(bad[0])]}, expected {ref[tuple(bad[0])]}")


@pytest.mark.parametrize("k", [1, 31, 128, 129, 250, 300])
def test_exact_integer_gram(ctx, k):
    rng = np.random.default_rng(2000 + k)
    for n in (1, 15, 16, 17, 1000):
        check_exact(ctx, rng, n, k)


def test_exact_integer_gram_with_many_slabs(ctx):
    n, k = SPLIT_SHAPE
    check_exact(ctx, np.random.default_rng(8), n, k)


@pytest.mark.parametrize("n,k", [(100, 20), (117, 33), (1000, 129), (47, 250), SPLIT_SHAPE, (3000, 300)])
def test_real_operands_symmetric_repeatable_and_bounded(ctx, n, k):
    """Real-valued operands: M[i,j] == M[j,i] bit for bit, the same call twice is bitwise equal, the result lies within
    the forward bound of an n-term inner product in any order over at most 64 slabs (plus the weight's rounding), and
    with omega = 1 it agrees with bigkrls_dev_gemm(ta = 1) within that bound."""
    rng = np.random.default_rng(n * 31 + k)
    A, omega = rng.standard_normal((n, k)), rng.standard_normal(n)
    a = gram(ctx, A, omega)
    assert np.array_equal(a, a.T)
    assert np.array_equal(a, gram(ctx, A, omega))
    Al = A.astype(np.longdouble)
    ref = Al.T @ (omega.astype(np.longdouble)[:, None] * Al)
    bound = (n + 72) * EPS * (np.abs(A).T @ (np.abs(omega)[:, None] * np.abs(A)))
    err = np.abs(a - ref.astype(np.float64))
    print(f"gram_weighted n={n} k={k}: max err / bound = {np.max(err / (bound + 1e-300)):.3e}")
    assert (err <= bound + 1e-300).all()
    unit = gram(ctx, A, np.ones(n))
    plain = gram(ctx, A, None, plain=True)
    bound1 = (n + 72) * EPS * (np.abs(A).T @ np.abs(A))
    assert np.array_equal(unit, unit.T)
    assert (np.abs(unit - plain) <= bound1 + 1e-300).all()


def test_empty_shapes_and_bad_leading_dimensions(ctx):
    rng = np.random.default_rng(3)
    A = rng.integers(-8, 9, size=(5, 7)).astype(np.float64)
    dA, dM = ctx.from_numpy(A), ctx.from_numpy(np.full((7, 7), SENT))
    dw, pw = vec(ctx, np.ones(5))
    _lib.call("bigkrls_dev_gram_weighted", ctx.handle, 5, 0, dA.ptr, 5, pw, dM.ptr, 7)        # k == 0: nothing
    assert (dM.to_numpy() == SENT).all()
    _lib.call("bigkrls_dev_gram_weighted", ctx.handle, 0, 7, dA.ptr, 5, pw, dM.ptr, 7)        # n == 0: zeros
    assert (dM.to_numpy() == 0.0).all()
    with pytest.raises(_lib.BigKRLSError, match="leading dimension"):
        _lib.call("bigkrls_dev_gram_weighted", ctx.handle, 5, 7, dA.ptr, 4, pw, dM.ptr, 7)
    with pytest.raises(_lib.BigKRLSError, match="leading dimension"):
        _lib.call("bigkrls_dev_gram_weighted", ctx.handle, 5, 7, dA.ptr, 5, pw, dM.ptr, 6)


def test_ops_wrapper_and_profile_name(ctx):
    from bigkrls_amd import ops
    rng = np.random.default_rng(11)
    A = rng.integers(-8, 9, size=(70, 37)).astype(np.float64)
    omega = rng.integers(-3, 4, size=70).astype(np.float64)
    ref = A.T @ (omega[:, None] * A)
    ctx.set_profile(True)
    try:
        got = ops.bGramWeighted(ctx.from_numpy(A), omega).to_numpy()
        got_dev = ops.bGramWeighted(ctx.from_numpy(A), ctx.from_numpy(omega)).to_numpy()
        prof = ctx.get_profile("gram_weighted")
    finally:
        ctx.set_profile(False)
    assert np.array_equal(got, ref) and np.array_equal(got_dev, ref)
    ms, work, launches = prof
    assert launches == 2 and work == 2 * 70 * 37 * 38 and ms > 0.0
    with pytest.raises(ValueError, match="omega must be"):
        ops.bGramWeighted(ctx.from_numpy(A), omega[:-1])
