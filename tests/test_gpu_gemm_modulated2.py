"""bigkrls_dev_gemm_modulated2 (csrc/gemm.hip: gemm_modulated2, gemm_modulated2_kernel, gemm_tile<.., MOD, .., MOD2>):
C = (A o F) B with F[i,l] = fma(fma(t1[i], s1[l], r1[i]), fma(t2[i], s2[l], r2[i]), d), called through the C ABI so that
leading dimensions exceed the row counts. The file mirrors tests/test_gpu_gemm_modulated.py.

Exact reference: A and B hold integers with |value| <= 8, r, t, s and d integers with |value| <= 3. Each modulation
(|.| <= 12), the factor (|.| <= 147) and every modulated entry (|.| <= 1176) are integers, and every partial sum is an
integer below 1176 * 8 * k < 2^53 (k <= 20000: 1.9e8), so the result does not depend on the summation order, the split
count or FMA contraction and must equal the numpy product bit for bit: every indexing, tail and split-K error shows.

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


def product(ctx, A, mods, B, d=0.0, entry="modulated2"):
    """entry: "modulated2" (mods = r1, t1, s1, r2, t2, s2), "modulated" (mods = r, t, s) or "plain" (mods unused)."""
    m, k = A.shape
    n = B.shape[1]
    dA, pA, lda, _, _ = place(ctx, A)
    dB, pB, ldb, _, _ = place(ctx, B)
    dC, pC, ldc, r0, c0 = place(ctx, np.full((m, n), np.nan), fill=SENT)     # C is overwritten, never read
    if entry == "plain":
        _lib.call("bigkrls_dev_gemm", ctx.handle, 0, 0, m, n, k, 1.0, pA, lda, pB, ldb, 0.0, pC, ldc)
    else:
        held = [vec(ctx, v) for v in mods]
        ptrs = [p for _, p in held]
        if entry == "modulated":
            _lib.call("bigkrls_dev_gemm_modulated", ctx.handle, m, n, k, pA, lda, *ptrs, pB, ldb, pC, ldc)
        else:
            _lib.call("bigkrls_dev_gemm_modulated2", ctx.handle, m, n, k, pA, lda, *ptrs, float(d), pB, ldb, pC, ldc)
    out = np.array(dC.to_numpy())
    blk = out[r0:r0 + m, c0:c0 + n].copy()
    out[r0:r0 + m, c0:c0 + n] = SENT
    assert (out == SENT).all(), ("wrote outside the m x n block", m, n, k)
    return blk


def int_case(rng, m, n, k):
    A = rng.integers(-8, 9, size=(m, k)).astype(np.float64)
    B = rng.integers(-8, 9, size=(k, n)).astype(np.float64)
    r1, t1, r2, t2 = (rng.integers(-3, 4, size=m).astype(np.float64) for _ in range(4))
    s1, s2 = (rng.integers(-3, 4, size=k).astype(np.float64) for _ in range(2))
    d = float(rng.integers(-3, 4))
    return A, (r1, t1, s1, r2, t2, s2), B, d


def factor(mods, d):
    r1, t1, s1, r2, t2, s2 = mods
    return (r1[:, None] + t1[:, None] * s1[None, :]) * (r2[:, None] + t2[:, None] * s2[None, :]) + d


def check_exact(ctx, rng, m, n, k):
    A, mods, B, d = int_case(rng, m, n, k)
    got = product(ctx, A, mods, B, d)
    ref = (A * factor(mods, d)) @ B
    assert np.isfinite(got).all(), (m, n, k, "NaN / Inf in the result")
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError(f"gemm_modulated2 m={m} n={n} k={k}: {len(bad)} wrong entries, first at {tuple(bad[0])}: "
                             f"got {got[tuple(bad[0])]}, expected {ref[tuple(bad[0])]}")


@pytest.mark.parametrize("m", [1, 127, 129, 300])
def test_exact_integer_product(ctx, m):
    rng = np.random.default_rng(2000 + m)
    for n in (1, 33, 64, 65, 129, 250):
        for k in (1, 15, 16, 17, 100):
            check_exact(ctx, rng, m, n, k)


def test_exact_integer_product_with_k_splits(ctx):
    m, n, k = SPLIT_SHAPE
    check_exact(ctx, np.random.default_rng(8), m, n, k)


@pytest.mark.parametrize("m,n,k", [(129, 20, 100), (300, 33, 117), (127, 250, 47), SPLIT_SHAPE, (200, 40, 3000)])
def test_repeatable_bounded_and_bitwise_the_simpler_products(ctx, m, n, k):
    """Real-valued operands: the same call twice is bitwise equal; the forward error is within the bound of a k-term
    inner product; with r2 = 1, t2 = 0, d = 0 the second factor is exactly 1 and the result is bitwise
    bigkrls_dev_gemm_modulated's, and with both factors at unit bitwise bigkrls_dev_gemm's -- same tiles, same pipeline,
    same splits, same order."""
    rng = np.random.default_rng(m * 37 + n)
    A, B = rng.standard_normal((m, k)), rng.standard_normal((k, n))
    r1, t1, r2, t2 = (rng.standard_normal(m) for _ in range(4))
    s1, s2 = rng.standard_normal(k), rng.standard_normal(k)
    d = 0.75
    mods = (r1, t1, s1, r2, t2, s2)
    a = product(ctx, A, mods, B, d)
    b = product(ctx, A, mods, B, d)
    assert np.array_equal(a, b)
    # forward bound of a k-term inner product in any order, over at most 64 slabs (k + 72, as for one modulation), plus
    # the roundings of the factor: three fmas and the product with A are (1 + eps)^4 on the bound of |F| below, the first
    # modulation's own two of them counted in the 72 already: (k + 80) eps in all
    L = np.longdouble
    F = (r1.astype(L)[:, None] + t1.astype(L)[:, None] * s1.astype(L)[None, :]) * \
        (r2.astype(L)[:, None] + t2.astype(L)[:, None] * s2.astype(L)[None, :]) + L(d)
    ref = (A.astype(L) * F) @ B.astype(L)
    Fbound = (np.abs(r1)[:, None] + np.abs(t1)[:, None] * np.abs(s1)[None, :]) * \
             (np.abs(r2)[:, None] + np.abs(t2)[:, None] * np.abs(s2)[None, :]) + abs(d)
    bound = (k + 80) * EPS * ((np.abs(A) * Fbound) @ np.abs(B))
    err = np.abs(a - ref.astype(np.float64))
    print(f"gemm_modulated2 m={m} n={n} k={k}: max err / bound = {(err / (bound + 1e-300)).max():.3f}")
    assert (err <= bound + 1e-300).all()
    one, zero = np.ones(m), np.zeros(m)
    second_off = product(ctx, A, (r1, t1, s1, one, zero, s2), B, 0.0)
    first_order = product(ctx, A, (r1, t1, s1), B, entry="modulated")
    assert np.array_equal(second_off, first_order)
    unit = product(ctx, A, (one, zero, s1, one, zero, s2), B, 0.0)
    plain = product(ctx, A, None, B, entry="plain")
    assert np.array_equal(unit, plain)


def test_empty_sum_and_empty_result(ctx):
    rng = np.random.default_rng(3)
    A, mods, B, d = int_case(rng, 5, 7, 4)
    dA, dB, dC = ctx.from_numpy(A), ctx.from_numpy(B), ctx.from_numpy(np.full((5, 7), SENT))
    held = [vec(ctx, v) for v in mods]
    ptrs = [p for _, p in held]
    name = "bigkrls_dev_gemm_modulated2"
    _lib.call(name, ctx.handle, 0, 7, 4, dA.ptr, 5, *ptrs, d, dB.ptr, 4, dC.ptr, 5)
    _lib.call(name, ctx.handle, 5, 0, 4, dA.ptr, 5, *ptrs, d, dB.ptr, 4, dC.ptr, 5)
    assert (dC.to_numpy() == SENT).all()
    _lib.call(name, ctx.handle, 5, 7, 0, dA.ptr, 5, *ptrs, d, dB.ptr, 4, dC.ptr, 5)
    assert (dC.to_numpy() == 0.0).all()
    with pytest.raises(_lib.BigKRLSError, match="leading dimension"):
        _lib.call(name, ctx.handle, 5, 7, 4, dA.ptr, 4, *ptrs, d, dB.ptr, 4, dC.ptr, 5)
    with pytest.raises(_lib.BigKRLSError, match="leading dimension"):
        _lib.call(name, ctx.handle, 5, 7, 4, dA.ptr, 5, *ptrs, d, dB.ptr, 3, dC.ptr, 5)


def test_ops_wrapper(ctx):
    from bigkrls_amd import ops
    rng = np.random.default_rng(11)
    A, mods, B, d = int_case(rng, 70, 9, 37)
    r1, t1, s1, r2, t2, s2 = mods
    got = ops.bGemmModulated2(ctx.from_numpy(A), r1, t1, ctx.from_numpy(s1), r2, t2, s2, ctx.from_numpy(B), d).to_numpy()
    assert np.array_equal(got, (A * factor(mods, d)) @ B)
    ds = ctx.from_numpy(s1)                                   # one buffer for both s: the second derivative's operands
    got = ops.bGemmModulated2(ctx.from_numpy(A), r1, t1, ds, r2, t2, ds, ctx.from_numpy(B)).to_numpy()
    assert np.array_equal(got, (A * factor((r1, t1, s1, r2, t2, s1), 0.0)) @ B)
    with pytest.raises(ValueError, match="r2 must be"):
        ops.bGemmModulated2(ctx.from_numpy(A), r1, t1, s1, r2[:-1], t2, s2, ctx.from_numpy(B))
    with pytest.raises(ValueError, match="s1 must be"):
        ops.bGemmModulated2(ctx.from_numpy(A), r1, t1, s1[:-1], r2, t2, s2, ctx.from_numpy(B))
