"""bigkrls_dev_gemm (csrc/gemm.hip: gemm(), gemm_kernel, splitk_reduce_kernel, scale_matrix_kernel) against two
references, called through the C ABI so that leading dimensions can exceed the row counts and operands can be
sub-blocks of larger parents.

Exact reference: A, B and the initial C hold integers with |value| <= 64, alpha and beta are signed powers of two
(or 0). Every partial sum is an integer far below 2^53, so the result does not depend on the summation order, the
split count or FMA contraction, and must equal the numpy fp64 product bit for bit: every indexing, tail, layout and
split-K error shows.

Rounding reference: standard normal inputs, arbitrary alpha and beta, the product in np.longdouble, and elementwise
    |C - ref| <= (k + 70) 2^-53 (|alpha| |A||B| + |beta| |C0|),
the forward bound of a k-term inner product summed in any order (the 70 covers at most 64 split-K slabs, their
reduction and the epilogue). The bound is derived, not measured.

Every case is chosen from a branch of the code: the 32-, 64- and 128-wide tiles (n <= 32, n <= 64, else), the
two-k-tiles-in-flight pipeline of the narrow tiles, the clamped loader of a transposed operand whose last tile leaves
the matrix, partial last k-tiles, split-K (k >= 1024) with both cost models, the read-modify-write epilogue."""
import ctypes as C
import itertools

import numpy as np
import pytest

from bigkrls_amd import _lib

pytestmark = pytest.mark.gpu

TRANS = list(itertools.product((0, 1), (0, 1)))
SENT = -98765.4321          # finite and non-zero: `==` on it is a bitwise comparison
EPS = 2.0 ** -53


def place(ctx, block, sub, fill=np.nan):
    """Upload `block` (r x c). sub=False: a matrix of its own (ld = r). sub=True: inside a parent with an odd leading
    dimension > r, starting at row 2 of column 1 -- an odd element offset, so the block's first element is 8- but not
    16-byte aligned; the rest of the parent holds `fill`. Returns (parent DeviceMatrix, pointer, ld, r0, c0)."""
    r, c = block.shape
    if not sub:
        d = ctx.from_numpy(np.asfortranarray(block))
        return d, d.ptr, r, 0, 0
    ld = r + 3 if (r + 3) % 2 else r + 4
    host = np.full((ld, c + 2), fill, order="F")
    host[2:2 + r, 1:1 + c] = block
    d = ctx.from_numpy(host)
    assert (d.t.data_ptr() + 8 * (ld + 2)) % 16 == 8
    return d, d.col_ptr(1, 2), ld, 2, 1


def gemm_call(ctx, ta, tb, m, n, k, alpha, A, B, beta, C0, sub):
    """C = alpha op(A) op(B) + beta C0 on the device. A is stored k x m when ta else m x k, B n x k when tb else k x n.
    Everything of C's parent outside the m x n block must come back untouched. Returns the block."""
    dA, pA, lda, _, _ = place(ctx, A, sub)
    dB, pB, ldb, _, _ = place(ctx, B, sub)
    dC, pC, ldc, r0, c0 = place(ctx, C0, sub, fill=SENT)
    _lib.call("bigkrls_dev_gemm", ctx.handle, int(ta), int(tb), m, n, k, float(alpha), pA, lda, pB, ldb, float(beta),
              pC, ldc)
    out = np.array(dC.to_numpy())
    blk = out[r0:r0 + m, c0:c0 + n].copy()
    out[r0:r0 + m, c0:c0 + n] = SENT
    assert (out == SENT).all(), ("gemm wrote outside its m x n block", ta, tb, m, n, k)
    return blk


def int_operands(rng, ta, tb, m, n, k):
    A = rng.integers(-64, 65, size=(k, m) if ta else (m, k)).astype(np.float64)
    B = rng.integers(-64, 65, size=(n, k) if tb else (k, n)).astype(np.float64)
    C0 = rng.integers(-64, 65, size=(m, n)).astype(np.float64)
    return A, B, C0


def check_exact(ctx, rng, ta, tb, m, n, k, alpha, beta, sub=True):
    A, B, C0 = int_operands(rng, ta, tb, m, n, k)
    ref = alpha * ((A.T if ta else A) @ (B.T if tb else B))
    if beta != 0.0:
        ref = ref + beta * C0
    # beta = 0 must not read C: the block starts as NaN
    got = gemm_call(ctx, ta, tb, m, n, k, alpha, A, B, beta, C0 if beta != 0.0 else np.full((m, n), np.nan), sub)
    assert np.isfinite(got).all(), (ta, tb, m, n, k, alpha, beta, "NaN / Inf in the result")
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError(f"gemm ta={ta} tb={tb} m={m} n={n} k={k} alpha={alpha} beta={beta} sub={sub}: "
                             f"{len(bad)} wrong entries, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, "
                             f"expected {ref[tuple(bad[0])]}")


def check_rounding(ctx, rng, ta, tb, m, n, k, alpha, beta, sub=True):
    assert m * n * k <= 3e8
    A = rng.standard_normal((k, m) if ta else (m, k))
    B = rng.standard_normal((n, k) if tb else (k, n))
    C0 = rng.standard_normal((m, n))
    opA, opB = (A.T if ta else A), (B.T if tb else B)
    L = np.longdouble
    ref = L(alpha) * (opA.astype(L) @ opB.astype(L)) + L(beta) * C0.astype(L)
    bound = (k + 70) * EPS * (abs(alpha) * (np.abs(opA) @ np.abs(opB)) + abs(beta) * np.abs(C0))
    got = gemm_call(ctx, ta, tb, m, n, k, alpha, A, B, beta, C0, sub)
    err = np.abs(got.astype(L) - ref).astype(np.float64)
    worst = float(np.max(err / bound))
    assert worst <= 1.0, (f"gemm ta={ta} tb={tb} m={m} n={n} k={k} alpha={alpha} beta={beta}: error / bound = {worst:.3g} "
                          f"at {np.unravel_index(np.argmax(err / bound), err.shape)}")
    return got


# ---- tiles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", TRANS)
def test_tile_widths(ctx, ta, tb):
    """n through the 32-, 64- and 128-wide tiles and one past each: the last N tile leaves the matrix (with tb = 0 its
    operand takes the clamped loader). k = 40: two full k-tiles and a partial one."""
    rng = np.random.default_rng(100 + 2 * ta + tb)
    for i, n in enumerate((1, 31, 32, 33, 63, 64, 65, 129, 200)):
        alpha, beta = ((1.0, 0.0), (-2.0, 0.5), (0.5, -4.0))[i % 3]
        check_exact(ctx, rng, ta, tb, 130, n, 40, alpha, beta)


@pytest.mark.parametrize("ta,tb", TRANS)
def test_row_counts(ctx, ta, tb):
    """m around the 128-row tile: with ta = 1 the last M tile takes the clamped loader. Both the deep-pipelined
    64-wide tile and the 128-wide one."""
    rng = np.random.default_rng(200 + 2 * ta + tb)
    for i, m in enumerate((1, 127, 128, 129, 300)):
        for n in (48, 100):
            alpha, beta = ((1.0, 0.0), (0.25, -1.0))[(i + n) % 2]
            check_exact(ctx, rng, ta, tb, m, n, 50, alpha, beta)


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("n", [20, 64, 130])
def test_k_tiles(ctx, ta, tb, n):
    """One to four k-tiles of 16, a partial last tile, odd and even tile counts: n = 20 and 64 run the pipeline with two
    k-tiles in flight (its prologue, even and odd halves and every early exit), n = 130 the plain double buffer."""
    rng = np.random.default_rng(300 + 10 * n + 2 * ta + tb)
    for i, k in enumerate((1, 15, 16, 17, 32, 33, 48, 49, 64, 1000)):
        alpha, beta = ((1.0, 0.0), (-0.5, 2.0))[i % 2]
        check_exact(ctx, rng, ta, tb, 130, n, k, alpha, beta)


@pytest.mark.parametrize("ta,tb", TRANS)
def test_packed_layout(ctx, ta, tb):
    """The same kernels on operands that are matrices of their own (ld = rows, 16-byte aligned)."""
    rng = np.random.default_rng(400 + 2 * ta + tb)
    for m, n, k in ((129, 33, 17), (257, 65, 100), (64, 200, 1025)):
        check_exact(ctx, rng, ta, tb, m, n, k, -1.0, 0.5, sub=False)


# ---- split-K ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("n", [24, 64, 100])
def test_split_k_exact(ctx, ta, tb, n):
    """k >= 1024 on a small tile grid is split into slabs (gemm_kernel writes partials, splitk_reduce_kernel sums them
    and applies alpha and beta): chunk boundaries that do and do not fall on k, beta != 0 in the reduction, ldc > m."""
    rng = np.random.default_rng(500 + 10 * n + 2 * ta + tb)
    for i, k in enumerate((1024, 1025, 4099, 20000)):
        alpha, beta = ((1.0, 0.0), (2.0, -0.5))[i % 2]
        check_exact(ctx, rng, ta, tb, 70 + 60 * i, n, k, alpha, beta)
        check_exact(ctx, rng, ta, tb, 70 + 60 * i, n, k, beta or -1.0, alpha)


def test_split_k_many_tiles_long_k(ctx):
    """256 tiles and k = 16384: the other per-split cost model of launch_gemm (the block-Lanczos products), with edge
    tiles in both directions and beta applied by the reduction."""
    check_exact(ctx, np.random.default_rng(6), 0, 0, 2048 - 5, 2048 - 3, 16384, 0.5, -2.0, sub=False)


def test_split_k_is_deterministic(ctx):
    """The slabs are summed in a fixed order: two calls give bitwise equal results (the eigensolver's run-to-run
    determinism rests on this)."""
    rng = np.random.default_rng(7)
    for ta, tb in TRANS:
        m, n, k = 150, 40, 20000
        A, B = rng.standard_normal((k, m) if ta else (m, k)), rng.standard_normal((n, k) if tb else (k, n))
        C0 = rng.standard_normal((m, n))
        outs = [gemm_call(ctx, ta, tb, m, n, k, 0.7, A, B, -1.3, C0, True) for _ in range(2)]
        assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1]), (ta, tb)


# ---- rounding reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", TRANS)
def test_rounding_bound(ctx, ta, tb):
    rng = np.random.default_rng(800 + 2 * ta + tb)
    for m, n, k, alpha, beta in ((129, 65, 1000, 0.7, -1.3), (300, 33, 49, -1.9, 0.3), (130, 200, 1025, 0.7, -1.3),
                                 (77, 20, 4099, 3.1, 0.0), (40, 64, 20000, -0.7, 1.3)):
        check_rounding(ctx, rng, ta, tb, m, n, k, alpha, beta)


# ---- degenerate calls --------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_empty_output_does_nothing(ctx):
    rng = np.random.default_rng(9)
    A, B = ctx.from_numpy(rng.standard_normal((8, 8))), ctx.from_numpy(rng.standard_normal((8, 8)))
    C0 = rng.standard_normal((8, 8))
    C0[0, 0] = np.nan
    Cd = ctx.from_numpy(C0)
    for m, n in ((0, 8), (8, 0), (0, 0)):
        _lib.call("bigkrls_dev_gemm", ctx.handle, 0, 0, m, n, 8, 2.0, A.ptr, 8, B.ptr, 8, 3.0, Cd.ptr, 8)
    assert np.array_equal(_bits(Cd.to_numpy()), _bits(C0))


@pytest.mark.parametrize("k,alpha", [(0, 1.5), (37, 0.0), (0, 0.0)])
def test_no_product_scales_c(ctx, k, alpha):
    """k = 0 or alpha = 0: C = beta C (scale_matrix_kernel), A and B are not read -- they are NULL when k = 0 and full of
    NaN otherwise. beta = 0 turns a NaN-filled C into zeros, beta = 1 leaves C untouched bit for bit."""
    rng = np.random.default_rng(10)
    m, n, ldc = 70, 33, 75
    nanmat = ctx.from_numpy(np.full((max(m, n), max(k, 1)), np.nan))
    pA = pB = None if k == 0 else nanmat.ptr
    for beta in (0.0, 1.0, -0.5):
        host = np.full((ldc, n + 1), SENT, order="F")
        blk = rng.integers(-64, 65, size=(m, n)).astype(np.float64)
        if beta == 0.0:
            blk[:] = np.nan
        if beta == 1.0:
            blk[3, 4], blk[5, 6] = np.nan, -0.0
        host[2:2 + m, 1:] = blk
        Cd = ctx.from_numpy(host)
        _lib.call("bigkrls_dev_gemm", ctx.handle, 0, 1, m, n, k, alpha, pA, max(m, n), pB, max(m, n), beta, Cd.col_ptr(1, 2), ldc)
        out = np.array(Cd.to_numpy())
        got = out[2:2 + m, 1:].copy()
        out[2:2 + m, 1:] = SENT
        assert (out == SENT).all(), (k, alpha, beta, "wrote outside the block")
        if beta == 1.0:
            assert np.array_equal(_bits(got), _bits(blk)), (k, alpha)
        else:
            assert np.array_equal(got, np.zeros((m, n)) if beta == 0.0 else beta * blk), (k, alpha, beta)


# ---- Level-1 wrappers ------------------------------------------------------------------------------------------------
def test_level1_crossprods_take_split_k(lib):
    """bigkrls_crossprod / bigkrls_tcrossprod with an inner dimension >= 4096 (split-K through the host-pointer path)."""
    rng = np.random.default_rng(11)
    P = lambda a: C.c_void_p(a.ctypes.data)
    n, ak, bk = 4100, 40, 17
    A = np.asfortranarray(rng.integers(-64, 65, size=(n, ak)).astype(np.float64))
    B = np.asfortranarray(rng.integers(-64, 65, size=(n, bk)).astype(np.float64))
    out = np.asfortranarray(np.full((ak, bk), np.nan))
    assert lib.bigkrls_crossprod(P(A), n, ak, P(B), bk, P(out)) == 0, lib.bigkrls_last_error()
    assert np.array_equal(out, A.T @ B)
    an, k, bn = 33, 5000, 130
    A = np.asfortranarray(rng.integers(-64, 65, size=(an, k)).astype(np.float64))
    B = np.asfortranarray(rng.integers(-64, 65, size=(bn, k)).astype(np.float64))
    out = np.asfortranarray(np.full((an, bn), np.nan))
    assert lib.bigkrls_tcrossprod(P(A), an, k, P(B), bn, P(out)) == 0, lib.bigkrls_last_error()
    assert np.array_equal(out, A @ B.T)
