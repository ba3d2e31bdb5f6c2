"""The small device-resident helpers of the C ABI (csrc/vecops.hip, csrc/solveforc.hip) that the host layer and the
other tests use as instruments: bigkrls_dev_gemv, _dot, _diag, _scale, _copy_matrix, _multdiag, _qty and _solveforc
on a row block -- each against numpy.

Exact integer inputs (|value| <= 64, alpha and beta powers of two) where equality is wanted: every partial sum is an
integer below 2^53, so the result is exact in any summation order. On standard normal data the reference is computed
in np.longdouble and a length-L reduction must satisfy |got - ref| <= (L + 8) 2^-53 sum |terms| (the forward bound of
an L-term sum in any order; the 8 covers the products, alpha, beta and the combination of partial sums)."""
import ctypes as C

import numpy as np
import pytest

from bigkrls_amd import _lib
from oracle import krls_oracle as orc

pytestmark = pytest.mark.gpu

L = np.longdouble
EPS = 2.0 ** -53
SENT = -98765.4321          # finite and non-zero: `==` on it is a bitwise comparison


def ints(rng, *shape):
    return rng.integers(-64, 65, size=shape).astype(np.float64)


def in_parent(ctx, block, extra_rows=3, fill=np.nan):
    """`block` uploaded as rows [1, 1 + r) of a parent with leading dimension r + extra_rows; (parent, pointer, ld)."""
    assert extra_rows >= 1
    r, c = block.shape
    host = np.full((r + extra_rows, c), fill, order="F")
    host[1:1 + r] = block
    d = ctx.from_numpy(host)
    return d, d.col_ptr(0, 1), r + extra_rows


def vec(ctx, v):
    return ctx.from_numpy(np.asarray(v, dtype=np.float64).reshape(-1, 1))


# ---- gemv ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 1000])
def test_gemv(ctx, trans, m):
    """trans = 0: one thread per row in blocks of 256, the columns split over workgroups (remainders of the split and of
    the 4-column unroll); trans = 1: one wave per column with a 256-row unroll and its tail. lda > m throughout."""
    rng = np.random.default_rng(10 * m + trans)
    for n in (1, 63, 64, 65, 200, 1000):
        lx, ly = (m, n) if trans else (n, m)
        # exact
        A, x, y0 = ints(rng, m, n), ints(rng, lx), ints(rng, ly)
        for alpha, beta in ((2.0, -0.5), (-0.25, 0.0)):
            dA, pA, lda = in_parent(ctx, A)
            yd = vec(ctx, y0 if beta != 0.0 else np.full(ly, np.nan))          # beta = 0 must not read y
            xd = vec(ctx, x)
            _lib.call("bigkrls_dev_gemv", ctx.handle, trans, m, n, alpha, pA, lda, xd.ptr, beta, yd.ptr)
            ref = alpha * ((A.T if trans else A) @ x) + beta * y0
            assert np.array_equal(yd.to_numpy().ravel(), ref), (trans, m, n, alpha, beta)
        # rounding
        A, x, y0 = rng.standard_normal((m, n)), rng.standard_normal(lx), rng.standard_normal(ly)
        alpha, beta = 0.7, -1.3
        dA, pA, lda = in_parent(ctx, A)
        yd = vec(ctx, y0)
        xd = vec(ctx, x)
        _lib.call("bigkrls_dev_gemv", ctx.handle, trans, m, n, alpha, pA, lda, xd.ptr, beta, yd.ptr)
        op = A.T if trans else A
        ref = L(alpha) * (op.astype(L) @ x.astype(L)) + L(beta) * y0.astype(L)
        bound = (lx + 8) * EPS * (abs(alpha) * (np.abs(op) @ np.abs(x)) + abs(beta) * np.abs(y0))
        err = np.abs(yd.to_numpy().ravel().astype(L) - ref).astype(np.float64)
        assert np.all(err <= bound), (trans, m, n, float(np.max(err / bound)))


def test_gemv_without_columns_scales_y(ctx):
    """trans = 0 and n = 0: y = beta y (the partial sums are empty, the reduction applies beta)."""
    rng = np.random.default_rng(3)
    A = ctx.from_numpy(np.full((300, 1), np.nan))
    x = vec(ctx, [np.nan])
    y0 = ints(rng, 300)
    yd = vec(ctx, y0)
    _lib.call("bigkrls_dev_gemv", ctx.handle, 0, 300, 0, 2.0, A.ptr, 300, x.ptr, -0.5, yd.ptr)
    assert np.array_equal(yd.to_numpy().ravel(), -0.5 * y0)
    yd = vec(ctx, np.full(300, np.nan))
    _lib.call("bigkrls_dev_gemv", ctx.handle, 0, 300, 0, 2.0, A.ptr, 300, x.ptr, 0.0, yd.ptr)
    assert np.array_equal(yd.to_numpy().ravel(), np.zeros(300))


# ---- dot -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1024 * 256 + 3])
def test_dot(ctx, n):
    """Up to 1024 workgroups of 256 threads: the last size runs the grid-stride loop."""
    rng = np.random.default_rng(n)
    out = C.c_double(np.nan)
    x, y = ints(rng, max(n, 1)), ints(rng, max(n, 1))
    xd, yd = vec(ctx, x), vec(ctx, y)
    _lib.call("bigkrls_dev_dot", ctx.handle, n, xd.ptr, yd.ptr, C.byref(out))
    assert out.value == float(x[:n] @ y[:n])
    x, y = rng.standard_normal(max(n, 1)), rng.standard_normal(max(n, 1))
    xd, yd = vec(ctx, x), vec(ctx, y)
    _lib.call("bigkrls_dev_dot", ctx.handle, n, xd.ptr, yd.ptr, C.byref(out))
    ref = x[:n].astype(L) @ y[:n].astype(L)
    assert abs(L(out.value) - ref) <= (n + 8) * EPS * float(np.abs(x[:n]) @ np.abs(y[:n])), (n, out.value, ref)


# ---- diag, scale, copy_matrix, multdiag ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 256, 257, 700])
def test_diag_with_leading_dimension(ctx, n):
    A = np.random.default_rng(n).standard_normal((n, n))
    dA, pA, lda = in_parent(ctx, A, extra_rows=4)
    out = vec(ctx, np.full(n, np.nan))
    _lib.call("bigkrls_dev_diag", ctx.handle, pA, n, lda, out.ptr)
    assert np.array_equal(out.to_numpy().ravel(), np.diag(A))


@pytest.mark.parametrize("n", [1, 257, 4096 * 256 + 5])
def test_scale(ctx, n):
    """x *= alpha over n elements of a longer vector (4096 workgroups at most: the last size runs the grid-stride loop)."""
    x = np.random.default_rng(n).standard_normal(n + 2)
    d = vec(ctx, x)
    _lib.call("bigkrls_dev_scale", ctx.handle, n, -1.7, d.col_ptr(0, 1))
    ref = x.copy()
    ref[1:1 + n] *= -1.7
    assert np.array_equal(d.to_numpy().ravel(), ref)


@pytest.mark.parametrize("m,n", [(1, 1), (257, 33), (1000, 70)])
def test_copy_matrix(ctx, m, n):
    A = np.random.default_rng(m + n).standard_normal((m, n))
    # plain copy: lds == ldd == m
    dst = ctx.from_numpy(np.full((m, n), np.nan))
    src = ctx.from_numpy(A)
    _lib.call("bigkrls_dev_copy_matrix", ctx.handle, src.ptr, m, n, m, dst.ptr, m)
    assert np.array_equal(dst.to_numpy(), A)
    # strided: different leading dimensions on the two sides
    for src_pad, dst_pad in ((3, 5), (1, 2), (4, 1)):
        src, psrc, lds = in_parent(ctx, A, src_pad)
        dpar, pdst, ldd = in_parent(ctx, np.full((m, n), np.nan), dst_pad, fill=SENT)
        _lib.call("bigkrls_dev_copy_matrix", ctx.handle, psrc, m, n, lds, pdst, ldd)
        out = np.array(dpar.to_numpy())
        assert np.array_equal(out[1:1 + m], A), (src_pad, dst_pad)
        out[1:1 + m] = SENT
        assert (out == SENT).all(), "copy_matrix wrote outside the destination block"


@pytest.mark.parametrize("n,k", [(1, 1), (300, 70), (1001, 33)])
def test_multdiag_with_leading_dimensions(ctx, n, k):
    rng = np.random.default_rng(n + k)
    A, d = rng.standard_normal((n, k)), rng.standard_normal(k)
    dA, pA, lda = in_parent(ctx, A, 3)
    dO, pO, ldo = in_parent(ctx, np.full((n, k), np.nan), 6, fill=SENT)
    dd = vec(ctx, d)
    _lib.call("bigkrls_dev_multdiag", ctx.handle, pA, n, k, lda, dd.ptr, pO, ldo)
    out = np.array(dO.to_numpy())
    assert np.array_equal(out[1:1 + n], A * d)
    out[1:1 + n] = SENT
    assert (out == SENT).all(), "multdiag wrote outside its block"


# ---- qty, solveforc on a row block ---------------------------------------------------------------------------------------
def _eigen_like(n, k, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, k)))
    d = np.sort(rng.uniform(0.01, 50.0, k))[::-1].copy()
    return np.asfortranarray(Q), d, rng.standard_normal(n)


@pytest.mark.parametrize("n,k", [(1, 1), (257, 64), (1000, 130)])
def test_qty(ctx, n, k):
    Q, _, y = _eigen_like(n, k, n + k)
    dQ, pQ, ldq = in_parent(ctx, Q, 5)
    a = vec(ctx, np.full(k, np.nan))
    yd = vec(ctx, y)
    _lib.call("bigkrls_dev_qty", ctx.handle, pQ, n, k, ldq, yd.ptr, a.ptr)
    ref = Q.T.astype(L) @ y.astype(L)
    err = np.abs(a.to_numpy().ravel().astype(L) - ref).astype(np.float64)
    assert np.all(err <= (n + 8) * EPS * (np.abs(Q.T) @ np.abs(y)))
    Qi, yi = ints(np.random.default_rng(1), n, k), ints(np.random.default_rng(2), n)
    dQi, dyi = ctx.from_numpy(Qi), vec(ctx, yi)
    _lib.call("bigkrls_dev_qty", ctx.handle, dQi.ptr, n, k, n, dyi.ptr, a.ptr)
    assert np.array_equal(a.to_numpy().ravel(), Qi.T @ yi)


@pytest.mark.parametrize("n,k,r0", [(500, 120, 137), (1000, 40, 256), (300, 300, 1)])
def test_solveforc_on_row_blocks(ctx, n, k, r0):
    """bigkrls_dev_solveforc on rows [0, r0) and [r0, n) of Q (ldq = n, the pointer offset by the first row), as the
    multi-GPU lambda search calls it: the coefficients against the reference's literal row loop restricted to those rows,
    with and without c, and the two partial Le against the whole matrix's."""
    Q, d, y = _eigen_like(n, k, n + k + r0)
    lam = 0.3
    le_lit, c_lit = orc.solveforc_literal(Q, d, y, lam)
    w = 1.0 / (d.astype(L) + L(lam))
    g = (Q.astype(L) ** 2) @ w
    terms = (c_lit.astype(L) / g) ** 2
    dQ, dd, a = ctx.from_numpy(Q), vec(ctx, d), vec(ctx, np.full(k, np.nan))
    yd = vec(ctx, y)
    _lib.call("bigkrls_dev_qty", ctx.handle, dQ.ptr, n, k, n, yd.ptr, a.ptr)

    def probe(b0, b1, with_c):
        c = vec(ctx, np.full(b1 - b0, np.nan))
        le = C.c_double(np.nan)
        _lib.call("bigkrls_dev_solveforc", ctx.handle, dQ.col_ptr(0, b0), b1 - b0, k, n, dd.ptr, a.ptr, lam,
                  c.ptr if with_c else None, C.byref(le))
        return le.value, c.to_numpy().ravel()

    scale = np.max(np.abs(c_lit))
    les = {}
    for b0, b1 in ((0, r0), (r0, n), (0, n)):
        le_c, c = probe(b0, b1, True)
        le_n, _ = probe(b0, b1, False)
        assert np.max(np.abs(c - c_lit[b0:b1])) / scale < 1e-9, (b0, b1)
        le_ref = float(np.sum(terms[b0:b1]))
        assert abs(le_c - le_ref) / le_ref < 1e-9 and abs(le_n - le_ref) / le_ref < 1e-9, (b0, b1, le_c, le_n, le_ref)
        les[(b0, b1)] = le_c
    assert abs(les[(0, n)] - le_lit) / le_lit < 1e-9
    # the multi-GPU path adds the ranks' partial sums: the same n terms summed in another order
    assert abs((les[(0, r0)] + les[(r0, n)]) - les[(0, n)]) <= (n + 8) * EPS * les[(0, n)]
