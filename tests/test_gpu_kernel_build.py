"""The kernel builds of csrc/gemm.hip (kernel_block, kernel_contract) where the rest of the suite does not reach:

1. the 128 x 128 workgroup-tiled build (u, v >= 1024 and p > 32: the kernel of the largest configuration) entry by
   entry -- symmetric and rectangular, edge tiles, the scalar store path, a rank's column block;
2. the hand-written exponentials (exp_nonpos_tab, exp_nonpos) over their whole domain, with exact arguments driven
   through the public entry points;
3. data that are not centred: the builds expand |a - b|^2 into norms and a product, which cancels on rows far from the
   origin unless both operands are first moved by a common vector."""
import ctypes as C

import numpy as np
import pytest

from bigkrls_amd import _lib, ops
from oracle import krls_oracle as orc

pytestmark = pytest.mark.gpu

L = np.longdouble
SENT = -98765.4321          # finite and non-zero: `==` on it is a bitwise comparison


def F(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def P(a):
    return C.c_void_p(a.ctypes.data)


def check(lib, status):
    assert status == 0, lib.bigkrls_last_error().decode()


# ---- 1. the tiled kernel, entry by entry -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(1024, 33), (1153, 50), (1283, 64), (1500, 140)])
def test_tiled_symmetric_build(lib, n, p):
    """kernel_block_tiled_kernel<SYM = true>: full and edge tiles, the mirrored second store, 16-byte stores (even n)
    and the scalar path (odd n, hence odd ldo)."""
    X = np.random.default_rng(n + p).standard_normal((n, p))
    Xf, out = F(X), F(np.full((n, n), np.nan))
    check(lib, lib.bigkrls_gauss_kernel(P(Xf), n, p, float(p), P(out)))
    assert np.isfinite(out).all(), "an entry was never written"
    assert np.max(np.abs(out - orc.gauss_kernel_literal(X, float(p)))) < 1e-13
    assert np.array_equal(out, out.T)
    assert np.all(np.diag(out) == 1.0)


@pytest.mark.parametrize("u,v,p", [(1024, 1300, 33), (1301, 1025, 48), (1100, 1100, 129)])
def test_tiled_rectangular_build(lib, u, v, p):
    rng = np.random.default_rng(u + v + p)
    A, B = rng.standard_normal((u, p)), rng.standard_normal((v, p))
    Af, Bf, out = F(A), F(B), F(np.full((u, v), np.nan))
    check(lib, lib.bigkrls_temp_kernel(P(Af), u, P(Bf), v, p, float(p), P(out)))
    assert np.isfinite(out).all(), "an entry was never written"
    assert np.max(np.abs(out - orc.temp_kernel_literal(A, B, float(p)))) < 1e-13


@pytest.mark.parametrize("n,p,c0,c1", [(1200, 40, 130, 1160), (1200, 20, 130, 500)])
def test_column_block(ctx, n, p, c0, c1):
    """K[:, c0:c1) as every rank of a multi-GPU fit builds it (B = X + c0, diag_shift = c0): the tiled kernel's
    non-symmetric build (p > 32, >= 1024 columns) and the wave kernel (p <= 32)."""
    X = np.random.default_rng(n + p).standard_normal((n, p))
    Xd = ctx.from_numpy(X)
    ref = orc.gauss_kernel_literal(X, float(p))[:, c0:c1]
    got = ops.bGaussKernel(Xd, cols=(c0, c1)).to_numpy()
    assert np.isfinite(got).all()
    assert np.max(np.abs(got - ref)) < 1e-13
    j = np.arange(c1 - c0)
    assert np.all(got[c0 + j, j] == 1.0)
    # the same block into a parent with ldo > n whose first element is only 8-byte aligned: scalar stores
    ldo, v = n + 3, c1 - c0
    par = ctx.from_numpy(np.full((ldo, v + 2), SENT, order="F"))
    assert (par.t.data_ptr() + 8 * (ldo + 2)) % 16 == 8
    _lib.call("bigkrls_dev_kernel_block", ctx.handle, Xd.ptr, n, Xd.ld, Xd.col_ptr(0, c0), v, Xd.ld, p, float(p),
              par.col_ptr(1, 2), ldo, c0)
    out = np.array(par.to_numpy())
    blk = out[2:2 + n, 1:1 + v].copy()
    out[2:2 + n, 1:1 + v] = SENT
    assert (out == SENT).all(), "the build wrote outside its block"
    assert np.array_equal(blk, got)          # the store path does not change a value


# ---- 2. the exponentials over their whole domain --------------------------------------------------------------------
def _exp_arguments():
    """x >= 0 (the kernels evaluate exp(-x)), every one of the form fl(t^2) so that it can be driven exactly."""
    rng = np.random.default_rng(42)
    step = np.log(2.0) / 32.0
    j = np.arange(0, int(40.0 / step) + 2, dtype=np.float64)
    ulps = np.array([-3.0, -1.0, 0.0, 1.0, 3.0]) * 2.0 ** -52
    table_edges = ((j[:, None] * step) * (1.0 + ulps)).ravel()               # multiples of ln2/32: the reduced argument changes sign
    index_edges = (((j[:, None] + 0.5) * step) * (1.0 + ulps)).ravel()       # ... and where the table index steps
    binades = (2.0 ** np.arange(-80, 6, dtype=np.float64)[:, None] * (1.0 + ulps)).ravel()
    x = np.concatenate([
        [0.0, 1e-320, 1e-16, 1e-300],
        table_edges, index_edges, binades,
        rng.uniform(0.0, 40.0, 3000), rng.uniform(0.0, 1.0, 500) ** 8,
        np.linspace(40.0, 700.0, 600), rng.uniform(40.0, 708.0, 600),
        np.linspace(700.0, 708.4, 400),                                     # the last normal results (exp(-708.39) = 2^-1022)
        np.linspace(708.0, 745.2, 1200),                                    # subnormal results
        np.linspace(745.0, 746.5, 200), [746.0, 747.0, 800.0, 1e3, 1e6, 1e12, 1e300],
    ])
    t = np.concatenate([np.sqrt(x[x >= 0.0]), [1e-160, 1e-8, 1e6, 1e150, 1e300]])
    with np.errstate(over="ignore"):
        return t, t * t                                                       # (1e300^2 = inf: the result must be 0, not NaN)


def _check_exp(name, got, x):
    """relative error <= 2^-51 (2 ulp) where the true value is a normal number, absolute error <= 2 * 2^-1074 below,
    exactly 0 from -746 on. From the code: the Cody-Waite reduction is exact in its first product (the constant has 21
    trailing zero bits, |n| < 2^16) and rounds r twice (< 1.3e-18 each), the degree-6 polynomial truncates at 5e-18,
    the table entry and the final fma add 0.5 ulp each."""
    assert got.shape == x.shape
    assert not np.isnan(got).any(), f"{name}: NaN at x = {x[np.isnan(got)][:5]}"
    with np.errstate(under="ignore"):
        ref = np.exp(-np.minimum(x, 2e4).astype(L))
    err = np.abs(got.astype(L) - ref)
    normal = ref >= L(2.0) ** -1022
    rel = float(np.max(err[normal] / ref[normal]))
    sub = float(np.max(err[~normal])) / 2.0 ** -1074
    print(f"{name}: {x.size} arguments, largest relative error {rel / 2.0 ** -52:.3f} ulp (at x = "
          f"{x[normal][np.argmax(err[normal] / ref[normal])]!r}), largest subnormal-range error {sub:.3f} x 2^-1074")
    assert rel <= 2.0 ** -51, f"{name}: relative error {rel / 2.0 ** -52:.3f} ulp at x = {x[normal][np.argmax(err[normal] / ref[normal])]!r}"
    assert sub <= 2.0, f"{name}: absolute error {sub} x 2^-1074 below the normal range"
    assert np.all(got[x >= 746.0] == 0.0), f"{name}: not exactly 0 from -746 on"
    assert np.all(got[x == 0.0] == 1.0)


@pytest.mark.parametrize("name,u,p", [("wave kernel (exp_nonpos_tab)", 1, 1), ("tiled kernel (exp_nonpos_tab)", 1024, 33),
                                      ("p > 128 kernel (exp_nonpos)", 1, 129)])
def test_exponential_whole_domain(ctx, name, u, p):
    """A = 0 and B = [t, 0, ...] with sigma = 1 give d2 = fl(t_j^2) exactly, so entry j is exp(-fl(t_j^2))."""
    t, x = _exp_arguments()
    v = t.size
    assert v >= 1024
    B = np.zeros((v, p))
    B[:, 0] = t
    out = ops.bTempKernel(ctx.from_numpy(np.zeros((u, p))), ctx.from_numpy(B), 1.0).to_numpy()
    assert np.array_equal(out, np.broadcast_to(out[0], out.shape))       # every row of A is the same point
    _check_exp(name, np.ascontiguousarray(out[0]), x)


def test_exponential_whole_domain_contract_kernel(ctx):
    """The fused contraction with trans = 1, u = 1 and W = [1]: out[j] = K(A, B)[0, j] * 1."""
    t, x = _exp_arguments()
    B = t[:, None].copy()
    out = ops.bKernelContract(ctx.from_numpy(np.zeros((1, 1))), ctx.from_numpy(B), ctx.from_numpy(np.ones((1, 1))), 1.0,
                              trans=1).to_numpy()
    _check_exp("contract kernel (exp_nonpos_tab)", np.ascontiguousarray(out[:, 0]), x)


# ---- 3. data that are not centred ------------------------------------------------------------------------------------
# X = Z + offset g with Z (n x p) and g (p) standard normal. Reference: the literal loop in np.longdouble. Bound,
# elementwise, with z~ = X - colmean(A) (longdouble; the means of A for both operands):
#     |K - ref| <= ref (p + 12) 2^-53 (|z~_i| + |z~_j|)^2 / sigma + 4 * 2^-53
# -- the forward error of the norm expansion on the centred rows (p-term sums of products bounded by
# (|z~_i| + |z~_j|)^2, divided by sigma, times the derivative ref of the exponential) plus the exponential itself.
OFFSETS = [0.0, 10.0, 1e3, 1e5]


def _literal_ld(A, B, sigma):
    A, B = A.astype(L), B.astype(L)
    out = np.empty((A.shape[0], B.shape[0]), dtype=L)
    for i in range(A.shape[0]):
        d = A[i] - B
        out[i] = np.exp(-np.sum(d * d, axis=1) / L(sigma))
    return out


def _bound(A, B, sigma, ref):
    mu = np.mean(A.astype(L), axis=0)
    na = np.sqrt(np.sum((A.astype(L) - mu) ** 2, axis=1))
    nb = np.sqrt(np.sum((B.astype(L) - mu) ** 2, axis=1))
    p = A.shape[1]
    return ref * (p + 12) * L(2.0) ** -53 * (na[:, None] + nb[None, :]) ** 2 / L(sigma) + 4 * L(2.0) ** -53


def _shifted(rng, rows, p, offset):
    g = rng.standard_normal(p)
    return [rng.standard_normal((r, p)) + offset * g for r in rows]


def _assert_within(got, ref, bound, what):
    ratio = (np.abs(got.astype(L) - ref) / bound).astype(np.float64)
    worst = float(np.max(ratio))
    print(f"{what}: largest |error| {float(np.max(np.abs(got.astype(L) - ref))):.3g}, largest error / bound {worst:.3g}")
    assert np.isfinite(got).all()
    assert worst <= 1.0, f"{what}: error / bound = {worst:.3g} at {np.unravel_index(np.argmax(ratio), ratio.shape)}"


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("n,p", [(300, 1), (300, 5), (600, 50), (400, 150), (1100, 40)])
def test_gauss_kernel_uncentred(lib, n, p, offset):
    """Every variant of the build: the symmetric wave kernel (p <= 128), the p > 128 kernel, the tiled kernel."""
    (X,) = _shifted(np.random.default_rng(1000 * p + n), [n], p, offset)
    Xf, out = F(X), F(np.full((n, n), np.nan))
    check(lib, lib.bigkrls_gauss_kernel(P(Xf), n, p, float(p), P(out)))
    ref = _literal_ld(X, X, float(p))
    _assert_within(out, ref, _bound(X, X, float(p), ref), f"gauss_kernel n={n} p={p} offset={offset:g}")
    assert np.array_equal(out, out.T) and np.all(np.diag(out) == 1.0)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("u,v,p", [(200, 333, 7), (1030, 1100, 40)])
def test_temp_kernel_uncentred(lib, u, v, p, offset):
    A, B = _shifted(np.random.default_rng(1000 * p + u), [u, v], p, offset)
    Af, Bf, out = F(A), F(B), F(np.full((u, v), np.nan))
    check(lib, lib.bigkrls_temp_kernel(P(Af), u, P(Bf), v, p, float(p), P(out)))
    ref = _literal_ld(A, B, float(p))
    _assert_within(out, ref, _bound(A, B, float(p), ref), f"temp_kernel u={u} v={v} p={p} offset={offset:g}")


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("trans", [0, 1])
def test_kernel_contract_uncentred(ctx, trans, offset):
    """K(A, B) W and K(A, B)' W: the entries' bound carried through |W|, plus the rounding of an L-term sum in any
    order, (L + 8) 2^-53 sum |K| |W|."""
    u, v, p, q = 150, 700, 6, 5
    rng = np.random.default_rng(77)
    A, B = _shifted(rng, [u, v], p, offset)
    W = rng.standard_normal((u if trans else v, q))
    got = ops.bKernelContract(ctx.from_numpy(A), ctx.from_numpy(B), ctx.from_numpy(W), float(p), trans=trans).to_numpy()
    K = _literal_ld(A, B, float(p))
    bK = _bound(A, B, float(p), K)
    if trans:
        K, bK = K.T, bK.T
    Wl = np.abs(W).astype(L)
    ref = K @ W.astype(L)
    bound = bK @ Wl + (K.shape[1] + 8) * L(2.0) ** -53 * (K @ Wl)
    _assert_within(got, ref, bound, f"kernel_contract trans={trans} offset={offset:g}")
