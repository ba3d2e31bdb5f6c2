"""marginal_effects() on the GPU: the fused kernel contraction against the unfused chain, the in-sample identity with
the fit's own marginal effects, agreement with predict() and with the numpy restatement out of sample, bitwise
reproducibility and the device-memory bound (the u x n test kernel is never formed)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_me_cpu", os.path.join(_HERE, "test_marginal_effects_cpu.py"))
_me_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_me_cpu)
me_numpy = _me_cpu.me_numpy


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.fixture(scope="module")
def ctx():
    import bigkrls_amd as bk
    return bk.api.default_context()


# ---- Level 2: fused contraction == kernel_block + gemm ----------------------------------------------------------
def _contract_cases():
    sizes = (1, 15, 17, 513, 4099)
    ps, qs = (1, 3, 20, 67), (1, 16, 21, 68)
    out, i = [], 0
    for u in sizes:
        for v in sizes:
            out.append((u, v, ps[i % 4], qs[(i // 4 + i) % 4]))
            i += 1
    return out


@pytest.mark.parametrize("u,v,p,q", _contract_cases())
def test_kernel_contract_matches_unfused_chain(ctx, u, v, p, q):
    from bigkrls_amd import ops, _lib
    rng = np.random.default_rng(u * 7919 + v * 31 + p * 3 + q)
    A = rng.standard_normal((u, p)) * 0.7
    B = rng.standard_normal((v, p)) * 0.7
    sigma = float(p)
    dA, dB = ctx.from_numpy(A), ctx.from_numpy(B)
    K = ops.bTempKernel(dA, dB, sigma)                                    # kernel_block, diag_shift = -1
    for trans in (0, 1):
        W = rng.standard_normal((v if trans == 0 else u, q))
        dW = ctx.from_numpy(W)
        got = ops.bKernelContract(dA, dB, dW, sigma, trans=trans).to_numpy()
        m = u if trans == 0 else v
        ref = ctx.empty(m, q)
        _lib.call("bigkrls_dev_gemm", ctx.handle, trans, 0, m, q, v if trans == 0 else u, 1.0, K.ptr, K.ld,
                  dW.ptr, dW.ld, 0.0, ref.ptr, ref.ld)
        assert got.shape == (m, q)
        assert rel(got, ref.to_numpy()) < 1e-13, (trans, u, v, p, q)


# ---- fits shared by the tests below -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_c3():
    import bigkrls_amd as bk
    from bigkrls_amd.synth import synth
    X, y = synth(20000, 20, 103)
    return bk.bigKRLS(y, X, eigtrunc=0.001)


@pytest.fixture(scope="module")
def fit_binary_p67():
    """N = 3000, P = 67 with 50 binary columns (the shape of the reference's examples/data2016GE.csv)."""
    import bigkrls_amd as bk
    rng = np.random.default_rng(2016)
    n = 3000
    Xc = rng.standard_normal((n, 17))
    Xb = (rng.random((n, 50)) < rng.uniform(0.05, 0.6, size=50)).astype(np.float64)
    X = np.hstack([Xc, Xb])
    beta = rng.standard_normal(67) / 8.0
    y = np.sin(X @ beta) + 0.25 * rng.standard_normal(n)
    return bk.bigKRLS(y, X)


@pytest.fixture(scope="module")
def fit_small():
    import bigkrls_amd as bk
    from oracle import krls_oracle as orc
    X, y = orc.synth(300, 4, 21, binary_last=True)
    return bk.bigKRLS(y, X)


def _identity(out, newdata=None, which=None, exp_D=None):
    import bigkrls_amd as bk
    X = out["X"]
    me = bk.marginal_effects(out, X if newdata is None else newdata, which_derivatives=which)
    D = out["derivatives"] if exp_D is None else exp_D
    assert me["derivatives"].shape == D.shape
    assert rel(me["derivatives"], D) < 1e-9
    assert rel(me["avgderivatives"], np.asarray(D).mean(axis=0)[None, :]) < 1e-9
    return me


# ---- in-sample identity -------------------------------------------------------------------------------------------
def test_in_sample_identity_c3(fit_c3):
    from bigkrls_amd.device import is_device_matrix
    assert is_device_matrix(fit_c3["vcov.est.c"])
    me = _identity(fit_c3)
    assert rel(me["avgderivatives"], fit_c3["avgderivatives"]) < 1e-9
    assert me["var.avgderivatives"].shape == fit_c3["var.avgderivatives"].shape
    assert rel(me["var.avgderivatives"], fit_c3["var.avgderivatives"]) < 1e-8


def test_in_sample_identity_with_which_derivatives(fit_small):
    import bigkrls_amd as bk
    X, y = fit_small["X"], fit_small["y"]
    which = [4, 2]                                   # a binary and a continuous column, not in order
    out = bk.bigKRLS(y, X, which_derivatives=which)
    # the fit rescales column i of D by sd(x_i), not sd(x_which[i]) (the reference's quirk Q6): compare with the
    # standardised derivatives rescaled by the selected columns' sds, and the variances (correctly subset) as they are
    g = np.std(y, ddof=1) / X[:, [w - 1 for w in which]].std(axis=0, ddof=1)
    D = out["derivatives.std"] * g
    me = _identity(out, exp_D=D)                    # which_derivatives defaults to the object's own
    assert me["which.derivatives"] == which
    assert list(me["binaryindicator"]) == [True, False]
    assert rel(me["var.avgderivatives"], out["var.avgderivatives"]) < 1e-8


def test_in_sample_identity_p67_fifty_binary_columns(fit_binary_p67):
    out = fit_binary_p67
    assert int(np.sum(out["binaryindicator"])) == 50
    me = _identity(out)
    assert rel(me["avgderivatives"], out["avgderivatives"]) < 1e-9
    assert rel(me["var.avgderivatives"], out["var.avgderivatives"]) < 1e-8


def test_rows_subset(fit_binary_p67):
    import bigkrls_amd as bk
    out = fit_binary_p67
    rows = np.random.default_rng(3).choice(out["X"].shape[0], 77, replace=False)
    me = bk.marginal_effects(out, out["X"][rows])
    assert rel(me["derivatives"], out["derivatives"][rows]) < 1e-9


# ---- independent of the new algebra: through predict() ------------------------------------------------------------
def test_against_predict_differences(fit_small):
    import bigkrls_amd as bk
    out = fit_small
    X = out["X"]
    rng = np.random.default_rng(8)
    Z = X[rng.choice(X.shape[0], 25, replace=False)].copy()
    Z[:, :3] += 0.3 * rng.standard_normal((25, 3))              # off the training rows in the continuous columns
    me = bk.marginal_effects(out, Z)
    D = me["derivatives"]
    for j in range(X.shape[1]):
        x = X[:, j]
        if np.unique(x).size == 2:
            lo, hi = x.min(), x.max()
            Z1, Z0 = Z.copy(), Z.copy()
            Z1[:, j], Z0[:, j] = hi, lo
            fd = (bk.predict(out, Z1)["predicted"] - bk.predict(out, Z0)["predicted"]) / (hi - lo)
            assert rel(D[:, j], fd) < 1e-10, j
        else:
            h = 1e-4 * np.std(x, ddof=1)
            Zp, Zm = Z.copy(), Z.copy()
            Zp[:, j] += h
            Zm[:, j] -= h
            fd = (bk.predict(out, Zp)["predicted"] - bk.predict(out, Zm)["predicted"]) / (2 * h)
            assert rel(D[:, j], fd) < 1e-6, j


# ---- out of sample against the numpy restatement -------------------------------------------------------------------
def _vs_numpy(out, Z, which=None):
    import bigkrls_amd as bk
    me = bk.marginal_effects(out, Z, which_derivatives=which)
    V = out["vcov.est.c"]
    V = V.to_numpy() if hasattr(V, "to_numpy") else V
    D, avg, var = me_numpy(out["X"], out["y"], out["coeffs"], out["sigma"], Z, vcov_c=V,
                           which=which or out.get("which.derivatives"))
    scale = max(np.abs(D).max(), 1e-300)
    assert np.max(np.abs(me["derivatives"] - D)) <= 1e-10 * scale + 1e-300
    assert np.max(np.abs(me["avgderivatives"].ravel() - avg)) <= 1e-10 * scale + 1e-300
    vs = max(np.abs(var).max(), 1e-300)
    assert np.max(np.abs(me["var.avgderivatives"].ravel() - var)) <= 1e-8 * vs + 1e-300
    return me


def test_out_of_sample_shapes(fit_small):
    out = fit_small
    X = out["X"]
    n = X.shape[0]
    rng = np.random.default_rng(12)

    def draw(u):
        Z = rng.standard_normal((u, X.shape[1]))
        Z[:, -1] = rng.choice(np.unique(X[:, -1]), size=u)         # the binary column: training values only
        return Z
    _vs_numpy(out, draw(1))                                        # u = 1: the loop over n split across waves
    _vs_numpy(out, draw(3 * n))                                    # u = 3 n
    _vs_numpy(out, draw(37), which=[3, 4, 1])                      # u not a multiple of 16 / 32, subset of columns


def test_out_of_sample_single_column():
    import bigkrls_amd as bk
    rng = np.random.default_rng(13)
    X = rng.standard_normal((211, 1))
    y = np.sin(2 * X[:, 0]) + 0.1 * rng.standard_normal(211)
    out = bk.bigKRLS(y, X)
    _vs_numpy(out, rng.standard_normal((45, 1)))


def test_far_newdata_underflows_to_zero(fit_small):
    import bigkrls_amd as bk
    out = fit_small
    X = out["X"]
    Z = np.full((19, X.shape[1]), 1e3)
    Z[:, -1] = X[:, -1].max()
    me = bk.marginal_effects(out, Z)
    assert np.all(me["derivatives"] == 0.0)
    assert np.all(me["avgderivatives"] == 0.0)
    assert np.all(me["var.avgderivatives"] == 0.0)
    _vs_numpy(out, Z)


def test_no_variance_without_vcov(fit_small):
    import bigkrls_amd as bk
    from bigkrls_amd.api import BigKRLS
    obj = BigKRLS(fit_small)
    obj["vcov.est.c"] = None
    me = bk.marginal_effects(obj, fit_small["X"][:10])
    assert me["var.avgderivatives"] is None
    assert rel(me["derivatives"], fit_small["derivatives"][:10]) < 1e-9


def test_binary_value_not_in_training_raises(fit_small):
    import bigkrls_amd as bk
    Z = fit_small["X"][:3].copy()
    Z[1, -1] = 0.5
    with pytest.raises(ValueError, match=f"column {Z.shape[1]}"):
        bk.marginal_effects(fit_small, Z)


# ---- determinism and memory ----------------------------------------------------------------------------------------
def test_bitwise_reproducible(fit_small):
    import bigkrls_amd as bk
    rng = np.random.default_rng(4)
    Z = fit_small["X"][rng.choice(300, 200)] + 0.0
    Z[:, :3] += rng.standard_normal((200, 3))
    a = bk.marginal_effects(fit_small, Z)
    b = bk.marginal_effects(fit_small, Z)
    for k in ("derivatives", "avgderivatives", "var.avgderivatives"):
        assert np.array_equal(a[k], b[k]), k


def test_memory_bound_u40000(fit_c3, ctx):
    import torch
    import bigkrls_amd as bk
    rng = np.random.default_rng(40000)
    Z = rng.standard_normal((40000, 20))
    ctx.release_workspace()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    me = bk.marginal_effects(fit_c3, Z, ctx=ctx)
    torch.cuda.synchronize()
    assert me["derivatives"].shape == (40000, 20)
    assert np.all(np.isfinite(me["derivatives"])) and np.all(np.isfinite(me["var.avgderivatives"]))
    assert ctx.workspace_bytes() < 256 << 20
    assert torch.cuda.max_memory_allocated() - base < 256 << 20
