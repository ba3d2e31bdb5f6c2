"""partial_dependence() on the GPU: the fused leave-one-column-out pass (bigkrls_dev_kernel_loo_colsums) against the
direct sum in extended precision and against the unfused chain, and the whole path against brute force through
predict() -- one predict(se_pred=True) on the rewritten rows per grid value --, from both forms of vcov.est.c, on a
fit with many binary columns, and on an implicit fit that never stored K."""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_pd_cpu", os.path.join(_HERE, "test_partial_dependence_cpu.py"))
_pd_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_pd_cpu)
pd_numpy = _pd_cpu.pd_numpy


@pytest.fixture(scope="module")
def ctx():
    import bigkrls_amd as bk
    return bk.api.default_context()


# ---- Level 2: the fused pass -------------------------------------------------------------------------------------
CHUNK = 4   # KL_CW, csrc/gemm.hip: selected columns per wave
GROUP = 64  # KL_GROUP: selected columns per launch
LOO_CASES = [
    (1, 1, 1, [0]),
    (15, 17, 1, [0]),
    (17, 15, 3, [0, 1, 2]),
    (65, 64, 8, list(range(8))),
    (513, 129, 20, list(range(20))),
    (130, 513, 33, list(range(0, 33, 3))),
    (129, 65, 67, list(range(0, 67, 3))),
    (4099, 17, 5, list(range(5))),            # few stationary rows, many loop rows: the loop is split
    (17, 4099, 5, [4, 0]),                    # selected columns out of order
    (70, 90, 9, [8, 0, 3, 5, 2]),             # the chunk width + 1 columns
    (33, 40, 70, list(range(GROUP + 1))),     # one column more than a launch takes
]
assert len(LOO_CASES[9][3]) == CHUNK + 1


@functools.lru_cache(maxsize=None)
def _loo_inputs(case, wide):
    """(A, B, sigma, cols, longdouble reference): the direct sum over the other columns, computed once per case."""
    u, v, p, cols = LOO_CASES[case]
    rng = np.random.default_rng(1000 * case + u + v + p)
    A = rng.standard_normal((u, p)) * 0.7
    B = rng.standard_normal((v, p)) * 0.7
    if wide:                                   # a wide, uncentred column: the cancellation in d2 - dj^2 is real
        A[:, 0] = A[:, 0] * 40.0 + 1000.0
        B[:, 0] = B[:, 0] * 40.0 + 1000.0
    sigma = float(p)
    Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
    sq = [(Al[:, k][:, None] - Bl[:, k][None, :]) ** 2 for k in range(p)]
    ref = np.empty((v, len(cols)), dtype=np.longdouble)
    for jj, c in enumerate(cols):
        d2 = np.zeros((u, v), dtype=np.longdouble)
        for k in range(p):
            if k != c:
                d2 += sq[k]
        ref[:, jj] = np.exp(-d2 / np.longdouble(sigma)).sum(axis=0)
    for a in (A, B, ref):
        a.setflags(write=False)
    return A, B, sigma, cols, ref


def _restatement_f64(A, B, sigma, cols):
    """The formula of the pass in float64 numpy: both operands moved by the column means of A (the contract of the
    entry, as bigkrls_dev_kernel_block), d2 = max(|a|^2 + |b|^2 - 2 a.b, 0), then max(d2 - dj^2, 0)."""
    sh = A.mean(axis=0)
    Ac, Bc = A - sh, B - sh
    d2 = np.maximum((Ac ** 2).sum(axis=1)[:, None] + (Bc ** 2).sum(axis=1)[None, :] - 2.0 * (Ac @ Bc.T), 0.0)
    out = np.empty((B.shape[0], len(cols)))
    for jj, c in enumerate(cols):
        dj = Ac[:, c][:, None] - Bc[:, c][None, :]
        out[:, jj] = np.exp(-np.maximum(d2 - dj * dj, 0.0) / sigma).sum(axis=0)
    return out


def _run_loo(ctx, A, B, sigma, cols):
    from bigkrls_amd import ops
    return ops.bKernelLooColsums(ctx.from_numpy(A), ctx.from_numpy(B), sigma, cols).to_numpy()


def _err(got, ref):
    return float(np.max(np.abs(got.astype(np.longdouble) - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("case", range(len(LOO_CASES)))
def test_loo_colsums_against_extended_precision(ctx, case):
    A, B, sigma, cols, ref = _loo_inputs(case, False)
    got = _run_loo(ctx, A, B, sigma, cols)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    err = _err(got, ref)
    print(f"loo_colsums {LOO_CASES[case][:3]} ncols={len(cols)}: error {err:.3e} "
          f"(float64 numpy: {_err(_restatement_f64(A, B, sigma, cols), ref):.3e})")
    assert err < 1e-13


@pytest.mark.parametrize("case", range(len(LOO_CASES)))
def test_loo_colsums_wide_uncentred_column(ctx, case):
    A, B, sigma, cols, ref = _loo_inputs(case, True)
    got = _run_loo(ctx, A, B, sigma, cols)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    err = _err(got, ref)
    err64 = _err(_restatement_f64(A, B, sigma, cols), ref)
    bound = max(20.0 * err64, 1e-13)
    print(f"loo_colsums wide {LOO_CASES[case][:3]} ncols={len(cols)}: error {err:.3e}, float64 numpy {err64:.3e}, "
          f"bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("case", range(len(LOO_CASES)))
def test_loo_colsums_equals_unfused_chain_and_is_reproducible(ctx, case):
    from bigkrls_amd import ops
    A, B, sigma, cols, _ = _loo_inputs(case, False)
    u, v, p = A.shape[0], B.shape[0], A.shape[1]
    got = _run_loo(ctx, A, B, sigma, cols)
    again = _run_loo(ctx, A, B, sigma, cols)
    assert np.array_equal(got, again)
    ones = ctx.from_numpy(np.ones((u, 1)))
    chain = np.empty_like(got)
    for jj, c in enumerate(cols):
        if p == 1:                              # nothing is left of the distance: every term is exp(0)
            chain[:, jj] = float(u)
            continue
        keep = [k for k in range(p) if k != c]
        dA, dB = ctx.from_numpy(np.asfortranarray(A[:, keep])), ctx.from_numpy(np.asfortranarray(B[:, keep]))
        chain[:, jj] = ops.bKernelContract(dA, dB, ones, sigma, trans=1).to_numpy().ravel()
    assert np.max(np.abs(got - chain)) <= 1e-13 * np.max(np.abs(chain))


def test_loo_colsums_rejects_bad_columns(ctx):
    from bigkrls_amd import _lib
    A, B, sigma, _, _ = _loo_inputs(2, False)
    p = A.shape[1]
    dA, dB = ctx.from_numpy(A), ctx.from_numpy(B)
    out = ctx.empty(B.shape[0], 2)
    for cols in ([p], [0, -1], []):
        h = np.ascontiguousarray(cols, dtype=np.int64)
        with pytest.raises(_lib.BigKRLSError) as ei:
            _lib.call("bigkrls_dev_kernel_loo_colsums", ctx.handle, dA.ptr, dA.nrow, dA.ld, dB.ptr, dB.nrow, dB.ld, p,
                      sigma, h.ctypes.data if h.size else np.zeros(1, dtype=np.int64).ctypes.data, int(h.size), out.ptr,
                      out.ld)
        assert ei.value.code == _lib.EINVAL


def test_loo_colsums_profile_name(ctx):
    A, B, sigma, cols, _ = _loo_inputs(3, False)
    ctx.set_profile(True)
    try:
        _run_loo(ctx, A, B, sigma, cols)
        ms, work, launches = ctx.get_profile("kernel_loo_colsums")
    finally:
        ctx.set_profile(False)
    assert launches == 1 and work == A.shape[0] * B.shape[0] * len(cols)


# ---- fits shared by the tests below ---------------------------------------------------------------------------------
def _small_data():
    from oracle import krls_oracle as orc
    return orc.synth(300, 4, 21, binary_last=True)


@pytest.fixture(scope="module")
def fit_small():
    import bigkrls_amd as bk
    X, y = _small_data()
    return bk.bigKRLS(y, X)


@pytest.fixture(scope="module")
def fit_small_both():
    import bigkrls_amd as bk
    X, y = _small_data()
    return bk.bigKRLS(y, X, vcov_form="both")


@pytest.fixture(scope="module")
def fit_binary_p67():
    """N = 3000, P = 67 with 50 binary columns (the generator of tests/test_gpu_marginal_effects.py)."""
    import bigkrls_amd as bk
    rng = np.random.default_rng(2016)
    n = 3000
    Xc = rng.standard_normal((n, 17))
    Xb = (rng.random((n, 50)) < rng.uniform(0.05, 0.6, size=50)).astype(np.float64)
    X = np.hstack([Xc, Xb])
    beta = rng.standard_normal(67) / 8.0
    y = np.sin(X @ beta) + 0.25 * rng.standard_normal(n)
    return bk.bigKRLS(y, X)


def _host(M):
    return M.to_numpy() if hasattr(M, "to_numpy") else np.asarray(M)


def _brute_force(out, res, R, correct_SE, vcov=None):
    """Every grid value of every curve of `res` against one predict(se_pred=True) on the rows R with that column
    rewritten: pd within 1e-9 of max |pd - mean(y)| over all curves, se.pd^2 within 1e-8 relative. Returns the
    predictions of the curves, for the first differences."""
    import bigkrls_amd as bk
    u = R.shape[0]
    ym = float(np.mean(out["y"]))
    pd_scale = max(np.max(np.abs(np.concatenate(res["pd"]) - ym)), 1e-300)
    preds = []
    for jj, w in enumerate(res["which"]):
        preds.append([])
        for g, v in enumerate(res["grid"][jj]):
            Zmod = R.copy()
            Zmod[:, w - 1] = v
            pr = bk.predict(out, Zmod, se_pred=True, correct_SE=correct_SE, vcov=vcov)
            preds[-1].append(pr)
            assert abs(res["pd"][jj][g] - pr["predicted"].mean()) <= 1e-9 * pd_scale, (w, g)
            var = _host(pr["vcov.est.pred"]).sum() / u ** 2
            assert abs(res["se.pd"][jj][g] ** 2 - var) <= 1e-8 * var, (w, g)
            assert abs(res["vcov.pd"][jj][g, g] - var) <= 1e-8 * var, (w, g)
    return preds


# ---- brute force through the public API, dense form -------------------------------------------------------------------
@pytest.mark.parametrize("correct_SE", [True, False])
def test_against_predict_on_rewritten_rows(fit_small, correct_SE):
    import bigkrls_amd as bk
    out = fit_small
    X = out["X"]
    n = X.shape[0]
    res = bk.partial_dependence(out, grid=5, correct_SE=correct_SE)
    assert res["which"] == [1, 2, 3, 4] and list(res["binaryindicator"]) == [False, False, False, True]
    assert [g.size for g in res["grid"]] == [5, 5, 5, 2]
    assert np.array_equal(res["grid"][3], [X[:, 3].min(), X[:, 3].max()])
    assert np.array_equal(res["grid"][0], np.linspace(X[:, 0].min(), X[:, 0].max(), 5))
    assert res["newdata"] is None
    preds = _brute_force(out, res, X, correct_SE)
    # the binary column's first difference and its standard error from the same two predictions: the cross-covariance
    # a_lo' vcov.est.c a_hi with a = the column means of predict's newdataK, times predict()'s own factor on
    # vcov.est.pred under correct_SE -- sqrt(n / Neffective) (bigkrls_predict, R/bigKRLS.R:610-611), checked here
    lo, hi = preds[3]
    f = 1.0
    if correct_SE:
        plain = bk.predict(out, lo["newdata"], se_pred=True, correct_SE=False)
        f = float(lo["se.pred"][0] ** 2 / plain["se.pred"][0] ** 2)
        assert abs(f - np.sqrt(n / out["Neffective"])) <= 1e-12 * f
    Vc = _host(out["vcov.est.c"])
    a_lo, a_hi = _host(lo["newdataK"]).mean(axis=0), _host(hi["newdataK"]).mean(axis=0)
    var_fd = f * (a_lo @ Vc @ a_lo + a_hi @ Vc @ a_hi - 2.0 * (a_lo @ Vc @ a_hi))
    fd = hi["predicted"].mean() - lo["predicted"].mean()
    ym = float(np.mean(out["y"]))
    pd_scale = np.max(np.abs(np.concatenate(res["pd"]) - ym))
    assert res["first.difference"].shape == (1, 4) and np.all(np.isnan(res["first.difference"][0, :3]))
    assert np.all(np.isnan(res["se.first.difference"][0, :3]))
    assert abs(res["first.difference"][0, 3] - fd) <= 1e-9 * pd_scale
    assert abs(res["se.first.difference"][0, 3] ** 2 - var_fd) <= 1e-8 * var_fd
    assert abs(res["vcov.pd"][3][0, 1] - f * (a_lo @ Vc @ a_hi)) <= 1e-8 * abs(f * (a_lo @ Vc @ a_hi))


def test_single_reference_row_is_predict(fit_small):
    import bigkrls_amd as bk
    out = fit_small
    z = out["X"][[7]] + np.array([[0.3, -0.2, 0.1, 0.0]])
    res = bk.partial_dependence(out, grid=5, newdata=z)
    ym = float(np.mean(out["y"]))
    pd_scale = np.max(np.abs(np.concatenate(res["pd"]) - ym))
    for jj, w in enumerate(res["which"]):
        for g, v in enumerate(res["grid"][jj]):
            zm = z.copy()
            zm[0, w - 1] = v
            pr = bk.predict(out, zm, se_pred=True)
            assert abs(res["pd"][jj][g] - pr["predicted"][0]) <= 1e-9 * pd_scale
            assert abs(res["se.pd"][jj][g] ** 2 - pr["se.pred"][0] ** 2) <= 1e-8 * pr["se.pred"][0] ** 2


def test_without_variance(fit_small):
    import bigkrls_amd as bk
    a = bk.partial_dependence(fit_small, grid=5)
    b = bk.partial_dependence(fit_small, grid=5, se=False)
    assert b["se.pd"] is None and b["vcov.pd"] is None and b["se.first.difference"] is None
    for x, y in zip(a["pd"], b["pd"]):
        assert np.array_equal(x, y)
    again = bk.partial_dependence(fit_small, grid=5)
    for k in ("pd", "se.pd", "vcov.pd"):
        for x, y in zip(a[k], again[k]):
            assert np.array_equal(x, y), k


# ---- factors equal dense ---------------------------------------------------------------------------------------------
def test_factors_equal_dense(fit_small_both):
    import bigkrls_amd as bk
    out = fit_small_both
    d = bk.partial_dependence(out, grid=5, vcov="dense")
    f = bk.partial_dependence(out, grid=5, vcov="factors")
    se_max = max(np.max(s) for s in d["se.pd"])
    cov_max = max(np.max(np.abs(c)) for c in d["vcov.pd"])
    for jj in range(4):
        assert np.array_equal(d["pd"][jj], f["pd"][jj])
        assert np.max(np.abs(d["se.pd"][jj] - f["se.pd"][jj])) <= 1e-9 * se_max
        assert np.max(np.abs(d["vcov.pd"][jj] - f["vcov.pd"][jj])) <= 1e-9 * cov_max
    assert abs(d["se.first.difference"][0, 3] - f["se.first.difference"][0, 3]) <= 1e-9 * se_max


# ---- many binary columns ---------------------------------------------------------------------------------------------
def test_many_binary_columns_against_numpy(fit_binary_p67):
    import bigkrls_amd as bk
    out = fit_binary_p67
    X = out["X"]
    which = [3, 17, 9, 18, 67, 40, 25, 51]              # 3 continuous and 5 binary columns, not in order
    Z = X[:200]
    res = bk.partial_dependence(out, which=which, grid=4, newdata=Z)
    assert list(res["binaryindicator"]) == [False] * 3 + [True] * 5
    for jj, w in enumerate(which):
        x = X[:, w - 1]
        if jj >= 3:
            assert np.array_equal(res["grid"][jj], [x.min(), x.max()])
        else:
            assert np.array_equal(res["grid"][jj], np.linspace(x.min(), x.max(), 4))
    pds, ses, covs = pd_numpy(X, out["y"], out["coeffs"], out["sigma"], which, res["grid"], newdata=Z,
                              vcov_c=_host(out["vcov.est.c"]), neffective=out["Neffective"])
    ym = float(np.mean(out["y"]))
    pd_scale = max(np.max(np.abs(np.concatenate(pds) - ym)), 1e-300)
    se_max = max(np.max(s) for s in ses)
    for jj in range(len(which)):
        assert np.max(np.abs(res["pd"][jj] - pds[jj])) <= 1e-9 * pd_scale, which[jj]
        assert np.max(np.abs(res["se.pd"][jj] - ses[jj])) <= 1e-8 * se_max, which[jj]
        if jj >= 3:
            assert abs(res["first.difference"][0, jj] - (pds[jj][1] - pds[jj][0])) <= 1e-9 * pd_scale
            sefd = np.sqrt(covs[jj][0, 0] + covs[jj][1, 1] - 2.0 * covs[jj][0, 1])
            assert abs(res["se.first.difference"][0, jj] - sefd) <= 1e-8 * se_max


# ---- implicit fit: no stored K is needed -----------------------------------------------------------------------------
def test_implicit_fit_against_predict():
    import bigkrls_amd as bk
    from bigkrls_amd.synth import synth
    X, y = synth(2048, 6, 77)
    out = bk.bigKRLS(y, X, Neig=64, kernel="implicit", vcov_form="factors", noisy=False)
    assert out["K"] is None and out.get("vcov.est.c") is None
    R = X[np.random.default_rng(5).choice(2048, 128, replace=False)]
    res = bk.partial_dependence(out, which=[2, 5], grid=3, newdata=R)
    _brute_force(out, res, R, True)


# ---- the cap on a column's grid --------------------------------------------------------------------------------------
def test_grid_longer_than_the_cap_raises(fit_small):
    import bigkrls_amd as bk
    n = fit_small["X"].shape[0]
    cap = (1 << 30) // (8 * n)
    x = fit_small["X"][:, 0]
    grid = [np.linspace(x.min(), x.max(), cap + 1)]
    with pytest.raises(ValueError, match=rf"grid of column 1 has {cap + 1} values; at most {cap} "):
        bk.partial_dependence(fit_small, which=[1], grid=grid)
