"""Neig="auto": the block Lanczos grows until the spectrum is resolved down to eigtrunc * lambda_1 and returns what a
fit with Neig = lastkeeper + 1 returns.

The counts were computed on the host with numpy (eigvalsh of the host-built kernel, sigma = P, standardised
orc.synth data); the nearest eigenvalue on either side of the threshold is at least 8.8e-6 lambda_1 away from it, far
above the solver's 1e-10 tolerance, so the count is unambiguous:
    synth(2048, 3, 7):  tau = 0.03 -> 17,  tau = 0.001 -> 66
    synth(4500, 6, 52): tau = 0.001 (the n > 3000 default) -> 210
"""
import numpy as np
import pytest

from oracle import krls_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-6          # the file-level tolerance of tests/test_gpu_fit.py and tests/test_gpu_implicit_fit.py
KEYS = ("coeffs", "yfitted", "derivatives", "var.avgderivatives", "vcov.est.w")


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# ---- operator level ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    X, _ = orc.synth(2048, 3, 7)
    Xs = (X - X.mean(0)) / X.std(0, ddof=1)
    sq = (Xs * Xs).sum(1)
    K = np.exp(-np.maximum(sq[:, None] + sq[None, :] - 2.0 * Xs @ Xs.T, 0.0) / 3.0)
    np.fill_diagonal(K, 1.0)
    return Xs, np.linalg.eigvalsh(K)[::-1].copy()


@pytest.mark.parametrize("tau,count", [(0.03, 17), (0.001, 66)])
@pytest.mark.parametrize("form", ["implicit", "stored"])
def test_eigen_auto_finds_the_rank_of_the_host_spectrum(ctx, small, form, tau, count):
    """The bounds of test_eigen_implicit_matches_dense_on_the_stored_kernel, against numpy.linalg.eigvalsh."""
    from bigkrls_amd import ops
    Xs, lam = small
    assert int(np.sum(lam >= tau * lam[0])) == count                              # (the host's own count)
    dXs = ctx.from_numpy(Xs)
    Kd = ops.bGaussKernel(dXs, 3.0) if form == "stored" else None
    e = ops.bEigenAuto(dXs, 3.0, tau, K=Kd)
    print(f"{form} tau={tau}: n_vals {len(e.values)}, lastkeeper {e.lastkeeper}, "
          f"values {np.max(np.abs(e.values - lam[:len(e.values)])) / lam[0]:.3e}")
    assert len(e.values) == count + 1
    assert e.lastkeeper == count
    assert np.max(np.abs(e.values - lam[:count + 1])) <= 1e-11 * lam[0]
    Q = e.vectors.to_numpy()
    assert Q.shape == (2048, count)
    assert np.max(np.abs(Q.T @ Q - np.eye(count))) < 1e-11
    assert e.values[-1] < tau * lam[0]


def test_eigen_auto_refuses_what_it_cannot_do(ctx, small):
    from bigkrls_amd import ops, _lib
    Xs, _ = small
    dXs = ctx.from_numpy(Xs)
    with pytest.raises(_lib.BigKRLSError, match="kcap = 40") as e:                # 66 eigenvalues above the threshold
        ops.bEigenAuto(dXs, 3.0, 0.001, max_pairs=40)
    assert e.value.code == _lib.EINVAL and "keep_thresh" in str(e.value)
    with pytest.raises(_lib.BigKRLSError, match="4 n_vals <= n"):
        ops.bEigenAuto(dXs, 3.0, 0.001, max_pairs=600)
    with pytest.raises(ValueError):
        ops.bEigenAuto(dXs, 3.0, 0.0)


# ---- the fit ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    return orc.synth(4500, 6, 52)


def _fit(ctx, data, **kw):
    import bigkrls_amd as bk
    X, y = data
    return bk.bigKRLS(y, X, vcov_form="factors", ctx=ctx, noisy=False, **kw)


@pytest.fixture(scope="module")
def auto_implicit(ctx, data):
    return _fit(ctx, data, Neig="auto", kernel="implicit")


@pytest.fixture(scope="module")
def auto_stored(ctx, data):
    return _fit(ctx, data, Neig="auto")


@pytest.fixture(scope="module")
def reference(data):
    X, y = data
    return orc.fit(y, X, neig=211, literal=False, return_squares=False)


def assert_twins(auto, fixed, keys=KEYS):
    assert auto["lastkeeper"] == fixed["lastkeeper"]
    assert abs(auto["lambda"] - fixed["lambda"]) <= 1e-8 * abs(fixed["lambda"])
    assert rel(auto["K.eigenvalues"], fixed["K.eigenvalues"]) < 1e-9
    for k in keys:
        err = rel(auto[k], fixed[k])
        print(f"{k}: auto vs Neig=211 {err:.3e}")
        assert err < TOL, k


@pytest.mark.parametrize("kernel", ["implicit", "stored"])
def test_auto_fit_is_the_fit_with_the_rank_given(ctx, data, auto_implicit, auto_stored, reference, kernel):
    auto = auto_implicit if kernel == "implicit" else auto_stored
    assert auto["lastkeeper"] == 210 and len(auto["K.eigenvalues"]) == 211
    assert auto["K.eigenvalues"][-1] < 0.001 * auto["K.eigenvalues"][0] <= auto["K.eigenvalues"][-2]
    assert auto["vcov.est.Q"].to_numpy().shape == (4500, 210)
    assert (auto["K"] is None) == (kernel == "implicit")
    assert_twins(auto, _fit(ctx, data, Neig=211, kernel=kernel))
    assert auto["lastkeeper"] == reference["lastkeeper"]
    assert abs(auto["lambda"] - reference["lambda"]) <= TOL * abs(reference["lambda"])
    assert abs(auto["Neffective"] - reference["Neffective"]) <= TOL * abs(reference["Neffective"])
    for k in ("coeffs", "yfitted", "K.eigenvalues"):
        assert rel(auto[k], reference[k]) < TOL, k


@pytest.mark.parametrize("kernel", ["implicit", "stored"])
def test_two_auto_fits_are_bitwise_equal(ctx, data, auto_implicit, auto_stored, kernel):
    first = auto_implicit if kernel == "implicit" else auto_stored
    again = _fit(ctx, data, Neig="auto", kernel=kernel)
    assert again["lambda"] == first["lambda"] and again["lastkeeper"] == first["lastkeeper"]
    for k in ("K.eigenvalues",) + KEYS:
        assert np.array_equal(again[k], first[k]), k
    assert np.array_equal(again["vcov.est.Q"].to_numpy(), first["vcov.est.Q"].to_numpy())


def test_downstream_of_an_auto_fit(ctx, auto_implicit, tmp_path):
    import os
    import bigkrls_amd as bk
    rng = np.random.default_rng(77)
    Z = rng.standard_normal((301, 6))
    pa = bk.predict(auto_implicit, Z, se_pred=True, matrices=False, ctx=ctx)
    assert np.all(np.isfinite(pa["predicted"])) and np.all(pa["se.pred"] > 0)
    ma = bk.marginal_effects(auto_implicit, Z, ctx=ctx)
    assert ma["derivatives"].shape == (301, 6) and np.all(np.isfinite(ma["var.avgderivatives"]))
    assert bk.summary(auto_implicit, quiet=True)["ttests"].shape == (6, 4)
    folder = bk.save_bigKRLS(auto_implicit, str(tmp_path / "auto_fit"), noisy=False)
    assert "vcov.est.Q.txt" in os.listdir(folder)
    back = bk.load_bigKRLS(folder, noisy=False, ctx=ctx)
    assert back["lastkeeper"] == 210 and np.array_equal(back["K.eigenvalues"], auto_implicit["K.eigenvalues"])
    pb = bk.predict(back, Z, se_pred=True, matrices=False, ctx=ctx)
    assert np.array_equal(pb["predicted"], pa["predicted"]) and np.array_equal(pb["se.pred"], pa["se.pred"])


@pytest.mark.parametrize("kernel", ["implicit", "stored"])
def test_a_cap_below_the_rank_is_an_error_that_names_the_fix(ctx, data, kernel):
    with pytest.raises(ValueError, match="kcap = 100.*raise max_factors.*or pass Neig"):
        _fit(ctx, data, Neig="auto", kernel=kernel, max_factors=100)


def test_crossvalidate_passes_auto_through(ctx):
    import bigkrls_amd as bk
    X, y = orc.synth(9000, 6, 52)                 # two training sets of 4500 rows
    folds = (np.arange(9000) % 2) + 1
    kw = dict(Kfolds=2, folds=folds, ctx=ctx, vcov_form="factors", kernel="implicit", noisy=False)
    auto = bk.crossvalidate(y, X, Neig="auto", **kw)
    k1 = auto["fold_1"]["trained"]["lastkeeper"]
    assert len(auto["fold_1"]["trained"]["K.eigenvalues"]) == k1 + 1
    k2 = auto["fold_2"]["trained"]["lastkeeper"]
    if k1 == k2:                                  # (one Neig serves both folds only then)
        fixed = bk.crossvalidate(y, X, Neig=k1 + 1, **kw)
        for k in ("R2_is", "R2_oos", "MSE_is", "MSE_oos", "R2AME_oos"):
            assert rel(auto[k], fixed[k]) < TOL, k
    assert np.all(np.isfinite(auto["R2_oos"]))


def test_c_abi_fit_auto_and_its_refusals(ctx):
    """bigkrls_fit_auto itself: eigtrunc 0 and a cap outside [1, n / 4] are EINVAL; a good call writes lastkeeper + 1
    values; bigkrls_fit with the same options is the fit it always was."""
    import ctypes as C
    from bigkrls_amd import _lib
    X, y = orc.synth(1200, 3, 2)
    Xh, yh = np.asfortranarray(X), np.ascontiguousarray(y)
    vals = np.zeros(1200)

    def call(neig_max=None, **fields):
        opt, out = _lib.FitOptions(), _lib.FitOutputs()
        opt.struct_bytes, out.struct_bytes = C.sizeof(opt), C.sizeof(out)
        opt.sigma = opt.lambda_ = opt.L = opt.U = opt.eigtrunc = -1.0
        opt.derivative = opt.vcov_est = 0
        for k, v in fields.items():
            setattr(opt, k, v)
        out.eigenvalues = vals.ctypes.data
        head = (ctx.handle, Xh.ctypes.data, yh.ctypes.data, 1200, 3, C.byref(opt))
        if neig_max is None:
            _lib.call("bigkrls_fit", *head, C.byref(out))
        else:
            _lib.call("bigkrls_fit_auto", *head, neig_max, C.byref(out))
        return out
    for neig_max, fields, needle in [(200, dict(), "pass eigtrunc"), (200, dict(eigtrunc=0.0), "pass eigtrunc"),
                                     (301, dict(eigtrunc=0.01), "neig_max <= n / 4"),
                                     (0, dict(eigtrunc=0.01), "neig_max <= n / 4")]:
        with pytest.raises(_lib.BigKRLSError, match=needle) as e:
            call(neig_max, **fields)
        assert e.value.code == _lib.EINVAL
    out = call(300, eigtrunc=0.01, neig=7)                                        # (neig is ignored)
    assert out.neig == out.lastkeeper + 1 and 1 <= out.lastkeeper < 300
    assert vals[out.neig - 1] < 0.01 * vals[0] <= vals[out.neig - 2]
    assert call(neig=50).neig == 50
