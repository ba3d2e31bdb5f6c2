"""bigKRLS(kernel="implicit"): the fit that never stores the N x N kernel matrix, against the stored fit with the same
arguments and against the CPU oracle. The shapes are ones that other tests already force through the block Lanczos
and see converge: orc.synth(4500, 6, 52) with Neig = 96 (test_gpu_fit.py) and (4608, 6, Neig 128, eigtrunc 0)
(test_gpu_level1.py)."""
import numpy as np
import pytest

from oracle import krls_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-6          # the file-level tolerance of tests/test_gpu_fit.py


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def assert_twins(imp, sto, keys):
    assert imp["K"] is None and imp["kernel"] == "implicit"
    assert imp["lastkeeper"] == sto["lastkeeper"]
    assert abs(imp["lambda"] - sto["lambda"]) <= 1e-8 * abs(sto["lambda"])
    assert rel(imp["K.eigenvalues"], sto["K.eigenvalues"]) < 1e-9
    for k in keys:
        err = rel(imp[k], sto[k])
        print(f"{k}: implicit vs stored {err:.3e}")
        assert err < TOL, k


@pytest.fixture(scope="module")
def data():
    return orc.synth(4500, 6, 52)


@pytest.fixture(scope="module")
def stored(ctx, data):
    import bigkrls_amd as bk
    X, y = data
    return bk.bigKRLS(y, X, Neig=96, vcov_form="factors", ctx=ctx, noisy=False)


@pytest.fixture(scope="module")
def implicit(ctx, data):
    import bigkrls_amd as bk
    X, y = data
    return bk.bigKRLS(y, X, Neig=96, kernel="implicit", vcov_form="factors", ctx=ctx, noisy=False)


def test_eigen_implicit_matches_dense_on_the_stored_kernel(monkeypatch):
    """ops.bEigenImplicit against ops.bEigen (dense path) on the stored kernel: the bounds of
    test_eigen_block_lanczos_matches_dense_and_arpack."""
    import bigkrls_amd as bk
    from bigkrls_amd import ops
    ctx = bk.Context(0)
    n, p, neig, trunc = 4608, 6, 128, 0.0
    X, y = orc.synth(n, p, 31)
    Xs = (X - X.mean(0)) / X.std(0, ddof=1)
    dXs = ctx.from_numpy(Xs)
    K = ops.bGaussKernel(dXs, float(p))
    monkeypatch.setenv("BIGKRLS_EIGK", "dense")
    d = ops.bEigen(K, neig, trunc)
    a = ops.bEigenImplicit(dXs, float(p), neig, trunc)
    assert a.lastkeeper == d.lastkeeper
    assert np.max(np.abs(a.values - d.values)) <= 1e-11 * d.values[0]
    Qa, Qd = a.vectors.to_numpy(), d.vectors.to_numpy()
    assert np.max(np.abs(Qa.T @ Qa - np.eye(Qa.shape[1]))) < 1e-11
    ys = (y - y.mean()) / y.std(ddof=1)
    w = 1.0 / (d.values[:d.lastkeeper] + 0.5)
    cd, ca = Qd @ (w * (Qd.T @ ys)), Qa @ (w * (Qa.T @ ys))       # rotation/sign invariant
    assert np.max(np.abs(cd - ca)) <= 1e-8 * np.max(np.abs(cd))


def test_eigen_implicit_refuses_what_the_block_lanczos_cannot_do(ctx):
    from bigkrls_amd import ops, _lib
    rng = np.random.default_rng(1)
    with pytest.raises(_lib.BigKRLSError, match="n >= 1024 and 4 n_vals <= n"):
        ops.bEigenImplicit(ctx.from_numpy(rng.standard_normal((600, 3))), 3.0, 50)
    with pytest.raises(_lib.BigKRLSError, match="n >= 1024 and 4 n_vals <= n"):
        ops.bEigenImplicit(ctx.from_numpy(rng.standard_normal((1200, 3))), 3.0, 301)


def test_implicit_fit_matches_the_stored_fit(implicit, stored):
    assert stored["K"] is not None and "kernel" not in stored
    assert_twins(implicit, stored, ("coeffs", "yfitted", "derivatives", "var.avgderivatives", "vcov.est.w"))
    assert implicit["vcov.est.c"] is None and implicit["vcov.est.fitted"] is None
    assert implicit["vcov.est.Q"].to_numpy().shape == (4500, implicit["lastkeeper"])
    assert implicit["has.big.matrices"] == stored["has.big.matrices"]


def test_implicit_fit_matches_the_oracle(implicit, data):
    X, y = data
    ref = orc.fit(y, X, neig=96, literal=False, return_squares=False)
    assert implicit["lastkeeper"] == ref["lastkeeper"]
    assert abs(implicit["lambda"] - ref["lambda"]) <= TOL * abs(ref["lambda"])
    for k in ("coeffs", "yfitted"):
        assert rel(implicit[k], ref[k]) < TOL, k


@pytest.mark.parametrize("variant", ["binary", "which", "no_derivative", "lambda"])
def test_implicit_variants_match_their_stored_twins(ctx, data, variant):
    import bigkrls_amd as bk
    X, y = data
    kw = dict(Neig=96, vcov_form="factors", ctx=ctx, noisy=False)
    keys = ("coeffs", "yfitted", "derivatives", "var.avgderivatives", "vcov.est.w")
    if variant == "binary":
        X, y = orc.synth(4500, 6, 52, binary_last=True)
    elif variant == "which":
        kw["which_derivatives"] = [2, 5]
    elif variant == "no_derivative":
        kw.update(derivative=False, vcov_est=False, vcov_form="dense")
        keys = ("coeffs", "yfitted")
    else:
        kw["lambda_"] = 0.37
    sto = bk.bigKRLS(y, X, **kw)
    imp = bk.bigKRLS(y, X, kernel="implicit", **kw)
    assert_twins(imp, sto, keys)
    if variant == "binary":
        assert imp["binaryindicator"][-1] and np.array_equal(imp["binaryindicator"], sto["binaryindicator"])
    if variant == "which":
        assert imp["derivatives"].shape == (4500, 2)
    if variant == "lambda":
        assert imp["lambda"] == 0.37


def test_downstream_of_an_implicit_fit(ctx, implicit, stored, tmp_path):
    import bigkrls_amd as bk
    rng = np.random.default_rng(77)
    Z = rng.standard_normal((301, 6))
    pi = bk.predict(implicit, Z, se_pred=True, matrices=False, ctx=ctx)
    ps = bk.predict(stored, Z, se_pred=True, matrices=False, ctx=ctx)
    assert rel(pi["predicted"], ps["predicted"]) < TOL
    assert rel(pi["se.pred"], ps["se.pred"]) < TOL
    mi, ms = bk.marginal_effects(implicit, Z, ctx=ctx), bk.marginal_effects(stored, Z, ctx=ctx)
    for k in ("derivatives", "avgderivatives", "var.avgderivatives"):
        assert rel(mi[k], ms[k]) < TOL, k
    s = bk.summary(implicit, quiet=True)
    assert s["ttests"].shape == (6, 4)
    folder = bk.save_bigKRLS(implicit, str(tmp_path / "implicit_fit"), noisy=False)
    import os
    assert "K.txt" not in os.listdir(folder) and "vcov.est.Q.txt" in os.listdir(folder)
    back = bk.load_bigKRLS(folder, noisy=False, ctx=ctx)
    assert "K" in back and back["K"] is None and back["kernel"] == "implicit"
    assert np.array_equal(back["coeffs"], implicit["coeffs"])
    assert np.array_equal(back["vcov.est.Q"].to_numpy(), implicit["vcov.est.Q"].to_numpy())
    pb = bk.predict(back, Z, se_pred=True, matrices=False, ctx=ctx)
    assert np.array_equal(pb["predicted"], pi["predicted"]) and np.array_equal(pb["se.pred"], pi["se.pred"])


def test_crossvalidate_implicit(ctx):
    import bigkrls_amd as bk
    X, y = orc.synth(9000, 6, 52)                 # two training sets of 4500 rows: the shape of the fits above
    folds = (np.arange(9000) % 2) + 1
    kw = dict(Kfolds=2, folds=folds, ctx=ctx, Neig=96, vcov_form="factors", noisy=False)
    sto = bk.crossvalidate(y, X, **kw)
    imp = bk.crossvalidate(y, X, kernel="implicit", **kw)
    assert imp["fold_1"]["trained"]["K"] is None
    for k in ("R2_is", "R2_oos", "MSE_is", "MSE_oos", "R2AME_oos"):
        assert rel(imp[k], sto[k]) < TOL, k


def test_two_implicit_fits_are_bitwise_equal(ctx, data, implicit):
    import bigkrls_amd as bk
    X, y = data
    again = bk.bigKRLS(y, X, Neig=96, kernel="implicit", vcov_form="factors", ctx=ctx, noisy=False)
    assert again["lambda"] == implicit["lambda"]
    for k in ("K.eigenvalues", "coeffs", "yfitted", "derivatives", "var.avgderivatives", "vcov.est.w"):
        assert np.array_equal(again[k], implicit[k]), k
    assert np.array_equal(again["vcov.est.Q"].to_numpy(), implicit["vcov.est.Q"].to_numpy())


def test_implicit_fit_holds_less_than_one_kernel_matrix(ctx):
    """N = 17 000, P = 10, Neig = 60: K alone would be 8 N^2 = 2.3 GB. The bound is the feature's definition; the
    Lanczos basis (17 000 x 4 096 doubles, 0.56 GB) is the largest buffer of the fit."""
    import torch
    import bigkrls_amd as bk
    n = 17000
    X, y = orc.synth(n, 10, 3)
    ctx.release_workspace()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    out = bk.bigKRLS(y, X, Neig=60, kernel="implicit", vcov_form="factors", ctx=ctx, noisy=False)
    torch.cuda.synchronize()
    assert out["K"] is None and out["lastkeeper"] > 0 and np.all(np.isfinite(out["coeffs"]))
    print(f"workspace {ctx.workspace_bytes() / 1e9:.3f} GB, torch peak delta "
          f"{(torch.cuda.max_memory_allocated() - base) / 1e9:.3f} GB, one K {8 * n * n / 1e9:.3f} GB")
    assert ctx.workspace_bytes() < 8 * n * n
    assert torch.cuda.max_memory_allocated() - base < 8 * n * n


@pytest.mark.parametrize("n,kwargs", [
    (1200, dict(vcov_form="factors")),
    (1200, dict(Neig=301, vcov_form="factors")),
    (600, dict(Neig=96, vcov_form="factors")),
    (1200, dict(Neig=96, vcov_form="dense")),
    (1200, dict(Neig=96, vcov_form="factors", kernel="other")),
])
def test_implicit_value_errors(ctx, n, kwargs):
    import bigkrls_amd as bk
    X, y = orc.synth(n, 3, 2)
    kwargs.setdefault("kernel", "implicit")
    with pytest.raises(ValueError):
        bk.bigKRLS(y, X, ctx=ctx, **kwargs)


def test_implicit_refuses_a_communicator(ctx):
    import bigkrls_amd as bk
    X, y = orc.synth(1200, 3, 2)
    comm = type("Comm", (), {"ctx": ctx, "handle": None})()
    with pytest.raises(ValueError, match="comm"):
        bk.bigKRLS(y, X, Neig=96, kernel="implicit", vcov_form="factors", comm=comm)


def test_c_abi_refuses_outputs_an_implicit_fit_cannot_give(ctx):
    """bigkrls_fit itself (not only the Python layer): d_K, an unset neig and an unknown kernel_form are EINVAL."""
    import ctypes as C
    from bigkrls_amd import _lib
    X, y = orc.synth(1200, 3, 2)
    Xh, yh = np.asfortranarray(X), np.ascontiguousarray(y)
    K = ctx.empty(1200, 1200)
    for form, neig, dk, needle in [(1, 96, K.ptr, "d_K must be NULL"), (1, 0, None, "needs neig"),
                                   (1, 400, None, "4 neig <= n"), (2, 96, None, "kernel_form must be")]:
        opt, out = _lib.FitOptions(), _lib.FitOutputs()
        opt.struct_bytes, out.struct_bytes = C.sizeof(opt), C.sizeof(out)
        opt.sigma = opt.lambda_ = opt.L = opt.U = opt.eigtrunc = -1.0
        opt.neig, opt.kernel_form = neig, form
        if dk is not None:
            out.d_K = dk
        with pytest.raises(_lib.BigKRLSError, match=needle) as e:
            _lib.call("bigkrls_fit", ctx.handle, Xh.ctypes.data, yh.ctypes.data, 1200, 3, C.byref(opt), C.byref(out))
        assert e.value.code == _lib.EINVAL
