"""marginal_effects(se=True) on the GPU: the pointwise standard errors against the numpy restatement of their definition
(tests/test_marginal_effects_se_cpu.py) from both forms of vcov.est.c, the single-point identity with
var.avgderivatives, block boundaries, and the properties a caller relies on (finite, non-negative, repeatable, nothing
else in the result changed)."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import krls_oracle as orc

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_me_se_cpu", os.path.join(_HERE, "test_marginal_effects_se_cpu.py"))
_me_se_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_me_se_cpu)
me_se_numpy = _me_se_cpu.me_se_numpy


@pytest.fixture(scope="module")
def fit_small(ctx):
    import bigkrls_amd as bk
    X, y = orc.synth(300, 4, 21, binary_last=True)
    return bk.bigKRLS(y, X, vcov_form="both", ctx=ctx, noisy=False)


@pytest.fixture(scope="module")
def fit_three_binary(ctx):
    """P = 6 with three binary columns (different pairs of values), not next to each other"""
    import bigkrls_amd as bk
    rng = np.random.default_rng(66)
    n = 300
    X = rng.standard_normal((n, 6))
    X[:, 0] = (rng.random(n) < 0.3).astype(np.float64)
    X[:, 3] = np.where(rng.random(n) < 0.6, 2.0, -1.5)
    X[:, 5] = np.where(rng.random(n) < 0.5, 10.0, 11.0)
    y = np.sin(X @ np.linspace(0.2, 0.7, 6)) + 0.25 * rng.standard_normal(n)
    return bk.bigKRLS(y, X, vcov_form="both", ctx=ctx, noisy=False)


def draw(out, u, seed):
    """u out-of-sample points: normal in the continuous columns, one of the two training values in the binary ones"""
    X = np.asarray(out["X"])
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((u, X.shape[1]))
    for j in range(X.shape[1]):
        vals = np.unique(X[:, j])
        if vals.size == 2:
            Z[:, j] = rng.choice(vals, size=u)
    return Z


def vcov_matrix(out):
    V = out["vcov.est.c"]
    return V.to_numpy() if hasattr(V, "to_numpy") else np.asarray(V)


def check_against_numpy(out, Z, which=None):
    """se^2 from both forms against the restatement and against each other, each within 1e-8 max(se^2): the bound
    var.avgderivatives is held to against the same restatement (tests/test_gpu_marginal_effects.py)."""
    import bigkrls_amd as bk
    ref = me_se_numpy(out["X"], out["y"], out["coeffs"], out["sigma"], Z, vcov_matrix(out), which=which) ** 2
    tol = 1e-8 * max(ref.max(), 1e-300) + 1e-300
    got = {}
    for form in ("factors", "dense"):
        me = bk.marginal_effects(out, Z, which_derivatives=which, vcov=form, se=True)
        se = me["se.derivatives"]
        assert se.shape == me["derivatives"].shape == ref.shape
        assert np.all(np.isfinite(se)) and np.all(se >= 0.0)
        err = np.max(np.abs(se ** 2 - ref))
        print(f"u={Z.shape[0]} which={which} {form}: max |se^2 - ref| = {err:.3e}, bound {tol:.3e}")
        assert err <= tol, form
        got[form] = se ** 2
    err = np.max(np.abs(got["factors"] - got["dense"]))
    print(f"u={Z.shape[0]} which={which} factors vs dense: {err:.3e}, bound {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("u,which", [(1, None), (37, [3, 4, 1]), (300, None), (37, [4, 2])])
def test_against_the_numpy_restatement(fit_small, u, which):
    check_against_numpy(fit_small, draw(fit_small, u, 100 + u), which)


@pytest.mark.parametrize("u,which", [(1, None), (37, [6, 2, 4, 1]), (300, None)])
def test_against_the_numpy_restatement_three_binary_columns(fit_three_binary, u, which):
    check_against_numpy(fit_three_binary, draw(fit_three_binary, u, 200 + u), which)


@pytest.mark.parametrize("form", ["factors", "dense"])
def test_single_point_se_squared_is_var_avgderivatives(fit_small, fit_three_binary, form):
    import bigkrls_amd as bk
    for out in (fit_small, fit_three_binary):
        for seed in (1, 2, 3):                 # both groups of the binary columns turn up
            me = bk.marginal_effects(out, draw(out, 1, seed), vcov=form, se=True)
            assert any(me["binaryindicator"]) and not all(me["binaryindicator"])
            np.testing.assert_allclose(me["se.derivatives"][0] ** 2, me["var.avgderivatives"][0], rtol=1e-10, atol=0)


@pytest.mark.parametrize("form", ["factors", "dense"])
def test_block_boundaries(fit_small, form):
    """u = 300 in blocks of 128 rows (three blocks, the last one partial) is bitwise the single automatic block"""
    import bigkrls_amd as bk
    Z = draw(fit_small, 300, 5)
    whole = bk.marginal_effects(fit_small, Z, vcov=form, se=True)["se.derivatives"]
    blocked = bk.marginal_effects(fit_small, Z, vcov=form, se=True, _block_rows=128)["se.derivatives"]
    assert np.array_equal(whole, blocked)
    assert whole.max() > 0.0


def test_block_rows_must_be_a_multiple_of_128(fit_small, ctx):
    """the C entry returns BIGKRLS_EINVAL, which the Python API hands on as the ValueError of every validation error"""
    import bigkrls_amd as bk
    from bigkrls_amd import _lib
    out = fit_small
    with pytest.raises(ValueError, match="multiple of 128"):
        bk.marginal_effects(out, draw(out, 5, 1), se=True, _block_rows=100)
    X = np.asfortranarray(np.asarray(out["X"], dtype=np.float64))
    n, p = X.shape
    y = np.ascontiguousarray(out["y"], dtype=np.float64).ravel()
    c = np.ascontiguousarray(out["coeffs"], dtype=np.float64).ravel()
    w = np.ascontiguousarray(out["vcov.est.w"], dtype=np.float64).ravel()
    Z = np.asfortranarray(draw(out, 5, 1))
    se = np.full((5, p), -7.0, order="F")
    Q = out["vcov.est.Q"]
    Qd = Q if hasattr(Q, "ptr") else ctx.from_numpy(np.asarray(Q))
    for block_rows in (100, -128, 129):
        with pytest.raises(_lib.BigKRLSError, match="multiple of 128") as e:
            _lib.call("bigkrls_marginal_effects_se", ctx.handle, X.ctypes.data, n, p, y.ctypes.data, c.ctypes.data,
                      float(out["sigma"]), None, 0, Z.ctypes.data, 5, None, Qd.ptr, Qd.ld, Qd.ncol, w.ctypes.data,
                      block_rows, se.ctypes.data)
        assert e.value.code == _lib.EINVAL
    assert np.all(se == -7.0)                        # refused before anything was written


@pytest.mark.parametrize("form", ["factors", "dense"])
def test_far_newdata_gives_zero(fit_small, form):
    import bigkrls_amd as bk
    X = fit_small["X"]
    Z = draw(fit_small, 19, 9)
    Z[4, :3] = 1e3                                   # one far row among ordinary ones
    me = bk.marginal_effects(fit_small, Z, vcov=form, se=True)
    se = me["se.derivatives"]
    assert np.all(np.isfinite(se)) and np.all(se >= 0.0)
    assert np.all(se[4] == 0.0) and np.all(me["derivatives"][4] == 0.0)
    assert np.all(se[[0, 1, 2, 3, 5]] > 0.0)
    Z = np.full((7, X.shape[1]), 1e3)                # all rows far
    Z[:, -1] = X[:, -1].max()
    assert np.all(bk.marginal_effects(fit_small, Z, vcov=form, se=True)["se.derivatives"] == 0.0)


@pytest.mark.parametrize("form", [None, "factors", "dense"])
def test_repeatable_and_the_rest_of_the_result_is_unchanged(fit_small, form):
    import bigkrls_amd as bk
    Z = draw(fit_small, 200, 4)
    plain = bk.marginal_effects(fit_small, Z, vcov=form)
    assert "se.derivatives" not in plain
    a = bk.marginal_effects(fit_small, Z, vcov=form, se=True)
    b = bk.marginal_effects(fit_small, Z, vcov=form, se=True)
    assert set(a) == set(plain) | {"se.derivatives"}
    assert np.array_equal(a["se.derivatives"], b["se.derivatives"])
    for k in ("derivatives", "avgderivatives", "var.avgderivatives"):
        assert np.array_equal(a[k], plain[k]), k
    if form is None:                                 # the matrix is preferred, for the variances and the SEs alike
        dense = bk.marginal_effects(fit_small, Z, vcov="dense", se=True)
        assert np.array_equal(a["se.derivatives"], dense["se.derivatives"])


def test_object_without_vcov_raises(fit_small):
    import bigkrls_amd as bk
    from bigkrls_amd.api import BigKRLS
    obj = BigKRLS(fit_small)
    obj["vcov.est.c"] = obj["vcov.est.Q"] = obj["vcov.est.w"] = None
    with pytest.raises(ValueError, match="recompute bigKRLS object"):
        bk.marginal_effects(obj, fit_small["X"][:3], se=True)


def test_c_entry_wants_exactly_one_form(fit_small, ctx):
    from bigkrls_amd import _lib
    out = fit_small
    X = np.asfortranarray(np.asarray(out["X"], dtype=np.float64))
    n, p = X.shape
    y = np.ascontiguousarray(out["y"], dtype=np.float64).ravel()
    c = np.ascontiguousarray(out["coeffs"], dtype=np.float64).ravel()
    w = np.ascontiguousarray(out["vcov.est.w"], dtype=np.float64).ravel()
    Z = np.asfortranarray(draw(out, 3, 1))
    se = np.empty((3, p), order="F")
    V, Q = out["vcov.est.c"], out["vcov.est.Q"]
    Vd = V if hasattr(V, "ptr") else ctx.from_numpy(np.asarray(V))
    Qd = Q if hasattr(Q, "ptr") else ctx.from_numpy(np.asarray(Q))
    for vptr, qptr in ((Vd.ptr, Qd.ptr), (None, None)):
        with pytest.raises(_lib.BigKRLSError, match="exactly one"):
            _lib.call("bigkrls_marginal_effects_se", ctx.handle, X.ctypes.data, n, p, y.ctypes.data, c.ctypes.data,
                      float(out["sigma"]), None, 0, Z.ctypes.data, 3, vptr, qptr, Qd.ld, Qd.ncol, w.ctypes.data, 0,
                      se.ctypes.data)


def test_implicit_fit(ctx):
    """kernel="implicit" at the smallest size the mode accepts (N = 1024): se=True works from its factors and matches
    the stored twin's within the tolerance tests/test_gpu_implicit_fit.py holds twins to (1e-6)."""
    import bigkrls_amd as bk
    X, y = orc.synth(1024, 4, 52, binary_last=True)
    kw = dict(Neig=96, vcov_form="factors", ctx=ctx, noisy=False)
    sto = bk.bigKRLS(y, X, **kw)
    imp = bk.bigKRLS(y, X, kernel="implicit", **kw)
    assert imp["K"] is None and imp["vcov.est.c"] is None
    Z = draw(sto, 150, 8)
    a = bk.marginal_effects(imp, Z, se=True)
    b = bk.marginal_effects(sto, Z, se=True)
    assert a["se.derivatives"].shape == (150, 4) and np.all(a["se.derivatives"] > 0.0)
    err = float(np.max(np.abs(a["se.derivatives"] - b["se.derivatives"])) / np.max(np.abs(b["se.derivatives"])))
    print(f"implicit vs stored se.derivatives: {err:.3e}")
    assert err < 1e-6
