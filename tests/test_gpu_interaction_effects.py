"""interaction_effects() on the GPU: values, averages, variances of the averages and pointwise standard errors against
the numpy restatement of their definition (tests/test_interaction_effects_cpu.py) from both forms of vcov.est.c, against
differences of marginal_effects() itself, the single-point identity, block boundaries, and the properties a caller
relies on (finite, repeatable, nothing else in the result changed, robust and implicit objects work unchanged)."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import krls_oracle as orc

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_ie_cpu", os.path.join(_HERE, "test_interaction_effects_cpu.py"))
_ie_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ie_cpu)
ie_numpy, default_pairs = _ie_cpu.ie_numpy, _ie_cpu.default_pairs


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


@pytest.fixture(scope="module")
def fits(fit_small, fit_three_binary):
    return {"small": fit_small, "three_binary": fit_three_binary}


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


_refs = {}


def reference(fits, name, u):
    """(Z, pairs, ie_numpy's results over all default pairs), computed once per fit and u and never changed"""
    if (name, u) not in _refs:
        out = fits[name]
        Z = draw(out, u, 300 + u)
        ref = ie_numpy(out["X"], out["y"], out["coeffs"], out["sigma"], Z, vcov_matrix(out))
        for a in ref:
            a.setflags(write=False)
        _refs[(name, u)] = (Z, default_pairs(np.asarray(out["X"])), ref)
    return _refs[(name, u)]


def close(got, ref, rel, what):
    tol = rel * max(float(np.max(np.abs(ref))), 1e-300)
    err = float(np.max(np.abs(np.asarray(got) - ref)))
    print(f"{what}: max |got - ref| = {err:.3e}, bound {tol:.3e}")
    assert err <= tol, what


@pytest.mark.parametrize("name", ["small", "three_binary"])
@pytest.mark.parametrize("u", [1, 37, 300])
def test_against_the_numpy_restatement(fits, name, u):
    """values and averages within 1e-10 max|ref|, var and se^2 within 1e-8 max|ref| from both forms and between them:
    the bounds the first-order tests hold against their restatement. All default pairs, and a shuffled explicit subset
    (some pairs given as (k, j)) whose columns must be the matching ones of the full result's reference."""
    import bigkrls_amd as bk
    out = fits[name]
    Z, pairs, (vals, avg, var, se) = reference(fits, name, u)
    rng = np.random.default_rng(u)
    pick = rng.permutation(len(pairs))[:max(3, len(pairs) // 2)]
    subset = [pairs[i] if rng.random() < 0.5 else pairs[i][::-1] for i in pick]
    for label, arg, sel in (("all", None, np.arange(len(pairs))), ("subset", subset, pick)):
        got = {}
        for form in ("factors", "dense"):
            ie = bk.interaction_effects(out, Z, pairs=arg, vcov=form, se=True)
            assert ie["pairs"] == [pairs[i] for i in sel]
            assert ie["interactions"].shape == ie["se.interactions"].shape == (u, len(sel))
            assert np.all(np.isfinite(ie["se.interactions"])) and np.all(ie["se.interactions"] >= 0.0)
            tag = f"{name} u={u} {label} {form}"
            close(ie["interactions"], vals[:, sel], 1e-10, tag + " interactions")
            close(ie["avginteractions"][0], avg[sel], 1e-10, tag + " avginteractions")
            close(ie["var.avginteractions"][0], var[sel], 1e-8, tag + " var.avginteractions")
            close(ie["se.interactions"] ** 2, se[:, sel] ** 2, 1e-8, tag + " se.interactions^2")
            got[form] = ie
        tag = f"{name} u={u} {label} factors vs dense"
        close(got["factors"]["var.avginteractions"], got["dense"]["var.avginteractions"], 1e-8, tag + " var")
        close(got["factors"]["se.interactions"] ** 2, got["dense"]["se.interactions"] ** 2, 1e-8, tag + " se^2")
        assert np.array_equal(got["factors"]["interactions"], got["dense"]["interactions"])


@pytest.mark.parametrize("name", ["small", "three_binary"])
def test_against_differences_of_marginal_effects(fits, name):
    """Every default pair, in both orders: operator k applied to marginal_effects()["derivatives"][:, j]. Continuous k:
    central differences in raw column k with h = 1e-4 sd(x_k), within 1e-6 of the largest interaction; binary k: the
    difference between newdata with column k at its two values over their gap, within 1e-10."""
    import bigkrls_amd as bk
    out = fits[name]
    X = np.asarray(out["X"])
    p = X.shape[1]
    Z = draw(out, 37, 77)
    ie = bk.interaction_effects(out, Z)
    vals = ie["interactions"]
    top = np.abs(vals).max()
    applied = {}                                             # column k -> (operator k on every first-order effect, bound)
    for k in range(p):
        Zp, Zm = Z.copy(), Z.copy()
        if np.unique(X[:, k]).size == 2:
            Zp[:, k], Zm[:, k] = X[:, k].max(), X[:, k].min()
            step, bound = X[:, k].max() - X[:, k].min(), 1e-10
        else:
            h = 1e-4 * X[:, k].std(ddof=1)
            Zp[:, k] += h
            Zm[:, k] -= h
            step, bound = 2.0 * h, 1e-6
        Dp = bk.marginal_effects(out, Zp, which_derivatives=list(range(1, p + 1)))["derivatives"]
        Dm = bk.marginal_effects(out, Zm, which_derivatives=list(range(1, p + 1)))["derivatives"]
        applied[k] = ((Dp - Dm) / step, bound)
    assert len(ie["pairs"]) == p * (p + 1) // 2 - int(sum(np.unique(X[:, j]).size == 2 for j in range(p)))
    worst = {1e-6: 0.0, 1e-10: 0.0}
    for i, (j1, k1) in enumerate(ie["pairs"]):
        for a, b in {(j1 - 1, k1 - 1), (k1 - 1, j1 - 1)}:
            diff, bound = applied[b]
            err = float(np.abs(diff[:, a] - vals[:, i]).max() / top)
            worst[bound] = max(worst[bound], err)
            assert err <= bound, (name, a + 1, b + 1, err, bound)
    print(f"{name}: worst error relative to the largest interaction, by bound: {worst}")


@pytest.mark.parametrize("form", ["factors", "dense"])
def test_single_point_se_squared_is_var_avginteractions(fits, form):
    import bigkrls_amd as bk
    for out in fits.values():
        X = np.asarray(out["X"])
        hit = {j: set() for j in range(X.shape[1]) if np.unique(X[:, j]).size == 2}
        for seed in (1, 2, 3, 4, 5, 6):
            Z = draw(out, 1, seed)
            for j in hit:
                hit[j].add(float(Z[0, j]))
            ie = bk.interaction_effects(out, Z, vcov=form, se=True)
            np.testing.assert_allclose(ie["se.interactions"][0] ** 2, ie["var.avginteractions"][0], rtol=1e-10, atol=0)
        assert all(len(v) == 2 for v in hit.values()), "the seeds must hit both groups of every binary column"


@pytest.mark.parametrize("form", ["factors", "dense"])
def test_block_boundaries(fit_small, form):
    """u = 300 in blocks of 128 rows (128, 128, 44) is bitwise the single automatic block: n < 1024, one k split"""
    import bigkrls_amd as bk
    Z = draw(fit_small, 300, 5)
    whole = bk.interaction_effects(fit_small, Z, vcov=form, se=True)["se.interactions"]
    blocked = bk.interaction_effects(fit_small, Z, vcov=form, se=True, _block_rows=128)["se.interactions"]
    assert np.array_equal(whole, blocked)
    assert whole.max() > 0.0


def test_block_rows_must_be_a_multiple_of_128(fit_small):
    import bigkrls_amd as bk
    for bad in (100, 129, -128):
        with pytest.raises(ValueError, match="multiple of 128"):
            bk.interaction_effects(fit_small, draw(fit_small, 5, 1), se=True, _block_rows=bad)


def test_newdata_none_is_the_training_rows(fit_small):
    import bigkrls_amd as bk
    a = bk.interaction_effects(fit_small, se=True)
    b = bk.interaction_effects(fit_small, np.asarray(fit_small["X"]), se=True)
    for k in ("interactions", "avginteractions", "var.avginteractions", "se.interactions"):
        assert np.array_equal(a[k], b[k]), k
    assert a["interactions"].shape[0] == 300


@pytest.mark.parametrize("form", ["factors", "dense"])
def test_far_newdata_gives_finite_zeros(fit_small, form):
    """all continuous columns at +40 sd: the kernel underflows, nothing may turn into NaN or Inf"""
    import bigkrls_amd as bk
    X = np.asarray(fit_small["X"])
    Z = np.tile(X.mean(axis=0) + 40.0 * X.std(axis=0, ddof=1), (7, 1))
    Z[:, -1] = X[:, -1].max()
    ie = bk.interaction_effects(fit_small, Z, vcov=form, se=True)
    for k in ("interactions", "avginteractions", "var.avginteractions", "se.interactions"):
        assert np.all(np.isfinite(ie[k])) and np.all(ie[k] == 0.0), k


@pytest.mark.parametrize("form", [None, "factors", "dense"])
def test_repeatable_and_the_rest_of_the_result_is_unchanged(fit_small, form):
    import bigkrls_amd as bk
    Z = draw(fit_small, 200, 4)
    plain = bk.interaction_effects(fit_small, Z, vcov=form)
    assert "se.interactions" not in plain
    assert set(plain) == {"interactions", "avginteractions", "var.avginteractions", "pairs", "pairlabs",
                          "binaryindicator", "newdata"}
    a = bk.interaction_effects(fit_small, Z, vcov=form, se=True)
    b = bk.interaction_effects(fit_small, Z, vcov=form, se=True)
    assert set(a) == set(plain) | {"se.interactions"}
    for k in ("interactions", "avginteractions", "var.avginteractions", "se.interactions"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("interactions", "avginteractions", "var.avginteractions"):
        assert np.array_equal(a[k], plain[k]), k
    assert a["pairs"] == plain["pairs"] and a["pairlabs"] == plain["pairlabs"]
    assert np.array_equal(a["binaryindicator"], plain["binaryindicator"])


def test_robust_object(fit_small):
    import bigkrls_amd as bk
    rob = bk.robust_vcov(fit_small, "HC1")
    Z = draw(fit_small, 50, 12)
    a = bk.interaction_effects(fit_small, Z, vcov="factors", se=True)
    b = bk.interaction_effects(rob, Z, se=True)
    assert np.array_equal(a["interactions"], b["interactions"])
    assert np.array_equal(a["avginteractions"], b["avginteractions"])
    for k in ("var.avginteractions", "se.interactions"):
        assert np.all(np.isfinite(b[k])) and np.all(b[k] >= 0.0), k
        assert not np.array_equal(a[k], b[k]), k


def test_implicit_fit(ctx):
    """kernel="implicit" at the smallest size the mode accepts (N = 1024) against its stored twin, to the 1e-6
    tests/test_gpu_implicit_fit.py holds twins to"""
    import bigkrls_amd as bk
    X, y = orc.synth(1024, 4, 52, binary_last=True)
    kw = dict(Neig=64, vcov_form="factors", ctx=ctx, noisy=False)
    sto = bk.bigKRLS(y, X, **kw)
    imp = bk.bigKRLS(y, X, kernel="implicit", **kw)
    assert imp["K"] is None and imp["vcov.est.c"] is None
    Z = draw(sto, 150, 8)
    a = bk.interaction_effects(imp, Z, se=True)
    b = bk.interaction_effects(sto, Z, se=True)
    assert a["se.interactions"].shape == (150, 9) and np.all(a["se.interactions"] > 0.0)
    for k in ("interactions", "avginteractions", "var.avginteractions", "se.interactions"):
        err = float(np.max(np.abs(a[k] - b[k])) / np.max(np.abs(b[k])))
        print(f"implicit vs stored {k}: {err:.3e}")
        assert err < 1e-6, k


def test_c_entry_refusals(fit_small, ctx):
    from bigkrls_amd import _lib
    out = fit_small
    X = np.asfortranarray(np.asarray(out["X"], dtype=np.float64))
    n, p = X.shape
    y = np.ascontiguousarray(out["y"], dtype=np.float64).ravel()
    c = np.ascontiguousarray(out["coeffs"], dtype=np.float64).ravel()
    w = np.ascontiguousarray(out["vcov.est.w"], dtype=np.float64).ravel()
    Z = np.asfortranarray(draw(out, 3, 1))
    V, Q = out["vcov.est.c"], out["vcov.est.Q"]
    Vd = V if hasattr(V, "ptr") else ctx.from_numpy(np.asarray(V))
    Qd = Q if hasattr(Q, "ptr") else ctx.from_numpy(np.asarray(Q))

    def values(pairs, vptr, qptr):
        pr = np.ascontiguousarray(pairs, dtype=np.int64)
        m = len(pairs)
        vals, avg, var = np.full((3, m), -7.0, order="F"), np.full(m, -7.0), np.full(m, -7.0)
        try:
            _lib.call("bigkrls_interaction_effects", ctx.handle, X.ctypes.data, n, p, y.ctypes.data, c.ctypes.data,
                      float(out["sigma"]), pr.ctypes.data, m, Z.ctypes.data, 3, vptr, qptr, Qd.ld, Qd.ncol, w.ctypes.data,
                      vals.ctypes.data, avg.ctypes.data, var.ctypes.data)
        finally:
            assert np.all(vals == -7.0) and np.all(avg == -7.0) and np.all(var == -7.0)   # refused before any write

    def ses(pairs, vptr, qptr):
        pr = np.ascontiguousarray(pairs, dtype=np.int64)
        se = np.full((3, len(pairs)), -7.0, order="F")
        try:
            _lib.call("bigkrls_interaction_effects_se", ctx.handle, X.ctypes.data, n, p, y.ctypes.data, c.ctypes.data,
                      float(out["sigma"]), pr.ctypes.data, len(pairs), Z.ctypes.data, 3, vptr, qptr, Qd.ld, Qd.ncol,
                      w.ctypes.data, 0, se.ctypes.data)
        finally:
            assert np.all(se == -7.0)

    for fn in (values, ses):
        with pytest.raises(_lib.BigKRLSError, match="vcov.est.c and its factors") as e:
            fn([(1, 2)], Vd.ptr, Qd.ptr)
        assert e.value.code == _lib.EINVAL
        with pytest.raises(_lib.BigKRLSError, match=r"pair \(1, 3\) is given more than once") as e:
            fn([(1, 3), (2, 2), (3, 1)], None, Qd.ptr)
        assert e.value.code == _lib.EINVAL
        with pytest.raises(_lib.BigKRLSError, match=r"pair \(4, 4\) is not defined") as e:       # the last column is binary
            fn([(1, 2), (4, 4)], None, Qd.ptr)
        assert e.value.code == _lib.EINVAL
        with pytest.raises(_lib.BigKRLSError, match=r"pair \(2, 5\) must index") as e:
            fn([(2, 5)], None, Qd.ptr)
        assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.BigKRLSError, match="exactly one"):
        ses([(1, 2)], None, None)
