"""robust_vcov() on the GPU (bigkrls_vcov_robust, csrc/robust.hip) through the public API, on small fits.

The reference is numpy on the object's own downloaded Q, d, lambda and residuals: V_ref = sd(y)^2 scale G Omega G formed
densely, G = Q diag(1 / (d + lambda)) Q', Omega = diag(omega) or, clustered, the block matrix e_i e_j [c_i == c_j].
The check is max |Qout diag(wout) Qout' - V_ref| <= 64 (n + k) eps ||V_ref||_2: the sums are n long, the k x k
eigensolver and the rotation are backward stable, 64 is the margin. Every ratio error / bound is printed.

Downstream (predict, marginal_effects, partial_dependence, summary) the same V_ref is pushed through the numpy
definitions the tests of those functions restate, within the 1e-8 of the largest variance those tests hold the
library to."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -53
HC_TYPES = ["classical", "HC0", "HC1", "HC2", "HC3"]


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


se_pointwise_numpy = _load("_pp_cpu_for_robust", "test_predict_pointwise_cpu.py").se_pointwise_numpy
_me_se_cpu = _load("_me_se_cpu_for_robust", "test_marginal_effects_se_cpu.py")
me_se_numpy, me_numpy = _me_se_cpu.me_se_numpy, _me_se_cpu.me_numpy
pd_numpy = _load("_pd_cpu_for_robust", "test_partial_dependence_cpu.py").pd_numpy


def host(m):
    return m.to_numpy() if hasattr(m, "to_numpy") else np.asarray(m)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# ---- the fits and their robust objects, computed once ---------------------------------------------------------------
def _data(n, p, seed, binary):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    if binary:
        X[:, p - 1] = (rng.random(n) < 0.4).astype(np.float64)
    y = np.sin(X @ np.linspace(0.3, 0.9, p)) + (0.1 + 0.4 * np.abs(X[:, 0])) * rng.standard_normal(n)   # heteroskedastic
    return X, y


def _labels(n, G, seed=1):
    return np.random.default_rng(seed).permutation((np.arange(n) * G) // n)


@pytest.fixture(scope="module")
def fits(ctx):
    import bigkrls_amd as bk
    Xs, ys = _data(300, 3, 41, True)
    Xl, yl = _data(1100, 4, 42, False)
    return {"dense300": bk.bigKRLS(ys, Xs, eigtrunc=0, vcov_form="both", ctx=ctx, noisy=False),
            "trunc1100": bk.bigKRLS(yl, Xl, eigtrunc=0.01, vcov_form="both", ctx=ctx, noisy=False)}


_cache = {}


def robust(fits, ctx, name, type, G=None):
    import bigkrls_amd as bk
    key = (name, type, G)
    if key not in _cache:
        obj = fits[name]
        cluster = None if G is None else _labels(np.asarray(obj["X"]).shape[0], G)
        _cache[key] = bk.robust_vcov(obj, type=type, cluster=cluster, ctx=ctx)
    return _cache[key]


def parts(obj):
    Q = host(obj["vcov.est.Q"])
    k = Q.shape[1]
    d = np.asarray(obj["K.eigenvalues"], dtype=np.float64).ravel()[:k]
    y = np.asarray(obj["y"], dtype=np.float64).ravel()
    ysd = float(np.std(y, ddof=1))
    e = (y - y.mean()) / ysd - np.asarray(obj["yfitted.std"]).ravel()
    g = 1.0 / (d + float(obj["lambda"]))
    return Q, d, g, e, ysd, (Q ** 2) @ (d * g)


def v_ref(obj, type, labels=None):
    """sd(y)^2 scale G Omega G, densely, from the ORIGINAL fit `obj`"""
    Q, d, g, e, ysd, h = parts(obj)
    n = Q.shape[0]
    Gm = (Q * g) @ Q.T
    if labels is not None:
        G = len(set(labels.tolist()))
        Omega = np.outer(e, e) * (labels[:, None] == labels[None, :])
        scale = G / (G - 1.0) if type == "CR1" else 1.0
        return ysd ** 2 * scale * (Gm @ Omega @ Gm)
    omega = {"classical": np.full(n, float(obj["sigmasq"])), "HC0": e ** 2, "HC1": e ** 2 * (n / float(obj["Neffective"])),
             "HC2": e ** 2 / (1.0 - h), "HC3": e ** 2 / (1.0 - h) ** 2}[type]
    return ysd ** 2 * (Gm @ (omega[:, None] * Gm))


def v_of(obj):
    Q, w = host(obj["vcov.est.Q"]), np.asarray(obj["vcov.est.w"], dtype=np.float64)
    return (Q * w) @ Q.T


def assert_within_bound(got, ref, n, k, what):
    bound = 64 * (n + k) * EPS * np.linalg.norm(ref, 2)
    err = float(np.max(np.abs(got - ref)))
    print(f"robust_vcov {what}: n={n} k={k} max err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3e}")
    assert err <= bound, what


# ---- the variance itself --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type", HC_TYPES)
@pytest.mark.parametrize("name", ["dense300", "trunc1100"])
def test_every_hc_type_against_the_dense_sandwich(fits, ctx, name, type):
    obj = fits[name]
    r = robust(fits, ctx, name, type)
    Q = host(r["vcov.est.Q"])
    n, k = Q.shape
    w = np.asarray(r["vcov.est.w"])
    # eigtrunc=0 keeps the pairs down to the last eigenvalue >= 0: all but the few the kernel's rounding makes negative
    assert k == host(obj["vcov.est.Q"]).shape[1] == obj["lastkeeper"] and (k > n // 2 if name == "dense300" else k < n // 4)
    assert np.all(w >= 0) and np.all(np.diff(w) <= 0)                    # wout >= 0, descending
    assert r["vcov.type"] == type and r["vcov.clusters"] is None
    assert r["vcov.est.c"] is None and r["vcov.est.fitted"] is None
    assert_within_bound(v_of(r), v_ref(obj, type), n, k, f"{name} {type}")


@pytest.mark.parametrize("type", ["CR0", "CR1"])
@pytest.mark.parametrize("name", ["dense300", "trunc1100"])
def test_cluster_types_with_ten_shuffled_clusters(fits, ctx, name, type):
    obj = fits[name]
    r = robust(fits, ctx, name, type, G=10)
    n, k = host(r["vcov.est.Q"]).shape
    w = np.asarray(r["vcov.est.w"])
    assert np.all(w >= 0) and np.all(np.diff(w) <= 0) and r["vcov.clusters"] == 10 and r["vcov.type"] == type
    assert_within_bound(v_of(r), v_ref(obj, type, _labels(n, 10)), n, k, f"{name} {type} G=10")


@pytest.mark.parametrize("name", ["dense300", "trunc1100"])
def test_classical_reproduces_the_fit(fits, ctx, name):
    obj = fits[name]
    r = robust(fits, ctx, name, "classical")
    n, k = host(r["vcov.est.Q"]).shape
    assert_within_bound(v_of(r), host(obj["vcov.est.c"]), n, k, f"{name} classical vs the fit's vcov.est.c")
    assert r["var.avgderivatives"].shape == obj["var.avgderivatives"].shape
    assert rel(r["var.avgderivatives"], obj["var.avgderivatives"]) < 1e-8
    assert rel(r["var.avgderivatives.std"], obj["var.avgderivatives.std"]) < 1e-8


@pytest.mark.parametrize("name", ["dense300", "trunc1100"])
def test_every_row_its_own_cluster_is_hc0(fits, ctx, name):
    import bigkrls_amd as bk
    obj = fits[name]
    n = np.asarray(obj["X"]).shape[0]
    own = bk.robust_vcov(obj, type="CR0", cluster=np.random.default_rng(3).permutation(n), ctx=ctx)
    hc0 = robust(fits, ctx, name, "HC0")
    k = host(hc0["vcov.est.Q"]).shape[1]
    assert own["vcov.clusters"] == n
    assert_within_bound(v_of(own), v_of(hc0), n, k, f"{name} CR0 with G = n vs HC0")
    assert_within_bound(v_of(own), v_ref(obj, "HC0"), n, k, f"{name} CR0 with G = n vs the dense HC0")


@pytest.mark.parametrize("name", ["dense300", "trunc1100"])
def test_hc1_is_hc0_times_n_over_neffective(fits, ctx, name):
    obj = fits[name]
    w0 = np.asarray(robust(fits, ctx, name, "HC0")["vcov.est.w"])
    w1 = np.asarray(robust(fits, ctx, name, "HC1")["vcov.est.w"])
    f = np.asarray(obj["X"]).shape[0] / float(obj["Neffective"])
    assert rel(w1, w0 * f) <= 1e-13
    assert same_bits(host(robust(fits, ctx, name, "HC0")["vcov.est.Q"]), host(robust(fits, ctx, name, "HC1")["vcov.est.Q"]))


@pytest.mark.parametrize("name", ["dense300", "trunc1100"])
def test_three_clusters_give_rank_three(fits, ctx, name):
    obj = fits[name]
    r = robust(fits, ctx, name, "CR0", G=3)
    n, k = host(r["vcov.est.Q"]).shape
    w = np.asarray(r["vcov.est.w"])
    assert k > 3 and np.sum(w > 1e-12 * w[0]) <= 3
    assert_within_bound(v_of(r), v_ref(obj, "CR0", _labels(n, 3)), n, k, f"{name} CR0 G=3")


# ---- downstream: u = 5 new points ----------------------------------------------------------------------------------
def _new_points(obj, u=5, seed=77):
    X = np.asarray(obj["X"])
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((u, X.shape[1]))
    for j in range(X.shape[1]):
        vals = np.unique(X[:, j])
        if vals.size == 2:
            Z[:, j] = rng.choice(vals, size=u)
    return Z


@pytest.mark.parametrize("name,type,G", [("dense300", "HC3", None), ("dense300", "CR1", 10), ("trunc1100", "HC1", None)])
def test_downstream_functions_use_the_robust_factors(fits, ctx, name, type, G, capsys):
    import bigkrls_amd as bk
    obj = fits[name]
    r = robust(fits, ctx, name, type, G)
    X, y = np.asarray(obj["X"]), np.asarray(obj["y"]).ravel()
    n = X.shape[0]
    V = v_ref(obj, type, None if G is None else _labels(n, G))
    Z = _new_points(obj)
    # predict(se_pred=True)
    pr = bk.predict(r, Z, se_pred=True, ctx=ctx)
    ref = se_pointwise_numpy(X, y, obj["sigma"], V, Z, neff=obj["Neffective"]) ** 2
    assert np.max(np.abs(pr["se.pred"] ** 2 - ref)) <= 1e-8 * ref.max()
    assert same_bits(pr["predicted"], bk.predict(obj, Z, ctx=ctx)["predicted"])
    # marginal_effects(se=True) and the variance of the averages
    me = bk.marginal_effects(r, Z, ctx=ctx, se=True)
    ref = me_se_numpy(X, y, obj["coeffs"], obj["sigma"], Z, V) ** 2
    assert np.max(np.abs(me["se.derivatives"] ** 2 - ref)) <= 1e-8 * ref.max()
    ref_var = me_numpy(X, y, obj["coeffs"], obj["sigma"], Z, vcov_c=V)[2]
    assert np.max(np.abs(me["var.avgderivatives"].ravel() - ref_var)) <= 1e-8 * ref_var.max()
    # the object's own var.avgderivatives: the same definition at newdata = X
    ref_var = me_numpy(X, y, obj["coeffs"], obj["sigma"], X, vcov_c=V)[2]
    assert np.max(np.abs(np.asarray(r["var.avgderivatives"]).ravel() - ref_var)) <= 1e-8 * ref_var.max()
    assert same_bits(r["avgderivatives"], obj["avgderivatives"]) and same_bits(r["derivatives"], obj["derivatives"])
    # partial_dependence()
    which = [1, X.shape[1]]
    pdr = bk.partial_dependence(r, which=which, grid=4, newdata=Z, ctx=ctx)
    pds, ses, covs = pd_numpy(X, y, obj["coeffs"], obj["sigma"], which, pdr["grid"], newdata=Z, vcov_c=V,
                              neffective=obj["Neffective"])
    for jj in range(len(which)):
        assert np.max(np.abs(pdr["se.pd"][jj] ** 2 - ses[jj] ** 2)) <= 1e-8 * np.max(ses[jj] ** 2)
        assert np.max(np.abs(pdr["vcov.pd"][jj] - covs[jj])) <= 1e-8 * np.max(np.abs(covs[jj]))
    # summary(): the standard-error column is sqrt of the recomputed variances; one extra line
    capsys.readouterr()
    res = bk.summary(r)
    text = capsys.readouterr().out
    assert f"vcov: {type}\n" in text
    assert np.array_equal(res["ttests"][:, 1], np.sqrt(np.asarray(r["var.avgderivatives"]).ravel()))
    bk.summary(obj)
    assert "vcov:" not in capsys.readouterr().out


# ---- plumbing -------------------------------------------------------------------------------------------------------
def test_input_untouched_and_whole_call_repeatable(fits, ctx):
    import bigkrls_amd as bk
    obj = fits["trunc1100"]
    Q0, w0 = host(obj["vcov.est.Q"]).copy(), np.asarray(obj["vcov.est.w"]).copy()
    keys = set(obj)
    lab = _labels(1100, 10)
    for type, cluster in (("HC3", None), ("CR1", lab)):
        a = bk.robust_vcov(obj, type=type, cluster=cluster, ctx=ctx)
        b = bk.robust_vcov(obj, type=type, cluster=cluster, ctx=ctx)
        assert same_bits(host(a["vcov.est.Q"]), host(b["vcov.est.Q"])) and same_bits(a["vcov.est.w"], b["vcov.est.w"])
        assert same_bits(a["var.avgderivatives"], b["var.avgderivatives"])
        assert a["vcov.est.Q"] is not obj["vcov.est.Q"]
    assert same_bits(host(obj["vcov.est.Q"]), Q0) and same_bits(obj["vcov.est.w"], w0)
    assert set(obj) == keys and obj["vcov.est.c"] is not None


@pytest.mark.parametrize("binary", [False, True])
def test_save_load_round_trip_keeps_the_type(fits, ctx, tmp_path, binary):
    import bigkrls_amd as bk
    r = robust(fits, ctx, "dense300", "CR1", 10)
    back = bk.load_bigKRLS(bk.save_bigKRLS(r, str(tmp_path / "m"), noisy=False, binary=binary), noisy=False, ctx=ctx)
    assert back["vcov.type"] == "CR1" and back["vcov.clusters"] == 10 and back.get("vcov.est.c") is None
    assert same_bits(host(back["vcov.est.Q"]), host(r["vcov.est.Q"]))
    assert same_bits(np.asarray(back["vcov.est.w"], dtype=np.float64), r["vcov.est.w"])
    Z = _new_points(r)
    a, b = bk.predict(r, Z, se_pred=True, ctx=ctx), bk.predict(back, Z, se_pred=True, ctx=ctx)
    assert np.max(np.abs(a["se.pred"] - b["se.pred"])) <= 1e-12 * np.max(a["se.pred"])


def test_implicit_fit(ctx):
    import bigkrls_amd as bk
    # The implicit form has no dense fallback, and at N = 1100 the block Lanczos may use 4 blocks of 128 columns. P = 3
    # with sigma = 4: the 512th eigenvalue of this kernel is 5e-13 of the first (the residuals are held to 1e-10) and
    # the 128th 1e-5 (the first block is well conditioned); P = 4 leaves 3e-7 at 512, P = 2 breaks down in block one.
    X, y = _data(1100, 3, 43, False)
    obj = bk.bigKRLS(y, X, sigma=4.0, kernel="implicit", Neig=60, vcov_form="factors", ctx=ctx, noisy=False)
    r = bk.robust_vcov(obj, type="HC1", ctx=ctx)
    n, k = host(r["vcov.est.Q"]).shape
    assert (n, k) == (1100, host(obj["vcov.est.Q"]).shape[1]) and k <= 60
    assert_within_bound(v_of(r), v_ref(obj, "HC1"), n, k, "implicit HC1")
    c = bk.robust_vcov(obj, type="CR1", cluster=_labels(n, 10), ctx=ctx)
    assert_within_bound(v_of(c), v_ref(obj, "CR1", _labels(n, 10)), n, k, "implicit CR1 G=10")


def test_all_pairs_kept_k_equals_n(ctx):
    """k == n, the boundary of the library's k <= n: N = 40, P = 5 -- a kernel whose 40 eigenvalues are all far above
    rounding, so eigtrunc = 0 keeps every pair."""
    import bigkrls_amd as bk
    X, y = _data(40, 5, 45, False)
    obj = bk.bigKRLS(y, X, eigtrunc=0, vcov_form="both", ctx=ctx, noisy=False)
    assert obj["lastkeeper"] == 40 and host(obj["vcov.est.Q"]).shape == (40, 40)
    lab = _labels(40, 4)
    for type, cluster in (("classical", None), ("HC3", None), ("CR1", lab)):
        r = bk.robust_vcov(obj, type=type, cluster=cluster, ctx=ctx)
        assert host(r["vcov.est.Q"]).shape == (40, 40)
        assert_within_bound(v_of(r), v_ref(obj, type, cluster), 40, 40, f"k = n = 40 {type}")
    assert_within_bound(v_of(bk.robust_vcov(obj, type="classical", ctx=ctx)), host(obj["vcov.est.c"]), 40, 40,
                        "k = n = 40 classical vs the fit's vcov.est.c")


def test_object_without_factors_is_refused(ctx):
    import bigkrls_amd as bk
    X, y = _data(120, 3, 44, False)
    obj = bk.bigKRLS(y, X, ctx=ctx, noisy=False)                          # vcov_form="dense"
    with pytest.raises(ValueError, match=r'vcov_form="factors" or "both"'):
        bk.robust_vcov(obj, ctx=ctx)


def test_native_refusals(fits, ctx):
    """what the library itself refuses: Qout aliasing Q, a bad type, clusters with a leverage type"""
    from bigkrls_amd import _lib
    obj = fits["trunc1100"]
    Q = obj["vcov.est.Q"]
    n, k = Q.nrow, Q.ncol
    d = np.ascontiguousarray(np.asarray(obj["K.eigenvalues"])[:k])
    e, w, lab = np.zeros(n), np.zeros(k), np.zeros(n, dtype=np.int64)
    out = ctx.empty(n, k)

    def call(type, labels, G, qout):
        _lib.call("bigkrls_vcov_robust", ctx.handle, n, k, Q.ptr, Q.ld, d.ctypes.data, float(obj["lambda"]),
                  e.ctypes.data, 1.0, 1.0, type, labels.ctypes.data if labels is not None else None, G, qout.ptr,
                  qout.ld, w.ctypes.data)
    with pytest.raises(_lib.BigKRLSError, match="must not alias"):
        call(1, None, 0, Q)
    with pytest.raises(_lib.BigKRLSError, match="type must be"):
        call(5, None, 0, out)
    with pytest.raises(_lib.BigKRLSError, match="clusters go with type 1 or 2"):
        call(3, lab, 1, out)
    lab[5] = 2
    with pytest.raises(_lib.BigKRLSError, match=r"label of row 6 is outside \[0, G\)"):
        call(1, lab, 2, out)
