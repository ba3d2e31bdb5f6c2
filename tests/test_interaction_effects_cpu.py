"""CPU checks of interaction_effects(): the definition restated literally in numpy (also used by
tests/test_gpu_interaction_effects.py), its agreement with the product-of-modulations form the device code uses, with
differences of the first-order effects of tests/test_marginal_effects_cpu.py, the identity of se^2 with var.avg at a
single new point, the C ABI's three new entries against the ctypes table, and the Python checks that happen before any
native call."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_me_cpu", os.path.join(ROOT, "tests", "test_marginal_effects_cpu.py"))
_me_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_me_cpu)
me_numpy, _kernel, _header_arity = _me_cpu.me_numpy, _me_cpu._kernel, _me_cpu._header_arity


# --------------------------------------------------------------------------
# the definition
# --------------------------------------------------------------------------
def _standardise(X, y, newdata):
    X = np.asarray(X, dtype=np.float64)
    Z = np.asarray(newdata, dtype=np.float64)
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    binary = [((X[:, j].min() - m[j]) / s[j], (X[:, j].max() - m[j]) / s[j]) if np.unique(X[:, j]).size == 2 else None
              for j in range(X.shape[1])]
    return (X - m) / s, (Z - m) / s, s, float(np.std(y, ddof=1)), binary


def _first_order_literal(Zs, Xs, sigma, j, binary):
    """The u x n weights of the first-order effect of column j at the rows Zs, as me_std builds them."""
    if binary[j] is not None:
        z0, z1 = binary[j]
        Z1, Z0 = Zs.copy(), Zs.copy()
        Z1[:, j], Z0[:, j] = z1, z0
        return (_kernel(Z1, Xs, sigma) - _kernel(Z0, Xs, sigma)) / (z1 - z0)
    return (-2.0 / sigma) * (Zs[:, j][:, None] - Xs[:, j][None, :]) * _kernel(Zs, Xs, sigma)


def g_literal(Zs, Xs, sigma, j, k, binary):
    """G_jk (u x n) in standardised units, without the modulations: Kn o ((4/sigma^2) d_j d_k - (2/sigma) delta_jk) for a
    continuous pair; for a binary column the kernels are rebuilt with that column set to z1 / z0."""
    if binary[j] is None and binary[k] is None:
        dj = Zs[:, j][:, None] - Xs[:, j][None, :]
        dk = Zs[:, k][:, None] - Xs[:, k][None, :]
        return _kernel(Zs, Xs, sigma) * ((4.0 / sigma ** 2) * dj * dk - (2.0 / sigma if j == k else 0.0))
    if binary[j] is None:
        j, k = k, j                                            # j is binary from here on
    assert j != k, "a pair (j, j) on a binary column is not defined"
    z0, z1 = binary[j]
    Z1, Z0 = Zs.copy(), Zs.copy()
    Z1[:, j], Z0[:, j] = z1, z0
    # operator k (derivative or first difference) applied at column j's two values, then the first difference in j
    return (_first_order_literal(Z1, Xs, sigma, k, binary) - _first_order_literal(Z0, Xs, sigma, k, binary)) / (z1 - z0)


def modulation(Zs, Xs, sigma, j, binary):
    """r (u), t (u), s (n) of column j: me_se_rt_kernel and me_se_s_kernel (csrc/margeff.h)."""
    u = Zs.shape[0]
    if binary[j] is None:
        return (-2.0 / sigma) * Zs[:, j], np.full(u, 2.0 / sigma), Xs[:, j]
    z0, z1 = binary[j]
    sd = 1.0 / (z1 - z0)
    E = np.exp(-(z1 - z0) ** 2 / sigma)
    Einv = 1.0 / E
    hi = np.isclose(Zs[:, j], z1, rtol=0, atol=1e-9)
    r = np.where(hi, sd * (1.0 - Einv), -sd * (1.0 - E))
    return r, np.full(u, sd * (Einv - E)), np.isclose(Xs[:, j], z1, rtol=0, atol=1e-9).astype(np.float64)


def g_modulated(Zs, Xs, sigma, j, k, binary):
    """G_jk = Kn o m_j o m_k - (2/sigma) delta_jk Kn: the form of csrc/inteff.hip."""
    Kn = _kernel(Zs, Xs, sigma)
    rj, tj, sj = modulation(Zs, Xs, sigma, j, binary)
    rk, tk, sk = modulation(Zs, Xs, sigma, k, binary)
    mj = rj[:, None] + tj[:, None] * sj[None, :]
    mk = rk[:, None] + tk[:, None] * sk[None, :]
    return Kn * mj * mk - (2.0 / sigma if j == k else 0.0) * Kn


def default_pairs(X, which=None):
    p = X.shape[1]
    cols = sorted(which) if which is not None else list(range(1, p + 1))
    isbin = [np.unique(X[:, j]).size == 2 for j in range(p)]
    return [(j, k) for a, j in enumerate(cols) for k in cols[a:] if not (j == k and isbin[j - 1])]


def ie_numpy(X, y, coeffs, sigma, newdata, vcov_c=None, pairs=None):
    """interaction_effects() in numpy: (interactions u x m, avginteractions m, var.avginteractions m, se.interactions
    u x m) in the original units; the last two are None without vcov_c. pairs: 1-based (j, k); default: every j <= k
    without the binary diagonals. The quadratic forms are taken row by row."""
    Xs, Zs, s, ysd, binary = _standardise(X, y, newdata)
    u = Zs.shape[0]
    pairs = default_pairs(np.asarray(X)) if pairs is None else [(min(a, b), max(a, b)) for a, b in pairs]
    c = np.asarray(coeffs, dtype=np.float64)
    V = None if vcov_c is None else np.asarray(vcov_c, dtype=np.float64) / ysd ** 2
    vals = np.empty((u, len(pairs)))
    var = None if V is None else np.empty(len(pairs))
    se = None if V is None else np.empty((u, len(pairs)))
    for i, (j1, k1) in enumerate(pairs):
        j, k = j1 - 1, k1 - 1
        G = g_literal(Zs, Xs, sigma, j, k, binary)
        g = ysd / (s[j] * s[k])
        vals[:, i] = (G @ c) * g
        if V is not None:
            f = 2.0 if (binary[j] is not None or binary[k] is not None) else 1.0
            a = G.sum(axis=0) / u
            var[i] = f * (a @ V @ a) * g ** 2
            se[:, i] = np.sqrt(f * np.array([G[r] @ V @ G[r] for r in range(u)])) * g
    return vals, vals.mean(axis=0), var, se


def _data(n=60, p=4, seed=17, two_binary=False):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    X[:, 2] = np.where(rng.random(n) < 0.45, 3.0, -1.0)            # binary, values -1 and 3
    if two_binary:
        X[:, 0] = np.where(rng.random(n) < 0.6, 0.5, 2.0)          # binary, values 0.5 and 2
    y = np.sin(X @ np.linspace(0.3, 0.9, p)) + 0.1 * rng.standard_normal(n)
    c = rng.standard_normal(n)
    G = rng.standard_normal((n, n))
    return X, y, c, G @ G.T / n, rng


def _newdata(X, rng, u):
    Z = rng.standard_normal((u, X.shape[1]))
    for j in range(X.shape[1]):
        vals = np.unique(X[:, j])
        if vals.size == 2:
            Z[:, j] = rng.choice(vals, size=u)
    return Z


CASES = [dict(), dict(n=70, p=5, seed=23, two_binary=True)]


@pytest.mark.parametrize("case", CASES)
def test_product_of_modulations_equals_the_literal_operator(case):
    X, y, c, V, rng = _data(**case)
    sigma = float(X.shape[1])
    Z = _newdata(X, rng, 23)
    Xs, Zs, s, ysd, binary = _standardise(X, y, Z)
    for j1, k1 in default_pairs(X):
        lit = g_literal(Zs, Xs, sigma, j1 - 1, k1 - 1, binary)
        mod = g_modulated(Zs, Xs, sigma, j1 - 1, k1 - 1, binary)
        assert np.max(np.abs(mod - lit)) <= 1e-11 * np.max(np.abs(lit)), (j1, k1)
        np.testing.assert_allclose(mod @ c, lit @ c, rtol=0, atol=1e-11 * np.max(np.abs(lit @ c)))


@pytest.mark.parametrize("case", CASES)
def test_values_are_differences_of_the_first_order_effects(case):
    """For every ordered pair: operator k applied to me_numpy's first-order effect of column j. Continuous k: central
    differences with h = 1e-4 in standardised units, within 1e-6 of the largest interaction (truncation h^2/6 times the
    fourth-order effect, rounding eps/h: both below 1e-7 here). Binary k: the exact difference between column k's two
    values over their gap, within 1e-10."""
    X, y, c, V, rng = _data(**case)
    p = X.shape[1]
    sigma = float(p)
    Z = _newdata(X, rng, 23)
    sd = X.std(axis=0, ddof=1)
    pairs = default_pairs(X)
    vals, avg, _, _ = ie_numpy(X, y, c, sigma, Z)
    top = np.abs(vals).max()
    np.testing.assert_allclose(avg, vals.mean(axis=0), rtol=1e-15)
    worst = {"central": 0.0, "second": 0.0}
    for i, (j1, k1) in enumerate(pairs):
        for a, b in {(j1, k1), (k1, j1)}:                   # effect of column a, operator of column b
            col = b - 1
            if np.unique(X[:, col]).size == 2:
                lo, hi = X[:, col].min(), X[:, col].max()
                Zp, Zm = Z.copy(), Z.copy()
                Zp[:, col], Zm[:, col] = hi, lo
                step, kind, bound = hi - lo, "second", 1e-10
            else:
                h = 1e-4 * sd[col]
                Zp, Zm = Z.copy(), Z.copy()
                Zp[:, col] += h
                Zm[:, col] -= h
                step, kind, bound = 2.0 * h, "central", 1e-6
            Dp, _, _ = me_numpy(X, y, c, sigma, Zp, which=[a])
            Dm, _, _ = me_numpy(X, y, c, sigma, Zm, which=[a])
            err = np.abs((Dp[:, 0] - Dm[:, 0]) / step - vals[:, i]).max() / top
            worst[kind] = max(worst[kind], err)
            assert err <= bound, (a, b, kind, err)
    print("interaction values against differences of first-order effects, relative to the largest:", worst)


@pytest.mark.parametrize("case", CASES)
def test_single_point_se_squared_is_var_avginteractions(case):
    X, y, c, V, rng = _data(**case)
    sigma = float(X.shape[1])
    for _ in range(4):                                          # (the binary columns' groups vary with the draw)
        Z = _newdata(X, rng, 1)
        _, _, var, se = ie_numpy(X, y, c, sigma, Z, vcov_c=V)
        np.testing.assert_allclose(se[0] ** 2, var, rtol=1e-12)
    pairs = [(3, 1), (2, 2), (4, 3)]
    _, _, var, se = ie_numpy(X, y, c, sigma, Z, vcov_c=V, pairs=pairs)
    np.testing.assert_allclose(se[0] ** 2, var, rtol=1e-12)


def test_pairs_are_taken_ordered():
    X, y, c, V, rng = _data()
    Z = _newdata(X, rng, 5)
    a = ie_numpy(X, y, c, 4.0, Z, vcov_c=V, pairs=[(3, 1), (4, 2)])
    b = ie_numpy(X, y, c, 4.0, Z, vcov_c=V, pairs=[(1, 3), (2, 4)])
    for x, z in zip(a, b):
        assert np.array_equal(x, z)


# --------------------------------------------------------------------------
# the C ABI and its ctypes table
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name,arity", [("bigkrls_dev_gemm_modulated2", 17), ("bigkrls_interaction_effects", 19),
                                        ("bigkrls_interaction_effects_se", 18)])
def test_header_declares_and_ctypes_table_matches(name, arity):
    from bigkrls_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name]) == _header_arity(name) == arity


def test_entries_follow_the_first_order_ones():
    # gemm_modulated's arguments plus r2, t2, s2 and d
    assert _header_arity("bigkrls_dev_gemm_modulated2") == _header_arity("bigkrls_dev_gemm_modulated") + 4
    # marginal_effects_se's arguments (pairs and m in place of which and n_which), and for the values entry the three
    # outputs in place of block_rows and h_se
    assert _header_arity("bigkrls_interaction_effects_se") == _header_arity("bigkrls_marginal_effects_se")
    assert _header_arity("bigkrls_interaction_effects") == _header_arity("bigkrls_marginal_effects_se") - 2 + 3


def test_public_api():
    import inspect
    import bigkrls_amd as bk
    assert callable(bk.interaction_effects) and "interaction_effects" in bk.__all__
    params = inspect.signature(bk.interaction_effects).parameters
    assert list(params) == ["object", "newdata", "pairs", "which", "se", "vcov", "ctx", "_block_rows"]
    assert params["se"].default is False and params["newdata"].default is None and params["_block_rows"].default == 0
    assert callable(bk.ops.bGemmModulated2)


# --------------------------------------------------------------------------
# Python checks happen before any native call (no GPU here)
# --------------------------------------------------------------------------
def _object(vcov=True, factors=False):
    obj = _me_cpu._object()                                     # n = 40, p = 3, column 2 binary with values 1 and 3
    n = obj["X"].shape[0]
    if not vcov:
        obj["vcov.est.c"] = None
    if factors:
        obj["vcov.est.Q"] = np.eye(n)[:, :5]
        obj["vcov.est.w"] = np.ones(5)
    return obj


@pytest.fixture
def no_native(monkeypatch):
    from bigkrls_amd import api

    def boom(*a, **k):
        raise AssertionError("native call reached")
    monkeypatch.setattr(api, "_call_native", boom)
    monkeypatch.setattr(api, "default_context", boom)


@pytest.mark.parametrize("pairs,match", [
    ([(0, 1)], r"pair \(0, 1\)"), ([(1, 4)], r"pair \(1, 4\)"), ([(1, 3), (3, 1)], r"pair \(1, 3\) is given more than once"),
    ([(1, 1), (1, 1)], r"pair \(1, 1\) is given more than once"), ([(2, 2)], r"pair \(2, 2\) is not defined"),
])
def test_bad_pairs_raise_naming_the_pair(no_native, pairs, match):
    import bigkrls_amd as bk
    obj = _object()
    with pytest.raises(ValueError, match=match):
        bk.interaction_effects(obj, obj["X"][:3], pairs=pairs)


def test_newdata_checks_raise(no_native):
    import bigkrls_amd as bk
    obj = _object()
    with pytest.raises(ValueError, match="ncol"):
        bk.interaction_effects(obj, np.zeros((5, 4)))
    nd = obj["X"][:4].copy()
    nd[2, 1] = 2.0                                              # neither 1 nor 3
    with pytest.raises(ValueError, match="column 2"):
        bk.interaction_effects(obj, nd)
    # the same column outside every pair is not touched: no error up to the native call
    with pytest.raises(AssertionError, match="native call reached"):
        bk.interaction_effects(obj, nd, pairs=[(1, 3)])
    nd[0, 0] = np.inf
    with pytest.raises(ValueError, match="missing or infinite"):
        bk.interaction_effects(obj, nd, pairs=[(1, 3)])
    with pytest.raises(ValueError, match="which must index"):
        bk.interaction_effects(obj, which=[1, 4])
    with pytest.raises(TypeError):
        bk.interaction_effects({"X": np.zeros((3, 2))}, np.zeros((1, 2)))


def test_se_without_vcov_raises_before_any_native_call(no_native):
    import bigkrls_amd as bk
    obj = _object(vcov=False)
    with pytest.raises(ValueError, match="recompute bigKRLS object with bigKRLS\\(,vcov.est=TRUE\\)"):
        bk.interaction_effects(obj, obj["X"][:3], se=True)
    with pytest.raises(AssertionError, match="native call reached"):      # se=False goes on to the native call
        bk.interaction_effects(obj, obj["X"][:3])


def test_multi_gpu_object_without_factors_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    obj["rows"] = (0, 20)
    obj["vcov.est.c.cols"] = None
    with pytest.raises(NotImplementedError):
        bk.interaction_effects(obj, obj["X"][:3])
    obj = _object(factors=True)
    obj["rows"] = (0, 20)
    with pytest.raises(AssertionError, match="native call reached"):      # with the factors it goes on
        bk.interaction_effects(obj, obj["X"][:3], vcov="factors")


class _FakeCtx:
    handle = None

    def from_numpy(self, a):
        a = np.asarray(a)
        return type("M", (), {"ptr": None, "ld": a.shape[0], "nrow": a.shape[0], "ncol": a.shape[1]})()


KEYS = {"interactions", "avginteractions", "var.avginteractions", "pairs", "pairlabs", "binaryindicator", "newdata"}


@pytest.mark.parametrize("vcov", [None, "factors"])
def test_keys_defaults_and_entries_with_and_without_se(monkeypatch, vcov):
    from bigkrls_amd import _lib, api
    seen = []
    monkeypatch.setattr(api, "_call_native", lambda name, *args: seen.append((name, args)))
    obj = _object(factors=True)
    ie = api.interaction_effects(obj, ctx=_FakeCtx(), vcov=vcov)
    assert set(ie) == KEYS
    assert ie["pairs"] == [(1, 1), (1, 2), (1, 3), (2, 3), (3, 3)]         # no (2, 2): column 2 is binary
    assert ie["pairlabs"] == ["x1:x1", "x1:x2", "x1:x3", "x2:x3", "x3:x3"]
    assert ie["binaryindicator"].tolist() == [[False, False], [False, True], [False, False], [True, False], [False, False]]
    assert ie["newdata"] is not None and ie["interactions"].shape == (40, 5) and ie["avginteractions"].shape == (1, 5)
    assert [s[0] for s in seen] == ["bigkrls_interaction_effects"]
    del seen[:]
    ie = api.interaction_effects(obj, obj["X"][:3], pairs=[(3, 1), (2, 1)], ctx=_FakeCtx(), vcov=vcov, se=True)
    assert set(ie) == KEYS | {"se.interactions"}
    assert ie["pairs"] == [(1, 3), (1, 2)]
    assert ie["se.interactions"].shape == ie["interactions"].shape == (3, 2)
    assert [s[0] for s in seen] == ["bigkrls_interaction_effects", "bigkrls_interaction_effects_se"]
    n = obj["X"].shape[0]
    for name, args in seen:
        assert len(args) == len(_lib.SIGNATURES[name])
        assert args[8] == 2                                                # m
        # the scalars that go with the factors (ldq, k) are zero when the matrix is the chosen form
        assert (args[13], args[14]) == ((n, 5) if vcov == "factors" else (0, 0))
    assert seen[1][1][16] == 0                                             # block_rows: automatic
    ie = api.interaction_effects(obj, obj["X"][:3], which=[3, 1], ctx=_FakeCtx())
    assert ie["pairs"] == [(1, 1), (1, 3), (3, 3)]
