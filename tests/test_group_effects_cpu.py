"""CPU checks of group_effects(): an oracle written from the definition (also used by tests/test_gpu_group_effects.py)
against the column-side algebra of csrc/margeff.hip applied per group, the Wald statistic and the chi-square tail on
values known in closed form, the C ABI's two new entry points and their ctypes arity, the export, the labelling rule of
`bins`, and the Python validation, which raises before any native call."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------
# the oracle: from the definition
# --------------------------------------------------------------------------
def _kernel(A, B, sigma):
    d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2)
    return np.exp(-d2 / sigma)


def ge_numpy(X, y, coeffs, sigma, which, newdata, labels, vcov_c=None):
    """group_effects() in numpy, from the definition: the dense test kernel Kn, one weight vector g_ij (n) per new row i
    and selected variable j with derivative[i, j] = g_ij' c -- for a continuous column the derivative of the kernel, for a
    binary one the first difference between the kernels of the row with column j rewritten to each of the two training
    values --, the group means of the weights, and for the joint covariance Gbar' V Gbar with sqrt(2) on the binary entries.
    which: 1-based; labels: integers in [0, G). Returns (ame G x |J|, cov (G |J|) x (G |J|) with index jj G + g or None,
    derivatives u x |J|), original units."""
    X = np.asarray(X, dtype=np.float64)
    Z = np.asarray(newdata, dtype=np.float64)
    labels = np.asarray(labels)
    n, p = X.shape
    u = Z.shape[0]
    G = int(labels.max()) + 1
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    ysd = float(np.std(y, ddof=1))
    Xs, Zs = (X - m) / s, (Z - m) / s
    c = np.asarray(coeffs, dtype=np.float64).ravel()
    Kn = _kernel(Zs, Xs, sigma)                                                  # u x n
    nj = len(which)
    W = np.empty((u, nj, n))                                                     # the weights, original units up to sd(y)
    f = np.ones(nj)
    for jj, j1 in enumerate(which):
        j = j1 - 1
        if np.unique(X[:, j]).size == 2:
            lo, hi = X[:, j].min(), X[:, j].max()
            Z1, Z0 = Z.copy(), Z.copy()
            Z1[:, j], Z0[:, j] = hi, lo
            z1, z0 = (hi - m[j]) / s[j], (lo - m[j]) / s[j]
            W[:, jj, :] = (_kernel((Z1 - m) / s, Xs, sigma) - _kernel((Z0 - m) / s, Xs, sigma)) / (z1 - z0) / s[j]
            f[jj] = math.sqrt(2.0)
        else:
            W[:, jj, :] = (-2.0 / sigma) * (Zs[:, j][:, None] - Xs[:, j][None, :]) * Kn / s[j]
    D = ysd * (W @ c)                                                            # u x nj
    Gbar = np.zeros((nj * G, n))
    ame = np.full((G, nj), np.nan)
    for g in range(G):
        rows = labels == g
        if not rows.any():
            continue
        for jj in range(nj):
            Gbar[jj * G + g] = W[rows, jj, :].mean(axis=0)
            ame[g, jj] = ysd * (Gbar[jj * G + g] @ c)
    cov = None
    if vcov_c is not None:
        fe = np.repeat(f, G)
        cov = (Gbar @ np.asarray(vcov_c, dtype=np.float64) @ Gbar.T) * np.outer(fe, fe)
    return ame, cov, D


def margeff_cols_numpy(X, sigma, which, newdata, rows):
    """The algebra of csrc/margeff.hip on the new rows `rows` alone: the sums T = sum_i Kn[i, k] and H = sum_i Kn[i, k]
    Zs_ij (or over the new rows whose binary column holds the upper value), then me_cols_kernel's formulas, and the scaling
    a = -(2 / sigma) / (n_g sd(x_j)) or 1 / ((z1 - z0) n_g sd(x_j)). Returns a S (|J| x n): the group-mean weights."""
    X = np.asarray(X, dtype=np.float64)
    Z = np.asarray(newdata, dtype=np.float64)[rows]
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    Xs, Zs = (X - m) / s, (Z - m) / s
    Kn = _kernel(Zs, Xs, sigma)
    ng = Z.shape[0]
    T = Kn.sum(axis=0)
    out = np.empty((len(which), X.shape[0]))
    for jj, j1 in enumerate(which):
        j = j1 - 1
        x = Xs[:, j]
        if np.unique(X[:, j]).size == 2:
            lo, hi = X[:, j].min(), X[:, j].max()
            z1, z0 = (hi - m[j]) / s[j], (lo - m[j]) / s[j]
            H = Kn[Z[:, j] == hi].sum(axis=0)
            sd = 1.0 / (z1 - z0)
            E, Einv = math.exp(-1.0 / (sd * sd * sigma)), math.exp(1.0 / (sd * sd * sigma))
            up = X[:, j] == hi
            sv = np.where(up, (1.0 - E) * H + (Einv - 1.0) * (T - H), (1.0 - Einv) * H + (E - 1.0) * (T - H))
            out[jj] = sv / ((z1 - z0) * ng * s[j])
        else:
            H = (Kn * Zs[:, j][:, None]).sum(axis=0)
            out[jj] = (-2.0 / sigma) * (H - x * T) / (ng * s[j])
    return out


def _data():
    rng = np.random.default_rng(29)
    n, p, u = 40, 4, 23
    X = rng.standard_normal((n, p)) * np.array([1.0, 1.0, 3.0, 0.5]) + np.array([0.0, 0.0, 5.0, -1.0])
    X[:, 1] = (rng.random(n) < 0.4).astype(np.float64) * 2.0 + 1.0       # binary, values 1 and 3
    y = rng.standard_normal(n) * 2.0 + 0.7
    c = rng.standard_normal(n)
    Gm = rng.standard_normal((n, n))
    Vc = Gm @ Gm.T / n
    Z = rng.standard_normal((u, p)) * np.array([1.0, 1.0, 3.0, 0.5]) + np.array([0.0, 2.0, 5.0, -1.0])
    Z[:, 1] = (rng.random(u) < 0.5).astype(np.float64) * 2.0 + 1.0
    labels = rng.integers(0, 3, size=u)
    return X, y, c, Vc, Z, labels


def test_oracle_reproduces_the_algebra_of_margeff_per_group():
    X, y, c, Vc, Z, labels = _data()
    sigma = float(X.shape[1])
    which = [1, 2, 3, 4]
    G = 3
    ysd = y.std(ddof=1)
    ame, cov, D = ge_numpy(X, y, c, sigma, which, Z, labels, Vc)
    assert ame.shape == (G, 4) and cov.shape == (12, 12) and D.shape == (23, 4)
    S = np.empty((12, X.shape[0]))
    for g in range(G):
        S[[jj * G + g for jj in range(4)]] = margeff_cols_numpy(X, sigma, which, Z, labels == g)
    f = np.repeat([1.0, math.sqrt(2.0), 1.0, 1.0], G)
    ame_alg = ysd * (S @ c).reshape(4, G).T
    cov_alg = (S @ Vc @ S.T) * np.outer(f, f)
    assert np.max(np.abs(ame - ame_alg)) <= 1e-12 * np.max(np.abs(ame_alg))
    assert np.max(np.abs(cov - cov_alg)) <= 1e-12 * np.max(np.abs(cov_alg))
    # the group means of the pointwise effects, and a positive semi-definite covariance with the factor 2 on its diagonal
    for g in range(G):
        np.testing.assert_allclose(ame[g], D[labels == g].mean(axis=0), rtol=1e-12)
    assert np.linalg.eigvalsh(cov).min() >= -1e-12 * np.abs(cov).max()
    Wb = margeff_cols_numpy(X, sigma, [2], Z, labels == 1)[0]
    assert abs(cov[1 * G + 1, 1 * G + 1] - 2.0 * Wb @ Vc @ Wb) <= 1e-12 * cov[1 * G + 1, 1 * G + 1]
    assert ge_numpy(X, y, c, sigma, which, Z, labels)[1] is None


# --------------------------------------------------------------------------
# the Wald statistic and the chi-square tail
# --------------------------------------------------------------------------
def test_wald_on_values_known_in_closed_form():
    from bigkrls_amd.api import _wald
    stat, df, pv = _wald([1.0, 3.0, 6.0], np.eye(3), 0)
    assert abs(stat - 38.0 / 3.0) <= 1e-14 * 38.0 / 3.0 and df == 2
    assert abs(pv - math.exp(-19.0 / 3.0)) <= 1e-13 * math.exp(-19.0 / 3.0)
    # the statistic does not depend on the reference
    for ref in (1, 2):
        s2, d2, _ = _wald([1.0, 3.0, 6.0], np.eye(3), ref)
        assert abs(s2 - stat) <= 1e-13 * stat and d2 == 2


def test_wald_singular_covariance_lowers_df():
    from bigkrls_amd.api import _wald
    Sigma = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]])   # theta_0 - theta_1 has variance 0
    stat, df, pv = _wald([1.0, 3.0, 6.0], Sigma, 0)
    assert df == 1 and np.isfinite(stat) and 0.0 <= pv <= 1.0
    assert _wald([1.0, 3.0], np.zeros((2, 2)), 0)[:2] == (0.0, 0)
    stat, df, pv = _wald([2.5], [[1.0]], 0)
    assert stat == 0.0 and df == 0 and math.isnan(pv)
    with pytest.raises(ValueError):
        _wald([1.0, 2.0], np.eye(3), 0)
    with pytest.raises(ValueError):
        _wald([1.0, 2.0], np.eye(2), 2)


def test_chi_square_tail():
    from bigkrls_amd.api import _chi2_sf
    for x in (0.0, 0.3, 1.0, 7.5, 40.0, 900.0):
        assert _chi2_sf(x, 2) == math.exp(-x / 2)
    assert abs(_chi2_sf(3.841458820694124, 1) - 0.05) <= 1e-12
    assert abs(_chi2_sf(5.991464547107979, 2) - 0.05) <= 1e-12
    assert abs(_chi2_sf(18.307038053275146, 10) - 0.05) <= 1e-12
    # df = 1: erfc(sqrt(x / 2)), on both branches (series below df / 2 + 1, continued fraction above)
    for x in (0.01, 0.5, 2.9, 3.1, 25.0, 200.0):
        want = math.erfc(math.sqrt(x / 2.0))
        assert abs(_chi2_sf(x, 1) - want) <= 1e-12 * max(want, 1e-300) + 1e-15
    for df in (1, 3, 7, 50):
        assert _chi2_sf(1e6, df) == 0.0 and _chi2_sf(1e300, df) == 0.0 and _chi2_sf(float("inf"), df) == 0.0
        assert _chi2_sf(0.0, df) == 1.0
    assert math.isnan(_chi2_sf(1.0, 0)) and math.isnan(_chi2_sf(float("nan"), 3))


# --------------------------------------------------------------------------
# the C ABI and its ctypes table; the export
# --------------------------------------------------------------------------
def _header_arity(name):
    src = open(os.path.join(ROOT, "include", "bigkrls.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} not declared in include/bigkrls.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,arity", [("bigkrls_dev_kernel_contract_grouped", 16), ("bigkrls_group_effects", 21)])
def test_header_declares_and_ctypes_table_matches(name, arity):
    from bigkrls_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name]) == _header_arity(name) == arity


def test_public_api_exports_group_effects():
    import bigkrls_amd as bk
    from bigkrls_amd import ops
    assert callable(bk.group_effects) and "group_effects" in bk.__all__
    assert callable(ops.bKernelContractGrouped)


# --------------------------------------------------------------------------
# the labelling rule
# --------------------------------------------------------------------------
def test_bins_labelling_rule_on_a_column_with_ties():
    from bigkrls_amd.api import _group_labels
    col = np.array([1.0, 1.0, 1.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    nd = np.column_stack([np.arange(8.0), col])
    groups, labels = _group_labels(2, nd, 4)
    # quartile edges 1, 1, 1.5, 3.25, 5: bin (1, 1.5] holds no value and is dropped
    edges = np.quantile(col, np.linspace(0, 1, 5))
    assert np.array_equal(edges, [1.0, 1.0, 1.5, 3.25, 5.0])
    raw = np.digitize(col, edges[1:-1], right=True)
    assert np.array_equal(raw, [0, 0, 0, 0, 2, 2, 3, 3])
    assert groups == [(1.0, 1.0), (1.5, 3.25), (3.25, 5.0)]
    assert labels.dtype == np.int64 and np.array_equal(labels, [0, 0, 0, 0, 1, 1, 2, 2])
    # without bins: the distinct values; labels as an array: np.unique
    groups, labels = _group_labels(2, nd, None)
    assert groups == [1.0, 2.0, 3.0, 4.0, 5.0] and np.array_equal(labels, [0, 0, 0, 0, 1, 2, 3, 4])
    groups, labels = _group_labels(np.array(["b", "a", "b", "c", "a", "a", "c", "b"]), nd, None)
    assert groups == ["a", "b", "c"] and np.array_equal(labels, [1, 0, 1, 2, 0, 0, 2, 1])


# --------------------------------------------------------------------------
# validation happens in Python, before any native call (no GPU here)
# --------------------------------------------------------------------------
def _object(n=40, p=3, vcov=True):
    from bigkrls_amd.api import BigKRLS
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, p))
    X[:, 1] = (rng.random(n) < 0.4).astype(np.float64) * 2.0 + 1.0      # binary, values 1 and 3
    y = rng.standard_normal(n)
    return BigKRLS({"X": X, "y": y, "coeffs": rng.standard_normal(n), "sigma": float(p), "which.derivatives": None,
                    "vcov.est.c": np.eye(n) if vcov else None, "has.big.matrices": False,
                    "xlabs": [f"x{i + 1}" for i in range(p)]})


@pytest.fixture
def no_native(monkeypatch):
    from bigkrls_amd import api

    def boom(*a, **k):
        raise AssertionError("native call reached")
    monkeypatch.setattr(api, "_call_native", boom)
    monkeypatch.setattr(api, "default_context", boom)


LAB = np.arange(40) % 3


def test_valid_arguments_reach_the_native_call(no_native):
    import bigkrls_amd as bk
    for kw in (dict(by=LAB), dict(by=2), dict(by=1, bins=4), dict(by=LAB, reference=2),
               dict(by=LAB[:5], newdata=_object()["X"][:5]), dict(by=1, bins=4, reference=None)):
        with pytest.raises(AssertionError, match="native call reached"):
            bk.group_effects(_object(), **kw)
    with pytest.raises(AssertionError, match="native call reached"):       # without a variance form the object is enough
        bk.group_effects(_object(vcov=False), LAB)


def test_not_a_bigkrls_object_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(TypeError):
        bk.group_effects({"X": np.zeros((3, 2))}, [0, 1, 0])


def test_newdata_checks_are_those_of_marginal_effects(no_native):
    import bigkrls_amd as bk
    obj = _object()
    with pytest.raises(ValueError, match="ncol"):
        bk.group_effects(obj, [0] * 5, newdata=np.zeros((5, 4)))
    with pytest.raises(ValueError, match="missing or infinite"):
        bk.group_effects(obj, [0] * 5, newdata=np.full((5, 3), np.nan))
    with pytest.raises(ValueError, match="no rows"):
        bk.group_effects(obj, [], newdata=np.zeros((0, 3)))
    nd = obj["X"][:6].copy()
    nd[2, 1] = 2.0
    with pytest.raises(ValueError, match=r"newdata column 2 is binary.*\(1, 3\)"):
        bk.group_effects(obj, [0] * 6, newdata=nd)
    with pytest.raises(AssertionError, match="native call reached"):       # column 2 not selected: its values are free
        bk.group_effects(obj, [0] * 6, newdata=nd, which_derivatives=[1, 3])
    for bad in (0, 4, [], [1, 5]):
        with pytest.raises(ValueError, match="which.derivatives must index columns of X"):
            bk.group_effects(obj, LAB, which_derivatives=bad)


def test_vcov_choice_and_sharded_objects(no_native):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match="vcov must be"):
        bk.group_effects(_object(), LAB, vcov="sparse")
    with pytest.raises(ValueError, match="no vcov.est.Q"):
        bk.group_effects(_object(), LAB, vcov="factors")
    with pytest.raises(ValueError, match="no vcov.est.c"):
        bk.group_effects(_object(vcov=False), LAB, vcov="dense")
    obj = _object()
    obj["rows"] = (0, 20)
    obj["vcov.est.c.cols"] = None
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        bk.group_effects(obj, LAB)


def test_bad_by_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    with pytest.raises(ValueError, match=r"one label per row of newdata \(40\)"):
        bk.group_effects(obj, LAB[:39])
    with pytest.raises(ValueError, match=r"one label per row of newdata \(5\)"):
        bk.group_effects(obj, LAB, newdata=obj["X"][:5])
    with pytest.raises(ValueError, match="one label per row"):
        bk.group_effects(obj, np.zeros((40, 2)))
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match="by must index a column of newdata"):
            bk.group_effects(obj, bad)
    with pytest.raises(ValueError, match="bins must be a positive integer"):
        bk.group_effects(obj, 1, bins=0)
    with pytest.raises(ValueError, match="bins applies only when by is a column index"):
        bk.group_effects(obj, LAB, bins=3)


def test_unknown_reference_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    with pytest.raises(ValueError, match="reference 3 is not one of the groups"):
        bk.group_effects(obj, LAB, reference=3)
    with pytest.raises(ValueError, match="reference 'a' is not one of the groups"):
        bk.group_effects(obj, LAB, reference="a")
    with pytest.raises(ValueError, match="is not one of the groups"):
        bk.group_effects(obj, 2, reference=2.0)          # the binary column holds 1 and 3
    with pytest.raises(AssertionError, match="native call reached"):
        bk.group_effects(obj, 2, reference=3.0)


def test_too_many_average_effects_raises_naming_both_numbers(no_native):
    import bigkrls_amd as bk
    obj = _object(n=1400)
    with pytest.raises(ValueError, match=r"1400 groups x 3 columns = 4200 "):
        bk.group_effects(obj, np.arange(1400))
    with pytest.raises(AssertionError, match="native call reached"):       # 1400 x 2 = 2800 fits
        bk.group_effects(obj, np.arange(1400), which_derivatives=[1, 3])
