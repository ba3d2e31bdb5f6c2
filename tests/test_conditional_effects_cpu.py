"""CPU checks of conditional_effects(): a numpy restatement of the factorised algebra (also used by
tests/test_gpu_conditional_effects.py) against the literal definition -- the derivative, or the first difference, of the
fitted surface on the reference rows with the moderator's column overwritten, averaged, and a'Va for its weights --, the
C ABI's two new entry points and their ctypes arity, the export, and the Python validation, which raises before any
native call."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------
# numpy restatement of the algebra (include/bigkrls.h, bigkrls_conditional_effects)
# --------------------------------------------------------------------------
def loo_moments_numpy(A, B, sigma, entries, dtype=np.float64, with_scale=False):
    """out[l, e] = sum_i wgt exp(-d2_left(i, l) / sigma) for entries (kind, c, j): the direct sum over the columns that
    stay in the distance, in `dtype`. with_scale: also sum_i |wgt| exp(.), the scale an error of the sum is relative
    to."""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    p = A.shape[1]
    sq = [(A[:, k][:, None] - B[:, k][None, :]) ** 2 for k in range(p)]
    out = np.empty((B.shape[0], len(entries)), dtype=dtype)
    scale = np.empty_like(out)
    for e, (kind, c, j) in enumerate(entries):
        left_out = {c, j} if kind == 2 else {c}
        d2 = np.zeros((A.shape[0], B.shape[0]), dtype=dtype)
        for k in range(p):
            if k not in left_out:
                d2 += sq[k]
        ex = np.exp(-d2 / dtype(sigma))
        w = (B[:, j][None, :] - A[:, j][:, None]) if kind == 1 else np.ones_like(ex)
        out[:, e] = (w * ex).sum(axis=0)
        scale[:, e] = (np.abs(w) * ex).sum(axis=0)
    return (out, scale) if with_scale else out


def ce_numpy(X, y, coeffs, sigma, pairs, grids, newdata=None, vcov_c=None):
    """conditional_effects() in numpy: (ce, se, cov, contrast, se_contrast) -- the first three lists over `pairs`
    (1-based (effect j, moderator k)), the last two arrays over them --, in the original units; se, cov and
    se_contrast are None without vcov_c."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    Z = X if newdata is None else np.asarray(newdata, dtype=np.float64)
    u = Z.shape[0]
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    ysd = float(np.std(y, ddof=1))
    Xs, Zs = (X - m) / s, (Z - m) / s
    c = np.asarray(coeffs, dtype=np.float64).ravel()
    isbin = [np.unique(X[:, j]).size == 2 for j in range(p)]
    ces, ses, covs, con, secon = [], [], [], [], []
    for idx, (j1, k1) in enumerate(pairs):
        j, k = j1 - 1, k1 - 1
        vs = (np.asarray(grids[idx], dtype=np.float64) - m[k]) / s[k]
        E = np.exp(-(vs[:, None] - Xs[:, k][None, :]) ** 2 / sigma)                           # G x n
        if j == k:
            M0 = loo_moments_numpy(Zs, Xs, sigma, [(0, k, 0)])[:, 0]
            A = (2.0 / (sigma * u)) * E * (Xs[:, j][None, :] - vs[:, None]) * M0[None, :]
            f = 1.0
        elif not isbin[j]:
            M1 = loo_moments_numpy(Zs, Xs, sigma, [(1, k, j)])[:, 0]
            A = (2.0 / (sigma * u)) * E * M1[None, :]
            f = 1.0
        else:
            M2 = loo_moments_numpy(Zs, Xs, sigma, [(2, k, j)])[:, 0]
            z0, z1 = (X[:, j].min() - m[j]) / s[j], (X[:, j].max() - m[j]) / s[j]
            d = (np.exp(-(z1 - Xs[:, j]) ** 2 / sigma) - np.exp(-(z0 - Xs[:, j]) ** 2 / sigma)) / (z1 - z0)
            A = E * d[None, :] * M2[None, :] / u
            f = 2.0
        ce = ysd * (A @ c) / s[j]
        ces.append(ce)
        con.append(ce[-1] - ce[0])
        if vcov_c is not None:
            cov = f * (A @ np.asarray(vcov_c, dtype=np.float64) @ A.T) / s[j] ** 2
            covs.append(cov)
            ses.append(np.sqrt(np.maximum(np.diag(cov), 0.0)))
            secon.append(np.sqrt(max(cov[0, 0] + cov[-1, -1] - 2.0 * cov[0, -1], 0.0)))
    if vcov_c is None:
        return ces, None, None, np.array(con), None
    return ces, ses, covs, np.array(con), np.array(secon)


def _kernel(A, B, sigma):
    d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2)
    return np.exp(-d2 / sigma)


def _weights_by_definition(X, R, sigma, j, k, v):
    """a (n) with CE_jk(v) = sd(y) / sd(x_j) a'c, literally: on the rows R with column k set to v, the weights of the
    mean derivative in x_j (continuous) or of the mean first difference between the two training values (binary), in
    standardised units."""
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    Xs = (X - m) / s
    u = R.shape[0]
    Zmod = R.copy()
    Zmod[:, k] = v
    if np.unique(X[:, j]).size == 2:
        Z1, Z0 = Zmod.copy(), Zmod.copy()
        Z1[:, j], Z0[:, j] = X[:, j].max(), X[:, j].min()
        z1, z0 = (X[:, j].max() - m[j]) / s[j], (X[:, j].min() - m[j]) / s[j]
        return (_kernel((Z1 - m) / s, Xs, sigma) - _kernel((Z0 - m) / s, Xs, sigma)).sum(axis=0) / ((z1 - z0) * u)
    Zs = (Zmod - m) / s
    K = _kernel(Zs, Xs, sigma)                                    # u x n
    return (2.0 / (sigma * u)) * ((Xs[:, j][None, :] - Zs[:, j][:, None]) * K).sum(axis=0)


def _data():
    rng = np.random.default_rng(23)
    n, p, u = 40, 4, 23
    X = rng.standard_normal((n, p)) * np.array([1.0, 1.0, 3.0, 0.5]) + np.array([0.0, 0.0, 5.0, -1.0])
    X[:, 1] = (rng.random(n) < 0.4).astype(np.float64) * 2.0 + 1.0       # binary, values 1 and 3
    y = rng.standard_normal(n) * 2.0 + 0.7
    c = rng.standard_normal(n)
    Gm = rng.standard_normal((n, n))
    Vc = Gm @ Gm.T / n
    Z = rng.standard_normal((u, p)) * np.array([1.0, 1.0, 3.0, 0.5]) + np.array([0.0, 2.0, 5.0, -1.0])
    Z[:, 1] = (rng.random(u) < 0.5).astype(np.float64) * 2.0 + 1.0
    return X, y, c, Vc, Z


# the four pair types: (continuous, continuous), (binary, continuous), (continuous, binary), (j, j)
PAIRS = [(1, 3), (2, 1), (1, 2), (3, 3), (4, 1)]


def test_restatement_equals_the_definition():
    X, y, c, Vc, Z = _data()
    n, p = X.shape
    sigma = float(p)
    grids = [np.linspace(X[:, 2].min(), X[:, 2].max(), 4), np.array([-0.3, 0.0, 1.1, 0.5, 2.0]), np.array([1.0, 3.0]),
             np.linspace(X[:, 2].min(), X[:, 2].max(), 3), np.array([0.2, -1.5])]
    s = X.std(axis=0, ddof=1)
    ysd = y.std(ddof=1)
    for newdata in (None, Z):
        R = X if newdata is None else newdata
        ces, ses, covs, con, secon = ce_numpy(X, y, c, sigma, PAIRS, grids, newdata=newdata, vcov_c=Vc)
        for idx, (j1, k1) in enumerate(PAIRS):
            j, k = j1 - 1, k1 - 1
            f = 2.0 if np.unique(X[:, j]).size == 2 else 1.0
            a = np.array([_weights_by_definition(X, R, sigma, j, k, v) for v in grids[idx]])     # G x n
            ce_def = ysd * (a @ c) / s[j]
            cov_def = f * (a @ Vc @ a.T) / s[j] ** 2
            np.testing.assert_allclose(ces[idx], ce_def, rtol=0, atol=1e-12 * np.abs(ce_def).max())
            np.testing.assert_allclose(covs[idx], cov_def, rtol=0, atol=1e-12 * np.abs(cov_def).max())
            np.testing.assert_allclose(ses[idx], np.sqrt(np.diag(cov_def)), rtol=1e-10)
            assert abs(con[idx] - (ce_def[-1] - ce_def[0])) <= 1e-12 * np.abs(ce_def).max()
            var_con = cov_def[0, 0] + cov_def[-1, -1] - 2.0 * cov_def[0, -1]
            assert abs(secon[idx] ** 2 - var_con) <= 1e-10 * np.abs(cov_def).max()
    assert ce_numpy(X, y, c, sigma, PAIRS, grids)[1] is None


def test_continuous_effect_is_the_derivative_of_the_rewritten_surface():
    """The definition itself against a central difference of the fitted surface in x_j on the rewritten rows (k != j),
    and of the partial-dependence curve in v (k == j)."""
    X, y, c, _, Z = _data()
    sigma = float(X.shape[1])
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    Xs = (X - m) / s

    def mean_surface(R):
        return (_kernel((R - m) / s, Xs, sigma) @ c).mean()
    h = 1e-5
    for (j, k, v) in ((0, 2, 4.0), (2, 2, 6.0)):
        a = _weights_by_definition(X, Z, sigma, j, k, v)
        if j != k:
            Zmod = Z.copy()
            Zmod[:, k] = v
            up, dn = Zmod.copy(), Zmod.copy()
            up[:, j] += h * s[j]
            dn[:, j] -= h * s[j]
        else:
            up, dn = Z.copy(), Z.copy()
            up[:, k], dn[:, k] = v + h * s[k], v - h * s[k]
        fd = (mean_surface(up) - mean_surface(dn)) / (2.0 * h)
        assert abs(a @ c - fd) <= 1e-8 * max(abs(fd), 1.0)


# --------------------------------------------------------------------------
# the C ABI and its ctypes table
# --------------------------------------------------------------------------
def _header_arity(name):
    src = open(os.path.join(ROOT, "include", "bigkrls.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} not declared in include/bigkrls.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,arity", [("bigkrls_dev_kernel_loo_moments", 13), ("bigkrls_conditional_effects", 21)])
def test_header_declares_and_ctypes_table_matches(name, arity):
    from bigkrls_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name]) == _header_arity(name) == arity


def test_public_api_exports_conditional_effects():
    import bigkrls_amd as bk
    from bigkrls_amd import ops
    assert callable(bk.conditional_effects) and "conditional_effects" in bk.__all__
    assert callable(ops.bKernelLooMoments)


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


def test_wrong_ncol_of_newdata_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match="ncol"):
        bk.conditional_effects(_object(), 1, 3, newdata=np.zeros((5, 4)))
    with pytest.raises(ValueError, match="missing or infinite"):
        bk.conditional_effects(_object(), 1, 3, newdata=np.full((5, 3), np.nan))


def test_bad_columns_raise(no_native):
    import bigkrls_amd as bk
    obj = _object()
    for bad in (0, 4, [], [1, 5]):
        with pytest.raises(ValueError, match="effect must index columns of X"):
            bk.conditional_effects(obj, bad, 3)
        with pytest.raises(ValueError, match="along must index columns of X"):
            bk.conditional_effects(obj, 1, bad)


def test_binary_diagonal_and_repeated_pair_raise_naming_the_pair(no_native):
    import bigkrls_amd as bk
    obj = _object()
    with pytest.raises(ValueError, match=r"pair \(2, 2\) is not defined: column 2 is binary"):
        bk.conditional_effects(obj, [1, 2], [2, 3])
    with pytest.raises(ValueError, match=r"pair \(1, 3\) is given more than once"):
        bk.conditional_effects(obj, [1, 1], 3)
    with pytest.raises(AssertionError, match="native call reached"):     # (1, 1) on a continuous column is defined
        bk.conditional_effects(obj, 1, [1, 2, 3])


def test_bad_value_in_binary_moderator_grid_raises_naming_the_pair(no_native):
    import bigkrls_amd as bk
    obj = _object()
    with pytest.raises(ValueError, match=r"pair \(1, 2\): column 2 is binary.*\(1, 3\)"):
        bk.conditional_effects(obj, 1, [3, 2], grid=[np.array([0.0, 0.5]), np.array([1.0, 2.0])])
    # the two training values pass up to the native call
    with pytest.raises(AssertionError, match="native call reached"):
        bk.conditional_effects(obj, 1, [3, 2], grid=[np.array([0.0, 0.5]), np.array([3.0, 1.0])])
    with pytest.raises(ValueError, match="one array per pair"):
        bk.conditional_effects(obj, 1, [3, 2], grid=[np.array([0.0, 0.5])])
    with pytest.raises(ValueError, match=r"grid of pair \(1, 3\) must hold at least one finite value"):
        bk.conditional_effects(obj, 1, 3, grid=[np.array([0.0, np.inf])])


def test_grid_of_one_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match="grid must be at least 2"):
        bk.conditional_effects(_object(), 1, 3, grid=1)


def test_not_a_bigkrls_object_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(TypeError):
        bk.conditional_effects({"X": np.zeros((3, 2))}, 1, 2)


def test_se_without_any_vcov_form_raises(no_native):
    import bigkrls_amd as bk
    obj = _object(vcov=False)
    with pytest.raises(ValueError, match="vcov.est=TRUE"):
        bk.conditional_effects(obj, 1, 3)
    with pytest.raises(AssertionError, match="native call reached"):     # without SEs the object is enough
        bk.conditional_effects(obj, 1, 3, se=False)
    with pytest.raises(ValueError, match="vcov must be"):
        bk.conditional_effects(_object(), 1, 3, vcov="sparse")


def test_multi_gpu_object_with_sharded_matrix_only_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    obj["rows"] = (0, 20)
    obj["vcov.est.c.cols"] = None
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        bk.conditional_effects(obj, 1, 3)
