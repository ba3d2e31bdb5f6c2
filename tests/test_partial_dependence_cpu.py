"""CPU checks of partial_dependence(): a numpy restatement of the factorised algebra (also used by
tests/test_gpu_partial_dependence.py) against the definition -- the mean over the rewritten reference rows of
K(Zmod, X) c and the mean of K(Zmod_v, X) Vc K(Zmod_v', X)' --, the C ABI's two new entry points and their ctypes
arity, the export, and the Python validation, which raises before any native call."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------
# numpy restatement of the algebra (include/bigkrls.h, bigkrls_partial_dependence)
# --------------------------------------------------------------------------
def loo_colsums_numpy(A, B, sigma, cols, dtype=np.float64):
    """out[l, jj] = sum_i exp(-(||A_i - B_l||^2 - (A[i,c] - B[l,c])^2) / sigma), c = cols[jj]: the direct sum over
    the other columns, in `dtype`."""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    out = np.empty((B.shape[0], len(cols)), dtype=dtype)
    for jj, c in enumerate(cols):
        keep = [k for k in range(A.shape[1]) if k != c]
        d2 = np.zeros((A.shape[0], B.shape[0]), dtype=dtype)
        for k in keep:
            d2 += (A[:, k][:, None] - B[:, k][None, :]) ** 2
        out[:, jj] = np.exp(-d2 / dtype(sigma)).sum(axis=0)
    return out


def pd_numpy(X, y, coeffs, sigma, which, grids, newdata=None, vcov_c=None, neffective=None):
    """partial_dependence() in numpy: (pd, se, cov), lists over the columns of `which` (1-based), in the original
    units; se and cov are None without vcov_c. neffective: the variance carries predict()'s factor
    sqrt(n / neffective) (R/bigKRLS.R:610-611 as the library implements it, bigkrls_predict)."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    Z = X if newdata is None else np.asarray(newdata, dtype=np.float64)
    u = Z.shape[0]
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    ym, ysd = float(np.mean(y)), float(np.std(y, ddof=1))
    Xs, Zs = (X - m) / s, (Z - m) / s
    c = np.asarray(coeffs, dtype=np.float64).ravel()
    cols = [j - 1 for j in which]
    M = loo_colsums_numpy(Zs, Xs, sigma, cols)
    f = 1.0 if not neffective else np.sqrt(n / float(neffective))
    pds, ses, covs = [], [], []
    for jj, j in enumerate(cols):
        vs = (np.asarray(grids[jj], dtype=np.float64) - m[j]) / s[j]
        A = M[:, jj][None, :] * np.exp(-(vs[:, None] - Xs[:, j][None, :]) ** 2 / sigma) / u      # G x n
        pds.append(ym + ysd * (A @ c))
        if vcov_c is not None:
            cov = f * (A @ np.asarray(vcov_c, dtype=np.float64) @ A.T)
            covs.append(cov)
            ses.append(np.sqrt(np.maximum(np.diag(cov), 0.0)))
    return pds, (ses if vcov_c is not None else None), (covs if vcov_c is not None else None)


def _kernel(A, B, sigma):
    d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2)
    return np.exp(-d2 / sigma)


def test_restatement_equals_the_definition():
    rng = np.random.default_rng(17)
    n, p, u = 40, 3, 23
    X = rng.standard_normal((n, p)) * np.array([1.0, 1.0, 3.0]) + np.array([0.0, 0.0, 5.0])
    X[:, 1] = (rng.random(n) < 0.4).astype(np.float64) * 2.0 + 1.0       # binary, values 1 and 3
    y = rng.standard_normal(n) * 2.0 + 0.7
    c = rng.standard_normal(n)
    Gm = rng.standard_normal((n, n))
    Vc = Gm @ Gm.T / n
    sigma = float(p)
    Z = rng.standard_normal((u, p)) * np.array([1.0, 1.0, 3.0]) + np.array([0.0, 2.0, 5.0])
    which = [3, 2, 1]
    grids = [np.linspace(X[:, 2].min(), X[:, 2].max(), 4), np.array([1.0, 3.0]), np.array([-0.3, 0.0, 1.1, 0.5, 2.0])]
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    ym, ysd = y.mean(), y.std(ddof=1)
    Xs = (X - m) / s
    for newdata in (None, Z):
        R = X if newdata is None else newdata
        pds, ses, covs = pd_numpy(X, y, c, sigma, which, grids, newdata=newdata, vcov_c=Vc)
        for jj, w in enumerate(which):
            j = w - 1
            Ks = []
            for v in grids[jj]:
                Zmod = R.copy()
                Zmod[:, j] = v
                Ks.append(_kernel((Zmod - m) / s, Xs, sigma))
            pd_def = np.array([ym + ysd * (K @ c).mean() for K in Ks])
            cov_def = np.array([[(Ka @ Vc @ Kb.T).sum() / R.shape[0] ** 2 for Kb in Ks] for Ka in Ks])
            np.testing.assert_allclose(pds[jj], pd_def, rtol=0, atol=1e-12 * np.abs(pd_def).max())
            np.testing.assert_allclose(covs[jj], cov_def, rtol=0, atol=1e-12 * np.abs(cov_def).max())
            np.testing.assert_allclose(ses[jj], np.sqrt(np.diag(cov_def)), rtol=1e-10)
    # predict()'s factor on the variance
    _, ses_n, covs_n = pd_numpy(X, y, c, sigma, which, grids, vcov_c=Vc, neffective=10.0)
    _, _, covs_1 = pd_numpy(X, y, c, sigma, which, grids, vcov_c=Vc)
    np.testing.assert_allclose(covs_n[0], covs_1[0] * np.sqrt(n / 10.0), rtol=1e-14)
    assert pd_numpy(X, y, c, sigma, which, grids)[1] is None


# --------------------------------------------------------------------------
# the C ABI and its ctypes table
# --------------------------------------------------------------------------
def _header_arity(name):
    src = open(os.path.join(ROOT, "include", "bigkrls.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} not declared in include/bigkrls.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,arity", [("bigkrls_dev_kernel_loo_colsums", 13), ("bigkrls_partial_dependence", 22)])
def test_header_declares_and_ctypes_table_matches(name, arity):
    from bigkrls_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name]) == _header_arity(name) == arity


def test_public_api_exports_partial_dependence():
    import bigkrls_amd as bk
    assert callable(bk.partial_dependence) and "partial_dependence" in bk.__all__


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
        bk.partial_dependence(_object(), newdata=np.zeros((5, 4)))


def test_bad_which_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    for bad in ([0], [4], [], [1, 5]):
        with pytest.raises(ValueError, match="which.derivatives"):
            bk.partial_dependence(obj, which=bad)


def test_bad_value_in_binary_grid_raises_naming_the_column(no_native):
    import bigkrls_amd as bk
    obj = _object()
    with pytest.raises(ValueError, match=r"column 2 is binary.*\(1, 3\)"):
        bk.partial_dependence(obj, which=[1, 2], grid=[np.array([0.0, 0.5]), np.array([1.0, 2.0])])
    # the two training values pass up to the native call
    with pytest.raises(AssertionError, match="native call reached"):
        bk.partial_dependence(obj, which=[1, 2], grid=[np.array([0.0, 0.5]), np.array([3.0, 1.0])])
    with pytest.raises(ValueError, match="one array per column"):
        bk.partial_dependence(obj, which=[1, 2], grid=[np.array([0.0, 0.5])])


def test_grid_of_one_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match="grid must be at least 2"):
        bk.partial_dependence(_object(), grid=1)


def test_not_a_bigkrls_object_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(TypeError):
        bk.partial_dependence({"X": np.zeros((3, 2))})


def test_se_without_any_vcov_form_raises(no_native):
    import bigkrls_amd as bk
    obj = _object(vcov=False)
    with pytest.raises(ValueError, match="vcov.est=TRUE"):
        bk.partial_dependence(obj)
    with pytest.raises(AssertionError, match="native call reached"):     # without SEs the object is enough
        bk.partial_dependence(obj, se=False)


def test_multi_gpu_object_with_sharded_matrix_only_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    obj["rows"] = (0, 20)
    obj["vcov.est.c.cols"] = None
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        bk.partial_dependence(obj)
