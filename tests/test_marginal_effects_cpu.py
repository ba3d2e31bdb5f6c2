"""CPU checks of marginal_effects(): the C ABI declares both new entry points and the ctypes table matches their
arity, the Python validation raises before any native call, and the definition itself -- restated here in numpy
with the shifted test kernels Kn1 / Kn0 built literally -- reproduces the reference's marginal effects
(orc.derivmat_literal, src/bigderiv_v3.cpp) when the new points are the training rows."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------
# numpy restatement of the definition (also used by tests/test_gpu_marginal_effects.py)
# --------------------------------------------------------------------------
def _kernel(A, B, sigma):
    d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2)
    return np.exp(-d2 / sigma)


def me_std(Xs, Zs, c, sigma, V, binary, cols):
    """Standardised-unit D (u x |J|) and var (|J|; None without V) at the rows Zs. `binary[j]`: (z0, z1) of a binary
    training column, None otherwise. Kn1 / Kn0 are rebuilt with column j of Zs replaced."""
    u = Zs.shape[0]
    Kn = _kernel(Zs, Xs, sigma)
    D = np.empty((u, len(cols)))
    var = np.empty(len(cols)) if V is not None else None
    for jj, j in enumerate(cols):
        if binary[j] is not None:
            z0, z1 = binary[j]
            Z1, Z0 = Zs.copy(), Zs.copy()
            Z1[:, j], Z0[:, j] = z1, z0
            Kd = _kernel(Z1, Xs, sigma) - _kernel(Z0, Xs, sigma)
            D[:, jj] = Kd @ c / (z1 - z0)
            if V is not None:
                a = Kd.sum(axis=0)
                var[jj] = 2.0 / ((z1 - z0) ** 2 * u ** 2) * (a @ V @ a)
        else:
            L = (Zs[:, j][:, None] - Xs[:, j][None, :]) * Kn
            D[:, jj] = (-2.0 / sigma) * (L @ c)
            if V is not None:
                s = L.sum(axis=0)
                var[jj] = 4.0 / (sigma ** 2 * u ** 2) * (s @ V @ s)
    return D, var


def me_numpy(X, y, coeffs, sigma, newdata, vcov_c=None, which=None):
    """marginal_effects() in numpy: (derivatives, avgderivatives, var.avgderivatives) in the original units."""
    X = np.asarray(X, dtype=np.float64)
    Z = np.asarray(newdata, dtype=np.float64)
    n, p = X.shape
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    ysd = float(np.std(y, ddof=1))
    Xs, Zs = (X - m) / s, (Z - m) / s
    cols = [j - 1 for j in which] if which is not None else list(range(p))
    binary = [((X[:, j].min() - m[j]) / s[j], (X[:, j].max() - m[j]) / s[j]) if np.unique(X[:, j]).size == 2 else None
              for j in range(p)]
    V = None if vcov_c is None else np.asarray(vcov_c) / ysd ** 2
    D, var = me_std(Xs, Zs, np.asarray(coeffs, dtype=np.float64), sigma, V, binary, cols)
    g = np.array([ysd / s[j] for j in cols])
    D = D * g
    return D, D.mean(axis=0), None if var is None else var * g ** 2


# --------------------------------------------------------------------------
# the C ABI and its ctypes table
# --------------------------------------------------------------------------
def _header_arity(name):
    src = open(os.path.join(ROOT, "include", "bigkrls.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} not declared in include/bigkrls.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", ["bigkrls_dev_kernel_contract", "bigkrls_marginal_effects"])
def test_header_declares_and_ctypes_table_matches(name):
    from bigkrls_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name]) == _header_arity(name)


def test_public_api_exports_marginal_effects():
    import bigkrls_amd as bk
    assert callable(bk.marginal_effects) and "marginal_effects" in bk.__all__
    assert callable(bk.ops.bKernelContract)


# --------------------------------------------------------------------------
# validation happens in Python, before any native call (no GPU here)
# --------------------------------------------------------------------------
def _object(n=40, p=3):
    from bigkrls_amd.api import BigKRLS
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, p))
    X[:, 1] = (rng.random(n) < 0.4).astype(np.float64) * 2.0 + 1.0      # binary, values 1 and 3
    y = rng.standard_normal(n)
    return BigKRLS({"X": X, "y": y, "coeffs": rng.standard_normal(n), "sigma": float(p), "which.derivatives": None,
                    "vcov.est.c": np.eye(n), "has.big.matrices": False, "xlabs": [f"x{i + 1}" for i in range(p)]})


@pytest.fixture
def no_native(monkeypatch):
    from bigkrls_amd import api

    def boom(*a, **k):
        raise AssertionError("native call reached")
    monkeypatch.setattr(api, "_call_native", boom)
    monkeypatch.setattr(api, "default_context", boom)


def test_wrong_ncol_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    with pytest.raises(ValueError, match="ncol"):
        bk.marginal_effects(obj, np.zeros((5, 4)))


def test_bad_binary_value_raises_naming_the_column(no_native):
    import bigkrls_amd as bk
    obj = _object()
    nd = obj["X"][:4].copy()
    nd[2, 1] = 2.0                                    # neither 1 nor 3
    with pytest.raises(ValueError, match="column 2"):
        bk.marginal_effects(obj, nd)
    # the same column outside which_derivatives is not differentiated: no error up to the native call
    with pytest.raises(AssertionError, match="native call reached"):
        bk.marginal_effects(obj, nd, which_derivatives=[1, 3])


def test_bad_which_derivatives_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    for bad in ([0], [4], [], [1, 5]):
        with pytest.raises(ValueError, match="which.derivatives"):
            bk.marginal_effects(obj, obj["X"][:3], which_derivatives=bad)


def test_multi_gpu_object_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    obj["rows"] = (0, 20)
    obj["vcov.est.c.cols"] = None
    with pytest.raises(NotImplementedError):
        bk.marginal_effects(obj, obj["X"][:3])


def test_not_a_bigkrls_object_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(TypeError):
        bk.marginal_effects({"X": np.zeros((3, 2))}, np.zeros((1, 2)))


# --------------------------------------------------------------------------
# the definition: in-sample identity with the reference's literal marginal effects
# --------------------------------------------------------------------------
def test_numpy_restatement_in_sample_equals_derivmat_literal():
    from oracle import krls_oracle as orc
    rng = np.random.default_rng(11)
    n, p = 60, 5
    X = rng.standard_normal((n, p))
    X[:, 1] = (rng.random(n) < 0.3).astype(np.float64)          # binary, 0/1
    X[:, 4] = np.where(rng.random(n) < 0.6, 2.0, -1.5)           # binary, other values
    y = np.sin(X @ np.linspace(0.2, 1.0, p)) + 0.1 * rng.standard_normal(n)
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    Xs = (X - m) / s
    sigma = float(p)
    K = orc.gauss_kernel_literal(Xs, sigma)
    c = rng.standard_normal(n)
    G = rng.standard_normal((n, n))
    V = G @ G.T / n                                              # any symmetric PSD V
    D_ref, var_ref = orc.derivmat_literal(Xs, K, V, c, sigma)
    binary = [(Xs[:, j].min(), Xs[:, j].max()) if np.unique(X[:, j]).size == 2 else None for j in range(p)]
    D, var = me_std(Xs, Xs, c, sigma, V, binary, list(range(p)))
    np.testing.assert_allclose(D, D_ref, rtol=0, atol=1e-12 * np.abs(D_ref).max())
    np.testing.assert_allclose(var, var_ref, rtol=1e-10)
    # and in the original units through me_numpy (vcov.est.c = sd(y)^2 V)
    ysd = np.std(y, ddof=1)
    Do, avg, varo = me_numpy(X, y, c, sigma, X, vcov_c=V * ysd ** 2)
    g = ysd / s
    np.testing.assert_allclose(Do, D_ref * g, rtol=0, atol=1e-12 * np.abs(D_ref * g).max())
    np.testing.assert_allclose(avg, (D_ref * g).mean(axis=0), rtol=0, atol=1e-12 * np.abs(D_ref * g).max())
    np.testing.assert_allclose(varo, var_ref * g ** 2, rtol=1e-10)
