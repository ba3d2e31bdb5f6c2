"""CPU checks of marginal_effects(se=True): the definition of the pointwise standard errors restated literally in numpy
(also used by tests/test_gpu_marginal_effects_se.py), its identity with var.avgderivatives at a single new point, the
per-training-row form of the binary first difference the device code uses, the C ABI's two new entries against the
ctypes table, and the Python checks that happen before any native call."""
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
def me_se_numpy(X, y, coeffs, sigma, newdata, vcov_c, which=None):
    """se.derivatives (u x |J|) in the original units: derivative[i, j] = g_ij' coeffs in standardised units, so its
    variance is g_ij' V g_ij with V = vcov.est.c / sd(y)^2, times 2 for binary columns (src/bigderiv_v3.cpp:85), and
    se = sqrt(var) sd(y) / sd(x_j). Kn and Kn1 - Kn0 are built as in me_std, the quadratic form row by row."""
    X = np.asarray(X, dtype=np.float64)
    Z = np.asarray(newdata, dtype=np.float64)
    n, p = X.shape
    u = Z.shape[0]
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    ysd = float(np.std(y, ddof=1))
    Xs, Zs = (X - m) / s, (Z - m) / s
    cols = [j - 1 for j in which] if which is not None else list(range(p))
    V = np.asarray(vcov_c, dtype=np.float64) / ysd ** 2
    Kn = _kernel(Zs, Xs, sigma)
    se = np.empty((u, len(cols)))
    for jj, j in enumerate(cols):
        if np.unique(X[:, j]).size == 2:
            z0, z1 = (X[:, j].min() - m[j]) / s[j], (X[:, j].max() - m[j]) / s[j]
            Z1, Z0 = Zs.copy(), Zs.copy()
            Z1[:, j], Z0[:, j] = z1, z0
            G = (_kernel(Z1, Xs, sigma) - _kernel(Z0, Xs, sigma)) / (z1 - z0)
            f = 2.0
        else:
            G = (-2.0 / sigma) * (Zs[:, j][:, None] - Xs[:, j][None, :]) * Kn
            f = 1.0
        var = np.array([G[i] @ V @ G[i] for i in range(u)])
        se[:, jj] = np.sqrt(f * var) * ysd / s[j]
    return se


def _data(n=60, p=4, seed=17):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    X[:, 2] = np.where(rng.random(n) < 0.45, 3.0, -1.0)            # binary, values -1 and 3
    y = np.sin(X @ np.linspace(0.3, 0.9, p)) + 0.1 * rng.standard_normal(n)
    c = rng.standard_normal(n)
    G = rng.standard_normal((n, n))
    return X, y, c, G @ G.T / n, rng


def test_single_point_se_squared_is_var_avgderivatives():
    X, y, c, V, rng = _data()
    sigma = float(X.shape[1])
    for hi in (3.0, -1.0):
        Z = rng.standard_normal((1, X.shape[1]))
        Z[0, 2] = hi
        se = me_se_numpy(X, y, c, sigma, Z, V)
        _, _, var = me_numpy(X, y, c, sigma, Z, vcov_c=V)
        np.testing.assert_allclose(se[0] ** 2, var, rtol=1e-12)
    which = [3, 1]
    se = me_se_numpy(X, y, c, sigma, Z, V, which=which)
    _, _, var = me_numpy(X, y, c, sigma, Z, vcov_c=V, which=which)
    np.testing.assert_allclose(se[0] ** 2, var, rtol=1e-12)


def test_per_training_row_form_equals_the_kernel_difference():
    """g_ij[k] = Kn[i,k] (r_i + t_i s_k) with the binary coefficients of csrc/margeff.hip (me_se_rt_kernel) is
    (Kn1 - Kn0)[i,k] / (z1 - z0), and with the continuous ones -(2/sigma)(Zs_ij - Xs_kj) Kn[i,k]."""
    X, y, c, V, rng = _data()
    n, p = X.shape
    sigma = float(p)
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    Xs = (X - m) / s
    Z = rng.standard_normal((23, p))
    Z[:, 2] = rng.choice([-1.0, 3.0], size=23)
    Zs = (Z - m) / s
    Kn = _kernel(Zs, Xs, sigma)
    j = 2
    z0, z1 = Xs[:, j].min(), Xs[:, j].max()
    sd = 1.0 / (z1 - z0)
    E = np.exp(-(z1 - z0) ** 2 / sigma)
    Einv = 1.0 / E
    h = Z[:, j] == 3.0
    b = (X[:, j] == 3.0).astype(np.float64)
    r = np.where(h, sd * (1.0 - Einv), -sd * (1.0 - E))
    t = np.where(h, sd * (Einv - E), -sd * (E - Einv))
    G = Kn * (r[:, None] + t[:, None] * b[None, :])
    Z1, Z0 = Zs.copy(), Zs.copy()
    Z1[:, j], Z0[:, j] = z1, z0
    ref = (_kernel(Z1, Xs, sigma) - _kernel(Z0, Xs, sigma)) * sd
    assert np.max(np.abs(G - ref)) <= 1e-13 * np.max(np.abs(ref))
    j = 0
    G = Kn * ((-2.0 / sigma) * Zs[:, j][:, None] + (2.0 / sigma) * Xs[:, j][None, :])
    ref = (-2.0 / sigma) * (Zs[:, j][:, None] - Xs[:, j][None, :]) * Kn
    assert np.max(np.abs(G - ref)) <= 1e-13 * np.max(np.abs(ref))


# --------------------------------------------------------------------------
# the C ABI and its ctypes table
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bigkrls_dev_gemm_modulated", "bigkrls_marginal_effects_se"])
def test_header_declares_and_ctypes_table_matches(name):
    from bigkrls_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name]) == _header_arity(name)


def test_se_entry_takes_both_forms_block_rows_and_the_output():
    # bigkrls_marginal_effects_factored's inputs without its three outputs, plus d_vcov_c, block_rows and h_se
    assert _header_arity("bigkrls_marginal_effects_se") == _header_arity("bigkrls_marginal_effects_factored") - 3 + 3 == 18
    assert _header_arity("bigkrls_dev_gemm_modulated") == 13


def test_public_api():
    import inspect
    import bigkrls_amd as bk
    assert inspect.signature(bk.marginal_effects).parameters["se"].default is False
    assert callable(bk.ops.bGemmModulated)


# --------------------------------------------------------------------------
# Python checks happen before any native call (no GPU here)
# --------------------------------------------------------------------------
def _object(vcov=True, factors=False):
    obj = _me_cpu._object()
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


def test_se_without_vcov_raises_before_any_native_call(no_native):
    import bigkrls_amd as bk
    obj = _object(vcov=False)
    with pytest.raises(ValueError, match="recompute bigKRLS object with bigKRLS\\(,vcov.est=TRUE\\)"):
        bk.marginal_effects(obj, obj["X"][:3], se=True)
    with pytest.raises(AssertionError, match="native call reached"):      # se=False goes on to the native call
        bk.marginal_effects(obj, obj["X"][:3])


class _FakeCtx:
    handle = None

    def from_numpy(self, a):
        a = np.asarray(a)
        return type("M", (), {"ptr": None, "ld": a.shape[0], "nrow": a.shape[0], "ncol": a.shape[1]})()


TODAYS_KEYS = {"derivatives", "avgderivatives", "var.avgderivatives", "which.derivatives", "binaryindicator", "xlabs",
               "newdata"}


@pytest.mark.parametrize("vcov,entries", [
    (None, ["bigkrls_marginal_effects", "bigkrls_marginal_effects_se"]),
    ("factors", ["bigkrls_marginal_effects_factored", "bigkrls_marginal_effects_se"]),
])
def test_keys_and_entries_with_and_without_se(monkeypatch, vcov, entries):
    from bigkrls_amd import _lib, api
    seen = []
    monkeypatch.setattr(api, "_call_native", lambda name, *args: seen.append((name, args)))
    obj = _object(factors=True)
    me = api.marginal_effects(obj, obj["X"][:3], ctx=_FakeCtx(), vcov=vcov)
    assert set(me) == TODAYS_KEYS
    assert [s[0] for s in seen] == entries[:1]
    del seen[:]
    me = api.marginal_effects(obj, obj["X"][:3], ctx=_FakeCtx(), vcov=vcov, se=True)
    assert set(me) == TODAYS_KEYS | {"se.derivatives"}
    assert me["se.derivatives"].shape == me["derivatives"].shape
    assert [s[0] for s in seen] == entries
    name, args = seen[1]
    assert len(args) == len(_lib.SIGNATURES[name])
    # the scalars that go with the factors (ldq, k) are zero when the matrix is the chosen form
    n = obj["X"].shape[0]
    assert (args[13], args[14]) == ((n, 5) if vcov == "factors" else (0, 0))
    assert args[16] == 0                                                  # block_rows: automatic
