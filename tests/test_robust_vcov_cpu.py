"""robust_vcov() without a GPU: the algebra of the rotated factors against the definition of the sandwich, every
validation error (raised before the library is touched), the C ABI of the three new entry points against the ctypes
table, and the two small members through save / load."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"bigkrls_dev_gram_weighted": 8, "bigkrls_dev_cluster_scores": 10, "bigkrls_vcov_robust": 16}
EPS = 2.0 ** -53


# --------------------------------------------------------------------------
# the algebra (csrc/robust.hip): V_r = G diag(omega) G = (Q U) diag(theta) (Q U)'
# --------------------------------------------------------------------------
def sandwich_factors_numpy(Q, d, lam, omega=None, scores=None, scale=1.0):
    """(Qout, wout) as bigkrls_vcov_robust forms them, in numpy: M = Q' diag(omega) Q (or S S' from the cluster
    scores), S = diag(g) M diag(g) symmetrised, its eigenpairs descending with negative values set to 0, Qout = Q U."""
    g = 1.0 / (d + lam)
    M = Q.T @ (omega[:, None] * Q) if scores is None else scores @ scores.T
    S = g[:, None] * (0.5 * (M + M.T)) * g[None, :]
    theta, U = np.linalg.eigh(S)
    order = np.argsort(-theta)
    return Q @ U[:, order], scale * np.maximum(theta[order], 0.0)


def _problem(n=60, k=12, seed=5):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, k)))
    d = np.sort(rng.random(k) * 5.0 + 0.01)[::-1]
    return rng, Q, d, 0.3


def test_rotated_factors_equal_the_definition():
    rng, Q, d, lam = _problem()
    n, k = Q.shape
    omega = rng.random(n) * 2.0
    Gm = (Q / (d + lam)) @ Q.T
    V_def = Gm @ np.diag(omega) @ Gm
    Qo, w = sandwich_factors_numpy(Q, d, lam, omega=omega, scale=1.7)
    V = (Qo * w) @ Qo.T
    assert np.all(w >= 0) and np.all(np.diff(w) <= 0)
    assert np.max(np.abs(V - 1.7 * V_def)) <= 64 * (n + k) * EPS * np.linalg.norm(1.7 * V_def, 2)
    assert np.max(np.abs(Qo.T @ Qo - np.eye(k))) < 1e-13                 # a rotation of an orthonormal basis


def test_constant_weights_give_the_fits_own_variance():
    _, Q, d, lam = _problem(seed=6)
    sigmasq = 0.37
    Qo, w = sandwich_factors_numpy(Q, d, lam, omega=np.ones(Q.shape[0]), scale=sigmasq)
    V_fit = (Q * (sigmasq / (d + lam) ** 2)) @ Q.T
    assert np.max(np.abs((Qo * w) @ Qo.T - V_fit)) <= 64 * sum(Q.shape) * EPS * np.linalg.norm(V_fit, 2)
    assert np.allclose(np.sort(w), np.sort(sigmasq / (d + lam) ** 2), rtol=1e-12)


def test_clustered_middle_is_the_outer_product_of_the_score_sums():
    rng, Q, d, lam = _problem(seed=7)
    n, k = Q.shape
    e = rng.standard_normal(n)
    labels = rng.integers(0, 3, size=n)
    S = np.zeros((k, 3))
    np.add.at(S.T, labels, e[:, None] * Q)
    Omega = np.outer(e, e) * (labels[:, None] == labels[None, :])
    Gm = (Q / (d + lam)) @ Q.T
    V_def = Gm @ Omega @ Gm
    Qo, w = sandwich_factors_numpy(Q, d, lam, scores=S)
    assert np.max(np.abs((Qo * w) @ Qo.T - V_def)) <= 64 * (n + k) * EPS * np.linalg.norm(V_def, 2)
    assert np.sum(w > 1e-12 * w[0]) <= 3                                 # rank G < k
    own = np.zeros((k, n))                                               # every row its own cluster: HC0
    np.add.at(own.T, np.arange(n), e[:, None] * Q)
    Q1, w1 = sandwich_factors_numpy(Q, d, lam, scores=own)
    Q0, w0 = sandwich_factors_numpy(Q, d, lam, omega=e ** 2)
    V0 = (Q0 * w0) @ Q0.T
    assert np.max(np.abs((Q1 * w1) @ Q1.T - V0)) <= 64 * (n + k) * EPS * np.linalg.norm(V0, 2)


# --------------------------------------------------------------------------
# the C ABI and its ctypes table
# --------------------------------------------------------------------------
def _header_arity(name):
    src = open(os.path.join(ROOT, "include", "bigkrls.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} not declared in include/bigkrls.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(NEW_ENTRIES))
def test_header_declares_and_ctypes_table_matches(name):
    from bigkrls_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name]) == _header_arity(name) == NEW_ENTRIES[name]


def test_public_api():
    import inspect
    import bigkrls_amd as bk
    sig = inspect.signature(bk.robust_vcov)
    assert list(sig.parameters) == ["object", "type", "cluster", "ctx"]
    assert sig.parameters["type"].default == "HC1" and sig.parameters["cluster"].default is None
    assert "robust_vcov" in bk.__all__
    assert callable(bk.ops.bGramWeighted) and callable(bk.ops.bClusterScores)


# --------------------------------------------------------------------------
# validation happens in Python, before any native call (no GPU here)
# --------------------------------------------------------------------------
def _object(n=40, p=3, k=5, factors=True):
    from bigkrls_amd.api import BigKRLS
    rng = np.random.default_rng(7)
    obj = BigKRLS({"X": rng.standard_normal((n, p)), "y": rng.standard_normal(n), "coeffs": rng.standard_normal(n),
                   "sigma": float(p), "lambda": 0.2, "K.eigenvalues": np.linspace(3.0, 0.1, n),
                   "yfitted.std": rng.standard_normal(n), "sigmasq": 0.4, "Neffective": n - 3.5,
                   "vcov.est.c": np.eye(n), "vcov.est.fitted": np.eye(n), "has.big.matrices": False})
    if factors:
        obj["vcov.est.Q"], obj["vcov.est.w"] = np.linalg.qr(rng.standard_normal((n, k)))[0], np.ones(k)
    return obj


@pytest.fixture
def no_native(monkeypatch):
    from bigkrls_amd import api

    def boom(*a, **k):
        raise AssertionError("native call reached")
    monkeypatch.setattr(api, "_call_native", boom)
    monkeypatch.setattr(api, "default_context", boom)


def test_not_a_bigkrls_object_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(TypeError, match="not of class"):
        bk.robust_vcov({"X": np.zeros((3, 1))})


def test_object_without_factors_raises_naming_the_form(no_native):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match=r'vcov_form="factors" or "both"'):
        bk.robust_vcov(_object(factors=False))


@pytest.mark.parametrize("bad", ["hc1", "HC4", "robust", None, 1])
def test_bad_type_raises(no_native, bad):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match="type must be one of"):
        bk.robust_vcov(_object(), type=bad)


@pytest.mark.parametrize("type", ["classical", "HC0", "HC1", "HC2", "HC3"])
def test_cluster_with_an_hc_type_raises(no_native, type):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match="cluster goes with"):
        bk.robust_vcov(_object(), type=type, cluster=np.arange(40) % 4)


@pytest.mark.parametrize("type", ["CR0", "CR1"])
def test_cr_type_without_cluster_raises(no_native, type):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match="needs cluster"):
        bk.robust_vcov(_object(), type=type)


def test_bad_cluster_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match="one label per row"):
        bk.robust_vcov(_object(), type="CR1", cluster=np.arange(39))
    with pytest.raises(ValueError, match="at least 2 distinct"):
        bk.robust_vcov(_object(), type="CR0", cluster=["a"] * 40)


def test_factor_shapes_that_disagree_raise(no_native):
    import bigkrls_amd as bk
    obj = _object()
    obj["vcov.est.w"] = np.ones(4)                                        # Q is 40 x 5
    with pytest.raises(ValueError, match="vcov.est.Q must be"):
        bk.robust_vcov(obj)


def test_plan_scale_factors_labels_and_residuals(no_native):
    from bigkrls_amd import api
    obj = _object()
    n = 40
    assert api._robust_plan(obj, "HC0", None)["scale"] == 1.0
    assert api._robust_plan(obj, "HC1", None)["scale"] == n / obj["Neffective"]
    assert api._robust_plan(obj, "classical", None)["scale"] == obj["sigmasq"]
    assert [api._robust_plan(obj, t, None)["code"] for t in ("classical", "HC0", "HC1", "HC2", "HC3")] == [0, 1, 2, 3, 4]
    lab = ["b", "a", ("t", 1), "b"] * 10                                  # any hashable labels, in order of appearance
    plan = api._robust_plan(obj, "CR1", lab)
    assert plan["G"] == 3 and plan["scale"] == 3 / 2 and plan["code"] == 2
    assert plan["labels"].dtype == np.int64 and list(plan["labels"][:4]) == [0, 1, 2, 0]
    assert api._robust_plan(obj, "CR0", lab)["scale"] == 1.0 and api._robust_plan(obj, "CR0", lab)["code"] == 1
    y = np.asarray(obj["y"])
    e = (y - y.mean()) / np.std(y, ddof=1) - obj["yfitted.std"]
    assert np.array_equal(plan["resid"], e) and plan["k"] == 5 and np.array_equal(plan["d"], obj["K.eigenvalues"][:5])


def test_valid_call_reaches_the_one_entry_and_leaves_the_input_alone(monkeypatch):
    """The numeric body is ONE native call with the plan's arguments; the result is a new object."""
    from bigkrls_amd import api
    obj = _object()
    obj.pop("vcov.est.c"), obj.pop("vcov.est.fitted")
    before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in obj.items()}
    calls = []

    class FakeMatrix:
        def __init__(self, nrow, ncol):
            self.nrow, self.ncol, self.ld, self.ptr = nrow, ncol, nrow, None

    class FakeCtx:
        handle = None

        def from_numpy(self, a):
            return FakeMatrix(*a.shape)

        def empty(self, nrow, ncol=1):
            return FakeMatrix(nrow, ncol)
    monkeypatch.setattr(api, "_call_native", lambda name, *a: calls.append((name, a)))
    out = api.robust_vcov(obj, type="CR1", cluster=np.arange(40) % 4, ctx=FakeCtx())
    assert [c[0] for c in calls] == ["bigkrls_vcov_robust"]
    a = calls[0][1]
    assert a[1:3] == (40, 5) and a[10] == 2 and a[12] == 4 and a[9] == 4 / 3
    assert out is not obj and out["vcov.type"] == "CR1" and out["vcov.clusters"] == 4
    assert out["vcov.est.c"] is None and out["vcov.est.fitted"] is None
    assert set(obj) == set(before) and "vcov.type" not in obj
    for k, v in before.items():
        assert np.array_equal(obj[k], v) if isinstance(v, np.ndarray) else obj[k] == v


# --------------------------------------------------------------------------
# summary() and persistence
# --------------------------------------------------------------------------
def _with_derivatives(obj):
    n, p = np.asarray(obj["X"]).shape
    rng = np.random.default_rng(9)
    obj.update({"derivatives": rng.standard_normal((n, p)), "avgderivatives": rng.standard_normal((1, p)),
                "var.avgderivatives": rng.random((1, p)) + 0.1, "R2": 0.5, "R2AME": 0.4, "xlabs": ["a", "b", "c"],
                "binaryindicator": np.zeros(p, dtype=bool), "which.derivatives": None})
    return obj


def test_summary_prints_the_vcov_line_only_for_robust_objects(capsys):
    import bigkrls_amd as bk
    plain = _with_derivatives(_object())
    bk.summary(plain)
    text_plain = capsys.readouterr().out
    assert "vcov:" not in text_plain
    classical = _with_derivatives(_object())
    classical["vcov.type"] = "classical"
    bk.summary(classical)
    assert capsys.readouterr().out == text_plain                          # unchanged for a classical object
    robust = _with_derivatives(_object())
    robust["vcov.type"] = "HC3"
    res = bk.summary(robust)
    assert "vcov: HC3\n" in capsys.readouterr().out
    assert np.array_equal(res["ttests"][:, 1], np.sqrt(robust["var.avgderivatives"].ravel()))


def test_save_load_carries_the_two_small_members(tmp_path):
    import bigkrls_amd as bk
    robust = _with_derivatives(_object())
    robust["vcov.type"], robust["vcov.clusters"] = "CR1", 7
    back = bk.load_bigKRLS(bk.save_bigKRLS(robust, str(tmp_path / "r"), noisy=False), noisy=False, to_device=False)
    assert back["vcov.type"] == "CR1" and back["vcov.clusters"] == 7
    robust["vcov.type"], robust["vcov.clusters"] = "HC1", None
    back = bk.load_bigKRLS(bk.save_bigKRLS(robust, str(tmp_path / "h"), noisy=False), noisy=False, to_device=False)
    assert back["vcov.type"] == "HC1" and back.get("vcov.clusters") is None
    plain = _with_derivatives(_object())
    back = bk.load_bigKRLS(bk.save_bigKRLS(plain, str(tmp_path / "p"), noisy=False), noisy=False, to_device=False)
    assert "vcov.type" not in back and "vcov.clusters" not in back        # a classical fit keeps its member list
