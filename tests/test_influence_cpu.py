"""influence() without a GPU: the closed-form deletion algebra (csrc/influence.hip) restated in numpy and checked against
true deletion refits, the C ABI of the two new entry points against the ctypes table, every validation error (raised
before the library is touched) and the CR3 member of robust_vcov()'s plan."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"bigkrls_dev_deletion_residuals": 14, "bigkrls_influence": 27}


# --------------------------------------------------------------------------
# the algebra
# --------------------------------------------------------------------------
def influence_numpy(Q, d, lam, ys, labels, S):
    """What bigkrls_influence computes, in standardised units and before the AMEs' scalar factors: for the units
    0 .. G - 1 of `labels` the deletion residuals et (n), the leverages, Cook's distances (G), the coefficient changes
    c - c(-u) (n x G), dfame = S' (c - c(-u)) (G x |J|) for the column-side vectors S (n x |J|), its jackknife variance and
    the leave-one-out R2."""
    n, k = Q.shape
    g = 1.0 / (d + lam)
    w = d * g
    H = (Q * w) @ Q.T
    e = ys - H @ ys
    G = int(labels.max()) + 1
    et = np.zeros(n)
    dc = np.zeros((n, G))
    num = np.zeros(G)
    for u in range(G):
        idx = np.flatnonzero(labels == u)
        if idx.size == 0:
            continue
        et[idx] = np.linalg.solve(np.eye(idx.size) - H[np.ix_(idx, idx)], e[idx])
        s = Q[idx].T @ et[idx]
        dc[:, u] = Q @ (g * s)
        num[u] = np.sum((w * s) ** 2)
    tr = w.sum()
    cooks = num / (tr * (e @ e) / (n - tr))
    dfame = (S.T @ dc).T
    return {"et": et, "hat": np.einsum("ij,j,ij->i", Q, w, Q), "cooks": cooks, "dc": dc, "dfame": dfame,
            "var_jack": (G - 1.0) / G * np.sum(dfame ** 2, axis=0), "r2_loo": 1.0 - (et @ et) / (ys @ ys), "num": num}


def _kernel_problem(n, p, seed, lam=0.2):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    Xs = (X - X.mean(0)) / X.std(0, ddof=1)
    y = np.sin(Xs @ np.linspace(0.5, 1.0, p)) + 0.3 * rng.standard_normal(n)
    ys = (y - y.mean()) / y.std(ddof=1)
    D2 = ((Xs[:, None, :] - Xs[None, :, :]) ** 2).sum(-1)
    K = np.exp(-D2 / p)
    return rng, K, ys, lam


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("G", [2, 5, 60])
def test_full_basis_equals_the_deleted_refit(G):
    """n = 60, P = 2, every eigenpair kept: deleting S is the refit (K_RR + lambda I)^-1 ys_R on the remaining rows."""
    n = 60
    rng, K, ys, lam = _kernel_problem(n, 2, 3)
    d, Q = np.linalg.eigh(K)
    d, Q = np.maximum(d[::-1], 0.0), Q[:, ::-1]
    labels = rng.permutation((np.arange(n) * G) // n)
    S = rng.standard_normal((n, 3))
    c = Q @ ((Q.T @ ys) / (d + lam))
    got = influence_numpy(Q, d, lam, ys, labels, S)
    for u in range(G):
        s_idx, r_idx = np.flatnonzero(labels == u), np.flatnonzero(labels != u)
        c_del = np.zeros(n)
        c_del[r_idx] = np.linalg.solve(K[np.ix_(r_idx, r_idx)] + lam * np.eye(r_idx.size), ys[r_idx])
        assert rel(got["et"][s_idx], ys[s_idx] - K[s_idx] @ c_del) < 1e-9
        assert rel(got["dc"][:, u], c - c_del) < 1e-8
        assert abs(got["num"][u] - np.sum((K @ (c - c_del)) ** 2)) < 1e-8 * got["num"][u]
        assert rel(got["dfame"][u], S.T @ (c - c_del)) < 1e-8
    if G == n:
        e = ys - K @ c
        assert rel(got["et"], e / (1.0 - got["hat"])) < 1e-12


@pytest.mark.parametrize("G", [3, 7, 120])
def test_truncated_basis_equals_the_fixed_basis_normal_equations(G):
    """n = 120, k = 12: the fit is the penalised least-squares estimator on the fixed basis Q, and deleting S is
    (Q_R' Q_R + lambda D^-1)^-1 Q_R' ys_R."""
    n, k = 120, 12
    rng, K, ys, lam = _kernel_problem(n, 3, 4)
    d, Q = np.linalg.eigh(K)
    d, Q = d[::-1][:k], Q[:, ::-1][:, :k]
    labels = rng.permutation((np.arange(n) * G) // n)
    S = rng.standard_normal((n, 2))
    beta = np.linalg.solve(Q.T @ Q + lam * np.diag(1.0 / d), Q.T @ ys)
    got = influence_numpy(Q, d, lam, ys, labels, S)
    assert rel(Q @ beta, (Q * (d / (d + lam))) @ (Q.T @ ys)) < 1e-12          # the smoother is H
    for u in range(G):
        s_idx, r_idx = np.flatnonzero(labels == u), np.flatnonzero(labels != u)
        QR = Q[r_idx]
        beta_del = np.linalg.solve(QR.T @ QR + lam * np.diag(1.0 / d), QR.T @ ys[r_idx])
        assert rel(got["et"][s_idx], ys[s_idx] - Q[s_idx] @ beta_del) < 1e-11
        assert rel(got["dc"][:, u], Q @ ((beta - beta_del) / d)) < 1e-10
        assert abs(got["num"][u] - np.sum((Q @ (beta - beta_del)) ** 2)) < 1e-10 * got["num"][u]
    assert np.allclose(got["var_jack"], (G - 1.0) / G * np.sum(got["dfame"] ** 2, axis=0))
    assert got["r2_loo"] < 1.0 - ((ys - (Q * (d / (d + lam))) @ (Q.T @ ys)) ** 2).sum() / (ys @ ys)   # worse than in sample


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
    sig = inspect.signature(bk.influence)
    assert list(sig.parameters) == ["object", "cluster", "which_derivatives", "newdata", "ctx"]
    assert all(sig.parameters[k].default is None for k in ("cluster", "which_derivatives", "newdata", "ctx"))
    assert "influence" in bk.__all__ and callable(bk.ops.bDeletionResiduals)
    assert "deletion_residuals" in open(os.path.join(ROOT, "include", "bigkrls.h")).read().split("bigkrls_ctx_set_profile")[0]


# --------------------------------------------------------------------------
# validation happens in Python, before any native call (no GPU here)
# --------------------------------------------------------------------------
def _object(n=40, p=3, k=5, factors=True):
    from bigkrls_amd.api import BigKRLS
    rng = np.random.default_rng(7)
    X = rng.standard_normal((n, p))
    X[:, 2] = (rng.random(n) < 0.5).astype(float)
    obj = BigKRLS({"X": X, "y": rng.standard_normal(n), "coeffs": rng.standard_normal(n),
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
        bk.influence({"X": np.zeros((3, 1))})


def test_object_without_factors_raises_naming_the_form(no_native):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match=r'vcov_form="factors" or "both"'):
        bk.influence(_object(factors=False))


def test_bad_cluster_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match="one label per row"):
        bk.influence(_object(), cluster=np.arange(39))
    with pytest.raises(ValueError, match="at least 2 distinct"):
        bk.influence(_object(), cluster=["a"] * 40)


def test_factor_shapes_and_missing_members_raise(no_native):
    import bigkrls_amd as bk
    obj = _object()
    obj["vcov.est.w"] = np.ones(4)                                        # Q is 40 x 5
    with pytest.raises(ValueError, match="vcov.est.Q must be"):
        bk.influence(obj)
    obj = _object()
    obj["K.eigenvalues"] = np.ones(3)
    with pytest.raises(ValueError, match="K.eigenvalues do not cover"):
        bk.influence(obj)
    obj = _object()
    obj["lambda"] = None
    with pytest.raises(ValueError, match="has no lambda"):
        bk.influence(obj)


def test_which_and_newdata_are_validated(no_native):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match="which.derivatives must index"):
        bk.influence(_object(), which_derivatives=[0])
    with pytest.raises(ValueError, match="ncol\\(newdata\\) differs"):
        bk.influence(_object(), newdata=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="missing or infinite"):
        bk.influence(_object(), newdata=np.full((4, 3), np.nan))
    with pytest.raises(ValueError, match="is binary in the training data"):
        bk.influence(_object(), newdata=np.full((4, 3), 0.5))


def test_multi_gpu_and_stripped_robust_objects_are_refused(no_native):
    import bigkrls_amd as bk
    obj = _object()
    obj["rows"] = (0, 20)
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        bk.influence(obj)
    obj = _object()
    obj["vcov.type"] = "HC1"                                              # rotated factors without the fit's own
    with pytest.raises(ValueError, match="vcov.fit.Q"):
        bk.influence(obj)


def test_valid_call_reaches_the_one_entry(monkeypatch):
    """The numeric body is ONE native call; a robust object hands over the fit's ORIGINAL eigenvectors."""
    from bigkrls_amd import api
    calls = []

    class FakeMatrix:
        def __init__(self, a, tag):
            self.nrow, self.ncol = a.shape
            self.shape, self.ld, self.ptr, self.tag = a.shape, a.shape[0], tag, tag

    class FakeCtx:
        handle = None

        def from_numpy(self, a):
            return FakeMatrix(a, int(a[0, 0] * 1e6))

    monkeypatch.setattr(api, "_call_native", lambda name, *a: calls.append((name, a)))
    obj = _object()
    lab = ["b", "a", ("t", 1), "b"] * 10
    out = api.influence(obj, cluster=lab, which_derivatives=[3, 1], ctx=FakeCtx())
    assert [c[0] for c in calls] == ["bigkrls_influence"]
    a = calls[0][1]
    assert a[2:4] == (40, 3) and a[8] == 2 and a[9] is None and a[10] == 40 and a[13] == 5 and a[15] == 0.2 and a[18] == 3
    assert out["units"] == 3 and out["unit.labels"] == ["b", "a", ("t", 1)] and list(out["unit.sizes"]) == [20, 10, 10]
    assert out["which.derivatives"] == [3, 1] and out["dfame"].shape == (3, 2) and out["cooks"].shape == (3,)
    assert out["ame"].shape == (1, 2) and out["var.avgderivatives.jack"].shape == (1, 2) and out["hat"].shape == (40,)
    single = api.influence(obj, ctx=FakeCtx())
    assert single["units"] == 40 and single["unit.labels"] is None and calls[1][1][17] is None and calls[1][1][18] == 0
    assert single["dfame"].shape == (40, 3)
    rob = _object()
    rob["vcov.type"] = "CR1"
    rob["vcov.fit.Q"] = rob["vcov.est.Q"] + 0.0
    rob["vcov.est.Q"] = rob["vcov.est.Q"] @ np.linalg.qr(np.random.default_rng(1).standard_normal((5, 5)))[0]
    api.influence(rob, ctx=FakeCtx())
    assert calls[2][1][11] == int(rob["vcov.fit.Q"][0, 0] * 1e6) != int(rob["vcov.est.Q"][0, 0] * 1e6)


def test_robust_vcov_keeps_the_fits_eigenvectors(monkeypatch):
    from bigkrls_amd import api

    class FakeMatrix:
        def __init__(self, nrow, ncol):
            self.nrow, self.ncol, self.ld, self.ptr = nrow, ncol, nrow, None

    class FakeCtx:
        handle = None

        def from_numpy(self, a):
            return FakeMatrix(*a.shape)

        def empty(self, nrow, ncol=1):
            return FakeMatrix(nrow, ncol)
    monkeypatch.setattr(api, "_call_native", lambda name, *a: None)
    obj = _object()
    obj.pop("vcov.est.c"), obj.pop("vcov.est.fitted")
    out = api.robust_vcov(obj, type="HC0", ctx=FakeCtx())
    assert out["vcov.fit.Q"] is not out["vcov.est.Q"] and (out["vcov.fit.Q"].nrow, out["vcov.fit.Q"].ncol) == (40, 5)
    assert "vcov.fit.Q" not in obj


@pytest.mark.parametrize("binary", [False, True])
def test_save_load_carries_the_fits_eigenvectors(tmp_path, binary):
    """vcov.fit.Q of a robust object is written as a big-matrix file beside vcov.est.Q and read back: the saved object
    still serves influence(). (A device matrix whose contents live on the host stands in for the GPU's.)"""
    import bigkrls_amd as bk
    from bigkrls_amd.device import DeviceMatrix

    class HostBacked(DeviceMatrix):
        def __init__(self, a):
            self.a = np.asfortranarray(a)

        def to_numpy(self):
            return self.a

    rng = np.random.default_rng(11)
    rob = _object()
    rob.update({"derivatives": rng.standard_normal((40, 3)), "avgderivatives": rng.standard_normal((1, 3)),
                "var.avgderivatives": rng.random((1, 3)) + 0.1, "R2": 0.5, "R2AME": 0.4, "xlabs": ["a", "b", "c"],
                "binaryindicator": np.array([False, False, True]), "which.derivatives": None})
    Qfit, Qrot = rob["vcov.est.Q"], rob["vcov.est.Q"] @ np.linalg.qr(rng.standard_normal((5, 5)))[0]
    rob["vcov.type"], rob["vcov.clusters"] = "CR3", 4
    rob["vcov.est.Q"], rob["vcov.fit.Q"] = HostBacked(Qrot), HostBacked(Qfit)
    folder = bk.save_bigKRLS(rob, str(tmp_path / "m"), noisy=False, binary=binary)
    ext = ".npy" if binary else ".txt"
    assert os.path.exists(os.path.join(folder, "vcov.fit.Q" + ext)) and os.path.exists(os.path.join(folder, "vcov.est.Q" + ext))
    back = bk.load_bigKRLS(folder, noisy=False, to_device=False)
    assert np.array_equal(back["vcov.fit.Q"], Qfit) and np.array_equal(back["vcov.est.Q"], Qrot)
    assert back["vcov.type"] == "CR3" and back["vcov.clusters"] == 4
    from bigkrls_amd import api
    plan = api._influence_plan(back, None, None, None)                     # the loaded object is accepted, on the fit's own Q
    assert plan["Q"] is back["vcov.fit.Q"] and plan["k"] == 5
    # an object without it (a fit, or a robust object saved before) loads without the member and without a NOTE
    plain = _object()
    plain["vcov.est.Q"] = HostBacked(plain["vcov.est.Q"])
    plain.update({k: rob[k] for k in ("derivatives", "avgderivatives", "var.avgderivatives", "R2", "R2AME", "xlabs",
                                      "binaryindicator", "which.derivatives")})
    back = bk.load_bigKRLS(bk.save_bigKRLS(plain, str(tmp_path / "p"), noisy=False, binary=binary), noisy=False, to_device=False)
    assert "vcov.fit.Q" not in back


# --------------------------------------------------------------------------
# CR3 in robust_vcov()'s plan
# --------------------------------------------------------------------------
def test_cr3_is_accepted_with_code_5_and_the_jackknife_scale(no_native):
    from bigkrls_amd import api
    obj = _object()
    lab = ["b", "a", ("t", 1), "b"] * 10
    plan = api._robust_plan(obj, "CR3", lab)
    assert api.ROBUST_TYPES["CR3"] == 5 and plan["code"] == 5 and plan["G"] == 3 and plan["scale"] == 2 / 3
    assert list(plan["labels"][:4]) == [0, 1, 2, 0]
    with pytest.raises(ValueError, match="needs cluster"):
        api._robust_plan(obj, "CR3", None)
    with pytest.raises(ValueError, match="cluster goes with"):
        api._robust_plan(obj, "HC3", lab)
    with pytest.raises(ValueError, match="type must be one of .*CR3"):
        api._robust_plan(obj, "CR2", lab)
