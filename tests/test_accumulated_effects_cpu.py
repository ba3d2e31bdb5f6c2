"""CPU checks of accumulated_effects(): a numpy restatement of the linear form ale_j = sd(y) A_j c, cov_j = f A_j Vc A_j'
(also used by tests/test_gpu_accumulated_effects.py) against the definition -- loop over the bins, evaluate the
prediction function on the bin's rows rewritten to the upper and to the lower edge, average, accumulate, centre --, the
inverted-CDF edges, the C ABI's two new entry points and their ctypes arity, the export, and the Python validation, which
raises before any native call."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------
# numpy restatement of the algebra (include/bigkrls.h, bigkrls_accumulated_effects)
# --------------------------------------------------------------------------
def ale_bins(z, edges):
    """b(i) - 1 with b(i) = the smallest b >= 1 with z_i <= z_b (a row equal to z_0 goes to bin 1), and the counts."""
    lab = np.maximum(np.searchsorted(edges, z, side="left"), 1) - 1
    return lab, np.bincount(lab, minlength=len(edges) - 1)


def loo_binsums_numpy(A, B, sigma, cols, labels, nbins, dtype=np.float64):
    """out[l, off(jj) + b] = sum over i with labels[i, jj] = b of exp(-(||A_i - B_l||^2 - (A[i,c] - B[l,c])^2) / sigma),
    c = cols[jj]: the direct sum over the other columns, in `dtype`."""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    labels = np.asarray(labels).reshape(A.shape[0], len(cols))
    out = np.zeros((B.shape[0], int(np.sum(nbins))), dtype=dtype)
    at = 0
    for jj, c in enumerate(cols):
        d2 = np.zeros((A.shape[0], B.shape[0]), dtype=dtype)
        for k in range(A.shape[1]):
            if k != c:
                d2 += (A[:, k][:, None] - B[:, k][None, :]) ** 2
        E = np.exp(-d2 / dtype(sigma))
        for b in range(int(nbins[jj])):
            out[:, at + b] = E[labels[:, jj] == b].sum(axis=0)
        at += int(nbins[jj])
    return out


def ale_numpy(X, y, coeffs, sigma, which, edges, newdata=None, vcov_c=None, neffective=None):
    """accumulated_effects() in numpy: (ale, se, cov), lists over the columns of `which` (1-based), in the original
    units of y; se and cov are None without vcov_c. neffective: predict()'s factor sqrt(n / neffective) on the variance."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    Z = X if newdata is None else np.asarray(newdata, dtype=np.float64)
    u = Z.shape[0]
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    ysd = float(np.std(y, ddof=1))
    Xs, Zs = (X - m) / s, (Z - m) / s
    c = np.asarray(coeffs, dtype=np.float64).ravel()
    f = 1.0 if not neffective else np.sqrt(n / float(neffective))
    ales, ses, covs = [], [], []
    for jj, w in enumerate(which):
        j = w - 1
        e = np.asarray(edges[jj], dtype=np.float64)
        B = e.size - 1
        lab, cnt = ale_bins(Z[:, j], e)
        M = loo_binsums_numpy(Zs, Xs, sigma, [j], lab[:, None], [B])                       # n x B
        vs = (e - m[j]) / s[j]
        phi = np.exp(-(vs[:, None] - Xs[:, j][None, :]) ** 2 / sigma)                       # (B + 1) x n
        D = M.T * (phi[1:] - phi[:-1]) / cnt[:, None]                                       # B x n
        Cum = np.tril(np.ones((B + 1, B)), -1)
        wgt = np.zeros(B + 1)
        wgt[:-1] += cnt / (2.0 * u)
        wgt[1:] += cnt / (2.0 * u)
        A = (np.eye(B + 1) - np.outer(np.ones(B + 1), wgt)) @ Cum @ D                       # (B + 1) x n
        ales.append(ysd * (A @ c))
        if vcov_c is not None:
            cov = f * (A @ np.asarray(vcov_c, dtype=np.float64) @ A.T)
            covs.append(cov)
            ses.append(np.sqrt(np.maximum(np.diag(cov), 0.0)))
    return ales, (ses if vcov_c is not None else None), (covs if vcov_c is not None else None)


def _kernel(A, B, sigma):
    d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2)
    return np.exp(-d2 / sigma)


def test_restatement_equals_the_definition():
    rng = np.random.default_rng(23)
    n, p, u = 40, 3, 37
    X = rng.standard_normal((n, p)) * np.array([1.0, 1.0, 3.0]) + np.array([0.0, 0.0, 5.0])
    X[:, 1] = (rng.random(n) < 0.4).astype(np.float64) * 2.0 + 1.0       # binary, values 1 and 3
    y = rng.standard_normal(n) * 2.0 + 0.7
    c = rng.standard_normal(n)
    Gm = rng.standard_normal((n, n))
    Vc = Gm @ Gm.T / n
    sigma = float(p)
    Z = rng.standard_normal((u, p)) * np.array([1.0, 1.0, 3.0]) + np.array([0.3, 0.0, 5.0])
    Z[:, 1] = (rng.random(u) < 0.5).astype(np.float64) * 2.0 + 1.0
    Z[:, 0] = np.round(Z[:, 0] * 4.0) / 4.0                                # ties, and ties on an edge
    e0 = np.quantile(Z[:, 0], [0.0, 0.3, 0.55, 0.8, 1.0], method="inverted_cdf")
    e0 = np.unique(e0)
    assert np.sum(Z[:, 0] == e0[0]) >= 1 and np.sum(Z[:, 0] == e0[1]) >= 2     # a row equal to z_0; ties on an edge
    e2 = np.array([Z[:, 2].min(), 4.0, 5.5, Z[:, 2].max() + 1.0])
    which = [3, 2, 1]
    edges = [e2, np.array([1.0, 3.0]), e0]
    m, s = X.mean(axis=0), X.std(axis=0, ddof=1)
    ysd = y.std(ddof=1)
    Xs = (X - m) / s
    pred = lambda R: ysd * (_kernel((R - m) / s, Xs, sigma) @ c)       # the prediction without mean(y): it cancels
    for newdata in (None, Z):
        R = X if newdata is None else Z
        if newdata is None:
            edges_r = [np.array([X[:, 2].min(), 5.0, X[:, 2].max()]), np.array([1.0, 3.0]),
                       np.array([X[:, 0].min(), 0.0, X[:, 0].max()])]
        else:
            edges_r = edges
        uu = R.shape[0]
        ales, ses, covs = ale_numpy(X, y, c, sigma, which, edges_r, newdata=newdata, vcov_c=Vc)
        for jj, w in enumerate(which):
            j = w - 1
            e = edges_r[jj]
            B = e.size - 1
            # the definition, row by row: every row belongs to the first bin whose upper edge is not below it
            local, cnt = np.zeros(B), np.zeros(B)
            rows = []
            for b in range(1, B + 1):
                inb = np.array([(z <= e[b]) and (b == 1 or z > e[b - 1]) for z in R[:, j]])
                assert inb.any()
                hi, lo = R[inb].copy(), R[inb].copy()
                hi[:, j], lo[:, j] = e[b], e[b - 1]
                local[b - 1] = (pred(hi) - pred(lo)).mean()
                cnt[b - 1] = inb.sum()
                rows += [hi, lo]
            assert cnt.sum() == uu
            g = np.concatenate([[0.0], np.cumsum(local)])
            ale_def = g - np.sum(cnt * (g[:-1] + g[1:]) / 2.0) / uu
            np.testing.assert_allclose(ales[jj], ale_def, rtol=0, atol=1e-12 * np.abs(ale_def).max())
            # the covariance by the definition: omega' K Vc K' omega on the stacked rewritten rows
            S = np.vstack(rows)
            K = _kernel((S - m) / s, Xs, sigma)
            Wl = np.zeros((B, S.shape[0]))        # local_b as a combination of the stacked rows
            at = 0
            for b in range(B):
                nb = int(cnt[b])
                Wl[b, at:at + nb] = 1.0 / nb
                Wl[b, at + nb:at + 2 * nb] = -1.0 / nb
                at += 2 * nb
            Cum = np.tril(np.ones((B + 1, B)), -1)
            wgt = np.zeros(B + 1)
            wgt[:-1] += cnt / (2.0 * uu)
            wgt[1:] += cnt / (2.0 * uu)
            Om = (np.eye(B + 1) - np.outer(np.ones(B + 1), wgt)) @ Cum @ Wl
            np.testing.assert_allclose(ysd * (Om @ K @ c), ale_def, rtol=0, atol=1e-12 * np.abs(ale_def).max())
            cov_def = Om @ K @ Vc @ K.T @ Om.T
            np.testing.assert_allclose(covs[jj], cov_def, rtol=0, atol=1e-11 * np.abs(cov_def).max())
            np.testing.assert_allclose(ses[jj], np.sqrt(np.diag(cov_def)), rtol=1e-9)
            # the centring
            assert abs(np.sum(cnt * (ales[jj][:-1] + ales[jj][1:]) / 2.0)) <= 1e-12 * uu * np.abs(ales[jj]).max()
        # the binary column: (-d/2, +d/2)
        np.testing.assert_allclose(ales[1][0], -ales[1][1], rtol=1e-12)
    _, _, covs_n = ale_numpy(X, y, c, sigma, which, edges, newdata=Z, vcov_c=Vc, neffective=10.0)
    _, _, covs_1 = ale_numpy(X, y, c, sigma, which, edges, newdata=Z, vcov_c=Vc)
    np.testing.assert_allclose(covs_n[0], covs_1[0] * np.sqrt(n / 10.0), rtol=1e-14)
    assert ale_numpy(X, y, c, sigma, which, edges, newdata=Z)[1] is None


def test_inverted_cdf_edges_leave_no_empty_bin():
    rng = np.random.default_rng(3)
    z = rng.standard_normal(37)
    e = np.unique(np.quantile(z, np.arange(6) / 5, method="inverted_cdf"))
    assert e.size == 6 and np.all(np.isin(e, z))
    lab, cnt = ale_bins(z, e)
    assert list(cnt) == [8, 7, 8, 7, 7]
    assert lab[np.argmin(z)] == 0                                        # the row equal to z_0 is in bin 1
    # ties merge bins and still no bin is empty
    zt = np.round(z)
    et = np.unique(np.quantile(zt, np.arange(21) / 20, method="inverted_cdf"))
    assert et.size - 1 < 20 and np.all(ale_bins(zt, et)[1] > 0)


def test_native_call_takes_the_22_arguments(no_native_capture):
    import bigkrls_amd as bk
    obj = _object()
    Z = np.random.default_rng(3).standard_normal((37, 3))
    Z[:, 1] = 1.0
    with pytest.raises(_Reached) as ei:
        bk.accumulated_effects(obj, which=[1, 2], bins=5, newdata=Z)
    a = ei.value.args_
    assert a[0] == "bigkrls_accumulated_effects" and len(a) - 1 == 22


# --------------------------------------------------------------------------
# the C ABI and its ctypes table
# --------------------------------------------------------------------------
def _header_arity(name):
    src = open(os.path.join(ROOT, "include", "bigkrls.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} not declared in include/bigkrls.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,arity", [("bigkrls_dev_kernel_loo_binsums", 15), ("bigkrls_accumulated_effects", 22)])
def test_header_declares_and_ctypes_table_matches(name, arity):
    from bigkrls_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name]) == _header_arity(name) == arity


def test_library_exports_the_symbols():
    from bigkrls_amd import _lib
    lib = _lib.load()
    for name in ("bigkrls_dev_kernel_loo_binsums", "bigkrls_accumulated_effects"):
        assert getattr(lib, name) is not None


def test_public_api_exports_accumulated_effects():
    import bigkrls_amd as bk
    from bigkrls_amd import ops
    assert callable(bk.accumulated_effects) and "accumulated_effects" in bk.__all__
    assert callable(ops.bKernelLooBinsums)


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


class _Reached(Exception):
    def __init__(self, args_):
        super().__init__("native call reached")
        self.args_ = args_


@pytest.fixture
def no_native(monkeypatch):
    from bigkrls_amd import api

    def boom(*a, **k):
        raise AssertionError("native call reached")
    monkeypatch.setattr(api, "_call_native", boom)
    monkeypatch.setattr(api, "default_context", boom)


@pytest.fixture
def no_native_capture(monkeypatch):
    from bigkrls_amd import api

    class _Ctx:
        handle = None

    def call(*a, **k):
        raise _Reached(a)
    monkeypatch.setattr(api, "_call_native", call)
    monkeypatch.setattr(api, "_effects_device",
                        lambda object, form, ctx, p: (_Ctx(), None, None, None, np.zeros(1), np.zeros(1),
                                                      (None, None, 0, 0, None), [f"x{i + 1}" for i in range(p)]))


def test_wrong_ncol_of_newdata_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match="ncol"):
        bk.accumulated_effects(_object(), newdata=np.zeros((5, 4)))


def test_bad_which_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    for bad in ([0], [4], [], [1, 5]):
        with pytest.raises(ValueError, match="which.derivatives"):
            bk.accumulated_effects(obj, which=bad)


def test_bad_bins_raise(no_native):
    import bigkrls_amd as bk
    obj = _object()
    x = obj["X"][:, 0]
    with pytest.raises(ValueError, match="bins must be at least 1"):
        bk.accumulated_effects(obj, bins=0)
    with pytest.raises(ValueError, match="one array of edges per column"):
        bk.accumulated_effects(obj, which=[1, 3], bins=[np.array([0.0, 1.0])])
    for bad in (True, 20.0, "20", None, [1.0, 2.0, 3.0]):           # neither an int nor a list of edge arrays
        with pytest.raises(ValueError, match="bins must be an integer or a list with one array of edges"):
            bk.accumulated_effects(obj, bins=bad)
    with pytest.raises(ValueError, match="edges of column 1 must hold at least 2"):
        bk.accumulated_effects(obj, which=[1], bins=[np.array([0.0])])
    with pytest.raises(ValueError, match="edges of column 1 contain missing or infinite"):
        bk.accumulated_effects(obj, which=[1], bins=[np.array([x.min(), np.nan, x.max()])])
    with pytest.raises(ValueError, match="edges of column 1 must be strictly increasing"):
        bk.accumulated_effects(obj, which=[1], bins=[np.array([x.min(), 0.0, 0.0, x.max()])])
    with pytest.raises(ValueError, match="edges of column 1 do not cover the reference rows"):
        bk.accumulated_effects(obj, which=[1], bins=[np.array([x.min(), 0.0, np.sort(x)[-2]])])
    with pytest.raises(ValueError, match="edges of column 1 do not cover the reference rows"):
        bk.accumulated_effects(obj, which=[1], bins=[np.array([np.sort(x)[1], 0.0, x.max()])])
    with pytest.raises(ValueError, match="bin 2 of column 1 holds no reference row"):
        bk.accumulated_effects(obj, which=[1], bins=[np.array([x.min(), 0.0, np.nextafter(0.0, 1.0), x.max()])])
    # good explicit edges pass up to the native call
    with pytest.raises(AssertionError, match="native call reached"):
        bk.accumulated_effects(obj, which=[1], bins=[np.array([x.min(), 0.0, x.max()])])


def test_edges_of_a_binary_column_must_be_its_training_values(no_native):
    import bigkrls_amd as bk
    obj = _object()
    x = obj["X"][:, 0]
    good = np.array([x.min(), x.max()])
    for bad in (np.array([1.0, 2.0, 3.0]), np.array([0.0, 3.0]), np.array([1.0, 4.0])):
        with pytest.raises(ValueError, match=r"column 2 is binary.*\(1, 3\)"):
            bk.accumulated_effects(obj, which=[1, 2], bins=[good, bad])
    with pytest.raises(AssertionError, match="native call reached"):
        bk.accumulated_effects(obj, which=[1, 2], bins=[good, np.array([1.0, 3.0])])


def test_constant_reference_column_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    Z = obj["X"][:7].copy()
    Z[:, 2] = 0.25
    with pytest.raises(ValueError, match="one distinct value in column 3"):
        bk.accumulated_effects(obj, newdata=Z)
    with pytest.raises(ValueError, match="one distinct value in column 3"):
        bk.accumulated_effects(obj, which=[3], bins=[np.array([0.0, 1.0])], newdata=Z)


def test_not_a_bigkrls_object_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(TypeError):
        bk.accumulated_effects({"X": np.zeros((3, 2))})


def test_se_without_any_vcov_form_raises(no_native):
    import bigkrls_amd as bk
    obj = _object(vcov=False)
    with pytest.raises(ValueError, match="vcov.est=TRUE"):
        bk.accumulated_effects(obj)
    with pytest.raises(AssertionError, match="native call reached"):     # without SEs the object is enough
        bk.accumulated_effects(obj, se=False)


def test_multi_gpu_object_with_sharded_matrix_only_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    obj["rows"] = (0, 20)
    obj["vcov.est.c.cols"] = None
    with pytest.raises(NotImplementedError, match="accumulated_effects of a multi-GPU"):
        bk.accumulated_effects(obj)
