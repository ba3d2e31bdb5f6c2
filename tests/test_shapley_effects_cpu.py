"""shapley_effects() without a GPU: a numpy restatement of the definition in include/bigkrls.h (shapley_weights_numpy,
shapley_numpy -- the GPU tests import both) checked against brute force over all 2^M coalitions, efficiency and the
baseline, the deterministic background rule, the groups, the C ABI's entries and their ctypes table, and every Python
validation error, raised before any native call."""
import itertools
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------
# the definition, restated
# --------------------------------------------------------------------------
def _players(labels, p):
    labels = np.arange(p) if labels is None else np.asarray(labels, dtype=np.int64)
    M = int(labels.max()) + 1
    return labels, M, [np.flatnonzero(labels == m) for m in range(M)]


def shapley_weights_numpy(Z, X, Bg, sigma, labels=None, nodes=None, dtype=np.float64):
    """W ((u M) x n, row r M + m) of bigkrls_dev_shapley_weights, computed as the definition reads: per (explained row,
    background row) the factors A_m, B_m of every training row, Gauss-Legendre on [0,1] with `nodes` nodes (default
    ceil(M/2); any larger count integrates the same polynomial), the product without player m as prefix times suffix."""
    Z, X, Bg = (np.asarray(a, dtype=dtype) for a in (Z, X, Bg))
    u, p = Z.shape
    n, B = X.shape[0], Bg.shape[0]
    labels, M, cols = _players(labels, p)
    G = (M + 1) // 2 if nodes is None else int(nodes)
    x, w = np.polynomial.legendre.leggauss(G)
    t, w = ((1 + x) / 2).astype(dtype), (w / 2).astype(dtype)
    sigma = dtype(sigma)

    def factors(row):                                   # (n x M): exp(-sum_{l in m} (row_l - X_il)^2 / sigma)
        d2 = (row[None, :] - X) ** 2
        return np.exp(-np.stack([d2[:, c].sum(axis=1) for c in cols], axis=1) / sigma)

    W = np.zeros((u * M, n), dtype=dtype)
    Bf = [factors(Bg[b]) for b in range(B)]
    one = np.ones((n, G, 1), dtype=dtype)
    for r in range(u):
        A = factors(Z[r])
        for b in range(B):
            D = A - Bf[b]
            F = Bf[b][:, None, :] + t[None, :, None] * D[:, None, :]                  # n x G x M
            pre = np.concatenate([one, np.cumprod(F, axis=2)[:, :, :-1]], axis=2)
            suf = np.concatenate([np.cumprod(F[:, :, ::-1], axis=2)[:, :, ::-1][:, :, 1:], one], axis=2)
            integral = np.einsum("g,igm->im", w, pre * suf)                          # n x M
            W[r * M:(r + 1) * M, :] += (D * integral).T
    return W / dtype(B)


def _standardise(X, y, *others):
    mx, sx = X.mean(axis=0), X.std(axis=0, ddof=1)
    return (X - mx) / sx, y.mean(), y.std(ddof=1), [(o - mx) / sx for o in others]


def shapley_numpy(X, y, coeffs, sigma, newdata, background, labels=None, vcov_c=None, neffective=None, nodes=None):
    """(shapley u x M, baseline, se u x M or None) as bigkrls_shapley_effects defines them; vcov_c is the object's
    vcov.est.c (which carries sd(y)^2: the variance is f W vcov.est.c W' = f sd(y)^2 W V W' with V = vcov.est.c / sd(y)^2)."""
    X, y, coeffs = np.asarray(X, float), np.asarray(y, float).ravel(), np.asarray(coeffs, float).ravel()
    Xs, ym, ys, (Zs, Bs) = _standardise(X, y, np.asarray(newdata, float), np.asarray(background, float))
    u = Zs.shape[0]
    W = shapley_weights_numpy(Zs, Xs, Bs, sigma, labels, nodes)
    M = W.shape[0] // u
    phi = (ys * (W @ coeffs)).reshape(u, M)
    Kb = np.exp(-((Bs[:, None, :] - Xs[None, :, :]) ** 2).sum(axis=2) / sigma)
    baseline = float(np.mean(ym + ys * (Kb @ coeffs)))
    se = None
    if vcov_c is not None:
        f = 1.0 if neffective is None else math.sqrt(X.shape[0] / neffective)
        V = np.asarray(vcov_c, float) / ys ** 2
        se = np.sqrt(np.maximum(f * ys ** 2 * np.einsum("ij,jk,ik->i", W, V, W), 0.0)).reshape(u, M)
    return phi, baseline, se


def predict_numpy(X, y, coeffs, sigma, rows):
    Xs, ym, ys, (Rs,) = _standardise(np.asarray(X, float), np.asarray(y, float).ravel(), np.asarray(rows, float))
    K = np.exp(-((Rs[:, None, :] - Xs[None, :, :]) ** 2).sum(axis=2) / sigma)
    return ym + ys * (K @ np.asarray(coeffs, float).ravel())


def hybrid_rows(newdata, background, labels=None):
    """All u B 2^M hybrid rows "x on the coalition's columns, b elsewhere", ordered (row, coalition mask, background row);
    bit m of the mask says that player m is in the coalition."""
    newdata, background = np.asarray(newdata, float), np.asarray(background, float)
    u, p = newdata.shape
    labels, M, cols = _players(labels, p)
    B = background.shape[0]
    out = np.empty((u, 2 ** M, B, p))
    for mask in range(2 ** M):
        inside = np.zeros(p, dtype=bool)
        for m in range(M):
            if mask >> m & 1:
                inside[cols[m]] = True
        out[:, mask] = np.where(inside[None, None, :], newdata[:, None, :], background[None, :, :])
    return out.reshape(u * 2 ** M * B, p), M


def shapley_from_values(v, M):
    """Shapley values (u x M) from the coalition values v (u x 2^M, indexed by mask), by the textbook sum."""
    u = v.shape[0]
    phi = np.zeros((u, M))
    for m in range(M):
        for mask in range(2 ** M):
            if mask >> m & 1:
                continue
            s = bin(mask).count("1")
            wgt = math.factorial(s) * math.factorial(M - 1 - s) / math.factorial(M)
            phi[:, m] += wgt * (v[:, mask | 1 << m] - v[:, mask])
    return phi


def brute_force(X, y, coeffs, sigma, newdata, background, labels=None, predict=None):
    rows, M = hybrid_rows(newdata, background, labels)
    f = predict_numpy(X, y, coeffs, sigma, rows) if predict is None else predict(rows)
    u, B = np.asarray(newdata).shape[0], np.asarray(background).shape[0]
    v = np.asarray(f, float).reshape(u, 2 ** M, B).mean(axis=2)
    return shapley_from_values(v, M), v


def _data(n, p, u, B, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) * (1.0 + np.arange(p)) + np.arange(p)
    y = rng.standard_normal(n)
    c = rng.standard_normal(n) / np.sqrt(n)
    return X, y, c, rng.standard_normal((u, p)) * (1.0 + np.arange(p)) + np.arange(p), X[rng.choice(n, B, replace=False)]


BRUTE_CASES = [(1, None), (2, None), (3, None), (6, None), (6, [0, 1, 2, 0, 2, 2])]   # the last: groups {1,4},{2},{3,5,6}


@pytest.mark.parametrize("p,labels", BRUTE_CASES)
def test_restatement_equals_brute_force_over_all_coalitions(p, labels):
    X, y, c, Z, Bg = _data(23, p, 4, 3, 100 + p)
    phi, baseline, _ = shapley_numpy(X, y, c, float(p), Z, Bg, labels)
    want, v = brute_force(X, y, c, float(p), Z, Bg, labels)
    assert np.max(np.abs(y)) < 10.0                                  # |y| = O(1): the tolerance is absolute
    assert phi.shape == want.shape
    assert np.max(np.abs(phi - want)) <= 1e-12
    # efficiency and the baseline: v(empty) is the mean prediction at the background rows, v(all) the row's own prediction
    assert abs(baseline - np.mean(predict_numpy(X, y, c, float(p), Bg))) <= 1e-12
    assert np.max(np.abs(v[:, 0] - baseline)) <= 1e-12
    assert np.max(np.abs(phi.sum(axis=1) + baseline - predict_numpy(X, y, c, float(p), Z))) <= 1e-12


def test_more_nodes_than_needed_change_nothing_and_fewer_do():
    X, y, c, Z, Bg = _data(19, 7, 3, 2, 7)
    Xs, _, _, (Zs, Bs) = _standardise(X, y, Z, Bg)
    W = shapley_weights_numpy(Zs, Xs, Bs, 7.0)                       # ceil(7/2) = 4 nodes
    assert np.max(np.abs(W - shapley_weights_numpy(Zs, Xs, Bs, 7.0, nodes=7))) <= 1e-15
    assert np.max(np.abs(W - shapley_weights_numpy(Zs, Xs, Bs, 7.0, nodes=3))) > 1e-9


def test_weights_are_exactly_zero_where_row_and_background_agree():
    X, y, c, Z, Bg = _data(17, 5, 2, 1, 9)
    W = shapley_weights_numpy(Bg, X, Bg, 5.0)                        # the explained row IS the background row
    assert np.all(W == 0.0)
    Z2 = Bg.repeat(2, axis=0)
    Z2[:, [0, 3]] += 1.0                                             # players 1 and 2 and 4 agree with the background
    W2 = shapley_weights_numpy(Z2, X, Bg, 5.0).reshape(2, 5, 17)
    assert np.all(W2[:, [1, 2, 4], :] == 0.0) and np.all(W2[:, [0, 3], :] != 0.0)


def test_se_is_the_quadratic_form_in_either_scaling():
    X, y, c, Z, Bg = _data(21, 4, 3, 2, 13)
    y = 5.0 * y
    A = np.random.default_rng(1).standard_normal((21, 21))
    vc = A @ A.T * y.std(ddof=1) ** 2                                # "vcov.est.c" carries sd(y)^2
    phi, _, se = shapley_numpy(X, y, c, 4.0, Z, Bg, vcov_c=vc, neffective=10.0)
    Xs, _, ys, (Zs, Bs) = _standardise(X, y, Z, Bg)
    W = shapley_weights_numpy(Zs, Xs, Bs, 4.0)
    want = np.sqrt(math.sqrt(21 / 10.0) * np.diag(W @ vc @ W.T)).reshape(3, 4)
    assert np.allclose(se, want, rtol=1e-13, atol=0)


# --------------------------------------------------------------------------
# the deterministic background and the groups
# --------------------------------------------------------------------------
def test_background_rule():
    from bigkrls_amd.api import _shapley_background
    for n, B in [(10, 1), (10, 3), (10, 10), (10, 11), (97, 13), (20000, 100), (7, 6)]:
        idx = _shapley_background(n, B)
        if B >= n:
            assert np.array_equal(idx, np.arange(n))
            continue
        assert np.array_equal(idx, [((2 * k + 1) * n) // (2 * B) for k in range(B)])
        assert idx.size == B and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(_shapley_background(10, 1), [5]) and np.array_equal(_shapley_background(10, 3), [1, 5, 8])
    assert np.array_equal(_shapley_background(97, 13), _shapley_background(97, 13))      # no random numbers


def test_groups_become_players():
    from bigkrls_amd.api import _shapley_players
    lab, players = _shapley_players(None, 4)
    assert np.array_equal(lab, [0, 1, 2, 3]) and players == [[1], [2], [3], [4]]
    lab, players = _shapley_players([[1, 4], [2], [3, 5, 6]], 6)
    assert np.array_equal(lab, [0, 1, 2, 0, 2, 2]) and players == [[1, 4], [2], [3, 5, 6]]
    lab, players = _shapley_players([[5, 2]], 5)                     # unlisted columns: players of their own, behind
    assert np.array_equal(lab, [1, 0, 2, 3, 0]) and players == [[2, 5], [1], [3], [4]]
    lab, players = _shapley_players(["a", "b", "a", "c", "b"], 5)     # a label vector: players by first appearance
    assert np.array_equal(lab, [0, 1, 0, 2, 1]) and players == [[1, 3], [2, 5], [4]]
    lab, players = _shapley_players(np.array([2, 0, 1, 0, 2, 2, 1, 0, 3]), 9)
    assert np.array_equal(lab, [0, 1, 2, 1, 0, 0, 2, 1, 3]) and players == [[1, 5, 6], [2, 4, 8], [3, 7], [9]]


# --------------------------------------------------------------------------
# the C ABI and its ctypes table
# --------------------------------------------------------------------------
def _header_arity(name):
    src = open(os.path.join(ROOT, "include", "bigkrls.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} not declared in include/bigkrls.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,arity", [("bigkrls_dev_shapley_weights", 12), ("bigkrls_shapley_effects", 23)])
def test_header_declares_and_ctypes_table_matches(name, arity):
    from bigkrls_amd import _lib
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name]) == _header_arity(name) == arity


def test_library_exports_the_symbols():
    from bigkrls_amd import _lib
    lib = _lib.load()
    for name in ("bigkrls_dev_shapley_weights", "bigkrls_shapley_effects"):
        assert getattr(lib, name) is not None


def test_public_api_exports_shapley_effects():
    import bigkrls_amd as bk
    from bigkrls_amd import ops
    assert callable(bk.shapley_effects) and "shapley_effects" in bk.__all__
    assert callable(ops.bShapleyWeights)


# --------------------------------------------------------------------------
# validation happens in Python, before any native call (no GPU here)
# --------------------------------------------------------------------------
def _object(n=40, p=3, vcov=True):
    from bigkrls_amd.api import BigKRLS
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, p))
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


def test_native_call_takes_the_23_arguments(no_native_capture):
    import bigkrls_amd as bk
    with pytest.raises(_Reached) as ei:
        bk.shapley_effects(_object(), background=7, groups=[[1, 3]])
    a = ei.value.args_
    assert a[0] == "bigkrls_shapley_effects" and len(a) - 1 == 23
    assert a[9] == 2 and a[10] is None and a[11] == 40 and a[13] == 7        # M, newdata = None -> NULL, u = n, B


def test_bad_groups_raise(no_native):
    import bigkrls_amd as bk
    obj = _object()
    for bad, text in [([[1, 2], [2, 3]], "more than once"), ([[1, 4]], "outside 1..3"), ([[0]], "outside 1..3"),
                      ([[1], []], "is empty"), ([0, 1], "vector of 3 labels"), ([[1, 1]], "more than once")]:
        with pytest.raises(ValueError, match=text):
            bk.shapley_effects(obj, groups=bad)


def test_more_players_than_the_cap_raise(no_native):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match="129 players; at most 128"):
        bk.shapley_effects(_object(n=140, p=129))
    with pytest.raises(AssertionError, match="native call reached"):          # grouped below the cap: goes on
        bk.shapley_effects(_object(n=140, p=129), groups=[[1, 2]])


def test_bad_background_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    for bad, text in [(0, "at least 1"), (-3, "at least 1"), (np.zeros((5, 4)), "ncol"), (np.zeros((0, 3)), "no rows"),
                      (np.full((2, 3), np.nan), "missing or infinite")]:
        with pytest.raises(ValueError, match=text):
            bk.shapley_effects(obj, background=bad)


def test_bad_newdata_and_block_rows_raise(no_native):
    import bigkrls_amd as bk
    obj = _object()
    with pytest.raises(ValueError, match="ncol"):
        bk.shapley_effects(obj, newdata=np.zeros((5, 4)))
    with pytest.raises(ValueError, match="missing or infinite"):
        bk.shapley_effects(obj, newdata=np.full((2, 3), np.inf))
    with pytest.raises(ValueError, match="block_rows"):
        bk.shapley_effects(obj, block_rows=-1)


def test_not_a_bigkrls_object_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(TypeError, match="bigKRLS"):
        bk.shapley_effects({"X": np.zeros((3, 2))})


def test_se_without_any_vcov_form_raises(no_native):
    import bigkrls_amd as bk
    with pytest.raises(ValueError, match="vcov.est=TRUE"):
        bk.shapley_effects(_object(vcov=False), se=True)
    with pytest.raises(ValueError, match="vcov must be"):
        bk.shapley_effects(_object(), se=True, vcov="sparse")


def test_multi_gpu_object_with_sharded_matrix_only_raises(no_native):
    import bigkrls_amd as bk
    obj = _object()
    obj["vcov.est.c.cols"] = (0, 20)
    with pytest.raises(NotImplementedError, match="shapley_effects of a multi-GPU fit"):
        bk.shapley_effects(obj, se=True)
    with pytest.raises(AssertionError, match="native call reached"):          # without se it is accepted
        bk.shapley_effects(obj)
