"""shapley_effects() on the GPU: the weights kernel (bigkrls_dev_shapley_weights) against the numpy restatement of the
definition in extended precision with M nodes -- more than the ceil(M/2) the kernel uses, so the node count is checked
too -- its exact zeros, its finiteness when factors underflow and its bitwise repeatability; and the whole path against
brute force over all 2^M coalitions through predict(), efficiency, the standard errors from the dense matrix, from the
factors and from a robust_vcov() object, an implicit fit, the row blocks, newdata=None and the C ABI's error texts."""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_shap_cpu", os.path.join(_HERE, "test_shapley_effects_cpu.py"))
_shap_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_shap_cpu)
shapley_weights_numpy, shapley_numpy = _shap_cpu.shapley_weights_numpy, _shap_cpu.shapley_numpy
hybrid_rows, shapley_from_values = _shap_cpu.hybrid_rows, _shap_cpu.shapley_from_values


@pytest.fixture(scope="module")
def ctx():
    import bigkrls_amd as bk
    return bk.api.default_context()


# ---- Level 2: the weights ---------------------------------------------------------------------------------------------
# (u, n, B, p, players): None = one player per column
WEIGHT_CASES = [
    (1, 1, 1, 1, None),                                      # the smallest case
    (3, 65, 5, 2, None),                                     # one node
    (3, 63, 5, 3, None),
    (17, 130, 1, 7, None),                                   # odd M; rows that do not fill a thread's share
    (2, 63, 130, 33, None),                                  # more background rows than one LDS chunk (62); the bucket above 32
    (2, 40, 3, 67, None),                                    # the reference data's width: the last bucket
    (5, 70, 4, 9, [2, 0, 1, 0, 2, 2, 1, 0, 3]),              # grouped, columns out of order
    (4, 64, 3, 70, [c % 3 for c in range(70)]),              # 3 players, many columns per player
    (5, 66, 3, 12, None),                                    # the bucket of 16 (three rows per thread, a row count that is no multiple)
    (3, 30, 2, 20, None),                                    # the bucket of 20 (two rows per thread, an odd row count)
    (3, 31, 2, 23, None),                                    # the bucket of 24
    (2, 33, 2, 28, None),                                    # the bucket of 32
    (3, 20, 2, 4, [2, 0, 3, 1]),                             # one column per player, but player m is not column m
]


@functools.lru_cache(maxsize=None)
def _weight_inputs(case):
    """(Z, X, Bg, sigma, players, longdouble reference with M nodes), computed once per case"""
    u, n, B, p, players = WEIGHT_CASES[case]
    rng = np.random.default_rng(3000 * case + u + n + B + p)
    Z, X, Bg = (np.asfortranarray(rng.standard_normal((r, p)) * 0.7) for r in (u, n, B))
    sigma = float(p)
    M = p if players is None else max(players) + 1
    ref = shapley_weights_numpy(Z, X, Bg, sigma, players, nodes=M, dtype=np.longdouble)
    for a in (Z, X, Bg, ref):
        a.setflags(write=False)
    return Z, X, Bg, sigma, players, ref


def _run_weights(ctx, Z, X, Bg, sigma, players):
    from bigkrls_amd import ops
    return ops.bShapleyWeights(ctx.from_numpy(Z), ctx.from_numpy(X), ctx.from_numpy(Bg), sigma, players).to_numpy()


@pytest.mark.parametrize("case", range(len(WEIGHT_CASES)))
def test_weights_against_extended_precision(ctx, case):
    Z, X, Bg, sigma, players, ref = _weight_inputs(case)
    got = _run_weights(ctx, Z, X, Bg, sigma, players)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    scale = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(got.astype(np.longdouble) - ref))) / scale
    err64 = float(np.max(np.abs(shapley_weights_numpy(Z, X, Bg, sigma, players).astype(np.longdouble) - ref))) / scale
    print(f"shapley_weights {WEIGHT_CASES[case][:4]} M={ref.shape[0] // Z.shape[0]}: error {err:.3e} of max |W| "
          f"(float64 numpy: {err64:.3e})")
    assert err <= 1e-13
    # two calls are bitwise identical
    assert np.array_equal(got, _run_weights(ctx, Z, X, Bg, sigma, players))


@pytest.mark.parametrize("case", [3, 6, 8, 9])
def test_weights_of_a_row_block_are_bitwise_the_rows_of_the_whole(ctx, case):
    Z, X, Bg, sigma, players, ref = _weight_inputs(case)
    M = ref.shape[0] // Z.shape[0]
    whole = _run_weights(ctx, Z, X, Bg, sigma, players)
    for r0, r1 in [(0, 1), (1, Z.shape[0]), (2, 3)]:
        part = _run_weights(ctx, np.asfortranarray(Z[r0:r1]), X, Bg, sigma, players)
        assert np.array_equal(part, whole[r0 * M:r1 * M])


def test_factors_that_underflow_to_zero_give_finite_weights(ctx):
    rng = np.random.default_rng(77)
    u, n, B, p = 5, 20, 3, 2
    Z, X, Bg = (np.asfortranarray(rng.standard_normal((r, p)) * 0.7) for r in (u, n, B))
    Z[:, 0] *= 60.0
    sigma = float(p)
    assert np.any(np.exp(-(Z[:, 0][:, None] - X[:, 0][None, :]) ** 2 / sigma) == 0.0)      # the premise
    got = _run_weights(ctx, Z, X, Bg, sigma, None)
    ref = shapley_weights_numpy(Z, X, Bg, sigma, None, nodes=p, dtype=np.longdouble)
    assert np.all(np.isfinite(got))
    assert np.max(np.abs(got.astype(np.longdouble) - ref)) <= 1e-13 * np.max(np.abs(ref))


def test_exact_zeros(ctx):
    rng = np.random.default_rng(78)
    n, p = 70, 5
    X, Bg = (np.asfortranarray(rng.standard_normal((r, p)) * 0.7) for r in (n, 1))
    W = _run_weights(ctx, Bg, X, Bg, float(p), None)            # the explained row IS the one background row
    assert W.shape == (p, n) and np.all(W == 0.0)
    Z = np.asfortranarray(Bg.repeat(3, axis=0))
    Z[:, [0, 3]] += rng.standard_normal((3, 2))                 # players 1, 2 and 4 agree with the background row
    W = _run_weights(ctx, Z, X, Bg, float(p), None).reshape(3, p, n)
    assert np.all(W[:, [1, 2, 4], :] == 0.0) and np.all(W[:, [0, 3], :] != 0.0)
    lab = [0, 1, 1, 0, 2]                                       # grouped: players {1,4}, {2,3}, {5}
    W = _run_weights(ctx, Z, X, Bg, float(p), lab).reshape(3, 3, n)
    assert np.all(W[:, [1, 2], :] == 0.0) and np.all(W[:, 0, :] != 0.0)


def test_weights_profile_name(ctx):
    Z, X, Bg, sigma, players, ref = _weight_inputs(3)
    ctx.set_profile(True)
    try:
        _run_weights(ctx, Z, X, Bg, sigma, players)
        ms, work, launches = ctx.get_profile("shapley_weights")
    finally:
        ctx.set_profile(False)
    assert launches == 1 and work == 8 * 7 * 4 * 17 * 130 * 1


def test_weights_entry_refuses_naming_the_argument(ctx):
    from bigkrls_amd import _lib
    Z, X, Bg, sigma, _, _ = _weight_inputs(2)
    dZ, dX, dB = ctx.from_numpy(Z), ctx.from_numpy(X), ctx.from_numpy(Bg)
    out = ctx.empty(9, 63)

    def call(players, M, B=5):
        lab = None if players is None else np.ascontiguousarray(players, dtype=np.int64)
        _lib.call("bigkrls_dev_shapley_weights", ctx.handle, dZ.ptr, 3, dX.ptr, 63, dB.ptr, B, 3, sigma,
                  None if lab is None else lab.ctypes.data, M, out.ptr)

    for args, msg in [(([0, 1, 3], 3), r"players\[2\] = 3 is outside \[0, 3\)"),
                      (([0, -1, 1], 2), r"players\[1\] = -1 is outside \[0, 2\)"),
                      (([0, 2, 2], 3), r"player 1 owns no column"),
                      ((None, 2), r"M must equal p"),
                      (([0, 1, 2], 3, 0), r"B = 0; at least one background row")]:
        with pytest.raises(_lib.BigKRLSError, match=msg) as ei:
            call(*args)
        assert ei.value.code == _lib.EINVAL
    call([0, 1, 2], 3)                                          # ... and the valid call goes through


# ---- fits shared by the tests below ---------------------------------------------------------------------------------
def _host(M):
    return M.to_numpy() if hasattr(M, "to_numpy") else np.asarray(M)


@pytest.fixture(scope="module")
def fit5():
    import bigkrls_amd as bk
    from oracle import krls_oracle as orc
    X, y = orc.synth(60, 5, 31)
    return bk.bigKRLS(y, X, vcov_form="both", noisy=False)


@pytest.fixture(scope="module")
def fit6():
    import bigkrls_amd as bk
    from oracle import krls_oracle as orc
    X, y = orc.synth(90, 6, 32, binary_last=True)
    return bk.bigKRLS(y, X, vcov_form="both", noisy=False)


def _rows(out, u, seed):
    """u rows to explain: training rows moved a little (binary columns keep their values)"""
    X = np.asarray(out["X"])
    rng = np.random.default_rng(seed)
    Z = X[rng.choice(X.shape[0], u, replace=False)].copy()
    for j in range(X.shape[1]):
        if np.unique(X[:, j]).size > 2:
            Z[:, j] += 0.3 * X[:, j].std() * rng.standard_normal(u)
    return Z


def _brute_force(out, res, Z):
    """shapley, baseline and efficiency of `res` against predict() on all u B 2^M hybrid rows, in ONE predict call"""
    import bigkrls_amd as bk
    labels = np.empty(np.asarray(out["X"]).shape[1], dtype=np.int64)
    for m, cols in enumerate(res["players"]):
        labels[np.asarray(cols) - 1] = m
    Bg = res["background"]
    rows, M = hybrid_rows(Z, Bg, labels)
    f = bk.predict(out, rows)["predicted"].ravel()
    v = f.reshape(Z.shape[0], 2 ** M, Bg.shape[0]).mean(axis=2)
    want = shapley_from_values(v, M)
    bound = 1e-9 * max(1.0, float(np.max(np.abs(out["y"]))))
    err = float(np.max(np.abs(res["shapley"] - want)))
    eff = float(np.max(np.abs(res["shapley"].sum(axis=1) + res["baseline"] - bk.predict(out, Z)["predicted"].ravel())))
    print(f"shapley_effects M={M} u={Z.shape[0]} B={Bg.shape[0]}: brute force {err:.3e}, efficiency {eff:.3e}, "
          f"baseline {abs(res['baseline'] - v[0, 0]):.3e} (bound {bound:.3e})")
    assert res["shapley"].shape == want.shape
    assert err <= bound and eff <= bound
    assert abs(res["baseline"] - v[0, 0]) <= bound                        # v(empty) = the mean prediction at the background
    assert np.max(np.abs(res["predicted"] - (res["baseline"] + res["shapley"].sum(axis=1)))) == 0.0
    assert np.array_equal(res["importance"], np.abs(res["shapley"]).mean(axis=0, keepdims=True))


def test_against_brute_force_through_predict(fit5):
    import bigkrls_amd as bk
    Z = _rows(fit5, 4, 1)
    res = bk.shapley_effects(fit5, Z, background=3)
    assert res["players"] == [[1], [2], [3], [4], [5]] and res["se.shapley"] is None
    assert np.array_equal(res["background"], np.asarray(fit5["X"])[[10, 30, 50]]) and np.array_equal(res["newdata"], Z)
    _brute_force(fit5, res, Z)


def test_against_brute_force_with_a_binary_column(fit6):
    import bigkrls_amd as bk
    Z = _rows(fit6, 4, 2)
    res = bk.shapley_effects(fit6, Z, background=3)
    assert len(res["players"]) == 6
    _brute_force(fit6, res, Z)


def test_against_brute_force_with_groups(fit6):
    import bigkrls_amd as bk
    Z = _rows(fit6, 4, 3)
    res = bk.shapley_effects(fit6, Z, background=np.asarray(fit6["X"])[[5, 80, 41]], groups=[[1, 4], [3, 5, 6]])
    assert res["players"] == [[1, 4], [3, 5, 6], [2]]
    assert res["xlabs"] == ["x1+x4", "x3+x5+x6", "x2"]
    _brute_force(fit6, res, Z)


def _se_reference(out, res, Z, Vc, correct_SE, labels=None):
    _, _, se = shapley_numpy(out["X"], out["y"], out["coeffs"], out["sigma"], Z, res["background"], labels, vcov_c=Vc,
                             neffective=out["Neffective"] if correct_SE else None)
    return se


@pytest.mark.parametrize("correct_SE", [True, False])
def test_standard_errors_three_ways(fit6, correct_SE):
    import bigkrls_amd as bk
    Z = _rows(fit6, 5, 4)
    Vc = _host(fit6["vcov.est.c"])
    d = bk.shapley_effects(fit6, Z, background=4, se=True, vcov="dense", correct_SE=correct_SE)
    f = bk.shapley_effects(fit6, Z, background=4, se=True, vcov="factors", correct_SE=correct_SE)
    want = _se_reference(fit6, d, Z, Vc, correct_SE)
    Q, w = _host(fit6["vcov.est.Q"]), np.asarray(fit6["vcov.est.w"]).ravel()
    want_f = _se_reference(fit6, f, Z, (Q * w) @ Q.T, correct_SE)
    rob = bk.robust_vcov(fit6, type="HC1")
    r = bk.shapley_effects(rob, Z, background=4, se=True, correct_SE=correct_SE)
    Qr, wr = _host(rob["vcov.est.Q"]), np.asarray(rob["vcov.est.w"]).ravel()
    want_r = _se_reference(rob, r, Z, (Qr * wr) @ Qr.T, correct_SE)
    for name, got, ref in (("dense", d, want), ("factors", f, want_f), ("robust", r, want_r)):
        err = float(np.max(np.abs(got["se.shapley"] - ref))) / float(np.max(ref))
        print(f"se.shapley {name} correct_SE={correct_SE}: {err:.3e} of max se")
        assert got["se.shapley"].shape == (5, 6) and np.all(got["se.shapley"][:, :5] > 0.0)
        # the binary column: where the row agrees with all four background rows the weights are exactly 0
        assert np.array_equal(got["se.shapley"][:, 5] == 0.0, got["shapley"][:, 5] == 0.0)
        assert err <= 1e-9
    assert np.max(np.abs(d["se.shapley"] - f["se.shapley"])) <= 1e-9 * np.max(d["se.shapley"])
    assert np.array_equal(d["shapley"], f["shapley"]) and np.array_equal(d["shapley"], r["shapley"])
    assert not np.array_equal(d["se.shapley"], r["se.shapley"])
    if not correct_SE:                                                    # correct_SE drops f = sqrt(n / Neffective)
        with_f = bk.shapley_effects(fit6, Z, background=4, se=True, vcov="dense")
        fac = np.sqrt(np.sqrt(90.0 / float(fit6["Neffective"])))
        assert np.max(np.abs(with_f["se.shapley"] - fac * d["se.shapley"])) <= 1e-12 * np.max(with_f["se.shapley"])


def test_grouped_standard_errors(fit6):
    import bigkrls_amd as bk
    Z = _rows(fit6, 3, 5)
    res = bk.shapley_effects(fit6, Z, background=4, groups=[1, 2, 1, 3, 3, 2], se=True)
    assert res["players"] == [[1, 3], [2, 6], [4, 5]]
    want = _se_reference(fit6, res, Z, _host(fit6["vcov.est.c"]), True, labels=[0, 1, 0, 2, 2, 1])
    assert np.max(np.abs(res["se.shapley"] - want)) <= 1e-9 * np.max(want)


def test_row_blocks_and_repeatability(fit5):
    """n = 60: the products take one split for every block shape, so the rows are bitwise independent of the blocking
    (include/bigkrls.h)."""
    import bigkrls_amd as bk
    Z = _rows(fit5, 7, 6)
    a = bk.shapley_effects(fit5, Z, background=5, se=True)
    for br in (1, 3):
        b = bk.shapley_effects(fit5, Z, background=5, se=True, block_rows=br)
        assert np.array_equal(a["shapley"], b["shapley"]) and np.array_equal(a["se.shapley"], b["se.shapley"])
        assert a["baseline"] == b["baseline"]
    again = bk.shapley_effects(fit5, Z, background=5, se=True)
    assert np.array_equal(a["shapley"], again["shapley"]) and np.array_equal(a["se.shapley"], again["se.shapley"])


def test_newdata_none_explains_the_training_rows(fit5):
    import bigkrls_amd as bk
    X = np.asarray(fit5["X"])
    a = bk.shapley_effects(fit5, background=4, se=True)
    b = bk.shapley_effects(fit5, X, background=4, se=True)
    assert a["shapley"].shape == (60, 5) and np.array_equal(a["newdata"], X)
    assert np.array_equal(a["shapley"], b["shapley"]) and np.array_equal(a["se.shapley"], b["se.shapley"])
    bound = 1e-9 * max(1.0, float(np.max(np.abs(fit5["y"]))))
    assert np.max(np.abs(a["predicted"] - np.asarray(fit5["yfitted"]).ravel())) <= bound
    # all rows as background (B >= n): the baseline is the mean fitted value
    c = bk.shapley_effects(fit5, X[:2], background=1000)
    assert c["background"].shape == (60, 5) and abs(c["baseline"] - np.mean(fit5["yfitted"])) <= bound


def test_implicit_fit_equals_its_explicit_twin():
    """The implicit fit never stored K; shapley_effects never needs it. N = 1024 is the smallest size the mode accepts."""
    import bigkrls_amd as bk
    from oracle import krls_oracle as orc
    X, y = orc.synth(1024, 4, 52, binary_last=True)
    imp = bk.bigKRLS(y, X, Neig=64, kernel="implicit", vcov_form="factors", noisy=False)
    sto = bk.bigKRLS(y, X, Neig=64, vcov_form="factors", noisy=False)
    assert imp["K"] is None and imp.get("vcov.est.c") is None
    Z = _rows(imp, 6, 7)
    a = bk.shapley_effects(imp, Z, background=8, se=True)
    b = bk.shapley_effects(sto, Z, background=8, se=True)
    bound = 1e-9 * max(1.0, float(np.max(np.abs(y))))
    err = float(np.max(np.abs(a["shapley"] - b["shapley"])))
    own, base, se = shapley_numpy(X, y, imp["coeffs"], imp["sigma"], Z, a["background"],
                                  vcov_c=(_host(imp["vcov.est.Q"]) * np.asarray(imp["vcov.est.w"]).ravel())
                                  @ _host(imp["vcov.est.Q"]).T, neffective=imp["Neffective"])
    print(f"implicit vs stored: shapley {err:.3e} (bound {bound:.3e}); coeffs "
          f"{np.max(np.abs(np.asarray(imp['coeffs']) - np.asarray(sto['coeffs']))):.3e}; "
          f"implicit vs numpy from its own coefficients {np.max(np.abs(a['shapley'] - own)):.3e}")
    assert np.max(np.abs(a["shapley"] - own)) <= bound and abs(a["baseline"] - base) <= bound
    assert np.max(np.abs(a["se.shapley"] - se)) <= 1e-9 * np.max(se)
    assert err <= bound


def test_native_entry_refuses_on_its_own(fit5, ctx):
    """The C entry makes the same checks for callers that do not come through Python, naming the argument."""
    from bigkrls_amd import _lib
    X = np.asfortranarray(fit5["X"])
    n, p = X.shape
    y = np.ascontiguousarray(fit5["y"], dtype=np.float64).ravel()
    c = np.ascontiguousarray(fit5["coeffs"], dtype=np.float64).ravel()
    Z = np.asfortranarray(X[:3].copy())
    Bg = np.asfortranarray(X[5:7].copy())
    phi, se, base = np.empty(3 * p), np.empty(3 * p), np.empty(1)

    def call(players=None, M=p, Z=Z, Bg=Bg, B=2, se_ptr=None, block_rows=0):
        lab = None if players is None else np.ascontiguousarray(players, dtype=np.int64)
        _lib.call("bigkrls_shapley_effects", ctx.handle, X.ctypes.data, n, p, y.ctypes.data, c.ctypes.data,
                  float(fit5["sigma"]), None if lab is None else lab.ctypes.data, M, Z.ctypes.data, 3, Bg.ctypes.data, B,
                  None, None, 0, 0, None, -1.0, block_rows, phi.ctypes.data, se_ptr, base.ctypes.data)

    badZ, badB = Z.copy(), Bg.copy()
    badZ[1, 2] = np.nan
    badB[0, 0] = np.inf
    many = np.arange(200) % 129
    for kw, msg in [(dict(players=[0, 1, 2, 3, 5]), r"players\[4\] = 5 is outside \[0, 5\)"),
                    (dict(players=[0, 1, 1, 3, 3], M=4), r"player 2 owns no column"),
                    (dict(B=0), r"B = 0; at least one background row"),
                    (dict(Z=badZ), r"newdata contains missing or infinite values"),
                    (dict(Bg=badB), r"background contains missing or infinite values"),
                    (dict(players=many[:5], M=129), r"M = 129 players; at most 128"),
                    (dict(se_ptr=se.ctypes.data), r"h_se and h_cov are written only when vcov.est.c"),
                    (dict(block_rows=-1), r"block_rows must not be negative")]:
        with pytest.raises(_lib.BigKRLSError, match=msg) as ei:
            call(**kw)
        assert ei.value.code == _lib.EINVAL
    call()
    assert np.all(np.isfinite(phi)) and np.isfinite(base[0])
