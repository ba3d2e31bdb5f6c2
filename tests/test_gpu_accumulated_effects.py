"""accumulated_effects() on the GPU: the fused binned leave-one-column-out pass (bigkrls_dev_kernel_loo_binsums) against
the direct per-bin sum in extended precision and against the unfused chain (one bKernelLooColsums per column and bin on
the bin's gathered rows), and the whole path against brute force through predict() -- per bin one prediction on the
bin's rows rewritten to the upper edge and one to the lower edge --, from both forms of vcov.est.c, on an implicit fit
that never stored K, and from the factors of robust_vcov()."""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_ale_cpu", os.path.join(_HERE, "test_accumulated_effects_cpu.py"))
_ale_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ale_cpu)
ale_numpy, ale_bins = _ale_cpu.ale_numpy, _ale_cpu.ale_bins


@pytest.fixture(scope="module")
def ctx():
    import bigkrls_amd as bk
    return bk.api.default_context()


# ---- Level 2: the fused pass -------------------------------------------------------------------------------------
GROUP = 64  # KL_GROUP, csrc/ktplan.h: selected columns per launch


def _sizes(sizes):
    """labels of bins with these sizes, in bin order"""
    return np.repeat(np.arange(len(sizes)), sizes)


def _labels(case, u, cols, rng):
    """(labels u x len(cols), nbins) of a case: every column shuffles its own rows"""
    kind = BIN_CASES[case][4]
    lab = np.empty((u, len(cols)), dtype=np.int64)
    if kind == "one":
        nbins = [1] * len(cols)
        lab[:] = 0
    elif kind == "three":
        nbins = [3] * len(cols)
        for jj in range(len(cols)):
            lab[:, jj] = rng.permutation(_sizes([u // 3, u // 3, u - 2 * (u // 3)]))
    elif kind == "1/15/1":                       # a single-row bin; a segment that starts in the middle of a tile
        nbins = [3] * len(cols)
        for jj in range(len(cols)):
            lab[:, jj] = rng.permutation(_sizes([1, u - 2, 1])) if jj else _sizes([1, u - 2, 1])
    elif kind == "unequal4":
        nbins = [4] * len(cols)
        for jj in range(len(cols)):
            lab[:, jj] = rng.permutation(_sizes([3, 40, 5, u - 48]))
    elif kind == "two":
        nbins = [2] * len(cols)
        for jj in range(len(cols)):
            lab[:, jj] = rng.permutation(_sizes([u // 2 + jj % 3, u - u // 2 - jj % 3]))
    else:                                        # "mixed": another number of bins per column, an empty bin, column 0 twice
        nbins = [1, 4, 2, 3, 5]
        for jj, nb in enumerate(nbins):
            lab[:, jj] = rng.integers(0, nb, size=u)
        lab[lab[:, 4] == 2, 4] = 3               # bin 2 of the last selected column is empty
    return lab, nbins


BIN_CASES = [
    (1, 1, 1, [0], "one"),                                   # p = 1 writes the counts
    (15, 17, 1, [0], "three"),
    (17, 15, 3, [0, 1, 2], "1/15/1"),
    (65, 64, 8, list(range(8)), "unequal4"),
    (130, 513, 33, list(range(0, 33, 3)), "three"),          # KS = 0
    (33, 40, 70, list(range(GROUP + 1)), "two"),             # one column more than a launch takes
    (4099, 17, 5, list(range(5)), "two"),                    # long bins: cut into several segments (tests/test_binplan_cpu.py)
    (17, 4099, 5, [4, 0], "two"),                            # selected columns out of order
    (70, 90, 9, [8, 0, 3, 0, 2], "mixed"),
]


@functools.lru_cache(maxsize=None)
def _bin_inputs(case, wide):
    """(A, B, sigma, cols, labels, nbins, longdouble reference): the direct per-bin sum over the other columns, computed
    once per case."""
    u, v, p, cols, _ = BIN_CASES[case]
    rng = np.random.default_rng(2000 * case + u + v + p)
    A = rng.standard_normal((u, p)) * 0.7
    B = rng.standard_normal((v, p)) * 0.7
    lab, nbins = _labels(case, u, cols, rng)
    if wide:                                   # a wide, uncentred column: the cancellation in d2 - dj^2 is real
        A[:, 0] = A[:, 0] * 40.0 + 1000.0
        B[:, 0] = B[:, 0] * 40.0 + 1000.0
    sigma = float(p)
    ref = _ale_cpu.loo_binsums_numpy(A, B, sigma, cols, lab, nbins, dtype=np.longdouble)
    for a in (A, B, lab, ref):
        a.setflags(write=False)
    return A, B, sigma, cols, lab, nbins, ref


def _restatement_f64(A, B, sigma, cols, lab, nbins):
    """The formula of the pass in float64 numpy: both operands moved by the column means of ALL of A, d2 = max(|a|^2 +
    |b|^2 - 2 a.b, 0), then max(d2 - dj^2, 0), summed per bin."""
    sh = A.mean(axis=0)
    Ac, Bc = A - sh, B - sh
    d2 = np.maximum((Ac ** 2).sum(axis=1)[:, None] + (Bc ** 2).sum(axis=1)[None, :] - 2.0 * (Ac @ Bc.T), 0.0)
    out = np.zeros((B.shape[0], int(np.sum(nbins))))
    at = 0
    for jj, c in enumerate(cols):
        dj = Ac[:, c][:, None] - Bc[:, c][None, :]
        E = np.exp(-np.maximum(d2 - dj * dj, 0.0) / sigma)
        for b in range(nbins[jj]):
            out[:, at + b] = E[lab[:, jj] == b].sum(axis=0)
        at += nbins[jj]
    return out


def _run_bins(ctx, A, B, sigma, cols, lab, nbins):
    from bigkrls_amd import ops
    return ops.bKernelLooBinsums(ctx.from_numpy(A), ctx.from_numpy(B), sigma, cols, lab, nbins).to_numpy()


def _err(got, ref):
    """the largest error of an output column, i.e. of a (column, bin), relative to that column's largest entry: a small
    bin cannot hide behind a large one. An empty bin's column must be exactly zero."""
    scale = np.max(np.abs(ref), axis=0)
    diff = np.max(np.abs(got.astype(np.longdouble) - ref), axis=0)
    assert np.all(diff[scale == 0] == 0)
    return float(np.max(diff[scale > 0] / scale[scale > 0]))


@pytest.mark.parametrize("case", range(len(BIN_CASES)))
def test_loo_binsums_against_extended_precision(ctx, case):
    A, B, sigma, cols, lab, nbins, ref = _bin_inputs(case, False)
    got = _run_bins(ctx, A, B, sigma, cols, lab, nbins)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    err = _err(got, ref)
    print(f"loo_binsums {BIN_CASES[case][:3]} ncols={len(cols)} bins={sum(nbins)}: error {err:.3e} "
          f"(float64 numpy: {_err(_restatement_f64(A, B, sigma, cols, lab, nbins), ref):.3e})")
    if A.shape[1] == 1:                        # nothing is left of the distance: the counts, exactly
        assert np.array_equal(got, np.broadcast_to(np.bincount(lab[:, 0], minlength=nbins[0]), got.shape))
    assert err < 1e-13


@pytest.mark.parametrize("case", range(len(BIN_CASES)))
def test_loo_binsums_wide_uncentred_column(ctx, case):
    A, B, sigma, cols, lab, nbins, ref = _bin_inputs(case, True)
    got = _run_bins(ctx, A, B, sigma, cols, lab, nbins)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    err = _err(got, ref)
    err64 = _err(_restatement_f64(A, B, sigma, cols, lab, nbins), ref)
    bound = max(20.0 * err64, 1e-13)
    print(f"loo_binsums wide {BIN_CASES[case][:3]} ncols={len(cols)} bins={sum(nbins)}: error {err:.3e}, "
          f"float64 numpy {err64:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("case", range(len(BIN_CASES)))
def test_loo_binsums_equals_unfused_chain_and_is_reproducible(ctx, case):
    from bigkrls_amd import ops
    A, B, sigma, cols, lab, nbins, _ = _bin_inputs(case, False)
    got = _run_bins(ctx, A, B, sigma, cols, lab, nbins)
    again = _run_bins(ctx, A, B, sigma, cols, lab, nbins)
    assert np.array_equal(got, again)
    dB = ctx.from_numpy(B)
    chain = np.zeros_like(got)
    at = 0
    for jj, c in enumerate(cols):
        for b in range(nbins[jj]):
            rows = np.flatnonzero(lab[:, jj] == b)
            if rows.size:
                dA = ctx.from_numpy(np.asfortranarray(A[rows]))
                chain[:, at + b] = ops.bKernelLooColsums(dA, dB, sigma, [c]).to_numpy().ravel()
        at += nbins[jj]
    assert np.max(np.abs(got - chain)) <= 1e-13 * np.max(np.abs(chain))


def test_loo_binsums_rejects_bad_labels_naming_row_and_column(ctx):
    from bigkrls_amd import _lib, ops
    A, B, sigma, cols, lab, nbins, _ = _bin_inputs(2, False)
    dA, dB = ctx.from_numpy(A), ctx.from_numpy(B)
    for value in (3, -1):
        bad = np.array(lab)
        bad[3, 1] = value
        with pytest.raises(_lib.BigKRLSError, match=r"the label of row 4 of selected column 2 is outside \[0, 3\)") as ei:
            ops.bKernelLooBinsums(dA, dB, sigma, cols, bad, nbins)
        assert ei.value.code == _lib.EINVAL
    with pytest.raises(_lib.BigKRLSError, match="selected column 3 must have at least 1 bin") as ei:
        ops.bKernelLooBinsums(dA, dB, sigma, cols, lab, [3, 3, 0])
    assert ei.value.code == _lib.EINVAL
    with pytest.raises(_lib.BigKRLSError, match=r"column index 3 outside \[0, 3\)"):
        ops.bKernelLooBinsums(dA, dB, sigma, [0, 1, 3], lab, nbins)


def test_loo_binsums_profile_name(ctx):
    A, B, sigma, cols, lab, nbins, _ = _bin_inputs(3, False)
    ctx.set_profile(True)
    try:
        _run_bins(ctx, A, B, sigma, cols, lab, nbins)
        ms, work, launches = ctx.get_profile("kernel_loo_binsums")
    finally:
        ctx.set_profile(False)
    assert launches == 1 and work == A.shape[0] * B.shape[0] * len(cols)


# ---- fits shared by the tests below ---------------------------------------------------------------------------------
def _small_data():
    from oracle import krls_oracle as orc
    return orc.synth(300, 5, 21, binary_last=True)


@pytest.fixture(scope="module")
def fit_small():
    import bigkrls_amd as bk
    X, y = _small_data()
    return bk.bigKRLS(y, X)


@pytest.fixture(scope="module")
def fit_small_both():
    import bigkrls_amd as bk
    X, y = _small_data()
    return bk.bigKRLS(y, X, vcov_form="both")


def _host(M):
    return M.to_numpy() if hasattr(M, "to_numpy") else np.asarray(M)


def _brute_force(out, res, R, correct_SE, vcov=None):
    """Every curve of `res` against predict(se_pred=True) on the stacked rewritten rows of its column: per bin the
    bin's rows at the upper edge, then at the lower edge. ale = omega' predicted within 1e-9 of max |ale| over all
    curves (the rows of omega sum to zero, so mean(y) cancels); se.ale^2 and the diagonal of vcov.ale within 1e-8
    relative of omega' V omega, V = vcov.est.pred; the off-diagonal entries, which may cancel to nothing, within 1e-8 of
    sqrt(V_gg V_hh), the scale on which a covariance is that accurate."""
    import bigkrls_amd as bk
    u = R.shape[0]
    ale_scale = max(np.max(np.abs(np.concatenate(res["ale"]))), 1e-300)
    for jj, w in enumerate(res["which"]):
        e, cnt = res["edges"][jj], res["counts"][jj]
        B = e.size - 1
        lab, cnt_ref = ale_bins(R[:, w - 1], e)
        assert np.array_equal(cnt, cnt_ref) and cnt.sum() == u
        rows, Wl, at = [], np.zeros((B, 2 * u)), 0
        for b in range(B):
            inb = lab == b
            hi, lo = R[inb].copy(), R[inb].copy()
            hi[:, w - 1], lo[:, w - 1] = e[b + 1], e[b]
            rows += [hi, lo]
            nb = int(cnt[b])
            Wl[b, at:at + nb] = 1.0 / nb
            Wl[b, at + nb:at + 2 * nb] = -1.0 / nb
            at += 2 * nb
        pr = bk.predict(out, np.vstack(rows), se_pred=True, correct_SE=correct_SE, vcov=vcov)
        local = Wl @ pr["predicted"].ravel()
        g = np.concatenate([[0.0], np.cumsum(local)])
        ale = g - np.sum(cnt * (g[:-1] + g[1:]) / 2.0) / u
        assert np.max(np.abs(res["ale"][jj] - ale)) <= 1e-9 * ale_scale, w
        assert np.max(np.abs(res["local"][jj] - np.diff(res["ale"][jj]))) == 0.0
        wgt = np.zeros(B + 1)
        wgt[:-1] += cnt / (2.0 * u)
        wgt[1:] += cnt / (2.0 * u)
        Om = (np.eye(B + 1) - np.outer(np.ones(B + 1), wgt)) @ np.tril(np.ones((B + 1, B)), -1) @ Wl
        cov = Om @ _host(pr["vcov.est.pred"]) @ Om.T
        var = np.diag(cov)
        assert np.all(np.abs(res["se.ale"][jj] ** 2 - var) <= 1e-8 * var), w
        assert np.all(np.abs(np.diag(res["vcov.ale"][jj]) - var) <= 1e-8 * var), w
        assert np.all(np.abs(res["vcov.ale"][jj] - cov) <= 1e-8 * np.sqrt(np.outer(var, var))), w
        # the local effects' standard errors from the same matrix
        vloc = var[1:] + var[:-1] - 2.0 * np.diag(cov, 1)
        assert np.all(np.abs(res["se.local"][jj] ** 2 - vloc) <= 1e-8 * (var[1:] + var[:-1])), w
        # the centring: sum_b n_b (ale_{b-1} + ale_b) / 2 = 0
        a = res["ale"][jj]
        assert abs(np.sum(cnt * (a[:-1] + a[1:]) / 2.0)) <= 1e-12 * u * np.max(np.abs(a)), w


# ---- brute force through the public API, dense form -------------------------------------------------------------------
@pytest.mark.parametrize("correct_SE", [True, False])
def test_against_predict_on_rewritten_rows(fit_small, correct_SE):
    import bigkrls_amd as bk
    out = fit_small
    X = out["X"]
    res = bk.accumulated_effects(out, bins=5, correct_SE=correct_SE)
    assert res["which"] == [1, 2, 3, 4, 5] and list(res["binaryindicator"]) == [False] * 4 + [True]
    assert [e.size for e in res["edges"]] == [6, 6, 6, 6, 2]
    assert np.array_equal(res["edges"][4], [X[:, 4].min(), X[:, 4].max()]) and list(res["counts"][4]) == [300]
    assert np.array_equal(res["edges"][0], np.unique(np.quantile(X[:, 0], np.arange(6) / 5, method="inverted_cdf")))
    assert all(c.sum() == 300 and np.all(c > 0) for c in res["counts"]) and res["newdata"] is None
    _brute_force(out, res, X, correct_SE)
    # the binary column: ale = (-d / 2, +d / 2), and d is partial_dependence()'s first difference
    pd = bk.partial_dependence(out, which=[5], correct_SE=correct_SE)
    ym = float(np.mean(out["y"]))
    pd_scale = np.max(np.abs(np.concatenate(pd["pd"]) - ym))
    assert res["first.difference"].shape == (1, 5) and np.all(np.isnan(res["first.difference"][0, :4]))
    assert np.all(np.isnan(res["se.first.difference"][0, :4]))
    d = res["first.difference"][0, 4]
    assert abs(d - pd["first.difference"][0, 0]) <= 1e-9 * pd_scale
    assert abs(res["se.first.difference"][0, 4] - pd["se.first.difference"][0, 0]) <= 1e-8 * pd["se.first.difference"][0, 0]
    assert np.max(np.abs(res["ale"][4] - np.array([-d / 2.0, d / 2.0]))) <= 1e-12 * abs(d)
    assert res["local"][4][0] == d and res["se.local"][4][0] == res["se.first.difference"][0, 4]


def test_new_reference_rows_and_selected_columns(fit_small):
    import bigkrls_amd as bk
    out = fit_small
    rng = np.random.default_rng(9)
    R = out["X"][rng.choice(300, 37, replace=False)].copy()
    R[:, 1] = np.round(R[:, 1] * 2.0) / 2.0                 # ties: bins merge
    res = bk.accumulated_effects(out, which=[4, 2, 5], bins=20, newdata=R)
    assert res["edges"][1].size - 1 < 20 and all(np.all(c > 0) for c in res["counts"])
    assert np.array_equal(res["newdata"], R)
    _brute_force(out, res, R, True)


def test_without_variance_and_reproducible(fit_small):
    import bigkrls_amd as bk
    a = bk.accumulated_effects(fit_small, bins=5)
    b = bk.accumulated_effects(fit_small, bins=5, se=False)
    for k in ("se.ale", "vcov.ale", "se.local", "se.first.difference"):
        assert b[k] is None, k
    for x, y in zip(a["ale"], b["ale"]):
        assert np.array_equal(x, y)
    again = bk.accumulated_effects(fit_small, bins=5)
    for k in ("ale", "se.ale", "vcov.ale"):
        for x, y in zip(a[k], again[k]):
            assert np.array_equal(x, y), k


def test_explicit_edges_reproduce_the_int_path(fit_small):
    import bigkrls_amd as bk
    a = bk.accumulated_effects(fit_small, which=[2, 5, 1], bins=7)
    b = bk.accumulated_effects(fit_small, which=[2, 5, 1], bins=[np.array(e) for e in a["edges"]])
    for k in ("edges", "counts", "ale", "se.ale", "vcov.ale", "local", "se.local"):
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x, y), k


def test_refusals(fit_small):
    import bigkrls_amd as bk
    out = fit_small
    x = out["X"][:, 0]
    with pytest.raises(ValueError, match="bin 2 of column 1 holds no reference row"):
        bk.accumulated_effects(out, which=[1], bins=[np.array([x.min(), 0.0, np.nextafter(0.0, 1.0), x.max()])])
    with pytest.raises(ValueError, match="edges of column 1 do not cover the reference rows"):
        bk.accumulated_effects(out, which=[1], bins=[np.array([x.min(), 0.0, np.sort(x)[-2]])])
    Z = out["X"][:9].copy()
    Z[:, 2] = 0.5
    with pytest.raises(ValueError, match="one distinct value in column 3"):
        bk.accumulated_effects(out, newdata=Z)


def test_native_entry_refuses_on_its_own(fit_small, ctx):
    """The C entry makes the same checks for callers that do not come through Python, naming the column (and bin)."""
    from bigkrls_amd import _lib
    out = fit_small
    X = np.asfortranarray(out["X"])
    n, p = X.shape
    y = np.ascontiguousarray(out["y"], dtype=np.float64).ravel()
    c = np.ascontiguousarray(out["coeffs"], dtype=np.float64).ravel()
    x = X[:, 1]
    which = np.array([2], dtype=np.int64)
    cases = [
        (np.array([x.min()]), r"column 2 has 1 edges"),
        (np.array([x.min(), 0.0, 0.0, x.max()]), r"edges of column 2 are not strictly increasing at bin 2"),
        (np.array([x.min(), np.inf]), r"edge 2 of column 2 is missing or infinite"),
        (np.array([x.min(), 0.0, np.sort(x)[-2]]), r"reference row \d+ of column 2 lies outside the edges"),
        (np.array([x.min(), 0.0, np.nextafter(0.0, 1.0), x.max()]), r"bin 2 of column 2 holds no reference row"),
    ]
    for e, msg in cases:
        off = np.array([0, e.size], dtype=np.int64)
        ale = np.empty(e.size)
        with pytest.raises(_lib.BigKRLSError, match=msg) as ei:
            _lib.call("bigkrls_accumulated_effects", ctx.handle, X.ctypes.data, n, p, y.ctypes.data, c.ctypes.data,
                      float(out["sigma"]), which.ctypes.data, 1, None, n, e.ctypes.data, off.ctypes.data, None, None, 0, 0,
                      None, -1.0, ale.ctypes.data, None, None)
        assert ei.value.code == _lib.EINVAL


# ---- factors equal dense ---------------------------------------------------------------------------------------------
def test_factors_equal_dense(fit_small_both):
    import bigkrls_amd as bk
    out = fit_small_both
    d = bk.accumulated_effects(out, bins=5, vcov="dense")
    f = bk.accumulated_effects(out, bins=5, vcov="factors")
    se_max = max(np.max(s) for s in d["se.ale"])
    cov_max = max(np.max(np.abs(c)) for c in d["vcov.ale"])
    for jj in range(5):
        assert np.array_equal(d["ale"][jj], f["ale"][jj])
        assert np.max(np.abs(d["se.ale"][jj] - f["se.ale"][jj])) <= 1e-9 * se_max
        assert np.max(np.abs(d["vcov.ale"][jj] - f["vcov.ale"][jj])) <= 1e-9 * cov_max
    assert abs(d["se.first.difference"][0, 4] - f["se.first.difference"][0, 4]) <= 1e-9 * se_max


def _against_numpy(out, res, Vc, newdata=None):
    ales, ses, covs = ale_numpy(out["X"], out["y"], out["coeffs"], out["sigma"], res["which"], res["edges"],
                                newdata=newdata, vcov_c=Vc, neffective=out["Neffective"])
    ale_scale = max(np.max(np.abs(np.concatenate(ales))), 1e-300)
    se_max = max(np.max(s) for s in ses)
    for jj in range(len(res["which"])):
        assert np.max(np.abs(res["ale"][jj] - ales[jj])) <= 1e-9 * ale_scale, jj
        assert np.max(np.abs(res["se.ale"][jj] - ses[jj])) <= 1e-8 * se_max, jj
        assert np.max(np.abs(res["vcov.ale"][jj] - covs[jj])) <= 1e-8 * se_max ** 2, jj


# ---- implicit fit: no stored K is needed -----------------------------------------------------------------------------
def test_implicit_fit_against_numpy():
    import bigkrls_amd as bk
    from oracle import krls_oracle as orc
    # N = 1024 is the smallest size the mode accepts, and it has no dense fallback: the data of the implicit fit of
    # tests/test_gpu_interaction_effects.py, whose block Lanczos converges there (P = 4, the last column binary)
    X, y = orc.synth(1024, 4, 52, binary_last=True)
    out = bk.bigKRLS(y, X, Neig=64, kernel="implicit", vcov_form="factors", noisy=False)
    assert out["K"] is None and out.get("vcov.est.c") is None
    R = X[np.random.default_rng(5).choice(1024, 128, replace=False)]
    res = bk.accumulated_effects(out, which=[2, 4], bins=6, newdata=R)
    Q, w = _host(out["vcov.est.Q"]), np.asarray(out["vcov.est.w"]).ravel()
    _against_numpy(out, res, (Q * w) @ Q.T, newdata=R)


# ---- robust factors --------------------------------------------------------------------------------------------------
def test_robust_vcov_object_against_numpy(fit_small_both):
    import bigkrls_amd as bk
    rob = bk.robust_vcov(fit_small_both, type="HC1")
    res = bk.accumulated_effects(rob, which=[1, 5], bins=5)
    Q, w = _host(rob["vcov.est.Q"]), np.asarray(rob["vcov.est.w"]).ravel()
    _against_numpy(rob, res, (Q * w) @ Q.T)
    plain = bk.accumulated_effects(fit_small_both, which=[1, 5], bins=5)
    assert np.array_equal(plain["ale"][0], res["ale"][0]) and not np.array_equal(plain["se.ale"][0], res["se.ale"][0])
