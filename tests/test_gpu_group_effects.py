"""group_effects() on the GPU: the grouped fused contraction (bigkrls_dev_kernel_contract_grouped) against the direct
sum in extended precision, against one bigkrls_dev_kernel_contract(trans = 1) per group and against itself, and the whole
path against the oracle of tests/test_group_effects_cpu.py, against one marginal_effects() per group, against the pooled
identities that pin the covariances between groups, from both forms of vcov.est.c and on an implicit fit."""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_ge_cpu", os.path.join(_HERE, "test_group_effects_cpu.py"))
_ge_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ge_cpu)
ge_numpy = _ge_cpu.ge_numpy


@pytest.fixture(scope="module")
def ctx():
    import bigkrls_amd as bk
    return bk.api.default_context()


# ---- Level 2: the grouped pass ---------------------------------------------------------------------------------------
def _sizes(*sizes):
    return np.repeat(np.arange(len(sizes)), sizes)


# (u, v, p, q, labels, G)
GRP_CASES = [
    (1, 1, 1, 1, _sizes(1), 1),                               # minimal
    (50, 17, 2, 3, _sizes(1, 15, 16, 17, 1), 5),              # boundaries off the 16-row tile
    (130, 65, 8, 17, _sizes(64, 1, 65), 3),                   # CT = 2
    (200, 129, 20, 21, np.arange(200) % 7, 7),                # interleaved labels: the permutation path
    (140, 130, 33, 34, _sizes(33, 100, 7), 3),                # KS = 0, CT = 4
    (90, 70, 5, 71, _sizes(45, 45), 2),                       # two column chunks
    (4116, 17, 5, 6, _sizes(4099, 17), 2),                    # one group cut into several segments, one not
    (33, 40, 4, 5, _sizes(10, 0, 20, 3), 4),                  # an empty group gives exact zeros
]
assert all(len(lab) == u and lab.max() < G for u, _, _, _, lab, G in GRP_CASES)


@functools.lru_cache(maxsize=None)
def _grp_inputs(case, wide):
    """(A, B, W, sigma, labels, G, longdouble reference v x G q, its scale: the max over the outputs of sum_i |W| e),
    computed once per case."""
    u, v, p, q, labels, G = GRP_CASES[case]
    rng = np.random.default_rng(3000 * case + u + v + p + q)
    A = rng.standard_normal((u, p)) * 0.7
    B = rng.standard_normal((v, p)) * 0.7
    W = rng.standard_normal((u, q)) * 0.7
    if wide:                                   # a wide, uncentred column: |a|^2 + |b|^2 - 2 a.b cancels unless centred
        A[:, 0] = A[:, 0] * 40.0 + 1000.0
        B[:, 0] = B[:, 0] * 40.0 + 1000.0
    sigma = float(p)
    Al, Bl, Wl = (x.astype(np.longdouble) for x in (A, B, W))
    d2 = ((Al[:, None, :] - Bl[None, :, :]) ** 2).sum(axis=2)
    K = np.exp(-d2 / np.longdouble(sigma))                     # u x v
    ref = np.zeros((v, G * q), dtype=np.longdouble)
    scale = np.zeros((v, G * q), dtype=np.longdouble)
    for g in range(G):
        rows = labels == g
        ref[:, g * q:(g + 1) * q] = K[rows].T @ Wl[rows]
        scale[:, g * q:(g + 1) * q] = K[rows].T @ np.abs(Wl[rows])
    for a in (A, B, W, ref):
        a.setflags(write=False)
    return A, B, W, sigma, labels, G, ref, float(scale.max())


def _restatement_f64(A, B, W, sigma, labels, G):
    """The formula of the pass in float64 numpy: both operands moved by the column means of A, d2 = max(|a|^2 + |b|^2 -
    2 a.b, 0)."""
    sh = A.mean(axis=0)
    Ac, Bc = A - sh, B - sh
    d2 = np.maximum((Ac ** 2).sum(axis=1)[:, None] + (Bc ** 2).sum(axis=1)[None, :] - 2.0 * (Ac @ Bc.T), 0.0)
    K = np.exp(-d2 / sigma)
    q = W.shape[1]
    out = np.zeros((B.shape[0], G * q))
    for g in range(G):
        out[:, g * q:(g + 1) * q] = K[labels == g].T @ W[labels == g]
    return out


def _run_grp(ctx, A, B, W, sigma, labels, G):
    from bigkrls_amd import ops
    return ops.bKernelContractGrouped(ctx.from_numpy(A), ctx.from_numpy(B), ctx.from_numpy(W), sigma, labels, G).to_numpy()


def _err(got, ref, scale):
    return float(np.max(np.abs(got.astype(np.longdouble) - ref)) / scale)


@pytest.mark.parametrize("case", range(len(GRP_CASES)))
def test_grouped_contract_three_ways(ctx, case):
    """Against the direct sum in extended precision, against bKernelContract(trans=1) on each group's rows, and against a
    second call, bit for bit."""
    from bigkrls_amd import ops
    A, B, W, sigma, labels, G, ref, scale = _grp_inputs(case, False)
    q = W.shape[1]
    got = _run_grp(ctx, A, B, W, sigma, labels, G)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    err = _err(got, ref, scale)
    print(f"kernel_contract_grouped {GRP_CASES[case][:4]} G={G}: error {err:.3e}")
    assert err < 1e-13
    dB = ctx.from_numpy(B)
    for g in range(G):
        rows = labels == g
        blk = got[:, g * q:(g + 1) * q]
        if not rows.any():
            assert np.array_equal(blk, np.zeros_like(blk))
            continue
        want = ops.bKernelContract(ctx.from_numpy(np.asfortranarray(A[rows])), dB,
                                   ctx.from_numpy(np.asfortranarray(W[rows])), sigma, trans=1).to_numpy()
        assert np.max(np.abs(blk - want)) <= 1e-13 * scale, g
    again = _run_grp(ctx, A, B, W, sigma, labels, G)
    assert np.array_equal(got, again)


def test_grouped_contract_wide_uncentred_column(ctx):
    """Column 0 of both operands wide (sd 28) and far from the origin (1000): the pass centres by the column means of A, as
    kernel_contract does. What is left is the rounding of |a|^2 + |b|^2 - 2 a.b on a wide column, which the same formula
    in float64 numpy shows too: the bound is 20 times that error, and never below the 1e-13 of the centred cases (the
    bound of the wide-column test of the leave-out moments)."""
    A, B, W, sigma, labels, G, ref, scale = _grp_inputs(3, True)
    got = _run_grp(ctx, A, B, W, sigma, labels, G)
    err = _err(got, ref, scale)
    err64 = _err(_restatement_f64(A, B, W, sigma, labels, G), ref, scale)
    bound = max(20.0 * err64, 1e-13)
    print(f"kernel_contract_grouped wide: error {err:.3e}, float64 numpy {err64:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_grouped_contract_refuses_bad_labels(ctx):
    from bigkrls_amd import _lib
    A, B, W, sigma, labels, G, _, _ = _grp_inputs(1, False)
    dA, dB, dW = ctx.from_numpy(A), ctx.from_numpy(B), ctx.from_numpy(W)
    out = ctx.empty(B.shape[0], G * W.shape[1])

    def call(lab, groups):
        lab = np.ascontiguousarray(lab, dtype=np.int64)
        _lib.call("bigkrls_dev_kernel_contract_grouped", ctx.handle, dA.ptr, dA.nrow, dA.ld, dB.ptr, dB.nrow, dB.ld,
                  A.shape[1], sigma, dW.ptr, W.shape[1], dW.ld, lab.ctypes.data, groups, out.ptr, out.ld)
    bad = labels.copy()
    bad[7] = G                                   # a label equal to G
    with pytest.raises(_lib.BigKRLSError) as ei:
        call(bad, G)
    assert ei.value.code == _lib.EINVAL and "row 8" in str(ei.value), str(ei.value)
    bad[7] = -1
    with pytest.raises(_lib.BigKRLSError) as ei:
        call(bad, G)
    assert ei.value.code == _lib.EINVAL and "row 8" in str(ei.value), str(ei.value)
    with pytest.raises(_lib.BigKRLSError) as ei:
        call(np.zeros_like(labels), 0)           # G = 0
    assert ei.value.code == _lib.EINVAL and "row 1 is outside [0, G)" in str(ei.value), str(ei.value)


def test_grouped_contract_profile_name_and_work(ctx):
    A, B, W, sigma, labels, G, _, _ = _grp_inputs(3, False)
    u, p = A.shape
    v, q = B.shape[0], W.shape[1]
    ctx.set_profile(True)
    try:
        _run_grp(ctx, A, B, W, sigma, labels, G)
        ms, work, launches = ctx.get_profile("kernel_contract_grouped")
    finally:
        ctx.set_profile(False)
    assert launches == 1 and work == 2 * u * v * (p + q)


# ---- fits shared by the tests below ------------------------------------------------------------------------------------
def _small_data():
    from oracle import krls_oracle as orc
    return orc.synth(300, 4, 21, binary_last=True)


LABELS = np.arange(300) % 3


@pytest.fixture(scope="module")
def fit_both():
    import bigkrls_amd as bk
    X, y = _small_data()
    return bk.bigKRLS(y, X, vcov_form="both")


@pytest.fixture(scope="module")
def res_dense(fit_both):
    import bigkrls_amd as bk
    return bk.group_effects(fit_both, LABELS, vcov="dense")


def _host(M):
    return M.to_numpy() if hasattr(M, "to_numpy") else np.asarray(M)


def test_against_the_oracle(fit_both, res_dense):
    out, res = fit_both, res_dense
    X = np.asarray(out["X"])
    G, nj = 3, 4
    assert res["groups"] == [0, 1, 2] and np.array_equal(res["n"], [100, 100, 100]) and res["reference"] == 0
    assert res["ame"].shape == (G, nj) and res["vcov.ame"].shape == (G * nj, G * nj)
    assert res["which.derivatives"] == [1, 2, 3, 4] and list(res["binaryindicator"]) == [False, False, False, True]
    ame, cov, D = ge_numpy(X, out["y"], _host(out["coeffs"]).ravel(), float(out["sigma"]), [1, 2, 3, 4], X, LABELS,
                           _host(out["vcov.est.c"]))
    e_ame = np.max(np.abs(res["ame"] - ame)) / np.max(np.abs(ame))
    e_cov = np.max(np.abs(res["vcov.ame"] - cov)) / np.max(np.abs(cov))
    e_d = np.max(np.abs(res["derivatives"] - D)) / np.max(np.abs(D))
    # the blocks between variables, the continuous x binary ones (the last variable) among them, on their own scale
    cross = np.ones((G * nj, G * nj), dtype=bool)
    for jj in range(nj):
        cross[jj * G:(jj + 1) * G, jj * G:(jj + 1) * G] = False
    e_cross = np.max(np.abs(res["vcov.ame"] - cov)[cross]) / np.max(np.abs(cov))
    print(f"group_effects vs oracle: ame {e_ame:.3e}, vcov.ame {e_cov:.3e} (between variables {e_cross:.3e}), "
          f"derivatives {e_d:.3e}")
    assert e_ame <= 1e-9 and e_cov <= 1e-8 and e_d <= 1e-9
    assert np.max(np.abs(cov[cross])) > 1e-6 * np.max(np.abs(cov))          # (they are not negligible entries)
    assert np.array_equal(res["vcov.ame"], res["vcov.ame"].T)
    assert np.linalg.eigvalsh(res["vcov.ame"]).min() >= -1e-10 * np.abs(res["vcov.ame"]).max()


def test_per_group_against_marginal_effects(fit_both, res_dense):
    import bigkrls_amd as bk
    out, res = fit_both, res_dense
    X = np.asarray(out["X"])
    G = 3
    scale = np.max(np.abs(res["ame"]))
    for g in range(G):
        me = bk.marginal_effects(out, X[LABELS == g], vcov="dense")
        assert np.max(np.abs(res["ame"][g] - me["avgderivatives"][0])) <= 1e-9 * scale
        var = me["var.avgderivatives"][0]
        diag = np.diag(res["vcov.ame"])[g::G]
        assert np.all(np.abs(diag - var) <= 1e-8 * var), g
        assert np.all(np.abs(res["se.ame"][g] ** 2 - var) <= 1e-8 * var), g
        assert np.max(np.abs(res["derivatives"][LABELS == g] - me["derivatives"])) <= 1e-9 * np.max(
            np.abs(me["derivatives"]))


def test_pooled_identities_pin_the_covariances_between_groups(fit_both, res_dense):
    """With w_g = n_g / u the pooled average effect is w' ame[:, jj] and its variance w' Sigma_jj w: the latter holds only
    if every covariance between two groups is right."""
    import bigkrls_amd as bk
    out, res = fit_both, res_dense
    X = np.asarray(out["X"])
    G = 3
    me = bk.marginal_effects(out, X, vcov="dense")
    w = res["n"] / res["n"].sum()
    scale = np.max(np.abs(res["ame"]))
    for jj in range(4):
        assert abs(w @ res["ame"][:, jj] - me["avgderivatives"][0, jj]) <= 1e-9 * scale
        Sj = res["vcov.ame"][jj * G:(jj + 1) * G, jj * G:(jj + 1) * G]
        var = me["var.avgderivatives"][0, jj]
        assert abs(w @ Sj @ w - var) <= 1e-8 * var, jj


def test_diff_and_wald_are_the_host_helpers_on_the_returned_values(fit_both, res_dense):
    import bigkrls_amd as bk
    from bigkrls_amd.api import _wald
    G = 3
    for ref_label, res in ((0, res_dense), (2, bk.group_effects(fit_both, LABELS, vcov="dense", reference=2))):
        r = ref_label
        assert res["reference"] == r
        ame, cov = res["ame"], res["vcov.ame"]
        assert np.array_equal(res["diff"], ame - ame[r:r + 1])
        assert np.array_equal(res["diff"][r], np.zeros(4)) and np.array_equal(res["se.diff"][r], np.zeros(4))
        assert np.array_equal(res["se.ame"], np.sqrt(np.maximum(np.diag(cov), 0.0)).reshape(4, G).T)
        for jj in range(4):
            Sj = cov[jj * G:(jj + 1) * G, jj * G:(jj + 1) * G]
            for g in range(G):
                if g != r:
                    want = np.sqrt(max(Sj[g, g] + Sj[r, r] - 2.0 * Sj[g, r], 0.0))
                    assert res["se.diff"][g, jj] == want
            stat, df, pv = _wald(ame[:, jj], Sj, r)
            assert res["wald"]["statistic"][jj] == stat and res["wald"]["df"][jj] == df and res["wald"]["p"][jj] == pv
            assert df == 2 and stat >= 0.0 and 0.0 <= pv <= 1.0


def test_factors_equal_dense(fit_both, res_dense):
    import bigkrls_amd as bk
    f = bk.group_effects(fit_both, LABELS, vcov="factors")
    assert np.array_equal(f["ame"], res_dense["ame"]) and np.array_equal(f["derivatives"], res_dense["derivatives"])
    cov_max = np.max(np.abs(res_dense["vcov.ame"]))
    assert np.max(np.abs(f["vcov.ame"] - res_dense["vcov.ame"])) <= 1e-8 * cov_max
    assert np.array_equal(f["vcov.ame"], f["vcov.ame"].T)


@pytest.mark.parametrize("form", ["dense", "factors"])
def test_interleaved_labels_equal_the_rows_physically_sorted(fit_both, form):
    """The stable sort of the labels puts the rows of a group in their original order: the same rows uploaded in that order,
    with sorted labels, take the path without the permutation and give the same bits."""
    import bigkrls_amd as bk
    X = np.asarray(fit_both["X"])
    order = np.argsort(LABELS, kind="stable")
    a = bk.group_effects(fit_both, LABELS, vcov=form)
    b = bk.group_effects(fit_both, LABELS[order], newdata=X[order], vcov=form)
    assert np.array_equal(a["ame"], b["ame"])
    assert np.array_equal(a["vcov.ame"], b["vcov.ame"])
    assert np.array_equal(a["derivatives"][order], b["derivatives"])
    again = bk.group_effects(fit_both, LABELS, vcov=form)
    assert np.array_equal(a["vcov.ame"], again["vcov.ame"]) and np.array_equal(a["ame"], again["ame"])


def test_fit_without_variances(res_dense):
    import bigkrls_amd as bk
    X, y = _small_data()
    out = bk.bigKRLS(y, X, vcov_est=False, derivative=False)
    res = bk.group_effects(out, LABELS)
    for key in ("se.ame", "vcov.ame", "se.diff", "wald"):
        assert res[key] is None, key
    scale = np.max(np.abs(res_dense["ame"]))
    assert np.max(np.abs(res["ame"] - res_dense["ame"])) <= 1e-9 * scale
    assert np.array_equal(res["diff"], res["ame"] - res["ame"][0:1])


def test_by_a_column(fit_both):
    import bigkrls_amd as bk
    X = np.asarray(fit_both["X"])
    res = bk.group_effects(fit_both, 4)                                    # the binary column
    lo, hi = X[:, 3].min(), X[:, 3].max()
    assert res["groups"] == [lo, hi] and np.array_equal(res["n"], [(X[:, 3] == lo).sum(), (X[:, 3] == hi).sum()])
    assert res["ame"].shape == (2, 4) and np.all(res["wald"]["df"] == 1)
    by_labels = bk.group_effects(fit_both, (X[:, 3] == hi).astype(int))
    assert np.array_equal(res["ame"], by_labels["ame"]) and np.array_equal(res["vcov.ame"], by_labels["vcov.ame"])
    res = bk.group_effects(fit_both, 1, bins=4)
    assert len(res["groups"]) == 4 and np.array_equal(res["n"], [75, 75, 75, 75])
    edges = np.quantile(X[:, 0], np.linspace(0, 1, 5))
    assert res["groups"] == [(edges[b], edges[b + 1]) for b in range(4)]
    assert res["ame"].shape == (4, 4) and res["vcov.ame"].shape == (16, 16)


def test_implicit_fit_against_marginal_effects_per_group():
    import bigkrls_amd as bk
    from oracle import krls_oracle as orc
    # N = 1024 is the smallest size the mode accepts, and it has no dense fallback: the data and Neig = 64 of the implicit
    # fits of tests/test_gpu_interaction_effects.py and tests/test_gpu_conditional_effects.py, whose block Lanczos
    # converges there (with Neig = 128 on these data it stops at the subspace limit, worst residual 1.6e-7: ENOCONV)
    X, y = orc.synth(1024, 4, 52, binary_last=True)
    out = bk.bigKRLS(y, X, Neig=64, kernel="implicit", vcov_form="factors", noisy=False)
    assert out["K"] is None and out.get("vcov.est.c") is None
    labels = np.arange(1024) % 3
    res = bk.group_effects(out, labels)
    G = 3
    scale = np.max(np.abs(res["ame"]))
    for g in range(G):
        me = bk.marginal_effects(out, X[labels == g])
        assert np.max(np.abs(res["ame"][g] - me["avgderivatives"][0])) <= 1e-9 * scale
        var = me["var.avgderivatives"][0]
        assert np.all(np.abs(np.diag(res["vcov.ame"])[g::G] - var) <= 1e-8 * var), g


def test_native_refusals(fit_both, ctx):
    from bigkrls_amd import _lib
    out = fit_both
    X = np.asfortranarray(out["X"])
    n, p = X.shape
    y = np.ascontiguousarray(out["y"], dtype=np.float64).ravel()
    c = np.ascontiguousarray(_host(out["coeffs"]), dtype=np.float64).ravel()
    ame = np.empty((3, p), order="F")

    def call(labels, G, cov=None):
        lab = np.ascontiguousarray(labels, dtype=np.int64)
        _lib.call("bigkrls_group_effects", ctx.handle, X.ctypes.data, n, p, y.ctypes.data, c.ctypes.data,
                  float(out["sigma"]), None, 0, X.ctypes.data, n, lab.ctypes.data, G, None, None, 0, 0, None, None,
                  ame.ctypes.data, None if cov is None else cov.ctypes.data)
    bad = LABELS.copy()
    bad[41] = 3
    for labels, G, named in ((bad, 3, "row 42"), (LABELS, 0, "row 1 is outside [0, G)")):
        with pytest.raises(_lib.BigKRLSError) as ei:
            call(labels, G)
        assert ei.value.code == _lib.EINVAL and named in str(ei.value), str(ei.value)
    with pytest.raises(_lib.BigKRLSError) as ei:                             # a covariance without a variance form
        call(LABELS, 3, cov=np.empty((12, 12)))
    assert ei.value.code == _lib.EINVAL and "h_cov" in str(ei.value)
    call(LABELS, 3)
    assert np.all(np.isfinite(ame))
