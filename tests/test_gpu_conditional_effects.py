"""conditional_effects() on the GPU: the fused leave-out moments pass (bigkrls_dev_kernel_loo_moments) against the direct
sum in extended precision and against the leave-one-column-out pass, and the whole path against brute force through
marginal_effects() -- one call on the rewritten rows per grid value --, from both forms of vcov.est.c and on an implicit
fit that never stored K."""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_ce_cpu", os.path.join(_HERE, "test_conditional_effects_cpu.py"))
_ce_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ce_cpu)
ce_numpy = _ce_cpu.ce_numpy
loo_moments_numpy = _ce_cpu.loo_moments_numpy


@pytest.fixture(scope="module")
def ctx():
    import bigkrls_amd as bk
    return bk.api.default_context()


# ---- Level 2: the fused pass -------------------------------------------------------------------------------------
CHUNK = 3      # KM_CW, csrc/gemm.hip: entries of one c per wave ...
CHUNK_KS8 = 2  # ... KM_CW_KS8: the same for 29 <= P <= 32
GROUP = 64     # KL_GROUP: entries per launch


def _entries_65(p):
    out = []
    for e in range(GROUP + 1):
        c = (e * 7) % p
        out.append((e % 3, c, (c + 1 + e) % p if (c + 1 + e) % p != c else (c + 2) % p))
    return out


MOM_CASES = [
    (1, 1, 2, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (0, 1, 0), (1, 1, 0), (2, 1, 0)]),
    (15, 17, 2, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (2, 1, 0), (1, 1, 0), (0, 1, 0)]),   # all three kinds; P = 2
    (17, 15, 3, [e for c in range(3) for e in                                          # all kinds on all c
                 [(0, c, 0)] + [(1, c, j) for j in range(3) if j != c] + [(2, c, j) for j in range(3) if j != c]]),
    (65, 64, 8, [(1, 0, j) for j in range(1, 8)]),                                     # seven kind-1 entries on c = 0
    (513, 129, 20, [(0, 0, 0)] + [(1, 0, j) for j in range(1, 20)] +                   # one kind 0 + 19 kind 1 on c = 0,
     [(1, 5, 3), (2, 5, 7), (1, 11, 0), (2, 11, 19)]),                                 # kinds 1 and 2 on two more c
    (130, 513, 33, [(0, 32, 0), (1, 32, 0), (2, 32, 16), (1, 0, 32), (2, 0, 1), (0, 7, 0), (1, 7, 8), (1, 7, 9),
                    (1, 7, 10), (1, 7, 11)]),                                          # KS = 0
    (129, 65, 67, [(0, 66, 0), (1, 66, 65), (2, 66, 0), (1, 3, 64), (2, 3, 4), (2, 3, 5), (2, 3, 6), (2, 3, 7)]),
    (4099, 17, 5, [(0, 0, 0), (1, 0, 1), (2, 0, 2), (1, 3, 4), (2, 4, 3)]),            # the loop is split
    (17, 4099, 5, [(1, 4, 0), (0, 0, 0), (2, 4, 1), (1, 0, 3), (0, 4, 0), (2, 0, 2), (1, 2, 1)]),   # out of order, c interleaved
    (70, 90, 9, [(1, 2, 0), (1, 2, 5), (0, 2, 0), (2, 2, 8)]),                         # the chunk width + 1 entries on one c
    (33, 40, 70, _entries_65(70)),                                                     # one entry more than a launch takes
    (40, 50, 30, [(1, 4, 0), (1, 4, 1), (1, 4, 2), (0, 4, 0), (2, 4, 29), (2, 29, 0), (1, 29, 28)]),   # KS = 8: the narrower chunk
]
assert len(MOM_CASES[9][3]) == CHUNK + 1 and len({e[1] for e in MOM_CASES[9][3]}) == 1
assert sum(1 for e in MOM_CASES[11][3] if e[1] == 4) > CHUNK_KS8 + 1
assert all(k == 0 or (j != c and 0 <= j < p) for _, _, p, ents in MOM_CASES for k, c, j in ents)


@functools.lru_cache(maxsize=None)
def _mom_inputs(case, wide):
    """(A, B, sigma, entries, longdouble reference, its scale max over the outputs of sum_i |wgt| e): the direct sum over
    the columns that stay in the distance, computed once per case."""
    u, v, p, entries = MOM_CASES[case]
    rng = np.random.default_rng(2000 * case + u + v + p)
    A = rng.standard_normal((u, p)) * 0.7
    B = rng.standard_normal((v, p)) * 0.7
    if wide:                                   # a wide, uncentred column: the cancellation in d2 - dc^2 is real
        A[:, 0] = A[:, 0] * 40.0 + 1000.0
        B[:, 0] = B[:, 0] * 40.0 + 1000.0
    sigma = float(p)
    ref, scale = loo_moments_numpy(A, B, sigma, entries, dtype=np.longdouble, with_scale=True)
    for a in (A, B, ref):
        a.setflags(write=False)
    return A, B, sigma, entries, ref, float(scale.max())


def _restatement_f64(A, B, sigma, entries):
    """The formula of the pass in float64 numpy: both operands moved by the column means of A, d2 = max(|a|^2 + |b|^2 -
    2 a.b, 0), base = max(d2 - dc^2, 0), kind 2: max(base - dj^2, 0); the weight from the moved copies."""
    sh = A.mean(axis=0)
    Ac, Bc = A - sh, B - sh
    d2 = np.maximum((Ac ** 2).sum(axis=1)[:, None] + (Bc ** 2).sum(axis=1)[None, :] - 2.0 * (Ac @ Bc.T), 0.0)
    out = np.empty((B.shape[0], len(entries)))
    for e, (kind, c, j) in enumerate(entries):
        dc = Ac[:, c][:, None] - Bc[:, c][None, :]
        x = np.maximum(d2 - dc * dc, 0.0)
        w = 1.0
        if kind == 1:
            w = Bc[:, j][None, :] - Ac[:, j][:, None]
        elif kind == 2:
            dj = Ac[:, j][:, None] - Bc[:, j][None, :]
            x = np.maximum(x - dj * dj, 0.0)
        out[:, e] = (w * np.exp(-x / sigma)).sum(axis=0)
    return out


def _run_mom(ctx, A, B, sigma, entries):
    from bigkrls_amd import ops
    return ops.bKernelLooMoments(ctx.from_numpy(A), ctx.from_numpy(B), sigma, entries).to_numpy()


def _err(got, ref, scale):
    return float(np.max(np.abs(got.astype(np.longdouble) - ref)) / scale)


@pytest.mark.parametrize("case", range(len(MOM_CASES)))
def test_loo_moments_against_extended_precision(ctx, case):
    A, B, sigma, entries, ref, scale = _mom_inputs(case, False)
    got = _run_mom(ctx, A, B, sigma, entries)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    err = _err(got, ref, scale)
    print(f"loo_moments {MOM_CASES[case][:3]} entries={len(entries)}: error {err:.3e} "
          f"(float64 numpy: {_err(_restatement_f64(A, B, sigma, entries), ref, scale):.3e})")
    assert err < 1e-13
    if A.shape[1] == 2:                          # nothing is left of the distance: every term is exp(0)
        for e, (kind, _, _) in enumerate(entries):
            if kind == 2:
                assert np.array_equal(got[:, e], np.full(B.shape[0], float(A.shape[0])))


@pytest.mark.parametrize("case", range(len(MOM_CASES)))
def test_loo_moments_wide_uncentred_column(ctx, case):
    A, B, sigma, entries, ref, scale = _mom_inputs(case, True)
    got = _run_mom(ctx, A, B, sigma, entries)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    err = _err(got, ref, scale)
    err64 = _err(_restatement_f64(A, B, sigma, entries), ref, scale)
    bound = max(20.0 * err64, 1e-13)
    print(f"loo_moments wide {MOM_CASES[case][:3]} entries={len(entries)}: error {err:.3e}, float64 numpy {err64:.3e}, "
          f"bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("case", range(len(MOM_CASES)))
def test_loo_moments_equals_loo_colsums_and_is_reproducible(ctx, case):
    from bigkrls_amd import ops
    A, B, sigma, entries, _, _ = _mom_inputs(case, False)
    u, p = A.shape
    got = _run_mom(ctx, A, B, sigma, entries)
    again = _run_mom(ctx, A, B, sigma, entries)
    assert np.array_equal(got, again)
    dA, dB = ctx.from_numpy(A), ctx.from_numpy(B)
    for e, (kind, c, j) in enumerate(entries):
        if kind == 0:
            want = ops.bKernelLooColsums(dA, dB, sigma, [c]).to_numpy().ravel()
        elif kind == 2:
            keep = [k for k in range(p) if k != j]          # copies with column j deleted; c moves down past it
            want = ops.bKernelLooColsums(ctx.from_numpy(np.asfortranarray(A[:, keep])),
                                         ctx.from_numpy(np.asfortranarray(B[:, keep])), sigma,
                                         [c - (1 if c > j else 0)]).to_numpy().ravel()
        else:
            continue
        assert np.max(np.abs(got[:, e] - want)) <= 1e-13 * np.max(np.abs(want)), (e, kind, c, j)


def test_loo_moments_rejects_bad_entries(ctx):
    from bigkrls_amd import _lib
    A, B, sigma, _, _, _ = _mom_inputs(2, False)
    p = A.shape[1]
    dA, dB = ctx.from_numpy(A), ctx.from_numpy(B)
    out = ctx.empty(B.shape[0], 2)
    bad_lists = [
        ([(0, 0, 0), (3, 0, 1)], "entry 1"),          # unknown kind
        ([(-1, 0, 1)], "entry 0"),
        ([(0, p, 0)], "entry 0"),                     # c outside [0, p)
        ([(0, 0, 0), (0, -1, 0)], "entry 1"),
        ([(1, 0, p)], "entry 0"),                     # j outside [0, p)
        ([(2, 0, -1)], "entry 0"),
        ([(0, 1, 0), (1, 1, 1)], "entry 1"),          # j = c, kinds 1 and 2
        ([(2, 2, 2)], "entry 0"),
        ([], "n_entries"),
    ]
    for entries, named in bad_lists:
        h = np.ascontiguousarray(entries, dtype=np.int64).reshape(-1, 3)
        keep = h if h.size else np.zeros((1, 3), dtype=np.int64)
        with pytest.raises(_lib.BigKRLSError) as ei:
            _lib.call("bigkrls_dev_kernel_loo_moments", ctx.handle, dA.ptr, dA.nrow, dA.ld, dB.ptr, dB.nrow, dB.ld, p,
                      sigma, keep.ctypes.data, int(h.shape[0]), out.ptr, out.ld)
        assert ei.value.code == _lib.EINVAL and named in str(ei.value), (entries, str(ei.value))
    # kind 0 ignores j
    got = _run_mom(ctx, A, B, sigma, [(0, 1, 99), (0, 1, 1)])
    assert np.array_equal(got[:, 0], got[:, 1])


def test_loo_moments_profile_name_and_work(ctx):
    A, B, sigma, _, _, _ = _mom_inputs(3, False)
    entries = [(1, 0, j) for j in range(1, CHUNK + 1)]       # one chunk of kind-1 entries: one exponential per row pair
    ctx.set_profile(True)
    try:
        _run_mom(ctx, A, B, sigma, entries)
        ms, work, launches = ctx.get_profile("kernel_loo_moments")
    finally:
        ctx.set_profile(False)
    assert launches == 1 and work == A.shape[0] * B.shape[0] * 1


# ---- fits shared by the tests below ---------------------------------------------------------------------------------
def _small_data():
    from oracle import krls_oracle as orc
    return orc.synth(300, 4, 21, binary_last=True)


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


E2E_PAIRS = [(1, 2), (2, 1), (1, 4), (4, 1), (3, 3), (4, 3)]


def _run_pairs(out, pairs=E2E_PAIRS, **kw):
    """conditional_effects() takes effect x along; the pairs of the tests one call each, merged into one result."""
    import bigkrls_amd as bk
    res = None
    for j, k in pairs:
        r = bk.conditional_effects(out, j, k, **kw)
        assert r["pairs"] == [(j, k)]
        if res is None:
            res = {key: (list(val) if isinstance(val, list) else val) for key, val in r.items()}
            continue
        for key in ("pairs", "xlabs", "grid", "ce", "se.ce", "vcov.ce"):
            if r[key] is not None:
                res[key] += r[key]
        for key in ("binary.effect", "binary.moderator"):
            res[key] = np.concatenate([res[key], r[key]])
        for key in ("contrast", "se.contrast"):
            if r[key] is not None:
                res[key] = np.hstack([res[key], r[key]])
    return res


def _brute_force(out, res, R, vcov=None):
    """Every grid value of every curve of `res` against one marginal_effects() on the rows R with the moderator's column
    rewritten: ce within 1e-9 of max |ce| over all curves, se.ce^2 and the diagonal of vcov.ce within 1e-8 relative."""
    import bigkrls_amd as bk
    ce_scale = max(np.max(np.abs(np.concatenate(res["ce"]))), 1e-300)
    for idx, (j, k) in enumerate(res["pairs"]):
        for g, v in enumerate(res["grid"][idx]):
            Zmod = R.copy()
            Zmod[:, k - 1] = v
            me = bk.marginal_effects(out, Zmod, which_derivatives=[j], vcov=vcov)
            assert abs(res["ce"][idx][g] - me["avgderivatives"][0, 0]) <= 1e-9 * ce_scale, (j, k, g)
            var = me["var.avgderivatives"][0, 0]
            assert abs(res["se.ce"][idx][g] ** 2 - var) <= 1e-8 * var, (j, k, g)
            assert abs(res["vcov.ce"][idx][g, g] - var) <= 1e-8 * var, (j, k, g)


# ---- brute force through the public API ------------------------------------------------------------------------------
def test_against_marginal_effects_on_rewritten_rows(fit_small):
    import bigkrls_amd as bk
    out = fit_small
    X = out["X"]
    res = _run_pairs(out, grid=5)
    assert res["pairs"] == E2E_PAIRS
    assert list(res["binary.effect"]) == [False, False, False, True, False, True]
    assert list(res["binary.moderator"]) == [False, False, True, False, False, False]
    assert [g.size for g in res["grid"]] == [5, 5, 2, 5, 5, 5]
    assert np.array_equal(res["grid"][2], [X[:, 3].min(), X[:, 3].max()])
    assert np.array_equal(res["grid"][0], np.linspace(X[:, 1].min(), X[:, 1].max(), 5))
    assert res["newdata"] is None
    _brute_force(out, res, X)
    # all combinations in one call are the single calls, bit for bit (one fused pass for all pairs)
    both = bk.conditional_effects(out, [1, 4], [2, 3], grid=5)
    assert both["pairs"] == [(1, 2), (1, 3), (4, 2), (4, 3)]
    labs = list(out.get("xlabs") or [f"x{i + 1}" for i in range(4)])
    assert both["xlabs"][3] == (labs[3], labs[2])
    single = _run_pairs(out, pairs=both["pairs"], grid=5)
    for key in ("ce", "se.ce", "vcov.ce"):
        for a, b in zip(both[key], single[key]):
            assert np.array_equal(a, b), key
    assert np.array_equal(both["contrast"], single["contrast"])


def test_covariances_and_contrast_against_numpy(fit_small):
    out = fit_small
    res = _run_pairs(out, grid=5)
    ces, ses, covs, con, secon = ce_numpy(out["X"], out["y"], out["coeffs"], out["sigma"], E2E_PAIRS, res["grid"],
                                          vcov_c=_host(out["vcov.est.c"]))
    ce_scale = max(np.max(np.abs(c)) for c in ces)
    for idx in range(len(E2E_PAIRS)):
        cov_max = np.max(np.abs(covs[idx]))
        assert np.max(np.abs(res["ce"][idx] - ces[idx])) <= 1e-9 * ce_scale, E2E_PAIRS[idx]
        assert np.max(np.abs(res["vcov.ce"][idx] - covs[idx])) <= 1e-8 * cov_max, E2E_PAIRS[idx]
        assert abs(res["contrast"][0, idx] - con[idx]) <= 1e-9 * ce_scale
        assert abs(res["contrast"][0, idx] - (res["ce"][idx][-1] - res["ce"][idx][0])) == 0.0
        assert abs(res["se.contrast"][0, idx] ** 2 - secon[idx] ** 2) <= 1e-8 * cov_max, E2E_PAIRS[idx]
    assert res["contrast"].shape == (1, len(E2E_PAIRS)) == res["se.contrast"].shape


def test_reference_rows_and_explicit_grids(fit_small):
    out = fit_small
    X = out["X"]
    R = X[::7] + np.array([[0.2, -0.1, 0.3, 0.0]])
    grids = {(1, 2): np.array([0.3, -0.4, 1.0]), (4, 3): np.array([0.5]), (1, 4): np.array([X[:, 3].max()])}
    import bigkrls_amd as bk
    for (j, k), g in grids.items():
        res = bk.conditional_effects(out, j, k, grid=[g], newdata=R)
        assert np.array_equal(res["newdata"], R)
        # a binary moderator always gets its two training values
        assert np.array_equal(res["grid"][0], g if k != 4 else [X[:, 3].min(), X[:, 3].max()])
        _brute_force(out, res, R)


def test_single_reference_row_is_marginal_effects_se(fit_small):
    import bigkrls_amd as bk
    out = fit_small
    z = out["X"][[7]] + np.array([[0.3, -0.2, 0.1, 0.0]])
    res = _run_pairs(out, grid=3, newdata=z)
    ce_scale = np.max(np.abs(np.concatenate(res["ce"])))
    for idx, (j, k) in enumerate(res["pairs"]):
        for g, v in enumerate(res["grid"][idx]):
            zm = z.copy()
            zm[0, k - 1] = v
            me = bk.marginal_effects(out, zm, which_derivatives=[j], se=True)
            assert abs(res["ce"][idx][g] - me["derivatives"][0, 0]) <= 1e-9 * ce_scale
            se2 = me["se.derivatives"][0, 0] ** 2
            assert abs(res["se.ce"][idx][g] ** 2 - se2) <= 1e-8 * se2


def test_without_variance(fit_small):
    a = _run_pairs(fit_small, grid=5)
    b = _run_pairs(fit_small, grid=5, se=False)
    assert b["se.ce"] is None and b["vcov.ce"] is None and b["se.contrast"] is None
    for x, y in zip(a["ce"], b["ce"]):
        assert np.array_equal(x, y)
    assert np.array_equal(a["contrast"], b["contrast"])
    again = _run_pairs(fit_small, grid=5)
    for k in ("ce", "se.ce", "vcov.ce"):
        for x, y in zip(a[k], again[k]):
            assert np.array_equal(x, y), k


# ---- factors equal dense ---------------------------------------------------------------------------------------------
def test_factors_equal_dense(fit_small_both):
    out = fit_small_both
    d = _run_pairs(out, grid=5, vcov="dense")
    f = _run_pairs(out, grid=5, vcov="factors")
    se_max = max(np.max(s) for s in d["se.ce"])
    cov_max = max(np.max(np.abs(c)) for c in d["vcov.ce"])
    for idx in range(len(E2E_PAIRS)):
        assert np.array_equal(d["ce"][idx], f["ce"][idx])
        assert np.max(np.abs(d["se.ce"][idx] - f["se.ce"][idx])) <= 1e-9 * se_max
        assert np.max(np.abs(d["vcov.ce"][idx] - f["vcov.ce"][idx])) <= 1e-9 * cov_max
    assert np.max(np.abs(d["se.contrast"] - f["se.contrast"])) <= 1e-9 * se_max
    _brute_force(out, f, out["X"], vcov="factors")


# ---- implicit fit: no stored K is needed -----------------------------------------------------------------------------
def test_implicit_fit_against_marginal_effects():
    import bigkrls_amd as bk
    from oracle import krls_oracle as orc
    # N = 1024 is the smallest size the mode accepts, and it has no dense fallback: the data of the implicit fit of
    # tests/test_gpu_interaction_effects.py, whose block Lanczos converges there (P = 4, the last column binary)
    X, y = orc.synth(1024, 4, 52, binary_last=True)
    out = bk.bigKRLS(y, X, Neig=64, kernel="implicit", vcov_form="factors", noisy=False)
    assert out["K"] is None and out.get("vcov.est.c") is None
    R = X[np.random.default_rng(5).choice(1024, 128, replace=False)]
    res = bk.conditional_effects(out, [2, 4, 3], 3, grid=3, newdata=R)
    assert res["pairs"] == [(2, 3), (4, 3), (3, 3)]
    _brute_force(out, res, R)


# ---- the cap on a pair's grid, and what only the library can refuse ------------------------------------------------------
def test_grid_longer_than_the_cap_raises(fit_small):
    import bigkrls_amd as bk
    n = fit_small["X"].shape[0]
    cap = (1 << 30) // (8 * n)
    x = fit_small["X"][:, 1]
    grid = [np.linspace(x.min(), x.max(), cap + 1)]
    with pytest.raises(ValueError, match=rf"grid of pair \(1, 2\) has {cap + 1} values; at most {cap} "):
        bk.conditional_effects(fit_small, 1, 2, grid=grid)


def test_native_refusals_name_the_pair(fit_small, ctx):
    from bigkrls_amd import _lib
    out = fit_small
    X = np.asfortranarray(out["X"])
    n, p = X.shape
    y = np.ascontiguousarray(out["y"], dtype=np.float64).ravel()
    c = np.ascontiguousarray(out["coeffs"], dtype=np.float64).ravel()
    lo, hi = X[:, 3].min(), X[:, 3].max()

    def call(pairs, grids):
        pa = np.ascontiguousarray(pairs, dtype=np.int64)
        off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(g) for g in grids])]), dtype=np.int64)
        flat = np.ascontiguousarray(np.concatenate(grids), dtype=np.float64)
        ce = np.empty(flat.size)
        _lib.call("bigkrls_conditional_effects", ctx.handle, X.ctypes.data, n, p, y.ctypes.data, c.ctypes.data,
                  float(out["sigma"]), pa.ctypes.data, len(pairs), None, n, flat.ctypes.data, off.ctypes.data, None, None,
                  0, 0, None, ce.ctypes.data, None, None)
        return ce
    for pairs, grids, named in [([(4, 4)], [[lo, hi]], "pair (4, 4) is not defined"),
                                ([(1, 2), (1, 2)], [[0.0], [0.1]], "pair (1, 2) is given more than once"),
                                ([(1, 4)], [[lo, 0.5 * (lo + hi)]], "pair (1, 4): column 4 is binary"),
                                ([(1, 5)], [[0.0]], "pair (1, 5) must index columns of X"),
                                ([(0, 1)], [[0.0]], "pair (0, 1) must index columns of X")]:
        with pytest.raises(_lib.BigKRLSError) as ei:
            call(pairs, grids)
        assert ei.value.code == _lib.EINVAL and named in str(ei.value), str(ei.value)
    assert np.all(np.isfinite(call([(1, 4), (4, 1)], [[hi, lo], [0.0, 0.3]])))
