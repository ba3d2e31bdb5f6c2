"""vcov.est.c kept as Q diag(w) Q' on the GPU: the weighted row sums of squares (bigkrls_dev_rowsumsq_weighted) against
numpy, the factors a fit hands out against its own matrices, the capacity rule, predict() and marginal_effects() from
the factors against the dense forms, a multi-GPU object (world size 1, in process) used downstream, persistence, and
the device memory of a fit that keeps no N x N matrix but K."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import krls_oracle as orc

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_pp = _load("_pp_gpu_for_factors", "test_gpu_predict_pointwise.py")
_vf_cpu = _load("_vf_cpu", "test_vcov_factors_cpu.py")
assert_parity, SMALL, SIZES = _pp.assert_parity, _pp.SMALL, _pp.SIZES
block_rows_factored = _vf_cpu.block_rows_factored

GIB = 1 << 30
SMALL_OUTPUTS = ["K.eigenvalues", "lastkeeper", "Neffective", "coeffs", "sigma", "lambda", "binaryindicator",
                 "yfitted.std", "yfitted", "R2", "Looe", "Le", "sigmasq", "derivatives.std",
                 "var.avgderivatives.std", "R2AME", "avgderivatives", "var.avgderivatives", "derivatives"]


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def host(m):
    return m.to_numpy() if hasattr(m, "to_numpy") else np.asarray(m)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_small_outputs_bitwise(got, ref):
    for key in SMALL_OUTPUTS:
        if key in ref:
            assert key in got, key
            assert same_bits(got[key], ref[key]), key


# ---- 1. the operator against numpy ---------------------------------------------------------------------------------
@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("k", SIZES)
def test_rowsumsq_weighted_matches_numpy(ctx, m, k):
    from bigkrls_amd import ops
    rng = np.random.default_rng(m * 7919 + k * 31)
    T = rng.standard_normal((m, k))
    w = rng.random(k) if (m + k) % 2 else rng.standard_normal(k)           # variance weights, and signed ones
    dT = ctx.from_numpy(T)
    got = ops.bRowSumSqWeighted(dT, w).to_numpy().ravel()
    ref = (T ** 2) @ w
    assert got.shape == (m,)
    print(f"rowsumsq m={m} k={k}: max abs err / max |ref| = {np.max(np.abs(got - ref)) / np.max(np.abs(ref)):.3e}")
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))
    again = ops.bRowSumSqWeighted(dT, w).to_numpy().ravel()
    assert same_bits(got, again)


@pytest.mark.parametrize("m,k", [(1, 1), (17, 129), (129, 17), (513, 4099), (4099, 513), (1000, 250)])
def test_rowsumsq_weighted_submatrix(ctx, m, k):
    """T as a sub-block of a larger array (ldt > m) whose other entries are NaN: nothing outside may reach the result."""
    from bigkrls_amd import _lib
    rng = np.random.default_rng(m + 3 * k)
    T, w = rng.standard_normal((m, k)), rng.random(k)
    Tbig = np.full((m + 5, k + 3), np.nan)
    Tbig[2:2 + m, 1:1 + k] = T
    dT, dw, out = ctx.from_numpy(Tbig), ctx.from_numpy(w), ctx.empty(m, 1)
    _lib.call("bigkrls_dev_rowsumsq_weighted", ctx.handle, m, k, dT.col_ptr(1, 2), dT.ld, dw.ptr, out.ptr)
    got, ref = out.to_numpy().ravel(), (T ** 2) @ w
    assert np.all(np.isfinite(got))
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))


def test_rowsumsq_weighted_empty_shapes(ctx):
    from bigkrls_amd import _lib
    out = ctx.from_numpy(np.full(9, 7.0))
    _lib.call("bigkrls_dev_rowsumsq_weighted", ctx.handle, 9, 0, None, 9, None, out.ptr)       # k == 0: zeros
    assert np.array_equal(out.to_numpy().ravel(), np.zeros(9))
    out = ctx.from_numpy(np.full(9, 7.0))
    _lib.call("bigkrls_dev_rowsumsq_weighted", ctx.handle, 0, 4, None, 1, None, out.ptr)       # m == 0: nothing
    assert np.array_equal(out.to_numpy().ravel(), np.full(9, 7.0))


# ---- the fits ------------------------------------------------------------------------------------------------------
def _small_data():
    return orc.synth(700, 4, 23, binary_last=True)


@pytest.fixture(scope="module")
def small_fits(ctx):
    import bigkrls_amd as bk
    X, y = _small_data()
    return {form: bk.bigKRLS(y[:600], X[:600], eigtrunc=0.001, vcov_form=form, ctx=ctx, noisy=False)
            for form in ("dense", "both", "factors")}


def _c3_data():
    from bigkrls_amd.synth import synth
    return synth(20000, 20, 103)


@pytest.fixture(scope="module")
def c3_both(ctx):
    import bigkrls_amd as bk
    X, y = _c3_data()
    return bk.bigKRLS(y, X, eigtrunc=0.001, vcov_form="both", ctx=ctx, noisy=False)


@pytest.fixture(scope="module")
def c3_factors(ctx):
    import bigkrls_amd as bk
    X, y = _c3_data()
    return bk.bigKRLS(y, X, eigtrunc=0.001, vcov_form="factors", ctx=ctx, noisy=False)


# ---- 2. the fit hands out the factors ------------------------------------------------------------------------------
def _check_factor_shapes(out):
    from bigkrls_amd.device import is_device_matrix
    n, k = out["X"].shape[0], out["lastkeeper"]
    assert is_device_matrix(out["vcov.est.Q"]) and out["vcov.est.Q"].shape == (n, k)
    assert out["vcov.est.w"].shape == (k,) and np.all(out["vcov.est.w"] > 0.0)


def test_small_fit_both_equals_dense_and_rebuilds_the_matrices(small_fits):
    dense, both = small_fits["dense"], small_fits["both"]
    assert "vcov.est.Q" not in dense and "vcov.est.w" not in dense
    assert_small_outputs_bitwise(both, dense)
    for key in ("K", "vcov.est.c", "vcov.est.fitted"):
        assert same_bits(host(both[key]), host(dense[key])), key
    _check_factor_shapes(both)
    k = both["lastkeeper"]
    assert k < 600                                            # eigtrunc truncates: Q is n x k, not square
    Q, w, d = both["vcov.est.Q"].to_numpy(), both["vcov.est.w"], both["K.eigenvalues"][:k]
    V, Vf = host(dense["vcov.est.c"]), host(dense["vcov.est.fitted"])
    e1, e2 = np.max(np.abs((Q * w) @ Q.T - V)) / np.max(np.abs(V)), np.max(np.abs((Q * (w * d * d)) @ Q.T - Vf)) / np.max(np.abs(Vf))
    print(f"small fit: |Q diag(w) Q' - vcov.est.c| / max = {e1:.3e}, fitted: {e2:.3e}")
    assert e1 <= 1e-12 and e2 <= 1e-12


def test_small_fit_factors_only(small_fits):
    dense, fac = small_fits["dense"], small_fits["factors"]
    assert_small_outputs_bitwise(fac, dense)
    assert fac["vcov.est.c"] is None and fac["vcov.est.fitted"] is None
    assert same_bits(host(fac["K"]), host(dense["K"]))
    _check_factor_shapes(fac)
    assert same_bits(fac["vcov.est.Q"].to_numpy(), small_fits["both"]["vcov.est.Q"].to_numpy())
    assert same_bits(fac["vcov.est.w"], small_fits["both"]["vcov.est.w"])


def test_c3_fit_both_equals_dense(ctx, c3_both, c3_factors):
    import bigkrls_amd as bk
    X, y = _c3_data()
    dense = bk.bigKRLS(y, X, eigtrunc=0.001, ctx=ctx, noisy=False)
    assert_small_outputs_bitwise(c3_both, dense)
    assert_small_outputs_bitwise(c3_factors, dense)
    for key in ("K", "vcov.est.c", "vcov.est.fitted"):
        assert bool((c3_both[key].t == dense[key].t).all()), key
    assert c3_factors["vcov.est.c"] is None and c3_factors["vcov.est.fitted"] is None
    _check_factor_shapes(c3_both)
    _check_factor_shapes(c3_factors)
    # Q diag(w) Q' against a block of columns of the matrices (the whole product is formed on the host at small n above)
    k = c3_both["lastkeeper"]
    Q, w, d = c3_both["vcov.est.Q"].to_numpy(), c3_both["vcov.est.w"], c3_both["K.eigenvalues"][:k]
    for key, wk in (("vcov.est.c", w), ("vcov.est.fitted", w * d * d)):
        vmax = float(dense[key].t.abs().max())
        V = dense[key].cols(7000, 7300).to_numpy()
        assert np.max(np.abs((Q * wk) @ Q[7000:7300].T - V)) <= 1e-12 * vmax, key


# ---- 3. capacity ---------------------------------------------------------------------------------------------------
def test_capacity_error_names_both_counts(ctx, small_fits):
    import bigkrls_amd as bk
    X, y = _small_data()
    kept = small_fits["dense"]["lastkeeper"]
    assert kept > 1
    with pytest.raises(ValueError) as ei:
        bk.bigKRLS(y[:600], X[:600], eigtrunc=0.001, vcov_form="factors", max_factors=1, ctx=ctx, noisy=False)
    msg = str(ei.value)
    assert f"keeps {kept} eigenpairs" in msg and "hold 1 columns" in msg and "max_factors" in msg
    # exactly enough room is enough
    out = bk.bigKRLS(y[:600], X[:600], eigtrunc=0.001, vcov_form="factors", max_factors=kept, ctx=ctx, noisy=False)
    assert out["vcov.est.Q"].shape == (600, kept)


def test_default_capacity_holds_on_c3(c3_factors):
    assert c3_factors["lastkeeper"] <= 2048                   # the input meets the default's condition on its own
    assert c3_factors["vcov.est.Q"].ncol == c3_factors["lastkeeper"]


# ---- 4. predict ----------------------------------------------------------------------------------------------------
def assert_matrices_parity(fac, dense):
    assert rel(fac["predicted"], dense["predicted"]) <= 1e-12
    assert np.all(np.isfinite(fac["se.pred"])) and np.all(fac["se.pred"] >= 0.0)
    assert np.max(np.abs(fac["se.pred"] - dense["se.pred"])) <= 1e-9 * np.max(dense["se.pred"])
    assert same_bits(host(fac["newdataK"]), host(dense["newdataK"]))
    Vd, Vf = host(dense["vcov.est.pred"]), host(fac["vcov.est.pred"])
    assert Vf.shape == Vd.shape
    assert np.max(np.abs(Vf - Vd)) <= 1e-9 * np.max(np.abs(Vd))


@pytest.mark.parametrize("n,p,seed,binary,sigma,u", SMALL)
def test_predict_parity_small(ctx, n, p, seed, binary, sigma, u):
    import bigkrls_amd as bk
    X, y = orc.synth(n + 400, p, seed, binary_last=binary)
    out = bk.bigKRLS(y[:n], X[:n], sigma=sigma, eigtrunc=0.001, derivative=False, vcov_form="both", ctx=ctx, noisy=False)
    Xrest = X[n:]
    rng = np.random.default_rng(seed)
    Z = np.vstack([Xrest, Xrest[rng.integers(0, Xrest.shape[0], u)] + 0.1 * rng.standard_normal((u, p))])[:u]
    if binary:
        Z[:, -1] = Xrest[rng.integers(0, Xrest.shape[0], u), -1]
    for correct_SE in (True, False):
        dense = bk.predict(out, Z, se_pred=True, correct_SE=correct_SE, ctx=ctx, vcov="dense")
        fac = bk.predict(out, Z, se_pred=True, correct_SE=correct_SE, ctx=ctx, vcov="factors")
        assert_matrices_parity(fac, dense)
        pw_dense = bk.predict(out, Z, se_pred=True, correct_SE=correct_SE, ctx=ctx, matrices=False, vcov="dense")
        pw_fac = bk.predict(out, Z, se_pred=True, correct_SE=correct_SE, ctx=ctx, matrices=False, vcov="factors")
        assert_parity(pw_fac, pw_dense)
        assert_parity(pw_fac, dense)
    assert bk.predict(out, Z, ctx=ctx, matrices=False, vcov="factors")["se.pred"] is None


def test_predict_block_boundaries_c3(c3_both, ctx):
    import bigkrls_amd as bk
    n, k = 20000, c3_both["lastkeeper"]
    b = block_rows_factored(n, k)
    assert 128 <= b <= 6656 and b % 128 == 0
    Z = np.random.default_rng(6656).standard_normal((3 * b + 5, 20))
    dense = bk.predict(c3_both, Z, se_pred=True, ctx=ctx, matrices=False, vcov="dense")
    ctx.release_workspace()
    for u in (1, 127, 128, 129, b - 1, b, b + 1, 3 * b + 5):
        pw = bk.predict(c3_both, Z[:u], se_pred=True, ctx=ctx, matrices=False, vcov="factors")
        assert pw["predicted"].shape == (u,)
        assert_parity(pw, dense, rows=slice(0, u))
    again = bk.predict(c3_both, Z, se_pred=True, ctx=ctx, matrices=False, vcov="factors")
    assert same_bits(pw["se.pred"], again["se.pred"]) and same_bits(pw["predicted"], again["predicted"])
    ctx.release_workspace()


def test_predict_matrices_c3(c3_both, ctx):
    import bigkrls_amd as bk
    Z = np.random.default_rng(11).standard_normal((1500, 20))
    dense = bk.predict(c3_both, Z, se_pred=True, ctx=ctx, vcov="dense")
    fac = bk.predict(c3_both, Z, se_pred=True, ctx=ctx, vcov="factors")
    assert_matrices_parity(fac, dense)
    ctx.release_workspace()


def test_predict_far_points(c3_both, ctx):
    """Far from every training point the test kernel underflows: finite, non-negative SEs (exactly 0 here)."""
    import bigkrls_amd as bk
    Z = c3_both["X"][:300] + 1.0e3
    for matrices in (True, False):
        pw = bk.predict(c3_both, Z, se_pred=True, ctx=ctx, matrices=matrices, vcov="factors")
        assert np.all(np.isfinite(pw["se.pred"])) and np.all(pw["se.pred"] >= 0.0)
        assert np.all(pw["se.pred"] == 0.0)
    ctx.release_workspace()


def test_u200000_with_se_in_bounded_memory(c3_factors, c3_both, ctx):
    """include/bigkrls.h: below 1.25 GiB of extra device memory whatever u is."""
    import torch
    import bigkrls_amd as bk
    u = 200000
    rng = np.random.default_rng(200000)
    Z = rng.standard_normal((u, 20))
    ctx.release_workspace()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    pw = bk.predict(c3_factors, Z, se_pred=True, ctx=ctx, matrices=False)      # the only form the object has
    torch.cuda.synchronize()
    print(f"u=200000 from factors: workspace {ctx.workspace_bytes() / GIB:.3f} GiB, "
          f"torch extra {(torch.cuda.max_memory_allocated() - base) / GIB:.3f} GiB")
    assert ctx.workspace_bytes() < 1.25 * GIB
    assert torch.cuda.max_memory_allocated() - base < 1.25 * GIB
    assert pw["predicted"].shape == (u,) and pw["se.pred"].shape == (u,)
    assert np.all(np.isfinite(pw["predicted"])) and np.all(np.isfinite(pw["se.pred"])) and np.all(pw["se.pred"] >= 0)
    rows = np.sort(rng.choice(u, 512, replace=False))
    ctx.release_workspace()
    full = bk.predict(c3_both, Z[rows], se_pred=True, ctx=ctx, vcov="dense")
    ctx.release_workspace()
    assert_parity({"predicted": pw["predicted"][rows], "se.pred": pw["se.pred"][rows], "newdataK": None,
                   "vcov.est.pred": None}, full)


# ---- 5. marginal effects -------------------------------------------------------------------------------------------
def _assert_me_parity(fac, dense):
    assert same_bits(fac["derivatives"], dense["derivatives"])
    assert same_bits(fac["avgderivatives"], dense["avgderivatives"])
    assert fac["var.avgderivatives"].shape == dense["var.avgderivatives"].shape
    print("marginal effects, factors vs dense, rel err of var.avgderivatives:",
          rel(fac["var.avgderivatives"], dense["var.avgderivatives"]))
    assert rel(fac["var.avgderivatives"], dense["var.avgderivatives"]) < 1e-8


def test_marginal_effects_parity_small(small_fits, ctx):
    import bigkrls_amd as bk
    X, _ = _small_data()
    both = small_fits["both"]
    for Z, which in ((X[600:], None), (X[600:650], [4, 2]), (both["X"], None)):
        _assert_me_parity(bk.marginal_effects(both, Z, which_derivatives=which, ctx=ctx, vcov="factors"),
                          bk.marginal_effects(both, Z, which_derivatives=which, ctx=ctx, vcov="dense"))


def test_marginal_effects_parity_c3(c3_both, ctx):
    import bigkrls_amd as bk
    Z = np.random.default_rng(5).standard_normal((3000, 20))
    _assert_me_parity(bk.marginal_effects(c3_both, Z, ctx=ctx, vcov="factors"),
                      bk.marginal_effects(c3_both, Z, ctx=ctx, vcov="dense"))


@pytest.mark.parametrize("which", ["small", "c3"])
def test_marginal_effects_in_sample_on_a_factors_only_fit(small_fits, c3_factors, ctx, which):
    import bigkrls_amd as bk
    out = small_fits["factors"] if which == "small" else c3_factors
    me = bk.marginal_effects(out, out["X"], ctx=ctx)                      # the only form the object has
    assert me["var.avgderivatives"].shape == out["var.avgderivatives"].shape
    assert rel(me["var.avgderivatives"], out["var.avgderivatives"]) < 1e-8
    assert rel(me["avgderivatives"], out["avgderivatives"]) < 1e-9


# ---- 6. a multi-GPU object used downstream (world size 1, in process) ----------------------------------------------
def test_multi_gpu_object_with_factors(small_fits, ctx):
    import bigkrls_amd as bk
    from bigkrls_amd import dist
    X, y = _small_data()
    mg = dist.bigKRLS_dist(y[:600], X[:600], eigtrunc=0.001, vcov_form="factors", collectives="host", ctx=ctx)
    both = small_fits["both"]
    assert "rows" in mg and mg.get("vcov.est.c") is None and mg.get("vcov.est.c.cols") is None
    assert mg["vcov.est.Q"].shape == (600, mg["lastkeeper"]) and mg["lastkeeper"] == both["lastkeeper"]
    Z = X[600:]
    for correct_SE in (True, False):
        pw = bk.predict(mg, Z, se_pred=True, correct_SE=correct_SE, ctx=ctx, matrices=False)
        assert_parity(pw, bk.predict(both, Z, se_pred=True, correct_SE=correct_SE, ctx=ctx, vcov="dense"))
    me, ref = bk.marginal_effects(mg, Z, ctx=ctx), bk.marginal_effects(both, Z, ctx=ctx, vcov="dense")
    assert rel(me["derivatives"], ref["derivatives"]) < 1e-9 and rel(me["avgderivatives"], ref["avgderivatives"]) < 1e-9
    assert rel(me["var.avgderivatives"], ref["var.avgderivatives"]) < 1e-8
    # without factors the object is refused as before
    plain = dist.bigKRLS_dist(y[:600], X[:600], eigtrunc=0.001, collectives="host", ctx=ctx)
    assert "vcov.est.Q" not in plain
    with pytest.raises(ValueError, match="recompute bigKRLS object"):
        bk.predict(plain, Z, se_pred=True, ctx=ctx, matrices=False)
    with pytest.raises(NotImplementedError):
        bk.marginal_effects(plain, Z, ctx=ctx)


# ---- 7. persistence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [False, True])
def test_save_load_round_trip_of_a_factors_only_model(small_fits, ctx, tmp_path, binary):
    import bigkrls_amd as bk
    from bigkrls_amd.device import is_device_matrix
    X, _ = _small_data()
    fac = small_fits["factors"]
    folder = bk.save_bigKRLS(fac, str(tmp_path / "model"), noisy=False, binary=binary)
    back = bk.load_bigKRLS(folder, noisy=False, ctx=ctx)
    assert is_device_matrix(back["vcov.est.Q"]) and back.get("vcov.est.c") is None
    assert same_bits(back["vcov.est.Q"].to_numpy(), fac["vcov.est.Q"].to_numpy())
    assert same_bits(np.asarray(back["vcov.est.w"], dtype=np.float64), fac["vcov.est.w"])
    Z = X[600:]
    for matrices in (False, True):
        a = bk.predict(fac, Z, se_pred=True, ctx=ctx, matrices=matrices)
        b = bk.predict(back, Z, se_pred=True, ctx=ctx, matrices=matrices)
        assert np.max(np.abs(a["se.pred"] - b["se.pred"])) <= 1e-12 * np.max(a["se.pred"])
        assert rel(b["predicted"], a["predicted"]) <= 1e-12


# ---- 8. memory -----------------------------------------------------------------------------------------------------
def test_factors_fit_keeps_one_n_by_n_matrix_and_saves_two(ctx, monkeypatch):
    import torch
    import bigkrls_amd as bk
    X, y = _c3_data()
    n, cap = 20000, 2048
    shapes = []
    real_empty = ctx.empty

    def counting_empty(nrow, ncol=1):
        shapes.append((int(nrow), int(ncol)))
        return real_empty(nrow, ncol)
    monkeypatch.setattr(ctx, "empty", counting_empty)

    def peak(form):
        ctx.release_workspace()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        del shapes[:]
        out = bk.bigKRLS(y, X, eigtrunc=0.001, vcov_form=form, ctx=ctx, noisy=False)
        torch.cuda.synchronize()
        total = torch.cuda.max_memory_allocated() - base + ctx.workspace_bytes()
        square = [s for s in shapes if s == (n, n)]
        del out
        return total, square, list(shapes)
    dense_peak, dense_sq, _ = peak("dense")
    fac_peak, fac_sq, fac_shapes = peak("factors")
    ctx.release_workspace()
    torch.cuda.empty_cache()
    assert len(dense_sq) == 3 and len(fac_sq) == 1
    assert (n, cap) in fac_shapes
    saved = dense_peak - fac_peak
    print(f"peak device memory of the fit: dense {dense_peak / 1e9:.3f} GB, factors {fac_peak / 1e9:.3f} GB, "
          f"saved {saved / 1e9:.3f} GB, bound {(2 * 8 * n * n - 8 * n * cap) / 1e9:.3f} GB")
    assert saved >= 2 * 8 * n * n - 8 * n * cap
