"""predict(..., matrices=False) on the GPU: the diagonal of the quadratic form (bigkrls_dev_quadform_diag) against
numpy, parity of the pointwise path with today's predict() and with the oracle, the row-block boundaries, far points,
bitwise reproducibility, and u = 200 000 new points with SEs on a C3-shaped fit in about 1 GiB of extra memory (the
u x u path would need 384 GB there)."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import krls_oracle as orc

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_pp_cpu", os.path.join(_HERE, "test_predict_pointwise_cpu.py"))
_pp_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_pp_cpu)
block_rows = _pp_cpu.block_rows

GIB = 1 << 30


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def assert_parity(pw, full, rows=None):
    """matrices=False (pw) against matrices=True (full), optionally on a subset of full's rows."""
    fy, fs = full["predicted"], full["se.pred"]
    if rows is not None:
        fy, fs = fy[rows], (None if fs is None else fs[rows])
    assert rel(pw["predicted"], fy) <= 1e-12
    if fs is not None:
        assert np.all(np.isfinite(pw["se.pred"]))
        assert np.max(np.abs(pw["se.pred"] - fs)) <= 1e-9 * np.max(fs)
    assert pw["newdataK"] is None and pw["vcov.est.pred"] is None


# ---- Level 2: diag(A V A') against numpy ------------------------------------------------------------------------
SIZES = (1, 15, 17, 129, 513, 4099)


def _qf_cases():
    out, i = [], 0
    for m in SIZES:
        for n in SIZES:
            out.append((m, n, ("general", "psd")[i % 2]))
            i += 1
    return out


def _v(rng, n, kind):
    if kind == "psd":
        G = rng.standard_normal((n, n))
        return G @ G.T / n
    return rng.standard_normal((n, n))               # not symmetric


@pytest.mark.parametrize("m,n,kind", _qf_cases())
def test_quadform_diag_matches_numpy(ctx, m, n, kind):
    from bigkrls_amd import ops
    rng = np.random.default_rng(m * 7919 + n * 31 + len(kind))
    A = rng.standard_normal((m, n))
    V = _v(rng, n, kind)
    got = ops.bQuadformDiag(ctx.from_numpy(A), ctx.from_numpy(V)).to_numpy().ravel()
    ref = np.einsum("ij,ij->i", A @ V, A)
    assert got.shape == (m,)
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))


@pytest.mark.parametrize("m,n", [(1, 1), (17, 129), (129, 17), (513, 4099), (4099, 513), (1000, 2000)])
@pytest.mark.parametrize("kind", ["general", "psd"])
def test_quadform_diag_submatrix(ctx, m, n, kind):
    """A and V as sub-blocks of larger arrays (lda > m, ldv > n) whose other entries are NaN: nothing outside the
    blocks may reach the result."""
    from bigkrls_amd import _lib
    rng = np.random.default_rng(m + 3 * n)
    A = rng.standard_normal((m, n))
    V = _v(rng, n, kind)
    Abig = np.full((m + 5, n + 3), np.nan)
    Abig[2:2 + m, 1:1 + n] = A
    Vbig = np.full((n + 7, n + 2), np.nan)
    Vbig[3:3 + n, 2:2 + n] = V
    dA, dV = ctx.from_numpy(Abig), ctx.from_numpy(Vbig)
    out = ctx.empty(m, 1)
    _lib.call("bigkrls_dev_quadform_diag", ctx.handle, m, n, dA.col_ptr(1, 2), dA.ld, dV.col_ptr(2, 3), dV.ld,
              out.ptr)
    ref = np.einsum("ij,ij->i", A @ V, A)
    got = out.to_numpy().ravel()
    assert np.all(np.isfinite(got))
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))


# ---- parity with today's predict on small fits ------------------------------------------------------------------
def _small_fit(n, p, seed, binary, sigma):
    import bigkrls_amd as bk
    X, y = orc.synth(n + 400, p, seed, binary_last=binary)
    out = bk.bigKRLS(y[:n], X[:n], sigma=sigma, derivative=False, instructions=False, noisy=False)
    return out, X[n:]


SMALL = [   # n, p, seed, binary last column, user sigma, new points
    (300, 1, 61, False, None, 257),
    (800, 4, 62, True, None, 400),
    (1500, 20, 63, True, 7.5, 1100),
    (3000, 50, 64, False, None, 1300),        # p > 32 and u, n >= 1024: the tiled kernel_block
    (2000, 50, 65, True, 60.0, 700),
]


@pytest.mark.parametrize("n,p,seed,binary,sigma,u", SMALL)
def test_parity_with_matrices_true_and_oracle(ctx, n, p, seed, binary, sigma, u):
    import bigkrls_amd as bk
    out, Xrest = _small_fit(n, p, seed, binary, sigma)
    rng = np.random.default_rng(seed)
    Z = np.vstack([Xrest, Xrest[rng.integers(0, Xrest.shape[0], u)] + 0.1 * rng.standard_normal((u, p))])[:u]
    if binary:
        Z[:, -1] = Xrest[rng.integers(0, Xrest.shape[0], u), -1]
    assert out["Neffective"] is not None
    for correct_SE in (True, False):
        full = bk.predict(out, Z, se_pred=True, correct_SE=correct_SE, ctx=ctx)
        pw = bk.predict(out, Z, se_pred=True, correct_SE=correct_SE, ctx=ctx, matrices=False)
        assert_parity(pw, full)
        # and against the oracle's predict of the same model (first 200 rows)
        model = {"X": out["X"], "y": out["y"], "coeffs": out["coeffs"], "sigma": out["sigma"],
                 "Neffective": out["Neffective"], "vcov.est.c": out["vcov.est.c"].to_numpy()
                 if hasattr(out["vcov.est.c"], "to_numpy") else out["vcov.est.c"]}
        pr = orc.predict(model, Z[:200], se_pred=True, correct_se=correct_SE)
        assert rel(pw["predicted"][:200], pr["predicted"]) < 1e-6
        assert rel(pw["se.pred"][:200], pr["se.pred"]) < 1e-6
    # without SEs
    pw = bk.predict(out, Z, ctx=ctx, matrices=False)
    assert pw["se.pred"] is None
    assert rel(pw["predicted"], full["predicted"]) <= 1e-12


# ---- the C3-shaped fit of the block and memory tests --------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_c3():
    import bigkrls_amd as bk
    from bigkrls_amd.synth import synth
    X, y = synth(20000, 20, 103)
    return bk.bigKRLS(y, X, eigtrunc=0.001, derivative=False, instructions=False, noisy=False)


def test_block_boundaries(fit_c3, ctx):
    import bigkrls_amd as bk
    n = fit_c3["X"].shape[0]
    b = block_rows(n)
    assert b == 6656
    rng = np.random.default_rng(6656)
    Z = rng.standard_normal((3 * b + 5, 20))
    full = bk.predict(fit_c3, Z, se_pred=True, ctx=ctx)
    ctx.release_workspace()
    for u in (1, 127, 128, 129, b - 1, b, b + 1, 3 * b + 5):
        pw = bk.predict(fit_c3, Z[:u], se_pred=True, ctx=ctx, matrices=False)
        assert pw["predicted"].shape == (u,)
        assert_parity(pw, full, rows=slice(0, u))


def test_far_points(fit_c3, ctx):
    """Far from every training point the test kernel underflows to 0: se exactly 0 and the prediction mean(y)."""
    import bigkrls_amd as bk
    Z = fit_c3["X"][:300] + 1.0e3
    full = bk.predict(fit_c3, Z, se_pred=True, ctx=ctx)
    pw = bk.predict(fit_c3, Z, se_pred=True, ctx=ctx, matrices=False)
    assert np.all(pw["se.pred"] == 0.0) and np.array_equal(pw["se.pred"], full["se.pred"])
    assert np.array_equal(pw["predicted"], full["predicted"])
    y = np.asarray(fit_c3["y"]).ravel()
    assert np.all(np.abs(pw["predicted"] - np.mean(y)) <= 1e-15 * max(abs(np.mean(y)), 1.0))


def test_bitwise_repeatable(fit_c3, ctx):
    import bigkrls_amd as bk
    Z = np.random.default_rng(2).standard_normal((block_rows(20000) + 129, 20))
    a = bk.predict(fit_c3, Z, se_pred=True, ctx=ctx, matrices=False)
    b = bk.predict(fit_c3, Z, se_pred=True, ctx=ctx, matrices=False)
    assert np.array_equal(a["predicted"], b["predicted"]) and np.array_equal(a["se.pred"], b["se.pred"])


def test_u200000_with_se_in_bounded_memory(fit_c3, ctx):
    """The point of the feature: today's path would need 8 u (2n + u) = 384 GB here."""
    import torch
    import bigkrls_amd as bk
    n, u = 20000, 200000
    assert 8 * u * (2 * n + u) == 384 * 10 ** 9
    rng = np.random.default_rng(200000)
    Z = rng.standard_normal((u, 20))
    ctx.release_workspace()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    pw = bk.predict(fit_c3, Z, se_pred=True, ctx=ctx, matrices=False)
    torch.cuda.synchronize()
    assert ctx.workspace_bytes() < 1.25 * GIB
    assert torch.cuda.max_memory_allocated() - base < 1.25 * GIB
    assert pw["predicted"].shape == (u,) and pw["se.pred"].shape == (u,)
    assert np.all(np.isfinite(pw["predicted"])) and np.all(np.isfinite(pw["se.pred"]))
    rows = np.sort(rng.choice(u, 512, replace=False))
    ctx.release_workspace()
    full = bk.predict(fit_c3, Z[rows], se_pred=True, ctx=ctx)
    ctx.release_workspace()
    assert_parity({"predicted": pw["predicted"][rows], "se.pred": pw["se.pred"][rows], "newdataK": None,
                   "vcov.est.pred": None}, full)
