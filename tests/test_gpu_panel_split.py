"""The split panel factorisation of stage 1 (csrc/eigen_2stage.inc): head pq_chol<true> (the two CholeskyQR passes, W = V U
left for the big product A22 W) -> the Householder kernel's slot -> tail pq_tail (V, R, tau, T, Tfold = U^-1 T).

Directly through bigkrls_dev_panel_factor, references in numpy on the downloaded factors, and through the dense
eigensolver against numpy.linalg.eigvalsh, itself and the one-kernel form (BIGKRLS_PQ=fused).

Bars of the direct tests: a float64 restatement of CholeskyQR2 + reconstruction on the CPU gives 1.8e-15 (orthogonality),
9e-15 max|P| (factorisation) and 3e-16 (W Tfold against V T) on these panels; the bars leave a factor >= 10."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
B = 64
SHAPES = [128, 129, 256, 257, 1000, 4097]   # 2 b (the smallest pq_chol takes); one workgroup; a partial last one; 2 ... 17
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def F(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def normal_panel(m):
    return np.random.default_rng(1000 + m).standard_normal((m, B))


def graded_panel(m):
    """orthonormal columns times diag(1 ... 1e-4): condition number 1e4"""
    q, _ = np.linalg.qr(np.random.default_rng(2000 + m).standard_normal((m, B)))
    return q * np.logspace(0, -4, B)


def gauss_kernel(n, p, seed):
    from bigkrls_amd.synth import synth
    X, _ = synth(n, p, seed)
    Xs = (X - X.mean(0)) / X.std(0, ddof=1)
    sq = (Xs * Xs).sum(1)
    return np.exp(-np.maximum(sq[:, None] + sq[None, :] - 2.0 * Xs @ Xs.T, 0.0) / p)


def kernel_panel():
    """the first panel of stage 1 on a Gaussian kernel matrix (N = 1000, P = 20): rows 64 ..., columns 0 .. 63"""
    return gauss_kernel(1000, 20, 4)[B:, :B].copy()


def factor(ctx, P0):
    from bigkrls_amd import _lib
    m = P0.shape[0]
    P = ctx.from_numpy(F(P0))
    Vw, V, T, Tf, tau = ctx.empty(m, B), ctx.empty(m, B), ctx.empty(B, B), ctx.empty(B, B), ctx.empty(B, 1)
    fb = C.c_int32(-1)
    _lib.call("bigkrls_dev_panel_factor", ctx.handle, P.ptr, m, m, Vw.ptr, V.ptr, T.ptr, Tf.ptr, tau.ptr, C.byref(fb))
    return dict(P=P.to_numpy(), Vw=Vw.to_numpy(), V=V.to_numpy(), T=T.to_numpy(), Tfold=Tf.to_numpy(),
                tau=tau.to_numpy().ravel(), fallback=fb.value)


def reflector_errors(P0, out):
    """max |H'H - I| and max |H'P_in - [R; 0]| for H = I - V T V' (H'H - I = V (T'(V'V)T - T - T') V')"""
    V, T = out["V"], out["T"]
    m = V.shape[0]
    orth = np.abs(V @ (T.T @ (V.T @ V) @ T - T - T.T) @ V.T).max()
    if m <= 1000:        # ... and the matrix itself where it is small
        H = np.eye(m) - V @ T @ V.T
        orth = max(orth, np.abs(H.T @ H - np.eye(m)).max())
    R = np.zeros((m, B))
    R[:B] = np.triu(out["P"][:B])
    fact = np.abs(P0 - V @ (T.T @ (V.T @ P0)) - R).max()
    return float(orth), float(fact)


def check_panel(P0, out):
    m = P0.shape[0]
    V, T = out["V"], out["T"]
    assert out["fallback"] == 0
    orth, fact = reflector_errors(P0, out)
    VT = V @ T
    fold = float(np.linalg.norm(out["Vw"] @ out["Tfold"] - VT) / np.linalg.norm(VT))
    print(f"m={m}: |H'H - I| {orth:.2e}, |H'P - R| / max|P| {fact / np.abs(P0).max():.2e}, |W Tfold - V T| / |V T| {fold:.2e}")
    assert orth <= 1e-13
    assert fact <= 1e-13 * np.abs(P0).max()
    assert fold <= 1e-14
    assert np.array_equal(np.triu(V[:B], 1), np.zeros((B, B))) and np.array_equal(np.diag(V[:B]), np.ones(B))
    assert np.array_equal(np.tril(T, -1), np.zeros((B, B)))
    assert np.array_equal(out["tau"], np.diag(T))
    # R and V are left in the panel as stage 1 keeps them
    low = np.tril(np.ones((m, B), dtype=bool), -1)
    assert np.array_equal(out["P"][low], V[low])


@pytest.mark.parametrize("m", SHAPES)
def test_normal_panel(ctx, m):
    P0 = normal_panel(m)
    check_panel(P0, factor(ctx, P0))


@pytest.mark.parametrize("m", SHAPES)
def test_graded_panel_cond_1e4(ctx, m):
    P0 = graded_panel(m)
    check_panel(P0, factor(ctx, P0))


def test_first_panel_of_a_gaussian_kernel_matrix(ctx):
    P0 = kernel_panel()
    check_panel(P0, factor(ctx, P0))


def test_rank_deficient_panel_falls_back_with_w_space_equal_to_v_space(ctx):
    """A rank-3 panel has no safe Cholesky factor: the head leaves it to the Householder kernel, whose V is then the
    operand of the big product itself (Vw == V) and whose T is the folded factor (Tfold == T), bit for bit."""
    rng = np.random.default_rng(5)
    P0 = rng.standard_normal((1000, 3)) @ rng.standard_normal((3, B))
    out = factor(ctx, P0)
    assert out["fallback"] == 1
    assert np.array_equal(out["Vw"], out["V"]) and np.array_equal(out["Tfold"], out["T"])
    orth, fact = reflector_errors(P0, out)
    print(f"rank 3: |H'H - I| {orth:.2e}, |H'P - R| / max|P| {fact / np.abs(P0).max():.2e}")
    assert orth <= 1e-12 and fact <= 1e-12 * np.abs(P0).max()


@pytest.mark.parametrize("m", [257, 4097])
def test_two_calls_are_bitwise_equal(ctx, m):
    P0 = normal_panel(m)
    a, b = factor(ctx, P0), factor(ctx, P0)
    for key in ("P", "Vw", "V", "T", "Tfold", "tau"):
        assert np.array_equal(a[key], b[key]), key
    assert a["fallback"] == b["fallback"] == 0


# ---- through the decomposition ---------------------------------------------------------------------------------------
EIG_NS = [321, 1000, 2049]


@pytest.fixture(scope="module")
def kernels():
    out = {}
    for n in EIG_NS:
        K = gauss_kernel(n, 6, 30 + n)
        out[n] = (K, np.linalg.eigvalsh(K)[::-1])
    return out


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def eigen_quality(ops, K, Q, lam):
    """max |K Q - Q diag(lam)| / lam_1 and max |Q'Q - I| with the products on the device (as tests/test_gpu_configs.py)"""
    k = Q.ncol
    R = ops.gemm(False, False, K, Q).to_numpy() - Q.to_numpy() * lam[:k]
    G = ops.gemm(True, False, Q, Q).to_numpy()
    return float(np.abs(R).max() / lam[0]), float(np.abs(G - np.eye(k)).max())


@pytest.mark.parametrize("n", EIG_NS)
def test_decomposition_with_split_panels(ctx, kernels, monkeypatch, n):
    from bigkrls_amd import ops
    monkeypatch.delenv("BIGKRLS_PQ", raising=False)
    K, ref = kernels[n]
    Kd = ctx.from_numpy(F(K))
    e1 = ops.bEigen(Kd, None, 0.0)
    e2 = ops.bEigen(Kd, None, 0.0)
    err = rel(e1.values, ref)
    res, orth = eigen_quality(ops, Kd, e1.vectors, e1.values)
    print(f"n={n}: values {err:.2e}, residual {res:.2e}, orthogonality {orth:.2e}")
    assert err < 1e-13 and res < 1e-11 and orth < 1e-11
    assert np.array_equal(e1.values, e2.values) and np.array_equal(e1.vectors.to_numpy(), e2.vectors.to_numpy())


def test_one_kernel_form_agrees_with_split(ctx, kernels, tmp_path, monkeypatch):
    """BIGKRLS_PQ=fused (read once per decomposition; a process of its own, as for the other switches of the panel
    factorisation): same eigenvalues to 1e-13."""
    from bigkrls_amd import ops
    monkeypatch.delenv("BIGKRLS_PQ", raising=False)
    for n in EIG_NS:
        np.save(tmp_path / f"K{n}.npy", kernels[n][0])
    code = r"""
import sys, json
sys.path.insert(0, %r)
import numpy as np
import bigkrls_amd as bk
from bigkrls_amd import ops
ctx = bk.Context(0)
out = {}
for n in %r:
    K = np.load(sys.argv[1] + "/K%%d.npy" %% n)
    out[str(n)] = np.asarray(ops.bEigen(ctx.from_numpy(np.asfortranarray(K)), None, 0.0).values).ravel().tolist()
print(json.dumps(out))
""" % (ROOT, EIG_NS)
    env = dict(os.environ, BIGKRLS_PQ="fused")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    fused = json.loads(r.stdout.strip().splitlines()[-1])
    for n in EIG_NS:
        split = ops.bEigen(ctx.from_numpy(F(kernels[n][0])), None, 0.0).values
        d = rel(split, np.array(fused[str(n)]))
        print(f"n={n}: split against the one-kernel form {d:.2e}")
        assert d < 1e-13
