"""Panels, references and checks of the direct tests of stage 1's panel factorisation (tests/test_gpu_panel_routes.py on
the device, tests/test_panel_gate_cpu.py in numpy alone). Everything here is float64 numpy; nothing touches the GPU.

A factorisation is the dict test_gpu_panel_routes.factor returns: P (the panel as the kernels left it), V, T, tau, Vw,
Tfold, fallback."""
import functools

import numpy as np

B = 64
PQC_RATIO = 1e-5            # csrc/eigen_2stage.inc: min / max diagonal of the first Cholesky factor
PQC_E2MAX = 2.0 ** -7       # ... and the largest entry of Q1'Q1 - I after the first pass
KAHAN_C = [0.20, 0.21, 0.22, 0.23, 0.24, 0.25, 0.26, 0.27, 0.28, 0.29, 0.30, 0.31, 0.32, 0.35, 0.40]
MIXED_E = [5, 6, 6.5, 7, 8, 10]


# ---- panels -------------------------------------------------------------------------------------------------------------
def normal_panel(m):
    """(the normal panels of tests/test_gpu_panel_split.py)"""
    return np.random.default_rng(1000 + m).standard_normal((m, B))


def graded_panel(m):
    """orthonormal columns times diag(1 ... 1e-4): condition number 1e4 (tests/test_gpu_panel_split.py)"""
    q, _ = np.linalg.qr(np.random.default_rng(2000 + m).standard_normal((m, B)))
    return q * np.logspace(0, -4, B)


def orthonormal(m, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((m, B)))
    return q


def kahan_r(c):
    """Kahan's matrix: diag(s^j) (I - c triu(1, 1)), s = sqrt(1 - c^2). Its diagonal falls to s^63 only (0.27 at c = 0.2,
    0.004 at c = 0.4) while its condition number is 1e6 ... 1e12: what a ratio of diagonal entries cannot see."""
    s = np.sqrt(1.0 - c * c)
    return (s ** np.arange(B))[:, None] * (np.eye(B) - c * np.triu(np.ones((B, B)), 1))


def kahan_panel(m, c):
    return orthonormal(m, 3000 + m) @ kahan_r(c)


def mixed_panel(m, e):
    """Q0 diag(logspace(0, -e, 64)) Q1: condition number 10^e with every column of full size"""
    q1, _ = np.linalg.qr(np.random.default_rng(4000).standard_normal((B, B)))
    return (orthonormal(m, 3000 + m) * np.logspace(0, -e, B)) @ q1


def cond(P0):
    s = np.linalg.svd(P0, compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else float("inf")


# ---- the gate of pq_chol, restated ----------------------------------------------------------------------------------------
def _chol_upper(G):
    """right-looking Cholesky G = R'R as pq_chol does it; (R, None) or (None, 'breakdown') at a pivot that is not in (0, 1e300)"""
    A = np.array(G, dtype=np.float64)
    n = A.shape[0]
    R = np.zeros((n, n))
    for j in range(n):
        a = A[j, j]
        if not (a > 0.0) or not (a < 1e300):
            return None, "breakdown"
        d = np.sqrt(a)
        R[j, j] = d
        R[j, j + 1:] = A[j, j + 1:] / d
        A[j + 1:, j + 1:] -= np.outer(R[j, j + 1:], R[j, j + 1:])
    return R, None


def gate_restated(P0):
    """What the two CholeskyQR passes of pq_chol decide for the panel P0, in float64 numpy: None (CholeskyQR2 does the panel)
    or the test that leaves it to the Householder kernel: 'breakdown' (a pivot that is not positive, either pass), 'ratio'
    (first factor: dmin < PQC_RATIO dmax), 'far' (second Gram matrix: max |G2 - I| >= PQC_E2MAX) or 'second' (max |G2 - I|
    >= 1e-8 and a diagonal of its factor outside [0.5, 2])."""
    R1, why = _chol_upper(P0.T @ P0)
    if why:
        return why
    d = np.diag(R1)
    if d.min() < PQC_RATIO * d.max():
        return "ratio"
    Q = np.linalg.solve(R1.T, P0.T).T
    G2 = Q.T @ Q
    e2 = np.abs(G2 - np.eye(B)).max()
    if e2 < 1e-8:
        return None
    if not e2 < PQC_E2MAX:
        return "far"
    R2, why = _chol_upper(G2)
    if why:
        return why
    d = np.diag(R2)
    return "second" if d.min() < 0.5 or d.max() > 2.0 else None


# ---- LAPACK's Householder QR in the same form -------------------------------------------------------------------------------
def lapack_factor(P0):
    """numpy.linalg.qr(mode='raw') (dgeqrf) with T by the forward dlarft recurrence, as a factorisation dict"""
    m = P0.shape[0]
    k = min(m, B)
    h, tau_k = np.linalg.qr(P0, mode="raw")
    A = np.array(h.T)                                   # m x 64: R on and above the diagonal, V below
    V = np.tril(A, -1)
    V[np.arange(k), np.arange(k)] = 1.0
    V[:, k:] = 0.0
    tau = np.zeros(B)
    tau[:k] = tau_k
    G = V.T @ V
    T = np.zeros((B, B))
    for i in range(B):
        T[:i, i] = -tau[i] * (T[:i, :i] @ G[:i, i])
        T[i, i] = tau[i]
    return dict(P=A, V=V, T=T, tau=tau, Vw=V, Tfold=T, fallback=0)


# ---- errors -----------------------------------------------------------------------------------------------------------------
def orth_error(V, T, block=1024):
    """max |H'H - I| for H = I - V T V': H'H - I = V E V' with E = T'(V'V)T - T - T'. E is symmetric, so row block i of
    V E V' is formed against rows >= its first only; no m x m array. Where m <= 1000 the matrix itself as well."""
    m = V.shape[0]
    E = T.T @ (V.T @ V) @ T - T - T.T
    VE = V @ (0.5 * (E + E.T))                          # (E is symmetric but for the rounding of its first term)
    worst = 0.0
    for r0 in range(0, m, block):
        worst = max(worst, float(np.abs(VE[r0:r0 + block] @ V[r0:].T).max()))
    if m <= 1000:
        H = np.eye(m) - V @ T @ V.T
        worst = max(worst, float(np.abs(H.T @ H - np.eye(m)).max()))
    return worst


def r_of(out):
    """[R; 0]: the panel's entries on and above the diagonal"""
    return np.triu(out["P"])


def fact_error(P0, out):
    """max |H'P_in - [R; 0]| / max |P_in| (0 for a zero panel that came back as zeros)"""
    V, T = out["V"], out["T"]
    d = float(np.abs(P0 - V @ (T.T @ (V.T @ P0)) - r_of(out)).max())
    scale = float(np.abs(P0).max())
    return d / scale if scale > 0 else d


def fold_error(out):
    """|Vw Tfold - V T| / |V T| (Frobenius); 0 where V T is zero and so is Vw Tfold"""
    VT = out["V"] @ out["T"]
    d = float(np.linalg.norm(out["Vw"] @ out["Tfold"] - VT))
    nrm = float(np.linalg.norm(VT))
    return d / nrm if nrm > 0 else d


def errors(P0, out):
    return orth_error(out["V"], out["T"]), fact_error(P0, out), fold_error(out)


@functools.lru_cache(maxsize=None)
def reference_errors(maker, *args):
    """(orthogonality, factorisation) of LAPACK's factorisation of maker(*args), computed once per panel"""
    P0 = maker(*args)
    ref = lapack_factor(P0)
    return orth_error(ref["V"], ref["T"]), fact_error(P0, ref)


# the project's bars (tests/test_gpu_panel_split.py); a case's bar is the larger of these and 10 x LAPACK's own error
BARS = {"cholqr2": (1e-13, 1e-13), "householder": (1e-12, 1e-12)}
FOLD_BAR = 1e-14


def bars(method, ref):
    o, f = BARS[method]
    return max(o, 10.0 * ref[0]), max(f, 10.0 * ref[1])


# ---- structure ----------------------------------------------------------------------------------------------------------------
def _scaled_column_matches(x, v):
    """is there ONE double s with v == x * s, element by element, bit for bit?"""
    if not x.size:
        return True
    i = int(np.argmax(np.abs(x)))
    if x[i] == 0.0:
        return not v.any()
    s0 = v[i] / x[i]
    cand = [s0]
    lo = hi = s0
    for _ in range(4):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        cand += [lo, hi]
    return any(np.array_equal(x * s, v) for s in cand)


def check_structure(out, m, scaled_in_place):
    """V unit lower trapezoidal, T upper triangular, tau == diag(T), the panel R above and V below -- exactly.

    scaled_in_place: CholeskyQR2 did the panel, which leaves V itself below the diagonal (and 1 in stage 1's scales).
    The Householder kernels (pq_resident, pq_step) leave the columns as the reflections left them, x_c, and
    1 / (alpha_c - beta_c) in stage 1's scales, which the entry does not return: V[:, c] = x_c * scale_c (s1_extract_v
    and pq_resident's write-back form exactly this product), so below the diagonal the panel's column c times ONE double
    must give V's column c bit for bit.

    m < 64: min(64, m) reflectors (`ncolq`); columns >= m of V are zero, as are tau[m - 1:] (reflector m - 1 has nothing
    below its head: tau = 0; the kernels zero the rest) and with them rows and columns >= m - 1 of T."""
    V, T, tau, P = out["V"], out["T"], out["tau"], out["P"]
    k = min(m, B)
    assert V.shape == (m, B) and P.shape == (m, B)
    assert np.array_equal(np.triu(V, 1), np.zeros((m, B)))
    assert np.array_equal(np.diag(V)[:k], np.ones(k))
    assert np.array_equal(np.tril(T, -1), np.zeros((B, B)))
    assert np.array_equal(tau, np.diag(T))
    if m <= B:
        assert not V[:, m:].any() and not tau[m - 1:].any() and not T[m - 1:, :].any() and not T[:, m - 1:].any()
    low = np.tril(np.ones((m, B), dtype=bool), -1)
    if scaled_in_place:
        assert np.array_equal(P[low], V[low])
    else:
        for c in range(k):
            assert _scaled_column_matches(P[c + 1:, c], V[c + 1:, c]), f"column {c}: the panel is not V / scale below the diagonal"
    for key in ("P", "V", "T", "tau", "Vw", "Tfold"):
        assert np.isfinite(out[key]).all(), key
