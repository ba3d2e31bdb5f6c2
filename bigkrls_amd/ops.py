"""Host-side mirror of the reference's `b*` helpers (R/bigKRLS_Rcpp_functions.R).

Same names, same argument meaning and the same error behaviour as the R
wrappers, but every matrix is a `DeviceMatrix` in HBM and every numeric step is a
HIP kernel reached through the C ABI (include/bigkrls.h).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from .device import Context, DeviceMatrix

GOLDEN = 0.381966  # R/bigKRLS_Rcpp_functions.R:38-39


def _hptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


# ---------------------------------------------------------------------------
# kernels   (R/bigKRLS_Rcpp_functions.R:201-227)
# ---------------------------------------------------------------------------
def bGaussKernel(X: DeviceMatrix, bandwidth: Optional[float] = None,
                 cols: Optional[Tuple[int, int]] = None) -> DeviceMatrix:
    """K[i,j] = exp(-||x_i-x_j||^2/bandwidth)  (bGaussKernel, :201-210 -> BigGaussKernel,
    src/gauss_kernel.cpp:32-42).  `cols=(c0,c1)` builds only the column block
    K[:, c0:c1] (== the row block, K is symmetric) for the multi-GPU partition."""
    ctx = X.ctx
    n, p = X.nrow, X.ncol
    bandwidth = float(p) if bandwidth is None else float(bandwidth)
    c0, c1 = (0, n) if cols is None else cols
    out = ctx.empty(n, c1 - c0)
    _lib.call("bigkrls_dev_kernel_block", ctx.handle, X.ptr, n, X.ld, X.col_ptr(0, c0), c1 - c0,
              X.ld, p, bandwidth, out.ptr, out.ld, c0)
    return out


def bNeffective(X: DeviceMatrix) -> float:
    """Effective sample size as a function of the mean absolute pairwise correlation of the
    rows of X (bNeffective, R/bigKRLS_Rcpp_functions.R:212-217 -> BigNeffective,
    src/Neffective.cpp:13-76)."""
    out = np.zeros(1, dtype=np.float64)
    _lib.call("bigkrls_dev_neffective", X.ctx.handle, X.ptr, X.nrow, X.ld, X.ncol, _hptr(out))
    return float(out[0])


def bTempKernel(X_new: DeviceMatrix, X_old: DeviceMatrix, sigma: float) -> DeviceMatrix:
    """out[i,j] = exp(-||new_i - old_j||^2/sigma)  (bTempKernel, :219-227)."""
    ctx = X_new.ctx
    if X_new.ncol != X_old.ncol:
        raise ValueError("bTempKernel: column counts differ")
    out = ctx.empty(X_new.nrow, X_old.nrow)
    _lib.call("bigkrls_dev_kernel_block", ctx.handle, X_new.ptr, X_new.nrow, X_new.ld, X_old.ptr,
              X_old.nrow, X_old.ld, X_new.ncol, float(sigma), out.ptr, out.ld, -1)
    return out


def bKernelContract(A: DeviceMatrix, B: DeviceMatrix, W: DeviceMatrix, sigma: float, trans: int = 0) -> DeviceMatrix:
    """trans=0: K(A, B) W (u x q); trans=1: K(A, B)' W (v x q), with K(A, B) bTempKernel's kernel, built tile by
    tile in registers and never stored (bigkrls_dev_kernel_contract). No counterpart in the reference."""
    ctx = A.ctx
    if A.ncol != B.ncol:
        raise ValueError("bKernelContract: column counts of A and B differ")
    if trans not in (0, 1):
        raise ValueError("bKernelContract: trans must be 0 or 1")
    if W.nrow != (B.nrow if trans == 0 else A.nrow):
        raise ValueError("bKernelContract: W has the wrong number of rows")
    out = ctx.empty(A.nrow if trans == 0 else B.nrow, W.ncol)
    _lib.call("bigkrls_dev_kernel_contract", ctx.handle, A.ptr, A.nrow, A.ld, B.ptr, B.nrow, B.ld, A.ncol,
              float(sigma), W.ptr, W.ncol, W.ld, int(trans), out.ptr, out.ld)
    return out


def bKernelContractGrouped(A: DeviceMatrix, B: DeviceMatrix, W: DeviceMatrix, sigma: float, labels, G: int) -> DeviceMatrix:
    """out (nrow(B) x G ncol(W)): the block of columns [g q, (g + 1) q) is K(A[labels == g], B)' W[labels == g], i.e.
    bKernelContract(trans=1) on the rows of every group, all groups in one fused launch; K is bTempKernel(A, B)'s kernel
    (centred by the column means of all of A). labels: nrow(A) integers in [0, G) in any order; an empty group gives zero
    columns (bigkrls_dev_kernel_contract_grouped). No counterpart in the reference."""
    ctx = A.ctx
    if A.ncol != B.ncol:
        raise ValueError("bKernelContractGrouped: column counts of A and B differ")
    if W.nrow != A.nrow:
        raise ValueError("bKernelContractGrouped: W has the wrong number of rows")
    lab = np.ascontiguousarray(labels, dtype=np.int64).ravel()
    if lab.size != A.nrow:
        raise ValueError(f"bKernelContractGrouped: labels must have {A.nrow} entries")
    G = int(G)
    if G < 1:
        raise ValueError("bKernelContractGrouped: G must be at least 1")
    out = ctx.empty(B.nrow, G * W.ncol)
    _lib.call("bigkrls_dev_kernel_contract_grouped", ctx.handle, A.ptr, A.nrow, A.ld, B.ptr, B.nrow, B.ld, A.ncol,
              float(sigma), W.ptr, W.ncol, W.ld, lab.ctypes.data, G, out.ptr, out.ld)
    return out


def bKernelLooColsums(A: DeviceMatrix, B: DeviceMatrix, sigma: float, cols) -> DeviceMatrix:
    """out (nrow(B) x len(cols)): out[l, jj] = sum_i exp(-(||A_i - B_l||^2 - (A[i,c] - B[l,c])^2) / sigma), c = cols[jj]
    (0-based): the column sums of bTempKernel(A, B) with column c left out of the distance, all selected columns in one
    fused pass (bigkrls_dev_kernel_loo_colsums). No counterpart in the reference."""
    ctx = A.ctx
    if A.ncol != B.ncol:
        raise ValueError("bKernelLooColsums: column counts of A and B differ")
    h_cols = np.ascontiguousarray(cols, dtype=np.int64).ravel()
    out = ctx.empty(B.nrow, max(int(h_cols.size), 1))
    _lib.call("bigkrls_dev_kernel_loo_colsums", ctx.handle, A.ptr, A.nrow, A.ld, B.ptr, B.nrow, B.ld, A.ncol,
              float(sigma), h_cols.ctypes.data, int(h_cols.size), out.ptr, out.ld)
    return out


def bKernelLooBinsums(A: DeviceMatrix, B: DeviceMatrix, sigma: float, cols, labels, nbins) -> DeviceMatrix:
    """out (nrow(B) x sum(nbins)): bKernelLooColsums' sums per bin of the left-out column. labels (nrow(A) x len(cols)):
    labels[i, jj] in [0, nbins[jj]) is the bin of row i of A under selected column cols[jj] (0-based) -- every column
    groups the rows its own way; the bins of column jj are consecutive columns of out, the columns in the caller's
    order. All columns and bins in one fused pass (bigkrls_dev_kernel_loo_binsums); an empty bin gives zeros. No
    counterpart in the reference."""
    ctx = A.ctx
    if A.ncol != B.ncol:
        raise ValueError("bKernelLooBinsums: column counts of A and B differ")
    h_cols = np.ascontiguousarray(cols, dtype=np.int64).ravel()
    h_nbins = np.ascontiguousarray(nbins, dtype=np.int64).ravel()
    if h_nbins.size != h_cols.size:
        raise ValueError("bKernelLooBinsums: nbins must have one entry per selected column")
    lab = np.asarray(labels, dtype=np.int64)
    if lab.size != A.nrow * h_cols.size or (lab.ndim == 2 and lab.shape != (A.nrow, h_cols.size)):
        raise ValueError(f"bKernelLooBinsums: labels must be {A.nrow} x {h_cols.size}")
    lab = np.ascontiguousarray(lab.reshape(A.nrow, h_cols.size).T)         # column-major u x n_cols
    out = ctx.empty(B.nrow, max(int(h_nbins.sum()), 1))
    _lib.call("bigkrls_dev_kernel_loo_binsums", ctx.handle, A.ptr, A.nrow, A.ld, B.ptr, B.nrow, B.ld, A.ncol,
              float(sigma), h_cols.ctypes.data if h_cols.size else np.zeros(1, dtype=np.int64).ctypes.data,
              int(h_cols.size), lab.ctypes.data if lab.size else np.zeros(1, dtype=np.int64).ctypes.data,
              h_nbins.ctypes.data if h_nbins.size else np.zeros(1, dtype=np.int64).ctypes.data, out.ptr, out.ld)
    return out


def bShapleyWeights(Z: DeviceMatrix, X: DeviceMatrix, Bg: DeviceMatrix, sigma: float, players=None) -> DeviceMatrix:
    """W (nrow(Z) M x nrow(X)): the weights of the exact interventional Shapley values on the coefficients of a Gaussian-
    kernel fit, W[r M + m, i] for explained row r of Z, player m and training row i of X, against the background rows Bg
    (bigkrls_dev_shapley_weights; all three in the same units): W[r M + m, :] c is the Shapley value of player m at Z[r, :]
    for the function x -> sum_i c_i K(x, X_i). players: ncol labels in [0, M), the player of every column (every player
    owns at least one column, M <= 128); None: one player per column. No counterpart in the reference."""
    ctx = Z.ctx
    if Z.ncol != X.ncol or Bg.ncol != X.ncol:
        raise ValueError("bShapleyWeights: column counts of Z, X and Bg differ")
    p = X.ncol
    if players is None:
        lab, M = None, p
    else:
        lab = np.ascontiguousarray(players, dtype=np.int64).ravel()
        if lab.size != p:
            raise ValueError(f"bShapleyWeights: players must have {p} entries")
        M = int(lab.max()) + 1 if lab.size else 0
    out = ctx.empty(Z.nrow * max(M, 1), X.nrow)
    _lib.call("bigkrls_dev_shapley_weights", ctx.handle, Z.ptr, Z.nrow, X.ptr, X.nrow, Bg.ptr, Bg.nrow, p, float(sigma),
              lab.ctypes.data if lab is not None else None, M, out.ptr)      # packed: a DeviceMatrix has ld == nrow
    return out


def bKernelLooMoments(A: DeviceMatrix, B: DeviceMatrix, sigma: float, entries) -> DeviceMatrix:
    """out (nrow(B) x len(entries)) for entries (kind, c, j) with 0-based columns: out[l, e] = sum_i wgt
    exp(-max(d2(i,l) - dc^2 - [kind = 2] dj^2, 0) / sigma) with dc = A[i,c] - B[l,c], dj = A[i,j] - B[l,j]; kind 0: wgt = 1
    (bKernelLooColsums' quantity, j ignored), kind 1: wgt = B[l,j] - A[i,j], kind 2: wgt = 1 with columns c and j both left
    out of the distance. All entries in one fused pass (bigkrls_dev_kernel_loo_moments). No counterpart in the reference."""
    ctx = A.ctx
    if A.ncol != B.ncol:
        raise ValueError("bKernelLooMoments: column counts of A and B differ")
    h = np.asarray(entries, dtype=np.int64)
    if h.size and (h.ndim != 2 or h.shape[1] != 3):
        raise ValueError("bKernelLooMoments: entries must be a list of (kind, c, j)")
    h = np.ascontiguousarray(h.reshape(-1, 3))                # row-major e x 3 == column-major 3 x e
    out = ctx.empty(B.nrow, max(int(h.shape[0]), 1))
    _lib.call("bigkrls_dev_kernel_loo_moments", ctx.handle, A.ptr, A.nrow, A.ld, B.ptr, B.nrow, B.ld, A.ncol,
              float(sigma), h.ctypes.data if h.size else np.zeros(3, dtype=np.int64).ctypes.data, int(h.shape[0]),
              out.ptr, out.ld)
    return out


def bQuadformDiag(A: DeviceMatrix, V: DeviceMatrix) -> DeviceMatrix:
    """diag(A V A') (m x 1) for A m x n and a general V n x n: out[i] = sum_j (A V)[i,j] A[i,j], without storing
    A V (bigkrls_dev_quadform_diag). No counterpart in the reference."""
    ctx = A.ctx
    if V.nrow != A.ncol or V.ncol != A.ncol:
        raise ValueError("bQuadformDiag: V must be ncol(A) x ncol(A)")
    out = ctx.empty(A.nrow, 1)
    _lib.call("bigkrls_dev_quadform_diag", ctx.handle, A.nrow, A.ncol, A.ptr, A.ld, V.ptr, V.ld, out.ptr)
    return out


def bRowSumSqWeighted(T: DeviceMatrix, w) -> DeviceMatrix:
    """out[i] = sum_j w[j] T[i,j]^2 (m x 1) = diag(T diag(w) T') for T m x k and k weights (a DeviceMatrix or a host
    array): with T = A Q it is bQuadformDiag(A, Q diag(w) Q') from the factors (bigkrls_dev_rowsumsq_weighted). No
    counterpart in the reference."""
    ctx = T.ctx
    dw = w if isinstance(w, DeviceMatrix) else ctx.from_numpy(np.asarray(w, dtype=np.float64).ravel())
    if dw.nrow * dw.ncol != T.ncol:
        raise ValueError("bRowSumSqWeighted: w must have ncol(T) entries")
    out = ctx.empty(T.nrow, 1)
    _lib.call("bigkrls_dev_rowsumsq_weighted", ctx.handle, T.nrow, T.ncol, T.ptr, T.ld, dw.ptr, out.ptr)
    return out


def bGemmModulated(A: DeviceMatrix, r, t, s, B: DeviceMatrix) -> DeviceMatrix:
    """(A o (r 1' + t s')) B (m x n) for A m x k, B k x n, r and t with m entries and s with k (DeviceMatrix or host
    arrays): out[i,j] = sum_l A[i,l] (r[i] + t[i] s[l]) B[l,j]. A is modulated on its way into the multiply and the
    modulated copy is never stored (bigkrls_dev_gemm_modulated); with r = 1, t = 0 it is the plain product bitwise.
    No counterpart in the reference."""
    ctx = A.ctx
    if B.nrow != A.ncol:
        raise ValueError("bGemmModulated: B must have ncol(A) rows")
    dev = [v if isinstance(v, DeviceMatrix) else ctx.from_numpy(np.asarray(v, dtype=np.float64).ravel()) for v in (r, t, s)]
    for v, want, name in zip(dev, (A.nrow, A.nrow, A.ncol), "rts"):
        if v.nrow * v.ncol != want or (v.ncol > 1 and v.nrow > 1):
            raise ValueError(f"bGemmModulated: {name} must be a vector with {want} entries")
    out = ctx.empty(A.nrow, B.ncol)
    _lib.call("bigkrls_dev_gemm_modulated", ctx.handle, A.nrow, B.ncol, A.ncol, A.ptr, A.ld, dev[0].ptr, dev[1].ptr,
              dev[2].ptr, B.ptr, B.ld, out.ptr, out.ld)
    return out


def bGemmModulated2(A: DeviceMatrix, r1, t1, s1, r2, t2, s2, B: DeviceMatrix, d: float = 0.0) -> DeviceMatrix:
    """(A o F) B (m x n) with F[i,l] = (r1[i] + t1[i] s1[l]) (r2[i] + t2[i] s2[l]) + d for A m x k, B k x n, r1, t1, r2,
    t2 with m entries and s1, s2 with k (DeviceMatrix or host arrays; s1 and s2 may be the same one): the product with a
    doubly modulated left operand in one pass, the modulated copy never stored (bigkrls_dev_gemm_modulated2); with
    r2 = 1, t2 = 0, d = 0 it is bGemmModulated(A, r1, t1, s1, B) bitwise. No counterpart in the reference."""
    ctx = A.ctx
    if B.nrow != A.ncol:
        raise ValueError("bGemmModulated2: B must have ncol(A) rows")
    dev = [v if isinstance(v, DeviceMatrix) else ctx.from_numpy(np.asarray(v, dtype=np.float64).ravel())
           for v in (r1, t1, s1, r2, t2, s2)]
    for v, want, name in zip(dev, (A.nrow, A.nrow, A.ncol) * 2, ("r1", "t1", "s1", "r2", "t2", "s2")):
        if v.nrow * v.ncol != want or (v.ncol > 1 and v.nrow > 1):
            raise ValueError(f"bGemmModulated2: {name} must be a vector with {want} entries")
    out = ctx.empty(A.nrow, B.ncol)
    _lib.call("bigkrls_dev_gemm_modulated2", ctx.handle, A.nrow, B.ncol, A.ncol, A.ptr, A.ld, dev[0].ptr, dev[1].ptr,
              dev[2].ptr, dev[3].ptr, dev[4].ptr, dev[5].ptr, float(d), B.ptr, B.ld, out.ptr, out.ld)
    return out


def bGramWeighted(A: DeviceMatrix, omega) -> DeviceMatrix:
    """A' diag(omega) A (k x k) for A n x k and n weights (a DeviceMatrix or a host array). The weight is applied on the
    way into the multiply, no weighted copy of A is stored, and the result is symmetric bit for bit
    (bigkrls_dev_gram_weighted). No counterpart in the reference."""
    ctx = A.ctx
    dw = omega if isinstance(omega, DeviceMatrix) else ctx.from_numpy(np.asarray(omega, dtype=np.float64).ravel())
    if dw.nrow * dw.ncol != A.nrow or (dw.ncol > 1 and dw.nrow > 1):
        raise ValueError(f"bGramWeighted: omega must be a vector with {A.nrow} entries")
    out = ctx.empty(A.ncol, A.ncol)
    _lib.call("bigkrls_dev_gram_weighted", ctx.handle, A.nrow, A.ncol, A.ptr, A.ld, dw.ptr, out.ptr, out.ld)
    return out


def bClusterScores(A: DeviceMatrix, e, labels, G: int) -> DeviceMatrix:
    """S (k x G): S[j, g] = sum of e[i] A[i, j] over the rows i with labels[i] == g, for A n x k, e with n entries (a
    DeviceMatrix or a host array) and n integer labels in [0, G) in any order; an empty cluster gives a zero column
    (bigkrls_dev_cluster_scores). No counterpart in the reference."""
    ctx = A.ctx
    de = e if isinstance(e, DeviceMatrix) else ctx.from_numpy(np.asarray(e, dtype=np.float64).ravel())
    if de.nrow * de.ncol != A.nrow or (de.ncol > 1 and de.nrow > 1):
        raise ValueError(f"bClusterScores: e must be a vector with {A.nrow} entries")
    lab = np.ascontiguousarray(labels, dtype=np.int64).ravel()
    if lab.size != A.nrow:
        raise ValueError(f"bClusterScores: labels must have {A.nrow} entries")
    G = int(G)
    if G < 1:
        raise ValueError("bClusterScores: G must be at least 1")
    out = ctx.empty(A.ncol, G)
    _lib.call("bigkrls_dev_cluster_scores", ctx.handle, A.nrow, A.ncol, A.ptr, A.ld, de.ptr, lab.ctypes.data, G,
              out.ptr, out.ld)
    return out


def bDeletionResiduals(Q: DeviceMatrix, w, e, labels=None, G: int = 0, route: int = 0, hat: bool = False,
                       scores: bool = False):
    """et (n, host): for the rows S of every unit, et[S] = (I - H_SS)^-1 e[S] with H = Q diag(w) Q' (Q n x k on the
    device, w k weights, e n entries); labels: n integers in [0, G), or None: every row is its own unit. route 0: units of
    up to 256 rows in the fused kernel, 1: the general route through the eigensolver (bigkrls_dev_deletion_residuals).
    hat / scores: also the leverages (n, host) and the scores Q_S' et_S (a k x G DeviceMatrix). Returns et, or the tuple
    (et, hat, scores) with None for what was not asked for. No counterpart in the reference."""
    ctx = Q.ctx
    n, k = Q.nrow, Q.ncol
    wv = np.ascontiguousarray(w, dtype=np.float64).ravel()
    if wv.size != k:
        raise ValueError(f"bDeletionResiduals: w must have {k} entries")
    de = e if isinstance(e, DeviceMatrix) else ctx.from_numpy(np.asarray(e, dtype=np.float64).ravel())
    if de.nrow * de.ncol != n:
        raise ValueError(f"bDeletionResiduals: e must be a vector with {n} entries")
    lab = None
    if labels is not None:
        lab = np.ascontiguousarray(labels, dtype=np.int64).ravel()
        if lab.size != n:
            raise ValueError(f"bDeletionResiduals: labels must have {n} entries")
    U = int(G) if lab is not None else n
    det = ctx.empty(n, 1)
    dhat = ctx.empty(n, 1) if hat else None
    dS = ctx.empty(k, max(U, 1)) if scores else None
    _lib.call("bigkrls_dev_deletion_residuals", ctx.handle, n, k, Q.ptr, Q.ld, wv.ctypes.data, de.ptr,
              lab.ctypes.data if lab is not None else None, int(G), int(route), det.ptr,
              dhat.ptr if hat else None, dS.ptr if scores else None, dS.ld if scores else 0)
    et = det.to_numpy().ravel()
    if not hat and not scores:
        return et
    return et, (dhat.to_numpy().ravel() if hat else None), dS


# ---------------------------------------------------------------------------
# eigen   (R/bigKRLS_Rcpp_functions.R:173-199)
# ---------------------------------------------------------------------------
@dataclass
class Eigenobject:
    values: np.ndarray          # all Neig eigenvalues, descending (host)
    lastkeeper: int             # number of kept pairs
    vectors: DeviceMatrix       # N x lastkeeper
    values_dev: DeviceMatrix    # the same eigenvalues on the device


def bEigen(A: DeviceMatrix, Neig: Optional[int] = None, eigtrunc: float = 0.0,
           part: Optional[Tuple[int, int]] = None) -> Eigenobject:
    """bEigen (:173-199): all Neig eigenvalues are kept, eigenvectors only for
    1..lastkeeper = max(which(values >= eigtrunc*values[1])) (:190).  The sign flip
    at :186 is immaterial (quirk Q9) and not reproduced.  `part=(rank, world)` (multi-GPU):
    only this rank's slice of the kept eigenvector columns is back-transformed, the others
    are zeros (sum over ranks = Q)."""
    ctx = A.ctx
    n = A.nrow
    if A.ncol != n:
        raise ValueError("bEigen: matrix must be square")
    Neig = n if Neig is None else int(Neig)
    if not (1 <= Neig <= n):
        raise ValueError("bEigen: Neig out of range")
    vals = ctx.empty(Neig, 1)
    vecs = ctx.empty(n, Neig)
    nv = C.c_int64(0)
    if part is None:
        _lib.call("bigkrls_dev_eigen", ctx.handle, A.ptr, n, A.ld, Neig, vals.ptr, Neig,
                  float(eigtrunc), vecs.ptr, vecs.ld, C.byref(nv))
    else:
        _lib.call("bigkrls_dev_eigen_part", ctx.handle, A.ptr, n, A.ld, Neig, vals.ptr, Neig,
                  float(eigtrunc), vecs.ptr, vecs.ld, C.byref(nv), int(part[0]), int(part[1]))
    values = vals.to_numpy().ravel()
    lastkeeper = int(nv.value)
    return Eigenobject(values=values, lastkeeper=lastkeeper, vectors=vecs.cols(0, lastkeeper),
                       values_dev=vals)


def bEigenImplicit(X: DeviceMatrix, sigma: Optional[float] = None, Neig: int = 0, eigtrunc: float = 0.0) -> Eigenobject:
    """bEigen of bGaussKernel(X, sigma) without the matrix (bigkrls_dev_eigen_implicit): block Lanczos whose products
    with K are fused contractions over X. X is the standardised N x P data; needs N >= 1024 and 4 Neig <= N, and has no
    dense fallback (a spectrum the iteration does not resolve is an error)."""
    ctx = X.ctx
    n, p = X.nrow, X.ncol
    sigma = float(p) if sigma is None else float(sigma)
    Neig = int(Neig)
    if not (1 <= Neig <= n):
        raise ValueError("bEigenImplicit: Neig out of range")
    vals = ctx.empty(Neig, 1)
    vecs = ctx.empty(n, Neig)
    nv = C.c_int64(0)
    _lib.call("bigkrls_dev_eigen_implicit", ctx.handle, X.ptr, n, X.ld, p, sigma, Neig, vals.ptr, Neig,
              float(eigtrunc), vecs.ptr, vecs.ld, C.byref(nv))
    lastkeeper = int(nv.value)
    return Eigenobject(values=vals.to_numpy().ravel(), lastkeeper=lastkeeper, vectors=vecs.cols(0, lastkeeper),
                       values_dev=vals)


def bEigenAuto(X: DeviceMatrix, sigma: Optional[float] = None, eigtrunc: float = 0.001, max_pairs: Optional[int] = None,
               K: Optional[DeviceMatrix] = None) -> Eigenobject:
    """bEigen without a rank (bigkrls_dev_eigen_auto): the block Lanczos grows its subspace until the spectrum is
    resolved down to eigtrunc * lambda_1 (eigtrunc > 0) and returns what Neig = lastkeeper + 1 would: lastkeeper + 1
    values -- the last one below the threshold -- and lastkeeper vectors. `K`: the stored kernel matrix (X, sigma are
    then not used; the dense path takes over where the iteration does not converge); without it the operator built
    from the standardised N x P data X, as in bEigenImplicit. `max_pairs` caps the search (default min(N // 4, 2048));
    a spectrum with more eigenvalues above the threshold is an error."""
    src = K if K is not None else X
    ctx, n = src.ctx, src.nrow
    if K is not None and K.ncol != n:
        raise ValueError("bEigenAuto: K must be square")
    if not (0.0 < float(eigtrunc) <= 1.0):
        raise ValueError("bEigenAuto: eigtrunc must be in (0, 1]")
    cap = min(n // 4, 2048) if max_pairs is None else int(max_pairs)
    if not (1 <= cap <= n):
        raise ValueError("bEigenAuto: max_pairs out of range")
    p = 0 if X is None else X.ncol
    sigma = float(p) if sigma is None else float(sigma)
    vals = ctx.empty(cap, 1)
    vecs = ctx.empty(n, cap)
    nvals, nv = C.c_int64(0), C.c_int64(0)
    _lib.call("bigkrls_dev_eigen_auto", ctx.handle, K.ptr if K is not None else None, n, K.ld if K is not None else n,
              X.ptr if X is not None else None, X.ld if X is not None else n, p, sigma, float(eigtrunc), cap, vals.ptr,
              vecs.ptr, vecs.ld, C.byref(nvals), C.byref(nv))
    lastkeeper = int(nv.value)
    return Eigenobject(values=vals.to_numpy().ravel()[:int(nvals.value)].copy(), lastkeeper=lastkeeper,
                       vectors=vecs.cols(0, lastkeeper), values_dev=vals)


# ---------------------------------------------------------------------------
# solveforc / lambda search   (R/bigKRLS_Rcpp_functions.R:5-95)
# ---------------------------------------------------------------------------
class _SolveState:
    """a = Q'y hoisted out of the probes; cached per (Eigenobject, y)."""

    def __init__(self, eig: Eigenobject, y: DeviceMatrix):
        ctx = y.ctx
        Q = eig.vectors
        self.a = ctx.empty(Q.ncol, 1)
        _lib.call("bigkrls_dev_qty", ctx.handle, Q.ptr, Q.nrow, Q.ncol, Q.ld, y.ptr, self.a.ptr)


def _state(eig: Eigenobject, y: DeviceMatrix) -> _SolveState:
    """The cached a = Q'y is reused only for the very same tensor object in the very same state:
    the state keeps a reference to y's tensor (so its address cannot be recycled for another
    array while the cache lives) and torch's in-place version counter (bumped by every torch
    write). Writes torch cannot see (a raw kernel through the C ABI) must go through a new
    DeviceMatrix or `forget_solve_state`."""
    key = "_solve_state"
    st = getattr(eig, key, None)
    if st is None or st.y_tensor is not y.t or st.y_version != y.t._version:
        st = _SolveState(eig, y)
        st.y_tensor = y.t
        st.y_version = y.t._version
        setattr(eig, key, st)
    return st


def forget_solve_state(eig: Eigenobject) -> None:
    """Drop the cached Q'y of an Eigenobject (after y was overwritten behind torch's back)."""
    if hasattr(eig, "_solve_state"):
        delattr(eig, "_solve_state")


def bSolveForc(y: DeviceMatrix, Eigenobject: Eigenobject, lambda_: float):
    """bSolveForc (:84-90) -> BigSolveForc (src/solveforc.cpp:67-78).
    Returns dict(Le=..., coeffs=DeviceMatrix N x 1)."""
    ctx = y.ctx
    Q = Eigenobject.vectors
    st = _state(Eigenobject, y)
    c = ctx.empty(Q.nrow, 1)
    le = C.c_double()
    _lib.call("bigkrls_dev_solveforc", ctx.handle, Q.ptr, Q.nrow, Q.ncol, Q.ld,
              Eigenobject.values_dev.ptr, st.a.ptr, float(lambda_), c.ptr, C.byref(le))
    return {"Le": float(le.value), "coeffs": c}


def bLooLoss(y: DeviceMatrix, Eigenobject: Eigenobject, lambda_: float) -> float:
    """bLooLoss (:92-95)."""
    ctx = y.ctx
    Q = Eigenobject.vectors
    st = _state(Eigenobject, y)
    le = C.c_double()
    _lib.call("bigkrls_dev_solveforc", ctx.handle, Q.ptr, Q.nrow, Q.ncol, Q.ld,
              Eigenobject.values_dev.ptr, st.a.ptr, float(lambda_), None, C.byref(le))
    return float(le.value)


def lambda_bounds(values: np.ndarray, n: int) -> Tuple[float, float]:
    """The U and L loops of bLambdaSearch (:16-36) (host, uses ALL Neig values, quirk Q5)."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    L = C.c_double()
    U = C.c_double()
    _lib.call("bigkrls_lambda_bounds", _hptr(v), v.size, int(n), C.byref(L), C.byref(U))
    return float(L.value), float(U.value)


def bLambdaSearch(L=None, U=None, y: DeviceMatrix = None, Eigenobject: Eigenobject = None,
                  tol=None, noisy=False, trace: Optional[List[Tuple[float, float]]] = None,
                  loo=None) -> float:
    """bLambdaSearch (:5-82), statement for statement.  `loo(lambda)` may be
    supplied to evaluate the leave-one-out loss elsewhere (the multi-GPU path sums
    row-block partials with an all-reduce); by default it is bLooLoss."""
    if np.isnan(Eigenobject.values).any():
        raise ValueError("Missing eigenvalues prevent bigKRLS from obtaining the regularization "
                         "parameter lambda.\n\tCheck for repeated observations (or other perfect "
                         "linear combinations in X).")
    n = y.nrow
    if tol is None:
        tol = 1e-3 * n
    else:
        if not (np.isscalar(tol) and tol > 0):
            raise ValueError("tol must be a positive scalar")
    if U is None or L is None:
        L0, U0 = lambda_bounds(Eigenobject.values, n)
        U = U0 if U is None else U
        L = L0 if L is None else L
    if not (np.isscalar(U) and U > 0):
        raise ValueError("U must be a positive scalar")
    if not (np.isscalar(L) and L >= 0):
        raise ValueError("L must be a non-negative scalar")
    if loo is None:
        def loo(lam):
            return bLooLoss(y=y, Eigenobject=Eigenobject, lambda_=lam)

    def probe(lam):
        s = loo(lam)
        if trace is not None:
            trace.append((float(lam), float(s)))
        return s

    X1 = L + GOLDEN * (U - L)
    X2 = U - GOLDEN * (U - L)
    S1 = probe(X1)
    S2 = probe(X2)
    it = 0
    while abs(S1 - S2) > tol:
        if S1 < S2:
            U = X2
            X2 = X1
            X1 = L + GOLDEN * (U - L)
            S2 = S1
            S1 = probe(X1)
        else:
            L = X1
            X1 = X2
            X2 = U - GOLDEN * (U - L)
            S1 = S2
            S2 = probe(X2)
        it += 1
        if it > 10000 or not np.isfinite(S1 + S2):
            raise RuntimeError("bLambdaSearch: golden-section search did not terminate")
        if noisy:
            print(f"L: {L:.3f} X1: {X1:.3f} X2: {X2:.3f} U: {U:.3f} S1: {S1:.3f} S2: {S2:.3f}")
    return float(X1 if S1 < S2 else X2)


# ---------------------------------------------------------------------------
# multdiag / cross-products   (R/bigKRLS_Rcpp_functions.R:159-171, 229-258)
# ---------------------------------------------------------------------------
def bMultDiag(X: DeviceMatrix, v) -> DeviceMatrix:
    """out[:,i] = X[:,i]*v[i] (bMultDiag :159-171 -> src/multdiag.cpp:13-24)."""
    ctx = X.ctx
    v = np.asarray(v, dtype=np.float64).ravel()
    if v.size < X.ncol:
        raise ValueError("bMultDiag: diag shorter than ncol(X)")
    dv = ctx.from_numpy(v[: X.ncol])
    out = ctx.empty(X.nrow, X.ncol)
    _lib.call("bigkrls_dev_multdiag", ctx.handle, X.ptr, X.nrow, X.ncol, X.ld, dv.ptr, out.ptr, out.ld)
    return out


def gemm(ta: bool, tb: bool, A: DeviceMatrix, B: DeviceMatrix, alpha: float = 1.0,
         out: Optional[DeviceMatrix] = None, beta: float = 0.0) -> DeviceMatrix:
    ctx = A.ctx
    m = A.ncol if ta else A.nrow
    k = A.nrow if ta else A.ncol
    kb = B.ncol if tb else B.nrow
    n = B.nrow if tb else B.ncol
    if k != kb:
        raise ValueError(f"gemm: inner dimensions differ ({k} vs {kb})")
    if out is None:
        out = ctx.empty(m, n)
    _lib.call("bigkrls_dev_gemm", ctx.handle, int(ta), int(tb), m, n, k, float(alpha), A.ptr, A.ld,
              B.ptr, B.ld, float(beta), out.ptr, out.ld)
    return out


def bCrossProd(X: DeviceMatrix, Y: Optional[DeviceMatrix] = None) -> DeviceMatrix:
    """X'Y or X'X (bCrossProd :229-243 -> src/crossprod.cpp:13-48)."""
    return gemm(True, False, X, X if Y is None else Y)


def bTCrossProd(X: DeviceMatrix, Y: Optional[DeviceMatrix] = None) -> DeviceMatrix:
    """XY' or XX' (bTCrossProd :245-258 -> src/crossprod.cpp:51-85)."""
    return gemm(False, True, X, X if Y is None else Y)


def matvec(A: DeviceMatrix, x: DeviceMatrix, trans: bool = False) -> DeviceMatrix:
    """A %*% x for a single column x (bigalgebra dgemv, R/bigKRLS.R:291,601)."""
    ctx = A.ctx
    out = ctx.empty(A.ncol if trans else A.nrow, 1)
    _lib.call("bigkrls_dev_gemv", ctx.handle, int(trans), A.nrow, A.ncol, 1.0, A.ptr, A.ld, x.ptr,
              0.0, out.ptr)
    return out


# ---------------------------------------------------------------------------
# derivatives   (R/bigKRLS_Rcpp_functions.R:260-270)
# ---------------------------------------------------------------------------
def binary_columns(Xhost: np.ndarray) -> np.ndarray:
    """src/bigderiv_v3.cpp:28-31: a column with exactly two distinct values."""
    out = np.zeros(Xhost.shape[1], dtype=bool)
    for j in range(Xhost.shape[1]):
        col = Xhost[:, j]
        if col.size:
            lo, hi = col.min(), col.max()          # exactly two distinct values <=> everything is lo or hi
            out[j] = bool(lo != hi and np.all((col == lo) | (col == hi)))
    return out


def deriv_scales(Xhost: np.ndarray, is_binary: np.ndarray, sigma: float) -> np.ndarray:
    n, p = Xhost.shape
    sc = np.empty(p)
    for j in range(p):
        if is_binary[j]:
            sd = 1.0 / (Xhost[:, j].max() - Xhost[:, j].min())      # src/bigderiv_v3.cpp:36
            sc[j] = 2.0 * sd * sd / (float(n) ** 2)                  # :85
        else:
            sc[j] = 4.0 / (sigma * sigma * float(n) ** 2)            # :105
    return sc


def bDerivatives(X: DeviceMatrix, sigma: float, K: DeviceMatrix, coeffs: DeviceMatrix,
                 eig: Eigenobject, wv: np.ndarray, Xhost: np.ndarray):
    """bDerivatives (:260-270) -> BigDerivMat (src/bigderiv_v3.cpp:113-132) in its
    O(N^2) form.  `vcovmatc` is represented by its factors (eig.vectors, wv):
    V = Q diag(wv) Q'.  Returns dict(derivatives=DeviceMatrix N x P, varavgderiv=ndarray P)."""
    ctx = X.ctx
    n, p = X.nrow, X.ncol
    isb = binary_columns(Xhost)
    isb32 = np.ascontiguousarray(isb.astype(np.int32))
    D = ctx.empty(n, p)
    S = ctx.empty(n, p)
    _lib.call("bigkrls_dev_deriv_rows", ctx.handle, K.ptr, n, n, K.ld, 0, X.ptr, p, X.ld,
              _hptr(isb32), coeffs.ptr, float(sigma), D.ptr, D.ld, S.ptr, S.ld)
    scale = np.ascontiguousarray(deriv_scales(Xhost, isb, sigma))
    var = np.empty(p)
    Q = eig.vectors
    dwv = ctx.from_numpy(np.asarray(wv, dtype=np.float64)[: Q.ncol])
    _lib.call("bigkrls_dev_deriv_var", ctx.handle, Q.ptr, n, Q.ncol, Q.ld, dwv.ptr, S.ptr, p, S.ld,
              _hptr(scale), _hptr(var))
    return {"derivatives": D, "varavgderiv": var}
