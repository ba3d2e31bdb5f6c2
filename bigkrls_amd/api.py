"""bigKRLS(), predict(), crossvalidate(): host-side mirror of the reference's R API
(R/bigKRLS.R:97-516, 547-637, 1146-1336) over HIP device buffers.

The control flow, argument names (dots become underscores), defaults, validation
messages and output fields follow the R functions so that the parity tests read
like the reference's own; every N x N object lives in HBM as a DeviceMatrix and
every numeric step is a HIP kernel behind the C ABI (include/bigkrls.h).
"""
from __future__ import annotations

import math
import time
from typing import Dict, List, Optional, Sequence

import numpy as np

import ctypes as C

from . import _lib, ops
from ._lib import i64
from .device import Context, DeviceMatrix, is_device_matrix

_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx


def _sd(v) -> float:
    return float(np.std(np.asarray(v, dtype=np.float64), ddof=1))


def _var(v) -> float:
    return float(np.var(np.asarray(v, dtype=np.float64), ddof=1))


def _cor(a, b) -> float:
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    a0, b0 = a - a.mean(), b - b.mean()
    return float((a0 @ b0) / math.sqrt((a0 @ a0) * (b0 @ b0)))


class BigKRLS(dict):
    """The list `w` returned by bigKRLS() (R/bigKRLS.R:420-469), class "bigKRLS"."""

    r_class = "bigKRLS"


class BigKRLSPredicted(dict):
    r_class = "bigKRLS_predicted"


class BigKRLSCV(dict):
    """crossvalidate.bigKRLS's output (R/bigKRLS.R:1330-1336), class "bigKRLS_CV"."""

    r_class = "bigKRLS_CV"


def _as_host_matrix(X) -> np.ndarray:
    if is_device_matrix(X):
        return X.to_numpy()
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    return X


def _call_native(name, *args):
    """A library call whose BIGKRLS_EINVAL (the reference's validation errors, with R's message
    text) becomes the ValueError the R-mirroring API raises; BIGKRLS_ENOMEM is retried once after
    torch's cached-but-unused device blocks were released; everything else stays a BigKRLSError."""
    for attempt in (0, 1):
        try:
            _lib.call(name, *args)
            return
        except _lib.BigKRLSError as e:
            if e.code == _lib.EINVAL:
                raise ValueError(str(e).split(": ", 2)[-1]) from None
            if e.code == _lib.ENOMEM and attempt == 0:
                # the library's workspace comes from hipMalloc; blocks that torch's caching allocator
                # holds but does not use are invisible to it: hand them back to the driver and retry once
                import torch
                torch.cuda.empty_cache()
                continue
            raise


def bigKRLS(y=None, X=None, sigma=None, derivative=True, which_derivatives=None, vcov_est=True,
            Neig=None, eigtrunc=None, lambda_=None, L=None, U=None, tol=None,
            model_subfolder_name=None, overwrite_existing=False, Ncores=None,
            acf=False, noisy=None, instructions=True, ctx: Optional[Context] = None,
            timings: Optional[Dict[str, float]] = None,
            trace: Optional[list] = None, comm=None, keep_outputs: bool = True,
            vcov_form: str = "dense", max_factors: Optional[int] = None, kernel: str = "stored") -> BigKRLS:
    """Kernel-regularised least squares fit (R/bigKRLS.R:97-516).

    The numeric body -- validation of the data, standardisation, the five steps and the rescaling
    (R/bigKRLS.R:175-470) -- is ONE call into the C ABI, `bigkrls_fit` (include/bigkrls.h,
    csrc/fit.hip); this function checks the argument types, allocates the outputs (the reference's
    ownership rule: the caller allocates, native code writes in place) and assembles the list `w`.
    `which_derivatives` is 1-based like R.  `lambda_` is R's `lambda`.  `model_subfolder_name` /
    `overwrite_existing` (R/bigKRLS.R:111-133, :471-504): the fitted object is also written to that
    folder -- never silently into an existing one -- exactly as save_bigKRLS() does (device-resident
    matrices as text, the rest as estimates.RData), and `w["path"]` records where.  `Ncores` (PSOCK
    workers of the derivative loop, :337-363) and `instructions` are accepted and have no effect: the
    marginal effects of all columns are one pass over K on the GPU.  `timings`
    (optional dict) receives per-phase seconds measured with HIP events on the context's stream;
    `trace` (optional list) the (lambda, Le) probes of the golden-section search.
    `comm` (a bigkrls_amd.dist.Comm): the fit runs over the ranks of that communicator -- every process calls
    with the same y, X and arguments -- through `bigkrls_fit_dist`; the N x N outputs are then this rank's
    column blocks `K.cols`, `vcov.est.c.cols`, `vcov.est.fitted.cols` (n x (r1 - r0), rows `w["rows"]`),
    or not kept at all with keep_outputs=False.
    `vcov_form`: how the variance of the coefficients is returned. "dense" (default): the N x N matrices
    `vcov.est.c` and `vcov.est.fitted`. "factors": `vcov.est.Q` (a DeviceMatrix, N x lastkeeper: the kept
    eigenvectors) and `vcov.est.w` (lastkeeper weights) with vcov.est.c = Q diag(w) Q' and vcov.est.fitted =
    Q diag(w d^2) Q' (d = K.eigenvalues[:lastkeeper]); both matrices are None and K is the only N x N buffer of the
    call. "both": all of them from one fit. predict() and marginal_effects() work from either form. With a
    communicator every rank holds the whole Q and w, so a multi-GPU object with factors can be used downstream on any
    single rank. The buffer for Q has `Neig` columns when Neig was given or nothing is truncated (eigtrunc 0),
    otherwise `max_factors` (default min(N, 2048)); a fit that keeps more eigenpairs than that raises a ValueError --
    factors are never truncated -- and the columns not needed are released after the call.
    `kernel`: "stored" (default) builds the N x N kernel matrix; "implicit" never stores it -- every product with K
    (the block Lanczos steps, the check of the decomposition, K c, the marginal-effects pass) rebuilds the kernel tiles
    from X inside a fused contraction, so the fit holds no N x N buffer at all: O(N maxdim + N Neig) doubles with
    maxdim = min(N/2, max(16 Neig, 4096)). It needs `Neig` with N >= 1024 and 4 Neig <= N (block Lanczos only: there is
    no dense fallback), one GPU, and vcov_form="factors" whenever vcov_est is true. The object then has K = None and
    w["kernel"] = "implicit"; predict(), marginal_effects(), summary() and save / load work on it unchanged.
    `Neig="auto"` (one GPU, N >= 1024, either kernel form): the block Lanczos finds the rank itself -- it grows its
    subspace until the spectrum is resolved down to eigtrunc * lambda_1 and returns what a fit with
    Neig = lastkeeper + 1 returns, so `K.eigenvalues` has lastkeeper + 1 entries. eigtrunc must be > 0 (the default is
    0 for N <= 3000: pass one). The search is capped at min(N // 4, max_factors if given else 2048) pairs; a spectrum
    with more eigenvalues above the threshold raises a ValueError. An eigenvalue of multiplicity above the block size
    128 can be missed, as with a given Neig.
    """
    ctx = (comm.ctx if comm is not None else ctx) or default_context()
    if X is None or y is None:
        raise ValueError("y and X are required")
    if model_subfolder_name is not None and not isinstance(model_subfolder_name, str):        # :112
        raise TypeError("model_subfolder_name must be a character string")
    return_big_rectangles = is_device_matrix(X)                                  # :149
    # column-major like R / the C ABI
    Xh = np.array(_as_host_matrix(X), dtype=np.float64, order="F")
    yh = np.ascontiguousarray(np.array(_as_host_matrix(y), dtype=np.float64).ravel())
    n, p = Xh.shape
    return_big_squares = return_big_rectangles or n > 2500                       # :150
    w = BigKRLS()
    w["has.big.matrices"] = bool(return_big_squares or return_big_rectangles)
    noisy = (n > 2000) if noisy is None else bool(noisy)                          # :153
    xlabs = [f"x{i + 1}" for i in range(p)]                                       # :167
    # ---- argument checks the C ABI cannot see (its "unset" is <= 0 / NULL) ----------------------
    if eigtrunc is not None and (not np.isscalar(eigtrunc) or eigtrunc < 0 or eigtrunc > 1):   # :195-201
        raise ValueError("eigtrunc must be between 0 (no truncation) and 1 (keep largest only).")
    if which_derivatives is not None:                                             # :206-215
        if not derivative:
            raise ValueError("which.derivative requires derivative = TRUE")
        which_derivatives = [int(i) for i in which_derivatives]
        if not which_derivatives or not all(1 <= i <= p for i in which_derivatives):
            raise ValueError("which.derivatives must index columns of X")
    if n != yh.shape[0]:
        raise ValueError("nrow(X) not equal to number of elements in y.")
    if lambda_ is not None and not (np.isscalar(lambda_) and lambda_ > 0):        # :225
        raise ValueError("lambda must be a positive scalar")
    if sigma is not None and not (np.isscalar(sigma) and sigma > 0):              # :227
        raise ValueError("sigma must be a positive scalar")
    if tol is not None and not (np.isscalar(tol) and tol > 0):                    # :232-236 (validated, never forwarded: :274-275)
        raise ValueError("tol must be a positive scalar")
    if U is not None and not (np.isscalar(U) and U > 0):
        raise ValueError("U must be a positive scalar")
    if L is not None and not (np.isscalar(L) and L >= 0):
        raise ValueError("L must be a non-negative scalar")
    neig_auto = isinstance(Neig, str)
    if neig_auto:
        if Neig != "auto":
            raise ValueError('Neig must be a positive integer or "auto"')
        if comm is not None:
            raise ValueError('Neig="auto" runs on one GPU: drop comm, or pass Neig')
        if n < 1024:
            raise ValueError(f'Neig="auto" needs N >= 1024 (N = {n}): pass Neig, or leave it out')
        if ((0.001 if n > 3000 else 0.0) if eigtrunc is None else float(eigtrunc)) == 0.0:
            raise ValueError('Neig="auto" finds the rank from eigtrunc, which is 0 here (the default for N <= 3000): '
                             'pass eigtrunc > 0')
    elif Neig is not None and int(Neig) < 1:
        raise ValueError("Neig must be a positive integer")
    neig = n if Neig is None else (n // 4 if neig_auto else min(n, int(Neig)))    # :194 (auto: the cap, see below)
    if vcov_form not in ("dense", "factors", "both"):
        raise ValueError('vcov_form must be "dense", "factors" or "both"')
    if max_factors is not None and not (isinstance(max_factors, (int, np.integer)) and not isinstance(max_factors, bool)
                                        and max_factors >= 1):
        raise ValueError("max_factors must be a positive integer")
    if kernel not in ("stored", "implicit"):
        raise ValueError('kernel must be "stored" or "implicit"')
    implicit = kernel == "implicit"
    if implicit:
        if comm is not None:
            raise ValueError('kernel="implicit" runs on one GPU: drop comm, or use kernel="stored"')
        if Neig is None:
            raise ValueError('kernel="implicit" needs Neig (the block Lanczos computes the Neig largest eigenpairs): '
                             'pass Neig <= N/4, or use kernel="stored"')
        if n < 1024:
            raise ValueError(f'kernel="implicit" needs N >= 1024 (N = {n}): use kernel="stored"')
        if 4 * neig > n:
            raise ValueError(f'kernel="implicit" needs 4 Neig <= N (Neig = {neig}, N = {n}): pass Neig <= {n // 4}, '
                             'or use kernel="stored"')
        if vcov_est and vcov_form != "factors":
            raise ValueError('kernel="implicit" returns the variance as factors: pass vcov_form="factors" '
                             '(or vcov_est=False, derivative=False)')
    want_dense, want_factors = vcov_form != "factors", vcov_form != "dense"
    if want_factors and not vcov_est:
        raise ValueError('vcov_form = "factors" / "both" requires vcov_est = True')
    if neig_auto:                     # the cap of the rank search: the eigenvalue buffer and the factor buffer hold it
        neig = min(n // 4, int(max_factors) if max_factors is not None else 2048)
    qcap = 0
    if want_factors:
        eigtrunc_eff = (0.001 if n > 3000 else 0.0) if eigtrunc is None else float(eigtrunc)      # :195-201
        if Neig is not None or eigtrunc_eff == 0.0:       # (Neig="auto": neig is the cap)
            qcap = neig
        else:
            qcap = min(neig, int(max_factors) if max_factors is not None else min(n, 2048))
    pd = 0 if not derivative else (p if which_derivatives is None else len(which_derivatives))

    opt = _lib.FitOptions()
    opt.struct_bytes = C.sizeof(_lib.FitOptions)
    opt.sigma = -1.0 if sigma is None else float(sigma)
    opt.lambda_ = -1.0 if lambda_ is None else float(lambda_)
    opt.L = -1.0 if L is None else float(L)
    opt.U = -1.0 if U is None else float(U)
    opt.eigtrunc = -1.0 if eigtrunc is None else float(eigtrunc)
    opt.neig = 0 if neig_auto else neig             # (auto: ignored, the cap is bigkrls_fit_auto's own argument)
    opt.derivative = int(bool(derivative))
    opt.vcov_est = int(bool(vcov_est))
    opt.acf = int(bool(acf))
    opt.kernel_form = 1 if implicit else 0
    which_arr = None
    if which_derivatives is not None:
        which_arr = np.ascontiguousarray(which_derivatives, dtype=np.int64)
        opt.which_derivatives = which_arr.ctypes.data_as(_lib.pi64)
        opt.n_which = which_arr.size

    def hbuf(*shape):
        return np.empty(shape, dtype=np.float64, order="F")

    out = _lib.FitOutputs()
    out.struct_bytes = C.sizeof(_lib.FitOutputs)
    vals, coeffs, yf, yfs = hbuf(neig), hbuf(n), hbuf(n), hbuf(n)
    isbin = np.zeros(p, dtype=np.int32)
    max_trace = 512
    tracebuf = hbuf(2 * max_trace)
    out.eigenvalues, out.coeffs = vals.ctypes.data, coeffs.ctypes.data
    out.yfitted, out.yfitted_std = yf.ctypes.data, yfs.ctypes.data
    out.binaryindicator = isbin.ctypes.data
    out.lambda_trace, out.max_trace = tracebuf.ctypes.data, max_trace
    if derivative:
        D, Dstd = hbuf(n, pd), hbuf(n, pd)
        avg, var, varstd = hbuf(pd), hbuf(pd), hbuf(pd)
        out.derivatives, out.derivatives_std = D.ctypes.data, Dstd.ctypes.data
        out.avgderivatives, out.var_avgderivatives = avg.ctypes.data, var.ctypes.data
        out.var_avgderivatives_std = varstd.ctypes.data
    r0, r1 = 0, n
    if comm is not None:
        a0, a1 = i64(0), i64(0)
        _call_native("bigkrls_fit_dist_rows", comm.handle, n, C.byref(opt), C.byref(a0), C.byref(a1))
        r0, r1 = int(a0.value), int(a1.value)
    ncols = r1 - r0                                                               # columns of K this process holds
    K = vcovmatc = vcovmatyhat = Qf = wf = None
    if (keep_outputs or comm is None) and not implicit:
        K = ctx.empty(n, max(ncols, 1))                                           # :434
        out.d_K = K.ptr
        if vcov_est and want_dense:
            vcovmatc, vcovmatyhat = ctx.empty(n, max(ncols, 1)), ctx.empty(n, max(ncols, 1))
            out.d_vcov_c, out.d_vcov_fitted = vcovmatc.ptr, vcovmatyhat.ptr
    if want_factors:                                                              # whole on every rank
        Qf, wf = ctx.empty(n, qcap), np.zeros(qcap)
        out.d_vcov_q, out.vcov_q_cols_max, out.vcov_w = Qf.ptr, qcap, wf.ctypes.data

    t_wall0 = time.perf_counter()
    try:
        if neig_auto:
            _call_native("bigkrls_fit_auto", ctx.handle, Xh.ctypes.data, yh.ctypes.data, n, p, C.byref(opt), neig,
                         C.byref(out))
        elif comm is None:
            _call_native("bigkrls_fit", ctx.handle, Xh.ctypes.data, yh.ctypes.data, n, p, C.byref(opt), C.byref(out))
        else:
            _call_native("bigkrls_fit_dist", comm.handle, Xh.ctypes.data, yh.ctypes.data, n, p, C.byref(opt),
                         C.byref(out))
    except ValueError as e:
        if neig_auto and "kcap" in str(e):                   # the cap of the rank search (bigkrls_dev_eigen_auto)
            raise ValueError(f'{e}: Neig="auto" searched up to {neig} pairs -- raise max_factors (at most N // 4 = '
                             f'{n // 4}), or pass Neig') from None
        if want_factors and int(out.lastkeeper) > qcap:      # the library's capacity error (include/bigkrls.h)
            raise ValueError(f"{e}: pass max_factors >= {int(out.lastkeeper)} (or vcov_form='dense')") from None
        raise
    t_native = time.perf_counter() - t_wall0
    if want_factors:
        kq = int(out.vcov_q_cols)
        if kq < qcap:                                         # keep the lastkeeper columns, release the rest
            Qf = Qf.keep_first_cols(kq)
            wf = wf[:kq].copy()

    if trace is not None:
        for i in range(min(int(out.n_probes), max_trace)):
            trace.append((float(tracebuf[2 * i]), float(tracebuf[2 * i + 1])))
    w["X"] = Xh
    w["K.eigenvalues"] = vals[:int(out.neig)].copy() if neig_auto else vals       # :268 (auto: lastkeeper + 1 values)
    w["lastkeeper"] = int(out.lastkeeper)                                         # :269
    w["Neffective"] = float(out.Neffective)                                       # :280
    if derivative:
        w["derivatives.std"] = Dstd
        w["var.avgderivatives.std"] = varstd
        w["R2AME"] = float(out.R2AME)                                             # :392
    w["Neffective.acf"] = float(out.Neffective_acf) if (acf and p > 2) else None  # :412-416, :431
    w["coeffs"] = coeffs                                                          # :420
    w["y"] = yh
    w["sigma"] = float(out.sigma)
    w["lambda"] = float(out.lambda_)
    w["binaryindicator"] = isbin.astype(bool)
    w["which.derivatives"] = which_derivatives
    w["xlabs"] = xlabs
    w["yfitted.std"] = yfs
    w["yfitted"] = yf                                                             # :428
    w["R2"] = float(out.R2)                                                       # :429
    w["Looe"] = float(out.Looe)                                                   # :430
    w["Le"] = float(out.Le)
    w["sigmasq"] = float(out.sigmasq) if vcov_est else None
    if comm is not None:
        w["rows"] = (r0, r1)
        if keep_outputs:
            cut = (lambda m: m if ncols > 0 else None)
            w["K.cols"] = cut(K)
            w["vcov.est.c.cols"] = cut(vcovmatc) if vcovmatc is not None else None
            w["vcov.est.fitted.cols"] = cut(vcovmatyhat) if vcovmatyhat is not None else None
    else:
        w["K"] = None if implicit else (K if return_big_squares else K.to_numpy())   # :434
        if vcovmatc is not None:
            w["vcov.est.c"] = vcovmatc if return_big_squares else vcovmatc.to_numpy()          # :438
            w["vcov.est.fitted"] = vcovmatyhat if return_big_squares else vcovmatyhat.to_numpy()   # :445
        else:
            w["vcov.est.c"] = None
            w["vcov.est.fitted"] = None
    if want_factors:                                          # flat keys: save_bigKRLS / load_bigKRLS carry them as they are
        w["vcov.est.Q"] = Qf
        w["vcov.est.w"] = wf
    if implicit:                                              # (stored fits keep the member list they always had)
        w["kernel"] = "implicit"
    w["derivative.call"] = derivative
    if derivative:
        w["avgderivatives"] = avg[None, :]                                        # :400
        w["var.avgderivatives"] = var[None, :]                                    # :403-407
        w["derivatives"] = D
    if timings is not None:
        for name, sec in zip(_lib.PHASES, out.phase_s):
            timings[name] = float(sec)
        timings["native"] = t_native
        timings["wall"] = time.perf_counter() - t_wall0
    w["_ctx"] = ctx
    if model_subfolder_name is not None:                                          # :471-504
        from .persist import save_bigKRLS
        if comm is None:
            save_bigKRLS(w, model_subfolder_name, overwrite_existing=overwrite_existing, noisy=noisy)
        elif comm.rank == 0:
            # every rank holds the same small outputs: ONE rank writes them (several would race for the folder name);
            # the sharded column blocks are not members load_bigKRLS knows and stay on the GPUs
            small = BigKRLS({k: v for k, v in w.items() if not k.endswith(".cols")})
            save_bigKRLS(small, model_subfolder_name, overwrite_existing=overwrite_existing, noisy=noisy)
            w["path"], w["model_subfolder_name"] = small["path"], small["model_subfolder_name"]
    return w


def _betacf(a: float, b: float, x: float) -> float:
    """Continued fraction of the regularised incomplete beta function (modified Lentz)."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 500):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h


def _chi2_sf(x: float, df: float) -> float:
    """P(X > x) for a chi-square with df degrees of freedom (R: pchisq(x, df, lower.tail=FALSE)): the regularised upper
    incomplete gamma function Q(df/2, x/2) -- the series of P below a + 1, the continued fraction of Q (modified Lentz)
    above, the common factor exp(-x + a log x - lgamma(a)) formed in logs so that a large x underflows to 0. df = 2 is
    exp(-x/2) itself."""
    if not np.isfinite(df) or not df > 0 or x != x:
        return float("nan")
    if x <= 0.0:
        return 1.0
    a, z = 0.5 * df, 0.5 * x
    if a == 1.0:
        return math.exp(-z)
    if z == float("inf"):
        return 0.0
    front = math.exp(-z + a * math.log(z) - math.lgamma(a))
    if z < a + 1.0:
        term = total = 1.0 / a
        ap = a
        for _ in range(10000):
            ap += 1.0
            term *= z / ap
            total += term
            if abs(term) < abs(total) * 1e-17:
                break
        return min(max(1.0 - front * total, 0.0), 1.0)
    tiny = 1e-300
    b = z + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / (b if abs(b) > tiny else tiny)
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = b + an / c
        c = c if abs(c) > tiny else tiny
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return min(max(front * h, 0.0), 1.0)


def _wald(theta, Sigma, reference_index: int):
    """Wald test of H0: all entries of theta are equal, theta ~ N(., Sigma). With C the (G - 1) x G differences against
    entry `reference_index`: (C theta)' pinv(C Sigma C') (C theta), the pseudo-inverse from the symmetric eigenpairs above
    max eigenvalue x (G - 1) x machine epsilon; df = the rank used, p = the upper chi-square tail. Returns
    (statistic, df, p); G = 1, or a covariance of rank 0, gives (0, 0, nan). Host only."""
    theta = np.asarray(theta, dtype=np.float64).ravel()
    Sigma = np.asarray(Sigma, dtype=np.float64)
    G = theta.size
    if Sigma.shape != (G, G):
        raise ValueError("Sigma must be length(theta) x length(theta)")
    if not 0 <= int(reference_index) < G:
        raise ValueError("reference_index must index theta")
    if G < 2:
        return 0.0, 0, float("nan")
    Cm = np.delete(np.eye(G), int(reference_index), axis=0)
    Cm[:, int(reference_index)] = -1.0
    d = Cm @ theta
    Vd = Cm @ Sigma @ Cm.T
    w, U = np.linalg.eigh(0.5 * (Vd + Vd.T))
    keep = w > max(w.max(), 0.0) * (G - 1) * np.finfo(np.float64).eps
    df = int(keep.sum())
    if df == 0:
        return 0.0, 0, float("nan")
    z = U[:, keep].T @ d
    stat = float(np.sum(z * z / w[keep]))
    return stat, df, _chi2_sf(stat, df)


def _pt_upper(t: float, df: float) -> float:
    """P(T > t) for Student's t with df degrees of freedom, t >= 0 (R: pt(t, df, lower.tail=FALSE)):
    0.5 I_x(df/2, 1/2) with x = df / (df + t^2)."""
    if not np.isfinite(t) or not df > 0:
        return float("nan")
    import math
    x = df / (df + t * t)
    a, b = 0.5 * df, 0.5
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 0.5
    lbeta = math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b)
    front = math.exp(lbeta + a * math.log(x) + b * math.log1p(-x))
    if x < (a + 1.0) / (a + b + 2.0):
        ib = front * _betacf(a, b, x) / a
    else:
        ib = 1.0 - front * _betacf(b, a, 1.0 - x) / b
    return 0.5 * ib


def summary(object: BigKRLS, degrees: str = "Neffective", probs=(0.05, 0.25, 0.5, 0.75, 0.95),
            digits: int = 4, labs=None, quiet: bool = False) -> Optional[dict]:
    """summary.bigKRLS (R/bigKRLS.R:666-757): t-tests of the average marginal effects and the
    percentiles of the pointwise marginal effects. Returns {"ttests": (P' x 4), "percentiles":
    (P' x len(probs)), "rownames": [...]}; prints the R text unless `quiet`."""
    if not isinstance(object, BigKRLS):
        raise TypeError("Object not of class 'bigKRLS'")
    if degrees not in ("acf", "Neffective", "N"):                                 # :677
        raise ValueError('degrees must be one of "acf", "Neffective", "N"')
    Xh = np.asarray(object["X"], dtype=np.float64)
    N = n = Xh.shape[0]
    if degrees == "Neffective":                                                   # :679-681
        n = object["Neffective"]
    if degrees == "acf":                                                          # :682-691
        if object.get("Neffective.acf") is None:
            ctx = object.get("_ctx") or default_context()
            Xs = (Xh - Xh.mean(axis=0)) / Xh.std(axis=0, ddof=1)                  # scale(object$X[])
            n = ops.bNeffective(ctx.from_numpy(Xs))
        else:
            n = object["Neffective.acf"]
    say = (lambda *a: None) if quiet else (lambda *a: print(*a))
    say("\n\nMODEL SUMMARY:\n")
    say("lambda:", round(object["lambda"], digits))
    say("N:", N)
    if n != N:
        say("N Effective:", n)
    p = Xh.shape[1]
    say("R2:", round(float(object["R2"]), digits))
    if object.get("vcov.type") not in (None, "classical"):
        say("vcov:", object["vcov.type"])
    if object.get("derivatives") is None:                                         # :700-703
        say("\nrecompute with bigKRLS(..., derivative = TRUE) for estimates of marginal effects\n")
        return None
    if object.get("R2AME") is not None:
        say("R2AME**:", round(float(object["R2AME"]), digits), "\n")
    if labs is not None:                                                          # :708-714
        if len(labs) != p:
            raise ValueError("length(labs) must equal ncol(X)")
        names = list(labs)
    else:
        names = list(object["xlabs"])
    which = object.get("which.derivatives") or list(range(1, p + 1))              # :716-718
    est = np.asarray(object["avgderivatives"], dtype=np.float64).ravel()          # :720
    se = np.sqrt(np.asarray(object["var.avgderivatives"], dtype=np.float64).ravel())
    if degrees != "Neffective":                                                   # :722-724
        se = se * N / n
    tval = est / se
    pval = np.array([2.0 * _pt_upper(abs(t), n - p) for t in tval])              # :726
    AME = np.column_stack([est, se, tval, pval])
    isbin = np.asarray(object["binaryindicator"], dtype=bool)
    rown = [names[i - 1] + ("*" if isbin[i - 1] else "") for i in which]          # :729-733
    deriv = np.asarray(object["derivatives"], dtype=np.float64).reshape(N, len(which))
    qderiv = np.quantile(deriv, list(probs), axis=0).T                            # R quantile type 7
    say("Average Marginal Effects:\n")
    say("%-12s %12s %12s %12s %12s" % ("", "Estimate", "Std. Error", "t value", "Pr(>|t|)"))
    for nm, row in zip(rown, np.round(AME, digits)):
        say("%-12s %12g %12g %12g %12g" % (nm, *row))
    say("\n\nPercentiles of Marginal Effects:\n")
    say("%-12s " % "" + " ".join("%11s%%" % (100 * q) for q in probs))
    for nm, row in zip(rown, np.round(qderiv, digits)):
        say("%-12s " % nm + " ".join("%12g" % v for v in row))
    if isbin.any():
        say("\n(*) Reported average and percentiles of dy/dx is for discrete change of the dummy "
            "variable from min to max (usually 0 to 1)).\n")
    say("\n(**) Pseudo-R^2 computed using only the Average Marginal Effects.")
    return {"ttests": AME, "percentiles": qderiv, "rownames": rown,
            "colnames": ["Estimate", "Std. Error", "t value", "Pr(>|t|)"], "n": n}


def _vcov_choice(object, vcov):
    """The form of vcov.est.c a post-fit call works from: "dense" (the N x N matrix), "factors" (vcov.est.Q and
    vcov.est.w) or None (the object has neither). vcov=None prefers the dense matrix; "dense" / "factors" force a
    form and raise when the object does not carry it."""
    if vcov not in (None, "dense", "factors"):
        raise ValueError('vcov must be None, "dense" or "factors"')
    has_dense = object.get("vcov.est.c") is not None
    has_factors = object.get("vcov.est.Q") is not None and object.get("vcov.est.w") is not None
    if vcov == "dense" and not has_dense:
        raise ValueError('the object has no vcov.est.c: refit with vcov_form="dense" or "both"')
    if vcov == "factors" and not has_factors:
        raise ValueError('the object has no vcov.est.Q / vcov.est.w: refit with vcov_form="factors" or "both"')
    if vcov is None:
        return "dense" if has_dense else ("factors" if has_factors else None)
    return vcov


def _factors(object, ctx):
    """(Q on the device, w contiguous on the host) of an object that carries the factors of vcov.est.c."""
    Q = object["vcov.est.Q"]
    Qd = Q if is_device_matrix(Q) else ctx.from_numpy(np.asarray(Q, dtype=np.float64))
    wv = np.ascontiguousarray(np.asarray(object["vcov.est.w"], dtype=np.float64).ravel())
    if wv.size != Qd.ncol or Qd.nrow != np.asarray(object["X"]).shape[0]:
        raise ValueError("vcov.est.Q must be nrow(X) x length(vcov.est.w)")
    return Qd, wv


def _effects_open(name, object, newdata, vcov, se, gated=False, default=None):
    """The common opening of the post-estimation functions, up to what needs no device: the class check, the form of
    vcov.est.c, the se-without-vcov error, the multi-GPU refusal (under `name`), X, newdata and the two-valued columns.
    gated: without se no variance is computed at all (form None, a multi-GPU object accepted). default: what
    newdata=None means -- None: not allowed, "training": X itself, "null": the native call takes a null pointer for the
    training rows (nd_init and nd None, u = n). Returns Xh, n, p, nd_init, nd, u, isbin, form."""
    if not isinstance(object, BigKRLS):
        raise TypeError("Object not of class 'bigKRLS'")
    form = _vcov_choice(object, vcov)
    if gated and not se:
        form = None
    if se and form is None:
        raise ValueError("recompute bigKRLS object with bigKRLS(,vcov.est=TRUE) to compute standard errors")
    if (se or not gated) and ("vcov.est.c.cols" in object or "rows" in object) and form != "factors":
        raise NotImplementedError(f"{name} of a multi-GPU fit (sharded vcov.est.c.cols) is not supported; "
                                  "refit on one GPU or with vcov_form=\"factors\"")
    Xh = np.asfortranarray(np.asarray(object["X"], dtype=np.float64))
    n, p = Xh.shape
    nd_init, nd, u = None, None, n
    if newdata is not None or default != "null":
        nd_init = Xh if newdata is None and default == "training" else _as_host_matrix(newdata)
        nd = np.array(nd_init, dtype=np.float64, order="F")
        if nd.ndim != 2 or nd.shape[1] != p:
            raise ValueError("ncol(newdata) differs from ncol(X) from fitted bigKRLS object")
        u = nd.shape[0]
        if u < 1:
            raise ValueError("newdata has no rows")
        if not np.all(np.isfinite(nd)):
            raise ValueError("newdata contains missing or infinite values")
    isbin = np.array([np.unique(Xh[:, j]).size == 2 for j in range(p)])          # the fit's rule (R/bigKRLS.R:242)
    return Xh, n, p, nd_init, nd, u, isbin, form


def _effects_device(object, form, ctx, p):
    """... and, after the function's own validation, what the native call takes: the context, vcov.est.c on the device in
    the chosen form, y and the coefficients, the five vcov arguments of the C ABI (d_vcov_c, d_Q, ldq, k, h_w), the labels.
    Returns ctx, Vd, Qd, wv, yv, coeffs, vcov_args, xlabs."""
    ctx = ctx or object.get("_ctx") or default_context()
    V = object.get("vcov.est.c") if form == "dense" else None
    Vd = None if V is None else (V if is_device_matrix(V) else ctx.from_numpy(np.asarray(V, dtype=np.float64)))
    Qd, wv = _factors(object, ctx) if form == "factors" else (None, None)
    yv = np.ascontiguousarray(np.asarray(object["y"], dtype=np.float64).ravel())
    coeffs = np.ascontiguousarray(np.asarray(object["coeffs"], dtype=np.float64).ravel())
    vcov_args = (Vd.ptr if form == "dense" else None, Qd.ptr if form == "factors" else None,
                 Qd.ld if form == "factors" else 0, Qd.ncol if form == "factors" else 0,
                 wv.ctypes.data if form == "factors" else None)
    xlabs = list(object.get("xlabs") or [f"x{i + 1}" for i in range(p)])
    return ctx, Vd, Qd, wv, yv, coeffs, vcov_args, xlabs


def _check_binary_newdata(Xh, nd, isbin, cols):
    """newdata must hold one of the two training values in every binary column of cols (0-based, in this order)."""
    for j in cols:
        if isbin[j]:
            lo, hi = Xh[:, j].min(), Xh[:, j].max()
            if not np.all((nd[:, j] == lo) | (nd[:, j] == hi)):
                raise ValueError(f"newdata column {j + 1} is binary in the training data; its values must be "
                                 f"one of the two training values ({lo:g}, {hi:g})")


def predict(object: BigKRLS, newdata, se_pred=False, correct_SE=True, ytest=None,
            ctx: Optional[Context] = None, matrices=True, vcov: Optional[str] = None) -> BigKRLSPredicted:
    """predict.bigKRLS (R/bigKRLS.R:547-637); the numeric body (:590-621) is ONE call into the
    C ABI, `bigkrls_predict` (include/bigkrls.h, csrc/fit.hip).

    matrices=False: the same `predicted` and `se.pred` through `bigkrls_predict_pointwise`, which takes the new
    points in row blocks and never forms newdataK (u x n) or vcov.est.pred (u x u); both come back as None. Its
    extra device memory stays near 1.1 GiB whatever the number of new points.

    vcov: the form of vcov.est.c the standard errors come from. None: the N x N matrix when the object has it, else
    its factors (a fit with vcov_form="factors", on one GPU or several); "dense" / "factors" force one and raise a
    ValueError when the object does not carry it. From the factors the numeric body is `bigkrls_predict_factored`:
    se^2_i = sum_j w_j (newdataK Q)_ij^2, about n / lastkeeper times fewer flops than the product with the matrix."""
    if not isinstance(object, BigKRLS):
        raise TypeError("Object not of class 'bigKRLS'")
    form = _vcov_choice(object, vcov)
    if se_pred and form is None:
        raise ValueError("recompute bigKRLS object with bigKRLS(,vcov.est=TRUE) to compute standard errors")
    ctx = ctx or object.get("_ctx") or default_context()
    Xh = np.asfortranarray(np.asarray(object["X"], dtype=np.float64))
    bigmatrix_in = is_device_matrix(newdata) or bool(object["has.big.matrices"])   # :582
    nd_init = _as_host_matrix(newdata)
    nd = np.array(nd_init, dtype=np.float64, order="F")
    if Xh.shape[1] != nd.shape[1]:
        raise ValueError("ncol(newdata) differs from ncol(X) from fitted bigKRLS object")
    n, p = Xh.shape
    u = nd.shape[0]
    yv = np.ascontiguousarray(np.asarray(object["y"], dtype=np.float64).ravel())
    coeffs = np.ascontiguousarray(np.asarray(object["coeffs"], dtype=np.float64).ravel())
    ypred = np.empty(u)
    if se_pred and form == "factors":
        return _predict_factored(object, ctx, Xh, nd, nd_init, yv, coeffs, ypred, correct_SE, ytest, bigmatrix_in,
                                 matrices)
    if not matrices:
        return _predict_pointwise(object, ctx, Xh, nd, nd_init, yv, coeffs, ypred, se_pred, correct_SE, ytest,
                                  bigmatrix_in)
    newdataK = ctx.empty(u, n)
    se = vcov_est_pred = Vd = None
    neff = -1.0
    if se_pred:
        V = object["vcov.est.c"]
        Vd = V if is_device_matrix(V) else ctx.from_numpy(np.asarray(V))
        vcov_est_pred = ctx.empty(u, u)
        se = np.empty(u)
        if correct_SE and object.get("Neffective") is not None:                   # :610-611
            neff = float(object["Neffective"])
    _call_native("bigkrls_predict", ctx.handle, Xh.ctypes.data, n, p, yv.ctypes.data, coeffs.ctypes.data,
                 float(object["sigma"]), nd.ctypes.data, u, Vd.ptr if se_pred else None, neff,
                 ypred.ctypes.data, se.ctypes.data if se_pred else None, newdataK.ptr,
                 vcov_est_pred.ptr if se_pred else None)
    if not bigmatrix_in:                                                          # :623-626
        vcov_est_pred = None if vcov_est_pred is None else vcov_est_pred.to_numpy()
        newdataK = newdataK.to_numpy()
    out = BigKRLSPredicted(predicted=ypred, newdata=nd_init, newdataK=newdataK, ytest=ytest)
    out["se.pred"] = se
    out["vcov.est.pred"] = vcov_est_pred
    out["has.big.matrices"] = bigmatrix_in
    return out


def _predict_pointwise(object, ctx, Xh, nd, nd_init, yv, coeffs, ypred, se_pred, correct_SE, ytest, bigmatrix_in):
    """predict(..., matrices=False) after predict()'s own checks: one call into bigkrls_predict_pointwise."""
    n, p = Xh.shape
    u = nd.shape[0]
    se = Vd = None
    neff = -1.0
    if se_pred:
        V = object["vcov.est.c"]
        Vd = V if is_device_matrix(V) else ctx.from_numpy(np.asarray(V))
        se = np.empty(u)
        if correct_SE and object.get("Neffective") is not None:                   # :610-611
            neff = float(object["Neffective"])
    _call_native("bigkrls_predict_pointwise", ctx.handle, Xh.ctypes.data, n, p, yv.ctypes.data, coeffs.ctypes.data,
                 float(object["sigma"]), nd.ctypes.data, u, Vd.ptr if se_pred else None, neff,
                 ypred.ctypes.data, se.ctypes.data if se_pred else None)
    out = BigKRLSPredicted(predicted=ypred, newdata=nd_init, newdataK=None, ytest=ytest)
    out["se.pred"] = se
    out["vcov.est.pred"] = None
    out["has.big.matrices"] = bigmatrix_in
    return out


def _predict_factored(object, ctx, Xh, nd, nd_init, yv, coeffs, ypred, correct_SE, ytest, bigmatrix_in, matrices):
    """predict(..., se_pred=True) from the factors of vcov.est.c after predict()'s own checks: one call into
    bigkrls_predict_factored, with the two matrices as outputs (matrices=True) or in row blocks without them."""
    n, p = Xh.shape
    u = nd.shape[0]
    Qd, wv = _factors(object, ctx)
    newdataK = ctx.empty(u, n) if matrices else None
    vcov_est_pred = ctx.empty(u, u) if matrices else None
    se = np.empty(u)
    neff = -1.0
    if correct_SE and object.get("Neffective") is not None:                       # :610-611
        neff = float(object["Neffective"])
    _call_native("bigkrls_predict_factored", ctx.handle, Xh.ctypes.data, n, p, yv.ctypes.data, coeffs.ctypes.data,
                 float(object["sigma"]), nd.ctypes.data, u, Qd.ptr, Qd.ld, Qd.ncol, wv.ctypes.data, neff,
                 ypred.ctypes.data, se.ctypes.data, newdataK.ptr if matrices else None,
                 vcov_est_pred.ptr if matrices else None)
    if matrices and not bigmatrix_in:                                             # :623-626
        vcov_est_pred, newdataK = vcov_est_pred.to_numpy(), newdataK.to_numpy()
    out = BigKRLSPredicted(predicted=ypred, newdata=nd_init, newdataK=newdataK, ytest=ytest)
    out["se.pred"] = se
    out["vcov.est.pred"] = vcov_est_pred
    out["has.big.matrices"] = bigmatrix_in
    return out


def marginal_effects(object: BigKRLS, newdata, which_derivatives=None, ctx: Optional[Context] = None,
                     vcov: Optional[str] = None, se: bool = False, _block_rows: int = 0) -> dict:
    """Marginal effects of a fitted model at new data points, without refitting: the pointwise derivatives
    (u x |J|), their averages (1 x |J|) and the variances of the averages (1 x |J|; None when the object has no
    vcov.est.c), in the original units and with the fit's definitions -- with newdata = X they are the fit's
    `derivatives`, `avgderivatives` and `var.avgderivatives`. Binary training columns take the first difference
    between their two training values, so newdata must hold one of those two values there. `which_derivatives`
    (1-based) defaults to the object's own, or all columns. No counterpart in the reference (which computes the
    marginal effects at the training rows only, R/bigKRLS.R:318-407). The numeric body is ONE call into the C ABI,
    `bigkrls_marginal_effects`, which never forms the u x n test kernel. `vcov` chooses the form of vcov.est.c the
    variances come from, as in predict(): from the factors (`bigkrls_marginal_effects_factored`) the variance step is
    the fit's own sum_k w_k (q_k's)^2, and a multi-GPU object that carries them is accepted.

    se=True adds "se.derivatives" (u x |J|, the columns of "derivatives"): the standard error of every pointwise
    derivative, sqrt(g' vcov.est.c g) / sd(x_j) for the weights g with derivative = g'c, from the same form of vcov.est.c
    as "var.avgderivatives" (a second call, `bigkrls_marginal_effects_se`; everything else in the result is bitwise
    what se=False returns). Binary columns carry the reference's factor 2 on the variance, as var.avgderivatives does,
    so for a single new point se.derivatives[0, j]**2 == var.avgderivatives[0, j] in every column. The factors are the
    fast form: 2 u n lastkeeper flops per column against 2 u n^2 from the matrix; the new points are taken in row blocks
    of at most 1 GiB of test kernel either way. Raises the ValueError of predict(se_pred=True) when the object carries
    neither form. With se=False the result has exactly the keys it always had."""
    Xh, n, p, nd_init, nd, u, isbin, form = _effects_open("marginal_effects", object, newdata, vcov, se)
    if which_derivatives is None:
        which_derivatives = object.get("which.derivatives")
    if which_derivatives is None:
        which = list(range(1, p + 1))
    else:
        which = [int(i) for i in np.atleast_1d(which_derivatives)]
        if not which or not all(1 <= i <= p for i in which):
            raise ValueError("which.derivatives must index columns of X")
    _check_binary_newdata(Xh, nd, isbin, sorted(set(i - 1 for i in which)))
    ctx, Vd, Qd, wv, yv, coeffs, vcov_args, xlabs = _effects_device(object, form, ctx, p)
    which_arr = np.ascontiguousarray(which, dtype=np.int64)
    nj = which_arr.size
    D = np.empty((u, nj), dtype=np.float64, order="F")
    avg = np.empty(nj)
    var = np.empty(nj) if form is not None else None
    if form == "factors":
        _call_native("bigkrls_marginal_effects_factored", ctx.handle, Xh.ctypes.data, n, p, yv.ctypes.data,
                     coeffs.ctypes.data, float(object["sigma"]), which_arr.ctypes.data, nj, nd.ctypes.data, u,
                     Qd.ptr, Qd.ld, Qd.ncol, wv.ctypes.data, D.ctypes.data, avg.ctypes.data, var.ctypes.data)
    else:
        _call_native("bigkrls_marginal_effects", ctx.handle, Xh.ctypes.data, n, p, yv.ctypes.data, coeffs.ctypes.data,
                     float(object["sigma"]), which_arr.ctypes.data, nj, nd.ctypes.data, u,
                     Vd.ptr if Vd is not None else None, D.ctypes.data, avg.ctypes.data,
                     var.ctypes.data if var is not None else None)
    out = {"derivatives": D, "avgderivatives": avg[None, :],
           "var.avgderivatives": None if var is None else var[None, :],
           "which.derivatives": which, "binaryindicator": isbin[which_arr - 1],
           "xlabs": [xlabs[i - 1] for i in which], "newdata": nd_init}
    if se:
        sed = np.empty((u, nj), dtype=np.float64, order="F")
        _call_native("bigkrls_marginal_effects_se", ctx.handle, Xh.ctypes.data, n, p, yv.ctypes.data,
                     coeffs.ctypes.data, float(object["sigma"]), which_arr.ctypes.data, nj, nd.ctypes.data, u,
                     *vcov_args, int(_block_rows), sed.ctypes.data)
        out["se.derivatives"] = sed
    return out


def interaction_effects(object: BigKRLS, newdata=None, pairs=None, which=None, se: bool = False,
                        vcov: Optional[str] = None, ctx: Optional[Context] = None, _block_rows: int = 0) -> dict:
    """Interaction effects of a fitted model at new data points, without refitting: does the effect of x_j depend on
    x_k? For every pair (j, k) the pointwise values "interactions" (u x m), their averages "avginteractions" (1 x m) and
    the variances of the averages "var.avginteractions" (1 x m; None when the object has no vcov.est.c), in the original
    units. Continuous x continuous: the cross-derivative d^2 yhat / dx_j dx_k (j = k: the second derivative); binary x
    continuous: the derivative in x_k of the first difference in x_j; binary x binary (j != k): the second difference
    over the two pairs of training values, divided by both gaps. A pair (j, j) on a binary column is not defined. The
    Gaussian kernel gives all of them in closed form: the second-order operator is the product of marginal_effects'
    first-order modulations (include/bigkrls.h, bigkrls_interaction_effects). No counterpart in the reference.

    newdata=None: the training X. `pairs`: 1-based (j, k), each stored ordered (j <= k) in the result; the default is
    every j <= k over `which` (default: the object's which.derivatives, or all columns) without the binary diagonals.
    Binary columns of a pair must hold one of their two training values in newdata. `vcov` and the multi-GPU rule are
    marginal_effects'. se=True adds "se.interactions" (u x m): the standard error of every pointwise value from the
    same form of vcov.est.c (a second call, `bigkrls_interaction_effects_se`; the factors are the fast form:
    2 u n lastkeeper flops per pair in one pass of bigkrls_dev_gemm_modulated2); everything else in the result is
    bitwise what se=False returns. Variances carry the reference's factor 2 when a column of the pair is binary, so for
    a single new point se.interactions[0, i]**2 == var.avginteractions[0, i] for every pair."""
    Xh, n, p, nd_init, nd, u, isbin, form = _effects_open("interaction_effects", object, newdata, vcov, se,
                                                         default="training")
    if pairs is None:
        if which is None:
            which = object.get("which.derivatives")
        if which is None:
            cols = list(range(1, p + 1))
        else:
            cols = sorted(set(int(i) for i in np.atleast_1d(which)))
            if not cols or not all(1 <= i <= p for i in cols):
                raise ValueError("which must index columns of X")
        pairs = [(j, k) for a, j in enumerate(cols) for k in cols[a:] if not (j == k and isbin[j - 1])]
        if not pairs:
            raise ValueError("no pair is left: the only selected column is binary")
    else:
        if which is not None:
            raise ValueError("give pairs or which, not both")
        try:
            pairs = [(int(j), int(k)) for j, k in pairs]
        except (TypeError, ValueError):
            raise ValueError("pairs must be a list of (j, k) column indices") from None
        if not pairs:
            raise ValueError("pairs is empty")
    ordered = []
    for j, k in pairs:
        if not (1 <= j <= p and 1 <= k <= p):
            raise ValueError(f"pair ({j}, {k}) must index columns of X")
        j, k = min(j, k), max(j, k)
        if j == k and isbin[j - 1]:
            raise ValueError(f"pair ({j}, {k}) is not defined: column {j} is binary in the training data")
        if (j, k) in ordered:
            raise ValueError(f"pair ({j}, {k}) is given more than once")
        ordered.append((j, k))
    _check_binary_newdata(Xh, nd, isbin, sorted(set(c - 1 for pr in ordered for c in pr)))
    ctx, Vd, Qd, wv, yv, coeffs, vcov_args, xlabs = _effects_device(object, form, ctx, p)
    pair_arr = np.ascontiguousarray(ordered, dtype=np.int64)                      # m x 2 row-major: pair after pair
    m = len(ordered)
    vals = np.empty((u, m), dtype=np.float64, order="F")
    avg = np.empty(m)
    var = np.empty(m) if form is not None else None
    _call_native("bigkrls_interaction_effects", ctx.handle, Xh.ctypes.data, n, p, yv.ctypes.data, coeffs.ctypes.data,
                 float(object["sigma"]), pair_arr.ctypes.data, m, nd.ctypes.data, u, *vcov_args, vals.ctypes.data,
                 avg.ctypes.data, var.ctypes.data if var is not None else None)
    out = {"interactions": vals, "avginteractions": avg[None, :],
           "var.avginteractions": None if var is None else var[None, :],
           "pairs": ordered, "pairlabs": [f"{xlabs[j - 1]}:{xlabs[k - 1]}" for j, k in ordered],
           "binaryindicator": isbin[pair_arr - 1], "newdata": nd_init}
    if se:
        sev = np.empty((u, m), dtype=np.float64, order="F")
        _call_native("bigkrls_interaction_effects_se", ctx.handle, Xh.ctypes.data, n, p, yv.ctypes.data,
                     coeffs.ctypes.data, float(object["sigma"]), pair_arr.ctypes.data, m, nd.ctypes.data, u, *vcov_args,
                     int(_block_rows), sev.ctypes.data)
        out["se.interactions"] = sev
    return out


ROBUST_TYPES = {"classical": 0, "HC0": 1, "HC1": 2, "HC2": 3, "HC3": 4, "CR0": 1, "CR1": 2, "CR3": 5}


def _robust_plan(object, type, cluster):
    """Everything robust_vcov() decides before it touches the library: the validated inputs, the native type code, the
    scalar factor on the middle matrix, and the cluster labels mapped to 0 .. G - 1 (or None)."""
    if not isinstance(object, BigKRLS):
        raise TypeError("Object not of class 'bigKRLS'")
    if type not in ROBUST_TYPES:
        raise ValueError('type must be one of "classical", "HC0", "HC1", "HC2", "HC3", or "CR0", "CR1", "CR3" with '
                         'cluster')
    if object.get("vcov.est.Q") is None or object.get("vcov.est.w") is None:
        raise ValueError('the object has no vcov.est.Q / vcov.est.w: refit with vcov_form="factors" or "both"')
    clustered = type.startswith("CR")
    if clustered and cluster is None:
        raise ValueError(f'type="{type}" needs cluster (one label per row)')
    if cluster is not None and not clustered:
        raise ValueError(f'cluster goes with type="CR0", "CR1" or "CR3", not "{type}"')
    n = np.asarray(object["X"]).shape[0]
    k = len(np.asarray(object["vcov.est.w"]).ravel())
    d = np.asarray(object["K.eigenvalues"], dtype=np.float64).ravel()
    if tuple(getattr(object["vcov.est.Q"], "shape", ())) != (n, k):
        raise ValueError("vcov.est.Q must be nrow(X) x length(vcov.est.w)")
    if k < 1 or d.size < k:
        raise ValueError("the object's K.eigenvalues do not cover its vcov.est.w")
    for key in ("lambda", "y", "yfitted.std", "sigmasq", "Neffective"):
        if object.get(key) is None:
            raise ValueError(f"the object has no {key}")
    labels = G = None
    if clustered:
        labels, names = _unit_labels(cluster, n)             # any hashable labels, numbered in order of appearance
        G = len(names)
    if type == "classical":
        scale = float(object["sigmasq"])
    elif type == "HC1":
        scale = n / float(object["Neffective"])
    elif type == "CR1":
        scale = G / (G - 1.0)
    elif type == "CR3":
        scale = (G - 1.0) / G
    else:
        scale = 1.0
    yv = np.asarray(object["y"], dtype=np.float64).ravel()
    y_sd = _sd(yv)
    resid = np.ascontiguousarray((yv - yv.mean()) / y_sd - np.asarray(object["yfitted.std"], dtype=np.float64).ravel())
    return {"n": n, "k": k, "d": np.ascontiguousarray(d[:k]), "code": ROBUST_TYPES[type], "scale": float(scale),
            "labels": labels, "G": G, "y_sd": float(y_sd), "resid": resid}


def robust_vcov(object: BigKRLS, type: str = "HC1", cluster=None, ctx: Optional[Context] = None) -> BigKRLS:
    """Heteroskedasticity- or cluster-robust variance of the coefficients of a fitted model, without refitting and
    without an N x N matrix: a NEW object whose `vcov.est.Q` / `vcov.est.w` are the factors of the sandwich
    V_r = G diag(omega) G, G = Q diag(1 / (d + lambda)) Q' on the fit's kept eigenpairs, so that predict(se_pred=True),
    marginal_effects(), marginal_effects(se=True), partial_dependence(), summary() and save_bigKRLS() work from it as
    they do from a fit with vcov_form="factors". The input object is untouched. No counterpart in the reference.

    type: "classical" (omega = sigmasq: the fit's own variance, rotated), "HC0" (e_i^2), "HC1" (HC0 times
    N / Neffective, the package's degrees of freedom), "HC2" (e_i^2 / (1 - h_i)), "HC3" (e_i^2 / (1 - h_i)^2) with h the
    leverages of the smoother K (K + lambda I)^-1; "CR0" / "CR1" with `cluster` (N hashable labels, at least 2 distinct):
    the clustered middle sum_g s_g s_g', s_g the score sum of cluster g, CR1 times G / (G - 1); "CR3": the cluster jackknife,
    recommended when the clusters are few -- the same middle on the deletion residuals (I - H_SS)^-1 e_S of every
    cluster (see influence()), times (G - 1) / G.

    The object must carry the factors (a fit with vcov_form="factors" or "both"; kernel="implicit", Neig="auto" and
    multi-GPU objects do). The numeric body is ONE call into the C ABI, `bigkrls_vcov_robust`. In the result
    `vcov.est.c` and `vcov.est.fitted` are None: the identity vcov.est.fitted = Q diag(w d^2) Q' does not hold for the
    rotated factors, and standard errors of fitted values come from predict(obj, X, se_pred=True). `vcov.type` is the
    type, `vcov.clusters` the number of clusters or None; with derivatives in the object `var.avgderivatives` (and
    `.std`) are recomputed from the new factors, so summary() reports robust standard errors."""
    plan = _robust_plan(object, type, cluster)
    ctx = ctx or object.get("_ctx") or default_context()
    n, k = plan["n"], plan["k"]
    Qd, _ = _factors(object, ctx)                              # (raises unless Q is N x length(vcov.est.w))
    Qout = ctx.empty(n, k)
    wout = np.zeros(k)
    labels = plan["labels"]
    _call_native("bigkrls_vcov_robust", ctx.handle, n, k, Qd.ptr, Qd.ld, plan["d"].ctypes.data, float(object["lambda"]),
                 plan["resid"].ctypes.data, plan["y_sd"], plan["scale"], plan["code"],
                 labels.ctypes.data if labels is not None else None, plan["G"] or 0, Qout.ptr, Qout.ld,
                 wout.ctypes.data)
    out = BigKRLS(object)
    for key in ("vcov.est.c.cols", "vcov.est.fitted.cols", "path", "model_subfolder_name"):
        out.pop(key, None)
    out["vcov.est.Q"], out["vcov.est.w"] = Qout, wout
    if out.get("vcov.fit.Q") is None:                          # the fit's own eigenvectors (no copy): influence() needs them
        out["vcov.fit.Q"] = Qd
    out["vcov.est.c"] = out["vcov.est.fitted"] = None
    out["vcov.type"], out["vcov.clusters"] = type, plan["G"]
    out["_ctx"] = ctx
    if object.get("derivatives") is not None:
        me = marginal_effects(out, out["X"], ctx=ctx, vcov="factors")
        var = np.asarray(me["var.avgderivatives"], dtype=np.float64)
        out["var.avgderivatives"] = var
        if object.get("var.avgderivatives.std") is not None:  # standardised units: the fit's g = sd(y) / sd(x_j), var = g^2 var.std
            Xh = np.asarray(out["X"], dtype=np.float64)
            g = plan["y_sd"] / np.array([_sd(Xh[:, j - 1]) for j in me["which.derivatives"]])
            out["var.avgderivatives.std"] = var.ravel() / (g * g)
    return out


def _unit_labels(cluster, n):
    """cluster labels as _robust_plan maps them: any hashable labels numbered 0 .. G - 1 in order of appearance, at least
    2 distinct. Returns (labels int64, the distinct labels in that order)."""
    raw = list(cluster.tolist() if isinstance(cluster, np.ndarray) else cluster)
    if len(raw) != n:
        raise ValueError(f"cluster must have one label per row: {len(raw)} labels for N = {n}")
    index = {}
    labels = np.empty(n, dtype=np.int64)
    for i, lab in enumerate(raw):
        labels[i] = index.setdefault(lab, len(index))
    if len(index) < 2:
        raise ValueError("cluster must hold at least 2 distinct labels")
    return labels, list(index)


def _influence_plan(object, cluster, which_derivatives, newdata):
    """Everything influence() decides before it touches the library: the class check, the factors and what goes with them
    (robust_vcov's messages), the multi-GPU refusal, the units, the selected columns and newdata."""
    if not isinstance(object, BigKRLS):
        raise TypeError("Object not of class 'bigKRLS'")
    if object.get("vcov.est.Q") is None or object.get("vcov.est.w") is None:
        raise ValueError('the object has no vcov.est.Q / vcov.est.w: refit with vcov_form="factors" or "both"')
    if "vcov.est.c.cols" in object or "rows" in object:
        raise NotImplementedError("influence of a multi-GPU fit (sharded vcov.est.c.cols) is not supported; refit on one GPU")
    rotated = object.get("vcov.type") is not None        # a robust_vcov() object: vcov.est.Q is the fit's Q times a rotation
    Q = object.get("vcov.fit.Q") if rotated else object["vcov.est.Q"]
    if Q is None:
        raise ValueError("the object is a robust_vcov() result that no longer carries the fit's own eigenvectors "
                         "(vcov.fit.Q): call influence() on the fit it was made from")
    Xh = np.asfortranarray(np.asarray(object["X"], dtype=np.float64))
    n, p = Xh.shape
    k = len(np.asarray(object["vcov.est.w"]).ravel())
    d = np.asarray(object["K.eigenvalues"], dtype=np.float64).ravel()
    if tuple(getattr(Q, "shape", ())) != (n, k):
        raise ValueError("vcov.est.Q must be nrow(X) x length(vcov.est.w)")
    if k < 1 or d.size < k:
        raise ValueError("the object's K.eigenvalues do not cover its vcov.est.w")
    for key in ("lambda", "y", "yfitted.std", "coeffs", "sigma"):
        if object.get(key) is None:
            raise ValueError(f"the object has no {key}")
    labels = names = None
    if cluster is not None:
        labels, names = _unit_labels(cluster, n)
    if which_derivatives is None:
        which_derivatives = object.get("which.derivatives")
    if which_derivatives is None:
        which = list(range(1, p + 1))
    else:
        which = [int(i) for i in np.atleast_1d(which_derivatives)]
        if not which or not all(1 <= i <= p for i in which):
            raise ValueError("which.derivatives must index columns of X")
    nd = None
    if newdata is not None:
        nd = np.array(_as_host_matrix(newdata), dtype=np.float64, order="F")
        if nd.ndim != 2 or nd.shape[1] != p:
            raise ValueError("ncol(newdata) differs from ncol(X) from fitted bigKRLS object")
        if nd.shape[0] < 1:
            raise ValueError("newdata has no rows")
        if not np.all(np.isfinite(nd)):
            raise ValueError("newdata contains missing or infinite values")
        isbin = np.array([np.unique(Xh[:, j]).size == 2 for j in range(p)])
        _check_binary_newdata(Xh, nd, isbin, sorted(set(i - 1 for i in which)))
    yv = np.ascontiguousarray(np.asarray(object["y"], dtype=np.float64).ravel())
    resid = np.ascontiguousarray((yv - yv.mean()) / _sd(yv) - np.asarray(object["yfitted.std"], dtype=np.float64).ravel())
    return {"Q": Q, "Xh": Xh, "n": n, "p": p, "k": k, "d": np.ascontiguousarray(d[:k]), "labels": labels, "names": names,
            "G": None if labels is None else len(names), "which": which, "newdata": nd, "y": yv, "resid": resid}


def influence(object: BigKRLS, cluster=None, which_derivatives=None, newdata=None, ctx: Optional[Context] = None) -> dict:
    """Case- and cluster-deletion diagnostics of a fitted model, without refitting: which observations -- or, with
    `cluster` (N hashable labels, at least 2 distinct), which clusters -- the result rests on. A unit is one observation,
    or one cluster. Deleting a unit HOLDS THE BASIS (the kept eigenvectors of the full kernel), sigma, lambda AND THE
    STANDARDISATION AT THEIR FULL-SAMPLE VALUES: with every eigenpair kept that is the refit on the remaining rows at the
    same lambda; with a truncated basis it is the penalised least-squares refit on the same basis. The closed form is
    et_S = (I - H_SS)^-1 e_S on the smoother H = Q diag(d / (d + lambda)) Q', one small system per unit, solved on the GPU
    (`bigkrls_dev_deletion_residuals`); the numeric body is ONE call into the C ABI, `bigkrls_influence`. No counterpart
    in the reference.

    Returns a dict: "hat" (N leverages), "resid.deleted" and "fitted.deleted" (N: y minus / the prediction of every row
    by the fit without its unit), "cooks" (U: ||yhat - yhat(-u)||^2 / (tr(H) e'e / (N - tr(H))) in standardised units),
    "dfame" (U x |J|: AME_j of the full fit minus AME_j without unit u, in marginal_effects' units, on `newdata` --
    default the training rows), "ame" (1 x |J|), "var.avgderivatives.jack" (1 x |J|: ((U - 1) / U) sum_u dfame^2, the
    jackknife variance, times the reference's factor 2 for a binary column as in every var.avgderivatives; with clusters
    it equals robust_vcov(type="CR3")'s var.avgderivatives), "R2.loo"
    (1 - sum et^2 / sum ys^2), "units" (U), "unit.labels" (the distinct labels in order of appearance, or None),
    "unit.sizes" and "which.derivatives".

    The object must carry the factors (vcov_form="factors" or "both"; kernel="implicit" and Neig="auto" objects do). A
    robust_vcov() object is accepted and uses the fit's ORIGINAL eigenvectors, which it carries as `vcov.fit.Q`. A
    multi-GPU sharded object is refused. A unit whose block leverage reaches 1 raises a ValueError naming it."""
    plan = _influence_plan(object, cluster, which_derivatives, newdata)
    ctx = ctx or object.get("_ctx") or default_context()
    n, p, k, G = plan["n"], plan["p"], plan["k"], plan["G"]
    Q = plan["Q"]
    Qd = Q if is_device_matrix(Q) else ctx.from_numpy(np.asarray(Q, dtype=np.float64))
    U = n if G is None else G
    which_arr = np.ascontiguousarray(plan["which"], dtype=np.int64)
    nj = which_arr.size
    nd, labels = plan["newdata"], plan["labels"]
    coeffs = np.ascontiguousarray(np.asarray(object["coeffs"], dtype=np.float64).ravel())
    hat, rdel, fdel, cooks = np.empty(n), np.empty(n), np.empty(n), np.empty(U)
    dfame = np.empty((U, nj), dtype=np.float64, order="F")
    ame, vjack, r2 = np.empty(nj), np.empty(nj), np.empty(1)
    _call_native("bigkrls_influence", ctx.handle, plan["Xh"].ctypes.data, n, p, plan["y"].ctypes.data, coeffs.ctypes.data,
                 float(object["sigma"]), which_arr.ctypes.data, nj, nd.ctypes.data if nd is not None else None,
                 nd.shape[0] if nd is not None else n, Qd.ptr, Qd.ld, k, plan["d"].ctypes.data, float(object["lambda"]),
                 plan["resid"].ctypes.data, labels.ctypes.data if labels is not None else None, G or 0,
                 hat.ctypes.data, rdel.ctypes.data, fdel.ctypes.data, cooks.ctypes.data, dfame.ctypes.data,
                 ame.ctypes.data, vjack.ctypes.data, r2.ctypes.data)
    sizes = np.ones(n, dtype=np.int64) if labels is None else np.bincount(labels, minlength=G).astype(np.int64)
    return {"hat": hat, "resid.deleted": rdel, "fitted.deleted": fdel, "cooks": cooks, "dfame": dfame, "ame": ame[None, :],
            "var.avgderivatives.jack": vjack[None, :], "R2.loo": float(r2[0]), "units": U, "unit.labels": plan["names"],
            "unit.sizes": sizes, "which.derivatives": plan["which"]}


def partial_dependence(object: BigKRLS, which=None, grid=20, newdata=None, se: bool = True, correct_SE: bool = True,
                       vcov: Optional[str] = None, ctx: Optional[Context] = None) -> dict:
    """Partial dependence of the fitted outcome on one predictor at a time: for every column j of `which` (1-based;
    default: the object's which.derivatives, else all columns) and every grid value v, the mean over the reference rows
    of the prediction with x_j set to v, with its standard error -- the curve of the expected outcome against x_j and its
    confidence band. For a binary training column the grid is exactly its two training values (lo, hi), and
    "first.difference" / "se.first.difference" are pd(hi) - pd(lo) and its standard error. No counterpart in the
    reference. The numeric body is ONE call into the C ABI, `bigkrls_partial_dependence`: the Gaussian kernel factorises
    over the columns, so all curves come from one fused O(u n) pass (`bigkrls_dev_kernel_loo_colsums`) instead of one
    predict() on u rewritten rows per grid value; neither a u x n nor a u x u matrix is formed.

    grid: an int G >= 2 (np.linspace(min, max, G) of the training column) or a list of arrays aligned with `which`; an
    explicit grid for a binary column must hold its two training values only. newdata: the reference rows (u x p,
    standardised with the training moments); None: the training rows. Column j of them is never read for column j's
    curve. se / vcov: as in marginal_effects(); correct_SE: as in predict(). Returns a dict: "which", "xlabs",
    "binaryindicator", "grid", "pd", "se.pd", "vcov.pd" (lists over the columns; the last two None without a variance),
    "first.difference", "se.first.difference" (1 x |J|, NaN for continuous columns; the second None without a
    variance) and "newdata"."""
    # (the multi-GPU refusal has always named marginal_effects here)
    Xh, n, p, nd_init, nd, u, isbin, form = _effects_open("marginal_effects", object, newdata, vcov, se, gated=True,
                                                         default="null")
    if which is None:
        which = object.get("which.derivatives")
    if which is None:
        which = list(range(1, p + 1))
    else:
        which = [int(i) for i in np.atleast_1d(which)]
        if not which or not all(1 <= i <= p for i in which):
            raise ValueError("which.derivatives must index columns of X")
    explicit = not isinstance(grid, (int, np.integer))
    if explicit:
        grid = list(grid)
        if len(grid) != len(which):
            raise ValueError("grid must be an integer or a list with one array per column of which")
    elif grid < 2:
        raise ValueError("grid must be at least 2")
    grids = []
    for idx, i in enumerate(which):
        j = i - 1
        lo, hi = Xh[:, j].min(), Xh[:, j].max()
        if explicit:
            g = np.ascontiguousarray(np.asarray(grid[idx], dtype=np.float64).ravel())
            if g.size < 1 or not np.all(np.isfinite(g)):
                raise ValueError(f"the grid of column {i} must hold at least one finite value")
            if isbin[j] and not np.all((g == lo) | (g == hi)):
                raise ValueError(f"grid column {i} is binary in the training data; its values must be "
                                 f"one of the two training values ({lo:g}, {hi:g})")
        if isbin[j]:
            g = np.array([lo, hi])
        elif not explicit:
            g = np.linspace(lo, hi, int(grid))
        grids.append(g)
    ctx, Vd, Qd, wv, yv, coeffs, vcov_args, xlabs = _effects_device(object, form, ctx, p)
    which_arr = np.ascontiguousarray(which, dtype=np.int64)
    nj = which_arr.size
    sizes = np.array([g.size for g in grids], dtype=np.int64)
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)]), dtype=np.int64)
    cov_off = np.concatenate([[0], np.cumsum(sizes * sizes)])
    flat = np.ascontiguousarray(np.concatenate(grids))
    total = int(off[-1])
    pd = np.empty(total)
    sev = np.empty(total) if se else None
    cov = np.empty(int(cov_off[-1])) if se else None
    neff = -1.0
    if se and correct_SE and object.get("Neffective") is not None:                # predict(): R/bigKRLS.R:610-611
        neff = float(object["Neffective"])
    _call_native("bigkrls_partial_dependence", ctx.handle, Xh.ctypes.data, n, p, yv.ctypes.data, coeffs.ctypes.data,
                 float(object["sigma"]), which_arr.ctypes.data, nj, nd.ctypes.data if nd is not None else None, u,
                 flat.ctypes.data, off.ctypes.data, *vcov_args, neff, pd.ctypes.data,
                 sev.ctypes.data if se else None, cov.ctypes.data if se else None)
    cut = lambda v: [v[off[i]:off[i + 1]] for i in range(nj)]
    covs = None
    if se:
        covs = [cov[cov_off[i]:cov_off[i + 1]].reshape(sizes[i], sizes[i], order="F") for i in range(nj)]
    bin_sel = isbin[which_arr - 1]
    fd = np.full((1, nj), np.nan)
    sefd = np.full((1, nj), np.nan) if se else None
    for i in range(nj):
        if bin_sel[i]:
            fd[0, i] = pd[off[i] + 1] - pd[off[i]]
            if se:
                c = covs[i]
                sefd[0, i] = np.sqrt(max(c[0, 0] + c[1, 1] - 2.0 * c[0, 1], 0.0))
    return {"which": which, "xlabs": [xlabs[i - 1] for i in which], "binaryindicator": bin_sel, "grid": grids,
            "pd": cut(pd), "se.pd": cut(sev) if se else None, "vcov.pd": covs, "first.difference": fd,
            "se.first.difference": sefd, "newdata": nd_init}


def _ale_bins(z, edges):
    """The bin of every reference value z under the edges z_0 < ... < z_B: b(i) = the smallest b >= 1 with z <= z_b (a row
    equal to z_0 goes to bin 1), 0-based; and the rows per bin."""
    lab = np.maximum(np.searchsorted(edges, z, side="left"), 1) - 1
    return lab, np.bincount(lab, minlength=edges.size - 1)


def accumulated_effects(object: BigKRLS, which=None, bins=20, newdata=None, se: bool = True, correct_SE: bool = True,
                        vcov: Optional[str] = None, ctx: Optional[Context] = None) -> dict:
    """Accumulated local effects (ALE, Apley & Zhu) of the fitted outcome on one predictor at a time, with standard
    errors: for every column j of `which` (1-based; default: the object's which.derivatives, else all columns) and every
    bin of x_j, the mean change of the prediction over the reference rows that fall into the bin when x_j moves from
    the bin's lower to its upper edge ("local"), accumulated over the bins and centred ("ale", at the edges). Unlike
    partial_dependence() no prediction is taken at a combination of values the data do not contain, which matters with
    correlated predictors. No counterpart in the reference. The numeric body is ONE call into the C ABI,
    `bigkrls_accumulated_effects`: the Gaussian kernel factorises over the columns, so all curves are linear in the
    coefficients and come, with their covariance, from one fused O(u n) pass (`bigkrls_dev_kernel_loo_binsums`) instead of
    two predict() calls per bin.

    bins: an int B >= 1 -- the edges are the distinct inverted-CDF quantiles of the reference column at k/B, k = 0..B, so
    every edge is a sample value, no bin is empty and ties merge bins -- or a list of edge arrays aligned with `which`
    (strictly increasing, covering the reference column, no bin empty). A binary training column has one bin between its
    two training values (lo, hi): ale = (-d/2, +d/2) with d = partial_dependence()'s "first.difference"; explicit edges
    for it must be those two values. newdata: the reference rows (u x p); None: the training rows. se / vcov: as in
    marginal_effects(); correct_SE: as in predict(). Returns a dict: "which", "xlabs", "binaryindicator", "edges",
    "counts" (rows per bin), "ale", "se.ale", "vcov.ale" (lists over the columns, at the edges; the last two None without
    a variance), "local", "se.local" (per bin: the differences of "ale" and their standard errors from "vcov.ale"),
    "first.difference", "se.first.difference" (1 x |J|, NaN for continuous columns) and "newdata"."""
    Xh, n, p, nd_init, nd, u, isbin, form = _effects_open("accumulated_effects", object, newdata, vcov, se, gated=True,
                                                         default="null")
    if which is None:
        which = object.get("which.derivatives")
    if which is None:
        which = list(range(1, p + 1))
    else:
        which = [int(i) for i in np.atleast_1d(which)]
        if not which or not all(1 <= i <= p for i in which):
            raise ValueError("which.derivatives must index columns of X")
    explicit = not isinstance(bins, (int, np.integer)) or isinstance(bins, (bool, np.bool_))
    if explicit:
        try:
            bins = [np.asarray(e, dtype=np.float64) for e in bins]
        except (TypeError, ValueError):
            bins = None
        if isinstance(bins, list) and any(e.ndim == 0 for e in bins):
            bins = None
        if bins is None or len(bins) != len(which):
            raise ValueError("bins must be an integer or a list with one array of edges per column of which")
    elif bins < 1:
        raise ValueError("bins must be at least 1")
    ref = Xh if nd is None else nd
    edges, counts = [], []
    for idx, i in enumerate(which):
        j = i - 1
        z = ref[:, j]
        lo, hi = Xh[:, j].min(), Xh[:, j].max()
        if explicit:
            e = np.ascontiguousarray(np.asarray(bins[idx], dtype=np.float64).ravel())
            if e.size < 2:
                raise ValueError(f"the edges of column {i} must hold at least 2 values")
            if not np.all(np.isfinite(e)):
                raise ValueError(f"the edges of column {i} contain missing or infinite values")
            if not np.all(np.diff(e) > 0):
                raise ValueError(f"the edges of column {i} must be strictly increasing")
            if isbin[j] and not (e.size == 2 and e[0] == lo and e[1] == hi):
                raise ValueError(f"column {i} is binary in the training data; its edges must be "
                                 f"its two training values ({lo:g}, {hi:g})")
        if isbin[j]:
            e = np.array([lo, hi])
        else:
            if np.unique(z).size < 2:
                raise ValueError(f"the reference rows hold one distinct value in column {i}: no accumulated effect")
            if not explicit:
                e = np.unique(np.quantile(z, np.arange(int(bins) + 1) / int(bins), method="inverted_cdf"))
        if z.min() < e[0] or z.max() > e[-1]:
            raise ValueError(f"the edges of column {i} do not cover the reference rows: [{e[0]:g}, {e[-1]:g}] against "
                             f"[{z.min():g}, {z.max():g}]")
        _, cnt = _ale_bins(z, e)
        if np.any(cnt == 0):
            raise ValueError(f"bin {int(np.argmin(cnt != 0)) + 1} of column {i} holds no reference row")
        edges.append(e)
        counts.append(cnt)
    ctx, Vd, Qd, wv, yv, coeffs, vcov_args, xlabs = _effects_device(object, form, ctx, p)
    which_arr = np.ascontiguousarray(which, dtype=np.int64)
    nj = which_arr.size
    sizes = np.array([e.size for e in edges], dtype=np.int64)
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)]), dtype=np.int64)
    cov_off = np.concatenate([[0], np.cumsum(sizes * sizes)])
    flat = np.ascontiguousarray(np.concatenate(edges))
    total = int(off[-1])
    ale = np.empty(total)
    sev = np.empty(total) if se else None
    cov = np.empty(int(cov_off[-1])) if se else None
    neff = -1.0
    if se and correct_SE and object.get("Neffective") is not None:                # predict(): R/bigKRLS.R:610-611
        neff = float(object["Neffective"])
    _call_native("bigkrls_accumulated_effects", ctx.handle, Xh.ctypes.data, n, p, yv.ctypes.data, coeffs.ctypes.data,
                 float(object["sigma"]), which_arr.ctypes.data, nj, nd.ctypes.data if nd is not None else None, u,
                 flat.ctypes.data, off.ctypes.data, *vcov_args, neff, ale.ctypes.data,
                 sev.ctypes.data if se else None, cov.ctypes.data if se else None)
    cut = lambda v: [v[off[i]:off[i + 1]] for i in range(nj)]
    ales = cut(ale)
    covs = None
    if se:
        covs = [cov[cov_off[i]:cov_off[i + 1]].reshape(sizes[i], sizes[i], order="F") for i in range(nj)]
    local = [np.diff(a) for a in ales]
    selocal = None
    if se:                                                                        # var(ale_b - ale_{b-1}) from vcov.ale
        selocal = []
        for c in covs:
            d = np.diag(c)
            selocal.append(np.sqrt(np.maximum(d[1:] + d[:-1] - 2.0 * np.diag(c, 1), 0.0)))
    bin_sel = isbin[which_arr - 1]
    fd = np.full((1, nj), np.nan)
    sefd = np.full((1, nj), np.nan) if se else None
    for i in range(nj):
        if bin_sel[i]:
            fd[0, i] = local[i][0]
            if se:
                sefd[0, i] = selocal[i][0]
    return {"which": which, "xlabs": [xlabs[i - 1] for i in which], "binaryindicator": bin_sel, "edges": edges,
            "counts": counts, "ale": ales, "se.ale": cut(sev) if se else None, "vcov.ale": covs, "local": local,
            "se.local": selocal, "first.difference": fd, "se.first.difference": sefd, "newdata": nd_init}


def _shapley_background(n: int, B: int):
    """The deterministic background rule: 0-based training rows floor((2k + 1) n / (2B)), k = 0 .. B-1 -- the midpoints of
    B equal slices of the row order, no random numbers; every row when B >= n."""
    B = int(B)
    if B >= n:
        return np.arange(n, dtype=np.int64)
    return ((2 * np.arange(B, dtype=np.int64) + 1) * n) // (2 * B)


def _shapley_players(groups, p: int):
    """(labels, players) from `groups`: labels[l] in [0, M) is the player of column l (0-based), players the list of the
    players' 1-based column lists. None: one player per column. A list of lists of 1-based columns: each list is one
    player, in the order given, and every unlisted column a player of its own behind them, in column order. A length-p
    vector of labels (anything hashable): the players in the order of their first column."""
    if groups is None:
        return np.arange(p, dtype=np.int64), [[l + 1] for l in range(p)]
    groups = list(groups)
    nested = len(groups) > 0 and all(isinstance(g, (list, tuple, np.ndarray)) for g in groups)
    labels = np.full(p, -1, dtype=np.int64)
    if nested:
        for m, g in enumerate(groups):
            cols = [int(c) for c in np.atleast_1d(np.asarray(g)).ravel()]
            if not cols:
                raise ValueError(f"groups: group {m + 1} is empty")
            for c in cols:
                if not 1 <= c <= p:
                    raise ValueError(f"groups: column {c} of group {m + 1} is outside 1..{p}")
                if labels[c - 1] != -1:
                    raise ValueError(f"groups: column {c} is listed more than once")
                labels[c - 1] = m
        nxt = len(groups)
        for l in range(p):
            if labels[l] == -1:
                labels[l] = nxt
                nxt += 1
    else:
        if len(groups) != p:
            raise ValueError(f"groups must be a list of column lists or a vector of {p} labels")
        seen = {}
        for l, g in enumerate(groups):
            g = g.item() if isinstance(g, np.generic) else g
            labels[l] = seen.setdefault(g, len(seen))
    M = int(labels.max()) + 1
    return labels, [[int(l) + 1 for l in np.flatnonzero(labels == m)] for m in range(M)]


SHAPLEY_MAX_PLAYERS = 128


def shapley_effects(object: BigKRLS, newdata=None, background=100, groups=None, se: bool = False,
                    correct_SE: bool = True, vcov: Optional[str] = None, block_rows: int = 0,
                    ctx: Optional[Context] = None) -> dict:
    """How much of one row's prediction is due to each predictor: exact interventional Shapley values of the fitted
    prediction, with standard errors. For a generic model they cost 2^P predictions per row; the Gaussian kernel
    factorises over the columns, so here they are exact and cheap -- one fused O(u n B) pass
    (`bigkrls_dev_shapley_weights`) -- and linear in the coefficients, which gives their standard errors from either form of
    vcov.est.c. No counterpart in the reference. The numeric body is ONE call into the C ABI, `bigkrls_shapley_effects`;
    the kernel matrix is never needed, so implicit fits work unchanged.

    The value of a coalition S at row x is the mean, over the background rows b, of the prediction at "x on the columns of
    the players in S, b elsewhere"; "shapley"[r, m] is player m's Shapley value in that game, in the units of y, and
    rowsum("shapley") + "baseline" = predict(newdata) with "baseline" = the mean prediction at the background rows.

    newdata: the explained rows (u x p); None: the training rows. background: an int B -- the training rows
    floor((2k + 1) n / (2B)), k = 0 .. B-1, 0-based (deterministic, no random numbers; all rows when B >= n) -- or a B x p
    array used as given. groups: None -- one player per column; a list of lists of 1-based columns -- each list is one
    player (a set of dummies counts as one feature), every unlisted column a player of its own behind them; or a length-p
    vector of labels. At most 128 players. se / vcov: as in marginal_effects(); correct_SE: as in predict(). The standard
    errors are conditional on X and on the background rows. block_rows: explained rows per block of the weight matrix
    (0: as many as fit 1 GiB).

    Returns a dict: "shapley" (u x M), "se.shapley" (u x M or None), "baseline", "predicted" (u: baseline + the row sums),
    "importance" (1 x M, the mean over the rows of |shapley|), "players" (the players' 1-based column lists), "xlabs" (a
    group is labelled by its columns' labels joined with "+"), "background" (B x p) and "newdata"."""
    Xh, n, p, nd_init, nd, u, isbin, form = _effects_open("shapley_effects", object, newdata, vcov, se, gated=True,
                                                         default="training")
    labels, players = _shapley_players(groups, p)
    M = len(players)
    if M > SHAPLEY_MAX_PLAYERS:
        raise ValueError(f"groups: {M} players; at most {SHAPLEY_MAX_PLAYERS} are supported -- group columns "
                         "(e.g. a set of dummies) into one player")
    if isinstance(background, (int, np.integer)) and not isinstance(background, (bool, np.bool_)):
        if background < 1:
            raise ValueError("background must be at least 1")
        bg = np.asfortranarray(Xh[_shapley_background(n, int(background))])
    else:
        bg = np.array(_as_host_matrix(background), dtype=np.float64, order="F")
        if bg.ndim != 2 or bg.shape[1] != p:
            raise ValueError("ncol(background) differs from ncol(X) from fitted bigKRLS object")
        if bg.shape[0] < 1:
            raise ValueError("background has no rows")
        if not np.all(np.isfinite(bg)):
            raise ValueError("background contains missing or infinite values")
    B = bg.shape[0]
    block_rows = int(block_rows)
    if block_rows < 0:
        raise ValueError("block_rows must not be negative")
    ctx, Vd, Qd, wv, yv, coeffs, vcov_args, xlabs = _effects_device(object, form, ctx, p)
    phi = np.empty((u, M))
    sev = np.empty((u, M)) if se else None
    base = np.empty(1)
    neff = -1.0
    if se and correct_SE and object.get("Neffective") is not None:                # predict(): R/bigKRLS.R:610-611
        neff = float(object["Neffective"])
    _call_native("bigkrls_shapley_effects", ctx.handle, Xh.ctypes.data, n, p, yv.ctypes.data, coeffs.ctypes.data,
                 float(object["sigma"]), labels.ctypes.data, M, nd.ctypes.data if newdata is not None else None, u,
                 bg.ctypes.data, B, *vcov_args, neff, block_rows, phi.ctypes.data, sev.ctypes.data if se else None,
                 base.ctypes.data)
    baseline = float(base[0])
    return {"shapley": phi, "se.shapley": sev, "baseline": baseline, "predicted": baseline + phi.sum(axis=1),
            "importance": np.abs(phi).mean(axis=0, keepdims=True), "players": players,
            "xlabs": ["+".join(xlabs[c - 1] for c in cols) for cols in players], "background": bg, "newdata": nd_init}


def conditional_effects(object: BigKRLS, effect, along, grid=20, newdata=None, se: bool = True,
                        vcov: Optional[str] = None, ctx: Optional[Context] = None) -> dict:
    """Marginal effects along a moderator: how does the effect of x_j change with x_k? For every pair (j, k) of `effect`
    x `along` (1-based ints or lists; all combinations) and every grid value v of x_k, the mean over the reference rows
    of the marginal effect of x_j evaluated with x_k set to v -- the derivative for a continuous x_j (k == j: the slope
    of the partial-dependence curve), the first difference between its two training values for a binary x_j -- with its
    standard error and the covariance over the grid: the curve, its confidence band, and a test of "is the effect at
    high x_k different from the effect at low x_k" ("contrast"). For every pair and every v the value and variance are
    `avgderivatives` and `var.avgderivatives` of marginal_effects() on the reference rows with column k set to v, in its
    units and with its factor 2 on the variances of a binary x_j. No counterpart in the reference. The numeric body is
    ONE call into the C ABI, `bigkrls_conditional_effects`: the Gaussian kernel factorises over the columns, so all
    curves come from one fused O(u n) pass (`bigkrls_dev_kernel_loo_moments`) instead of one marginal_effects() on u
    rewritten rows per grid value.

    grid: an int G >= 2 (np.linspace(min, max, G) of the moderator's training column) or a list with one array per
    pair; a binary moderator always gets its two training values, and an explicit grid for it must hold only those.
    newdata: the reference rows (u x p); None: the training rows. Column k of them is never read, nor column j for a
    binary x_j. A pair (j, j) on a binary column is not defined. se / vcov and the multi-GPU rule: as in
    marginal_effects() and partial_dependence(). Returns a dict: "pairs", "xlabs" (pairs of labels), "binary.effect",
    "binary.moderator", "grid", "ce", "se.ce", "vcov.ce" (lists over the pairs; the last two None without a variance),
    "contrast" = ce(last grid value) - ce(first) and "se.contrast" from the covariance (1 x m; the second None without a
    variance), and "newdata"."""
    Xh, n, p, nd_init, nd, u, isbin, form = _effects_open("conditional_effects", object, newdata, vcov, se, gated=True,
                                                         default="null")

    def columns(arg, name):
        try:
            cols = [int(i) for i in np.atleast_1d(arg)]
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a column index or a list of column indices") from None
        if not cols or not all(1 <= i <= p for i in cols):
            raise ValueError(f"{name} must index columns of X")
        return cols
    effects, alongs = columns(effect, "effect"), columns(along, "along")
    pairs = []
    for j in effects:
        for k in alongs:
            if j == k and isbin[j - 1]:
                raise ValueError(f"pair ({j}, {k}) is not defined: column {j} is binary in the training data")
            if (j, k) in pairs:
                raise ValueError(f"pair ({j}, {k}) is given more than once")
            pairs.append((j, k))
    explicit = not isinstance(grid, (int, np.integer))
    if explicit:
        grid = list(grid)
        if len(grid) != len(pairs):
            raise ValueError("grid must be an integer or a list with one array per pair (effect x along)")
    elif grid < 2:
        raise ValueError("grid must be at least 2")
    grids = []
    for idx, (j, k) in enumerate(pairs):
        lo, hi = Xh[:, k - 1].min(), Xh[:, k - 1].max()
        if explicit:
            g = np.ascontiguousarray(np.asarray(grid[idx], dtype=np.float64).ravel())
            if g.size < 1 or not np.all(np.isfinite(g)):
                raise ValueError(f"the grid of pair ({j}, {k}) must hold at least one finite value")
            if isbin[k - 1] and not np.all((g == lo) | (g == hi)):
                raise ValueError(f"the grid of pair ({j}, {k}): column {k} is binary in the training data; its values "
                                 f"must be one of the two training values ({lo:g}, {hi:g})")
        if isbin[k - 1]:
            g = np.array([lo, hi])
        elif not explicit:
            g = np.linspace(lo, hi, int(grid))
        grids.append(g)
    ctx, Vd, Qd, wv, yv, coeffs, vcov_args, xlabs = _effects_device(object, form, ctx, p)
    pair_arr = np.ascontiguousarray(pairs, dtype=np.int64)                        # m x 2 row-major: pair after pair
    m = len(pairs)
    sizes = np.array([g.size for g in grids], dtype=np.int64)
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)]), dtype=np.int64)
    cov_off = np.concatenate([[0], np.cumsum(sizes * sizes)])
    flat = np.ascontiguousarray(np.concatenate(grids))
    total = int(off[-1])
    ce = np.empty(total)
    sev = np.empty(total) if se else None
    cov = np.empty(int(cov_off[-1])) if se else None
    _call_native("bigkrls_conditional_effects", ctx.handle, Xh.ctypes.data, n, p, yv.ctypes.data, coeffs.ctypes.data,
                 float(object["sigma"]), pair_arr.ctypes.data, m, nd.ctypes.data if nd is not None else None, u,
                 flat.ctypes.data, off.ctypes.data, *vcov_args, ce.ctypes.data,
                 sev.ctypes.data if se else None, cov.ctypes.data if se else None)
    cut = lambda v: [v[off[i]:off[i + 1]] for i in range(m)]
    covs = None
    if se:
        covs = [cov[cov_off[i]:cov_off[i + 1]].reshape(sizes[i], sizes[i], order="F") for i in range(m)]
    contrast = np.array([[ce[off[i + 1] - 1] - ce[off[i]] for i in range(m)]])
    secon = None
    if se:
        secon = np.array([[np.sqrt(max(c[0, 0] + c[-1, -1] - 2.0 * c[0, -1], 0.0)) for c in covs]])
    return {"pairs": pairs, "xlabs": [(xlabs[j - 1], xlabs[k - 1]) for j, k in pairs],
            "binary.effect": isbin[pair_arr[:, 0] - 1], "binary.moderator": isbin[pair_arr[:, 1] - 1], "grid": grids,
            "ce": cut(ce), "se.ce": cut(sev) if se else None, "vcov.ce": covs, "contrast": contrast,
            "se.contrast": secon, "newdata": nd_init}


def _group_labels(by, nd, bins):
    """(groups, labels) of group_effects(): `by` as u labels (groups = np.unique(by)), or as a 1-based column index of nd:
    the column's distinct values, or with bins=B its quantile bins
    np.digitize(col, np.quantile(col, np.linspace(0, 1, B + 1))[1:-1], right=True), empty bins dropped, reported by their
    (lo, hi] edges. labels: int64 indices into groups. Host only."""
    u, p = nd.shape
    if isinstance(by, (int, np.integer)) and not isinstance(by, (bool, np.bool_)):
        if not 1 <= int(by) <= p:
            raise ValueError("by must index a column of newdata (1-based) or hold one label per row")
        col = nd[:, int(by) - 1]
        if bins is None:
            groups, labels = np.unique(col, return_inverse=True)
            return list(groups), np.ascontiguousarray(labels.ravel(), dtype=np.int64)
        if not isinstance(bins, (int, np.integer)) or isinstance(bins, (bool, np.bool_)) or bins < 1:
            raise ValueError("bins must be a positive integer")
        edges = np.quantile(col, np.linspace(0.0, 1.0, int(bins) + 1))
        raw = np.digitize(col, edges[1:-1], right=True)
        used, labels = np.unique(raw, return_inverse=True)
        groups = [(float(edges[b]), float(edges[b + 1])) for b in used]
        return groups, np.ascontiguousarray(labels.ravel(), dtype=np.int64)
    if bins is not None:
        raise ValueError("bins applies only when by is a column index")
    arr = np.asarray(by)
    if arr.ndim == 2 and 1 in arr.shape:
        arr = arr.ravel()
    if arr.ndim != 1 or arr.size != u:
        raise ValueError(f"by must hold one label per row of newdata ({u}); it has shape {np.asarray(by).shape}")
    groups, labels = np.unique(arr, return_inverse=True)
    return list(groups), np.ascontiguousarray(labels.ravel(), dtype=np.int64)


def group_effects(object: BigKRLS, by, newdata=None, which_derivatives=None, bins=None, reference=None,
                  vcov: Optional[str] = None, ctx: Optional[Context] = None) -> dict:
    """Average marginal effects by subgroup, with their joint covariance and a test of heterogeneity: does the effect of
    x_j differ between the groups of the rows actually observed? For every group g of `by` and every selected column j,
    "ame"[g, j] is the mean of marginal_effects()'s derivatives over the rows of the group; "vcov.ame" is the joint
    covariance of all of them (index jj * G + g: the groups of one variable are adjacent), so that differences between
    groups and joint statements over several variables have standard errors. Every diagonal entry is
    marginal_effects(object, newdata[rows of g])["var.avgderivatives"], binary columns with the reference's factor 2
    (carried as sqrt(2) per side off the diagonal, which keeps the matrix positive semi-definite). No counterpart in
    the reference. The numeric body is ONE call into the C ABI, `bigkrls_group_effects`: the column side of all groups
    comes from one grouped fused contraction (`bigkrls_dev_kernel_contract_grouped`) and the covariance from the factors
    of vcov.est.c (or the matrix) on the device; nothing N x N reaches the host.

    newdata defaults to the training X. by: one label per row (any sortable dtype; the groups are np.unique(by)), or a
    1-based column index of newdata: its distinct values, or with bins=B its B quantile bins (empty bins dropped;
    "groups" then holds the (lo, hi] edges). reference: a group label (default: the first group). which_derivatives,
    vcov and the multi-GPU rule: as in marginal_effects(). G * |J| may be at most 4096.

    Returns a dict: "groups", "n" (rows per group), "ame" (G x |J|), "se.ame", "vcov.ame", "diff" and "se.diff" (each
    group minus the reference, per variable; the reference row is 0), "wald" = {"statistic", "df", "p"} (each of length
    |J|; H0: the group AMEs of x_j are all equal, see _wald; G = 1 gives 0, 0, nan), "reference", "derivatives" (u x |J|),
    "which.derivatives", "binaryindicator", "xlabs", "newdata". Without a variance form on the object "se.ame",
    "vcov.ame", "se.diff" and "wald" are None."""
    Xh, n, p, nd_init, nd, u, isbin, form = _effects_open("group_effects", object, newdata, vcov, False,
                                                         default="training")
    if which_derivatives is None:
        which_derivatives = object.get("which.derivatives")
    if which_derivatives is None:
        which = list(range(1, p + 1))
    else:
        which = [int(i) for i in np.atleast_1d(which_derivatives)]
        if not which or not all(1 <= i <= p for i in which):
            raise ValueError("which.derivatives must index columns of X")
    _check_binary_newdata(Xh, nd, isbin, sorted(set(i - 1 for i in which)))
    groups, labels = _group_labels(by, nd, bins)
    G, nj = len(groups), len(which)
    if G < 1:
        raise ValueError("by gives no group")
    if reference is None:
        ref = 0
    else:
        hits = [i for i, g in enumerate(groups)
                if np.shape(g) == np.shape(reference) and bool(np.all(np.asarray(g) == np.asarray(reference)))]
        if not hits:
            raise ValueError(f"reference {reference!r} is not one of the groups {groups!r}")
        ref = hits[0]
    if G * nj > 4096:
        raise ValueError(f"{G} groups x {nj} columns = {G * nj} average effects: the covariance is (G |J|)^2 doubles on "
                         "the host and G |J| may be at most 4096; use fewer groups (bins=) or which_derivatives")
    ctx, Vd, Qd, wv, yv, coeffs, vcov_args, xlabs = _effects_device(object, form, ctx, p)
    which_arr = np.ascontiguousarray(which, dtype=np.int64)
    D = np.empty((u, nj), dtype=np.float64, order="F")
    ame = np.empty((G, nj), dtype=np.float64, order="F")
    cov = np.empty((G * nj, G * nj), dtype=np.float64, order="F") if form is not None else None
    _call_native("bigkrls_group_effects", ctx.handle, Xh.ctypes.data, n, p, yv.ctypes.data, coeffs.ctypes.data,
                 float(object["sigma"]), which_arr.ctypes.data, nj, nd.ctypes.data, u, labels.ctypes.data, G,
                 *vcov_args, D.ctypes.data, ame.ctypes.data,
                 cov.ctypes.data if cov is not None else None)
    diff = ame - ame[ref:ref + 1, :]
    se_ame = se_diff = wald = None
    if cov is not None:
        se_ame = np.sqrt(np.maximum(np.diag(cov), 0.0)).reshape(nj, G).T
        se_diff = np.zeros((G, nj))
        stats, dfs, ps = np.zeros(nj), np.zeros(nj, dtype=np.int64), np.full(nj, np.nan)
        for jj in range(nj):
            Sj = cov[jj * G:(jj + 1) * G, jj * G:(jj + 1) * G]
            se_diff[:, jj] = np.sqrt(np.maximum(np.diag(Sj) + Sj[ref, ref] - 2.0 * Sj[:, ref], 0.0))
            se_diff[ref, jj] = 0.0
            stats[jj], dfs[jj], ps[jj] = _wald(ame[:, jj], Sj, ref)
        wald = {"statistic": stats, "df": dfs, "p": ps}
    return {"groups": groups, "n": np.bincount(labels, minlength=G), "ame": ame, "se.ame": se_ame, "vcov.ame": cov,
            "diff": diff, "se.diff": se_diff, "wald": wald, "reference": groups[ref], "derivatives": D,
            "which.derivatives": which, "binaryindicator": isbin[which_arr - 1],
            "xlabs": [xlabs[i - 1] for i in which], "newdata": nd_init}


def _run_folds(jobs, contexts, fit_fn, predict_fn):
    """Run independent (train, test) jobs, one worker thread per context (== per GPU), and return
    the results in job order. Fold k goes to context k mod G: a fixed assignment, and because every
    kernel is deterministic the result of a fold does not depend on which GPU computed it. The
    native calls release the GIL (ctypes), a context serves one thread at a time (include/bigkrls.h,
    "Threading"), and HIP's current device is per thread -- no process is spawned, so this is safe
    in a process that has already initialised the GPU."""
    import threading
    results = [None] * len(jobs)
    errors = []

    def worker(slot):
        cx = contexts[slot]
        try:
            if hasattr(cx, "torch"):
                cx.torch.cuda.set_device(cx.device_index)          # thread-local current device
            for j in range(slot, len(jobs), len(contexts)):
                results[j] = jobs[j](cx, fit_fn, predict_fn)
        except BaseException as e:                                 # re-raised in the caller's thread
            errors.append(e)

    if len(contexts) == 1:
        worker(0)
    else:
        threads = [threading.Thread(target=worker, args=(g,), name=f"bigkrls-fold-gpu{g}") for g in range(len(contexts))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    if errors:
        raise errors[0]
    return results


def _fold_contexts(ctx, devices, folds_per_device=1):
    """One context per requested GPU. `devices`: None (the given / default context only), "all",
    or a list of device indices (or of ready-made contexts). `folds_per_device` = 2 adds a second context
    with a stream of its own on every device (two folds side by side per GPU)."""
    if folds_per_device not in (1, 2):
        # measured (tools/cv_concurrency.py, N = 4000): two at a time 25 ms per fit against 41 one after the other;
        # three 37 (an odd split of the GPU between the persistent kernels), four 22-28: the second context is where
        # the gain is, and every further one costs its own N x N workspaces
        raise ValueError("folds_per_device must be 1 or 2")
    if folds_per_device == 2:
        base = _fold_contexts(ctx, devices)
        return base + [Context(c.device_index, own_stream=True) for c in base]
    if devices is None:
        return [ctx or default_context()]
    import torch
    if devices == "all":
        devices = list(range(torch.cuda.device_count()))
    devices = list(devices)
    if not devices:
        raise ValueError("devices must name at least one GPU")
    out = []
    for d in devices:
        if not isinstance(d, (int, np.integer)):                   # a ready-made context
            out.append(d)
        elif ctx is not None and ctx.device_index == int(d) and ctx not in out:
            out.append(ctx)
        else:
            out.append(Context(int(d)))
    return out


def crossvalidate(y, X, seed=None, Kfolds=None, ptesting=None, train_idx=None, folds=None,
                  ctx: Optional[Context] = None, devices=None, folds_per_device=1, **fit_args) -> BigKRLSCV:
    """crossvalidate.bigKRLS (R/bigKRLS.R:1146-1336).

    R partitions with set.seed(seed); sample() (:1168,1179,1232), a stream that
    cannot be reproduced without R, so the partition can be supplied explicitly:
    `train_idx` (0-based rows, ptesting branch) or `folds` (label 1..Kfolds per
    row, Kfolds branch).  Without them numpy's default_rng(seed) draws one.

    `devices` (None, "all" or a list of GPU indices): the folds of the Kfolds branch are whole,
    independent fits (the loop at :1268-1282), so they run as replicas, one fold per GPU at a time
    (last row): one context and one worker thread per GPU, no data-path
    collective. The statistics are identical to the sequential loop's.
    `folds_per_device` = 2 runs two folds side by side on every GPU (a second context with its own stream and
    worker thread): fold-sized fits are bound by latency chains that leave most of the GPU idle -- eight fits of
    N = 4000 take 0.33 s one after the other and 0.20 s two at a time (`tools/cv_concurrency.py`); results bitwise
    those of the sequential loop (tests/test_gpu_fit.py, two contexts). More than two gain little (see _fold_contexts) and are refused.
    """
    if (Kfolds is None) + (ptesting is None) != 1:
        raise ValueError("Specify either Kfolds or ptesting but not both.")
    Xh = _as_host_matrix(X)
    yh = np.asarray(_as_host_matrix(y), dtype=np.float64).ravel()
    N = Xh.shape[0]
    marginals = fit_args.get("derivative", True)
    rng = np.random.default_rng(seed)

    def one_split(tr, te, cx, fit_fn, predict_fn):
        trained = fit_fn(yh[tr], Xh[tr], ctx=cx, **fit_args)
        tested = predict_fn(trained, Xh[te])
        ytest = yh[te]
        tested["ytest"] = ytest
        r = {"trained": trained, "tested": tested}
        r["pseudoR2_is"] = trained["R2"]
        r["pseudoR2_oos"] = _cor(tested["predicted"], ytest) ** 2                 # :1195
        r["MSE_oos"] = float(np.mean((tested["predicted"] - ytest) ** 2))         # :1196
        r["MSE_is"] = float(np.mean((trained["yfitted"] - trained["y"]) ** 2))    # :1197
        if marginals:
            r["pseudoR2AME_is"] = trained["R2AME"]
            delta = np.asarray(trained["avgderivatives"]).ravel()
            r["MSE_AME_is"] = float(np.mean((trained["y"] - trained["X"] @ delta) ** 2))   # :1206
            yhat_ame = Xh[te] @ delta
            r["pseudoR2AME_oos"] = _cor(ytest, yhat_ame) ** 2                     # :1212
            r["MSE_AME_oos"] = float(np.mean((ytest - yhat_ame) ** 2))            # :1213
        return r

    contexts = _fold_contexts(ctx, devices, folds_per_device)
    if ptesting is not None:
        if ptesting < 0 or ptesting > 100:
            raise ValueError("ptesting, the percentage of data to be used for validation, must be between 0 and 100.")
        Ntesting = int(round(N * ptesting / 100.0))
        Ntraining = N - Ntesting
        if train_idx is None:
            train_idx = rng.choice(N, Ntraining, replace=False)
        tr = np.asarray(train_idx)
        te = np.setdiff1d(np.arange(N), tr)
        out = BigKRLSCV(one_split(tr, te, contexts[0], _cv_fit, _cv_predict))
        out.update(type="crossvalidated", seed=seed, ptesting=ptesting,
                   indices={"train.set": tr, "test.set": te})
        return out

    if not (float(Kfolds) > 0 and float(Kfolds) % 1 == 0):
        raise ValueError("Kfolds must be a positive integer")
    Kfolds = int(Kfolds)
    if folds is None:
        perm = rng.permutation(N)
        folds = np.empty(N, dtype=int)
        folds[perm] = (np.arange(N) * Kfolds // N) + 1
    folds = np.asarray(folds)
    out = BigKRLSCV({"type": "KfoldsCV", "Kfolds": Kfolds, "seed": seed, "folds": folds})
    keys = ["R2_is", "R2_oos", "MSE_is", "MSE_oos"]
    if marginals:
        keys += ["R2AME_is", "R2AME_oos", "MSE_AME_is", "MSE_AME_oos"]
    for k in keys:
        out[k] = []

    def job(k):
        tr = np.nonzero(folds != k)[0]
        te = np.nonzero(folds == k)[0]
        return lambda cx, fit_fn, predict_fn: one_split(tr, te, cx, fit_fn, predict_fn)

    results = _run_folds([job(k) for k in range(1, Kfolds + 1)], contexts, _cv_fit, _cv_predict)
    out["devices"] = [getattr(c, "device_index", None) for c in contexts]
    for k, r in zip(range(1, Kfolds + 1), results):
        out[f"fold_{k}"] = r
        out["R2_is"].append(r["pseudoR2_is"])
        out["R2_oos"].append(r["pseudoR2_oos"])
        out["MSE_is"].append(r["MSE_is"])
        out["MSE_oos"].append(r["MSE_oos"])
        if marginals:
            out["R2AME_is"].append(r["pseudoR2AME_is"])
            out["R2AME_oos"].append(r["pseudoR2AME_oos"])
            out["MSE_AME_is"].append(r["MSE_AME_is"])
            out["MSE_AME_oos"].append(r["MSE_AME_oos"])
    return out


# the fit / predict the cross-validation driver calls (module-level so that the CPU tests of the fold
# scheduler can substitute doubles that need no GPU)
_cv_fit = bigKRLS
_cv_predict = predict
