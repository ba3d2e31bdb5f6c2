"""Every BASELINE.json configuration as a full fit on one MI355X.

C2 (N=5000, P=10)   bigKRLS() against the CPU oracle at 1e-6, eigtrunc 0.001 and 0 (quirk Q7 guarded)
C3 (N=20000, P=20)  eigen residual / orthonormality on the kept vectors at the bench size, and the
                    top of the spectrum, lambda and c against ARPACK on the host (the oracle's
                    stand-in for eigs_sym)
C4 (N=50000, P=20, Neig=512)            size-independent properties + block Lanczos vs the dense path
C5 (N=100000, P=50, Neig=1024, which.derivatives=c(1,3,5))   the same, plus quirk Q6
n = 33000           the dense path where bc_wavefront / pq_step are selected by size, not by a switch

Tolerances: 1e-6 relative on c, yhat, lambda, derivatives (north_star); eigen residuals 1e-11.
The properties are the ones SURVEY.md section 8(d) lists for sizes no CPU oracle reaches: the
lastkeeper rule, ||K Q - Q D||, ||Q'Q - I||, the normal equations on the kept subspace, the
derivative identities, trace identities of the variance matrices.
"""
import os
import time

import numpy as np
import pytest

from oracle import krls_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-6


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def unit_columns(n, rows):
    E = np.zeros((n, len(rows)))
    E[np.asarray(rows), np.arange(len(rows))] = 1.0
    return E


def standardized(X, y):
    return (X - X.mean(0)) / X.std(0, ddof=1), (y - y.mean()) / y.std(ddof=1)


def eigen_quality(ops, K, Q, lam):
    """max |K Q - Q diag(lam)| / lam_1 and max |Q'Q - I| with the products on the device."""
    k = Q.ncol
    R = ops.gemm(False, False, K, Q).to_numpy() - Q.to_numpy() * lam[:k]
    G = ops.gemm(True, False, Q, Q).to_numpy()
    return float(np.abs(R).max() / lam[0]), float(np.abs(G - np.eye(k)).max())


def kept_subspace_checks(ctx, ops, out, K, Q, ys, n):
    """Identities every fit must satisfy whatever its size, with K and Q on the device:
    lastkeeper rule (R/bigKRLS_Rcpp_functions.R:190), c and yhat inside span(Q), the normal
    equations projected on the kept subspace, Neffective (all Neig values, quirk Q5), sigmasq."""
    d = out["K.eigenvalues"]
    k = out["lastkeeper"]
    lam = out["lambda"]
    c = out["coeffs"]
    yhat = out["yfitted.std"]
    assert np.all(np.diff(d) <= 1e-9 * d[0])
    assert abs(out["Neffective"] - (n - np.sum(d / (d + lam)))) < 1e-9 * n
    cd, yd = ctx.from_numpy(c), ctx.from_numpy(ys)
    a_c = ops.matvec(Q, cd, trans=True).to_numpy().ravel()              # Q'c
    a_y = ops.matvec(Q, yd, trans=True).to_numpy().ravel()              # Q'y
    # c = Q (Q'y / (d + lam))  <=>  Q'c = Q'y/(d+lam) and c in span(Q)
    assert rel(a_c, a_y / (d[:k] + lam)) < 1e-8
    c_proj = ops.matvec(Q, ctx.from_numpy(a_c)).to_numpy().ravel()
    assert rel(c_proj, c) < 1e-9
    # yhat = K c (full K, R/bigKRLS.R:291) and, on the kept pairs, = Q (d Q'y/(d+lam))
    Kc = ops.matvec(K, cd).to_numpy().ravel()
    assert rel(Kc, yhat) < 1e-10
    yk = ops.matvec(Q, ctx.from_numpy(d[:k] * a_y / (d[:k] + lam))).to_numpy().ravel()
    assert rel(yk, yhat) < 1e-8
    # (K + lam I) c = y on the kept subspace
    r = Kc + lam * c - ys
    assert np.abs(ops.matvec(Q, ctx.from_numpy(r), trans=True).to_numpy()).max() < 1e-9 * np.abs(a_y).max()
    assert abs(out["sigmasq"] - np.sum((ys - yhat) ** 2) / n) < 1e-12
    g = ops.bSolveForc(yd, ops.Eigenobject(values=d, lastkeeper=k, vectors=Q, values_dev=ctx.from_numpy(d)), lam)
    assert abs(g["Le"] - out["Le"]) <= 1e-12 * out["Le"]


def derivative_identities(ctx, ops, out, K, Xs, cols, sigma):
    """Continuous columns: D_j = (-2/sigma) (x_j o Kc - K (x_j o c)) (src/bigderiv_v3.cpp:90-103 in its
    O(N^2) form) recomputed with plain matvecs, independent of the fused derivative kernel.
    `cols` are 0-based columns of X; with which.derivatives the outputs hold only the selected ones."""
    c = out["coeffs"]
    Kc = out["yfitted.std"]
    D = out["derivatives.std"]
    which = out["which.derivatives"]
    for j in cols:
        i = j if which is None else which.index(j + 1)
        x = Xs[:, j]
        Kxc = ops.matvec(K, ctx.from_numpy(x * c)).to_numpy().ravel()
        assert rel(D[:, i], (-2.0 / sigma) * (x * Kc - Kxc)) < 1e-9, j


def host_checks_from_downloaded_pairs(ctx, ops, out, K, Qh, Xs, ys, X, y, cols, rows, dvc, dvf, sigma):
    """Checks whose expected values contain NOTHING computed by the library but (i) the eigenpairs of the fit,
    downloaded (their residual against K is checked separately), and (ii) a few rows of K, downloaded and pinned
    against the literal kernel formula here: lambda, Le and c from the oracle's golden-section search and solveforc
    on the host (R/bigKRLS_Rcpp_functions.R:5-82, src/solveforc.cpp:13-65); the derivatives of `cols` at `rows`
    from numpy products with the K rows (src/bigderiv_v3.cpp:103); the diagonals of both variance matrices from the
    host copy of Q (R/bigKRLS.R:299-307, :438, :445). `dvc`, `dvf`: the diagonals as the fit returned them."""
    n = Xs.shape[0]
    d = out["K.eigenvalues"]
    k = out["lastkeeper"]
    eig_h = orc.EigenObject(values=d, lastkeeper=k, vectors=Qh[:, :k])
    lam_h = orc.lambda_search(eig_h, ys)
    assert abs(out["lambda"] - lam_h) <= TOL * lam_h
    le_h, c_h = orc.solveforc_fast(eig_h.vectors, eig_h.values, ys, lam_h)
    assert rel(out["coeffs"], c_h) < TOL
    assert abs(out["Le"] - le_h) <= TOL * le_h
    # K rows: pulled from the device, checked entry by entry against exp(-||x_i - x_j||^2 / sigma)
    Krows = ops.gemm(False, False, K, ctx.from_numpy(unit_columns(n, rows))).to_numpy().T     # len(rows) x n
    for a, r in enumerate(rows):
        assert rel(Krows[a], orc.temp_kernel_literal(Xs, Xs[r:r + 1], sigma).ravel()) < 1e-13, r
    assert rel(out["yfitted.std"][rows], Krows @ c_h) < TOL                                   # R/bigKRLS.R:291
    which = out["which.derivatives"]
    for j in cols:
        i = j if which is None else which.index(j + 1)
        x = Xs[:, j]
        want = (-2.0 / sigma) * (x[rows] * (Krows @ c_h) - Krows @ (x * c_h))                 # src/bigderiv_v3.cpp:103
        assert rel(out["derivatives.std"][rows, i], want) < TOL, j
    sigsq_h = out["sigmasq"]
    wv = sigsq_h * (d[:k] + lam_h) ** -2.0
    sd2 = y.std(ddof=1) ** 2
    q2 = Qh[:, :k] ** 2
    assert rel(dvc, sd2 * (q2 @ wv)) < TOL
    assert rel(dvf, sd2 * (q2 @ (wv * d[:k] ** 2))) < TOL
    return lam_h, c_h


# --------------------------------------------------------------------------------------------
# C2
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eigtrunc", [0.001, 0.0])
def test_c2_full_fit_vs_oracle(ctx, eigtrunc):
    """BASELINE.json configs[1]: N=5000, P=10, seed 102, full eigendecomposition, all derivatives,
    vcov matrices; eigtrunc = 0.001 (the default for n > 3000) and 0 (quirk Q7 --
    c-parity at eigtrunc=0 is only well posed when min(d) > 1e-9 max(d), asserted first)."""
    import bigkrls_amd as bk
    n, p = 5000, 10
    X, y = orc.synth(n, p, 102)
    trace_ref = orc.LambdaTrace(0, 0)
    ref = orc.fit(y, X, eigtrunc=eigtrunc, literal=False, trace=trace_ref)
    d = ref["K.eigenvalues"]
    if eigtrunc == 0.0:
        assert d.min() > 1e-9 * d.max(), "Q7: K numerically singular, c-parity ill-posed at eigtrunc=0"
        assert ref["lastkeeper"] == n
    tr = []
    out = bk.bigKRLS(y, X, eigtrunc=eigtrunc, ctx=ctx, trace=tr)
    assert out["lastkeeper"] == ref["lastkeeper"]
    assert rel(out["K.eigenvalues"], d) < 1e-11
    assert len(tr) == len(trace_ref.probes)                      # same golden-section path (Q8)
    assert abs(out["lambda"] - ref["lambda"]) <= TOL * ref["lambda"]
    for key in ["coeffs", "yfitted", "derivatives", "avgderivatives", "var.avgderivatives",
                "derivatives.std", "var.avgderivatives.std"]:
        assert rel(out[key], ref[key]) < TOL, key
    for key in ["R2", "R2AME", "Looe", "Neffective", "sigmasq"]:
        assert abs(out[key] - ref[key]) <= TOL * abs(ref[key]), key
    for key in ["K", "vcov.est.c", "vcov.est.fitted"]:           # n > 2500: device-resident outputs
        assert hasattr(out[key], "to_numpy")
        assert rel(out[key].to_numpy(), ref[key]) < TOL, key


def test_c2_size_fit_with_a_binary_column_vs_oracle(ctx):
    """A C2-size fit (N=5000, P=10) whose last column is binary (SURVEY 8(d)'s binary variant of G(N,P,seed);
    threshold from examples/numeric_convergence.md:13): the first-difference branch of BigDerivMat
    (src/bigderiv_v3.cpp:31-87) at a size where the derivative pass runs many tiles, against the oracle."""
    import bigkrls_amd as bk
    n, p = 5000, 10
    X, y = orc.synth(n, p, 112, binary_last=True)
    assert np.unique(X[:, -1]).size == 2
    ref = orc.fit(y, X, literal=False)
    out = bk.bigKRLS(y, X, ctx=ctx)
    assert out["binaryindicator"].tolist() == [False] * (p - 1) + [True]
    assert out["lastkeeper"] == ref["lastkeeper"]
    assert abs(out["lambda"] - ref["lambda"]) <= TOL * ref["lambda"]
    for key in ["coeffs", "yfitted", "derivatives", "avgderivatives", "var.avgderivatives",
                "derivatives.std", "var.avgderivatives.std"]:
        assert rel(out[key], ref[key]) < TOL, key
    # the binary column by itself (its scale differs from the continuous ones')
    assert rel(out["derivatives.std"][:, -1], ref["derivatives.std"][:, -1]) < TOL
    assert abs(out["var.avgderivatives.std"][-1] - ref["var.avgderivatives.std"][-1]) <= TOL * ref["var.avgderivatives.std"][-1]
    for key in ["R2", "R2AME", "Looe", "Neffective"]:
        assert abs(out[key] - ref[key]) <= TOL * abs(ref[key]), key
    for key in ["vcov.est.c", "vcov.est.fitted"]:
        assert rel(out[key].to_numpy(), ref[key]) < TOL, key


# --------------------------------------------------------------------------------------------
# C3
# --------------------------------------------------------------------------------------------
def test_c3_eigen_residuals_and_host_arpack(ctx):
    """BASELINE.json configs[2] (the bench workload), N=20000, P=20, eigtrunc=0.001: the only size at
    which pq_resident runs 79 workgroups with the two-level exchange and bc_resident 312 co-resident
    workgroups. (i) residual and orthonormality of the kept eigenvectors; (ii) the top of the spectrum
    against ARPACK on the host (what the reference's eigs_sym is; scipy's build), then lambda and c
    recomputed on the host from those pairs with the oracle's lambda search."""
    import scipy.sparse.linalg as ssl
    import bigkrls_amd as bk
    from bigkrls_amd import ops
    n, p = 20000, 20
    X, y = orc.synth(n, p, 103)
    Xs, ys = standardized(X, y)
    before = ctx.counters()
    out = bk.bigKRLS(y, X, ctx=ctx)
    k = out["lastkeeper"]
    d = out["K.eigenvalues"]
    assert k == int(np.max(np.nonzero(d >= 0.001 * d[0])[0])) + 1
    assert abs(d.sum() - n) < 1e-10 * n
    K = out["K"]
    eo = ops.bEigen(K, n, 0.001)
    after = ctx.counters()
    # A second decomposition of the same K: the same kept pairs and the same eigenvalues. To rounding, not bit for bit:
    # this session's multi-rank cases share the GPU with this test, and at N = 20 000 the persistent kernels (312
    # workgroups that must be co-resident) may meet a watchdog in one of the two runs -- the call then redoes the
    # decomposition with the per-step kernels, whose results differ in the last bits. Bitwise
    # run-to-run equality is asserted at a size that leaves room: test_eigen_is_run_to_run_deterministic.
    assert eo.lastkeeper == k and rel(eo.values, d) < 1e-13
    # ... and bit for bit whenever neither run took a recovery path (the context counts them)
    print(f"C3: recovery counters before {before}, after {after}")
    if after == before:
        assert np.array_equal(eo.values, d)
    res, orth = eigen_quality(ops, K, eo.vectors, d)
    print(f"C3: kept {k}, max|KQ-QD|/d1 = {res:.2e}, max|Q'Q-I| = {orth:.2e}")
    assert res < 1e-11 and orth < 1e-11
    kept_subspace_checks(ctx, ops, out, K, eo.vectors, ys, n)
    derivative_identities(ctx, ops, out, K, Xs, [0, 7, 19], float(p))
    # ---- host oracle for the top of the spectrum ------------------------------------------------
    t0 = time.perf_counter()
    Kh = K.to_numpy()
    assert rel(Kh[:, 17], orc.temp_kernel_literal(Xs, Xs[17:18], float(p)).ravel()) < 1e-13
    kk = k + 6
    hv, hq = ssl.eigsh(Kh, k=kk, which="LA", tol=1e-13, ncv=min(n - 1, 2 * kk + 40))
    order = np.argsort(hv)[::-1]
    hv, hq = hv[order], hq[:, order]
    print(f"C3: host ARPACK top-{kk} in {time.perf_counter() - t0:.1f} s")
    assert rel(d[:kk], hv) < 1e-11
    # lambda search and coefficients on the host from ARPACK's pairs; the bounds need all N
    # eigenvalues (quirk Q5), which only the device has: the device's tail is checked by the trace
    # identity above and enters only through sum(d/(d+L)) in the bounds loops
    eig_h = orc.EigenObject(values=np.concatenate([hv[:k], d[k:]]), lastkeeper=k, vectors=hq[:, :k])
    lam_h = orc.lambda_search(eig_h, ys)
    assert abs(out["lambda"] - lam_h) <= TOL * lam_h
    le_h, c_h = orc.solveforc_fast(eig_h.vectors, eig_h.values, ys, lam_h)
    assert rel(out["coeffs"], c_h) < TOL
    assert abs(out["Le"] - le_h) <= TOL * le_h
    assert rel(out["yfitted.std"], Kh @ c_h) < TOL
    # ---- marginal effects and variances of ALL 20 columns from the host's K and ARPACK's pairs --------------
    # (src/bigderiv_v3.cpp:90-106 in the oracle's O(N^2) form; V = Q diag(wv) Q', R/bigKRLS.R:299-301)
    sigsq_h = float(np.sum((ys - Kh @ c_h) ** 2) / n)                                     # R/bigKRLS.R:294
    assert abs(out["sigmasq"] - sigsq_h) <= TOL * sigsq_h
    wv_h = sigsq_h * (hv[:k] + lam_h) ** -2.0
    t0 = time.perf_counter()
    D_h, var_h = orc.derivmat_fast(Xs, Kh, c_h, float(p), hq[:, :k], wv_h)
    print(f"C3: host derivatives of {p} columns in {time.perf_counter() - t0:.1f} s")
    assert out["derivatives.std"].shape == (n, p)
    for j in range(p):
        assert rel(out["derivatives.std"][:, j], D_h[:, j]) < TOL, j
    assert rel(out["var.avgderivatives.std"], var_h) < TOL
    sdy, sdx = y.std(ddof=1), X.std(0, ddof=1)
    assert rel(out["derivatives"], D_h * sdy / sdx) < TOL                                  # R/bigKRLS.R:394-397
    assert rel(out["avgderivatives"].ravel(), (D_h * sdy / sdx).mean(0)) < TOL             # :400
    assert rel(out["var.avgderivatives"].ravel(), (sdy / sdx) ** 2 * var_h) < TOL          # :403-407
    # diagonals of the variance matrices: sd(y)^2 sum_k q_ik^2 wv_k and ... d_k^2 wv_k     (:438, :445, :307)
    q2 = hq[:, :k] ** 2
    assert rel(out["vcov.est.c"].diag().ravel(), sdy ** 2 * (q2 @ wv_h)) < TOL
    assert rel(out["vcov.est.fitted"].diag().ravel(), sdy ** 2 * (q2 @ (wv_h * hv[:k] ** 2))) < TOL
    # ... and a sampled block of each against Q diag(w) Q' on the host
    rows = np.array([0, 1, 4097, 9999, n - 1])
    blk = sdy ** 2 * (hq[rows, :k] * wv_h) @ hq[:, :k].T
    Vc_rows = ops.gemm(False, False, out["vcov.est.c"], ctx.from_numpy(unit_columns(n, rows))).to_numpy()   # columns = rows (symmetric)
    assert rel(Vc_rows.T, blk) < TOL
    del Kh


# --------------------------------------------------------------------------------------------
# n > 32768 through the dense path
# --------------------------------------------------------------------------------------------
def test_dense_path_above_resident_limit(ctx, monkeypatch):
    """n = 33000 > 32768: more band locations than co-resident workgroups, so the library itself selects
    bc_wavefront (2n launches) and, for the first panels (> 80 workgroups), pq_step -- no environment
    switch. Kept eigenpairs at eigtrunc 0.001: residual, orthonormality, trace."""
    from bigkrls_amd import ops
    from bigkrls_amd.synth import synth
    for v in ("BIGKRLS_BC", "BIGKRLS_PQ", "BIGKRLS_EIG"):
        monkeypatch.delenv(v, raising=False)
    n, p = 33000, 8
    X, _ = synth(n, p, 77)
    Xs = (X - X.mean(0)) / X.std(0, ddof=1)
    K = ops.bGaussKernel(ctx.from_numpy(Xs), float(p))
    t0 = time.perf_counter()
    eo = ops.bEigen(K, None, 0.001)
    ctx.sync()
    dt = time.perf_counter() - t0
    k = eo.lastkeeper
    assert 0 < k < n and k == int(np.max(np.nonzero(eo.values >= 0.001 * eo.values[0])[0])) + 1
    res, orth = eigen_quality(ops, K, eo.vectors, eo.values)
    tr = abs(eo.values.sum() - n) / n
    print(f"n=33000 dense: {dt:.2f} s, kept {k}, resid {res:.2e}, orth {orth:.2e}, trace {tr:.2e}")
    assert res < 1e-11 and orth < 1e-11 and tr < 1e-11
    del K, eo
    ctx.release_workspace()


# --------------------------------------------------------------------------------------------
# C4
# --------------------------------------------------------------------------------------------
def test_c4_fit_properties_and_lanczos_vs_dense(ctx, monkeypatch):
    """BASELINE.json configs[3] on one GPU: N=50000, P=20, Neig=512 (the reference's eigs_sym branch,
    src/eigen.cpp:18-22 -> block Lanczos here)."""
    import bigkrls_amd as bk
    from bigkrls_amd import ops
    from bigkrls_amd.synth import synth
    monkeypatch.delenv("BIGKRLS_EIGK", raising=False)
    n, p, neig = 50000, 20, 512
    X, y = synth(n, p, 104)
    Xs, ys = standardized(X, y)
    T = {}
    out = bk.bigKRLS(y, X, Neig=neig, ctx=ctx, timings=T)
    print("C4 timings:", {k: round(v, 3) for k, v in T.items()}, "lastkeeper", out["lastkeeper"])
    d = out["K.eigenvalues"]
    k = out["lastkeeper"]
    assert d.shape == (neig,)
    assert k == int(np.max(np.nonzero(d >= 0.001 * d[0])[0])) + 1     # lastkeeper rule, eigtrunc default 0.001
    K = out["K"]
    eo = ops.bEigen(K, neig, 0.001)
    assert eo.lastkeeper == k and rel(eo.values, d) < 1e-13
    res, orth = eigen_quality(ops, K, eo.vectors, d)
    print(f"C4: kept {k}, resid {res:.2e}, orth {orth:.2e}")
    assert res < 1e-9 and orth < 1e-11        # Lanczos stops at Ritz residuals of 1e-10 theta_1
    kept_subspace_checks(ctx, ops, out, K, eo.vectors, ys, n)
    derivative_identities(ctx, ops, out, K, Xs, range(p), float(p))
    assert np.isfinite(out["derivatives"]).all()
    sd2 = y.std(ddof=1) ** 2
    lam = out["lambda"]
    # var(avg derivative) of every column, standardised: 4/(sigma^2 n^2) s'Vs with s = x o K1 - K x and
    # V = Q diag(wv) Q' (src/bigderiv_v3.cpp:105 in its O(N^2) form), from plain matvecs
    wv = out["sigmasq"] * (d[:k] + lam) ** -2.0
    K1 = ops.matvec(K, ctx.from_numpy(np.ones(n))).to_numpy().ravel()
    sdx, sdy = X.std(0, ddof=1), y.std(ddof=1)
    for j in range(p):
        x = Xs[:, j]
        s_j = x * K1 - ops.matvec(K, ctx.from_numpy(x)).to_numpy().ravel()
        qs = ops.matvec(eo.vectors, ctx.from_numpy(s_j), trans=True).to_numpy().ravel()
        want = 4.0 / (float(p) ** 2 * float(n) ** 2) * float(np.sum(wv * qs * qs))
        assert abs(out["var.avgderivatives.std"][j] - want) <= 1e-8 * want, j
    assert rel(out["var.avgderivatives"].ravel(), (sdy / sdx) ** 2 * out["var.avgderivatives.std"]) < 1e-13
    assert rel(out["derivatives"], out["derivatives.std"] * sdy / sdx) < 1e-13
    # three columns and the variance-matrix diagonals against the HOST: K rows pulled from the device, products
    # with numpy (nothing of the library in the expected values but the kernel entries, which C3 pins to 1e-13)
    c_fit, Kc_fit = out["coeffs"], out["yfitted.std"]
    Qh = eo.vectors.to_numpy()
    for j in (0, 11, 19):
        x = Xs[:, j]
        rows = np.array([3, 25000, n - 2])
        Krows = ops.gemm(False, False, K, ctx.from_numpy(unit_columns(n, rows))).to_numpy().T   # 3 x n rows of K
        assert rel(Krows[0], orc.temp_kernel_literal(Xs, Xs[rows[:1]], float(p)).ravel()) < 1e-13
        want = (-2.0 / float(p)) * (x[rows] * (Krows @ c_fit) - Krows @ (x * c_fit))         # src/bigderiv_v3.cpp:103
        assert rel(out["derivatives.std"][rows, j], want) < TOL, j
    q2 = Qh[:, :k] ** 2
    assert rel(out["vcov.est.c"].diag().ravel(), sd2 * (q2 @ wv)) < TOL
    assert rel(out["vcov.est.fitted"].diag().ravel(), sd2 * (q2 @ (wv * d[:k] ** 2))) < TOL
    # lambda, Le and c from the oracle's search / solveforc on the HOST, fed with the downloaded pairs
    # (the C3 pattern minus ARPACK: nothing of the library's own matvec in the expected values)
    t0 = time.perf_counter()
    lam_h, _ = host_checks_from_downloaded_pairs(ctx, ops, out, K, Qh, Xs, ys, X, y, [0, 11, 19],
                                                 np.array([3, 25000, n - 2]), out["vcov.est.c"].diag().ravel(),
                                                 out["vcov.est.fitted"].diag().ravel(), float(p))
    print(f"C4: host lambda search / solveforc / K rows in {time.perf_counter() - t0:.1f} s, lambda {lam_h:.12g}")
    del Qh, q2
    tv = out["vcov.est.c"].diag().sum() / sd2
    tf = out["vcov.est.fitted"].diag().sum() / sd2
    assert abs(tv - out["sigmasq"] * np.sum((d[:k] + lam) ** -2.0)) < 1e-8 * tv
    assert abs(tf - out["sigmasq"] * np.sum(d[:k] ** 2 * (d[:k] + lam) ** -2.0)) < 1e-8 * tf
    Qk = eo.vectors
    vk = d.copy()
    del out
    # ---- the same top-512 pairs through the dense two-stage path ------------------------------------
    monkeypatch.setenv("BIGKRLS_EIGK", "dense")
    t0 = time.perf_counter()
    de = ops.bEigen(K, neig, 0.001)
    ctx.sync()
    print(f"C4 dense path: {time.perf_counter() - t0:.2f} s")
    assert de.lastkeeper == k
    assert rel(de.values, vk) < 1e-11
    rng = np.random.default_rng(1)
    z = ctx.from_numpy(rng.standard_normal(n))
    pk = ops.matvec(Qk, ops.matvec(Qk, z, trans=True)).to_numpy()
    pd = ops.matvec(de.vectors, ops.matvec(de.vectors, z, trans=True)).to_numpy()
    gap = (vk[k - 1] - (vk[k] if k < neig else 0.0)) / vk[0]
    assert rel(pk, pd) < max(1e-7, 1e-11 / max(gap, 1e-300))          # same invariant subspace
    del de, Qk, K, eo
    ctx.release_workspace()
    ctx.torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------
# C5
# --------------------------------------------------------------------------------------------
def test_c5_fit_properties_which_derivatives(ctx, monkeypatch):
    """BASELINE.json configs[4] on one GPU: N=100000, P=50, Neig=1024, which.derivatives=c(1,3,5).
    K, vcov.est.c and vcov.est.fitted are 80 GB each; standardised derivatives are checked against the
    matvec identity, the rescaled ones against quirk Q6 (R/bigKRLS.R:395-397 divides column i of the
    subset by X.init.sd[i], not by the sd of the selected column)."""
    import bigkrls_amd as bk
    from bigkrls_amd import ops
    from bigkrls_amd.synth import synth
    monkeypatch.delenv("BIGKRLS_EIGK", raising=False)
    import gc
    gc.collect()                           # (device outputs of the test before this one, kept alive by reference cycles)
    ctx.release_workspace()                # 258 of the 288 GB are needed: start from an empty device
    ctx.torch.cuda.empty_cache()
    n, p, neig = 100000, 50, 1024
    which = [1, 3, 5]
    X, y = synth(n, p, 105)
    Xs, ys = standardized(X, y)
    T = {}
    out = bk.bigKRLS(y, X, Neig=neig, which_derivatives=which, ctx=ctx, timings=T)
    print("C5 timings:", {k: round(v, 3) for k, v in T.items()}, "lastkeeper", out["lastkeeper"])
    d = out["K.eigenvalues"]
    k = out["lastkeeper"]
    assert d.shape == (neig,) and k == int(np.max(np.nonzero(d >= 0.001 * d[0])[0])) + 1
    sd2 = y.std(ddof=1) ** 2
    lam = out["lambda"]
    tv = out["vcov.est.c"].diag().sum() / sd2
    tf = out["vcov.est.fitted"].diag().sum() / sd2
    assert abs(tv - out["sigmasq"] * np.sum((d[:k] + lam) ** -2.0)) < 1e-8 * tv
    assert abs(tf - out["sigmasq"] * np.sum(d[:k] ** 2 * (d[:k] + lam) ** -2.0)) < 1e-8 * tf
    dvc = out["vcov.est.c"].diag().ravel()
    dvf = out["vcov.est.fitted"].diag().ravel()
    out["vcov.est.c"] = out["vcov.est.fitted"] = None           # 160 GB back to the allocator
    ctx.torch.cuda.empty_cache()
    K = out["K"]
    eo = ops.bEigen(K, neig, 0.001)
    assert eo.lastkeeper == k and rel(eo.values, d) < 1e-13
    res, orth = eigen_quality(ops, K, eo.vectors, d)
    print(f"C5: kept {k}, resid {res:.2e}, orth {orth:.2e}")
    assert res < 1e-9 and orth < 1e-11
    kept_subspace_checks(ctx, ops, out, K, eo.vectors, ys, n)
    cols = [w - 1 for w in which]
    assert out["derivatives"].shape == (n, 3) and out["derivatives.std"].shape == (n, 3)
    derivative_identities(ctx, ops, out, K, Xs, cols, float(p))
    # var(avg derivative), standardised: 4/(sigma^2 n^2) s'Vs with s = x o K1 - K x, V = Q diag(wv) Q'
    wv = out["sigmasq"] * (d[:k] + lam) ** -2.0
    K1 = ops.matvec(K, ctx.from_numpy(np.ones(n))).to_numpy().ravel()
    for i, j in enumerate(cols):
        x = Xs[:, j]
        s = x * K1 - ops.matvec(K, ctx.from_numpy(x)).to_numpy().ravel()
        qs = ops.matvec(eo.vectors, ctx.from_numpy(s), trans=True).to_numpy().ravel()
        want = 4.0 / (float(p) ** 2 * float(n) ** 2) * float(np.sum(wv * qs * qs))
        assert abs(out["var.avgderivatives.std"][i] - want) <= 1e-8 * want
    # the host-side sample C4 has: three K rows against the literal formula, lambda / Le / c from the oracle on the
    # host with the downloaded pairs, the three selected columns' derivatives at those rows from numpy products, the
    # diagonals of both variance matrices from the host copy of Q -- independent of the library's own matvec
    t0 = time.perf_counter()
    Qh = eo.vectors.to_numpy()
    lam_h, _ = host_checks_from_downloaded_pairs(ctx, ops, out, K, Qh, Xs, ys, X, y, cols,
                                                 np.array([7, 50001, n - 3]), dvc, dvf, float(p))
    print(f"C5: host lambda search / solveforc / K rows in {time.perf_counter() - t0:.1f} s, lambda {lam_h:.12g}")
    del Qh
    # quirk Q6: rescaling by X.init.sd[1..3], not by the selected columns' sds
    sdx = X.std(0, ddof=1)
    sdy = y.std(ddof=1)
    for i in range(3):
        assert rel(out["derivatives"][:, i], out["derivatives.std"][:, i] * sdy / sdx[i]) < 1e-13
    assert rel(out["var.avgderivatives"].ravel(), (sdy / sdx[cols]) ** 2 * out["var.avgderivatives.std"]) < 1e-13
    assert rel(out["avgderivatives"].ravel(), out["derivatives"].mean(0)) < 1e-13
    del out, K, eo
    ctx.release_workspace()
    ctx.torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------
# in-process recovery paths of the eigensolver
# --------------------------------------------------------------------------------------------
def test_eigen_watchdog_retry_and_lanczos_fallback():
    """The recovery paths inside one eigen call (a fired watchdog -> per-step kernels; a block Lanczos that does not
    converge -> dense path), driven through the fault-injection hooks of the TEST build of the library in a process
    of its own (tests/_fault_inject.py); the shipped library carries no such hooks."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_fault_inject.py")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "fault injection OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_lanczos_sampled_verification_matches_full_rayleigh_ritz(ctx, monkeypatch):
    """The block Lanczos returns the Ritz pairs of its projected matrix after checking the true residual
    K q - theta q on the block of pairs that converges last; BIGKRLS_KRY_REFINE=1 refines all pairs by a
    Rayleigh-Ritz step against K instead (what every call did before, and the fallback when that check fails).
    Same eigenvalues to the square of the residual level, kept eigenvectors at rounding-level residual and
    orthogonality either way, and the same fit."""
    import bigkrls_amd as bk
    from bigkrls_amd import ops
    n, p, k = 16384, 6, 160
    X, y = orc.synth(n, p, 12)
    Xs = (X - X.mean(0)) / X.std(0, ddof=1)
    K = ops.bGaussKernel(ctx.from_numpy(Xs), float(p))
    fast = ops.bEigen(K, k, 0.001)
    monkeypatch.setenv("BIGKRLS_KRY_REFINE", "1")
    full = ops.bEigen(K, k, 0.001)
    fit_full = bk.bigKRLS(y, X, Neig=k, ctx=ctx)
    monkeypatch.delenv("BIGKRLS_KRY_REFINE")
    fit_fast = bk.bigKRLS(y, X, Neig=k, ctx=ctx)
    assert fast.lastkeeper == full.lastkeeper
    assert rel(fast.values, full.values) < 1e-11
    for e in (fast, full):
        res, orth = eigen_quality(ops, K, e.vectors, e.values)
        assert res < 1e-9 and orth < 1e-11, (res, orth)
    assert rel(fit_fast["coeffs"], fit_full["coeffs"]) < 1e-8
    assert rel(fit_fast["derivatives"], fit_full["derivatives"]) < 1e-8
    assert fit_fast["lambda"] == pytest.approx(fit_full["lambda"], rel=1e-9)


def test_aggregated_trailing_update_matches_one_update_per_panel(ctx, monkeypatch):
    """Stage 1 applies the trailing update for four panels at once (k = 512) while the trailing matrix has at least
    12800 rows, for two at once (k = 256, as two pieces of equal area) down to 10752, with thin corrections of
    everything that reads the stale matrix (csrc/eigen_2stage.inc, "aggregated phase"). n = 15700 runs eleven groups
    of four, the hand-over to pairs and the one to one update per panel; BIGKRLS_S1AGG=2 starts with pairs,
    BIGKRLS_S1AGG=0 is the plain loop. Same eigenvalues to rounding, kept eigenvectors with residual and
    orthogonality at rounding level."""
    from bigkrls_amd import ops
    from bigkrls_amd.synth import synth
    n, p = 15700, 7
    X, _ = synth(n, p, 91)
    Xs = (X - X.mean(0)) / X.std(0, ddof=1)
    K = ops.bGaussKernel(ctx.from_numpy(Xs), float(p))
    monkeypatch.setenv("BIGKRLS_S1AGG", "0")
    plain = ops.bEigen(K, None, 0.001)
    monkeypatch.delenv("BIGKRLS_S1AGG")
    agg = ops.bEigen(K, None, 0.001)
    monkeypatch.setenv("BIGKRLS_S1AGG", "2")
    pairs = ops.bEigen(K, None, 0.001)
    monkeypatch.delenv("BIGKRLS_S1AGG")
    for dec in (agg, pairs):
        assert dec.lastkeeper == plain.lastkeeper
        assert rel(dec.values, plain.values) < 1e-13
        res, orth = eigen_quality(ops, K, dec.vectors, dec.values)
        assert res < 1e-11 and orth < 1e-11 and abs(dec.values.sum() - n) < 1e-11 * n


def test_panel_factorisation_by_choleskyqr_matches_householder_kernel(ctx, monkeypatch):
    """Stage-1 panels are factorised by CholeskyQR2 + Householder reconstruction (pq_chol, csrc/eigen_2stage.inc);
    BIGKRLS_PQ=householder runs the 64-exchange Householder kernel (pq_resident) on every panel instead. Same
    eigenvalues to rounding, kept eigenvectors with residual and orthogonality at rounding level -- on a kernel
    matrix that crosses the aggregated phase and the hand-over (n = 12 200), and on a numerically singular one
    (P = 2: the later panels' Gram matrices are not positive definite, pq_chol leaves them to pq_resident)."""
    from bigkrls_amd import ops
    from bigkrls_amd.synth import synth
    for n, p, seed in ((12200, 9, 17), (2100, 2, 5)):
        X, _ = synth(n, p, seed)
        Xs = (X - X.mean(0)) / X.std(0, ddof=1)
        K = ops.bGaussKernel(ctx.from_numpy(Xs), float(p))
        monkeypatch.setenv("BIGKRLS_PQ", "householder")
        hh = ops.bEigen(K, None, 0.001)
        monkeypatch.delenv("BIGKRLS_PQ")
        ch = ops.bEigen(K, None, 0.001)
        assert ch.lastkeeper == hh.lastkeeper
        assert rel(ch.values, hh.values) < 1e-13
        res, orth = eigen_quality(ops, K, ch.vectors, ch.values)
        assert res < 1e-11 and orth < 1e-11 and abs(ch.values.sum() - n) < 1e-11 * n


def test_ill_conditioned_panels_fall_back_to_the_householder_kernel():
    """pq_chol leaves a panel whose Gram matrix has no safe Cholesky factor to pq_resident (launched behind it): on a
    rank-3 matrix every panel after the first ones does; BIGKRLS_VERBOSE reports the count (a process of its own: the
    library reads the variable at every call, the count goes to stderr)."""
    import subprocess
    import sys
    code = r"""
import sys, os
sys.path.insert(0, %r)
import numpy as np
import bigkrls_amd as bk
from bigkrls_amd import ops
rng = np.random.default_rng(3)
n = 1800
U = rng.standard_normal((n, 3))
A = U @ U.T + 1e-14 * np.eye(n)
ctx = bk.Context(0)
e = ops.bEigen(ctx.from_numpy(np.asfortranarray(A)), None, 0.0)
v = np.asarray(e.values).ravel()
ref = np.linalg.eigvalsh(A)[::-1]
print("max eigenvalue error", float(np.abs(v - ref).max() / ref[0]))
""" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BIGKRLS_VERBOSE="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    err = float(r.stdout.strip().split()[-1])
    assert err < 1e-13, r.stdout
    counts = [int(ln.split(":")[-1]) for ln in r.stderr.splitlines() if "panels left to the Householder kernel by pq_chol" in ln]
    assert counts and counts[0] > 0, r.stderr[-2000:]
