// bigkrls_group_effects(): the average marginal effect of every selected column within every subgroup of the new points,
// with the joint covariance of all of them -- what a test of "does the effect of x_j differ between the groups" needs --
// without one bigkrls_marginal_effects call per group and without any N x N matrix on the host.
//
// Notation and units are csrc/margeff.hip's (Xs, Zs, Kn, c, V = vcov.est.c / sd(y)^2). The pointwise effects D are
// bigkrls_marginal_effects' own (row side: R = Kn B, me_rows_kernel), and ame[g, jj] is the mean of column jj of D over
// the rows of group g. Each of them is linear in c: with the column-side vector of the group's rows alone,
//   S_e = me_cols_kernel(C_g),   C_g = K(Zs[g], Xs)' B*[g]   (n x q, q = 1 + |J|),        e = jj G + g,
//   ame_e = sd(y) a_e S_e' c,    a_e = -(2 / sigma) / (n_g sd(x_j))        continuous j
//                                a_e = +1 / ((z1 - z0) n_g sd(x_j))         binary j
// so cov[e, f] = a_e a_f S_e' V S_f (sd(y) cancels as in marginal_effects_impl). The reference's factor 2 on the variance
// of a binary column (src/bigderiv_v3.cpp:85) is carried as sqrt(2) on a_e of a binary entry: the diagonal is then exactly
// bigkrls_marginal_effects' h_var on the group's rows, and the matrix, a congruence of S' V S, stays positive semi-definite.
// All C_g come from ONE kernel_contract_grouped (csrc/gemm.hip); me_cols_kernel runs once with the group as blockIdx.y and
// writes S (n x G |J|) with the groups of one variable adjacent. M = S' V S: from the factors T = Q' S (gemm) and
// M = T' diag(w) T (gram_weighted: exactly symmetric); from the matrix P = V S and M = S' P (two gemm), symmetrised on the
// host. Device memory: O((u + n)(p + q)) + n G (q + |J|) + (G |J|)^2 doubles, never O(u n).
#include "margeff.h"

#include <cmath>

using namespace bk;

extern "C" {

int bigkrls_group_effects(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                          const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                          const double* h_newdata, int64_t u, const int64_t* h_group, int64_t G,
                          const double* d_vcov_c, const double* d_Q, int64_t ldq, int64_t k, const double* h_w,
                          double* h_derivatives, double* h_ame, double* h_cov) {
  BK_TRY(me_check_args(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_newdata, u, h_ame));
  BK_REQUIRE(!(d_vcov_c && d_Q), "group_effects: at most one of vcov.est.c and its factors may be given");
  const Vcov vc = d_vcov_c ? Vcov::matrix(d_vcov_c) : (d_Q ? Vcov::factors(d_Q, ldq, k, h_w) : Vcov());
  BK_REQUIRE(vc.given() == (h_cov != nullptr),
             "group_effects: h_cov is written exactly when vcov.est.c (or its factors) is given");
  BK_TRY(me_check_factors(vc, n));
  BK_REQUIRE(h_group, "group_effects: null labels");
  for (int64_t i = 0; i < u; ++i)    // (G < 1: row 1 is named)
    BK_REQUIRE(h_group[i] >= 0 && h_group[i] < G,
               "group_effects: the label of row " + std::to_string(i + 1) + " is outside [0, G)");
  BK_REQUIRE(G >= 1 && G < (1ll << 31), "group_effects: G must be at least 1");
  const int64_t kq = vc.cols();
  MePrep mp;
  BK_TRY(me_prepare(h_X, n, p, h_y, h_which, n_which, h_newdata, u, &mp));
  const int64_t nj = (int64_t)mp.cols.size(), q = 1 + nj, E = G * nj;
  BK_REQUIRE(E < (1ll << 15), "group_effects: " + std::to_string(G) + " groups x " + std::to_string(nj) +
                                  " columns: the covariance would have 2^30 entries or more");
  std::vector<int64_t> ng((size_t)G, 0);
  for (int64_t i = 0; i < u; ++i) ++ng[(size_t)h_group[i]];

  // ---- device layout ----------------------------------------------------------------------------------------------
  hipStream_t st = ctx->stream;
  const bool want_cov = vc.given();
  const int64_t colw = (int64_t)((sizeof(MeCol) + 7) / 8);
  const int64_t up_doubles = n * p + u * p + n + u + n * q + u * q + nj * colw + kq;   // uploaded, in this order
  const int64_t down_doubles = u * nj + (want_cov ? E * E : 0);                // read back: D, then M
  void* psmall = nullptr;
  BK_TRY(ws_get(ctx, SLOT_ME_SMALL, (up_doubles + u * q + down_doubles + 64) * (int64_t)sizeof(double), &psmall));
  double* qd = (double*)psmall;
  double* dXs = qd; qd += n * p;
  double* dZs = qd; qd += u * p;
  double* dnx = qd; qd += n;
  double* dnz = qd; qd += u;
  double* dB = qd; qd += n * q;
  double* dBs = qd; qd += u * q;
  MeCol* dcols = (MeCol*)qd; qd += nj * colw;
  double* dw = qd; qd += kq;
  double* dR = qd; qd += u * q;
  double* dD = qd; qd += u * nj;
  double* dM = qd; qd += want_cov ? E * E : 0;
  // C (n x G q) and S (n x G |J|); C is dead once S is written: T = Q' S (k x G |J|) or P = V S (n x G |J|) take its place
  void* pbig = nullptr;
  double *dC = nullptr, *dS = nullptr;
  if (want_cov) {
    BK_TRY(ws_get(ctx, SLOT_PP_K, n * G * (q + nj) * (int64_t)sizeof(double), &pbig));
    dC = (double*)pbig;
    dS = dC + n * G * q;
  }

  // ---- standardise (training means and sds, as bigkrls_predict), squared row norms, operands, upload. The training rows
  //      are centred by their standardisation, so the contractions take the operands as they are (as
  //      marginal_effects_se_impl's kernel blocks do): no shift by a column mean, whose rounding would depend on the order
  //      of the rows -- the same rows in another order give the same bits ------------------------------------------------
  double* pin = nullptr;
  BK_HIP(hipStreamSynchronize(st));   // (the pinned buffer may be reallocated)
  BK_TRY(pinned_get(ctx, std::max(up_doubles, down_doubles), &pin));
  {
    double* hXs = pin;
    double* hZs = hXs + n * p;
    double* hnx = hZs + u * p;
    double* hnz = hnx + n;
    double* hB = hnz + u;
    double* hBs = hB + n * q;
    MeCol* hcols = (MeCol*)(hBs + u * q);
    me_standardise(mp, h_X, n, p, h_newdata, u, hXs, hZs);
    auto sqnorms = [p](const double* A, int64_t rows, double* out) {
      for (int64_t i = 0; i < rows; ++i) out[i] = 0.0;
      for (int64_t j = 0; j < p; ++j)
        for (int64_t i = 0; i < rows; ++i) out[i] += A[j * rows + i] * A[j * rows + i];
    };
    sqnorms(hXs, n, hnx);
    sqnorms(hZs, u, hnz);
    for (int64_t i = 0; i < n; ++i) hB[i] = h_coeffs[i];
    for (int64_t i = 0; i < u; ++i) hBs[i] = 1.0;
    for (int64_t jj = 0; jj < nj; ++jj) {
      const int64_t j = mp.cols[jj];
      const double* x = h_X + j * n;
      const double* z = h_newdata + j * u;
      double* b = hB + (1 + jj) * n;
      double* bs = hBs + (1 + jj) * u;
      if (mp.isbin[j]) {                                // group membership on the raw values
        for (int64_t i = 0; i < n; ++i) b[i] = (x[i] == mp.hi[j] ? 1.0 : 0.0) * h_coeffs[i];
        for (int64_t i = 0; i < u; ++i) bs[i] = z[i] == mp.hi[j] ? 1.0 : 0.0;
      } else {
        for (int64_t i = 0; i < n; ++i) b[i] = hXs[j * n + i] * h_coeffs[i];
        std::memcpy(bs, hZs + j * u, (size_t)u * sizeof(double));
      }
      hcols[jj] = mp.col(jj);
    }
    if (kq > 0) std::memcpy((double*)hcols + nj * colw, vc.h_w, (size_t)kq * sizeof(double));
    BK_HIP(hipMemcpyAsync(dXs, pin, (size_t)up_doubles * sizeof(double), hipMemcpyHostToDevice, st));
  }

  // ---- row side: the pointwise effects ---------------------------------------------------------------------------------
  BK_TRY(kernel_contract_centred(ctx, dZs, u, u, dnz, dXs, n, n, dnx, p, sigma, dB, q, n, dR, u));    // R = Kn B
  int blocks = (int)std::min<int64_t>((u * nj + 255) / 256, 4096);
  hipLaunchKernelGGL(me_rows_kernel, dim3(blocks), dim3(256), 0, st, (int)u, (int)nj, (const double*)dR,
                     (const double*)dZs, (const double*)dBs, (const MeCol*)dcols, sigma, dD);
  BK_CHECK_LAUNCH();

  // ---- column side, all groups at once; M = S' V S ----------------------------------------------------------------------
  if (want_cov) {
    BK_TRY(kernel_contract_grouped_centred(ctx, dXs, n, n, dnx, dZs, u, u, dnz, p, sigma, dBs, q, u, h_group, G, dC,
                                           n));                                                       // all C_g
    const dim3 grid((unsigned)std::min<int64_t>((n * nj + 255) / 256, 1024), (unsigned)G);
    hipLaunchKernelGGL(me_cols_kernel, grid, dim3(256), 0, st, (int)n, (int)nj, (const double*)dC, (const double*)dXs,
                       (const MeCol*)dcols, sigma, dS, n * q, G * n, n);
    BK_CHECK_LAUNCH();
    if (vc.d_Q) {
      BK_TRY(gemm(ctx, 1, 0, kq, E, n, 1.0, vc.d_Q, vc.ldq, dS, n, 0.0, dC, kq));      // T = Q' S
      BK_TRY(gram_weighted(ctx, kq, E, dC, kq, dw, dM, E));                            // M = T' diag(w) T
    } else {
      BK_TRY(gemm(ctx, 0, 0, n, E, n, 1.0, vc.d_V, n, dS, n, 0.0, dC, n));             // P = vcov.est.c S
      BK_TRY(gemm(ctx, 1, 0, E, E, n, 1.0, dS, n, dC, n, 0.0, dM, E));                 // M = S' P
    }
  }
  // (gemm and gram_weighted do not touch the context's pinned buffer, and the grouped contraction stages its tables
  // through one of its own: `pin` is still the buffer sized above, and the upload from it has completed by stream order)
  BK_HIP(hipMemcpyAsync(pin, dD, (size_t)down_doubles * sizeof(double), hipMemcpyDeviceToHost, st));
  BK_HIP(hipStreamSynchronize(st));

  // ---- original units: D sd(y) / sd(x_j) (R/bigKRLS.R:393-407), its group means; cov[e, f] = a_e a_f M[e, f] -------------
  for (int64_t jj = 0; jj < nj; ++jj) {
    const int64_t j = mp.cols[jj];
    double* col = pin + jj * u;
    std::vector<long double> s((size_t)G, 0.0L);
    for (int64_t r = 0; r < u; ++r) {
      col[r] = (mp.y_sd * col[r]) / mp.x_sd[j];
      s[(size_t)h_group[r]] += col[r];
    }
    for (int64_t g = 0; g < G; ++g)
      h_ame[jj * G + g] = ng[(size_t)g] > 0 ? (double)(s[(size_t)g] / (long double)ng[(size_t)g]) : std::nan("");
    if (h_derivatives) std::memcpy(h_derivatives + jj * u, col, (size_t)u * sizeof(double));
  }
  if (want_cov) {
    std::vector<double> a((size_t)E, 0.0);
    for (int64_t jj = 0; jj < nj; ++jj) {
      const int64_t j = mp.cols[jj];
      const double dz = (mp.hi[j] - mp.x_mean[j]) / mp.x_sd[j] - (mp.lo[j] - mp.x_mean[j]) / mp.x_sd[j];
      for (int64_t g = 0; g < G; ++g) {
        const double den = (double)ng[(size_t)g] * mp.x_sd[j];
        if (ng[(size_t)g] == 0) continue;   // (an empty group: zero rows and columns)
        a[(size_t)(jj * G + g)] = mp.isbin[j] ? std::sqrt(2.0) / (dz * den) : (-2.0 / sigma) / den;
      }
    }
    const double* M = pin + u * nj;
    for (int64_t f = 0; f < E; ++f)
      for (int64_t e = 0; e < E; ++e)
        h_cov[e + f * E] = (a[(size_t)e] * a[(size_t)f]) * (0.5 * (M[e + f * E] + M[f + e * E]));
  }
  return BIGKRLS_OK;
}

}  // extern "C"
