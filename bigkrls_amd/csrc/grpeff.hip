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
  BK_TRY(effects_check_args(ctx, "marginal_effects", h_X && h_y && h_coeffs && h_newdata && h_ame, n, p, u, sigma));
  Vcov vc;
  BK_TRY(vcov_forms("group_effects", d_vcov_c, d_Q, ldq, k, h_w, false, &vc));
  BK_REQUIRE(vc.given() == (h_cov != nullptr),
             "group_effects: h_cov is written exactly when vcov.est.c (or its factors) is given");
  BK_TRY(vcov_check_factors("marginal_effects", vc, n));
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

  // ---- device layout (read back: D, then M) -----------------------------------------------------------------------
  hipStream_t st = ctx->stream;
  const bool want_cov = vc.given();
  Layout L;
  const Region Xs = L.up(n * p), Zs = L.up(u * p), nx = L.up(n), nz = L.up(u), B = L.up(n * q), Bs = L.up(u * q),
               cols = L.up_records<MeCol>(nj), w = L.up(kq);
  const Region R = L.dev(u * q), D = L.down(u * nj), M = L.down(want_cov ? E * E : 0);
  BK_TRY(layout_device(ctx, SLOT_ME_SMALL, &L));
  const MeCol* dcols = L.d<MeCol>(cols);
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
  //      me_se_frame's kernel blocks do): no shift by a column mean, whose rounding would depend on the order
  //      of the rows -- the same rows in another order give the same bits ------------------------------------------------
  BK_TRY(layout_pinned(ctx, &L));
  double* pin = L.pinned();
  me_standardise(mp, h_X, n, p, h_newdata, u, L.h(Xs), L.h(Zs));
  host_sqnorms(L.h(Xs), n, p, L.h(nx));
  host_sqnorms(L.h(Zs), u, p, L.h(nz));
  me_fill_operands(mp, h_X, n, h_newdata, u, h_coeffs, L.h(Xs), L.h(Zs), L.h(B), L.h(Bs));
  me_stage_cols(mp, vc, L.h<MeCol>(cols), L.h(w));
  BK_TRY(layout_upload(ctx, L));

  // ---- row side: the pointwise effects ---------------------------------------------------------------------------------
  BK_TRY(kernel_contract_centred(ctx, L.d(Zs), u, u, L.d(nz), L.d(Xs), n, n, L.d(nx), p, sigma, L.d(B), q, n, L.d(R),
                                 u));                                                                  // R = Kn B
  hipLaunchKernelGGL(me_rows_kernel, dim3(launch_blocks(u * nj, 4096)), dim3(256), 0, st, (int)u, (int)nj,
                     (const double*)L.d(R), (const double*)L.d(Zs), (const double*)L.d(Bs), dcols, sigma, L.d(D));
  BK_CHECK_LAUNCH();

  // ---- column side, all groups at once; M = S' V S ----------------------------------------------------------------------
  if (want_cov) {
    BK_TRY(kernel_contract_grouped_centred(ctx, L.d(Xs), n, n, L.d(nx), L.d(Zs), u, u, L.d(nz), p, sigma, L.d(Bs), q, u,
                                           h_group, G, dC, n));                                       // all C_g
    const dim3 grid(launch_blocks(n * nj, 1024), (unsigned)G);
    hipLaunchKernelGGL(me_cols_kernel, grid, dim3(256), 0, st, (int)n, (int)nj, (const double*)dC,
                       (const double*)L.d(Xs), dcols, sigma, dS, n * q, G * n, n);
    BK_CHECK_LAUNCH();
    if (vc.d_Q) {
      BK_TRY(gemm(ctx, 1, 0, kq, E, n, 1.0, vc.d_Q, vc.ldq, dS, n, 0.0, dC, kq));      // T = Q' S
      BK_TRY(gram_weighted(ctx, kq, E, dC, kq, L.d(w), L.d(M), E));                    // M = T' diag(w) T
    } else {
      BK_TRY(gemm(ctx, 0, 0, n, E, n, 1.0, vc.d_V, n, dS, n, 0.0, dC, n));             // P = vcov.est.c S
      BK_TRY(gemm(ctx, 1, 0, E, E, n, 1.0, dS, n, dC, n, 0.0, L.d(M), E));             // M = S' P
    }
  }
  // (gemm and gram_weighted do not touch the context's pinned buffer, and the grouped contraction stages its tables
  // through one of its own: `pin` is still the buffer sized above, and the upload from it has completed by stream order)
  BK_TRY(layout_download(ctx, L));

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
