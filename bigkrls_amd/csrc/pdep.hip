// bigkrls_partial_dependence(): the partial dependence of the fitted outcome on one predictor at a time -- the mean
// over a reference sample of the prediction with that predictor set to a grid value -- with its covariance over the
// grid, without the u x n test kernel and without one predict() per grid value.
//
// In standardised units (Xs n x p training rows, Zs u x p reference rows standardised with the TRAINING means and sds,
// c the coefficients, Vc = vcov.est.c in the fit's units, vs = (v - mean_j) / sd_j for a raw grid value v of column j):
//   pd_j(v)      = mean(y) + sd(y) a_j(v)' c,     a_j(v)[l] = (1/u) M[l,j] exp(-(vs - Xs[l,j])^2 / sigma)
//   M[l,j]       = sum_i exp(-(||Zs_i - Xs_l||^2 - (Zs[i,j] - Xs[l,j])^2) / sigma)      (column j left out of the distance)
//   cov_j(v, v') = a_j(v)' Vc a_j(v') f,          se_j(v) = sqrt(cov_j(v, v))
// because the Gaussian kernel factorises over the columns: K(z with z_j = vs, x_l) = exp(-(vs - x_lj)^2 / sigma) times
// the kernel of the other columns. f is bigkrls_predict's factor on vcov.est.pred, sqrt(n / neffective) when
// neffective > 0 (R/bigKRLS.R:610-611, quirk Q10), so that the curve's variance is the mean of predict()'s matrix.
// The only O(u n) work is M, one kernel_loo_colsums pass for all selected columns (csrc/gemm.hip); per column an
// elementwise kernel writes A_j (G_j x n, the rows a_j(v_g)'), pd = A_j c (gemv), and the variance is
//   factors Vc = Q diag(w) Q': T = A_j Q (gemm), diag = sum_m w_m T_gm^2 (rowsumsq_weighted), cov = (T diag(w)) T'
//   matrix:                    diag(A_j Vc A_j') (quadform_diag),                              cov = (A_j Vc) A_j'
// O(G n k) or O(G n^2) per column (curve_tail, curvetail.h). Column j of the reference sample is never read for column j's curve.
// Device memory: O((u + n)(p + |J|)) plus the loop splits' partials, and per column A_j (at most 1 GiB) with its product.
#include "curvetail.h"

namespace bk {
namespace {

// A (G x n, ld G): A[g, l] = M[l] exp(-(vs[g] - x[l])^2 / sigma) / u
__global__ void pd_rows_kernel(int G, int n, const double* __restrict__ M, const double* __restrict__ x,
                               const double* __restrict__ vs, double neg_inv_sigma, double inv_u,
                               double* __restrict__ A) {
  const int64_t total = (int64_t)G * n;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int g = (int)(e % G);
    const int l = (int)(e / G);
    const double d = vs[g] - x[l];
    A[e] = M[l] * exp(d * d * neg_inv_sigma) * inv_u;
  }
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bigkrls_partial_dependence(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                               const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                               const double* h_newdata, int64_t u, const double* h_grid, const int64_t* h_grid_off,
                               const double* d_vcov_c, const double* d_Q, int64_t ldq, int64_t k, const double* h_w,
                               double neffective, double* h_pd, double* h_se, double* h_cov) {
  CurveArgs ca;
  BK_TRY(curve_check_args(ctx, "partial_dependence", h_X && h_y && h_coeffs && h_grid && h_grid_off && h_pd, n, p,
                          h_newdata, &u, sigma, d_vcov_c, d_Q, ldq, k, h_w, h_se, h_cov, &ca));

  // ---- the selected columns and their grids ------------------------------------------------------------------
  std::vector<int64_t> cols;
  if (h_which) {
    BK_REQUIRE(n_which > 0, "partial_dependence: which is empty");
    for (int64_t i = 0; i < n_which; ++i) {
      BK_REQUIRE(h_which[i] >= 1 && h_which[i] <= p, "which.derivatives must index columns of X");
      cols.push_back(h_which[i] - 1);
    }
  } else {
    for (int64_t j = 0; j < p; ++j) cols.push_back(j);
  }
  const int64_t nj = (int64_t)cols.size();
  CurvePlan cp;
  BK_TRY(curve_plan("partial_dependence", n, p, nj, h_grid, h_grid_off, h_cov != nullptr, h_newdata, u,
                    [&](int64_t jj) { return "column " + std::to_string(cols[jj] + 1); }, &cp));
  const int64_t T = cp.T;

  // ---- the training moments (as bigkrls_marginal_effects) ----------------------------------------------------
  std::vector<double> x_mean((size_t)p), x_sd((size_t)p);
  for (int64_t j = 0; j < p; ++j) {
    mean_sd(h_X + j * n, n, &x_mean[j], &x_sd[j]);
    BK_REQUIRE(x_sd[j] > 0.0, "partial_dependence: training column " + std::to_string(j + 1) + " is constant");
  }
  double y_mean, y_sd;
  mean_sd(h_y, n, &y_mean, &y_sd);
  BK_REQUIRE(y_sd > 0.0, "partial_dependence: y is a constant");

  // ---- M for all selected columns in one fused pass, then column by column (curve_frame, curvetail.h) ----------
  const double* pin = nullptr;
  BK_TRY(curve_frame(
      ctx, h_X, n, p, h_coeffs, h_newdata, u, x_mean, x_sd, ca, h_cov != nullptr, cp, h_grid, h_grid_off, nj,
      [&](int64_t jj) { return cols[jj]; },
      [&](const double* dZs, const double* dXs, double* dM) {
        return kernel_loo_colsums(ctx, dZs, u, u, dXs, n, n, p, sigma, cols.data(), nj, dM, n);
      },
      [&](int64_t jj, int64_t G, const double* dXs, const double* dvs, const double* dM, double* dA) -> int {
        hipLaunchKernelGGL(pd_rows_kernel, dim3(launch_blocks(G * n, 8192)), dim3(256), 0, ctx->stream, (int)G, (int)n,
                           dM + jj * n, dXs + cols[jj] * n, dvs, -1.0 / sigma, 1.0 / (double)u, dA);
        BK_CHECK_LAUNCH();
        return BIGKRLS_OK;
      },
      &pin));

  // ---- original units; bigkrls_predict's factor on the variance (quirk Q10); a form that rounds below zero is zero ----
  const double f = neffective > 0.0 ? std::sqrt((double)n / neffective) : 1.0;
  for (int64_t i = 0; i < T; ++i) h_pd[i] = pin[i] * y_sd + y_mean;
  if (h_se)
    for (int64_t i = 0; i < T; ++i) h_se[i] = std::sqrt(std::max(f * pin[T + i], 0.0));
  if (h_cov)
    for (int64_t i = 0; i < cp.cov_doubles; ++i) h_cov[i] = f * pin[2 * T + i];
  return BIGKRLS_OK;
}

}  // extern "C"
