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
#include "hostprep.h"

#include <cstring>

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
  BK_TRY(check_ctx(ctx));
  BK_REQUIRE(h_X && h_y && h_coeffs && h_grid && h_grid_off && h_pd, "partial_dependence: null argument");
  if (!h_newdata) u = n;   // the reference sample is the training rows
  BK_REQUIRE(n > 1 && p > 0 && u > 0 && n < (1ll << 31) && u < (1ll << 31), "partial_dependence: bad dimensions");
  BK_REQUIRE(sigma > 0.0 && std::isfinite(sigma), "partial_dependence: sigma must be a positive scalar");
  BK_REQUIRE(!(d_vcov_c && d_Q), "partial_dependence: at most one of vcov.est.c and its factors may be given");
  const Vcov vc = d_vcov_c ? Vcov::matrix(d_vcov_c) : (d_Q ? Vcov::factors(d_Q, ldq, k, h_w) : Vcov());
  BK_REQUIRE(vc.given() || (!h_se && !h_cov),
             "partial_dependence: h_se and h_cov are written only when vcov.est.c (or its factors) is given");
  if (vc.d_Q) BK_REQUIRE(vc.h_w && vc.k > 0 && vc.k <= n && vc.ldq >= n, "partial_dependence: bad factors of vcov.est.c");
  const bool want_var = vc.given() && (h_se || h_cov);
  const int64_t kq = want_var ? vc.cols() : 0;

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
  const int64_t gcap = (1ll << 30) / (8 * n);
  BK_REQUIRE(h_grid_off[0] == 0, "partial_dependence: the grid offsets must start at 0");
  int64_t gmax = 0, cov_doubles = 0;
  for (int64_t jj = 0; jj < nj; ++jj) {
    const int64_t G = h_grid_off[jj + 1] - h_grid_off[jj];
    BK_REQUIRE(G >= 1, "partial_dependence: the grid of column " + std::to_string(cols[jj] + 1) + " is empty");
    BK_REQUIRE(G <= gcap, "partial_dependence: the grid of column " + std::to_string(cols[jj] + 1) + " has " +
                              std::to_string(G) + " values; at most " + std::to_string(gcap) +
                              " fit the 1 GiB block (8 G n <= 2^30 bytes)");
    gmax = std::max(gmax, G);
    cov_doubles += G * G;
  }
  const int64_t T = h_grid_off[nj];
  BK_REQUIRE(T < (1ll << 31), "partial_dependence: too many grid values");
  if (!h_cov) cov_doubles = 0;
  for (int64_t i = 0; i < T; ++i) BK_REQUIRE(std::isfinite(h_grid[i]), "partial_dependence: the grid contains missing or infinite values");
  if (h_newdata)
    for (int64_t i = 0; i < u * p; ++i)
      BK_REQUIRE(std::isfinite(h_newdata[i]), "partial_dependence: newdata contains missing or infinite values");

  // ---- the training moments (as bigkrls_marginal_effects) ----------------------------------------------------
  std::vector<double> x_mean((size_t)p), x_sd((size_t)p);
  for (int64_t j = 0; j < p; ++j) {
    mean_sd(h_X + j * n, n, &x_mean[j], &x_sd[j]);
    BK_REQUIRE(x_sd[j] > 0.0, "partial_dependence: training column " + std::to_string(j + 1) + " is constant");
  }
  double y_mean, y_sd;
  mean_sd(h_y, n, &y_mean, &y_sd);
  BK_REQUIRE(y_sd > 0.0, "partial_dependence: y is a constant");

  // ---- device layout -----------------------------------------------------------------------------------------
  hipStream_t st = ctx->stream;
  const int64_t zs_doubles = h_newdata ? u * p : 0;
  const int64_t up_doubles = n * p + zs_doubles + n + kq + T;   // uploaded, in this order
  const int64_t down_doubles = 2 * T + cov_doubles;             // read back: pd, the variances, the covariance blocks
  void* psmall = nullptr;
  BK_TRY(ws_get(ctx, SLOT_PD_SMALL, (up_doubles + n * nj + down_doubles + 64) * (int64_t)sizeof(double), &psmall));
  double* qd = (double*)psmall;
  double* dXs = qd; qd += n * p;
  double* dZs = h_newdata ? qd : dXs; qd += zs_doubles;
  double* dc = qd; qd += n;
  double* dw = qd; qd += kq;
  double* dvs = qd; qd += T;
  double* dM = qd; qd += n * nj;
  double* dpd = qd; qd += T;
  double* dvar = qd; qd += T;
  double* dcov = qd; qd += cov_doubles;
  // one column's A_j, and beside it T = A_j Q and T diag(w) (factors) or A_j vcov.est.c (matrix, only for the covariance)
  const int64_t wide = !want_var ? 0 : (vc.d_Q ? 2 * kq : (h_cov ? n : 0));
  void* pa = nullptr;
  BK_TRY(ws_get(ctx, SLOT_PD_A, gmax * (n + wide) * (int64_t)sizeof(double), &pa));
  double* dA = (double*)pa;
  double* dP = dA + gmax * n;

  // ---- standardise (training means and sds, as bigkrls_predict), upload ---------------------------------------
  double* pin = nullptr;
  BK_HIP(hipStreamSynchronize(st));   // (the pinned buffer may be reallocated)
  BK_TRY(pinned_get(ctx, std::max(up_doubles, down_doubles), &pin));
  {
    double* hXs = pin;
    double* hZs = hXs + n * p;
    double* hc = hZs + zs_doubles;
    double* hw = hc + n;
    double* hvs = hw + kq;
    for (int64_t j = 0; j < p; ++j) {
      standardise_column(h_X + j * n, n, x_mean[j], x_sd[j], hXs + j * n);
      if (h_newdata) standardise_column(h_newdata + j * u, u, x_mean[j], x_sd[j], hZs + j * u);
    }
    std::memcpy(hc, h_coeffs, (size_t)n * sizeof(double));
    if (kq > 0) std::memcpy(hw, vc.h_w, (size_t)kq * sizeof(double));
    for (int64_t jj = 0; jj < nj; ++jj) {
      const int64_t j = cols[jj], g0 = h_grid_off[jj];
      standardise_column(h_grid + g0, h_grid_off[jj + 1] - g0, x_mean[j], x_sd[j], hvs + g0);
    }
    BK_HIP(hipMemcpyAsync(dXs, pin, (size_t)up_doubles * sizeof(double), hipMemcpyHostToDevice, st));
  }

  // ---- M for all selected columns in one fused pass, then column by column ------------------------------------
  BK_TRY(kernel_loo_colsums(ctx, dZs, u, u, dXs, n, n, p, sigma, cols.data(), nj, dM, n));
  double* dcov_j = dcov;
  for (int64_t jj = 0; jj < nj; ++jj) {
    const int64_t j = cols[jj], g0 = h_grid_off[jj], G = h_grid_off[jj + 1] - g0;
    const int blocks = (int)std::min<int64_t>((G * n + 255) / 256, 8192);
    hipLaunchKernelGGL(pd_rows_kernel, dim3(blocks), dim3(256), 0, st, (int)G, (int)n, (const double*)(dM + jj * n),
                       (const double*)(dXs + j * n), (const double*)(dvs + g0), -1.0 / sigma, 1.0 / (double)u, dA);
    BK_CHECK_LAUNCH();
    BK_TRY(curve_tail(ctx, vc, want_var, G, n, kq, dA, dP, dc, dw, dpd + g0, dvar + g0, h_cov ? dcov_j : nullptr));
    if (h_cov) dcov_j += G * G;
  }
  BK_HIP(hipMemcpyAsync(pin, dpd, (size_t)down_doubles * sizeof(double), hipMemcpyDeviceToHost, st));
  BK_HIP(hipStreamSynchronize(st));

  // ---- original units; bigkrls_predict's factor on the variance (quirk Q10); a form that rounds below zero is zero ----
  const double f = neffective > 0.0 ? std::sqrt((double)n / neffective) : 1.0;
  for (int64_t i = 0; i < T; ++i) h_pd[i] = pin[i] * y_sd + y_mean;
  if (h_se)
    for (int64_t i = 0; i < T; ++i) h_se[i] = std::sqrt(std::max(f * pin[T + i], 0.0));
  if (h_cov)
    for (int64_t i = 0; i < cov_doubles; ++i) h_cov[i] = f * pin[2 * T + i];
  return BIGKRLS_OK;
}

}  // extern "C"
