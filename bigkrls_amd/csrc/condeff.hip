// bigkrls_conditional_effects(): the marginal effect of one predictor along a moderator -- for every pair (j, k) and
// every grid value v of x_k, the mean over a reference sample of the marginal effect of x_j evaluated with x_k set to v --
// with its covariance over the grid, without one bigkrls_marginal_effects call on u rewritten rows per grid value.
//
// In standardised units (Xs n x p training rows, Zs u x p reference rows standardised with the TRAINING means and sds,
// c the coefficients, V = vcov.est.c in the fit's units, vs = (v - mean_k) / sd_k, E_k(v)[l] = exp(-(vs - Xs[l,k])^2 / sigma),
// Kn_{-S}[i,l] the test kernel with the columns in S left out of the distance): CE_jk(v) = a_jk(v)' c with
//   continuous j, k != j: a[l] = (2 / (sigma u)) E_k(v)[l] M1[l],                  M1[l] = sum_i (Xs[l,j] - Zs[i,j]) Kn_{-k}[i,l]
//   continuous j, k == j: a[l] = (2 / (sigma u)) E_j(v)[l] (Xs[l,j] - vs) M0[l],   M0[l] = sum_i Kn_{-j}[i,l]
//   binary j (first difference between its two training values z0 < z1, standardised), k != j:
//                         a[l] = E_k(v)[l] (exp(-(z1 - Xs[l,j])^2 / sigma) - exp(-(z0 - Xs[l,j])^2 / sigma)) / (z1 - z0) M2[l] / u,
//                                                                                  M2[l] = sum_i Kn_{-j,-k}[i,l]
//   cov_jk(v, v') = f_j a(v)' V a(v'),  f_j = 2 for binary j (the reference's factor, src/bigderiv_v3.cpp:85), else 1
// because the Gaussian kernel factorises over the columns. Original units as bigkrls_marginal_effects: values times
// sd(y) / sd(x_j), variances times 1 / sd(x_j)^2; for every pair and every v they are avgderivatives and
// var.avgderivatives of bigkrls_marginal_effects on the reference rows with column k set to v.
// The only O(u n) work is M0 / M1 / M2: ONE kernel_loo_moments pass for all pairs (csrc/gemm.hip; kinds 0 / 1 / 2, the
// entries deduplicated); per pair an elementwise kernel writes A_jk (G x n) and curve_tail (curvetail.h, shared with
// bigkrls_partial_dependence) gives the values, the variances and the covariance. Column k of the reference rows is
// never read, nor column j for a binary j.
// Device memory: O((u + n)(p + entries)) plus the loop splits' partials, and per pair A_jk (at most 1 GiB) with its product.
#include "curvetail.h"
#include "hostprep.h"

#include <cstring>

namespace bk {
namespace {

// A (G x n, ld G) of one pair. type 0: continuous j, k != j; 1: k == j; 2: binary j. M: the pair's moment (n);
// xk, xj: columns k and j of Xs; vs: the standardised grid (G); scale: 2 / (sigma u), or 1 / ((z1 - z0) u) for type 2.
__global__ void ce_rows_kernel(int G, int n, int type, const double* __restrict__ M, const double* __restrict__ xk,
                               const double* __restrict__ xj, const double* __restrict__ vs, double neg_inv_sigma,
                               double scale, double z0, double z1, double* __restrict__ A) {
  const int64_t total = (int64_t)G * n;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int g = (int)(e % G);
    const int l = (int)(e / G);
    const double d = vs[g] - xk[l];
    double a = M[l] * exp(d * d * neg_inv_sigma) * scale;
    if (type == 1) {
      a *= xk[l] - vs[g];
    } else if (type == 2) {
      const double d1 = z1 - xj[l], d0 = z0 - xj[l];
      a *= exp(d1 * d1 * neg_inv_sigma) - exp(d0 * d0 * neg_inv_sigma);
    }
    A[e] = a;
  }
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bigkrls_conditional_effects(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                                const double* h_coeffs, double sigma, const int64_t* h_pairs, int64_t m,
                                const double* h_newdata, int64_t u, const double* h_grid, const int64_t* h_grid_off,
                                const double* d_vcov_c, const double* d_Q, int64_t ldq, int64_t k, const double* h_w,
                                double* h_ce, double* h_se, double* h_cov) {
  BK_TRY(check_ctx(ctx));
  BK_REQUIRE(h_X && h_y && h_coeffs && h_pairs && h_grid && h_grid_off && h_ce, "conditional_effects: null argument");
  if (!h_newdata) u = n;   // the reference sample is the training rows
  BK_REQUIRE(n > 1 && p > 0 && u > 0 && n < (1ll << 31) && u < (1ll << 31), "conditional_effects: bad dimensions");
  BK_REQUIRE(sigma > 0.0 && std::isfinite(sigma), "conditional_effects: sigma must be a positive scalar");
  BK_REQUIRE(!(d_vcov_c && d_Q), "conditional_effects: at most one of vcov.est.c and its factors may be given");
  const Vcov vc = d_vcov_c ? Vcov::matrix(d_vcov_c) : (d_Q ? Vcov::factors(d_Q, ldq, k, h_w) : Vcov());
  BK_REQUIRE(vc.given() || (!h_se && !h_cov),
             "conditional_effects: h_se and h_cov are written only when vcov.est.c (or its factors) is given");
  if (vc.d_Q) BK_REQUIRE(vc.h_w && vc.k > 0 && vc.k <= n && vc.ldq >= n, "conditional_effects: bad factors of vcov.est.c");
  const bool want_var = vc.given() && (h_se || h_cov);
  const int64_t kq = want_var ? vc.cols() : 0;

  // ---- the pairs and their grids -----------------------------------------------------------------------------
  BK_REQUIRE(m > 0 && m < (1ll << 20), "conditional_effects: pairs is empty (or holds 2^20 pairs or more)");
  auto pair_name = [h_pairs](int64_t i) {
    return "pair (" + std::to_string(h_pairs[2 * i]) + ", " + std::to_string(h_pairs[2 * i + 1]) + ")";
  };
  for (int64_t i = 0; i < m; ++i) {
    const int64_t j = h_pairs[2 * i], kk = h_pairs[2 * i + 1];
    BK_REQUIRE(j >= 1 && j <= p && kk >= 1 && kk <= p, "conditional_effects: " + pair_name(i) + " must index columns of X");
    for (int64_t i2 = 0; i2 < i; ++i2)
      BK_REQUIRE(h_pairs[2 * i2] != j || h_pairs[2 * i2 + 1] != kk,
                 "conditional_effects: " + pair_name(i) + " is given more than once");
  }
  const int64_t gcap = (1ll << 30) / (8 * n);
  BK_REQUIRE(h_grid_off[0] == 0, "conditional_effects: the grid offsets must start at 0");
  int64_t gmax = 0, cov_doubles = 0;
  for (int64_t i = 0; i < m; ++i) {
    const int64_t G = h_grid_off[i + 1] - h_grid_off[i];
    BK_REQUIRE(G >= 1, "conditional_effects: the grid of " + pair_name(i) + " is empty");
    BK_REQUIRE(G <= gcap, "conditional_effects: the grid of " + pair_name(i) + " has " + std::to_string(G) +
                              " values; at most " + std::to_string(gcap) + " fit the 1 GiB block (8 G n <= 2^30 bytes)");
    gmax = std::max(gmax, G);
    cov_doubles += G * G;
  }
  const int64_t T = h_grid_off[m];
  BK_REQUIRE(T < (1ll << 31), "conditional_effects: too many grid values");
  if (!h_cov) cov_doubles = 0;
  for (int64_t i = 0; i < T; ++i)
    BK_REQUIRE(std::isfinite(h_grid[i]), "conditional_effects: the grid contains missing or infinite values");
  if (h_newdata)
    for (int64_t i = 0; i < u * p; ++i)
      BK_REQUIRE(std::isfinite(h_newdata[i]), "conditional_effects: newdata contains missing or infinite values");

  // ---- the training moments and the two-valued columns (as bigkrls_marginal_effects) ---------------------------
  std::vector<double> x_mean((size_t)p), x_sd((size_t)p), lo((size_t)p), hi((size_t)p);
  std::vector<char> isbin((size_t)p);
  for (int64_t j = 0; j < p; ++j) {
    mean_sd(h_X + j * n, n, &x_mean[j], &x_sd[j]);
    BK_REQUIRE(x_sd[j] > 0.0, "conditional_effects: training column " + std::to_string(j + 1) + " is constant");
    isbin[j] = two_valued(h_X + j * n, n, &lo[j], &hi[j]);
  }
  double y_mean, y_sd;
  mean_sd(h_y, n, &y_mean, &y_sd);
  BK_REQUIRE(y_sd > 0.0, "conditional_effects: y is a constant");
  for (int64_t i = 0; i < m; ++i) {
    const int64_t j = h_pairs[2 * i] - 1, kk = h_pairs[2 * i + 1] - 1;
    BK_REQUIRE(!(j == kk && isbin[j]), "conditional_effects: " + pair_name(i) + " is not defined: column " +
                                           std::to_string(j + 1) + " is binary in the training data");
    if (!isbin[kk]) continue;
    for (int64_t g = h_grid_off[i]; g < h_grid_off[i + 1]; ++g)
      BK_REQUIRE(h_grid[g] == lo[kk] || h_grid[g] == hi[kk],
                 "conditional_effects: the grid of " + pair_name(i) + ": column " + std::to_string(kk + 1) +
                     " is binary in the training data; its values must be one of the two training values");
  }

  // ---- the entries of the fused pass: kind 1 (continuous j != k), kind 0 (j == k), kind 2 (binary j), deduplicated ----
  std::vector<int64_t> entries;            // (kind, c, j) per entry, 0-based
  std::vector<int64_t> entry_of((size_t)m);
  for (int64_t i = 0; i < m; ++i) {
    const int64_t j = h_pairs[2 * i] - 1, kk = h_pairs[2 * i + 1] - 1;
    const int64_t kind = j == kk ? 0 : (isbin[j] ? 2 : 1), jcol = kind == 0 ? 0 : j;
    int64_t e = 0;
    const int64_t ne = (int64_t)entries.size() / 3;
    while (e < ne && !(entries[3 * e] == kind && entries[3 * e + 1] == kk && entries[3 * e + 2] == jcol)) ++e;
    if (e == ne) entries.insert(entries.end(), {kind, kk, jcol});
    entry_of[i] = e;
  }
  const int64_t ne = (int64_t)entries.size() / 3;

  // ---- device layout -----------------------------------------------------------------------------------------
  hipStream_t st = ctx->stream;
  const int64_t zs_doubles = h_newdata ? u * p : 0;
  const int64_t up_doubles = n * p + zs_doubles + n + kq + T;   // uploaded, in this order
  const int64_t down_doubles = 2 * T + cov_doubles;             // read back: the values, the variances, the covariance blocks
  void* psmall = nullptr;
  BK_TRY(ws_get(ctx, SLOT_PD_SMALL, (up_doubles + n * ne + down_doubles + 64) * (int64_t)sizeof(double), &psmall));
  double* qd = (double*)psmall;
  double* dXs = qd; qd += n * p;
  double* dZs = h_newdata ? qd : dXs; qd += zs_doubles;
  double* dc = qd; qd += n;
  double* dw = qd; qd += kq;
  double* dvs = qd; qd += T;
  double* dM = qd; qd += n * ne;
  double* dce = qd; qd += T;
  double* dvar = qd; qd += T;
  double* dcov = qd; qd += cov_doubles;
  // one pair's A_jk, and beside it T = A Q and T diag(w) (factors) or A vcov.est.c (matrix, only for the covariance)
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
    for (int64_t i = 0; i < m; ++i) {
      const int64_t kk = h_pairs[2 * i + 1] - 1, g0 = h_grid_off[i];
      standardise_column(h_grid + g0, h_grid_off[i + 1] - g0, x_mean[kk], x_sd[kk], hvs + g0);
    }
    BK_HIP(hipMemcpyAsync(dXs, pin, (size_t)up_doubles * sizeof(double), hipMemcpyHostToDevice, st));
  }

  // ---- the moments of all pairs in one fused pass, then pair by pair -------------------------------------------
  BK_TRY(kernel_loo_moments(ctx, dZs, u, u, dXs, n, n, p, sigma, entries.data(), ne, dM, n));
  double* dcov_i = dcov;
  for (int64_t i = 0; i < m; ++i) {
    const int64_t j = h_pairs[2 * i] - 1, kk = h_pairs[2 * i + 1] - 1, g0 = h_grid_off[i], G = h_grid_off[i + 1] - g0;
    const int type = j == kk ? 1 : (isbin[j] ? 2 : 0);
    const double z0 = (lo[j] - x_mean[j]) / x_sd[j], z1 = (hi[j] - x_mean[j]) / x_sd[j];   // (as standardise_column)
    const double scale = type == 2 ? 1.0 / ((z1 - z0) * (double)u) : 2.0 / (sigma * (double)u);
    const int blocks = (int)std::min<int64_t>((G * n + 255) / 256, 8192);
    hipLaunchKernelGGL(ce_rows_kernel, dim3(blocks), dim3(256), 0, st, (int)G, (int)n, type,
                       (const double*)(dM + entry_of[i] * n), (const double*)(dXs + kk * n), (const double*)(dXs + j * n),
                       (const double*)(dvs + g0), -1.0 / sigma, scale, z0, z1, dA);
    BK_CHECK_LAUNCH();
    BK_TRY(curve_tail(ctx, vc, want_var, G, n, kq, dA, dP, dc, dw, dce + g0, dvar + g0, h_cov ? dcov_i : nullptr));
    if (h_cov) dcov_i += G * G;
  }
  BK_HIP(hipMemcpyAsync(pin, dce, (size_t)down_doubles * sizeof(double), hipMemcpyDeviceToHost, st));
  BK_HIP(hipStreamSynchronize(st));

  // ---- original units (bigkrls_marginal_effects'): values sd(y) / sd(x_j), variances 1 / sd(x_j)^2 on vcov.est.c in the
  //      fit's units; the factor 2 of a binary j; a form that rounds below zero is zero -----------------------------------
  const double* cov_in = pin + 2 * T;
  double* cov_out = h_cov;
  for (int64_t i = 0; i < m; ++i) {
    const int64_t j = h_pairs[2 * i] - 1, g0 = h_grid_off[i], G = h_grid_off[i + 1] - g0;
    const double vscale = (isbin[j] ? 2.0 : 1.0) / (x_sd[j] * x_sd[j]);
    for (int64_t g = g0; g < g0 + G; ++g) {
      h_ce[g] = (y_sd * pin[g]) / x_sd[j];
      if (h_se) h_se[g] = std::sqrt(std::max(vscale * pin[T + g], 0.0));
    }
    if (h_cov) {
      for (int64_t e = 0; e < G * G; ++e) cov_out[e] = vscale * cov_in[e];
      cov_in += G * G;
      cov_out += G * G;
    }
  }
  return BIGKRLS_OK;
}

}  // extern "C"
