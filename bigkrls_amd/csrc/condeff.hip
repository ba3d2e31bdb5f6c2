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
  CurveArgs ca;
  BK_TRY(curve_check_args(ctx, "conditional_effects", h_X && h_y && h_coeffs && h_pairs && h_grid && h_grid_off && h_ce,
                          n, p, h_newdata, &u, sigma, d_vcov_c, d_Q, ldq, k, h_w, h_se, h_cov, &ca));

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
  CurvePlan cp;
  BK_TRY(curve_plan("conditional_effects", n, p, m, h_grid, h_grid_off, h_cov != nullptr, h_newdata, u, pair_name, &cp));
  const int64_t T = cp.T;

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

  // ---- the moments of all pairs in one fused pass, then pair by pair (curve_frame, curvetail.h) ------------------
  const double* pin = nullptr;
  BK_TRY(curve_frame(
      ctx, h_X, n, p, h_coeffs, h_newdata, u, x_mean, x_sd, ca, h_cov != nullptr, cp, h_grid, h_grid_off, ne,
      [&](int64_t i) { return h_pairs[2 * i + 1] - 1; },
      [&](const double* dZs, const double* dXs, double* dM) {
        return kernel_loo_moments(ctx, dZs, u, u, dXs, n, n, p, sigma, entries.data(), ne, dM, n);
      },
      [&](int64_t i, int64_t G, const double* dXs, const double* dvs, const double* dM, double* dA) -> int {
        const int64_t j = h_pairs[2 * i] - 1, kk = h_pairs[2 * i + 1] - 1;
        const int type = j == kk ? 1 : (isbin[j] ? 2 : 0);
        const double z0 = (lo[j] - x_mean[j]) / x_sd[j], z1 = (hi[j] - x_mean[j]) / x_sd[j];   // (as standardise_column)
        const double scale = type == 2 ? 1.0 / ((z1 - z0) * (double)u) : 2.0 / (sigma * (double)u);
        hipLaunchKernelGGL(ce_rows_kernel, dim3(launch_blocks(G * n, 8192)), dim3(256), 0, ctx->stream, (int)G, (int)n,
                           type, dM + entry_of[i] * n, dXs + kk * n, dXs + j * n, dvs, -1.0 / sigma, scale, z0, z1, dA);
        BK_CHECK_LAUNCH();
        return BIGKRLS_OK;
      },
      &pin));

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
