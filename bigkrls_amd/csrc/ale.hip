// bigkrls_accumulated_effects(): the accumulated local effects (ALE, Apley & Zhu) of the fitted outcome on one predictor
// at a time -- per bin of x_j the mean change of the prediction over the rows that FALL INTO that bin when x_j moves
// from the bin's lower to its upper edge, accumulated over the bins and centred -- with its covariance over the edges.
// Where the partial dependence (csrc/pdep.hip) averages predictions at rewritten rows the data never contain, every term
// here stays inside a bin of the reference sample.
//
// In standardised units (the notation of csrc/pdep.hip; zs the edges z_0 < ... < z_B of column j standardised with the
// training moments; b(i) = the smallest b >= 1 with Z[i,j] <= z_b, a row equal to z_0 in bin 1; n_b rows in bin b):
//   M_j[l,b]   = sum_{i: b(i) = b} exp(-(||Zs_i - Xs_l||^2 - (Zs[i,j] - Xs[l,j])^2) / sigma)     (column j left out)
//   phi_j(v,l) = exp(-(vs - Xs[l,j])^2 / sigma)
//   D_j[b,l]   = M_j[l,b] (phi_j(z_b,l) - phi_j(z_{b-1},l)) / n_b        local effect of bin b = sd(y) D_j[b,:] c
//   g(z_k)     = sum_{b <= k} local_b,  g(z_0) = 0
//   ale_j(z_k) = g(z_k) - (1/u) sum_b n_b (g(z_{b-1}) + g(z_b)) / 2      (ALEPlot's centring)
// because the Gaussian kernel factorises over the columns: the curve is linear in the coefficients, ale_j = sd(y) A_j c
// with A_j = (I - 1 w') Cum D_j ((B + 1) x n), and cov_j = f A_j Vc A_j' -- curve_frame's tail (curvetail.h) from either
// form of vcov.est.c, f bigkrls_predict's factor as in bigkrls_partial_dependence. The only O(u n) work is M, ONE
// kernel_loo_binsums pass for all selected columns and bins (csrc/gemm.hip); per column one elementwise kernel writes
// A_j: per training row a serial loop over the bins for D, the running sum and the centring.
// The bins' counts reach the device behind the moments, as kernel arguments (no copy, no synchronisation).
#include "curvetail.h"

#include <algorithm>

namespace bk {
namespace {

// A ((B + 1) x n, ld B + 1) from M (n x B, ld n: this column's bins), the column x of Xs, the standardised edges vs and
// the counts cnt (B doubles): one thread per training row
__global__ void ale_rows_kernel(int B, int n, const double* __restrict__ M, const double* __restrict__ x,
                                const double* __restrict__ vs, const double* __restrict__ cnt, double neg_inv_sigma,
                                double inv_u, double* __restrict__ A) {
  for (int l = blockIdx.x * blockDim.x + threadIdx.x; l < n; l += gridDim.x * blockDim.x) {
    const double xl = x[l];
    double* a = A + (int64_t)l * (B + 1);
    double d = vs[0] - xl;
    double phi_prev = exp(d * d * neg_inv_sigma), g = 0.0, mean = 0.0;
    a[0] = 0.0;
    for (int b = 1; b <= B; ++b) {
      d = vs[b] - xl;
      const double phi = exp(d * d * neg_inv_sigma), nb = cnt[b - 1];
      const double gn = g + M[l + (int64_t)(b - 1) * n] * (phi - phi_prev) / nb;
      mean += nb * 0.5 * (g + gn);
      a[b] = gn;
      g = gn;
      phi_prev = phi;
    }
    mean *= inv_u;
    for (int b = 0; b <= B; ++b) a[b] -= mean;
  }
}

// up to ALE_INLINE values per launch, as a kernel argument
constexpr int ALE_INLINE = 256;
struct AleInline {
  double v[ALE_INLINE];
};
__global__ void ale_values_kernel(AleInline t, int count, double* __restrict__ dst) {
  const int i = threadIdx.x;
  if (i < count) dst[i] = t.v[i];
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bigkrls_accumulated_effects(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                                const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                                const double* h_newdata, int64_t u, const double* h_edges, const int64_t* h_grid_off,
                                const double* d_vcov_c, const double* d_Q, int64_t ldq, int64_t k, const double* h_w,
                                double neffective, double* h_ale, double* h_se, double* h_cov) {
  CurveArgs ca;
  BK_TRY(curve_check_args(ctx, "accumulated_effects", h_X && h_y && h_coeffs && h_edges && h_grid_off && h_ale, n, p,
                          h_newdata, &u, sigma, d_vcov_c, d_Q, ldq, k, h_w, h_se, h_cov, &ca));

  // ---- the selected columns and their edges ------------------------------------------------------------------
  std::vector<int64_t> cols;
  if (h_which) {
    BK_REQUIRE(n_which > 0, "accumulated_effects: which is empty");
    for (int64_t i = 0; i < n_which; ++i) {
      BK_REQUIRE(h_which[i] >= 1 && h_which[i] <= p, "which.derivatives must index columns of X");
      cols.push_back(h_which[i] - 1);
    }
  } else {
    for (int64_t j = 0; j < p; ++j) cols.push_back(j);
  }
  const int64_t nj = (int64_t)cols.size();
  auto name = [&](int64_t jj) { return "column " + std::to_string(cols[jj] + 1); };
  BK_REQUIRE(h_grid_off[0] == 0, "accumulated_effects: the grid offsets must start at 0");
  for (int64_t jj = 0; jj < nj; ++jj) {
    const int64_t g0 = h_grid_off[jj], G = h_grid_off[jj + 1] - g0;
    BK_REQUIRE(G >= 2, "accumulated_effects: " + name(jj) + " has " + std::to_string(std::max<int64_t>(G, 0)) +
                           " edges; a bin needs 2");
    for (int64_t g = 0; g < G; ++g)
      BK_REQUIRE(std::isfinite(h_edges[g0 + g]), "accumulated_effects: edge " + std::to_string(g + 1) + " of " + name(jj) +
                                                     " is missing or infinite");
    for (int64_t g = 1; g < G; ++g)
      BK_REQUIRE(h_edges[g0 + g] > h_edges[g0 + g - 1], "accumulated_effects: the edges of " + name(jj) +
                                                            " are not strictly increasing at bin " + std::to_string(g));
  }
  CurvePlan cp;
  BK_TRY(curve_plan("accumulated_effects", n, p, nj, h_edges, h_grid_off, h_cov != nullptr, h_newdata, u, name, &cp));
  const int64_t T = cp.T, nbt = T - nj;   // all edges; all bins

  // ---- the bin of every reference row under every selected column, from the RAW column and edges ---------------
  std::vector<int64_t> labels((size_t)(u * nj)), nbins((size_t)nj), bin_off((size_t)nj + 1, 0);
  std::vector<double> counts((size_t)nbt, 0.0);
  const double* Z = h_newdata ? h_newdata : h_X;
  for (int64_t jj = 0; jj < nj; ++jj) {
    const int64_t g0 = h_grid_off[jj], B = h_grid_off[jj + 1] - g0 - 1;
    const double* e = h_edges + g0;
    const double* z = Z + cols[jj] * u;
    nbins[(size_t)jj] = B;
    bin_off[(size_t)jj + 1] = bin_off[(size_t)jj] + B;
    double* cnt = counts.data() + bin_off[(size_t)jj];
    for (int64_t i = 0; i < u; ++i) {
      BK_REQUIRE(z[i] >= e[0] && z[i] <= e[B], "accumulated_effects: reference row " + std::to_string(i + 1) + " of " + name(jj) +
                                                   " lies outside the edges [" + std::to_string(e[0]) + ", " +
                                                   std::to_string(e[B]) + "]");
      const int64_t b = std::max<int64_t>(1, std::lower_bound(e, e + B + 1, z[i]) - e);   // the smallest b >= 1 with z <= z_b
      labels[(size_t)(i + jj * u)] = b - 1;
      cnt[b - 1] += 1.0;
    }
    for (int64_t b = 0; b < B; ++b)
      BK_REQUIRE(cnt[b] > 0.0, "accumulated_effects: bin " + std::to_string(b + 1) + " of " + name(jj) +
                                   " holds no reference row");
  }

  // ---- the training moments (as bigkrls_marginal_effects) ----------------------------------------------------
  std::vector<double> x_mean((size_t)p), x_sd((size_t)p);
  for (int64_t j = 0; j < p; ++j) {
    mean_sd(h_X + j * n, n, &x_mean[j], &x_sd[j]);
    BK_REQUIRE(x_sd[j] > 0.0, "accumulated_effects: training column " + std::to_string(j + 1) + " is constant");
  }
  double y_mean, y_sd;
  mean_sd(h_y, n, &y_mean, &y_sd);
  BK_REQUIRE(y_sd > 0.0, "accumulated_effects: y is a constant");

  // ---- M for all columns and bins in one fused pass, the counts behind it; then column by column (curve_frame) ----
  const int64_t count_cols = (nbt + n - 1) / n;   // whole columns of the moments' buffer that hold the counts
  const double* pin = nullptr;
  BK_TRY(curve_frame(
      ctx, h_X, n, p, h_coeffs, h_newdata, u, x_mean, x_sd, ca, h_cov != nullptr, cp, h_edges, h_grid_off,
      nbt + count_cols, [&](int64_t jj) { return cols[jj]; },
      [&](const double* dZs, const double* dXs, double* dM) -> int {
        for (int64_t b0 = 0; b0 < nbt; b0 += ALE_INLINE) {
          AleInline t;
          const int64_t cnt = std::min<int64_t>(ALE_INLINE, nbt - b0);
          std::memcpy(t.v, counts.data() + b0, (size_t)cnt * sizeof(double));
          hipLaunchKernelGGL(ale_values_kernel, dim3(1), dim3(ALE_INLINE), 0, ctx->stream, t, (int)cnt, dM + n * nbt + b0);
          BK_CHECK_LAUNCH();
        }
        return kernel_loo_binsums(ctx, dZs, u, u, dXs, n, n, p, sigma, cols.data(), nj, labels.data(), nbins.data(), dM, n);
      },
      [&](int64_t jj, int64_t G, const double* dXs, const double* dvs, const double* dM, double* dA) -> int {
        hipLaunchKernelGGL(ale_rows_kernel, dim3(launch_blocks(n, 4096)), dim3(256), 0, ctx->stream, (int)(G - 1), (int)n,
                           dM + bin_off[(size_t)jj] * n, dXs + cols[jj] * n, dvs, dM + n * nbt + bin_off[(size_t)jj],
                           -1.0 / sigma, 1.0 / (double)u, dA);
        BK_CHECK_LAUNCH();
        return BIGKRLS_OK;
      },
      &pin));

  // ---- original units (centred: no mean(y)); the variance as bigkrls_partial_dependence scales its own ---------
  const double f = neffective > 0.0 ? std::sqrt((double)n / neffective) : 1.0;
  for (int64_t i = 0; i < T; ++i) h_ale[i] = pin[i] * y_sd;
  if (h_se)
    for (int64_t i = 0; i < T; ++i) h_se[i] = std::sqrt(std::max(f * pin[T + i], 0.0));
  if (h_cov)
    for (int64_t i = 0; i < cp.cov_doubles; ++i) h_cov[i] = f * pin[2 * T + i];
  return BIGKRLS_OK;
}

}  // extern "C"
