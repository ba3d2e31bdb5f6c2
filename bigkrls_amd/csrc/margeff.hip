// bigkrls_marginal_effects(): pointwise marginal effects, their averages and the variances of the averages at new
// data points of a fitted model, without refitting and without the u x n test kernel in memory.
//
// In standardised units (Xs n x p training rows, Zs u x p new rows standardised with the TRAINING means and sds,
// Kn[i,k] = exp(-||Zs_i - Xs_k||^2 / sigma), c the coefficients, V = vcov.est.c / sd(y)^2):
//   continuous column j: D[i,j] = -(2/sigma) sum_k (Zs_ij - Xs_kj) Kn[i,k] c_k,
//                        s_k = sum_i (Zs_ij - Xs_kj) Kn[i,k],            var_j = 4/(sigma^2 u^2) s'V s
//   binary column j (two raw training values, standardised z0 < z1; Kn1 / Kn0: column j of Zs set to z1 / z0):
//                        D[i,j] = (Kn1 - Kn0)[i,:] c / (z1 - z0),  a_k = sum_i (Kn1 - Kn0)[i,k],
//                        var_j = 2/((z1 - z0)^2 u^2) a'V a              (the factor 2: src/bigderiv_v3.cpp:85)
// With newdata = X every one of them is the fit's own (csrc/deriv.hip; R/bigKRLS.R:318-407).
//
// Everything reduces to two contractions over Kn (kernel_contract, csrc/gemm.hip: Kn rebuilt in registers, never
// stored):
//   row side    R = Kn B   (u x q),  B  = [c, {x_j o c | b_j o c}_j]      b_j: training group indicator (raw == max)
//   column side C = Kn' B* (n x q),  B* = [1, {Zs_j | h_j}_j]             h_j: newdata group indicator (raw == max)
// q = 1 + |J|. D is a per-row finalise of R and Zs, s / a a per-row finalise of C and Xs; the binary columns use the
// group-sum algebra of deriv_finalize_kernel (csrc/deriv.hip): Kn1 and Kn0 differ from Kn only by the factors
// E = exp(-(z1 - z0)^2 / sigma) and 1/E on the rows / columns of the other group. The variances are T = V S (gemm)
// and column dots, or -- bigkrls_marginal_effects_factored, V = Q diag(w) Q' given by its factors -- sum_k w_k (q_k'S_j)^2
// (deriv_var, what the fit itself does); the two entries differ in that step only.
// Device memory: O((u + n)(p + q)) plus the loop splits' partials, never O(u n).
#include "hostprep.h"

#include <cstring>

namespace bk {
namespace {

// Per-column constants of the selected columns (device, 4 per column): is_binary, z0, z1 and the column index.
struct MeCol {
  double bin, z0, z1, col;
};

// D (u x nj, ld u): row side. R (u x q, ld u) = Kn B, Zs (u x p, ld u), Bs (u x q) = B* (its binary columns are the
// newdata group indicators h_j).
__global__ void me_rows_kernel(int u, int nj, const double* __restrict__ R, const double* __restrict__ Zs,
                               const double* __restrict__ Bs, const MeCol* __restrict__ cols, double sigma,
                               double* __restrict__ D) {
  const int64_t total = (int64_t)u * nj;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e % u);
    const int jj = (int)(e / u);
    const MeCol cj = cols[jj];
    const double Kc = R[i];
    const double Kvc = R[(int64_t)(1 + jj) * u + i];
    double dv;
    if (cj.bin == 0.0) {
      const double z = Zs[i + (int64_t)cj.col * u];
      dv = (-2.0 / sigma) * (z * Kc - Kvc);
    } else {
      const double sd = 1.0 / (cj.z1 - cj.z0);
      const double phi = -1.0 / (sd * sd * sigma);
      const double E = exp(phi), Einv = exp(-phi);
      const bool hi = Bs[(int64_t)(1 + jj) * u + i] != 0.0;
      const double Sc = hi ? Kvc : Kc - Kvc;     // over the training rows of the point's own group
      const double Oc = hi ? Kc - Kvc : Kvc;     // ... and of the other one
      dv = sd * (hi ? 1.0 : -1.0) * ((1.0 - E) * Sc + (1.0 - Einv) * Oc);
    }
    D[e] = dv;
  }
}

// S (n x nj, ld n): column side. C (n x q, ld n) = Kn' B*, Xs (n x p, ld n). s_k for continuous columns, a_k for
// binary ones (training group of k: Xs == z1, the fit's own test, csrc/deriv.hip).
__global__ void me_cols_kernel(int n, int nj, const double* __restrict__ Cm, const double* __restrict__ Xs,
                               const MeCol* __restrict__ cols, double sigma, double* __restrict__ S) {
  const int64_t total = (int64_t)n * nj;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(e % n);
    const int jj = (int)(e / n);
    const MeCol cj = cols[jj];
    const double T = Cm[k];                                  // sum_i Kn[i,k]
    const double H = Cm[(int64_t)(1 + jj) * n + k];          // sum_i Kn[i,k] Zs_ij, or over the new points with h = 1
    const double x = Xs[k + (int64_t)cj.col * n];
    double sv;
    if (cj.bin == 0.0) {
      sv = H - x * T;
    } else {
      const double sd = 1.0 / (cj.z1 - cj.z0);
      const double phi = -1.0 / (sd * sd * sigma);
      const double E = exp(phi), Einv = exp(-phi);
      sv = (x == cj.z1) ? (1.0 - E) * H + (Einv - 1.0) * (T - H) : (1.0 - Einv) * H + (E - 1.0) * (T - H);
    }
    S[e] = sv;
  }
}

// out[j] = sum_k S[k,j] T[k,j]; one block per column, fixed order
__global__ __launch_bounds__(256) void me_coldot_kernel(int n, const double* __restrict__ S,
                                                        const double* __restrict__ T, double* __restrict__ out) {
  __shared__ double sh[4];
  const double* s = S + (int64_t)blockIdx.x * n;
  const double* t = T + (int64_t)blockIdx.x * n;
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a = fma(s[i], t[i], a);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// both entries: vcov.est.c as the n x n matrix, as its factors, or not at all (no variances) -- Vcov, common.h
int marginal_effects_impl(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                          const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                          const double* h_newdata, int64_t u, const Vcov& vc, double* h_derivatives, double* h_avg,
                          double* h_var) {
  BK_TRY(check_ctx(ctx));
  BK_REQUIRE(h_X && h_y && h_coeffs && h_newdata && h_avg, "marginal_effects: null argument");
  BK_REQUIRE(n > 1 && p > 0 && u > 0 && n < (1ll << 31) && u < (1ll << 31), "marginal_effects: bad dimensions");
  BK_REQUIRE(sigma > 0.0 && std::isfinite(sigma), "marginal_effects: sigma must be a positive scalar");
  BK_REQUIRE(vc.given() == (h_var != nullptr),
             "marginal_effects: h_var is written exactly when vcov.est.c (or its factors) is given");
  if (vc.d_Q) BK_REQUIRE(vc.h_w && vc.k > 0 && vc.k <= n && vc.ldq >= n, "marginal_effects: bad factors of vcov.est.c");
  const int64_t k = vc.cols();
  std::vector<int64_t> cols;
  if (h_which) {
    BK_REQUIRE(n_which > 0, "marginal_effects: which_derivatives is empty");
    for (int64_t i = 0; i < n_which; ++i) {
      BK_REQUIRE(h_which[i] >= 1 && h_which[i] <= p, "which.derivatives must index columns of X");
      cols.push_back(h_which[i] - 1);
    }
  } else {
    for (int64_t j = 0; j < p; ++j) cols.push_back(j);
  }
  const int64_t nj = (int64_t)cols.size(), q = 1 + nj;
  for (int64_t i = 0; i < u * p; ++i)
    BK_REQUIRE(std::isfinite(h_newdata[i]), "marginal_effects: newdata contains missing or infinite values");
  std::vector<double> x_mean(p), x_sd(p), lo(p), hi(p);
  std::vector<char> isbin(p);
  for (int64_t j = 0; j < p; ++j) {
    mean_sd(h_X + j * n, n, &x_mean[j], &x_sd[j]);
    BK_REQUIRE(x_sd[j] > 0.0, "marginal_effects: training column " + std::to_string(j + 1) + " is constant");
    isbin[j] = two_valued(h_X + j * n, n, &lo[j], &hi[j]);
  }
  for (int64_t i = 0; i < nj; ++i) {
    const int64_t j = cols[i];
    if (!isbin[j]) continue;
    const double* z = h_newdata + j * u;
    for (int64_t r = 0; r < u; ++r)
      BK_REQUIRE(z[r] == lo[j] || z[r] == hi[j],
                 "newdata column " + std::to_string(j + 1) +
                     " is binary in the training data; its values must be one of the two training values");
  }
  double y_mean, y_sd;
  mean_sd(h_y, n, &y_mean, &y_sd);
  BK_REQUIRE(y_sd > 0.0, "marginal_effects: y is a constant");

  // ---- device layout -------------------------------------------------------------------------------
  hipStream_t st = ctx->stream;
  const int64_t colw = (int64_t)((sizeof(MeCol) + 7) / 8);
  const int64_t up_doubles = n * p + u * p + n * q + u * q + nj * colw + k;  // uploaded, in this order
  const int64_t small_doubles = up_doubles + u * q + n * q + u * nj + 2 * n * nj + nj + 64;
  void* psmall = nullptr;
  BK_TRY(ws_get(ctx, SLOT_ME_SMALL, small_doubles * (int64_t)sizeof(double), &psmall));
  double* qd = (double*)psmall;
  double* dXs = qd; qd += n * p;
  double* dZs = qd; qd += u * p;
  double* dB = qd; qd += n * q;
  double* dBs = qd; qd += u * q;
  MeCol* dcols = (MeCol*)qd; qd += nj * colw;
  double* dw = qd; qd += k;
  double* dR = qd; qd += u * q;
  double* dC = qd; qd += n * q;
  double* dD = qd; qd += u * nj;
  double* dS = qd; qd += n * nj;
  double* dT = qd; qd += n * nj;
  double* dvar = qd; qd += nj;

  // ---- standardise (training means and sds, as bigkrls_predict), operands, upload ---------------------
  double* pin = nullptr;
  BK_HIP(hipStreamSynchronize(st));   // (the pinned buffer may be reallocated)
  BK_TRY(pinned_get(ctx, std::max(up_doubles, u * nj + nj), &pin));
  {
    double* hXs = pin;
    double* hZs = hXs + n * p;
    double* hB = hZs + u * p;
    double* hBs = hB + n * q;
    MeCol* hcols = (MeCol*)(hBs + u * q);
    for (int64_t j = 0; j < p; ++j) {
      standardise_column(h_X + j * n, n, x_mean[j], x_sd[j], hXs + j * n);
      standardise_column(h_newdata + j * u, u, x_mean[j], x_sd[j], hZs + j * u);
    }
    for (int64_t i = 0; i < n; ++i) hB[i] = h_coeffs[i];
    for (int64_t i = 0; i < u; ++i) hBs[i] = 1.0;
    for (int64_t jj = 0; jj < nj; ++jj) {
      const int64_t j = cols[jj];
      const double* x = h_X + j * n;
      const double* z = h_newdata + j * u;
      double* b = hB + (1 + jj) * n;
      double* bs = hBs + (1 + jj) * u;
      if (isbin[j]) {                                   // group membership on the raw values
        for (int64_t i = 0; i < n; ++i) b[i] = (x[i] == hi[j] ? 1.0 : 0.0) * h_coeffs[i];
        for (int64_t i = 0; i < u; ++i) bs[i] = z[i] == hi[j] ? 1.0 : 0.0;
      } else {
        for (int64_t i = 0; i < n; ++i) b[i] = hXs[j * n + i] * h_coeffs[i];
        std::memcpy(bs, hZs + j * u, (size_t)u * sizeof(double));
      }
      hcols[jj].bin = isbin[j] ? 1.0 : 0.0;
      hcols[jj].z0 = (lo[j] - x_mean[j]) / x_sd[j];
      hcols[jj].z1 = (hi[j] - x_mean[j]) / x_sd[j];
      hcols[jj].col = (double)j;
    }
    if (k > 0) std::memcpy((double*)hcols + nj * colw, vc.h_w, (size_t)k * sizeof(double));
    BK_HIP(hipMemcpyAsync(dXs, pin, (size_t)up_doubles * sizeof(double), hipMemcpyHostToDevice, st));
  }

  // ---- the two fused contractions and their finalise -----------------------------------------------
  BK_TRY(kernel_contract(ctx, dZs, u, u, dXs, n, n, p, sigma, dB, q, n, 0, dR, u));    // R = Kn B
  BK_TRY(kernel_contract(ctx, dZs, u, u, dXs, n, n, p, sigma, dBs, q, u, 1, dC, n));   // C = Kn' B*
  int blocks = (int)std::min<int64_t>((u * nj + 255) / 256, 4096);
  hipLaunchKernelGGL(me_rows_kernel, dim3(blocks), dim3(256), 0, st, (int)u, (int)nj, (const double*)dR,
                     (const double*)dZs, (const double*)dBs, (const MeCol*)dcols, sigma, dD);
  BK_CHECK_LAUNCH();
  blocks = (int)std::min<int64_t>((n * nj + 255) / 256, 4096);
  hipLaunchKernelGGL(me_cols_kernel, dim3(blocks), dim3(256), 0, st, (int)n, (int)nj, (const double*)dC,
                     (const double*)dXs, (const MeCol*)dcols, sigma, dS);
  BK_CHECK_LAUNCH();
  if (vc.d_V) {
    BK_TRY(gemm(ctx, 0, 0, n, nj, n, 1.0, vc.d_V, n, dS, n, 0.0, dT, n));          // T = vcov.est.c S
    hipLaunchKernelGGL(me_coldot_kernel, dim3((unsigned)nj), dim3(256), 0, st, (int)n, (const double*)dS,
                       (const double*)dT, dvar);
    BK_CHECK_LAUNCH();
  }
  // s'(vcov.est.c)s per column. From the factors it is the fit's own step, which returns synchronised with its result
  // on the host (deriv_var stages it through the context's pinned buffer, the one `pin` points into: the upload above
  // has completed by then, and nothing of `pin` is read again before it is overwritten below).
  std::vector<double> qf((size_t)nj, 0.0);
  if (vc.d_Q) {
    const std::vector<double> ones((size_t)nj, 1.0);
    BK_TRY(deriv_var(ctx, vc.d_Q, n, k, vc.ldq, dw, dS, nj, n, ones.data(), qf.data()));
  }
  BK_HIP(hipMemcpyAsync(pin, dD, (size_t)(u * nj) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (vc.d_V) BK_HIP(hipMemcpyAsync(pin + u * nj, dvar, (size_t)nj * sizeof(double), hipMemcpyDeviceToHost, st));
  BK_HIP(hipStreamSynchronize(st));
  if (vc.d_V) std::memcpy(qf.data(), pin + u * nj, (size_t)nj * sizeof(double));

  // ---- original units (R/bigKRLS.R:393-407): D sd(y)/sd(x_j), its column means, var (sd(y)/sd(x_j))^2 -----
  for (int64_t jj = 0; jj < nj; ++jj) {
    const int64_t j = cols[jj];
    double* col = pin + jj * u;
    long double s = 0.0L;
    for (int64_t r = 0; r < u; ++r) {
      col[r] = (y_sd * col[r]) / x_sd[j];
      s += col[r];
    }
    h_avg[jj] = (double)(s / (long double)u);
    if (h_derivatives) std::memcpy(h_derivatives + jj * u, col, (size_t)u * sizeof(double));
    if (h_var) {
      // sd(y)^2 cancels: V = vcov.est.c / sd(y)^2 in standardised units, (sd(y)/sd(x_j))^2 back to the original ones
      const double ud = (double)u;
      double scale;
      if (isbin[j]) {
        const double dz = (hi[j] - x_mean[j]) / x_sd[j] - (lo[j] - x_mean[j]) / x_sd[j];
        scale = 2.0 / (dz * dz * ud * ud);
      } else {
        scale = 4.0 / (sigma * sigma * ud * ud);
      }
      h_var[jj] = scale * qf[jj] / (x_sd[j] * x_sd[j]);
    }
  }
  return BIGKRLS_OK;
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bigkrls_marginal_effects(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                             const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                             const double* h_newdata, int64_t u, const double* d_vcov_c, double* h_derivatives,
                             double* h_avg, double* h_var) {
  return marginal_effects_impl(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_which, n_which, h_newdata, u,
                               Vcov::matrix(d_vcov_c), h_derivatives, h_avg, h_var);
}

int bigkrls_marginal_effects_factored(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                                      const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                                      const double* h_newdata, int64_t u, const double* d_Q, int64_t ldq, int64_t k,
                                      const double* h_w, double* h_derivatives, double* h_avg, double* h_var) {
  return marginal_effects_impl(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_which, n_which, h_newdata, u,
                               Vcov::factors(d_Q, ldq, k, h_w), h_derivatives, h_avg, h_var);
}

}  // extern "C"
