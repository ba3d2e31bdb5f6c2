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
//
// bigkrls_marginal_effects_se(): the standard error of every D[i,j]. D[i,j] = g_ij' c is linear in c with the weights
//   g_ij[k] = Kn[i,k] (r_i + t_i s_k)
//   continuous j: s_k = Xs_kj, r_i = -(2/sigma) Zs_ij, t_i = 2/sigma
//   binary j:     s_k = b_k;  h_i = 1: r_i = sd (1 - 1/E), t_i = sd (1/E - E);  h_i = 0: r_i = -sd (1 - E), t_i = sd (1/E - E)
//                 (sd = 1/(z1 - z0); me_rows_kernel's sd (+-1) ((1 - E) Sc + (1 - 1/E) Oc) written per training row)
// so Var(D[i,j]) = g_ij' V g_ij = sum_m w_m ((G_j Q)[i,m])^2 with G_j = Kn o (r 1' + t s') and V = Q diag(w) Q'. The new
// points go in row blocks of the test kernel (at most 1 GiB, predict_blocks' rule, csrc/fit.hip); per block Kn_b is built
// once and per column T = G_j Q comes from gemm_modulated (csrc/gemm.hip: G_j is never stored) and rowsumsq_weighted
// writes column j of the result. With V as the n x n matrix G_j is stored beside the block and quadform_diag gives the
// diagonal (2 u n^2 flops per column instead of 2 u n k). Original units: se = sqrt(f_j var) / sd(x_j), f_j = 2 for
// binary columns (the reference's factor, as in var_j above): at u = 1, se^2 is var_j.
#include "margeff.h"

namespace bk {
namespace {

// ---- pointwise standard errors (s, r and t: me_se_s_kernel, me_se_rt_kernel, margeff.h) ------------------------------
// G (rows x n, ld rows) = Kn o (r 1' + t s'), the factor as gemm_modulated forms it (dense vcov.est.c only)
__global__ void me_se_modulate_kernel(int rows, int n, const double* __restrict__ Kn, const double* __restrict__ r,
                                      const double* __restrict__ t, const double* __restrict__ s,
                                      double* __restrict__ G) {
  const int64_t total = (int64_t)rows * n;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e % rows);
    const int k = (int)(e / rows);
    G[e] = Kn[e] * fma(t[i], s[k], r[i]);
  }
}

// both entries: vcov.est.c as the n x n matrix, as its factors, or not at all (no variances) -- Vcov, common.h
int marginal_effects_impl(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                          const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                          const double* h_newdata, int64_t u, const Vcov& vc, double* h_derivatives, double* h_avg,
                          double* h_var) {
  BK_TRY(me_check_args(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_newdata, u, h_avg));
  BK_REQUIRE(vc.given() == (h_var != nullptr),
             "marginal_effects: h_var is written exactly when vcov.est.c (or its factors) is given");
  BK_TRY(me_check_factors(vc, n));
  const int64_t k = vc.cols();
  MePrep mp;
  BK_TRY(me_prepare(h_X, n, p, h_y, h_which, n_which, h_newdata, u, &mp));
  const std::vector<int64_t>& cols = mp.cols;
  const std::vector<double>&x_mean = mp.x_mean, &x_sd = mp.x_sd, &lo = mp.lo, &hi = mp.hi;
  const std::vector<char>& isbin = mp.isbin;
  const double y_sd = mp.y_sd;
  const int64_t nj = (int64_t)cols.size(), q = 1 + nj;

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
    me_standardise(mp, h_X, n, p, h_newdata, u, hXs, hZs);
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
      hcols[jj] = mp.col(jj);
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
                     (const double*)dXs, (const MeCol*)dcols, sigma, dS, (int64_t)0, n, (int64_t)0);
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

// bigkrls_marginal_effects_se: vc is the matrix or the factors (exactly one, checked by the entry)
int marginal_effects_se_impl(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                             const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                             const double* h_newdata, int64_t u, const Vcov& vc, int64_t block_rows, double* h_se) {
  BK_TRY(me_check_args(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_newdata, u, h_se));
  BK_REQUIRE(block_rows >= 0 && block_rows % 128 == 0, "marginal_effects_se: block_rows must be 0 or a multiple of 128");
  BK_TRY(me_check_factors(vc, n));
  const int64_t k = vc.cols();
  MePrep mp;
  BK_TRY(me_prepare(h_X, n, p, h_y, h_which, n_which, h_newdata, u, &mp));
  const int64_t nj = (int64_t)mp.cols.size();
  // rows per block: beside the b x n block of the test kernel, T = G_j Q (b x k) or the stored G_j (b x n)
  const int64_t wide = vc.d_Q ? k : n;
  const int64_t b = std::min(block_rows > 0 ? block_rows : pointwise_block_rows(n, wide), u);

  // ---- device layout -------------------------------------------------------------------------------
  hipStream_t st = ctx->stream;
  const int64_t colw = (int64_t)((sizeof(MeCol) + 7) / 8);
  const int64_t up_doubles = n * p + u * p + n + u + nj * colw + k;   // uploaded, in this order
  const int64_t small_doubles = up_doubles + n * nj + 2 * b * nj + u * nj + 64;
  void* psmall = nullptr;
  BK_TRY(ws_get(ctx, SLOT_ME_SMALL, small_doubles * (int64_t)sizeof(double), &psmall));
  double* qd = (double*)psmall;
  double* dXs = qd; qd += n * p;
  double* dZs = qd; qd += u * p;
  double* dnx = qd; qd += n;
  double* dnz = qd; qd += u;
  MeCol* dcols = (MeCol*)qd; qd += nj * colw;
  double* dw = qd; qd += k;
  double* dS = qd; qd += n * nj;
  double* dR = qd; qd += b * nj;
  double* dT = qd; qd += b * nj;
  double* dse = qd; qd += u * nj;
  void* pk = nullptr;
  BK_TRY(ws_get(ctx, SLOT_PP_K, b * (n + wide) * (int64_t)sizeof(double), &pk));
  double* dKn = (double*)pk;
  double* dP = dKn + b * n;   // T = G_j Q, or G_j

  // ---- standardise, squared row norms (the training rows are centred by their standardisation: no further shift),
  //      upload -----------------------------------------------------------------------------------------
  double* pin = nullptr;
  BK_HIP(hipStreamSynchronize(st));   // (the pinned buffer may be reallocated)
  BK_TRY(pinned_get(ctx, std::max(up_doubles, u * nj), &pin));
  {
    double* hXs = pin;
    double* hZs = hXs + n * p;
    double* hnx = hZs + u * p;
    double* hnz = hnx + n;
    MeCol* hcols = (MeCol*)(hnz + u);
    me_standardise(mp, h_X, n, p, h_newdata, u, hXs, hZs);
    auto sqnorms = [p](const double* A, int64_t rows, double* out) {
      for (int64_t i = 0; i < rows; ++i) out[i] = 0.0;
      for (int64_t j = 0; j < p; ++j)
        for (int64_t i = 0; i < rows; ++i) out[i] += A[j * rows + i] * A[j * rows + i];
    };
    sqnorms(hXs, n, hnx);
    sqnorms(hZs, u, hnz);
    for (int64_t jj = 0; jj < nj; ++jj) hcols[jj] = mp.col(jj);
    if (k > 0) std::memcpy((double*)hcols + nj * colw, vc.h_w, (size_t)k * sizeof(double));
    BK_HIP(hipMemcpyAsync(dXs, pin, (size_t)up_doubles * sizeof(double), hipMemcpyHostToDevice, st));
  }
  int blocks = (int)std::min<int64_t>((n * nj + 255) / 256, 4096);
  hipLaunchKernelGGL(me_se_s_kernel, dim3(blocks), dim3(256), 0, st, (int)n, (int)nj, (const double*)dXs,
                     (const MeCol*)dcols, dS);
  BK_CHECK_LAUNCH();

  // ---- row blocks of the new points ---------------------------------------------------------------------
  for (int64_t r0 = 0; r0 < u; r0 += b) {
    const int64_t rows = std::min(b, u - r0);
    BK_TRY(kernel_block_centred(ctx, dZs + r0, rows, u, dnz + r0, dXs, n, n, dnx, p, sigma, dKn, rows, -1));
    blocks = (int)std::min<int64_t>((rows * nj + 255) / 256, 4096);
    hipLaunchKernelGGL(me_se_rt_kernel, dim3(blocks), dim3(256), 0, st, (int)rows, (int)nj, (const double*)(dZs + r0),
                       u, (const MeCol*)dcols, sigma, dR, dT);
    BK_CHECK_LAUNCH();
    for (int64_t jj = 0; jj < nj; ++jj) {
      const double *r = dR + jj * rows, *t = dT + jj * rows, *s = dS + jj * n;
      double* out = dse + jj * u + r0;
      if (vc.d_Q) {
        BK_TRY(gemm_modulated(ctx, rows, k, n, dKn, rows, r, t, s, vc.d_Q, vc.ldq, dP, rows));     // T = G_j Q
        BK_TRY(rowsumsq_weighted(ctx, rows, k, dP, rows, dw, out));
      } else {
        blocks = (int)std::min<int64_t>((rows * n + 255) / 256, 8192);
        hipLaunchKernelGGL(me_se_modulate_kernel, dim3(blocks), dim3(256), 0, st, (int)rows, (int)n,
                           (const double*)dKn, r, t, s, dP);
        BK_CHECK_LAUNCH();
        BK_TRY(quadform_diag(ctx, rows, n, dP, rows, vc.d_V, n, out));                             // diag(G_j V G_j')
      }
    }
  }
  BK_HIP(hipMemcpyAsync(pin, dse, (size_t)(u * nj) * sizeof(double), hipMemcpyDeviceToHost, st));
  BK_HIP(hipStreamSynchronize(st));

  // ---- original units: the variance times (sd(y)/sd(x_j))^2 with V = vcov.est.c / sd(y)^2 -- sd(y)^2 cancels as in
  //      marginal_effects_impl; the factor 2 of the binary columns; a quadratic form that rounds below zero is zero -----
  for (int64_t jj = 0; jj < nj; ++jj) {
    const int64_t j = mp.cols[jj];
    const double scale = (mp.isbin[j] ? 2.0 : 1.0) / (mp.x_sd[j] * mp.x_sd[j]);
    const double* v = pin + jj * u;
    double* se = h_se + jj * u;
    for (int64_t i = 0; i < u; ++i) se[i] = std::sqrt(std::max(scale * v[i], 0.0));
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

int bigkrls_marginal_effects_se(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                                const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                                const double* h_newdata, int64_t u, const double* d_vcov_c, const double* d_Q,
                                int64_t ldq, int64_t k, const double* h_w, int64_t block_rows, double* h_se) {
  BK_REQUIRE((d_vcov_c != nullptr) != (d_Q != nullptr),
             "marginal_effects_se: exactly one of vcov.est.c and its factors must be given");
  return marginal_effects_se_impl(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_which, n_which, h_newdata, u,
                                  d_vcov_c ? Vcov::matrix(d_vcov_c) : Vcov::factors(d_Q, ldq, k, h_w), block_rows, h_se);
}

}  // extern "C"
