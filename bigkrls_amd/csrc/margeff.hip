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
  BK_TRY(effects_check_args(ctx, "marginal_effects", h_X && h_y && h_coeffs && h_newdata && h_avg, n, p, u, sigma));
  BK_REQUIRE(vc.given() == (h_var != nullptr),
             "marginal_effects: h_var is written exactly when vcov.est.c (or its factors) is given");
  BK_TRY(vcov_check_factors("marginal_effects", vc, n));
  const int64_t k = vc.cols();
  MePrep mp;
  BK_TRY(me_prepare(h_X, n, p, h_y, h_which, n_which, h_newdata, u, &mp));
  const int64_t nj = (int64_t)mp.cols.size(), q = 1 + nj;

  // ---- device layout -------------------------------------------------------------------------------
  hipStream_t st = ctx->stream;
  Layout L;
  const Region Xs = L.up(n * p), Zs = L.up(u * p), B = L.up(n * q), Bs = L.up(u * q), cols = L.up_records<MeCol>(nj),
               w = L.up(k);
  const Region R = L.dev(u * q), C = L.dev(n * q), D = L.dev(u * nj), S = L.dev(n * nj), T = L.dev(n * nj),
               var = L.dev(nj);
  BK_TRY(layout_device(ctx, SLOT_ME_SMALL, &L));
  const MeCol* dcols = L.d<MeCol>(cols);

  // ---- standardise (training means and sds, as bigkrls_predict), operands, upload ---------------------
  BK_TRY(layout_pinned(ctx, &L, u * nj + nj));
  double* pin = L.pinned();
  me_standardise(mp, h_X, n, p, h_newdata, u, L.h(Xs), L.h(Zs));
  me_fill_operands(mp, h_X, n, h_newdata, u, h_coeffs, L.h(Xs), L.h(Zs), L.h(B), L.h(Bs));
  me_stage_cols(mp, vc, L.h<MeCol>(cols), L.h(w));
  BK_TRY(layout_upload(ctx, L));

  // ---- the two fused contractions and their finalise -----------------------------------------------
  BK_TRY(kernel_contract(ctx, L.d(Zs), u, u, L.d(Xs), n, n, p, sigma, L.d(B), q, n, 0, L.d(R), u));    // R = Kn B
  BK_TRY(kernel_contract(ctx, L.d(Zs), u, u, L.d(Xs), n, n, p, sigma, L.d(Bs), q, u, 1, L.d(C), n));   // C = Kn' B*
  hipLaunchKernelGGL(me_rows_kernel, dim3(launch_blocks(u * nj, 4096)), dim3(256), 0, st, (int)u, (int)nj,
                     (const double*)L.d(R), (const double*)L.d(Zs), (const double*)L.d(Bs), dcols, sigma, L.d(D));
  BK_CHECK_LAUNCH();
  hipLaunchKernelGGL(me_cols_kernel, dim3(launch_blocks(n * nj, 4096)), dim3(256), 0, st, (int)n, (int)nj,
                     (const double*)L.d(C), (const double*)L.d(Xs), dcols, sigma, L.d(S), (int64_t)0, n, (int64_t)0);
  BK_CHECK_LAUNCH();
  if (vc.d_V) {
    BK_TRY(gemm(ctx, 0, 0, n, nj, n, 1.0, vc.d_V, n, L.d(S), n, 0.0, L.d(T), n));          // T = vcov.est.c S
    hipLaunchKernelGGL(me_coldot_kernel, dim3((unsigned)nj), dim3(256), 0, st, (int)n, (const double*)L.d(S),
                       (const double*)L.d(T), L.d(var));
    BK_CHECK_LAUNCH();
  }
  // s'(vcov.est.c)s per column. From the factors it is the fit's own step, which returns synchronised with its result
  // on the host (deriv_var stages it through the context's pinned buffer, the one `pin` points into: the upload above
  // has completed by then, and nothing of `pin` is read again before it is overwritten below).
  std::vector<double> qf((size_t)nj, 0.0);
  if (vc.d_Q) {
    const std::vector<double> ones((size_t)nj, 1.0);
    BK_TRY(deriv_var(ctx, vc.d_Q, n, k, vc.ldq, L.d(w), L.d(S), nj, n, ones.data(), qf.data()));
  }
  BK_HIP(hipMemcpyAsync(pin, L.d(D), (size_t)(u * nj) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (vc.d_V) BK_HIP(hipMemcpyAsync(pin + u * nj, L.d(var), (size_t)nj * sizeof(double), hipMemcpyDeviceToHost, st));
  BK_HIP(hipStreamSynchronize(st));
  if (vc.d_V) std::memcpy(qf.data(), pin + u * nj, (size_t)nj * sizeof(double));

  // ---- original units (R/bigKRLS.R:393-407): D sd(y)/sd(x_j), its column means, var (sd(y)/sd(x_j))^2 -----
  for (int64_t jj = 0; jj < nj; ++jj) {
    const int64_t j = mp.cols[jj];
    double* col = pin + jj * u;
    long double s = 0.0L;
    for (int64_t r = 0; r < u; ++r) {
      col[r] = (mp.y_sd * col[r]) / mp.x_sd[j];
      s += col[r];
    }
    h_avg[jj] = (double)(s / (long double)u);
    if (h_derivatives) std::memcpy(h_derivatives + jj * u, col, (size_t)u * sizeof(double));
    if (h_var) {
      // sd(y)^2 cancels: V = vcov.est.c / sd(y)^2 in standardised units, (sd(y)/sd(x_j))^2 back to the original ones
      const double ud = (double)u;
      double scale;
      if (mp.isbin[j]) {
        const double dz = (mp.hi[j] - mp.x_mean[j]) / mp.x_sd[j] - (mp.lo[j] - mp.x_mean[j]) / mp.x_sd[j];
        scale = 2.0 / (dz * dz * ud * ud);
      } else {
        scale = 4.0 / (sigma * sigma * ud * ud);
      }
      h_var[jj] = scale * qf[jj] / (mp.x_sd[j] * mp.x_sd[j]);
    }
  }
  return BIGKRLS_OK;
}

// bigkrls_marginal_effects_se: vc is the matrix or the factors (exactly one, checked by the entry). Original units: the
// variance times (sd(y)/sd(x_j))^2 with V = vcov.est.c / sd(y)^2 -- sd(y)^2 cancels as in marginal_effects_impl; the
// factor 2 of the binary columns.
int marginal_effects_se_impl(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                             const double* h_coeffs, double sigma, const int64_t* h_which, int64_t n_which,
                             const double* h_newdata, int64_t u, const Vcov& vc, int64_t block_rows, double* h_se) {
  BK_TRY(effects_check_args(ctx, "marginal_effects", h_X && h_y && h_coeffs && h_newdata && h_se, n, p, u, sigma));
  BK_REQUIRE(block_rows >= 0 && block_rows % 128 == 0, "marginal_effects_se: block_rows must be 0 or a multiple of 128");
  BK_TRY(vcov_check_factors("marginal_effects", vc, n));
  MePrep mp;
  BK_TRY(me_prepare(h_X, n, p, h_y, h_which, n_which, h_newdata, u, &mp));
  const int64_t k = vc.cols();
  auto column = [&](int64_t jj, const SeBlock& b, double* out) -> int {
    const double *r = b.R + jj * b.rows, *t = b.T + jj * b.rows, *s = b.S + jj * n;
    if (vc.d_Q) {
      BK_TRY(gemm_modulated(ctx, b.rows, k, n, b.Kn, b.rows, r, t, s, vc.d_Q, vc.ldq, b.P, b.rows));     // T = G_j Q
      return rowsumsq_weighted(ctx, b.rows, k, b.P, b.rows, b.w, out);
    }
    hipLaunchKernelGGL(me_se_modulate_kernel, dim3(launch_blocks(b.rows * n, 8192)), dim3(256), 0, ctx->stream,
                       (int)b.rows, (int)n, b.Kn, r, t, s, b.P);
    BK_CHECK_LAUNCH();
    return quadform_diag(ctx, b.rows, n, b.P, b.rows, vc.d_V, n, out);                                 // diag(G_j V G_j')
  };
  auto scale = [&](int64_t jj) {
    const int64_t j = mp.cols[jj];
    return (mp.isbin[j] ? 2.0 : 1.0) / (mp.x_sd[j] * mp.x_sd[j]);
  };
  return me_se_frame(ctx, mp, h_X, n, p, h_newdata, u, sigma, vc, block_rows, (int64_t)mp.cols.size(), column, scale,
                     h_se);
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
