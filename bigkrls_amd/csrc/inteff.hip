// bigkrls_interaction_effects(): pointwise interaction effects (cross-derivatives), their averages and the variances of
// the averages at new data points of a fitted model; bigkrls_interaction_effects_se(): their pointwise standard errors.
//
// In the standardised units of csrc/margeff.hip (Kn[i,l] = exp(-||Zs_i - Xs_l||^2 / sigma), c the coefficients,
// V = vcov.est.c / sd(y)^2) the first-order operator of a column j is the modulation of Kn by
//   m_j(i,l) = r_j[i] + t_j[i] s_j[l]        (me_se_rt_kernel, me_se_s_kernel, margeff.h; t_j is constant over i)
// and, the Gaussian kernel being a product over the columns, the second-order operator of a pair (j, k) is
//   G_jk = Kn o m_j o m_k - (2/sigma) delta_jk Kn,        I[i,(j,k)] = G_jk[i,:] c
// continuous x continuous: the cross-derivative (j = k: the second derivative, hence the delta term); binary x continuous:
// the derivative in x_k of the first difference in x_j; binary x binary, j != k: the second difference over the two
// pairs of training values. A pair (j, j) on a binary column is not defined.
//
// Values, averages and the variances of the averages never form the u x n kernel: two kernel_contract calls
// (csrc/gemm.hip), as bigkrls_marginal_effects. With J' the columns that occur in any pair and tau_j = t_j:
//   row side    R = Kn [c, {s_j o c}_J', {s_j o s_k o c}_pairs]   (u x q, q = 1 + |J'| + m)
//               I = r_j r_k R_0 + r_j tau_k R_k + tau_j r_k R_j + tau_j tau_k R_jk - (2/sigma) delta_jk R_0
//   column side C = Kn' [1, {r_j}_J', {r_j o r_k}_pairs]          (n x q)
//               S[:,jk] = 1' G_jk = C_jk + tau_k s_k o C_j + tau_j s_j o C_k + tau_j tau_k s_j o s_k o C_0 - (2/sigma) delta_jk C_0
// var.avg = f_jk s'V s / u^2 from the matrix (gemm and column dots) or from the factors (deriv_var), f_jk = 2 when a
// column of the pair is binary (the reference's factor, src/bigderiv_v3.cpp:85, once), else 1.
// Device memory: O((u + n)(p + q)) plus the contractions' partials.
//
// The standard errors take the new points in row blocks as bigkrls_marginal_effects_se does: per block Kn_b once, and per
// pair T = G_jk Q by gemm_modulated2 (G_jk is never stored) and rowsumsq_weighted, or -- vcov.est.c as the matrix -- G_jk
// written beside the block, with the GEMM's fma expression, and quadform_diag.
// Original units: values times sd(y) / (sd(x_j) sd(x_k)); se = sqrt(f_jk var) / (sd(x_j) sd(x_k)) with vcov.est.c itself.
#include "margeff.h"

namespace bk {
namespace {

// a pair by the positions of its columns among the selected ones (J')
struct IePair {
  int a, b;
};

// out (rows x (1 + nj + m), ld rows) = [base, {V_a o base}, {V_a o V_b o base}_pairs]; base == nullptr: ones.
// V (rows x nj, ld ldv).
__global__ void ie_operand_kernel(int rows, int nj, int m, const double* __restrict__ V, int64_t ldv,
                                  const IePair* __restrict__ pairs, const double* __restrict__ base,
                                  double* __restrict__ out) {
  const int64_t total = (int64_t)rows * (1 + nj + m);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e % rows);
    const int col = (int)(e / rows);
    const double b = base ? base[i] : 1.0;
    double v;
    if (col == 0) {
      v = b;
    } else if (col <= nj) {
      v = V[i + (int64_t)(col - 1) * ldv] * b;
    } else {
      const IePair pr = pairs[col - 1 - nj];
      v = V[i + (int64_t)pr.a * ldv] * V[i + (int64_t)pr.b * ldv] * b;
    }
    out[e] = v;
  }
}

// I (u x m, ld u): row side. Rm (u x q, ld u) = Kn B; R, T (u x nj, ld u): r and t of every new point.
__global__ void ie_rows_kernel(int u, int nj, int m, const double* __restrict__ Rm, const double* __restrict__ R,
                               const double* __restrict__ T, const IePair* __restrict__ pairs, double sigma,
                               double* __restrict__ I) {
  const int64_t total = (int64_t)u * m;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e % u);
    const int pi = (int)(e / u);
    const IePair pr = pairs[pi];
    const double rj = R[i + (int64_t)pr.a * u], rk = R[i + (int64_t)pr.b * u];
    const double tj = T[i + (int64_t)pr.a * u], tk = T[i + (int64_t)pr.b * u];
    const double R0 = Rm[i];
    const double Rj = Rm[i + (int64_t)(1 + pr.a) * u], Rk = Rm[i + (int64_t)(1 + pr.b) * u];
    const double Rjk = Rm[i + (int64_t)(1 + nj + pi) * u];
    double v = rj * rk * R0 + rj * tk * Rk + tj * rk * Rj + tj * tk * Rjk;
    if (pr.a == pr.b) v -= (2.0 / sigma) * R0;
    I[e] = v;
  }
}

// Sv (n x m, ld n): column side, 1' G_jk. Cm (n x q, ld n) = Kn' B*; S (n x nj, ld n): s of every training row; tau:
// the first row of T (stride ldt between columns).
__global__ void ie_cols_kernel(int n, int nj, int m, const double* __restrict__ Cm, const double* __restrict__ S,
                               const double* __restrict__ T, int64_t ldt, const IePair* __restrict__ pairs, double sigma,
                               double* __restrict__ Sv) {
  const int64_t total = (int64_t)n * m;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int l = (int)(e % n);
    const int pi = (int)(e / n);
    const IePair pr = pairs[pi];
    const double sj = S[l + (int64_t)pr.a * n], sk = S[l + (int64_t)pr.b * n];
    const double tj = T[(int64_t)pr.a * ldt], tk = T[(int64_t)pr.b * ldt];
    const double C0 = Cm[l];
    const double Cj = Cm[l + (int64_t)(1 + pr.a) * n], Ck = Cm[l + (int64_t)(1 + pr.b) * n];
    const double Cjk = Cm[l + (int64_t)(1 + nj + pi) * n];
    double v = Cjk + tk * sk * Cj + tj * sj * Ck + tj * tk * sj * sk * C0;
    if (pr.a == pr.b) v -= (2.0 / sigma) * C0;
    Sv[e] = v;
  }
}

// G (rows x n, ld rows) = Kn o F, the factor as gemm_modulated2 forms it (dense vcov.est.c only)
__global__ void ie_se_modulate_kernel(int rows, int n, const double* __restrict__ Kn, const double* __restrict__ r1,
                                      const double* __restrict__ t1, const double* __restrict__ s1,
                                      const double* __restrict__ r2, const double* __restrict__ t2,
                                      const double* __restrict__ s2, double d, double* __restrict__ G) {
  const int64_t total = (int64_t)rows * n;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e % rows);
    const int k = (int)(e / rows);
    G[e] = Kn[e] * fma(fma(t1[i], s1[k], r1[i]), fma(t2[i], s2[k], r2[i]), d);
  }
}

// the pairs ordered (j <= k, 0-based), the columns J' they touch (ascending) and every pair by its positions in J'
struct IePlan {
  std::vector<int64_t> pj, pk;
  std::vector<int64_t> which;     // J', 1-based: me_prepare's h_which
  std::vector<IePair> pos;
};

std::string ie_pair_name(int64_t j, int64_t k) {
  return "(" + std::to_string(j) + ", " + std::to_string(k) + ")";
}

int ie_plan_pairs(const int64_t* h_pairs, int64_t m, int64_t p, IePlan* pl) {
  BK_REQUIRE(h_pairs && m > 0, "interaction_effects: pairs is empty");
  BK_REQUIRE(m < (1ll << 20), "interaction_effects: too many pairs");
  std::vector<char> used((size_t)p, 0);
  for (int64_t i = 0; i < m; ++i) {
    const int64_t a = h_pairs[2 * i], b = h_pairs[2 * i + 1];
    BK_REQUIRE(a >= 1 && a <= p && b >= 1 && b <= p,
               "interaction_effects: pair " + ie_pair_name(a, b) + " must index columns of X");
    pl->pj.push_back(std::min(a, b) - 1);
    pl->pk.push_back(std::max(a, b) - 1);
    used[(size_t)(a - 1)] = used[(size_t)(b - 1)] = 1;
  }
  std::vector<std::pair<int64_t, int64_t>> seen;
  for (int64_t i = 0; i < m; ++i) seen.emplace_back(pl->pj[i], pl->pk[i]);
  std::sort(seen.begin(), seen.end());
  for (int64_t i = 1; i < m; ++i)
    BK_REQUIRE(seen[i] != seen[i - 1], "interaction_effects: pair " +
                                           ie_pair_name(seen[i].first + 1, seen[i].second + 1) +
                                           " is given more than once");
  std::vector<int> where((size_t)p, -1);
  for (int64_t j = 0; j < p; ++j)
    if (used[(size_t)j]) {
      where[(size_t)j] = (int)pl->which.size();
      pl->which.push_back(j + 1);
    }
  for (int64_t i = 0; i < m; ++i) pl->pos.push_back(IePair{where[(size_t)pl->pj[i]], where[(size_t)pl->pk[i]]});
  return BIGKRLS_OK;
}

// after me_prepare: a pair (j, j) needs a continuous column
int ie_check_diagonals(const IePlan& pl, const MePrep& mp) {
  for (size_t i = 0; i < pl.pj.size(); ++i)
    BK_REQUIRE(!(pl.pj[i] == pl.pk[i] && mp.isbin[(size_t)pl.pj[i]]),
               "interaction_effects: pair " + ie_pair_name(pl.pj[i] + 1, pl.pk[i] + 1) + " is not defined: column " +
                   std::to_string(pl.pj[i] + 1) + " is binary in the training data");
  return BIGKRLS_OK;
}

// f_jk / (sd(x_j) sd(x_k))^2: the variance of pair i in original units from its standardised quadratic form
double ie_var_scale(const IePlan& pl, const MePrep& mp, int64_t i) {
  const int64_t j = pl.pj[(size_t)i], k = pl.pk[(size_t)i];
  const double sdp = mp.x_sd[(size_t)j] * mp.x_sd[(size_t)k];
  return ((mp.isbin[(size_t)j] || mp.isbin[(size_t)k]) ? 2.0 : 1.0) / (sdp * sdp);
}

int interaction_effects_impl(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                             const double* h_coeffs, double sigma, const int64_t* h_pairs, int64_t m,
                             const double* h_newdata, int64_t u, const Vcov& vc, double* h_interactions, double* h_avg,
                             double* h_var) {
  BK_TRY(effects_check_args(ctx, "marginal_effects", h_X && h_y && h_coeffs && h_newdata && h_avg, n, p, u, sigma));
  BK_REQUIRE(vc.given() == (h_var != nullptr),
             "interaction_effects: h_var is written exactly when vcov.est.c (or its factors) is given");
  BK_TRY(vcov_check_factors("marginal_effects", vc, n));
  const int64_t k = vc.cols();
  IePlan pl;
  BK_TRY(ie_plan_pairs(h_pairs, m, p, &pl));
  MePrep mp;
  BK_TRY(me_prepare(h_X, n, p, h_y, pl.which.data(), (int64_t)pl.which.size(), h_newdata, u, &mp));
  BK_TRY(ie_check_diagonals(pl, mp));
  const int64_t nj = (int64_t)mp.cols.size(), q = 1 + nj + m;

  // ---- device layout -------------------------------------------------------------------------------
  hipStream_t st = ctx->stream;
  Layout L;
  const Region Xs = L.up(n * p), Zs = L.up(u * p), c = L.up(n), cols = L.up_records<MeCol>(nj),
               pairs = L.up_records<IePair>(m), w = L.up(k);
  const Region S = L.dev(n * nj);                            // s of the training rows
  const Region R = L.dev(u * nj), T = L.dev(u * nj);         // r, t of the new points
  const Region B = L.dev(n * q), Bs = L.dev(u * q), Rm = L.dev(u * q), Cm = L.dev(n * q);   // operands and products
  const Region I = L.dev(u * m), Sv = L.dev(n * m), Tv = L.dev(n * m), var = L.dev(m);
  BK_TRY(layout_device(ctx, SLOT_ME_SMALL, &L));
  const MeCol* dcols = L.d<MeCol>(cols);
  const IePair* dpairs = L.d<IePair>(pairs);

  // ---- standardise (training means and sds), upload ----------------------------------------------------
  BK_TRY(layout_pinned(ctx, &L, u * m + m));
  double* pin = L.pinned();
  me_standardise(mp, h_X, n, p, h_newdata, u, L.h(Xs), L.h(Zs));
  std::memcpy(L.h(c), h_coeffs, (size_t)n * sizeof(double));
  std::memset(L.h(pairs), 0, (size_t)pairs.len * sizeof(double));
  std::memcpy(L.h(pairs), pl.pos.data(), (size_t)m * sizeof(IePair));
  me_stage_cols(mp, vc, L.h<MeCol>(cols), L.h(w));
  BK_TRY(layout_upload(ctx, L));

  // ---- r, t, s of the selected columns; the operands; the two fused contractions and their finalise ---------
  auto grid_for = [](int64_t total) { return dim3(launch_blocks(total, 4096)); };
  hipLaunchKernelGGL(me_se_s_kernel, grid_for(n * nj), dim3(256), 0, st, (int)n, (int)nj, (const double*)L.d(Xs), dcols,
                     L.d(S));
  BK_CHECK_LAUNCH();
  hipLaunchKernelGGL(me_se_rt_kernel, grid_for(u * nj), dim3(256), 0, st, (int)u, (int)nj, (const double*)L.d(Zs), u,
                     dcols, sigma, L.d(R), L.d(T));
  BK_CHECK_LAUNCH();
  hipLaunchKernelGGL(ie_operand_kernel, grid_for(n * q), dim3(256), 0, st, (int)n, (int)nj, (int)m,
                     (const double*)L.d(S), n, dpairs, (const double*)L.d(c), L.d(B));
  BK_CHECK_LAUNCH();
  hipLaunchKernelGGL(ie_operand_kernel, grid_for(u * q), dim3(256), 0, st, (int)u, (int)nj, (int)m,
                     (const double*)L.d(R), u, dpairs, (const double*)nullptr, L.d(Bs));
  BK_CHECK_LAUNCH();
  BK_TRY(kernel_contract(ctx, L.d(Zs), u, u, L.d(Xs), n, n, p, sigma, L.d(B), q, n, 0, L.d(Rm), u));    // R = Kn B
  BK_TRY(kernel_contract(ctx, L.d(Zs), u, u, L.d(Xs), n, n, p, sigma, L.d(Bs), q, u, 1, L.d(Cm), n));   // C = Kn' B*
  hipLaunchKernelGGL(ie_rows_kernel, grid_for(u * m), dim3(256), 0, st, (int)u, (int)nj, (int)m, (const double*)L.d(Rm),
                     (const double*)L.d(R), (const double*)L.d(T), dpairs, sigma, L.d(I));
  BK_CHECK_LAUNCH();
  hipLaunchKernelGGL(ie_cols_kernel, grid_for(n * m), dim3(256), 0, st, (int)n, (int)nj, (int)m, (const double*)L.d(Cm),
                     (const double*)L.d(S), (const double*)L.d(T), u, dpairs, sigma, L.d(Sv));
  BK_CHECK_LAUNCH();
  if (vc.d_V) {
    BK_TRY(gemm(ctx, 0, 0, n, m, n, 1.0, vc.d_V, n, L.d(Sv), n, 0.0, L.d(Tv), n));          // T = vcov.est.c S
    hipLaunchKernelGGL(me_coldot_kernel, dim3((unsigned)m), dim3(256), 0, st, (int)n, (const double*)L.d(Sv),
                       (const double*)L.d(Tv), L.d(var));
    BK_CHECK_LAUNCH();
  }
  // s'(vcov.est.c)s per pair; from the factors the fit's own step (see marginal_effects_impl on the pinned buffer)
  std::vector<double> qf((size_t)m, 0.0);
  if (vc.d_Q) {
    const std::vector<double> ones((size_t)m, 1.0);
    BK_TRY(deriv_var(ctx, vc.d_Q, n, k, vc.ldq, L.d(w), L.d(Sv), m, n, ones.data(), qf.data()));
  }
  BK_HIP(hipMemcpyAsync(pin, L.d(I), (size_t)(u * m) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (vc.d_V) BK_HIP(hipMemcpyAsync(pin + u * m, L.d(var), (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
  BK_HIP(hipStreamSynchronize(st));
  if (vc.d_V) std::memcpy(qf.data(), pin + u * m, (size_t)m * sizeof(double));

  // ---- original units: I sd(y) / (sd(x_j) sd(x_k)), its column means, var f_jk / (u sd(x_j) sd(x_k))^2 (sd(y)^2
  //      cancels against V = vcov.est.c / sd(y)^2, as in marginal_effects_impl) ------------------------------------
  for (int64_t i = 0; i < m; ++i) {
    const double sdp = mp.x_sd[(size_t)pl.pj[(size_t)i]] * mp.x_sd[(size_t)pl.pk[(size_t)i]];
    double* col = pin + i * u;
    long double s = 0.0L;
    for (int64_t r = 0; r < u; ++r) {
      col[r] = (mp.y_sd * col[r]) / sdp;
      s += col[r];
    }
    h_avg[i] = (double)(s / (long double)u);
    if (h_interactions) std::memcpy(h_interactions + i * u, col, (size_t)u * sizeof(double));
    if (h_var) h_var[i] = ie_var_scale(pl, mp, i) * qf[(size_t)i] / ((double)u * (double)u);
  }
  return BIGKRLS_OK;
}

// vc is the matrix or the factors (exactly one, checked by the entry)
int interaction_effects_se_impl(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                                const double* h_coeffs, double sigma, const int64_t* h_pairs, int64_t m,
                                const double* h_newdata, int64_t u, const Vcov& vc, int64_t block_rows, double* h_se) {
  BK_TRY(effects_check_args(ctx, "marginal_effects", h_X && h_y && h_coeffs && h_newdata && h_se, n, p, u, sigma));
  BK_REQUIRE(block_rows >= 0 && block_rows % 128 == 0,
             "interaction_effects_se: block_rows must be 0 or a multiple of 128");
  BK_TRY(vcov_check_factors("marginal_effects", vc, n));
  IePlan pl;
  BK_TRY(ie_plan_pairs(h_pairs, m, p, &pl));
  MePrep mp;
  BK_TRY(me_prepare(h_X, n, p, h_y, pl.which.data(), (int64_t)pl.which.size(), h_newdata, u, &mp));
  BK_TRY(ie_check_diagonals(pl, mp));
  const int64_t k = vc.cols();
  auto pair = [&](int64_t i, const SeBlock& b, double* out) -> int {
    const IePair pr = pl.pos[(size_t)i];
    const double *r1 = b.R + pr.a * b.rows, *t1 = b.T + pr.a * b.rows, *s1 = b.S + pr.a * n;
    const double *r2 = b.R + pr.b * b.rows, *t2 = b.T + pr.b * b.rows, *s2 = b.S + pr.b * n;
    const double d = pr.a == pr.b ? -2.0 / sigma : 0.0;
    if (vc.d_Q) {
      BK_TRY(gemm_modulated2(ctx, b.rows, k, n, b.Kn, b.rows, r1, t1, s1, r2, t2, s2, d, vc.d_Q, vc.ldq, b.P,
                             b.rows));                                                                 // T = G_jk Q
      return rowsumsq_weighted(ctx, b.rows, k, b.P, b.rows, b.w, out);
    }
    hipLaunchKernelGGL(ie_se_modulate_kernel, dim3(launch_blocks(b.rows * n, 8192)), dim3(256), 0, ctx->stream,
                       (int)b.rows, (int)n, b.Kn, r1, t1, s1, r2, t2, s2, d, b.P);
    BK_CHECK_LAUNCH();
    return quadform_diag(ctx, b.rows, n, b.P, b.rows, vc.d_V, n, out);                                 // diag(G_jk V G_jk')
  };
  return me_se_frame(ctx, mp, h_X, n, p, h_newdata, u, sigma, vc, block_rows, m, pair,
                     [&](int64_t i) { return ie_var_scale(pl, mp, i); }, h_se);
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bigkrls_interaction_effects(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                                const double* h_coeffs, double sigma, const int64_t* h_pairs, int64_t m,
                                const double* h_newdata, int64_t u, const double* d_vcov_c, const double* d_Q,
                                int64_t ldq, int64_t k, const double* h_w, double* h_interactions, double* h_avg,
                                double* h_var) {
  Vcov vc;
  BK_TRY(vcov_forms("interaction_effects", d_vcov_c, d_Q, ldq, k, h_w, false, &vc));
  return interaction_effects_impl(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_pairs, m, h_newdata, u, vc, h_interactions,
                                  h_avg, h_var);
}

int bigkrls_interaction_effects_se(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                                   const double* h_coeffs, double sigma, const int64_t* h_pairs, int64_t m,
                                   const double* h_newdata, int64_t u, const double* d_vcov_c, const double* d_Q,
                                   int64_t ldq, int64_t k, const double* h_w, int64_t block_rows, double* h_se) {
  Vcov vc;
  BK_TRY(vcov_forms("interaction_effects_se", d_vcov_c, d_Q, ldq, k, h_w, true, &vc));
  return interaction_effects_se_impl(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_pairs, m, h_newdata, u, vc, block_rows,
                                     h_se);
}

}  // extern "C"
