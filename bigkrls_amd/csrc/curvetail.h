// The frame that bigkrls_partial_dependence (csrc/pdep.hip) and bigkrls_conditional_effects (csrc/condeff.hip) share:
// the entry checks, the plan of the grids, the packed layout, the standardised upload, the loop over the curves and
// the read-back; and the tail of one curve: from its rows A (G x n, ld G: the grid values' weights on the coefficients)
// its values A c, its variances diag(A Vc A') and, where asked for, its covariance A Vc A', with Vc = vcov.est.c as the
// matrix or as its factors. Each entry supplies what differs: its items (columns / pairs) and their names, its moments
// pass, its rows kernel and the conversion to original units. Internal and header-only, as hostprep.h.
#pragma once
#include "hostprep.h"

#include <cstring>

namespace bk {

// the entry checks up to the forms of vcov.est.c, in the entries' order; newdata == nullptr: the reference sample is the
// training rows (*u = n). want_var: a variance is asked for and can be given; kq: the factors' columns then, else 0.
struct CurveArgs {
  Vcov vc;
  bool want_var = false;
  int64_t kq = 0;
};

static inline int curve_check_args(bigkrls_ctx* ctx, const char* who, bool pointers, int64_t n, int64_t p,
                                   const double* h_newdata, int64_t* u, double sigma, const double* d_vcov_c,
                                   const double* d_Q, int64_t ldq, int64_t k, const double* h_w, const double* h_se,
                                   const double* h_cov, CurveArgs* ca) {
  if (!h_newdata) *u = n;
  BK_TRY(effects_check_args(ctx, who, pointers, n, p, *u, sigma));
  BK_TRY(vcov_forms(who, d_vcov_c, d_Q, ldq, k, h_w, false, &ca->vc));
  BK_REQUIRE(ca->vc.given() || (!h_se && !h_cov),
             std::string(who) + ": h_se and h_cov are written only when vcov.est.c (or its factors) is given");
  BK_TRY(vcov_check_factors(who, ca->vc, n));
  ca->want_var = ca->vc.given() && (h_se || h_cov);
  ca->kq = ca->want_var ? ca->vc.cols() : 0;
  return BIGKRLS_OK;
}

// the grids of the m items: grid i is h_grid[h_grid_off[i] .. h_grid_off[i + 1]); at most gcap values each (A_i within
// 1 GiB); T values in all; cov_doubles: the covariance blocks, 0 when none is asked for. name(i): item i in a message.
struct CurvePlan {
  int64_t m = 0, gmax = 0, cov_doubles = 0, T = 0;
};

template <class Name>
int curve_plan(const char* who_c, int64_t n, int64_t p, int64_t m, const double* h_grid, const int64_t* h_grid_off,
               bool want_cov, const double* h_newdata, int64_t u, Name name, CurvePlan* cp) {
  const std::string who = std::string(who_c) + ": ";
  const int64_t gcap = (1ll << 30) / (8 * n);
  BK_REQUIRE(h_grid_off[0] == 0, who + "the grid offsets must start at 0");
  cp->m = m;
  for (int64_t i = 0; i < m; ++i) {
    const int64_t G = h_grid_off[i + 1] - h_grid_off[i];
    BK_REQUIRE(G >= 1, who + "the grid of " + name(i) + " is empty");
    BK_REQUIRE(G <= gcap, who + "the grid of " + name(i) + " has " + std::to_string(G) + " values; at most " +
                              std::to_string(gcap) + " fit the 1 GiB block (8 G n <= 2^30 bytes)");
    cp->gmax = std::max(cp->gmax, G);
    cp->cov_doubles += G * G;
  }
  cp->T = h_grid_off[m];
  BK_REQUIRE(cp->T < (1ll << 31), who + "too many grid values");
  if (!want_cov) cp->cov_doubles = 0;
  for (int64_t i = 0; i < cp->T; ++i)
    BK_REQUIRE(std::isfinite(h_grid[i]), who + "the grid contains missing or infinite values");
  if (h_newdata)
    for (int64_t i = 0; i < u * p; ++i)
      BK_REQUIRE(std::isfinite(h_newdata[i]), who + "newdata contains missing or infinite values");
  return BIGKRLS_OK;
}

// dval (G) = A c. With want_var: dvar (G) = diag(A Vc A') and, dcov != nullptr, dcov (G x G, ld G) = A Vc A':
//   factors Vc = Q diag(w) Q': T = A Q (gemm), diag = sum_m w_m T_gm^2 (rowsumsq_weighted), cov = (T diag(w)) T'
//   matrix:                    diag(A Vc A') (quadform_diag),                              cov = (A Vc) A'
// dc the coefficients (n), dw the weights (kq = vc.cols()) on the device; dP: scratch beside A, G x 2 kq doubles
// (factors), G x n (matrix with dcov), none otherwise.
static inline int curve_tail(bigkrls_ctx* ctx, const Vcov& vc, bool want_var, int64_t G, int64_t n, int64_t kq,
                             const double* dA, double* dP, const double* dc, const double* dw, double* dval,
                             double* dvar, double* dcov) {
  BK_TRY(gemv(ctx, 0, G, n, 1.0, dA, G, dc, 0.0, dval));                                        // A c
  if (!want_var) return BIGKRLS_OK;
  if (vc.d_Q) {
    double* dTw = dP + G * kq;
    BK_TRY(gemm(ctx, 0, 0, G, kq, n, 1.0, dA, G, vc.d_Q, vc.ldq, 0.0, dP, G));                  // T = A Q
    BK_TRY(rowsumsq_weighted(ctx, G, kq, dP, G, dw, dvar));
    if (dcov) {
      BK_TRY(multdiag(ctx, dP, G, kq, G, dw, dTw, G));
      BK_TRY(gemm(ctx, 0, 1, G, G, kq, 1.0, dTw, G, dP, G, 0.0, dcov, G));                      // (T diag(w)) T'
    }
  } else {
    BK_TRY(quadform_diag(ctx, G, n, dA, G, vc.d_V, n, dvar));                                   // diag(A Vc A')
    if (dcov) {
      BK_TRY(gemm(ctx, 0, 0, G, n, n, 1.0, dA, G, vc.d_V, n, 0.0, dP, G));
      BK_TRY(gemm(ctx, 0, 1, G, G, n, 1.0, dP, G, dA, G, 0.0, dcov, G));                        // (A Vc) A'
    }
  }
  return BIGKRLS_OK;
}

// After the checks and the moments: standardise X, newdata and the grids (grid i with the moments of column
// grid_col(i)), upload; moments(dZs, dXs, dM) is the entry's fused O(u n) pass into dM (n x n_moments); then per item
// rows(i, G, dXs, dvs, dM, dA) launches the kernel that writes A_i (G x n, ld G) from the item's standardised grid dvs,
// and curve_tail finishes the curve. Returns with *out pointing at the read-back in standardised units: the values (T),
// the variances (T), the covariance blocks (cov_doubles), one item after the other.
template <class GridCol, class Moments, class Rows>
int curve_frame(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_coeffs,
                const double* h_newdata, int64_t u, const std::vector<double>& x_mean, const std::vector<double>& x_sd,
                const CurveArgs& ca, bool want_cov, const CurvePlan& cp, const double* h_grid, const int64_t* h_grid_off,
                int64_t n_moments, GridCol grid_col, Moments moments, Rows rows, const double** out) {
  const Vcov& vc = ca.vc;
  const int64_t kq = ca.kq, T = cp.T;
  Layout L;
  const Region Xs = L.up(n * p), Zs = h_newdata ? L.up(u * p) : Xs, c = L.up(n), w = L.up(kq), vs = L.up(T);
  const Region M = L.dev(n * n_moments), val = L.down(T), var = L.down(T), cov = L.down(cp.cov_doubles);
  BK_TRY(layout_device(ctx, SLOT_PD_SMALL, &L));
  // one item's A, and beside it T = A Q and T diag(w) (factors) or A vcov.est.c (matrix, only for the covariance)
  const int64_t wide = !ca.want_var ? 0 : (vc.d_Q ? 2 * kq : (want_cov ? n : 0));
  void* pa = nullptr;
  BK_TRY(ws_get(ctx, SLOT_PD_A, cp.gmax * (n + wide) * (int64_t)sizeof(double), &pa));
  double* dA = (double*)pa;
  double* dP = dA + cp.gmax * n;

  // ---- standardise (training means and sds, as bigkrls_predict), upload ---------------------------------------
  BK_TRY(layout_pinned(ctx, &L));
  for (int64_t j = 0; j < p; ++j) {
    standardise_column(h_X + j * n, n, x_mean[j], x_sd[j], L.h(Xs) + j * n);
    if (h_newdata) standardise_column(h_newdata + j * u, u, x_mean[j], x_sd[j], L.h(Zs) + j * u);
  }
  std::memcpy(L.h(c), h_coeffs, (size_t)n * sizeof(double));
  if (kq > 0) std::memcpy(L.h(w), vc.h_w, (size_t)kq * sizeof(double));
  for (int64_t i = 0; i < cp.m; ++i) {
    const int64_t j = grid_col(i), g0 = h_grid_off[i];
    standardise_column(h_grid + g0, h_grid_off[i + 1] - g0, x_mean[j], x_sd[j], L.h(vs) + g0);
  }
  BK_TRY(layout_upload(ctx, L));

  // ---- the moments of all items in one fused pass, then item by item ------------------------------------------
  BK_TRY(moments(L.d(Zs), L.d(Xs), L.d(M)));
  double* dcov_i = L.d(cov);
  for (int64_t i = 0; i < cp.m; ++i) {
    const int64_t g0 = h_grid_off[i], G = h_grid_off[i + 1] - g0;
    BK_TRY(rows(i, G, (const double*)L.d(Xs), (const double*)(L.d(vs) + g0), (const double*)L.d(M), dA));
    BK_TRY(curve_tail(ctx, vc, ca.want_var, G, n, kq, dA, dP, L.d(c), L.d(w), L.d(val) + g0, L.d(var) + g0,
                      want_cov ? dcov_i : nullptr));
    if (want_cov) dcov_i += G * G;
  }
  BK_TRY(layout_download(ctx, L));
  *out = L.pinned();
  return BIGKRLS_OK;
}

}  // namespace bk
