// The tail that bigkrls_partial_dependence (csrc/pdep.hip) and bigkrls_conditional_effects (csrc/condeff.hip) share:
// from one curve's rows A (G x n, ld G: the grid values' weights on the coefficients) its values A c, its variances
// diag(A Vc A') and, where asked for, its covariance A Vc A', with Vc = vcov.est.c as the matrix or as its factors.
// Internal and header-only, as hostprep.h.
#pragma once
#include "common.h"

namespace bk {

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

}  // namespace bk
