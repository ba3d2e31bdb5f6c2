// Host-side preparation shared by the whole-path entries (csrc/fit.hip, csrc/margeff.hip): the context check, column
// moments as R computes them, the two-valued test and the standardisation; for the post-estimation entries also their
// argument checks, the two forms of vcov.est.c, and the packed layout (layout.h) bound to a workspace slot and the pinned
// buffer. Header-only, so that every user compiles the arithmetic with its own translation unit's flags; `static`, so
// that nothing here joins the exported symbols.
#pragma once
#include "common.h"
#include "layout.h"

#include <algorithm>
#include <cmath>
#include <thread>

namespace bk {

static inline int check_ctx(bigkrls_ctx* ctx) {
  if (!ctx) {
    set_error("null context");
    return BIGKRLS_EINVAL;
  }
  BK_HIP(hipSetDevice(ctx->device));
  return BIGKRLS_OK;
}

// f(j) for the columns j = 0 .. ncols - 1, on up to eight host threads when the columns are long enough to pay for them
// (round 6). The fit's host side -- validation scans, column means / sds in extended precision, standardisation,
// rescaling of the marginal effects -- is O(N P) work per phase, single-threaded in the reference too; at N = 100 000,
// P = 50 it was 30 ms of a 1.55-s fit, at N = 20 000, P = 20 3 ms of 0.395. Every column is independent: the results
// do not depend on the number of threads.
template <class F>
static void for_columns(int64_t ncols, int64_t rows, F&& f) {
  int64_t nt = std::min<int64_t>({ncols, (int64_t)8, (int64_t)std::max(1u, std::thread::hardware_concurrency())});
  if (ncols * rows < 400000 || nt <= 1) {
    for (int64_t j = 0; j < ncols; ++j) f(j);
    return;
  }
  std::vector<std::thread> th;
  th.reserve((size_t)nt - 1);
  for (int64_t t = 1; t < nt; ++t)
    th.emplace_back([&f, t, nt, ncols] { for (int64_t j = t; j < ncols; j += nt) f(j); });
  for (int64_t j = 0; j < ncols; j += nt) f(j);
  for (auto& x : th) x.join();
}

// mean and R's sd() (n - 1 denominator, biganalytics::colsd, R/bigKRLS.R:179,248) of a column
static inline void mean_sd(const double* x, int64_t n, double* mean, double* sd) {
  long double s = 0.0L;
  for (int64_t i = 0; i < n; ++i) s += x[i];
  const long double m = s / (long double)n;
  long double q = 0.0L;
  for (int64_t i = 0; i < n; ++i) {
    const long double dlt = (long double)x[i] - m;
    q += dlt * dlt;
  }
  *mean = (double)m;
  *sd = n > 1 ? (double)std::sqrt((double)(q / (long double)(n - 1))) : 0.0;
}

// exactly two distinct values (R/bigKRLS.R:242, src/bigderiv_v3.cpp:28-31)
static inline bool two_valued(const double* x, int64_t n, double* lo_out, double* hi_out) {
  double lo = x[0], hi = x[0];
  for (int64_t i = 1; i < n; ++i) {
    lo = std::min(lo, x[i]);
    hi = std::max(hi, x[i]);
  }
  *lo_out = lo;
  *hi_out = hi;
  if (lo == hi) return false;
  for (int64_t i = 0; i < n; ++i)
    if (x[i] != lo && x[i] != hi) return false;
  return true;
}

// dst = (src - mean) / sd (R/bigKRLS.R:248-254; predict and marginal effects: the TRAINING mean and sd, :590-597)
static inline void standardise_column(const double* src, int64_t rows, double mean, double sd, double* dst) {
  for (int64_t i = 0; i < rows; ++i) dst[i] = (src[i] - mean) / sd;
}

// rows per block of the pointwise entries (include/bigkrls.h): the largest multiple of 128 whose b x (n + k) doubles
// -- the test-kernel block, and beside it its product with the k factor columns (or, k = n, a second block) -- fit
// 1 GiB, at least 128
static inline int64_t pointwise_block_rows(int64_t n, int64_t k) {
  return std::max<int64_t>(128, ((1ll << 30) / ((n + k) * (int64_t)sizeof(double))) / 128 * 128);
}

// ---- the post-estimation entries -----------------------------------------------------------------------------------
// blocks of 256 threads for `total` elements of a grid-stride kernel, at most `cap`
static inline unsigned launch_blocks(int64_t total, int64_t cap) {
  return (unsigned)std::min<int64_t>((total + 255) / 256, cap);
}

// out[i] = ||A[i, :]||^2 of A (rows x p, ld rows), column after column
static inline void host_sqnorms(const double* A, int64_t rows, int64_t p, double* out) {
  for (int64_t i = 0; i < rows; ++i) out[i] = 0.0;
  for (int64_t j = 0; j < p; ++j)
    for (int64_t i = 0; i < rows; ++i) out[i] += A[j * rows + i] * A[j * rows + i];
}

// the context, the pointers (`pointers`: all that must not be null are not), the dimensions and sigma; u is the number
// of new rows, n where newdata may be null and is
static inline int effects_check_args(bigkrls_ctx* ctx, const char* who, bool pointers, int64_t n, int64_t p, int64_t u,
                                     double sigma) {
  BK_TRY(check_ctx(ctx));
  BK_REQUIRE(pointers, std::string(who) + ": null argument");
  BK_REQUIRE(n > 1 && p > 0 && u > 0 && n < (1ll << 31) && u < (1ll << 31), std::string(who) + ": bad dimensions");
  BK_REQUIRE(sigma > 0.0 && std::isfinite(sigma), std::string(who) + ": sigma must be a positive scalar");
  return BIGKRLS_OK;
}

// vcov.est.c as the n x n matrix, as its factors, or not at all (Vcov, common.h), from the arguments of an entry that
// takes both forms
static inline int vcov_forms(const char* who, const double* d_vcov_c, const double* d_Q, int64_t ldq, int64_t k,
                             const double* h_w, bool required, Vcov* vc) {
  BK_REQUIRE(!(d_vcov_c && d_Q), std::string(who) + ": at most one of vcov.est.c and its factors may be given");
  BK_REQUIRE(!required || d_vcov_c || d_Q, std::string(who) + ": exactly one of vcov.est.c and its factors must be given");
  *vc = d_vcov_c ? Vcov::matrix(d_vcov_c) : (d_Q ? Vcov::factors(d_Q, ldq, k, h_w) : Vcov());
  return BIGKRLS_OK;
}

static inline int vcov_check_factors(const char* who, const Vcov& vc, int64_t n) {
  if (vc.d_Q)
    BK_REQUIRE(vc.h_w && vc.k > 0 && vc.k <= n && vc.ldq >= n, std::string(who) + ": bad factors of vcov.est.c");
  return BIGKRLS_OK;
}

// the layout's slot ...
static inline int layout_device(bigkrls_ctx* ctx, int slot, Layout* L) {
  BK_REQUIRE(L->valid() && L->down_adjacent(), "internal: a packed layout is out of order");
  void* base = nullptr;
  BK_TRY(ws_get(ctx, slot, L->slot_doubles() * (int64_t)sizeof(double), &base));
  L->bind_device(base);
  return BIGKRLS_OK;
}

// ... its staging area in the context's pinned buffer, which also takes what is read back (`down_doubles`: at least
// the layout's own) ...
static inline int layout_pinned(bigkrls_ctx* ctx, Layout* L, int64_t down_doubles = 0) {
  double* pin = nullptr;
  BK_HIP(hipStreamSynchronize(ctx->stream));   // (the pinned buffer may be reallocated)
  BK_TRY(pinned_get(ctx, std::max({L->up_doubles(), L->down_doubles(), down_doubles}), &pin));
  L->bind_host(pin);
  return BIGKRLS_OK;
}

// ... the ONE upload of everything staged, and the ONE read-back of the adjacent regions marked for it (to the start
// of the pinned buffer, synchronised)
static inline int layout_upload(bigkrls_ctx* ctx, const Layout& L) {
  BK_HIP(hipMemcpyAsync(L.d(Region()), L.pinned(), (size_t)L.up_doubles() * sizeof(double), hipMemcpyHostToDevice,
                        ctx->stream));
  return BIGKRLS_OK;
}

static inline int layout_download(bigkrls_ctx* ctx, const Layout& L) {
  BK_HIP(hipMemcpyAsync(L.pinned(), L.d(Region{L.down_off(), 0}), (size_t)L.down_doubles() * sizeof(double),
                        hipMemcpyDeviceToHost, ctx->stream));
  BK_HIP(hipStreamSynchronize(ctx->stream));
  return BIGKRLS_OK;
}

}  // namespace bk
