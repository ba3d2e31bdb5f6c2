// Host-side preparation shared by the whole-path entries (csrc/fit.hip, csrc/margeff.hip): the context check, column
// moments as R computes them, the two-valued test and the standardisation. Header-only, so that every user compiles
// the arithmetic with its own translation unit's flags; `static`, so that nothing here joins the exported symbols.
#pragma once
#include "common.h"

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

}  // namespace bk
