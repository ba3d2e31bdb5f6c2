// bigkrls_fit() / bigkrls_predict(): the whole hot path behind one C call each.
//
// bigkrls_fit is the numeric body of the reference's bigKRLS() (R/bigKRLS.R:175-470): the
// validation block (:183-240), standardisation (:248-254), step 1 kernel (:262), step 2 eigen
// (:266-269), step 3 lambda search (:271-278), step 4 coefficients / fitted values / variance
// matrices (:280-307), step 5 marginal effects (:321-376) and the rescaling back to the original
// units (:384-445), with every N x N object resident in HBM: the phases of `struct Fit`, run in that order by
// fit_impl, which also owns the one loop that redoes a decomposition. bigkrls_predict is predict.bigKRLS()
// (R/bigKRLS.R:590-621). The host-side arithmetic (means, sds, rescaling) is O(NP).
#include "hostprep.h"

#include <cstring>
#include <limits>

namespace bk {

namespace {

const double kNaN = std::numeric_limits<double>::quiet_NaN();

double r_cor(const double* a, const double* b, int64_t n) {
  long double sa = 0, sb = 0;
  for (int64_t i = 0; i < n; ++i) { sa += a[i]; sb += b[i]; }
  const long double ma = sa / n, mb = sb / n;
  long double ab = 0, aa = 0, bb = 0;
  for (int64_t i = 0; i < n; ++i) {
    const long double x = a[i] - ma, y = b[i] - mb;
    ab += x * y; aa += x * x; bb += y * y;
  }
  return (double)(ab / std::sqrt((double)(aa * bb)));
}

struct PhaseTimer {
  bigkrls_ctx* ctx;
  hipEvent_t ev[9];
  int n = 0;
  bool ok = true;
  explicit PhaseTimer(bigkrls_ctx* c) : ctx(c) {
    for (auto& e : ev) e = nullptr;
  }
  ~PhaseTimer() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  void mark() {   // event n closes phase n - 1
    if (n >= 9) return;
    if (hipEventCreate(&ev[n]) != hipSuccess) { ok = false; ev[n] = nullptr; return; }
    if (hipEventRecord(ev[n], ctx->stream) != hipSuccess) ok = false;
    ++n;
  }
  void rewind(int to) {   // (a phase is run again: its events and the later ones are recorded anew)
    for (int i = to; i < n; ++i)
      if (ev[i]) { (void)hipEventDestroy(ev[i]); ev[i] = nullptr; }
    if (to < n) n = to;
  }
  void collect(double* out8) {
    for (int i = 0; i < 8; ++i) out8[i] = 0.0;
    if (!ok) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i + 1 < n; ++i) {
      float ms = 0.f;
      if (ev[i] && ev[i + 1] && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) out8[i] = ms * 1e-3;
    }
  }
};

// host <-> device through the context's pinned staging buffer (no user pages are pinned per call)
int upload(bigkrls_ctx* ctx, double* dst_dev, const double* src_pinned, int64_t n) {
  if (n > 0)
    BK_HIP(hipMemcpyAsync(dst_dev, src_pinned, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  return BIGKRLS_OK;
}

int download(bigkrls_ctx* ctx, double* dst_host, const double* src_dev, int64_t n, double* pinned) {
  if (n <= 0) return BIGKRLS_OK;
  BK_HIP(hipMemcpyAsync(pinned, src_dev, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BK_HIP(hipStreamSynchronize(ctx->stream));
  std::memcpy(dst_host, pinned, (size_t)n * sizeof(double));
  return BIGKRLS_OK;
}

// out (n x (r1 - r0), ld n) = alpha M Q[r0:r1, :]' with M = Q diag(w): the rows r0:r1 of the block are symmetric
// (lower tiles computed and mirrored, half the MFMA work), the rows above and below plain products
int vcov_cols(bigkrls_ctx* ctx, int64_t n, int64_t k, int64_t r0, int64_t r1, double alpha, const double* M,
              const double* Q, double* out) {
  const int64_t nloc = r1 - r0;
  if (r0 > 0) BK_TRY(gemm(ctx, 0, 1, r0, nloc, k, alpha, M, n, Q + r0, n, 0.0, out, n));
  BK_TRY(syrk_mirror_set(ctx, nloc, k, alpha, M + r0, n, Q + r0, n, out + r0, n));
  if (r1 < n) BK_TRY(gemm(ctx, 0, 1, n - r1, nloc, k, alpha, M + r1, n, Q + r0, n, 0.0, out + r1, n));
  return BIGKRLS_OK;
}

// The rows a rank owns and the eigensolver a multi-GPU fit uses: block Lanczos with sharded
// K B_j products when Neig << N (like the single-GPU library), otherwise the dense path with stage 1 partitioned by
// column blocks (64-column panels must not straddle two ranks), tiny problems replicated.
enum DistEigen { DE_KRYLOV = 0, DE_DENSE = 1, DE_REPLICATED = 2 };
int dist_plan(bigkrls_comm* comm, int64_t n, const bigkrls_fit_options* opt, int* mode, int64_t* nb, int64_t* r0,
              int64_t* r1) {
  const int64_t neig = (opt->neig > 0) ? std::min<int64_t>(n, opt->neig) : n;
  int m = (neig * 8 <= n && n >= 16384) ? DE_KRYLOV : (n > 256 ? DE_DENSE : DE_REPLICATED);
  if (const char* e = getenv("BIGKRLS_DIST_EIGEN")) {
    const std::string v = e;
    if (v == "krylov" && neig < n && neig * 4 <= n) m = DE_KRYLOV;
    else if (v == "dense" && n > 256) m = DE_DENSE;
    else if (v == "replicated") m = DE_REPLICATED;
  }
  *mode = m;
  dist_partition(n, comm->nranks, m == DE_DENSE ? 64 : 1, comm->rank, nb, r0, r1);
  return BIGKRLS_OK;
}

// BIGKRLS_VERIFY=0 switches the fit's check of its decomposition off (A/B timing)
bool verify_on() {
  static const bool on = [] { const char* e = getenv("BIGKRLS_VERIFY"); return !(e && e[0] == '0'); }();
  return on;
}

bool report_redo() { return verbose() || getenv("BIGKRLS_REPORT_REDO"); }

// One fit: what its phases share, and the phases, in the reference's order. Each returns a status; fit_impl runs them.
// comm == nullptr is the single-GPU fit; with a communicator every N x N object is this rank's column block, and
// where a phase differs it has a `_single` and a `_dist` body, chosen once at its top.
//
// The rule of the multi-GPU path: a local failure (an allocation, a launch) must not let this rank leave while its
// peers wait in the next collective, so the status of every local stretch is agreed (all-reduce MIN, agreed()) before
// the exchange that follows it.
struct Fit {
  // ---- the arguments
  bigkrls_ctx* ctx;
  bigkrls_comm* comm;
  const double* h_X;
  const double* h_y;
  int64_t n, p;
  const bigkrls_fit_options* opt;
  bigkrls_fit_outputs* out;
  hipStream_t st = nullptr;
  // ---- validated options and the moments of the raw data
  int64_t neig = 0, pd = 0;
  bool neig_auto = false;                      // bigkrls_fit_auto: the eigensolver finds the rank, neig is the cap until it has (decompose)
  int64_t neig_max = 0, neig_cap = 0;
  double eigtrunc = 0.0, sigma = 0.0;
  bool derivative = false, vcov_est = false, acf = false;
  bool implicit = false;                       // kernel_form = 1: K is never stored, `kop` stands in for dK
  KernelOp kop;
  std::vector<int64_t> cols;                   // 0-based selected columns
  std::vector<double> x_mean, x_sd;
  double y_mean = 0.0, y_sd = 0.0;
  // ---- the rows this rank owns (comm == nullptr: all of them)
  int dist_mode = DE_REPLICATED;
  int64_t nb = 0, r0 = 0, r1 = 0, nloc = 0;
  // ---- device: SLOT_FIT_SMALL in this order (dy follows dX, dyhat follows dc: single copies rely on it), Q and K
  double *dX = nullptr, *dy = nullptr, *dc = nullptr, *dyhat = nullptr, *dXe = nullptr, *dD = nullptr, *dS = nullptr;
  double *dDloc = nullptr, *dSloc = nullptr;   // row-block results before their all-gather
  double *dvals = nullptr, *da = nullptr, *dw = nullptr, *dQ = nullptr, *dK = nullptr;
  double* pin = nullptr;                       // the context's pinned buffer: re-got after every call that may grow it
  int64_t pin_doubles = 0;
  // ---- host results
  const double* Xs = nullptr;                  // standardised X (ctx->h_xs) for the O(NP) post-processing
  std::vector<double> ys, vals, coeffs, yhat, wv, ame_scale, var;
  std::vector<int32_t> isbin;
  int64_t lastkeeper = 0, k = 0, nprobes = 0;
  double lambda = 0.0, Le = 0.0, sigmasq = kNaN;
  // ---- redoing a decomposition (redo_or_give_up) and the check it answers (verify_decomposition)
  enum Redo { IMMEDIATE = 0, DEFERRED = 1 };
  int redo_left[2] = {1, 1};
  bool first_try = true;                       // cleared before any redo of the decomposition
  bool nan_agreed = false;                     // some rank's eigenvalues of the last attempt hold NaNs
  bool verify_pending = false;                 // the deferred comparison is still to come
  double* dVU = nullptr;                       // device: [U | L | R] of the check (SLOT_FIT_VERIFY)
  std::vector<double> verify_l;                // host copy of L = Q (lambda o r), n x 2
  double verify_tol = 0.0;
  PhaseTimer timer;
  int timer_n_before_eigen = 0;

  Fit(bigkrls_ctx* ctx_, bigkrls_comm* comm_, const double* X_, const double* y_, int64_t n_, int64_t p_,
      const bigkrls_fit_options* opt_, bigkrls_fit_outputs* out_)
      : ctx(ctx_), comm(comm_), h_X(X_), h_y(y_), n(n_), p(p_), opt(opt_), out(out_), timer(ctx_) {}

  static int fail(const std::string& msg) { set_error(msg); return BIGKRLS_EINVAL; }
  int agreed(int rc) { return comm ? comm_agree(comm, rc) : rc; }
  // K is this fit's own kernel matrix, built from inputs validated as finite (so finite, symmetric): a block
  // Lanczos whose Ritz pairs fail its check against K, or NaNs after a tridiagonalisation (the eigensolver flags both in
  // ctx->corrupt_run), are a fault of the run, not of the input -- redone once like a failed check
  int soften(int rc) {
    const bool corrupt = ctx->corrupt_run;
    ctx->corrupt_run = false;
    return (rc != BIGKRLS_OK && corrupt) ? (int)BK_EWATCHDOG : rc;
  }
  // On one GPU with marginal effects asked for, ONE pass over K in step 4 delivers the marginal effects, the fitted
  // values and the product of the decomposition's check (see verify_decomposition)
  bool one_pass_over_k() const { return !comm && derivative; }
  int64_t pd1() const { return std::max<int64_t>(pd, 1); }

  // ---- validation, in the reference's order (R/bigKRLS.R:183-242) ---------------------------------------------------
  int validate() {
    BK_TRY(check_ctx(ctx));
    BK_REQUIRE(h_X && h_y && opt && out, "fit: null argument");
    BK_REQUIRE(opt->struct_bytes == (int64_t)sizeof(bigkrls_fit_options), "fit: options struct size mismatch");
    BK_REQUIRE(out->struct_bytes == (int64_t)sizeof(bigkrls_fit_outputs), "fit: outputs struct size mismatch");
    BK_REQUIRE(n > 1 && p > 0 && n < (1ll << 30), "fit: bad dimensions");
    st = ctx->stream;
    {
      std::string bad;
      std::vector<char> col_nan(p), col_inf(p);                // one scan of X for both checks
      for_columns(p, n, [&](int64_t j) { scan_column(h_X + j * n, &col_nan[j], &col_inf[j]); });
      for (int64_t j = 0; j < p; ++j)
        if (col_nan[j]) bad += (bad.empty() ? "" : ", ") + std::to_string(j + 1);
      if (!bad.empty())
        return fail("the following columns in X contain missing data, which must be removed: " + bad);   // :183-187
      // (the reference has no check for Inf: its standardised column, and with it every entry of K, turns NaN and the
      //  fit ends in the "Missing eigenvalues" message; here the input error is named before any GPU work)
      for (int64_t j = 0; j < p; ++j)
        if (col_inf[j]) bad += (bad.empty() ? "" : ", ") + std::to_string(j + 1);
      if (!bad.empty()) return fail("the following columns in X contain infinite values, which must be removed: " + bad);
    }
    acf = opt->acf != 0 && p > 2;                                                                        // :192
    neig = (opt->neig > 0) ? std::min<int64_t>(n, opt->neig) : n;                                        // :194
    if (neig_auto) neig = neig_cap = std::max<int64_t>(neig_max, 1);          // (checked below, with eigtrunc)
    if (opt->kernel_form != 0 && opt->kernel_form != 1) return fail("fit: kernel_form must be 0 (stored) or 1 (implicit)");
    implicit = opt->kernel_form == 1;
    if (implicit) {
      if (comm) return fail("fit: the implicit kernel form runs on one GPU (bigkrls_fit), not in bigkrls_fit_dist");
      if (out->d_K) return fail("fit: the implicit kernel form stores no kernel matrix: d_K must be NULL");
      if (out->d_vcov_c || out->d_vcov_fitted)
        return fail("fit: the implicit kernel form returns the variance as factors (d_vcov_q, vcov_w): d_vcov_c and d_vcov_fitted must be NULL");
      if (opt->neig <= 0 && !neig_auto) return fail("fit: the implicit kernel form needs neig (block Lanczos for the neig largest pairs)");
      if (n < 1024 || 4 * neig > n)
        return fail("fit: the implicit kernel form needs n >= 1024 and 4 neig <= n (n = " + std::to_string((long long)n) +
                    ", neig = " + std::to_string((long long)neig) + ")");
    }
    eigtrunc = opt->eigtrunc;
    if (eigtrunc < 0.0 || std::isnan(eigtrunc)) eigtrunc = n > 3000 ? 0.001 : 0.0;                       // :195-201
    else if (eigtrunc > 1.0) return fail("eigtrunc must be between 0 (no truncation) and 1 (keep largest only).");
    if (neig_auto) {
      if (!(eigtrunc > 0.0))
        return fail("fit: bigkrls_fit_auto finds the rank from eigtrunc, which must be > 0 (unset, it is 0 for n <= 3000): pass eigtrunc");
      if (n < 1024 || neig_max < 1 || 4 * neig_max > n)
        return fail("fit: bigkrls_fit_auto needs n >= 1024 and 1 <= neig_max <= n / 4 (n = " + std::to_string((long long)n) +
                    ", neig_max = " + std::to_string((long long)neig_max) + ")");
    }
    derivative = opt->derivative != 0;
    vcov_est = opt->vcov_est != 0;
    if (opt->which_derivatives != nullptr) {                                                              // :206-215
      if (!derivative) return fail("which.derivative requires derivative = TRUE");
      cols = std::vector<int64_t>((size_t)std::max<int64_t>(opt->n_which, 0));
      for (size_t i = 0; i < cols.size(); ++i) {
        const int64_t w = opt->which_derivatives[i];
        if (w < 1 || w > p) return fail("which.derivatives must index columns of X");
        cols[i] = w - 1;
      }
      if (cols.empty()) return fail("which.derivatives must index columns of X");
    } else {
      cols = std::vector<int64_t>((size_t)p);
      for (int64_t j = 0; j < p; ++j) cols[j] = j;
    }
    pd = derivative ? (int64_t)cols.size() : 0;
    x_mean.resize(p);
    x_sd.resize(p);
    {
      std::string constant;
      for_columns(p, n, [&](int64_t j) { mean_sd(h_X + j * n, n, &x_mean[j], &x_sd[j]); });              // :179
      for (int64_t j = 0; j < p; ++j)
        if (x_sd[j] == 0.0) constant += (constant.empty() ? "" : ", ") + std::to_string(j + 1);
      if (!constant.empty())
        return fail("The following columns in X are constant and must be removed: " + constant);         // :217
    }
    for (int64_t i = 0; i < n; ++i)
      if (std::isnan(h_y[i])) return fail("y contains missing data.");
    for (int64_t i = 0; i < n; ++i)
      if (!std::isfinite(h_y[i])) return fail("y contains infinite values.");
    mean_sd(h_y, n, &y_mean, &y_sd);
    if (y_sd == 0.0) return fail("y is a constant.");
    if (std::isnan(opt->lambda) || std::isinf(opt->lambda)) return fail("lambda must be a positive scalar");   // :225
    if (std::isnan(opt->sigma) || std::isinf(opt->sigma)) return fail("sigma must be a positive scalar");      // :227
    sigma = opt->sigma > 0.0 ? opt->sigma : (double)p;                                                   // :230
    if (derivative && !vcov_est)                                                                          // :239
      return fail("vcov.est is needed to get derivatives (derivative==TRUE requires vcov.est=TRUE).");
    if (out->d_vcov_q) {                       // vcov.est.c handed out as its factors Q diag(w) Q'
      if (!vcov_est) return fail("the factors of vcov.est.c require vcov.est = TRUE");
      BK_REQUIRE(out->vcov_w && out->vcov_q_cols_max > 0, "fit: d_vcov_q needs vcov_w and vcov_q_cols_max > 0");
      out->vcov_q_cols = 0;
    }
    if (out->binaryindicator) {                                                                           // :242 (raw X)
      for_columns(p, n, [&](int64_t j) {
        double lo, hi;
        out->binaryindicator[j] = two_valued(h_X + j * n, n, &lo, &hi) ? 1 : 0;
      });
    }
    return BIGKRLS_OK;
  }

  void scan_column(const double* x, char* any_nan, char* any_inf) const {
    bool has_nan = false, inf = false;
    for (int64_t i = 0; i < n; ++i) {
      has_nan |= std::isnan(x[i]);
      inf |= !std::isfinite(x[i]);
    }
    *any_nan = has_nan;
    *any_inf = inf;
  }

  // ---- the rows this rank owns, the workspace and its layout -------------------------------------------------------
  int plan_and_allocate() {
    nb = n, r0 = 0, r1 = n;
    if (comm) BK_TRY(dist_plan(comm, n, opt, &dist_mode, &nb, &r0, &r1));
    nloc = r1 - r0;
    const int64_t small_doubles = n * p + n * (3 + 5 * pd1()) + 3 * neig + 64;
    pin_doubles = std::max<int64_t>(n * std::max<int64_t>(p, pd) + n, 2 * neig + 64);
    void *psmall = nullptr, *pq = nullptr, *pk = nullptr;
    BK_TRY(agreed(allocate(small_doubles, &psmall, &pq, &pk)));
    double* q = (double*)psmall;
    dX = q; q += n * p;
    dy = q; q += n;
    dc = q; q += n;
    dyhat = q; q += n;
    dXe = q; q += n * pd1();
    dD = q; q += n * pd1();
    dS = q; q += n * pd1();
    dDloc = q; q += n * pd1();
    dSloc = q; q += n * pd1();
    dvals = q; q += neig;
    da = q; q += neig;
    dw = q; q += neig;
    dQ = (double*)pq;
    dK = out->d_K ? out->d_K : (double*)pk;

    if (trace_on()) BK_TRY(trace_host("L:fit_begin", nullptr, 0, n));
    BK_TRY(ws_poison_all(ctx));
    timer.mark();
    return BIGKRLS_OK;
  }

  int allocate(int64_t small_doubles, void** psmall, void** pq, void** pk) {
    void* unused = nullptr;
    BK_TRY(ws_get(ctx, SLOT_FIT_SMALL, small_doubles * (int64_t)sizeof(double), psmall));
    BK_TRY(ws_get(ctx, SLOT_FIT_Q, n * neig * (int64_t)sizeof(double), pq));
    if (!out->d_K && !implicit)   // K: the whole matrix, or this rank's column block K[:, r0:r1) (n x nloc, ld n)
      BK_TRY(ws_get(ctx, comm ? SLOT_DIST_K : SLOT_FIT_K, n * std::max<int64_t>(nloc, 1) * (int64_t)sizeof(double), pk));
    if (comm && vcov_est && (out->d_vcov_c || out->d_vcov_fitted))   // Q diag(w) of the variance matrices, up front
      BK_TRY(ws_get(ctx, SLOT_FIT_M, n * neig * (int64_t)sizeof(double), &unused));
    if (comm)      // the staging of the row-block all-gathers (c, yhat, D, S)
      BK_TRY(ws_get(ctx, SLOT_COMM_STAGE, (int64_t)(comm->nranks + 1) * nb * pd1() * (int64_t)sizeof(double), &unused));
    BK_TRY(pinned_get(ctx, pin_doubles, &pin));
    return BIGKRLS_OK;
  }

  // ---- standardise (R/bigKRLS.R:248-254) straight into the pinned staging buffer, upload ---------------------------
  int standardise_upload() {
    std::vector<double>& h_xs = ctx->h_xs;                                 // host copies for the O(NP) post-processing
    if ((int64_t)h_xs.size() < n * p) h_xs.resize((size_t)(n * p));
    Xs = h_xs.data();
    ys.resize((size_t)n);
    for_columns(p, n, [&](int64_t j) {
      standardise_column(h_X + j * n, n, x_mean[j], x_sd[j], pin + j * n);
      std::memcpy(h_xs.data() + j * n, pin + j * n, (size_t)n * sizeof(double));
    });
    double* ys_pin = pin + n * p;
    standardise_column(h_y, n, y_mean, y_sd, ys_pin);
    std::memcpy(ys.data(), ys_pin, (size_t)n * sizeof(double));
    BK_TRY(upload(ctx, dX, pin, n * p + n));                                // dy follows dX in the slab
    BK_HIP(hipStreamSynchronize(st));                                       // the pinned buffer is reused below
    timer.mark();                                                           // h2d
    return BIGKRLS_OK;
  }

  // ---- step 1: kernel (:262) ---------------------------------------------------------------------------------------
  int build_kernel() {
    if (implicit) {   // no matrix: the centred copy of X and its norms, once for every product of the fit
      BK_TRY(kernel_op_prepare(ctx, dX, n, n, p, sigma, &kop));
      timer.mark();                                                         // kernel (about 0: the products land in `eigen`)
      return BIGKRLS_OK;
    }
    if (!comm) BK_TRY(kernel_block(ctx, dX, n, n, dX, n, n, p, sigma, dK, n, 0));
    else BK_TRY(agreed(nloc > 0 ? kernel_block(ctx, dX, n, n, dX + r0, nloc, n, p, sigma, dK, n, r0) : BIGKRLS_OK));   // K[:, r0:r1): no exchange
    timer.mark();                                                           // kernel
    if (trace_on()) BK_TRY(trace_point(ctx, st, "L:fit_K", dK, n * std::max<int64_t>(nloc, 1), r0));
    return BIGKRLS_OK;
  }

  // ---- step 2: eigen (:266-269; bEigen's lastkeeper rule on the device side), one attempt --------------------------
  // BK_EWATCHDOG (agreed by all ranks): the attempt is a fault of the run, to be redone (fit_impl).
  int decompose() {
    lastkeeper = 0;
    nan_agreed = false;
    // (the flag only concerns the block Lanczos: see common.h; every exit of an attempt goes through the guard)
    struct Flag { bool& f; ~Flag() { f = false; } } flag_guard{ctx->caller_verifies};
    ctx->caller_verifies = verify_on() && first_try;
    if (!comm) BK_TRY(eigen_single());
    else if (dist_mode == DE_KRYLOV) BK_TRY(eigen_dist_krylov());
    else if (dist_mode == DE_DENSE) BK_TRY(eigen_dist_dense());
    else BK_TRY(eigen_dist_replicated());
    return fetch_and_agree_eigenvalues();
  }

  int eigen_single() {
    if (neig_auto) {      // the buffers hold neig_cap values / columns; from here on neig is what the eigensolver returned
      neig = neig_cap;
      int64_t found = 0;
      const int rc = implicit ? eigen_implicit(ctx, kop, neig_cap, dvals, neig_cap, eigtrunc, dQ, n, &lastkeeper, true, &found)
                              : eigen_auto(ctx, dK, n, n, neig_cap, dvals, eigtrunc, dQ, n, &found, &lastkeeper);
      if (rc == BIGKRLS_OK) neig = found;
      return soften(rc);
    }
    if (implicit) return soften(eigen_implicit(ctx, kop, neig, dvals, neig, eigtrunc, dQ, n, &lastkeeper));
    return soften(eigen(ctx, dK, n, n, neig, dvals, neig, eigtrunc, dQ, n, &lastkeeper));
  }

  int eigen_dist_krylov() {
    return agreed(soften(eigen_krylov_dist(comm, dK, n, r0, r1, nb, neig, dvals, neig, eigtrunc, dQ, n, &lastkeeper)));
  }

  int eigen_dist_dense() {
    // the reduction overwrites its operand: it works on a copy of the column block
    void* pa = nullptr;
    BK_TRY(comm_agree(comm, ws_get(ctx, SLOT_DIST_A, n * std::max<int64_t>(nloc, 1) * (int64_t)sizeof(double), &pa)));
    // A fired watchdog of a persistent kernel (panel factorisation / bulge chasing: their workgroups must be
    // co-resident, and here they share the GPU with the collectives' kernels) is agreed on by all ranks inside
    // eigen_dense_dist and the decomposition is redone ONCE, on every rank, with the launch-per-step kernels --
    // K[:, r0:r1) is untouched, so the replay starts from a fresh copy (the single-GPU eigen() does the same inside its
    // call, DenseEig::replay in csrc/eigen.hip: both drain the context's streams first, drain_streams). The same
    // replay answers ranks whose replicated decompositions did not come out identical (eigen_dense_dist).
    int rc_e = BIGKRLS_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
      // (a failed copy is a local failure like any other: agreed on before the peers enter the decomposition's first
      //  collective, not returned from here while they wait in it)
      int rc_copy = BIGKRLS_OK;
      if (nloc > 0 && hipMemcpyAsync(pa, dK, (size_t)(n * nloc) * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess) {
        set_error("fit: copy of the column block of K failed");
        rc_copy = BIGKRLS_EHIP;
      }
      rc_e = comm_agree(comm, rc_copy);
      if (rc_e != BIGKRLS_OK) break;
      rc_e = eigen_dense_dist(comm, (double*)pa, n, nb, neig, eigtrunc, dvals, dQ, &lastkeeper);
      if (rc_e != BK_EWATCHDOG || attempt == 1 || ctx->no_resident) break;
      if (verbose())
        fprintf(stderr, "[bigkrls] rank %d: %s; replaying the distributed decomposition with per-step launches\n",
                comm->rank, bigkrls_last_error());
      (void)drain_streams(ctx);
      ctx->n_replayed++;
      ctx->no_resident = true;
    }
    ctx->no_resident = false;
    if (rc_e == BK_EWATCHDOG) {
      set_error(std::string(bigkrls_last_error()) + " (also after the replay with per-step launches)");
      rc_e = BIGKRLS_EHIP;
    } else if (rc_e != BIGKRLS_OK) {
      // (the code is agreed, the flag beside it is rank-local: any rank's flag makes all of them redo the decomposition)
      double f = ctx->corrupt_run ? -1.0 : 0.0;
      ctx->corrupt_run = false;
      BK_TRY(comm_all_reduce_host(comm, &f, 1, COMM_MIN));
      if (f < 0.0) rc_e = BK_EWATCHDOG;
    }
    return rc_e;
  }

  // tiny problems: K gathered (its column blocks are row blocks of K' = K), the decomposition replicated with the
  // back-transform split by eigenvector column, Q assembled by an all-reduce (sum)
  int eigen_dist_replicated() {
    void* pa = nullptr;
    BK_TRY(comm_agree(comm, ws_get(ctx, SLOT_DIST_A, n * n * (int64_t)sizeof(double), &pa)));
    double* Kfull = (double*)pa;
    // K[:, r0:r1) as the rows r0:r1 of K' (nloc x n, ld nloc would need a transpose): gather the columns instead,
    // as blocks of nb columns = contiguous slabs of n nb doubles
    double *send = nullptr, *recv = nullptr;
    BK_TRY(agreed(stage_column_block(&send, &recv)));
    BK_TRY(comm_all_gather(comm, send, recv, nb * n));
    BK_TRY(agreed(hipMemcpyAsync(Kfull, recv, (size_t)(n * n) * sizeof(double), hipMemcpyDeviceToDevice, st) == hipSuccess
                      ? BIGKRLS_OK : BIGKRLS_EHIP));
    BK_TRY(comm_agree(comm, soften(eigen(ctx, Kfull, n, n, neig, dvals, neig, eigtrunc, dQ, n, &lastkeeper, comm->rank, comm->nranks))));
    if (lastkeeper > 0) BK_TRY(comm_all_reduce(comm, dQ, n * lastkeeper, COMM_SUM));
    return BIGKRLS_OK;
  }

  int stage_column_block(double** send, double** recv) {     // (local steps before a collective: their status is agreed)
    void* pst = nullptr;
    BK_TRY(ws_get(ctx, SLOT_COMM_STAGE, (int64_t)(comm->nranks + 1) * nb * n * (int64_t)sizeof(double), &pst));
    *send = (double*)pst;
    *recv = *send + nb * n;
    BK_HIP(hipMemsetAsync(*send, 0, (size_t)(nb * n) * sizeof(double), st));
    if (nloc > 0) BK_HIP(hipMemcpyAsync(*send, dK, (size_t)(n * nloc) * sizeof(double), hipMemcpyDeviceToDevice, st));
    return BIGKRLS_OK;
  }

  int fetch_eigenvalues() {
    BK_TRY(pinned_get(ctx, pin_doubles, &pin));   // (the eigensolver may have grown -- and so moved -- the pinned buffer)
    return download(ctx, vals.data(), dvals, neig, pin);
  }

  int fetch_and_agree_eigenvalues() {
    vals.resize(neig);
    BK_TRY(agreed(fetch_eigenvalues()));
    if (!comm) return BIGKRLS_OK;
    // The eigenvalues are replicated: every rank computed its own copy (deterministic kernels, so normally the same
    // bits). The bounds loops and the golden section of the lambda search branch on them on every rank separately, and a
    // copy that is off in its last bit -- a valid decomposition, which the check against K lets through by design --
    // could flip one rank's branch: the ranks would probe different lambdas while all-reducing one loss. So the search
    // does not rely on the copies being identical: rank 0's eigenvalues (device and host copy) are what EVERY rank uses,
    // one broadcast of 8 Neig bytes; the kept-pair count follows from the same values and is agreed the same way. The
    // reference's workers all read one K and one set of eigenvalues too (R/bigKRLS.R:345-362).
    std::vector<double> mine(vals);
    BK_TRY(comm_broadcast(comm, dvals, neig, 0));
    BK_TRY(agreed(fetch_eigenvalues()));
    if (std::memcmp(mine.data(), vals.data(), (size_t)neig * sizeof(double)) != 0) {
      ctx->n_replica_diff++;
      if (report_redo())
        fprintf(stderr, "[bigkrls] rank %d: the replicated eigenvalues differ from rank 0's; using rank 0's\n", comm->rank);
    }
    double lk[2] = {(double)lastkeeper, -(double)lastkeeper};
    BK_TRY(comm_all_reduce_host(comm, lk, 2, COMM_MIN));
    if (lk[0] != -lk[1]) {        // (every rank sees the same two numbers: all of them redo the decomposition)
      set_error("fit: the ranks disagree on the number of kept eigenpairs (" + std::to_string((long long)lk[0]) + " ... " +
                std::to_string((long long)-lk[1]) + ")");
      return BK_EWATCHDOG;
    }
    return BIGKRLS_OK;
  }

  bool has_nan() const {
    for (int64_t i = 0; i < neig; ++i)
      if (std::isnan(vals[i])) return true;
    return false;
  }

  // NaN among the eigenvalues / no kept pair (local)
  int check_values() {
    if (!has_nan() && lastkeeper > 0) return BIGKRLS_OK;
    set_error(has_nan() ? "fit: NaN among the eigenvalues" : "fit: no eigenpair passes the eigtrunc threshold");
    return BK_EWATCHDOG;
  }

  // ---- ... verified against K itself ---------------------------------------------------------
  // With many processes on one GPU about one fit in 10 000 came back different from its repetitions, a handful of them
  // grossly wrong, with no error (round 5; the account is DESIGN.md section 8). A decomposition that is off by more than
  // rounding cannot pass these checks:
  //   * the whole spectrum is known (Neig = N): sum of the eigenvalues = trace(K) = N (the kernel's diagonal is 1);
  //   * ALL kept pairs through two fixed +-1 combinations of them, u = Q r: |K u - Q (lambda o r)| <= 1e-8 lambda_1
  //     sqrt(k) and | |u|^2 - k | <= 1e-8 k, from one pass over K (rank-local rows in a multi-GPU fit), 8 N^2 bytes, and
  //     one over Q: 0.6 ms of a 410-ms fit at N = 20 000. (A sample of three pairs was not enough: a run whose
  //     eigenvalues were right to 1e-15 came back with c off by 4 % -- some columns of Q wrong, none of the three.)
  // The block Lanczos (Neig << N) on its own checks only the last block of its Ritz pairs against K itself
  // (csrc/eigen.hip), i.e. a sample -- the kind of check that was not enough above: in a fit its pairs go through the
  // same two combinations at the same tolerance (the iteration stops at 1e-10 lambda_1 per pair), and the sample check
  // -- a K-times-block product of 13 ms at N = 50 000, 50 ms at N = 100 000 -- is left out of the first attempt
  // (ctx->caller_verifies); a redo runs with it, and with the Rayleigh-Ritz refinement where it asks for one.
  // BIGKRLS_VERIFY=0 switches the check off (A/B timing).
  // On one GPU with marginal effects asked for, the product K [u_1 u_2] is DEFERRED (round 6): the combinations ride
  // along in the one pass over K that step 4 makes anyway (marginal effects + fitted values), and the comparison happens
  // there (verify_deferred); what can be checked without K -- the trace, |Q r|^2 = k -- is checked here. If the
  // deferred comparison fails, everything from the decomposition on is redone once (the lambda search and the
  // coefficients of a wrong decomposition, 2 ms, are thrown away). One pass over K behind the eigensolver instead of
  // three: -0.6 ms at N = 20 000, -4.5 ms at N = 50 000, -18 ms at N = 100 000.
  // (Local: the caller agrees the status.)
  int verify_decomposition() {
    verify_pending = false;
    if (!verify_on() || lastkeeper <= 0) return BIGKRLS_OK;
    // (block Lanczos: the iteration stops at Ritz residuals of 1e-10 lambda_1 per pair, <= 1e-10 lambda_1 sqrt(k) for a
    //  combination; its own sample check against K is left out in a first attempt -- ctx->caller_verifies -- so this
    //  is the check of its pairs, at the tolerance of the dense path)
    const double vtol = 1e-8;
    const bool defer_k = one_pass_over_k();
    char buf[256];
    if (neig == n) {
      long double tr = 0.0L;
      for (int64_t i = 0; i < neig; ++i) tr += vals[i];
      if (!(std::fabs((double)tr - (double)n) <= 1e-9 * (double)n)) {
        snprintf(buf, sizeof buf, "fit: the eigenvalues sum to %.15g, the trace of the kernel matrix is %lld", (double)tr, (long long)n);
        set_error(buf);
        return BK_EWATCHDOG;
      }
    }
    // all kept pairs at once through two fixed +-1 combinations r_1, r_2 of them (a wrong column, or a wrong slice of
    // one rank's back-transform, cannot hide among the others the way it can from a sample of columns):
    //   u_i = Q r_i,  |K u_i - Q (lambda o r_i)| <= 1e-8 lambda_1 sqrt(k),  | |u_i|^2 - k | <= 1e-8 k
    const int64_t kk = lastkeeper;
    const int64_t rows = comm ? nloc : n, rr0 = comm ? r0 : 0;
    void* pv = nullptr;
    BK_TRY(ws_get(ctx, SLOT_FIT_VERIFY, (6 * n + 4 * kk) * (int64_t)sizeof(double), &pv));
    double* dU = (double*)pv;             // n x 2: Q r
    double* dL = dU + 2 * n;              // n x 2: Q (lambda o r)
    double* dR = dL + 2 * n;              // rows x 2: K[rows, :] U
    double* dC = dR + 2 * n;              // k x 4: [r_1 r_2 | lambda o r_1, lambda o r_2]
    double* hp = nullptr;
    BK_TRY(pinned_get(ctx, std::max<int64_t>(pin_doubles, 6 * n + 4 * kk), &hp));
    pin = hp;
    for (int64_t j = 0; j < kk; ++j) {
      const uint32_t h1 = (uint32_t)(j + 1) * 2654435761u, h2 = (uint32_t)(j + 1) * 2246822519u;
      const double s1 = ((h1 >> 15) & 1u) ? 1.0 : -1.0, s2 = ((h2 >> 13) & 1u) ? 1.0 : -1.0;
      hp[j] = s1;
      hp[kk + j] = s2;
      hp[2 * kk + j] = s1 * vals[j];
      hp[3 * kk + j] = s2 * vals[j];
    }
    BK_HIP(hipMemcpyAsync(dC, hp, (size_t)(4 * kk) * sizeof(double), hipMemcpyHostToDevice, st));
    BK_TRY(gemm(ctx, 0, 0, n, 4, kk, 1.0, dQ, n, dC, kk, 0.0, dU, n));          // [U | L] = Q [R | Lambda R]  (dL follows dU)
    if (rows > 0 && !defer_k) {
      if (implicit) BK_TRY(kernel_op_times(ctx, kop, dU, 2, n, dR, n));
      else if (!comm) BK_TRY(gemm(ctx, 0, 0, n, 2, n, 1.0, dK, n, dU, n, 0.0, dR, n));
      else BK_TRY(gemm(ctx, 1, 0, rows, 2, n, 1.0, dK, n, dU, n, 0.0, dR, rows));
    }
    BK_HIP(hipStreamSynchronize(st));     // (the pinned buffer was the source of the upload)
    BK_HIP(hipMemcpyAsync(hp, dU, (size_t)(4 * n) * sizeof(double), hipMemcpyDeviceToHost, st));
    if (rows > 0 && !defer_k) BK_HIP(hipMemcpyAsync(hp + 4 * n, dR, (size_t)(2 * rows) * sizeof(double), hipMemcpyDeviceToHost, st));
    BK_HIP(hipStreamSynchronize(st));
    const double scale = std::fabs(vals[0]) > 0.0 ? std::fabs(vals[0]) : 1.0;
    if (defer_k) {
      dVU = dU;
      verify_l.assign(hp + 2 * n, hp + 4 * n);
      verify_tol = vtol * scale * std::sqrt((double)kk);
      verify_pending = true;
    }
    for (int i = 0; i < 2; ++i) {
      const double* u = hp + i * n;
      const double* l = hp + 2 * n + i * n;
      const double* r = hp + 4 * n + i * rows;
      long double nrm = 0.0L;
      for (int64_t t = 0; t < n; ++t) nrm += (long double)u[t] * u[t];
      double worst = 0.0;
      for (int64_t t = 0; t < (defer_k ? 0 : rows); ++t) {
        const double d = std::fabs(r[t] - l[rr0 + t]);
        worst = (d > worst || d != d) ? d : worst;
      }
      if (!(std::fabs((double)nrm - (double)kk) <= vtol * (double)kk) || !(worst <= vtol * scale * std::sqrt((double)kk))) {
        snprintf(buf, sizeof buf, "fit: the %lld kept eigenpairs fail the check against K (|K Q r - Q Lambda r| = %.3e with lambda_1 = %.3e, |Q r|^2 = %.12g)",
                 (long long)kk, worst, scale, (double)nrm);
        set_error(buf);
        return BK_EWATCHDOG;
      }
    }
    return BIGKRLS_OK;
  }

  // the deferred half of the check of the decomposition against K: |K Q r - Q (lambda o r)| over all rows, K [u_1 u_2]
  // from step 4's pass over K
  int verify_deferred() {
    verify_pending = false;
    BK_HIP(hipMemcpyAsync(pin, dVU + 4 * n, (size_t)(2 * n) * sizeof(double), hipMemcpyDeviceToHost, st));
    BK_HIP(hipStreamSynchronize(st));
    double worst = 0.0;
    for (int64_t t = 0; t < 2 * n; ++t) {
      const double d = std::fabs(pin[t] - verify_l[t]);
      worst = (d > worst || d != d) ? d : worst;
    }
    if (worst <= verify_tol) return BIGKRLS_OK;
    char buf[256];
    snprintf(buf, sizeof buf, "fit: the %lld kept eigenpairs fail the check against K (|K Q r - Q Lambda r| = %.3e, tolerance %.3e)",
             (long long)k, worst, verify_tol);
    set_error(buf);
    return BK_EWATCHDOG;
  }

  // The values and the pairs of one attempt, checked by ALL ranks together: after a fault one rank's copy of the
  // replicated eigenvalues may hold NaNs or no kept pair while its peers' copies are fine -- a rank that decided on its
  // own would leave the others waiting in the next collective. One agreement for either check, then the NaN flag.
  int check_decomposition() {
    int rc = check_values();
    if (rc == BIGKRLS_OK) rc = verify_decomposition();
    rc = agreed(rc);
    double nn = has_nan() ? -1.0 : 0.0;
    if (comm) BK_TRY(comm_all_reduce_host(comm, &nn, 1, COMM_MIN));
    nan_agreed = nn < 0.0;
    return rc;
  }

  // The ONE copy of the redo policy. Two budgets, kept apart on purpose: one redo for an attempt that failed
  // at once (the decomposition itself or its check, IMMEDIATE) and one for a failed deferred comparison in step 4
  // (DEFERRED), after which the immediate budget is whole again -- up to four decompositions in the worst case. One
  // merged count of attempts would turn fits that recover with a redo of each kind into errors.
  int redo_or_give_up(Redo which) {
    if (redo_left[which] == 0) {
      set_error(std::string(bigkrls_last_error()) + " -- also after the decomposition was redone");
      return BIGKRLS_EHIP;
    }
    if (report_redo()) fprintf(stderr, "[bigkrls] %s; redoing the decomposition\n", bigkrls_last_error());
    redo_left[which]--;
    if (which == DEFERRED) redo_left[IMMEDIATE] = 1;
    ctx->n_redone++;
    first_try = false;
    timer.rewind(timer_n_before_eigen);     // (everything from the decomposition on is timed anew)
    return BIGKRLS_OK;
  }

  // NaNs on every attempt are the input's doing (the reference's message), not a fault to retry for ever. (NaNs agreed
  // beside a passed check can only follow a failed agreement: they end the fit as well.)
  bool nans_are_final(int rc_check) const { return nan_agreed && (rc_check == BIGKRLS_OK || redo_left[IMMEDIATE] == 0); }
  static int missing_eigenvalues() {
    return fail("Missing eigenvalues prevent bigKRLS from obtaining the regularization parameter lambda.\n\t"
                "Check for repeated observations (or other perfect linear combinations in X).");
  }

  // the decomposition stands: diagnostics of what every rank holds (csrc/trace.hip, BIGKRLS_VERBOSE)
  int accept_decomposition() {
    BK_REQUIRE(lastkeeper > 0, "fit: no eigenpair passes the eigtrunc threshold");
    k = lastkeeper;
    // the caller's room for the factors, checked before anything is computed with them: never silently truncated (the
    // count is agreed between the ranks of a multi-GPU fit, so every rank returns this)
    if (out->d_vcov_q && lastkeeper > out->vcov_q_cols_max) {
      out->lastkeeper = lastkeeper;
      return fail("fit: the decomposition keeps " + std::to_string((long long)lastkeeper) +
                  " eigenpairs, the buffers for the factors of vcov.est.c hold " +
                  std::to_string((long long)out->vcov_q_cols_max) + " columns");
    }
    if (trace_on()) {
      BK_TRY(trace_host("R:fit_vals", vals.data(), neig, k));
      BK_TRY(trace_point(ctx, st, "R:fit_Q", dQ, n * k, dist_mode));
    }
    if (verbose()) {
      // (equal lines on all ranks -- and Q'Q of the first and last kept columns; a column with a non-finite entry
      //  shows as nan)
      long double sv = 0.0L;
      for (int64_t i = 0; i < k; ++i) sv += vals[i];
      double g[2] = {0.0, 0.0};
      void* pg = nullptr;
      if (ws_get(ctx, SLOT_COMM_SMALL, 64 * sizeof(double), &pg) == BIGKRLS_OK) {
        double* dg = (double*)pg;
        (void)gemm(ctx, 1, 0, 1, 1, n, 1.0, dQ, n, dQ, n, 0.0, dg, 1);
        (void)gemm(ctx, 1, 0, 1, 1, n, 1.0, dQ + (k - 1) * n, n, dQ + (k - 1) * n, n, 0.0, dg + 1, 1);
        PinnedFetch pf(ctx, 2);
        if (pf.add(g, dg, 2 * sizeof(double)) == BIGKRLS_OK) (void)pf.finish();
      }
      fprintf(stderr, "[bigkrls] fit: rank %d kept %lld, sum(vals[:k]) = %.17g, vals[0] = %.17g, vals[k-1] = %.17g, |q_0|^2 = %.15g, |q_k-1|^2 = %.15g\n",
              comm ? comm->rank : 0, (long long)k, (double)sv, vals[0], vals[k - 1], g[0], g[1]);
    }
    timer.mark();                                                           // eigen
    return BIGKRLS_OK;
  }

  // ---- step 3: lambda (:271-280; `tol` is never forwarded by the reference: 1e-3 n) --------------------------------
  int search_lambda() {
    if (!comm) {
      BK_TRY(qty(ctx, dQ, n, k, n, dy, da));
    } else {                                  // a = Q'y from the row blocks: one all-reduce of K doubles
      BK_TRY(agreed(own_qty()));
      BK_TRY(comm_all_reduce(comm, da, k, COMM_SUM));
    }
    if (trace_on()) BK_TRY(trace_point(ctx, st, "R:fit_a", da, k, 0));
    lambda = opt->lambda;
    nprobes = 0;
    if (!(lambda > 0.0)) {
      if (opt->U >= 0.0 && !(opt->U > 0.0)) return fail("U must be a positive scalar");
      BK_TRY(lambda_search(ctx, dQ + r0, nloc, k, n, dvals, da, vals.data(), neig, opt->L, opt->U, -1.0, &lambda, &nprobes,
                           out->lambda_trace, out->lambda_trace ? out->max_trace : 0, comm, n));
    }
    timer.mark();                                                           // lambda
    long double s = 0.0L;
    for (int64_t i = 0; i < neig; ++i) s += vals[i] / (vals[i] + lambda);                                // :280 (all Neig, Q5)
    out->Neffective = (double)((long double)n - s);
    return BIGKRLS_OK;
  }

  int own_qty() {
    if (nloc > 0) return qty(ctx, dQ + r0, nloc, k, n, dy + r0, da);
    BK_HIP(hipMemsetAsync(da, 0, (size_t)k * sizeof(double), st));
    return BIGKRLS_OK;
  }

  // ---- step 4: coefficients, fitted values (:286-291) --------------------------------------------------------------
  // BK_EWATCHDOG: the deferred comparison of the decomposition's check failed (single GPU with marginal effects).
  int coefficients_and_fitted() {
    Le = 0.0;
    // the columns of the marginal-effects pass (step 5), decided here because on one GPU that pass -- ONE product of K
    // with [1, c, x_j, x_j o c ...] -- also delivers K c, the fitted values: no pass over K of their own (round 6;
    // 0.55 ms at N = 20 000, 13 ms at N = 100 000)
    isbin.resize(pd);
    ame_scale.resize(pd);
    var.resize(pd);
    for_columns(pd, n, [&](int64_t i) { derivative_column(i); });
    BK_TRY(comm ? coefficients_dist() : coefficients_single());
    coeffs.resize(n);
    yhat.resize(n);
    BK_TRY(agreed(fetch_coefficients()));              // (the derivative pass has collectives of its own)
    timer.mark();                                                           // coeffs
    if (trace_on()) {
      BK_TRY(trace_host("R:fit_lambda", &lambda, 1, nprobes));
      BK_TRY(trace_host("R:fit_c", coeffs.data(), n, 0));
      BK_TRY(trace_host("R:fit_yhat", yhat.data(), n, 0));
    }
    return BIGKRLS_OK;
  }

  void derivative_column(int64_t i) {
    const double* x = Xs + cols[i] * n;
    double lo, hi;
    isbin[i] = two_valued(x, n, &lo, &hi) ? 1 : 0;                                                       // src/bigderiv_v3.cpp:28-31
    if (isbin[i]) {
      const double sd = 1.0 / (hi - lo);                                                                 // :36
      ame_scale[i] = 2.0 * sd * sd / ((double)n * (double)n);                                                // :85
    } else {
      ame_scale[i] = 4.0 / (sigma * sigma * (double)n * (double)n);                                          // :105
    }
  }

  int upload_x_estimate() {                                                                              // X_estimate (:326)
    for (int64_t i = 0; i < pd; ++i) std::memcpy(pin + i * n, Xs + cols[i] * n, (size_t)n * sizeof(double));
    return upload(ctx, dXe, pin, n * pd);
  }

  int coefficients_single() {
    BK_TRY(solveforc(ctx, dQ, n, k, n, dvals, da, lambda, dc, &Le));
    if (!one_pass_over_k()) {
      if (ctx->profile) BK_TRY(prof_begin(ctx, "yhat_gemv", 8.0 * (double)n * (double)n));
      if (implicit) BK_TRY(kernel_op_times(ctx, kop, dc, 1, n, dyhat, n));
      else BK_TRY(gemv(ctx, 0, n, n, 1.0, dK, n, dc, 0.0, dyhat));                                       // yfitted = K c (full K)
      if (ctx->profile) BK_TRY(prof_end(ctx, "yhat_gemv"));
      return BIGKRLS_OK;
    }
    BK_TRY(upload_x_estimate());
    if (ctx->profile) BK_TRY(prof_begin(ctx, "deriv_rows", 8.0 * (double)n * (double)n));
    BK_TRY(deriv_rows(ctx, dK, n, n, n, 0, dXe, pd, n, isbin.data(), dc, sigma, dD, n, dS, n, dyhat,     // + yfitted = K c (:291)
                      verify_pending ? dVU : (const double*)nullptr, verify_pending ? 2 : 0,
                      verify_pending ? dVU + 4 * n : (double*)nullptr,                                  // + K [u_1 u_2]
                      implicit ? &kop : (const KernelOp*)nullptr));
    if (ctx->profile) BK_TRY(prof_end(ctx, "deriv_rows"));
    return verify_pending ? verify_deferred() : (int)BIGKRLS_OK;
  }

  // own rows of c and of K c (K symmetric: K[:, r0:r1)' c), one all-gather each; Le is a sum over the row blocks
  int coefficients_dist() {
    BK_TRY(agreed(nloc > 0 ? solveforc(ctx, dQ + r0, nloc, k, n, dvals, da, lambda, dDloc, &Le) : BIGKRLS_OK));
    BK_TRY(comm_all_reduce_host(comm, &Le, 1, COMM_SUM));
    BK_TRY(comm_gather_rows(comm, dDloc, nloc, std::max<int64_t>(nloc, 1), 1, nb, n, dc, n));
    BK_TRY(agreed(nloc > 0 ? gemv(ctx, 1, n, nloc, 1.0, dK, n, dc, 0.0, dSloc) : BIGKRLS_OK));
    return comm_gather_rows(comm, dSloc, nloc, std::max<int64_t>(nloc, 1), 1, nb, n, dyhat, n);
  }

  int fetch_coefficients() {
    BK_HIP(hipMemcpyAsync(pin, dc, (size_t)(2 * n) * sizeof(double), hipMemcpyDeviceToHost, st));        // dyhat follows dc
    BK_HIP(hipStreamSynchronize(st));
    // (out of the pinned buffer before the status is agreed: the agreement stages its words through the same buffer)
    std::memcpy(coeffs.data(), pin, (size_t)n * sizeof(double));
    std::memcpy(yhat.data(), pin + n, (size_t)n * sizeof(double));
    return BIGKRLS_OK;
  }

  // ---- ... and the variance matrices (:294-307) --------------------------------------------------------------------
  int variance_matrices() {
    sigmasq = kNaN;
    wv.assign((size_t)k, 0.0);
    if (vcov_est) {
      long double rs = 0.0L;
      for (int64_t i = 0; i < n; ++i) {
        const long double r = (long double)ys[i] - yhat[i];
        rs += r * r;
      }
      sigmasq = (double)(rs / (long double)n);                                                           // :294
      for (int64_t i = 0; i < k; ++i) wv[i] = sigmasq * std::pow(vals[i] + lambda, -2.0);                // :299
    }
    // (one local stretch between the collectives of the coefficients and those of the derivative pass: its status is
    //  agreed at the end, so that a rank that fails here does not leave its peers waiting in the next all-gather)
    const bool matrices = vcov_est && (out->d_vcov_c || out->d_vcov_fitted);
    if (matrices || out->d_vcov_q) return agreed(variance_outputs_local(matrices));
    timer.mark();
    timer.mark();
    return BIGKRLS_OK;
  }

  int variance_outputs_local(bool matrices) {
    if (out->d_vcov_q) BK_TRY(hand_out_factors());
    if (matrices) return variance_matrices_local();
    timer.mark();
    timer.mark();
    return BIGKRLS_OK;
  }

  // vcov.est.c = Q diag(w) Q' as its factors: the kept columns of dQ (replicated on every rank of a multi-GPU fit, so
  // no exchange) and w_j = sd(y)^2 wv_j, the weights the fit itself uses times the rescaling of :438
  int hand_out_factors() {
    BK_TRY(copy_matrix(ctx, dQ, n, k, n, out->d_vcov_q, n));
    const double sd2 = y_sd * y_sd;
    for (int64_t i = 0; i < k; ++i) out->vcov_w[i] = sd2 * wv[i];
    out->vcov_q_cols = k;
    return BIGKRLS_OK;
  }

  int variance_matrices_local() {
    void* pm = nullptr;
    BK_TRY(ws_get(ctx, SLOT_FIT_M, n * k * (int64_t)sizeof(double), &pm));
    if (out->d_vcov_c) {
      // vcov.est.c = sd(y)^2 (Q diag(wv)) Q'   (:299-301, :438)
      std::memcpy(pin, wv.data(), (size_t)k * sizeof(double));
      BK_TRY(variance_matrix((double*)pm, out->d_vcov_c));
    }
    timer.mark();                                                           // vcov_c
    if (out->d_vcov_fitted) {
      // :307 crossprod(K, vcovmatc %*% K) == Q diag(wv d^2) Q' on the kept pairs (K Q = Q D):
      // 2 N^2 K flops instead of 4 N^3
      for (int64_t i = 0; i < k; ++i) pin[i] = wv[i] * vals[i] * vals[i];
      BK_TRY(variance_matrix((double*)pm, out->d_vcov_fitted));
    }
    timer.mark();                                                           // vcov_fitted
    return BIGKRLS_OK;
  }

  // d_out = sd(y)^2 (Q diag(w)) Q' with the k weights w staged at the start of the pinned buffer; dM: n x k scratch
  int variance_matrix(double* dM, double* d_out) {
    const double sd2 = y_sd * y_sd;
    BK_TRY(upload(ctx, dw, pin, k));
    BK_TRY(multdiag(ctx, dQ, n, k, n, dw, dM, n));
    if (!comm) {
      if (ctx->profile) BK_TRY(prof_begin(ctx, "vcov_syrk", (double)n * ((double)n + 1.0) * (double)k));
      BK_TRY(syrk_mirror_set(ctx, n, k, sd2, dM, n, dQ, n, d_out, n));
      if (ctx->profile) BK_TRY(prof_end(ctx, "vcov_syrk"));
    } else if (nloc > 0) {   // the column block V[:, r0:r1) = (Q diag(w)) Q[r0:r1, :]': kept sharded, no exchange
      BK_TRY(vcov_cols(ctx, n, k, r0, r1, sd2, dM, dQ, d_out));
    }
    BK_HIP(hipStreamSynchronize(st));
    return BIGKRLS_OK;
  }

  // ---- step 5: marginal effects (:321-376) and their post-processing (:384-409) ------------------------------------
  int marginal_effects() {
    out->R2AME = kNaN;
    if (!derivative) {
      timer.mark();
      return BIGKRLS_OK;
    }
    // (one GPU: the pass over K ran in step 4, where it also produced the fitted values)
    if (comm) BK_TRY(derivatives_dist());
    BK_HIP(hipStreamSynchronize(st));
    std::memcpy(pin, wv.data(), (size_t)k * sizeof(double));
    BK_TRY(upload(ctx, dw, pin, k));
    BK_TRY(deriv_var(ctx, dQ, n, k, n, dw, dS, pd, n, ame_scale.data(), var.data()));
    std::vector<double> D((size_t)n * pd);
    BK_TRY(download(ctx, D.data(), dD, n * pd, pin));
    timer.mark();                                                           // derivatives
    if (trace_on()) {
      BK_TRY(trace_host("R:fit_D", D.data(), n * pd, 0));
      BK_TRY(trace_host("R:fit_var", var.data(), pd, 0));
    }
    if (out->derivatives_std) std::memcpy(out->derivatives_std, D.data(), D.size() * sizeof(double));
    if (out->var_avgderivatives_std) std::memcpy(out->var_avgderivatives_std, var.data(), (size_t)pd * sizeof(double));
    // R2AME in standardised units (:390-392)
    std::vector<double> dmean(pd), yhat_ame(n, 0.0);
    for_columns(pd, n, [&](int64_t i) {
      long double s = 0.0L;
      for (int64_t r = 0; r < n; ++r) s += D[(size_t)i * n + r];
      dmean[i] = (double)(s / (long double)n);
    });
    for (int64_t i = 0; i < pd; ++i) {           // (in column order: the sum's rounding must not depend on threads)
      const double* x = Xs + cols[i] * n;
      for (int64_t r = 0; r < n; ++r) yhat_ame[r] += x[r] * dmean[i];
    }
    const double c_ame = r_cor(h_y, yhat_ame.data(), n);
    out->R2AME = c_ame * c_ame;
    for_columns(pd, n, [&](int64_t i) { rescale_derivative_column(i, D.data() + (size_t)i * n); });
    if (out->derivatives) std::memcpy(out->derivatives, D.data(), D.size() * sizeof(double));
    return BIGKRLS_OK;
  }

  // own rows of D and S from the own column block, one all-gather of each (N x P')
  int derivatives_dist() {
    BK_TRY(upload_x_estimate());
    const int64_t ldl = std::max<int64_t>(nloc, 1);
    BK_TRY(agreed(nloc > 0 ? deriv_rows(ctx, dK, n, nloc, n, r0, dXe, pd, n, isbin.data(), dc, sigma, dDloc, ldl, dSloc, ldl)
                           : BIGKRLS_OK));
    BK_TRY(comm_gather_rows(comm, dDloc, nloc, ldl, pd, nb, n, dD, n));
    return comm_gather_rows(comm, dSloc, nloc, ldl, pd, nb, n, dS, n);
  }

  // rescale: D *= sd(y); column i /= X.init.sd[i] -- index i, not which.derivatives[i] (:394-397, quirk Q6)
  void rescale_derivative_column(int64_t i, double* col) {
    // (which.derivatives may repeat columns, so pd can exceed p: X.init.sd[i] is then NA in R)
    const double f = i < p ? x_sd[i] : kNaN;
    long double s = 0.0L;
    for (int64_t r = 0; r < n; ++r) {
      col[r] = (y_sd * col[r]) / f;
      s += col[r];
    }
    if (out->avgderivatives) out->avgderivatives[i] = (double)(s / (long double)n);                      // :400
    if (out->var_avgderivatives) {
      const double g = y_sd / x_sd[cols[i]];                                                             // :403-407 (correctly subset)
      out->var_avgderivatives[i] = g * g * var[i];
    }
  }

  // ---- Neffective of the ACF rule (:412-416) and the list `w` (:420-469) -------------------------------------------
  int finish() {
    out->Neffective_acf = kNaN;
    if (acf) BK_TRY(neffective(ctx, dX, n, n, p, &out->Neffective_acf));
    if (out->eigenvalues) std::memcpy(out->eigenvalues, vals.data(), (size_t)neig * sizeof(double));
    if (out->coeffs) std::memcpy(out->coeffs, coeffs.data(), (size_t)n * sizeof(double));
    if (out->yfitted_std) std::memcpy(out->yfitted_std, yhat.data(), (size_t)n * sizeof(double));
    {
      // yfitted (:428), R2 = 1 - var(y - yfitted)/sd(y)^2 (:429)
      long double s = 0.0L;
      std::vector<double> res(n);
      for (int64_t i = 0; i < n; ++i) {
        const double yf = yhat[i] * y_sd + y_mean;
        if (out->yfitted) out->yfitted[i] = yf;
        res[i] = h_y[i] - yf;
        s += res[i];
      }
      const long double m = s / (long double)n;
      long double qq = 0.0L;
      for (int64_t i = 0; i < n; ++i) {
        const long double dlt = (long double)res[i] - m;
        qq += dlt * dlt;
      }
      out->R2 = 1.0 - (double)(qq / (long double)(n - 1)) / (y_sd * y_sd);
    }
    out->lastkeeper = lastkeeper;
    out->neig = neig;
    out->n_deriv = pd;
    out->n_probes = nprobes;
    out->sigma = sigma;
    out->lambda = lambda;
    out->Le = Le;
    out->Looe = Le * y_sd;                                                                                // :430
    out->sigmasq = sigmasq;
    out->y_mean = y_mean;
    out->y_sd = y_sd;
    timer.collect(out->phase_s);
    BK_HIP(hipStreamSynchronize(st));
    return BIGKRLS_OK;
  }
};

// bigKRLS() (R/bigKRLS.R:175-470): the phases in the reference's order, and the one loop that redoes a decomposition
// which failed the fit's checks (a fault of the run). Every decision in the loop is taken on
// statuses that the ranks of a multi-GPU fit have agreed, so all of them take the same turn.
int fit_impl(bigkrls_ctx* ctx, bigkrls_comm* comm, const double* h_X, const double* h_y, int64_t n, int64_t p,
             const bigkrls_fit_options* opt, bigkrls_fit_outputs* out, bool neig_auto = false, int64_t neig_max = 0) {
  Fit f(ctx, comm, h_X, h_y, n, p, opt, out);
  f.neig_auto = neig_auto;
  f.neig_max = neig_max;
  BK_TRY(f.validate());
  BK_TRY(f.plan_and_allocate());
  BK_TRY(f.standardise_upload());
  BK_TRY(f.build_kernel());                                                 // step 1
  f.timer_n_before_eigen = f.timer.n;
  for (;;) {
    int rc = f.decompose();                                                 // step 2, one attempt
    if (rc == BIGKRLS_OK) {
      rc = f.check_decomposition();
      if (f.nans_are_final(rc)) return Fit::missing_eigenvalues();
    }
    const bool decomposed = rc == BIGKRLS_OK;                               // (what fails from here on is the deferred check)
    if (decomposed) rc = f.accept_decomposition();
    if (rc == BIGKRLS_OK) rc = f.search_lambda();                           // step 3
    if (rc == BIGKRLS_OK) rc = f.coefficients_and_fitted();                 // step 4
    if (rc == BIGKRLS_OK) break;
    if (rc != BK_EWATCHDOG) return rc;
    BK_TRY(f.redo_or_give_up(decomposed ? Fit::DEFERRED : Fit::IMMEDIATE));
  }
  BK_TRY(f.variance_matrices());
  BK_TRY(f.marginal_effects());                                             // step 5
  return f.finish();
}

// ---- predict.bigKRLS() (R/bigKRLS.R:590-621): what the whole-matrix and the pointwise entries share ----------------
struct TrainMoments {
  std::vector<double> x_mean, x_sd;
  double y_mean = 0.0, y_sd = 0.0;
};

// the argument checks and the TRAINING means and sds both are standardised with (:590-597)
int predict_prepare(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y, const double* h_coeffs,
                    double sigma, const double* h_newdata, int64_t u, const double* h_predicted, bool want_se,
                    const Vcov& vc, TrainMoments* tm) {
  BK_TRY(check_ctx(ctx));
  BK_REQUIRE(h_X && h_y && h_coeffs && h_newdata && h_predicted, "predict: null argument");
  BK_REQUIRE(n > 1 && p > 0 && u > 0 && sigma > 0.0, "predict: bad dimensions or sigma");
  if (want_se && !vc.given()) {
    set_error("recompute bigKRLS object with bigKRLS(,vcov.est=TRUE) to compute standard errors");     // R/bigKRLS.R:553
    return BIGKRLS_EINVAL;
  }
  if (vc.d_Q) BK_REQUIRE(vc.h_w && vc.k > 0 && vc.k <= n && vc.ldq >= n, "predict: bad factors of vcov.est.c");
  tm->x_mean.resize(p);
  tm->x_sd.resize(p);
  for (int64_t j = 0; j < p; ++j) {
    mean_sd(h_X + j * n, n, &tm->x_mean[j], &tm->x_sd[j]);
    if (tm->x_sd[j] == 0.0) {
      set_error("predict: a training column is constant");
      return BIGKRLS_EINVAL;
    }
  }
  mean_sd(h_y, n, &tm->y_mean, &tm->y_sd);
  return BIGKRLS_OK;
}

// [yhat | diag of vcov.est.pred] (device, 2 u) through `pinned`: predicted = yhat sd(y) + mean(y) (:621), se.pred (:613)
int predict_finish(bigkrls_ctx* ctx, const double* dpred, int64_t u, bool want_se, double* pinned, const TrainMoments& tm,
                   double* h_predicted, double* h_se_pred) {
  BK_HIP(hipMemcpyAsync(pinned, dpred, (size_t)(want_se ? 2 * u : u) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  BK_HIP(hipStreamSynchronize(ctx->stream));
  for (int64_t i = 0; i < u; ++i) h_predicted[i] = pinned[i] * tm.y_sd + tm.y_mean;
  if (h_se_pred)
    for (int64_t i = 0; i < u; ++i) h_se_pred[i] = std::sqrt(pinned[u + i]);
  return BIGKRLS_OK;
}

// bigkrls_predict / bigkrls_predict_factored with a device output: the u x n test kernel as a whole
int predict_whole(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y, const double* h_coeffs,
                  double sigma, const double* h_newdata, int64_t u, const Vcov& vc, double neff, double* h_predicted,
                  double* h_se_pred, double* d_newdataK, double* d_vcov_pred) {
  const bool want_se = h_se_pred != nullptr || d_vcov_pred != nullptr;
  TrainMoments tm;
  BK_TRY(predict_prepare(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_newdata, u, h_predicted, want_se, vc, &tm));
  hipStream_t st = ctx->stream;
  const int64_t k = want_se ? vc.cols() : 0;
  const int64_t small_doubles = n * p + u * p + n + k + 2 * u + 64;
  void* psmall = nullptr;
  BK_TRY(ws_get(ctx, SLOT_FIT_SMALL, small_doubles * (int64_t)sizeof(double), &psmall));
  double* q = (double*)psmall;
  double* dX = q; q += n * p;
  double* dN = q; q += u * p;
  double* dc = q; q += n;
  double* dw = q; q += k;
  double* dpred = q; q += u;
  double* ddiag = q; q += u;
  double* dKn = d_newdataK;
  if (!dKn) {
    void* pk = nullptr;
    BK_TRY(ws_get(ctx, SLOT_FIT_K, u * n * (int64_t)sizeof(double), &pk));
    dKn = (double*)pk;
  }
  double* pin = nullptr;
  BK_TRY(pinned_get(ctx, n * p + u * p + n + k + u, &pin));
  for (int64_t j = 0; j < p; ++j) {
    standardise_column(h_X + j * n, n, tm.x_mean[j], tm.x_sd[j], pin + j * n);
    standardise_column(h_newdata + j * u, u, tm.x_mean[j], tm.x_sd[j], pin + n * p + j * u);
  }
  std::memcpy(pin + n * p + u * p, h_coeffs, (size_t)n * sizeof(double));
  if (k > 0) std::memcpy(pin + n * p + u * p + n, vc.h_w, (size_t)k * sizeof(double));
  BK_HIP(hipMemcpyAsync(dX, pin, (size_t)(n * p + u * p + n + k) * sizeof(double), hipMemcpyHostToDevice, st));
  BK_TRY(kernel_block(ctx, dN, u, u, dX, n, n, p, sigma, dKn, u, -1));                                 // bTempKernel (:599)
  BK_TRY(gemv(ctx, 0, u, n, 1.0, dKn, u, dc, 0.0, dpred));                                            // newdataK %*% coeffs (:601)
  const double q10 = neff > 0.0 ? std::sqrt((double)n / neff) : 1.0;                                   // :610-611 (quirk Q10)
  if (want_se && vc.d_V) {
    const double vy = tm.y_sd * tm.y_sd;
    void* pm = nullptr;
    BK_TRY(ws_get(ctx, SLOT_FIT_M, (u * n + (d_vcov_pred ? 0 : u * u)) * (int64_t)sizeof(double), &pm));
    double* dT = (double*)pm;
    double* dVp = d_vcov_pred ? d_vcov_pred : dT + u * n;
    // var(y) * tcrossprod(newdataK %*% (vcov.est.c * (1/var(y))), newdataK)   (:608)
    BK_TRY(gemm(ctx, 0, 0, u, n, n, 1.0 / vy, dKn, u, vc.d_V, n, 0.0, dT, u));
    BK_TRY(gemm(ctx, 0, 1, u, u, n, vy, dT, u, dKn, u, 0.0, dVp, u));
    if (neff > 0.0) BK_TRY(scale(ctx, u * u, q10, dVp));
    BK_TRY(diag_extract(ctx, dVp, u, u, ddiag));
  } else if (want_se) {
    // the same matrix from the factors: T = newdataK Q, vcov.est.pred = (T diag(w)) T', its diagonal sum_j w_j T_ij^2
    void* pm = nullptr;
    BK_TRY(ws_get(ctx, SLOT_FIT_M, (d_vcov_pred ? 2 : 1) * u * k * (int64_t)sizeof(double), &pm));
    double* dT = (double*)pm;
    BK_TRY(gemm(ctx, 0, 0, u, k, n, 1.0, dKn, u, vc.d_Q, vc.ldq, 0.0, dT, u));
    BK_TRY(rowsumsq_weighted(ctx, u, k, dT, u, dw, ddiag));
    if (neff > 0.0) BK_TRY(scale(ctx, u, q10, ddiag));
    if (d_vcov_pred) {
      double* dM = dT + u * k;
      BK_TRY(multdiag(ctx, dT, u, k, u, dw, dM, u));
      BK_TRY(gemm(ctx, 0, 1, u, u, k, q10, dM, u, dT, u, 0.0, d_vcov_pred, u));
    }
  }
  return predict_finish(ctx, dpred, u, want_se, pin, tm, h_predicted, h_se_pred);
}

// bigkrls_predict_pointwise / bigkrls_predict_factored without device outputs: bigkrls_predict's validation and
// standardisation; then row blocks of b new points: kernel_block, gemv, and for the SEs the one entry of vcov.est.pred
// per point that se.pred needs -- diag(Kn_b vcov.est.c Kn_b') (quadform_diag), or from the factors T = Kn_b Q (gemm)
// and sum_j w_j T_ij^2 (rowsumsq_weighted).
int predict_blocks(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y, const double* h_coeffs,
                   double sigma, const double* h_newdata, int64_t u, const Vcov& vc, double neff, double* h_predicted,
                   double* h_se_pred) {
  const bool want_se = h_se_pred != nullptr;
  TrainMoments tm;
  BK_TRY(predict_prepare(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_newdata, u, h_predicted, want_se, vc, &tm));
  const int64_t k = want_se ? vc.cols() : 0;
  const int64_t b = std::min(pointwise_block_rows(n, k), u);
  hipStream_t st = ctx->stream;
  const int64_t small_doubles = n * p + n + k + b * p + 2 * u + 64;
  void* psmall = nullptr;
  BK_TRY(ws_get(ctx, SLOT_PP_SMALL, small_doubles * (int64_t)sizeof(double), &psmall));
  double* q = (double*)psmall;
  double* dX = q; q += n * p;
  double* dc = q; q += n;
  double* dw = q; q += k;
  double* dZ = q; q += b * p;
  double* dpred = q; q += u;
  double* ddiag = q; q += u;
  void* pk = nullptr;
  BK_TRY(ws_get(ctx, SLOT_PP_K, b * (n + k) * (int64_t)sizeof(double), &pk));
  double* dKn = (double*)pk;
  double* dT = dKn + b * n;
  // pinned host: [Xs | c | w | Zs, block by block, each block's rows x p contiguous] uploaded, [yhat | diag] read back
  double* pin = nullptr;
  BK_HIP(hipStreamSynchronize(st));   // (the pinned buffer may be reallocated)
  BK_TRY(pinned_get(ctx, n * p + n + k + u * p + 2 * u, &pin));
  double* pz = pin + n * p + n + k;
  double* pout = pz + u * p;
  for (int64_t j = 0; j < p; ++j) {
    standardise_column(h_X + j * n, n, tm.x_mean[j], tm.x_sd[j], pin + j * n);
    for (int64_t r0 = 0; r0 < u; r0 += b) {
      const int64_t rows = std::min(b, u - r0);
      standardise_column(h_newdata + j * u + r0, rows, tm.x_mean[j], tm.x_sd[j], pz + r0 * p + j * rows);
    }
  }
  std::memcpy(pin + n * p, h_coeffs, (size_t)n * sizeof(double));
  if (k > 0) std::memcpy(pin + n * p + n, vc.h_w, (size_t)k * sizeof(double));
  BK_HIP(hipMemcpyAsync(dX, pin, (size_t)(n * p + n + k) * sizeof(double), hipMemcpyHostToDevice, st));
  for (int64_t r0 = 0; r0 < u; r0 += b) {
    const int64_t rows = std::min(b, u - r0);
    BK_HIP(hipMemcpyAsync(dZ, pz + r0 * p, (size_t)(rows * p) * sizeof(double), hipMemcpyHostToDevice, st));
    BK_TRY(kernel_block(ctx, dZ, rows, rows, dX, n, n, p, sigma, dKn, rows, -1));                       // bTempKernel (:599)
    BK_TRY(gemv(ctx, 0, rows, n, 1.0, dKn, rows, dc, 0.0, dpred + r0));                                // :601
    if (want_se && vc.d_V) {
      BK_TRY(quadform_diag(ctx, rows, n, dKn, rows, vc.d_V, n, ddiag + r0));                            // diag of :608
    } else if (want_se) {
      BK_TRY(gemm(ctx, 0, 0, rows, k, n, 1.0, dKn, rows, vc.d_Q, vc.ldq, 0.0, dT, rows));               // T = Kn_b Q
      BK_TRY(rowsumsq_weighted(ctx, rows, k, dT, rows, dw, ddiag + r0));
    }
  }
  if (want_se && neff > 0.0) BK_TRY(scale(ctx, u, std::sqrt((double)n / neff), ddiag));                // :610-611 (Q10)
  return predict_finish(ctx, dpred, u, want_se, pout, tm, h_predicted, h_se_pred);
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bigkrls_fit(bigkrls_ctx* ctx, const double* h_X, const double* h_y, int64_t n, int64_t p,
                const bigkrls_fit_options* opt, bigkrls_fit_outputs* out) {
  return fit_impl(ctx, nullptr, h_X, h_y, n, p, opt, out);
}

int bigkrls_fit_auto(bigkrls_ctx* ctx, const double* h_X, const double* h_y, int64_t n, int64_t p,
                     const bigkrls_fit_options* opt, int64_t neig_max, bigkrls_fit_outputs* out) {
  return fit_impl(ctx, nullptr, h_X, h_y, n, p, opt, out, true, neig_max);
}

int bigkrls_fit_dist_rows(bigkrls_comm* comm, int64_t n, const bigkrls_fit_options* opt, int64_t* r0, int64_t* r1) {
  BK_REQUIRE(comm && opt && r0 && r1 && n > 1, "fit_dist_rows: bad arguments");
  BK_REQUIRE(opt->struct_bytes == (int64_t)sizeof(bigkrls_fit_options), "fit_dist_rows: options struct size mismatch");
  int mode = 0;
  int64_t nb = 0;
  return dist_plan(comm, n, opt, &mode, &nb, r0, r1);
}

int bigkrls_fit_dist(bigkrls_comm* comm, const double* h_X, const double* h_y, int64_t n, int64_t p,
                     const bigkrls_fit_options* opt, bigkrls_fit_outputs* out) {
  BK_REQUIRE(comm && comm->ctx, "fit_dist: the communicator has no context");
  return fit_impl(comm->ctx, comm, h_X, h_y, n, p, opt, out);
}

int bigkrls_predict(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                    const double* h_coeffs, double sigma, const double* h_newdata, int64_t u,
                    const double* d_vcov_c, double neff, double* h_predicted, double* h_se_pred,
                    double* d_newdataK, double* d_vcov_pred) {
  const Vcov vc = Vcov::matrix(d_vcov_c);
  return predict_whole(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_newdata, u, vc, neff, h_predicted, h_se_pred, d_newdataK,
                       d_vcov_pred);
}

int bigkrls_predict_pointwise(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                              const double* h_coeffs, double sigma, const double* h_newdata, int64_t u,
                              const double* d_vcov_c, double neff, double* h_predicted, double* h_se_pred) {
  const Vcov vc = Vcov::matrix(d_vcov_c);
  return predict_blocks(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_newdata, u, vc, neff, h_predicted, h_se_pred);
}

int bigkrls_predict_factored(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                             const double* h_coeffs, double sigma, const double* h_newdata, int64_t u,
                             const double* d_Q, int64_t ldq, int64_t k, const double* h_w, double neff,
                             double* h_predicted, double* h_se_pred, double* d_newdataK, double* d_vcov_pred) {
  const Vcov vc = Vcov::factors(d_Q, ldq, k, h_w);
  if (d_newdataK || d_vcov_pred)
    return predict_whole(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_newdata, u, vc, neff, h_predicted, h_se_pred,
                         d_newdataK, d_vcov_pred);
  return predict_blocks(ctx, h_X, n, p, h_y, h_coeffs, sigma, h_newdata, u, vc, neff, h_predicted, h_se_pred);
}

}  // extern "C"
