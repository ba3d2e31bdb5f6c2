// Heteroskedasticity- and cluster-robust variance of the coefficients as factors (no counterpart in the reference).
//
// With Q (n x k) and d the kept eigenpairs of the fit, g_j = 1 / (d_j + lambda) and G = Q diag(g) Q', the fit's own
// variance is sigmasq G G. The sandwich replaces the scalar by the rows' own weights:
//   V_r = G diag(omega) G = Q diag(g) M diag(g) Q',   M = Q' diag(omega) Q   (k x k)
// and with S = diag(g) M diag(g) = U diag(theta) U' (a k x k eigenproblem)
//   V_r = (Q U) diag(theta) (Q U)',
// the (vcov.est.Q, vcov.est.w) form everything after the fit already consumes. Clustered: M = S_c S_c' with
// S_c[j, c] = sum_{i in cluster c} e_i Q_ij, the per-cluster score sums. The O(n) work is the weighted Gram matrix
// (gram_weighted, csrc/gemm.hip) or the cluster scores (cluster_scores, below), the leverages and the rotation Q U.
// Type 5, CR3 (the cluster jackknife): the same clustered middle on the deletion residuals (I - H_SS)^-1 e_S of every
// cluster (deletion_residuals, csrc/influence.hip) in place of e.
//
// cluster_scores: the host makes a stable counting sort of the labels (rows of one cluster in their original order)
// and cuts the sorted rows into pieces: maximal runs of one cluster inside one 64-row chunk. One wave takes a chunk
// and 16 columns: lane l holds e A of sorted row 64 c + l, a segmented tree reduction over the lanes (six shuffle
// steps, masks computed once per chunk) leaves every piece's sum in its first lane, and the sums go through an LDS
// tile so that the 16 columns of a piece are stored as one 128-byte segment. A piece that is a whole cluster is stored
// straight into S; the pieces of a cluster that spans chunks go to a k x pieces scratch and a second kernel adds them
// in piece order (and zeroes the empty clusters). The order of every sum depends on the cluster sizes only: no atomics,
// two calls give the same bits. Rows already grouped (identity permutation) are read without the indirection, 64
// consecutive doubles of a column per wave; G = n needs no second pass at all.
#include "hostprep.h"
#include "ktplan.h"

#include <cstring>

namespace bk {
namespace {

constexpr int CS_ROWS = 64;     // rows per chunk: one wave
constexpr int CS_COLS = 16;     // columns per wave
constexpr int CS_WAVES = 4;     // waves per workgroup: 64 columns
constexpr int CS_LD = CS_COLS + 1;
constexpr long long CS_NONE = INT64_MIN;

__global__ __launch_bounds__(CS_ROWS * CS_WAVES) void cluster_scores_kernel(
    int n, int k, const double* __restrict__ A, int64_t lda, const double* __restrict__ e, const int* __restrict__ perm,
    const int* __restrict__ row_piece, const long long* __restrict__ piece_dst, double* __restrict__ S,
    double* __restrict__ P) {
  __shared__ double tile[CS_WAVES][CS_ROWS * CS_LD];
  __shared__ long long dst[CS_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * CS_ROWS + lane;
  const bool valid = r < n;
  const int rc = valid ? (int)r : n - 1;
  const int src = perm ? perm[rc] : rc;
  const double ev = valid ? e[src] : 0.0;
  const int pid = valid ? row_piece[rc] : -1;
  // the pieces of this chunk: heads, the last lane of every lane's piece, the rank of a head among the heads
  const int prev = __shfl_up(pid, 1);
  const bool head = lane == 0 || pid != prev;
  const unsigned long long H = __ballot(head);
  const unsigned long long above = lane == 63 ? 0ull : (H >> (lane + 1)) << (lane + 1);
  const int last = above ? __ffsll((long long)above) - 2 : 63;
  const int rank = __popcll(H & ((1ull << lane) - 1ull));
  const int nheads = __popcll(H);
  if (wave == 0 && head) dst[rank] = valid ? piece_dst[pid] : CS_NONE;
  const int j0 = (blockIdx.y * CS_WAVES + wave) * CS_COLS;
  double x[CS_COLS];
#pragma unroll
  for (int jj = 0; jj < CS_COLS; ++jj) {
    const int j = j0 + jj < k ? j0 + jj : k - 1;
    x[jj] = A[(int64_t)src + (int64_t)j * lda];
  }
#pragma unroll
  for (int jj = 0; jj < CS_COLS; ++jj) {
    double v = valid ? x[jj] * ev : 0.0;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const double o = __shfl_down(v, s);
      if (lane + s <= last) v += o;
    }
    if (head) tile[wave][rank * CS_LD + jj] = v;
  }
  __syncthreads();
  const int jj = lane & 15, j = j0 + jj;
  for (int s0 = 0; s0 < nheads; s0 += 4) {     // (nheads is the same in every wave: the same rows)
    const int slot = s0 + (lane >> 4);
    if (slot < nheads && j < k) {
      const long long d = dst[slot];
      if (d != CS_NONE) {
        double* o = d >= 0 ? S + d : P + (-(d + 1));
        o[j] = tile[wave][slot * CS_LD + jj];
      }
    }
  }
}

// the clusters of several pieces (and the empty ones, count 0): S[:, g] = the pieces' sums. A workgroup takes 256 / nsl
// columns; the piece range of a cluster is cut into nsl equal slices (nsl = 1 or 16, chosen by the host from the largest
// piece count), slice q adds its pieces in piece order and the slices' sums are added in slice order: a long cluster
// (G = 2: n / 128 pieces) is not one thread's serial chain, and the order still depends on the sizes only.
__global__ __launch_bounds__(256) void cluster_combine_kernel(int k, int nmulti, int nsl, const int* __restrict__ multi,
                                                              const double* __restrict__ P, double* __restrict__ S,
                                                              int64_t lds) {
  __shared__ double part[256];
  const int cpb = 256 / nsl;
  const int c = threadIdx.x % cpb, q = threadIdx.x / cpb;
  const int j = blockIdx.x * cpb + c;
  for (int i = blockIdx.y; i < nmulti; i += gridDim.y) {     // (uniform over the workgroup: the barriers are safe)
    const int g = multi[3 * i], pb = multi[3 * i + 1], pc = multi[3 * i + 2];
    const int len = (pc + nsl - 1) / nsl;
    const int q0 = min(q * len, pc), q1 = min(q0 + len, pc);
    double s = 0.0;
    if (j < k) {
      const double* p = P + (int64_t)pb * k + j;
      int r = q0;
      for (; r + 4 <= q1; r += 4) {
        const double a0 = p[(int64_t)(r + 0) * k], a1 = p[(int64_t)(r + 1) * k];
        const double a2 = p[(int64_t)(r + 2) * k], a3 = p[(int64_t)(r + 3) * k];
        s += a0; s += a1; s += a2; s += a3;
      }
      for (; r < q1; ++r) s += p[(int64_t)r * k];
    }
    if (nsl > 1) {
      part[threadIdx.x] = s;
      __syncthreads();
      if (q == 0)
        for (int t = 1; t < nsl; ++t) s += part[t * cpb + c];
      __syncthreads();
    }
    if (q == 0 && j < k) S[(int64_t)j + (int64_t)g * lds] = s;
  }
}

// omega by type (include/bigkrls.h); *bad_row = the first row whose leverage is >= 1 (types 3 and 4)
__global__ void omega_kernel(int n, int type, const double* __restrict__ e, const double* __restrict__ h,
                             double* __restrict__ omega, int* __restrict__ bad_row) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double w = 1.0;
  if (type != 0) {
    w = e[i] * e[i];
    if (type >= 3) {
      const double hi = h[i];
      if (!(hi < 1.0)) atomicMin(bad_row, i);
      const double om = 1.0 - hi;
      w = type == 3 ? w / om : w / (om * om);
    }
  }
  omega[i] = w;
}

// S = diag(g) M diag(g), symmetrised: S[i,j] = (g_i g_j) (M[i,j] + M[j,i]) / 2 -- the same bits at (j, i). The scalar
// `scale` stays outside the eigenproblem (it multiplies theta): HC1 is HC0 times its factor to the last bit but one.
__global__ void sandwich_kernel(int k, const double* __restrict__ M, const double* __restrict__ g,
                                double* __restrict__ S) {
  const int64_t total = (int64_t)k * k;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e % k), j = (int)(e / k);
    const double sym = 0.5 * (M[(int64_t)i + (int64_t)j * k] + M[(int64_t)j + (int64_t)i * k]);
    S[e] = (g[i] * g[j]) * sym;
  }
}

// The sorted rows cut into pieces (maximal runs of one cluster inside one 64-row chunk): the piece of every sorted row,
// where every piece's sum goes (>= 0: the offset of the cluster's column in S; < 0: -(offset in the scratch) - 1), and
// (cluster, first scratch column, pieces) of the clusters that are not one piece, the empty ones with 0 pieces.
struct ClusterPieces {
  std::vector<int32_t> row_piece, multi;
  std::vector<long long> piece_dst;
  int64_t ncolsP = 0, max_pieces = 0;   // scratch columns; the most pieces of one cluster
};
ClusterPieces cluster_pieces(const std::vector<int64_t>& off, int64_t n, int64_t G, int64_t k, int64_t lds) {
  ClusterPieces pc;
  pc.row_piece.resize((size_t)n);
  for (int64_t g = 0; g < G; ++g) {
    const int64_t b = off[(size_t)g], t = off[(size_t)g + 1];
    if (b == t) {
      pc.multi.insert(pc.multi.end(), {(int32_t)g, 0, 0});
      continue;
    }
    const int64_t c0 = b / CS_ROWS, c1 = (t - 1) / CS_ROWS;
    if (c1 > c0) pc.multi.insert(pc.multi.end(), {(int32_t)g, (int32_t)pc.ncolsP, (int32_t)(c1 - c0 + 1)});
    if (c1 > c0) pc.max_pieces = std::max(pc.max_pieces, c1 - c0 + 1);
    for (int64_t c = c0; c <= c1; ++c) {
      const int64_t rb = std::max(b, c * CS_ROWS), re = std::min(t, (c + 1) * CS_ROWS);
      for (int64_t r = rb; r < re; ++r) pc.row_piece[(size_t)r] = (int32_t)pc.piece_dst.size();
      pc.piece_dst.push_back(c1 == c0 ? (long long)(g * lds) : -(long long)(pc.ncolsP++ * k) - 1);
    }
  }
  return pc;
}

}  // namespace

int cluster_scores(bigkrls_ctx* ctx, int64_t n, int64_t k, const double* A, int64_t lda, const double* e,
                   const int64_t* h_cluster, int64_t G, double* S, int64_t lds) {
  BK_REQUIRE(n >= 0 && k >= 0 && n < (1ll << 31) && k < (1ll << 31), "cluster_scores: bad dimensions");
  BK_REQUIRE(G >= 1 && G < (1ll << 31), "cluster_scores: G must be at least 1");
  BK_REQUIRE(n == 0 || h_cluster, "cluster_scores: null labels");
  // stable counting sort (csrc/ktplan.h): the rows of one cluster in their original order
  const GroupOrder go = group_order(h_cluster, n, G);
  BK_REQUIRE(go.bad < 0, "cluster_scores: the label of row " + std::to_string(go.bad + 1) + " is outside [0, G)");
  if (k == 0) return BIGKRLS_OK;
  BK_REQUIRE(S && lds >= k, "cluster_scores: null S or leading dimension of S too small");
  BK_REQUIRE(n == 0 || (A && e), "cluster_scores: null pointer");
  BK_REQUIRE(lda >= n, "cluster_scores: leading dimension of A too small");
  BK_REQUIRE(G * lds < (1ll << 62) / 8, "cluster_scores: S too large");
  hipStream_t st = ctx->stream;

  // ---- the pieces ----------------------------------------------------------------------------------------------
  const std::vector<int32_t>& perm = go.perm;
  const bool identity = perm.empty();   // (no row moves: the labels never decrease)
  const ClusterPieces pc = cluster_pieces(go.off, n, G, k, lds);
  const std::vector<int32_t>&row_piece = pc.row_piece, &multi = pc.multi;
  const std::vector<long long>& piece_dst = pc.piece_dst;
  const int64_t ncolsP = pc.ncolsP, max_pieces = pc.max_pieces;
  const int64_t npieces = (int64_t)piece_dst.size(), nmulti = (int64_t)multi.size() / 3;
  BK_REQUIRE(ncolsP < (1ll << 31), "cluster_scores: too many pieces");

  // ---- upload (pinned), launch ---------------------------------------------------------------------------------
  const int64_t b_perm = identity ? 0 : (n * 4 + 7) / 8 * 8, b_rp = (n * 4 + 7) / 8 * 8, b_pd = npieces * 8;
  const int64_t b_mu = (nmulti * 12 + 7) / 8 * 8, b_all = b_perm + b_rp + b_pd + b_mu;
  void* pidx = nullptr;
  void* ppart = nullptr;
  BK_TRY(ws_get(ctx, SLOT_CS_INDEX, b_all + 64, &pidx));
  BK_TRY(ws_get(ctx, SLOT_CS_PART, std::max<int64_t>(ncolsP, 1) * k * (int64_t)sizeof(double), &ppart));
  char* dbase = (char*)pidx;
  const int* d_perm = identity ? nullptr : (const int*)dbase;
  const int* d_rp = (const int*)(dbase + b_perm);
  const long long* d_pd = (const long long*)(dbase + b_perm + b_rp);
  const int* d_mu = (const int*)(dbase + b_perm + b_rp + b_pd);
  if (b_all > 0) {
    double* pin = nullptr;
    BK_HIP(hipStreamSynchronize(st));   // (the pinned buffer may be in use or reallocated)
    BK_TRY(pinned_get(ctx, b_all / 8 + 8, &pin));
    char* hb = (char*)pin;
    if (!identity) std::memcpy(hb, perm.data(), (size_t)n * 4);
    if (n > 0) std::memcpy(hb + b_perm, row_piece.data(), (size_t)n * 4);
    if (npieces > 0) std::memcpy(hb + b_perm + b_rp, piece_dst.data(), (size_t)npieces * 8);
    if (nmulti > 0) std::memcpy(hb + b_perm + b_rp + b_pd, multi.data(), (size_t)nmulti * 12);
    BK_HIP(hipMemcpyAsync(dbase, hb, (size_t)b_all, hipMemcpyHostToDevice, st));
  }
  BK_TRY(prof_begin(ctx, "cluster_scores", 8.0 * (double)n * (double)k));
  if (n > 0) {
    const dim3 grid((unsigned)((n + CS_ROWS - 1) / CS_ROWS), (unsigned)((k + CS_COLS * CS_WAVES - 1) / (CS_COLS * CS_WAVES)));
    hipLaunchKernelGGL(cluster_scores_kernel, grid, dim3(CS_ROWS * CS_WAVES), 0, st, (int)n, (int)k, A, lda, e, d_perm,
                       d_rp, d_pd, S, (double*)ppart);
    BK_CHECK_LAUNCH();
  }
  if (nmulti > 0) {
    const int nsl = max_pieces >= 32 ? 16 : 1;
    const int cpb = 256 / nsl;
    const dim3 grid((unsigned)((k + cpb - 1) / cpb), (unsigned)std::min<int64_t>(nmulti, 4096));
    hipLaunchKernelGGL(cluster_combine_kernel, grid, dim3(256), 0, st, (int)k, (int)nmulti, nsl, d_mu, (const double*)ppart, S,
                       lds);
    BK_CHECK_LAUNCH();
  }
  BK_TRY(prof_end(ctx, "cluster_scores"));
  return BIGKRLS_OK;
}

}  // namespace bk

using namespace bk;

extern "C" {

int bigkrls_dev_gram_weighted(bigkrls_ctx* ctx, int64_t n, int64_t k, const double* A, int64_t lda, const double* omega,
                              double* M, int64_t ldm) {
  BK_TRY(check_ctx(ctx));
  return gram_weighted(ctx, n, k, A, lda, omega, M, ldm);
}

int bigkrls_dev_cluster_scores(bigkrls_ctx* ctx, int64_t n, int64_t k, const double* A, int64_t lda, const double* e,
                               const int64_t* h_cluster, int64_t G, double* S, int64_t lds) {
  BK_TRY(check_ctx(ctx));
  return cluster_scores(ctx, n, k, A, lda, e, h_cluster, G, S, lds);
}

int bigkrls_vcov_robust(bigkrls_ctx* ctx, int64_t n, int64_t k, const double* d_Q, int64_t ldq, const double* h_d,
                        double lambda, const double* h_resid, double y_sd, double scale, int32_t type,
                        const int64_t* h_cluster, int64_t G, double* d_Qout, int64_t ldqo, double* h_wout) {
  BK_TRY(check_ctx(ctx));
  BK_REQUIRE(d_Q && h_d && d_Qout && h_wout, "vcov_robust: null argument");
  BK_REQUIRE(n >= 1 && k >= 1 && k <= n && n < (1ll << 31), "vcov_robust: bad dimensions");
  BK_REQUIRE(ldq >= n && ldqo >= n, "vcov_robust: leading dimension of Q or Qout too small");
  {
    const char* a0 = (const char*)d_Q;
    const char* a1 = a0 + ((k - 1) * ldq + n) * (int64_t)sizeof(double);
    const char* b0 = (const char*)d_Qout;
    const char* b1 = b0 + ((k - 1) * ldqo + n) * (int64_t)sizeof(double);
    BK_REQUIRE(a1 <= b0 || b1 <= a0, "vcov_robust: Qout must not alias Q");
  }
  BK_REQUIRE(type >= 0 && type <= 5 && (type != 5 || h_cluster),
             "vcov_robust: type must be 0 (classical), 1 (HC0), 2 (HC1), 3 (HC2) or 4 (HC3), or 5 (CR3) with clusters");
  BK_REQUIRE(type == 0 || h_resid, "vcov_robust: the residuals are required for every type but 0");
  BK_REQUIRE(!h_cluster || type == 1 || type == 2 || type == 5,
             "vcov_robust: clusters go with type 1 or 2 (the scale is the caller's) or 5");
  BK_REQUIRE(std::isfinite(lambda) && std::isfinite(scale) && scale >= 0.0, "vcov_robust: lambda and scale must be finite, scale >= 0");
  BK_REQUIRE(y_sd > 0.0 && std::isfinite(y_sd), "vcov_robust: y_sd must be positive");
  for (int64_t j = 0; j < k; ++j)
    BK_REQUIRE(std::isfinite(h_d[j]) && h_d[j] + lambda > 0.0, "vcov_robust: d_j + lambda must be positive");
  if (type != 0)
    for (int64_t i = 0; i < n; ++i) BK_REQUIRE(std::isfinite(h_resid[i]), "vcov_robust: the residuals contain missing or infinite values");
  if (h_cluster) {
    BK_REQUIRE(G >= 1 && G < (1ll << 31), "vcov_robust: G must be at least 1");
    for (int64_t i = 0; i < n; ++i)
      BK_REQUIRE(h_cluster[i] >= 0 && h_cluster[i] < G, "vcov_robust: the label of row " + std::to_string(i + 1) + " is outside [0, G)");
  }
  hipStream_t st = ctx->stream;
  const bool lev = type >= 3;
  const int64_t kG = h_cluster ? k * G : 0;

  // ---- device layout: O(k^2 + n + k G) doubles -------------------------------------------------------------------
  void* psmall = nullptr;
  BK_TRY(ws_get(ctx, SLOT_RV_SMALL, (2 * k + 3 * n + 3 * k * k + k + kG + 64) * (int64_t)sizeof(double), &psmall));
  double* qd = (double*)psmall;
  double* dg = qd; qd += k;
  double* ddg = qd; qd += k;
  double* de = qd; qd += n;
  double* dh = qd; qd += n;
  double* dom = qd; qd += n;
  double* dM = qd; qd += k * k;
  double* dS = qd; qd += k * k;
  double* dU = qd; qd += k * k;
  double* dth = qd; qd += k;
  int* dflag = (int*)qd; qd += 1;
  double* dSc = qd;

  // ---- upload g, d g, the residuals ------------------------------------------------------------------------------
  double* pin = nullptr;
  BK_HIP(hipStreamSynchronize(st));   // (the pinned buffer may be reallocated)
  BK_TRY(pinned_get(ctx, 2 * k + n + 8, &pin));
  for (int64_t j = 0; j < k; ++j) {
    pin[j] = 1.0 / (h_d[j] + lambda);
    pin[k + j] = h_d[j] * pin[j];
  }
  if (type != 0) std::memcpy(pin + 2 * k, h_resid, (size_t)n * sizeof(double));
  BK_HIP(hipMemcpyAsync(dg, pin, (size_t)(2 * k + (type != 0 ? n : 0)) * sizeof(double), hipMemcpyHostToDevice, st));

  // ---- M --------------------------------------------------------------------------------------------------------
  if (h_cluster) {
    // CR3, the cluster jackknife: CR0's machinery on the deletion residuals (csrc/influence.hip; dh is free here)
    if (type == 5) BK_TRY(deletion_residuals(ctx, n, k, d_Q, ldq, ddg, de, h_cluster, G, 0, dh, nullptr, nullptr, 0));
    BK_TRY(cluster_scores(ctx, n, k, d_Q, ldq, type == 5 ? dh : de, h_cluster, G, dSc, k));
    BK_TRY(gemm(ctx, 0, 1, k, k, G, 1.0, dSc, k, dSc, k, 0.0, dM, k));
  } else {
    if (lev) {
      BK_TRY(rowsumsq_weighted(ctx, n, k, d_Q, ldq, ddg, dh));          // h_i = sum_j Q_ij^2 d_j g_j
      BK_HIP(hipMemsetAsync(dflag, 0x7f, sizeof(int), st));
    }
    hipLaunchKernelGGL(omega_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (int)n, (int)type,
                       (const double*)de, (const double*)dh, dom, dflag);
    BK_CHECK_LAUNCH();
    if (lev) {
      BK_HIP(hipMemcpyAsync(pin, dflag, sizeof(int), hipMemcpyDeviceToHost, st));
      BK_HIP(hipStreamSynchronize(st));
      int bad;
      std::memcpy(&bad, pin, sizeof(int));
      BK_REQUIRE(bad >= n, "vcov_robust: the leverage of row " + std::to_string(bad + 1) +
                               " is >= 1: HC2 / HC3 are not defined (use HC0 or HC1)");
    }
    BK_TRY(gram_weighted(ctx, n, k, d_Q, ldq, dom, dM, k));
  }

  // ---- S = diag(g) M diag(g); its eigenpairs; the rotation; the scale -------------------------------------------------
  {
    const int blocks = (int)std::min<int64_t>((k * k + 255) / 256, 2048);
    hipLaunchKernelGGL(sandwich_kernel, dim3(blocks), dim3(256), 0, st, (int)k, (const double*)dM, (const double*)dg,
                       dS);
    BK_CHECK_LAUNCH();
  }
  int64_t nv = 0;
  BK_TRY(eigen(ctx, dS, k, k, k, dth, k, -1.0, dU, k, &nv));
  BK_REQUIRE(nv == k, "vcov_robust: the eigensolver returned " + std::to_string(nv) + " of " + std::to_string(k) + " vectors");
  BK_TRY(gemm(ctx, 0, 0, n, k, k, 1.0, d_Q, ldq, dU, k, 0.0, d_Qout, ldqo));
  BK_HIP(hipStreamSynchronize(st));
  BK_TRY(pinned_get(ctx, k, &pin));
  BK_HIP(hipMemcpyAsync(pin, dth, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
  BK_HIP(hipStreamSynchronize(st));
  const double sd2 = y_sd * y_sd;
  for (int64_t j = 0; j < k; ++j) h_wout[j] = sd2 * scale * std::max(pin[j], 0.0);   // (theta < 0: rounding, or rank G < k)
  return BIGKRLS_OK;
}

}  // extern "C"
