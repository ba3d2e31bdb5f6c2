// bigkrls_shapley_effects(): exact interventional Shapley values of the fitted prediction, with standard errors; and
// its O(u n B) pass, shapley_weights (bigkrls_dev_shapley_weights).
//
// The columns are partitioned into M players. For an explained row x, a background row b and a training row i (all
// standardised with the TRAINING moments) player m has the factor
//   A_m = exp(-sum_{l in m} (x_l - X_il)^2 / sigma)  in a coalition,   B_m = exp(-sum_{l in m} (b_l - X_il)^2 / sigma)  outside,
// and the kernel entry of the hybrid row "x on the coalition's columns, b elsewhere" is the product of the chosen factors:
// a product game. Its Shapley weights |S|! (M-1-|S|)! / M! are the Beta integrals of t^|S| (1-t)^(M-1-|S|), so
//   phi_m(x; b, i) = (A_m - B_m) int_0^1 prod_{l != m} (B_l + t (A_l - B_l)) dt,
// a polynomial of degree M - 1 that Gauss-Legendre with G = ceil(M / 2) nodes integrates exactly, every term a product of
// numbers in [0, 1]: no alternating sums. With the mean over the B background rows
//   W[(r, m), i] = (1/B) sum_b (A_m - B_m) sum_g w_g prod_{l != m} (B_l + t_g (A_l - B_l)),      phi_m(x_r) = sd(y) W[(r, m), :] c,
// so everything is linear in the coefficients: Var phi_m(x_r) = f W[(r,m),:] vcov.est.c W[(r,m),:]' from either form of
// vcov.est.c (curve_tail, curvetail.h), f bigkrls_predict's factor. K is never needed.
//
// shapley_weights_kernel (buckets of up to 8 / 16 / 20 / 24 / 32 players): a thread owns one training row i and R explained
// rows; A (R x MB), the running weights (R x MB) and, per background row, B_m, A_m - B_m, the prefix products and the
// integrals stay in registers, every loop over the players fully unrolled over the bucket MB (players beyond M carry the
// neutral factors A = B = 1), so no register array is indexed at run time. The background rows go through LDS in chunks
// (shap_chunk_rows, shapplan.h), already in player order; B_m is computed once per (background row, training row) and
// serves the thread's R explained rows. The product without player m is prefix[m] * suffix, never a quotient: a factor
// may be exactly 0. shapley_weights_lds_kernel (buckets 64 / 128): the same loops over the M players with the four arrays
// in LDS ([m][thread], conflict-free), one explained row per thread.
// The sums over the background rows and the nodes run in a fixed order inside one thread: no atomics, no partials; a
// W entry depends on its explained row, its training row, the background and the player table only.
#include "hostprep.h"
#include "curvetail.h"
#include "expnp.h"
#include "shapplan.h"

#include <cstring>

namespace bk {
namespace {

// nodes, weights and the players' first positions in the column order: a kernel argument (no upload)
struct ShapTable {
  double t[SHAP_MAX_NODES], w[SHAP_MAX_NODES];
  int pstart[SHAP_MAX_PLAYERS + 1];
  int G, M;
};

// up to SHAP_INLINE ints per launch, as a kernel argument (the column order: no copy, no synchronisation)
constexpr int SHAP_INLINE = 512;
struct ShapInline {
  int v[SHAP_INLINE];
};
__global__ void shap_values_kernel(ShapInline t, int count, int* __restrict__ dst) {
  const int i = threadIdx.x;
  if (i < count) dst[i] = t.v[i];
}

// this chunk of background rows in player order: bgs[c * p + q] = Bg[c0 + c, perm[q]]
__device__ __forceinline__ void shap_stage_chunk(const double* __restrict__ Bg, int64_t ldb, const int* __restrict__ perm,
                                                 int p, int c0, int cn, double* bgs) {
  for (int e = threadIdx.x; e < cn * p; e += blockDim.x) {
    const int c = e / p, q = e - c * p;
    bgs[e] = Bg[(int64_t)(c0 + c) + (int64_t)perm[q] * ldb];
  }
}

// SINGLE: one column per player (M == p, the column order is the identity). The tile's 64 training rows then sit in LDS,
// xs[m * 64 + thread], and every factor is one unrolled expression: the loads of a background row's M factors issue
// together. Otherwise a player's columns are a run-time range of the column order, read from global memory (L1).
template <int MB, int R, bool SINGLE>
__global__ __launch_bounds__(64) void shapley_weights_kernel(const ShapTable tb, const int* __restrict__ perm,
                                                            const double* __restrict__ Z, int u, int64_t ldz,
                                                            const double* __restrict__ X, int n, int64_t ldx,
                                                            const double* __restrict__ Bg, int nb, int64_t ldb, int p,
                                                            int chunk, int tiles, double neg_inv_sigma, double inv_b,
                                                            double* __restrict__ W, int64_t ldw) {
  extern __shared__ __attribute__((aligned(16))) double shap_smem[];
  double* etab = shap_smem;                          // 32
  double* bgs = shap_smem + 32;                      // chunk x p
  double* xs = bgs + chunk * p + threadIdx.x;        // SINGLE: p x 64
  if (threadIdx.x < 32) etab[threadIdx.x] = kExp2Tab32[threadIdx.x];
  const int tile = (int)(blockIdx.x % (unsigned)tiles), rg = (int)(blockIdx.x / (unsigned)tiles);
  const int i = tile * 64 + (int)threadIdx.x;
  const bool live = i < n;
  const double* xi = X + (live ? i : n - 1);          // (idle lanes of the last tile repeat its last row; nothing stored)
  const int r0 = rg * R;
  const int M = tb.M, G = tb.G;
  if (SINGLE) {
#pragma unroll
    for (int m = 0; m < MB; ++m)
      if (m < M) xs[m * 64] = xi[(int64_t)m * ldx];
  }
  __syncthreads();

  double A[R][MB], acc[R][MB];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double* zr = Z + min(r0 + r, u - 1);
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      double a = 1.0;
      if (m < M) {
        double d = 0.0;
        if (SINGLE) {
          const double df = zr[(int64_t)m * ldz] - xs[m * 64];
          d = df * df;
        } else {
#pragma unroll 4
          for (int q = tb.pstart[m]; q < tb.pstart[m + 1]; ++q) {
            const int64_t c = perm[q];
            const double df = zr[c * ldz] - xi[c * ldx];
            d = fma(df, df, d);
          }
        }
        a = exp_nonpos_tab(d * neg_inv_sigma, etab);
      }
      A[r][m] = a;
      acc[r][m] = 0.0;
    }
  }

  for (int c0 = 0; c0 < nb; c0 += chunk) {
    const int cn = min(chunk, nb - c0);
    __syncthreads();
    shap_stage_chunk(Bg, ldb, perm, p, c0, cn, bgs);
    __syncthreads();
    for (int c = 0; c < cn; ++c) {
      const double* bc = bgs + c * p;
      double Bm[MB];
#pragma unroll
      for (int m = 0; m < MB; ++m) {
        double b = 1.0;
        if (m < M) {
          double d = 0.0;
          if (SINGLE) {
            const double df = bc[m] - xs[m * 64];
            d = df * df;
          } else {
#pragma unroll 4
            for (int q = tb.pstart[m]; q < tb.pstart[m + 1]; ++q) {
              const double df = bc[q] - xi[(int64_t)perm[q] * ldx];
              d = fma(df, df, d);
            }
          }
          b = exp_nonpos_tab(d * neg_inv_sigma, etab);
        }
        Bm[m] = b;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        double D[MB], I[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m) {
          D[m] = A[r][m] - Bm[m];
          I[m] = 0.0;
        }
        for (int g = 0; g < G; ++g) {
          const double t = tb.t[g];
          double pre[MB], run = 1.0;
#pragma unroll
          for (int m = 0; m < MB; ++m) {          // prefix products of the factors B_l + t (A_l - B_l)
            pre[m] = run;
            run *= fma(t, D[m], Bm[m]);
          }
          double suf = tb.w[g];                   // the node's weight rides on the suffix product
#pragma unroll
          for (int m = MB - 1; m >= 0; --m) {
            I[m] = fma(pre[m], suf, I[m]);
            suf *= fma(t, D[m], Bm[m]);
          }
        }
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[r][m] = fma(D[m], I[m], acc[r][m]);
      }
    }
  }

  if (!live) return;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r0 + r < u) {
      double* dst = W + (int64_t)(r0 + r) * M + (int64_t)i * ldw;
#pragma unroll
      for (int m = 0; m < MB; ++m)
        if (m < M) dst[m] = acc[r][m] * inv_b;
    }
  }
}

// the buckets above 32 players: A, B, the prefix products and the running weights in LDS, arr[m * T + thread]
__global__ __launch_bounds__(64) void shapley_weights_lds_kernel(const ShapTable tb, const int* __restrict__ perm,
                                                                const double* __restrict__ Z, int u, int64_t ldz,
                                                                const double* __restrict__ X, int n, int64_t ldx,
                                                                const double* __restrict__ Bg, int nb, int64_t ldb, int p,
                                                                int chunk, int tiles, double neg_inv_sigma, double inv_b,
                                                                double* __restrict__ W, int64_t ldw) {
  extern __shared__ __attribute__((aligned(16))) double shap_smem[];
  const int T = (int)blockDim.x, tid = (int)threadIdx.x;
  const int M = tb.M, G = tb.G;
  double* etab = shap_smem;
  double* bgs = shap_smem + 32;
  double* Aa = bgs + (int64_t)chunk * p + tid;
  double* Ba = Aa + M * T;
  double* Pa = Ba + M * T;
  double* Wa = Pa + M * T;
  if (tid < 32) etab[tid] = kExp2Tab32[tid];
  const int tile = (int)(blockIdx.x % (unsigned)tiles), r = (int)(blockIdx.x / (unsigned)tiles);   // r < u
  const int i = tile * T + tid;
  const bool live = i < n;
  const double* xi = X + (live ? i : n - 1);
  const double* zr = Z + r;
  __syncthreads();

  for (int m = 0; m < M; ++m) {
    double d = 0.0;
#pragma unroll 4
    for (int q = tb.pstart[m]; q < tb.pstart[m + 1]; ++q) {
      const int64_t c = perm[q];
      const double df = zr[c * ldz] - xi[c * ldx];
      d = fma(df, df, d);
    }
    Aa[m * T] = exp_nonpos_tab(d * neg_inv_sigma, etab);
    Wa[m * T] = 0.0;
  }
  for (int c0 = 0; c0 < nb; c0 += chunk) {
    const int cn = min(chunk, nb - c0);
    __syncthreads();
    shap_stage_chunk(Bg, ldb, perm, p, c0, cn, bgs);
    __syncthreads();
    for (int c = 0; c < cn; ++c) {
      const double* bc = bgs + c * p;
      for (int m = 0; m < M; ++m) {
        double d = 0.0;
#pragma unroll 4
        for (int q = tb.pstart[m]; q < tb.pstart[m + 1]; ++q) {
          const double df = bc[q] - xi[(int64_t)perm[q] * ldx];
          d = fma(df, df, d);
        }
        Ba[m * T] = exp_nonpos_tab(d * neg_inv_sigma, etab);
      }
      for (int g = 0; g < G; ++g) {
        const double t = tb.t[g];
        double run = 1.0;
        for (int m = 0; m < M; ++m) {
          const double b = Ba[m * T];
          Pa[m * T] = run;
          run *= fma(t, Aa[m * T] - b, b);
        }
        double suf = tb.w[g];
        for (int m = M - 1; m >= 0; --m) {
          const double b = Ba[m * T], dm = Aa[m * T] - b;
          Wa[m * T] = fma(dm * Pa[m * T], suf, Wa[m * T]);
          suf *= fma(t, dm, b);
        }
      }
    }
  }
  if (!live) return;
  double* dst = W + (int64_t)r * M + (int64_t)i * ldw;
  for (int m = 0; m < M; ++m) dst[m] = Wa[m * T] * inv_b;
}

template <int MB, int R>
int launch_registers(bigkrls_ctx* ctx, const ShapTable& tb, const int* perm, bool single, const double* Z, int64_t u,
                     int64_t ldz, const double* X, int64_t n, int64_t ldx, const double* Bg, int64_t B, int64_t ldb,
                     int64_t p, int64_t chunk, size_t lds, double sigma, double* W, int64_t ldw) {
  const int64_t tiles = (n + 63) / 64, groups = (u + R - 1) / R;
  BK_REQUIRE(tiles * groups < (1ll << 31), "shapley_weights: too many workgroups; explain fewer rows per call");
  auto kernel = single ? shapley_weights_kernel<MB, R, true> : shapley_weights_kernel<MB, R, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles * groups)), dim3(64), lds, ctx->stream, tb, perm, Z, (int)u, ldz, X,
                     (int)n, ldx, Bg, (int)B, ldb, (int)p, (int)chunk, (int)tiles, -1.0 / sigma, 1.0 / (double)B, W, ldw);
  BK_CHECK_LAUNCH();
  return BIGKRLS_OK;
}

}  // namespace

int shapley_weights(bigkrls_ctx* ctx, const double* Z, int64_t u, int64_t ldz, const double* X, int64_t n, int64_t ldx,
                    const double* Bg, int64_t B, int64_t ldb, int64_t p, double sigma, const int64_t* h_players,
                    int64_t M, double* W, int64_t ldw) {
  BK_REQUIRE(Z && X && Bg && W, "shapley_weights: null argument");
  BK_REQUIRE(B >= 1, "shapley_weights: B = " + std::to_string(B) + "; at least one background row is needed");
  BK_REQUIRE(u >= 1 && n >= 1 && p >= 1 && u < (1ll << 31) && n < (1ll << 31) && B < (1ll << 31),
             "shapley_weights: bad dimensions");
  BK_REQUIRE(sigma > 0.0 && std::isfinite(sigma), "shapley_weights: sigma must be a positive scalar");
  std::vector<int> pstart, perm;
  std::string err;
  BK_REQUIRE(shap_player_table(h_players, p, M, &pstart, &perm, &err), "shapley_weights: " + err);
  BK_REQUIRE(p <= shap_max_columns(), "shapley_weights: p = " + std::to_string(p) + " columns; at most " +
                                          std::to_string(shap_max_columns()) + " fit the background chunk in LDS");
  BK_REQUIRE(u * M < (1ll << 31), "shapley_weights: u M must stay below 2^31");
  BK_REQUIRE(ldz >= u && ldx >= n && ldb >= B && ldw >= u * M, "shapley_weights: a leading dimension is too small");

  ShapTable tb;
  std::memset(&tb, 0, sizeof(tb));
  tb.G = shap_nodes(M);
  tb.M = (int)M;
  shap_gauss_legendre(tb.G, tb.t, tb.w);
  std::memcpy(tb.pstart, pstart.data(), pstart.size() * sizeof(int));

  void* pt = nullptr;
  BK_TRY(ws_get(ctx, SLOT_SHAP_TABLE, (p + SHAP_INLINE) * (int64_t)sizeof(int), &pt));
  int* dperm = (int*)pt;
  for (int64_t q0 = 0; q0 < p; q0 += SHAP_INLINE) {
    ShapInline t;
    const int64_t cnt = std::min<int64_t>(SHAP_INLINE, p - q0);
    std::memcpy(t.v, perm.data() + q0, (size_t)cnt * sizeof(int));
    hipLaunchKernelGGL(shap_values_kernel, dim3(1), dim3(SHAP_INLINE), 0, ctx->stream, t, (int)cnt, dperm + q0);
    BK_CHECK_LAUNCH();
  }

  const ShapShape sh = shap_shape(M);
  const int64_t chunk = shap_chunk_rows(B, p);
  bool single = !sh.in_lds && M == p;                  // one column per player, and player m is column m
  for (int64_t q = 0; single && q < p; ++q) single = perm[(size_t)q] == q;
  const size_t lds = (size_t)shap_lds_bytes(sh, M, chunk, p);
  // the operation count the measurements are quoted against: 4 M G fused multiply-adds per (explained, training,
  // background) triple, 2 flops each
  if (ctx->profile)
    BK_TRY(prof_begin(ctx, "shapley_weights", 8.0 * (double)M * (double)tb.G * (double)u * (double)n * (double)B));
  switch (sh.bucket) {
    case 8:
      BK_TRY((launch_registers<8, 6>(ctx, tb, dperm, single, Z, u, ldz, X, n, ldx, Bg, B, ldb, p, chunk, lds, sigma, W, ldw)));
      break;
    case 16:
      BK_TRY((launch_registers<16, 3>(ctx, tb, dperm, single, Z, u, ldz, X, n, ldx, Bg, B, ldb, p, chunk, lds, sigma, W, ldw)));
      break;
    case 20:
      BK_TRY((launch_registers<20, 2>(ctx, tb, dperm, single, Z, u, ldz, X, n, ldx, Bg, B, ldb, p, chunk, lds, sigma, W, ldw)));
      break;
    case 24:
      BK_TRY((launch_registers<24, 1>(ctx, tb, dperm, single, Z, u, ldz, X, n, ldx, Bg, B, ldb, p, chunk, lds, sigma, W, ldw)));
      break;
    case 32:
      BK_TRY((launch_registers<32, 1>(ctx, tb, dperm, single, Z, u, ldz, X, n, ldx, Bg, B, ldb, p, chunk, lds, sigma, W, ldw)));
      break;
    default: {
      const int64_t tiles = (n + sh.threads - 1) / sh.threads;
      BK_REQUIRE(tiles * u < (1ll << 31), "shapley_weights: too many workgroups; explain fewer rows per call");
      BK_TRY(ensure_dyn_smem(ctx, (const void*)shapley_weights_lds_kernel, lds));
      hipLaunchKernelGGL(shapley_weights_lds_kernel, dim3((unsigned)(tiles * u)), dim3((unsigned)sh.threads), lds,
                         ctx->stream, tb, (const int*)dperm, Z, (int)u, ldz, X, (int)n, ldx, Bg, (int)B, ldb, (int)p,
                         (int)chunk, (int)tiles, -1.0 / sigma, 1.0 / (double)B, W, ldw);
      BK_CHECK_LAUNCH();
    }
  }
  if (ctx->profile) BK_TRY(prof_end(ctx, "shapley_weights"));
  return BIGKRLS_OK;
}

}  // namespace bk

using namespace bk;

extern "C" {

// packed operands (include/bigkrls.h); the whole-path entry below reaches shapley_weights with a row block of Z
int bigkrls_dev_shapley_weights(bigkrls_ctx* ctx, const double* Z, int64_t u, const double* X, int64_t n, const double* Bg,
                                int64_t B, int64_t p, double sigma, const int64_t* h_players, int64_t M, double* W) {
  BK_TRY(check_ctx(ctx));
  return shapley_weights(ctx, Z, u, u, X, n, n, Bg, B, B, p, sigma, h_players, M, W, u * M);
}

int bigkrls_shapley_effects(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y,
                            const double* h_coeffs, double sigma, const int64_t* h_players, int64_t M,
                            const double* h_newdata, int64_t u, const double* h_background, int64_t B,
                            const double* d_vcov_c, const double* d_Q, int64_t ldq, int64_t k, const double* h_w,
                            double neffective, int64_t block_rows, double* h_phi, double* h_se, double* h_baseline) {
  const std::string who = "shapley_effects: ";
  CurveArgs ca;
  BK_TRY(curve_check_args(ctx, "shapley_effects", h_X && h_y && h_coeffs && h_background && h_phi && h_baseline, n, p,
                          h_newdata, &u, sigma, d_vcov_c, d_Q, ldq, k, h_w, h_se, nullptr, &ca));
  BK_REQUIRE(B >= 1, who + "B = " + std::to_string(B) + "; at least one background row is needed");
  BK_REQUIRE(B < (1ll << 31), who + "bad dimensions");
  BK_REQUIRE(block_rows >= 0, who + "block_rows must not be negative");
  std::vector<int> pstart, perm;
  std::string err;
  BK_REQUIRE(shap_player_table(h_players, p, M, &pstart, &perm, &err), who + err);
  BK_REQUIRE(p <= shap_max_columns(), who + "p = " + std::to_string(p) + " columns; at most " +
                                          std::to_string(shap_max_columns()) + " fit the background chunk in LDS");
  if (h_newdata)
    for (int64_t i = 0; i < u * p; ++i)
      BK_REQUIRE(std::isfinite(h_newdata[i]), who + "newdata contains missing or infinite values");
  for (int64_t i = 0; i < B * p; ++i)
    BK_REQUIRE(std::isfinite(h_background[i]), who + "background contains missing or infinite values");
  BK_REQUIRE(u * M < (1ll << 31), who + "u M must stay below 2^31");

  // ---- the training moments (as bigkrls_marginal_effects) ----------------------------------------------------
  std::vector<double> x_mean((size_t)p), x_sd((size_t)p);
  for (int64_t j = 0; j < p; ++j) {
    mean_sd(h_X + j * n, n, &x_mean[j], &x_sd[j]);
    BK_REQUIRE(x_sd[j] > 0.0, who + "training column " + std::to_string(j + 1) + " is constant");
  }
  double y_mean, y_sd;
  mean_sd(h_y, n, &y_mean, &y_sd);
  BK_REQUIRE(y_sd > 0.0, who + "y is a constant");

  // ---- layout: one slot; behind the vectors one row block of W and, from the factors, of W Q -----------------
  const int64_t kq = ca.kq, b = shap_block_rows(u, n, M, block_rows);
  Layout L;
  const Region Xs = L.up(n * p), Zs = h_newdata ? L.up(u * p) : Xs, Bs = L.up(B * p), c = L.up(n), w = L.up(kq);
  const Region phi = L.down(u * M), var = L.down(ca.want_var ? u * M : 0), kb = L.down(B);
  const Region Wb = L.dev(b * M * n), Pb = L.dev(b * M * kq);
  BK_TRY(layout_device(ctx, SLOT_SHAP_SMALL, &L));
  double* dW = L.d(Wb);
  double* dP = L.d(Pb);

  BK_TRY(layout_pinned(ctx, &L));
  for (int64_t j = 0; j < p; ++j) {
    standardise_column(h_X + j * n, n, x_mean[j], x_sd[j], L.h(Xs) + j * n);
    if (h_newdata) standardise_column(h_newdata + j * u, u, x_mean[j], x_sd[j], L.h(Zs) + j * u);
    standardise_column(h_background + j * B, B, x_mean[j], x_sd[j], L.h(Bs) + j * B);
  }
  std::memcpy(L.h(c), h_coeffs, (size_t)n * sizeof(double));
  if (kq > 0) std::memcpy(L.h(w), ca.vc.h_w, (size_t)kq * sizeof(double));
  BK_TRY(layout_upload(ctx, L));

  // ---- the fits at the background rows (the baseline), then block by block: W, W c and diag(W Vc W') ----------
  BK_TRY(kernel_contract(ctx, L.d(Bs), B, B, L.d(Xs), n, n, p, sigma, L.d(c), 1, n, 0, L.d(kb), B));
  for (int64_t r0 = 0; r0 < u; r0 += b) {
    const int64_t rows = std::min(b, u - r0), G = rows * M;
    BK_TRY(shapley_weights(ctx, L.d(Zs) + r0, rows, u, L.d(Xs), n, n, L.d(Bs), B, B, p, sigma, h_players, M, dW, G));
    BK_TRY(curve_tail(ctx, ca.vc, ca.want_var, G, n, kq, dW, dP, L.d(c), L.d(w), L.d(phi) + r0 * M, L.d(var) + r0 * M,
                      nullptr));
  }
  BK_TRY(layout_download(ctx, L));

  // ---- original units; bigkrls_predict's factor on the variance (as bigkrls_partial_dependence) ----------------
  const double* pin = L.pinned();
  const int64_t T = u * M, voff = ca.want_var ? T : 0;
  const double f = neffective > 0.0 ? std::sqrt((double)n / neffective) : 1.0;
  for (int64_t i = 0; i < T; ++i) h_phi[i] = pin[i] * y_sd;
  if (h_se)
    for (int64_t i = 0; i < T; ++i) h_se[i] = std::sqrt(std::max(f * pin[T + i], 0.0));
  long double s = 0.0L;
  for (int64_t i = 0; i < B; ++i) s += pin[T + voff + i];
  *h_baseline = y_mean + y_sd * (double)(s / (long double)B);
  return BIGKRLS_OK;
}

}  // extern "C"
