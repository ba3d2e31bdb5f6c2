// Case- and cluster-deletion diagnostics (no counterpart in the reference): which observations, or which clusters, does
// the result rest on -- without one refit per unit.
//
// Standardised units. Q (n x k) and d are the kept eigenpairs, lambda the fit's ridge parameter, g = 1 / (d + lambda),
// w = d g, H = Q diag(w) Q' the smoother (yfitted.std = H ys), e = ys - H ys, Ginv = Q diag(g) Q'. With k < N the fit is
// the penalised least-squares estimator on the fixed basis Q. Deleting the rows S of one unit (one observation, or one
// cluster) with the basis, sigma, lambda and the standardisation HELD AT THEIR FULL-SAMPLE VALUES gives in closed form
//   et_S            = (I - H_SS)^-1 e_S                 deletion residuals: ys_S minus the prediction of the fit without S
//   c - c(-S)       = Q diag(g) (Q_S' et_S)
//   yhat - yhat(-S) = Q diag(w) (Q_S' et_S),            ||yhat - yhat(-S)||^2 = sum_m (w_m s_m)^2,  s = Q_S' et_S
// and for a single row et_i = e_i / (1 - h_i), h_i = sum_m Q_im^2 w_m.
//
// deletion_residuals: the batched solve of the small SPD systems (I - H_SS) x = e_S, one per unit (plan: csrc/delplan.h).
//   one row      no system: one vector kernel on the leverages (rowsumsq_weighted) for all of them
//   2 .. 256     del_fused_kernel, one workgroup per unit, four instances (m <= 16 on one wave; m <= 64 and m <= 128 on four
//                waves; m <= 256 on eight waves, with I - H_SS in the workspace -- L2 -- instead of LDS): the
//                unit's rows of Q are gathered through the index list into LDS chunk by chunk of 16 columns, once plain
//                and once scaled by w; the lower 16 x 16 tiles of H_SS are accumulated in registers by the f64 MFMA; then
//                I - H_SS is stored to LDS (the staging buffer aliases that region; the wide instance stores it to its 514 KiB
//                of workspace), factorised in place by a right-looking
//                Cholesky in column blocks of 16 (diagonal block in one wave's registers, panel solve one row per thread,
//                trailing update by the MFMA again; three barriers per block), and one wave does both triangular solves
//                on e_S and writes et_S. Fixed summation order, no atomics in the arithmetic: two calls give the same bits.
//                A pivot that is not positive means a block leverage of 1 or more: the first such unit is recorded by an
//                atomicMin on (unit, column) and nothing is written for it.
//   larger       (or every unit of two rows or more with route = 1) the general route from the library's own entries:
//                gather Q_S, H_SS = (Q_S diag(w)) Q_S' by gemm, A = I - H_SS, its m eigenpairs by eigen(), et_S = V
//                diag(1 / theta) V' e_S by gemv. One unit after the other; 8 m^2 <= 2^30 bytes. For m > k the Woodbury form
//                (a k x k system) would be cheaper; it is not built.
//
// bigkrls_influence: leverages, deletion residuals and fits, Cook's distances, the change of every AME when a unit is
// deleted (dfame) and its jackknife variance, the leave-one-out R2 -- argument checks, standardisation and the AMEs'
// column side through hostprep.h / margeff.h as the other post-estimation entries.
#include "margeff.h"
#include "delplan.h"

#include <cstring>

namespace bk {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int DF_KC = 16;            // columns of Q per staged chunk: four MFMA k-steps
constexpr int DF_LDS = DF_KC + 1;    // leading dimension of the staged rows (odd: the 16 rows of a tile hit 16 banks)
constexpr unsigned long long DEL_NO_BAD = ~0ull;

// LDS of one workgroup: I - H_SS (MB x (MB + 1)) with the staging buffer inside it, or -- WIDE, the matrix in the
// workspace -- the staging buffer alone
template <int MB, bool WIDE>
constexpr size_t del_fused_lds_bytes() {
  return sizeof(double) * (size_t)(!WIDE && MB * (MB + 1) > 2 * MB * DF_LDS ? MB * (MB + 1) : 2 * MB * DF_LDS);
}

// tile t of the lower triangle enumerated row by row: (0,0), (1,0), (1,1), (2,0), ...
__device__ __forceinline__ void lower_tile(int t, int* ti, int* tj) {
  int a = 0;
  while ((a + 1) * (a + 2) / 2 <= t) ++a;
  *ti = a;
  *tj = t - a * (a + 1) / 2;
}

// One workgroup per unit of at most MB rows (see the head of the file). rows: the sorted rows' original indices; units:
// this class's list; bad: min over the failing units of (unit << 32 | pivot column). WIDE: I - H_SS lives in gws, MB (MB + 1)
// doubles per workgroup of the launch (it stays in L2; a workgroup's waves share one L1, and __syncthreads orders their
// global accesses), and the staging buffer has the LDS to itself. In both regimes the rows of the last 16-row tile beyond m
// are never written: the trailing update's MFMA reads them as they are (stale LDS, uninitialised workspace), an output
// depends on its own two rows only, and the outputs of those rows are not stored.
template <int MB, int NT, bool WIDE>
__global__ __launch_bounds__(NT) void del_fused_kernel(int k, const double* __restrict__ Q, int64_t ldq,
                                                       const double* __restrict__ w, const double* __restrict__ e,
                                                       const int* __restrict__ rows, const DelUnit* __restrict__ units,
                                                       double* __restrict__ et, unsigned long long* __restrict__ bad,
                                                       double* gws) {   // (no __restrict__: other waves write what this one reads)
  extern __shared__ double sm[];
  __shared__ int s_bad;
  constexpr int LDA = MB + 1;
  constexpr int NTILE = MB / 16, NW = NT / 64;
  constexpr int NLOW = NTILE * (NTILE + 1) / 2, TPW = (NLOW + NW - 1) / NW;
  constexpr int CSTEP = NT / MB;
  static_assert(NT % MB == 0 && MB % 16 == 0 && NT % 64 == 0, "del_fused_kernel: shape");
  // I - H_SS, row i at i LDA (lower triangle)
  double* As = WIDE ? gws + (size_t)blockIdx.x * (size_t)(MB * LDA) : sm;
  double* Qs = sm;                   // staged rows of Q_S (aliases As in LDS: the tiles live in registers until the k loop ends)
  double* Qw = sm + MB * DF_LDS;     // ... scaled by w

  const DelUnit un = units[blockIdx.x];
  const int m = un.m, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lm = lane & 15, lk = lane >> 4;
  if (tid == 0) s_bad = -1;

  // ---- H_SS: lower tiles in registers ------------------------------------------------------------------------------
  const int gi = tid % MB, gc0 = tid / MB;
  const int64_t grow = gi < m ? (int64_t)rows[un.first + gi] : -1;
  int ti[TPW], tj[TPW];
  bool on[TPW];
  d4 acc[TPW];
#pragma unroll
  for (int s = 0; s < TPW; ++s) {
    const int t = wave + NW * s;
    lower_tile(t < NLOW ? t : 0, &ti[s], &tj[s]);
    on[s] = t < NLOW && 16 * ti[s] < m;          // (uniform over the wave)
    acc[s] = (d4){0.0, 0.0, 0.0, 0.0};
  }
  for (int c0 = 0; c0 < k; c0 += DF_KC) {
    __syncthreads();                             // the previous chunk has been read
    for (int cc = gc0; cc < DF_KC; cc += CSTEP) {
      const int c = c0 + cc;
      double q = 0.0, wc = 0.0;
      if (grow >= 0 && c < k) {
        q = Q[grow + (int64_t)c * ldq];
        wc = w[c];
      }
      Qs[gi * DF_LDS + cc] = q;
      Qw[gi * DF_LDS + cc] = q * wc;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < TPW; ++s) {
      if (!on[s]) continue;
#pragma unroll
      for (int kk = 0; kk < DF_KC; kk += 4) {
        const double x = Qw[(16 * ti[s] + lm) * DF_LDS + kk + lk];
        const double y = Qs[(16 * tj[s] + lm) * DF_LDS + kk + lk];
        acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc[s], 0, 0, 0);
      }
    }
  }
  __syncthreads();                               // the staging buffer is dead: As takes its place
  // acc[s][r] = H[16 ti + lk + 4 r][16 tj + lm]
#pragma unroll
  for (int s = 0; s < TPW; ++s) {
    if (!on[s]) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * ti[s] + lk + 4 * r, j = 16 * tj[s] + lm;
      if (i < m && j <= i) As[i * LDA + j] = (i == j ? 1.0 : 0.0) - acc[s][r];
    }
  }
  __syncthreads();

  // ---- Cholesky in place, right-looking, column blocks of 16 ---------------------------------------------------------
  const int nt = (m + 15) / 16;
  for (int p = 0; p < nt; ++p) {
    const int j0 = 16 * p, jb = min(16, m - j0);
    if (wave == 0) {
      // the diagonal block in registers: lane l < jb holds row j0 + l, every other lane a row of the identity
      double row[16];
      const bool act = lane < jb;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        row[c] = (act && c <= lane) ? As[(j0 + lane) * LDA + j0 + c] : (c == lane ? 1.0 : 0.0);
      int badc = -1;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double piv = __shfl(row[j], j);
        if (!(piv > 0.0) && badc < 0) badc = j;  // (uniform: every lane sees lane j's value)
        const double dj = sqrt(piv);
        row[j] = lane == j ? dj : row[j] / dj;
#pragma unroll
        for (int c = j + 1; c < 16; ++c) {
          const double lc = __shfl(row[j], c);   // L[c][j]
          if (lane >= c) row[c] = fma(-row[j], lc, row[c]);
        }
      }
      if (badc >= 0) {
        if (lane == 0) s_bad = j0 + badc;
      } else if (act) {
#pragma unroll
        for (int c = 0; c < 16; ++c)
          if (c <= lane) As[(j0 + lane) * LDA + j0 + c] = row[c];
      }
    }
    __syncthreads();
    if (s_bad >= 0) break;                       // (uniform: read after the barrier, never written again)
    // the panel below: row i of L21 = A21 L11^-T, one row per thread
    for (int i = j0 + 16 + tid; i < m; i += NT) {
      double x[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) x[c] = As[i * LDA + j0 + c];
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        double s = x[c];
#pragma unroll
        for (int t = 0; t < c; ++t) s = fma(-x[t], As[(j0 + c) * LDA + j0 + t], s);
        x[c] = s / As[(j0 + c) * LDA + j0 + c];
      }
#pragma unroll
      for (int c = 0; c < 16; ++c) As[i * LDA + j0 + c] = x[c];
    }
    __syncthreads();
    // the trailing update A22 -= L21 L21': the lower tiles (a, b), p < b <= a < nt, over the waves. The rows of the last
    // tile beyond m are whatever the region held: an entry depends on its own two rows only and those entries are not stored.
    const int rem = nt - p - 1, count = rem * (rem + 1) / 2;
    for (int t = wave; t < count; t += NW) {
      int a, b;
      lower_tile(t, &a, &b);
      a += p + 1;
      b += p + 1;
      d4 c4 = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < 16; kk += 4) {
        const double x = As[(16 * a + lm) * LDA + j0 + kk + lk];
        const double y = As[(16 * b + lm) * LDA + j0 + kk + lk];
        c4 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, c4, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * a + lk + 4 * r, j = 16 * b + lm;
        if (i < m && j <= i) As[i * LDA + j] -= c4[r];
      }
    }
    __syncthreads();
  }
  if (s_bad >= 0) {
    if (tid == 0) atomicMin(bad, ((unsigned long long)(unsigned)un.unit << 32) | (unsigned)s_bad);
    return;
  }

  // ---- L y = e_S, L' x = y: one wave, lane l holds the entries l, l + 64, ... --------------------------------------------
  if (wave == 0) {
    constexpr int EPL = (MB + 63) / 64;
    double y[EPL];
#pragma unroll
    for (int q = 0; q < EPL; ++q) {
      const int i = lane + 64 * q;
      y[q] = i < m ? e[rows[un.first + i]] : 0.0;
    }
    for (int j = 0; j < m; ++j) {
      double src = y[0];
#pragma unroll
      for (int q = 1; q < EPL; ++q)
        if ((j >> 6) == q) src = y[q];
      const double yj = __shfl(src, j & 63) / As[j * LDA + j];
#pragma unroll
      for (int q = 0; q < EPL; ++q) {
        const int i = lane + 64 * q;
        if (i == j) y[q] = yj;
        else if (i > j && i < m) y[q] = fma(-As[i * LDA + j], yj, y[q]);
      }
    }
    for (int j = m - 1; j >= 0; --j) {
      double src = y[0];
#pragma unroll
      for (int q = 1; q < EPL; ++q)
        if ((j >> 6) == q) src = y[q];
      const double xj = __shfl(src, j & 63) / As[j * LDA + j];
#pragma unroll
      for (int q = 0; q < EPL; ++q) {
        const int i = lane + 64 * q;
        if (i == j) y[q] = xj;
        else if (i < j) y[q] = fma(-As[j * LDA + i], xj, y[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < EPL; ++q) {
      const int i = lane + 64 * q;
      if (i < m) et[rows[un.first + i]] = y[q];
    }
  }
}

// the units of one row: et = e / (1 - h). units == nullptr: every row is its own unit (count = n).
__global__ void del_single_kernel(int count, const int* __restrict__ rows, const DelUnit* __restrict__ units,
                                  const double* __restrict__ e, const double* __restrict__ h, double* __restrict__ et,
                                  unsigned long long* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int r = units ? rows[units[i].first] : i;
  const unsigned unit = units ? (unsigned)units[i].unit : (unsigned)i;
  const double hi = h[r];
  if (!(hi < 1.0)) {
    atomicMin(bad, (unsigned long long)unit << 32);
    return;
  }
  et[r] = e[r] / (1.0 - hi);
}

// ---- the general route's small kernels -----------------------------------------------------------------------------------
// Qg (m x k, ld m) = the unit's rows of Q; eg (m) = its entries of e
__global__ void del_gather_kernel(int m, int k, const double* __restrict__ Q, int64_t ldq, const double* __restrict__ e,
                                  const int* __restrict__ rows, double* __restrict__ Qg, double* __restrict__ eg) {
  const int64_t total = (int64_t)m * k;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t x = t0; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(x % m);
    Qg[x] = Q[rows[i] + (x / m) * ldq];
  }
  for (int64_t i = t0; i < m; i += (int64_t)gridDim.x * blockDim.x) eg[i] = e[rows[i]];
}

// A (m x m) = the identity
__global__ void del_identity_kernel(int m, double* __restrict__ A) {
  const int64_t total = (int64_t)m * m;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x)
    A[x] = (x % m) == (x / m) ? 1.0 : 0.0;
}

// A (m x m) symmetrised: both triangles take the mean, the same bits at (i, j) and (j, i)
__global__ void del_symmetrise_kernel(int m, double* __restrict__ A) {
  const int64_t total = (int64_t)m * m;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(x % m), j = (int)(x / m);
    if (i <= j) continue;
    const double v = 0.5 * (A[i + (int64_t)j * m] + A[j + (int64_t)i * m]);
    A[i + (int64_t)j * m] = v;
    A[j + (int64_t)i * m] = v;
  }
}

__global__ void del_divide_kernel(int m, const double* __restrict__ theta, double* __restrict__ z) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) z[i] = z[i] / theta[i];
}

__global__ void del_scatter_kernel(int m, const double* __restrict__ x, const int* __restrict__ rows,
                                   double* __restrict__ et) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) et[rows[i]] = x[i];
}

std::string del_unit_text(int64_t unit, int64_t m) {
  return "unit " + std::to_string(unit) + " (" + std::to_string(m) + (m == 1 ? " row)" : " rows)");
}

// gws: the wide instance's workspace (MB (MB + 1) doubles per unit of a launch, at most DEL_WIDE_BATCH units per launch)
template <int MB, int NT, bool WIDE = false>
int launch_fused(bigkrls_ctx* ctx, int64_t count, int64_t k, const double* Q, int64_t ldq, const double* w,
                 const double* e, const int* rows, const DelUnit* units, double* et, unsigned long long* bad,
                 double* gws = nullptr) {
  if (count == 0) return BIGKRLS_OK;
  constexpr size_t lds = del_fused_lds_bytes<MB, WIDE>();
  if (lds > 48 * 1024) BK_TRY(ensure_dyn_smem(ctx, (const void*)del_fused_kernel<MB, NT, WIDE>, lds));
  const int64_t batch = WIDE ? DEL_WIDE_BATCH : count;
  for (int64_t b0 = 0; b0 < count; b0 += batch) {     // (launches on one stream: a batch reuses the workspace of the one before)
    hipLaunchKernelGGL((del_fused_kernel<MB, NT, WIDE>), dim3((unsigned)std::min(batch, count - b0)), dim3(NT), lds,
                       ctx->stream, (int)k, Q, ldq, w, e, rows, units + b0, et, bad, gws);
    BK_CHECK_LAUNCH();
  }
  return BIGKRLS_OK;
}

// one unit through the eigensolver (see the head of the file); ws: the general route's workspace
int general_unit(bigkrls_ctx* ctx, const DelUnit& un, int64_t k, const double* Q, int64_t ldq, const double* w,
                 const double* e, const int* rows, double* ws, double* et) {
  hipStream_t st = ctx->stream;
  const int64_t m = un.m;
  double* Qg = ws;
  double* T = Qg + m * k;
  double* A = T + m * k;
  double* V = A + m * m;
  double* theta = V + m * m;
  double* eg = theta + m;
  double* z = eg + m;
  double* x = z + m;
  hipLaunchKernelGGL(del_gather_kernel, dim3(launch_blocks(m * k, 4096)), dim3(256), 0, st, (int)m, (int)k, Q, ldq, e,
                     rows + un.first, Qg, eg);
  BK_CHECK_LAUNCH();
  hipLaunchKernelGGL(del_identity_kernel, dim3(launch_blocks(m * m, 4096)), dim3(256), 0, st, (int)m, A);
  BK_CHECK_LAUNCH();
  BK_TRY(multdiag(ctx, Qg, m, k, m, w, T, m));
  BK_TRY(gemm(ctx, 0, 1, m, m, k, -1.0, T, m, Qg, m, 1.0, A, m));           // A = I - (Q_S diag(w)) Q_S'
  hipLaunchKernelGGL(del_symmetrise_kernel, dim3(launch_blocks(m * m, 4096)), dim3(256), 0, st, (int)m, A);
  BK_CHECK_LAUNCH();
  int64_t nv = 0;
  BK_TRY(eigen(ctx, A, m, m, m, theta, m, -1.0, V, m, &nv));
  BK_REQUIRE(nv == m, "deletion_residuals: the eigensolver returned " + std::to_string(nv) + " of " + std::to_string(m) +
                          " vectors for " + del_unit_text(un.unit, m));
  double tmin = 0.0;
  {
    PinnedFetch pf(ctx, 8);
    BK_TRY(pf.add(&tmin, theta + (m - 1), sizeof(double)));                   // (descending: the last is the smallest)
    BK_TRY(pf.finish());
  }
  BK_REQUIRE(tmin > 0.0, "deletion_residuals: " + del_unit_text(un.unit, m) + ": the smallest eigenvalue of I - H_SS is " +
                             std::to_string(tmin) + ", not positive: a block leverage of 1 or more");
  BK_TRY(gemv(ctx, 1, m, m, 1.0, V, m, eg, 0.0, z));                          // z = V' e_S
  hipLaunchKernelGGL(del_divide_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, (int)m, (const double*)theta, z);
  BK_CHECK_LAUNCH();
  BK_TRY(gemv(ctx, 0, m, m, 1.0, V, m, z, 0.0, x));                           // x = V diag(1 / theta) V' e_S
  hipLaunchKernelGGL(del_scatter_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, (int)m, (const double*)x,
                     rows + un.first, et);
  BK_CHECK_LAUNCH();
  return BIGKRLS_OK;
}

// out[u] = sum_m (w_m S[m, u])^2, S k x U (lds): one wave per unit, fixed order
__global__ __launch_bounds__(64) void cook_numerator_kernel(int k, const double* __restrict__ S, int64_t lds,
                                                            const double* __restrict__ w, double* __restrict__ out) {
  const double* s = S + (int64_t)blockIdx.x * lds;
  double a = 0.0;
  for (int m = threadIdx.x; m < k; m += 64) {
    const double v = w[m] * s[m];
    a = fma(v, v, a);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
  if (threadIdx.x == 0) out[blockIdx.x] = a;
}

// T (k x nj) <- diag(g) T
__global__ void scale_rows_kernel(int k, int nj, const double* __restrict__ g, double* __restrict__ T) {
  const int64_t total = (int64_t)k * nj;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x)
    T[x] *= g[x % k];
}

}  // namespace

// d_et[S] = (I - H_SS)^-1 e[S] for every unit, H = Q diag(w) Q'; w, e on the device, the labels on the host (nullptr:
// every row its own unit). d_hat (n, may be null): the leverages; d_S (k x G, lds; may be null): the scores Q_S' et_S.
int deletion_residuals(bigkrls_ctx* ctx, int64_t n, int64_t k, const double* d_Q, int64_t ldq, const double* d_w,
                       const double* d_e, const int64_t* h_unit, int64_t G, int route, double* d_et, double* d_hat,
                       double* d_S, int64_t lds) {
  BK_REQUIRE(n >= 1 && k >= 1 && n < (1ll << 31) && k < (1ll << 31), "deletion_residuals: bad dimensions");
  BK_REQUIRE(d_Q && d_w && d_e && d_et, "deletion_residuals: null argument");
  BK_REQUIRE(ldq >= n, "deletion_residuals: leading dimension of Q too small");
  BK_REQUIRE(route == 0 || route == 1, "deletion_residuals: route must be 0 (by size) or 1 (the general route)");
  if (!h_unit) G = n;
  BK_REQUIRE(G >= 1 && G < (1ll << 31), "deletion_residuals: G must be at least 1");
  BK_REQUIRE(!d_S || lds >= k, "deletion_residuals: leading dimension of the scores too small");
  hipStream_t st = ctx->stream;

  // ---- the plan, before anything is allocated ---------------------------------------------------------------------
  DelPlan pl;
  if (h_unit) {
    pl = plan_deletion(h_unit, n, G, k, route);
    BK_REQUIRE(pl.bad < 0, "deletion_residuals: the label of row " + std::to_string(pl.bad + 1) + " is outside [0, G)");
    BK_REQUIRE(pl.over_unit < 0, "deletion_residuals: " + del_unit_text(pl.over_unit, pl.over_m) +
                                     ": the general route holds the unit's m x m matrix, 8 m^2 bytes, at most 2^30 (m <= " +
                                     std::to_string(del_cap_rows()) + ")");
  }
  const bool singles = !h_unit || !pl.list[DEL_SINGLE].empty();

  // ---- device: the index lists, the flag word, the leverages -------------------------------------------------------------
  const int64_t b_idx = h_unit ? pl.index_bytes : 0;
  const int64_t b_all = b_idx + 8 + ((!d_hat && singles) ? n * 8 : 0);
  void* pidx = nullptr;
  BK_TRY(ws_get(ctx, SLOT_DEL_INDEX, b_all + 64, &pidx));
  char* dbase = (char*)pidx;
  const int* d_rows = (const int*)dbase;
  unsigned long long* d_bad = (unsigned long long*)(dbase + b_idx);
  double* hat = d_hat ? d_hat : (double*)(dbase + b_idx + 8);
  if (b_idx > 0) {
    double* pin = nullptr;
    BK_HIP(hipStreamSynchronize(st));   // (the pinned buffer may be in use or reallocated)
    BK_TRY(pinned_get(ctx, b_idx / 8 + 8, &pin));
    char* hb = (char*)pin;
    std::memcpy(hb, pl.rows.data(), (size_t)n * 4);
    for (int c = 0; c < DEL_CLASSES; ++c)
      if (!pl.list[c].empty())
        std::memcpy(hb + pl.list_off[c], pl.list[c].data(), pl.list[c].size() * sizeof(DelUnit));
    BK_HIP(hipMemcpyAsync(dbase, hb, (size_t)b_idx, hipMemcpyHostToDevice, st));
  }
  BK_HIP(hipMemsetAsync(d_bad, 0xff, 8, st));
  auto units_of = [&](int c) { return (const DelUnit*)(dbase + pl.list_off[c]); };

  const double sum_m2 = h_unit ? pl.sum_m2 : (double)n;
  BK_TRY(prof_begin(ctx, "deletion_residuals", 2.0 * (double)k * sum_m2));
  int rc = BIGKRLS_OK;
  unsigned long long bad = DEL_NO_BAD;     // the lowest failing unit of the kernels' classes: unit << 32 | pivot column
  auto fetch_bad = [&]() -> int {
    PinnedFetch pf(ctx, 8);
    BK_TRY(pf.add(&bad, d_bad, 8));
    return pf.finish();
  };
  auto run = [&]() -> int {
    if (d_hat || singles) BK_TRY(rowsumsq_weighted(ctx, n, k, d_Q, ldq, d_w, hat));       // h_i = sum_m Q_im^2 w_m
    if (!h_unit) {
      hipLaunchKernelGGL(del_single_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (int)n, (const int*)nullptr,
                         (const DelUnit*)nullptr, d_e, (const double*)hat, d_et, d_bad);
      BK_CHECK_LAUNCH();
      return fetch_bad();
    }
    const int64_t n1 = (int64_t)pl.list[DEL_SINGLE].size();
    if (n1 > 0) {
      hipLaunchKernelGGL(del_single_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, (int)n1, d_rows,
                         units_of(DEL_SINGLE), d_e, (const double*)hat, d_et, d_bad);
      BK_CHECK_LAUNCH();
    }
    BK_TRY((launch_fused<16, 64>(ctx, (int64_t)pl.list[DEL_WAVE].size(), k, d_Q, ldq, d_w, d_e, d_rows, units_of(DEL_WAVE),
                                 d_et, d_bad)));
    BK_TRY((launch_fused<64, 256>(ctx, (int64_t)pl.list[DEL_MID].size(), k, d_Q, ldq, d_w, d_e, d_rows, units_of(DEL_MID),
                                  d_et, d_bad)));
    BK_TRY((launch_fused<DEL_MB, 256>(ctx, (int64_t)pl.list[DEL_BLOCK].size(), k, d_Q, ldq, d_w, d_e, d_rows,
                                      units_of(DEL_BLOCK), d_et, d_bad)));
    if (!pl.list[DEL_WIDE].empty()) {
      void* pw = nullptr;
      BK_TRY(ws_get(ctx, SLOT_DEL_WIDE, pl.wide_doubles * (int64_t)sizeof(double), &pw));
      BK_TRY((launch_fused<DEL_WIDE_MB, 512, true>(ctx, (int64_t)pl.list[DEL_WIDE].size(), k, d_Q, ldq, d_w, d_e, d_rows,
                                                   units_of(DEL_WIDE), d_et, d_bad, (double*)pw)));
    }
    BK_TRY(fetch_bad());
    if (!pl.list[DEL_GENERAL].empty()) {
      // in label order, and only the units below the kernels' lowest failing one: a unit that fails here returns at
      // once and is then the lowest failing unit of the call
      void* pg = nullptr;
      BK_TRY(ws_get(ctx, SLOT_DEL_GENERAL, pl.general_doubles * (int64_t)sizeof(double), &pg));
      for (const DelUnit& un : pl.list[DEL_GENERAL]) {
        if (bad != DEL_NO_BAD && (unsigned long long)(unsigned)un.unit > (bad >> 32)) break;
        BK_TRY(general_unit(ctx, un, k, d_Q, ldq, d_w, d_e, d_rows, (double*)pg, d_et));
      }
    }
    return BIGKRLS_OK;
  };
  rc = run();
  BK_TRY(prof_end(ctx, "deletion_residuals"));
  BK_TRY(rc);

  // ---- the first unit whose system is not positive definite ------------------------------------------------------------
  if (bad != DEL_NO_BAD) {
    const int64_t unit = (int64_t)(bad >> 32), col = (int64_t)(bad & 0xffffffffull);
    const int64_t m = h_unit ? pl.size[(size_t)unit] : 1;
    if (m == 1)
      BK_REQUIRE(false, "deletion_residuals: " + del_unit_text(unit, 1) + ": the leverage is >= 1: deleting it is not defined");
    BK_REQUIRE(false, "deletion_residuals: " + del_unit_text(unit, m) + ": the pivot of column " + std::to_string(col + 1) +
                          " of I - H_SS is not positive: a block leverage of 1 or more");
  }
  if (d_S) {
    if (h_unit) return cluster_scores(ctx, n, k, d_Q, ldq, d_et, h_unit, G, d_S, lds);
    std::vector<int64_t> own((size_t)n);
    for (int64_t i = 0; i < n; ++i) own[(size_t)i] = i;
    return cluster_scores(ctx, n, k, d_Q, ldq, d_et, own.data(), n, d_S, lds);
  }
  return BIGKRLS_OK;
}

}  // namespace bk

using namespace bk;

extern "C" {

int bigkrls_dev_deletion_residuals(bigkrls_ctx* ctx, int64_t n, int64_t k, const double* d_Q, int64_t ldq,
                                   const double* h_w, const double* d_e, const int64_t* h_unit, int64_t G, int32_t route,
                                   double* d_et, double* d_hat, double* d_S, int64_t lds) {
  BK_TRY(check_ctx(ctx));
  BK_REQUIRE(h_w && k >= 1 && k < (1ll << 31), "deletion_residuals: null weights or bad dimensions");
  for (int64_t j = 0; j < k; ++j) BK_REQUIRE(std::isfinite(h_w[j]), "deletion_residuals: the weights must be finite");
  void* pw = nullptr;
  BK_TRY(ws_get(ctx, SLOT_DEL_W, k * (int64_t)sizeof(double), &pw));
  double* pin = nullptr;
  BK_HIP(hipStreamSynchronize(ctx->stream));   // (the pinned buffer may be reallocated)
  BK_TRY(pinned_get(ctx, k, &pin));
  std::memcpy(pin, h_w, (size_t)k * sizeof(double));
  BK_HIP(hipMemcpyAsync(pw, pin, (size_t)k * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  return deletion_residuals(ctx, n, k, d_Q, ldq, (const double*)pw, d_e, h_unit, G, (int)route, d_et, d_hat, d_S, lds);
}

int bigkrls_influence(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y, const double* h_coeffs,
                      double sigma, const int64_t* h_which, int64_t n_which, const double* h_newdata, int64_t u,
                      const double* d_Q, int64_t ldq, int64_t k, const double* h_d, double lambda, const double* h_resid,
                      const int64_t* h_unit, int64_t G, double* h_hat, double* h_resid_deleted, double* h_fitted_deleted,
                      double* h_cooks, double* h_dfame, double* h_ame, double* h_var_jack, double* h_r2_loo) {
  if (!h_newdata) u = n;
  BK_TRY(effects_check_args(ctx, "influence", h_X && h_y && h_coeffs && d_Q && h_d && h_resid, n, p, u, sigma));
  BK_REQUIRE(k >= 1 && k <= n && ldq >= n, "influence: bad factors (k must be in [1, n], ldq >= n)");
  BK_REQUIRE(std::isfinite(lambda), "influence: lambda must be finite");
  for (int64_t j = 0; j < k; ++j)
    BK_REQUIRE(std::isfinite(h_d[j]) && h_d[j] + lambda > 0.0, "influence: d_j + lambda must be positive");
  for (int64_t i = 0; i < n; ++i)
    BK_REQUIRE(std::isfinite(h_resid[i]), "influence: the residuals contain missing or infinite values");
  BK_REQUIRE(!h_unit || (G >= 1 && G < (1ll << 31)), "influence: G must be at least 1");   // (the labels: deletion_residuals' plan)
  const int64_t U = h_unit ? G : n;
  const double* nd = h_newdata ? h_newdata : h_X;
  MePrep mp;
  BK_TRY(me_prepare(h_X, n, p, h_y, h_which, n_which, nd, u, &mp));
  const int64_t nj = (int64_t)mp.cols.size(), q = 1 + nj;
  const bool want_ame = h_dfame || h_ame || h_var_jack;
  const bool want_cook = h_cooks != nullptr;
  const bool scores = want_cook && h_unit;
  hipStream_t st = ctx->stream;

  // ---- device layout ---------------------------------------------------------------------------------------------------------
  Layout L;
  const Region Xs = L.up(want_ame ? n * p : 0), Zs = L.up(want_ame ? u * p : 0), B = L.up(want_ame ? n * q : 0),
               Bs = L.up(want_ame ? u * q : 0), cols = L.up_records<MeCol>(want_ame ? nj : 0), g = L.up(k), w = L.up(k),
               w2 = L.up(k), e = L.up(n);
  const Region et = L.dev(n), hat = L.dev(n), num = L.dev(want_cook ? U : 0), ame = L.dev(want_ame ? nj : 0);
  BK_TRY(layout_device(ctx, SLOT_INF_SMALL, &L));
  // C (n x q), S (n x |J|), T (k x |J|), Bm (n x |J|), the AME scores (|J| x U); the units' scores (k x G)
  const int64_t big = (want_ame ? n * q + 2 * n * nj + k * nj + (h_unit ? nj * U : 0) : 0) + (scores ? k * U : 0);
  void* pbig = nullptr;
  BK_TRY(ws_get(ctx, SLOT_INF_BIG, (big + 8) * (int64_t)sizeof(double), &pbig));
  double* dC = (double*)pbig;
  double* dS = dC + (want_ame ? n * q : 0);
  double* dT = dS + (want_ame ? n * nj : 0);
  double* dBm = dT + (want_ame ? k * nj : 0);
  double* dAs = dBm + (want_ame ? n * nj : 0);
  double* dSc = dAs + (want_ame && h_unit ? nj * U : 0);

  // ---- standardise, operands, g, w = d g, w^2, the residuals; ONE upload ---------------------------------------------------
  BK_TRY(layout_pinned(ctx, &L));
  if (want_ame) {
    me_standardise(mp, h_X, n, p, nd, u, L.h(Xs), L.h(Zs));
    me_fill_operands(mp, h_X, n, nd, u, h_coeffs, L.h(Xs), L.h(Zs), L.h(B), L.h(Bs));
    me_stage_cols(mp, Vcov(), L.h<MeCol>(cols), nullptr);
  }
  double trH = 0.0;
  for (int64_t j = 0; j < k; ++j) {
    const double gj = 1.0 / (h_d[j] + lambda), wj = h_d[j] * gj;
    L.h(g)[j] = gj;
    L.h(w)[j] = wj;
    L.h(w2)[j] = wj * wj;
    trH += wj;
  }
  std::memcpy(L.h(e), h_resid, (size_t)n * sizeof(double));
  BK_TRY(layout_upload(ctx, L));

  // ---- the deletion residuals, the leverages, the units' scores ----------------------------------------------------------------
  BK_TRY(deletion_residuals(ctx, n, k, d_Q, ldq, L.d(w), L.d(e), h_unit, G, 0, L.d(et), L.d(hat), scores ? dSc : nullptr, k));
  if (want_cook) {
    if (h_unit) {
      hipLaunchKernelGGL(cook_numerator_kernel, dim3((unsigned)U), dim3(64), 0, st, (int)k, (const double*)dSc, k,
                         (const double*)L.d(w), L.d(num));
      BK_CHECK_LAUNCH();
    } else {
      BK_TRY(rowsumsq_weighted(ctx, n, k, d_Q, ldq, L.d(w2), L.d(num)));      // times et_i^2 on the host
    }
  }
  // ---- the AMEs' column side S (margeff.h), B = Q diag(g) (Q' S), the units' sums of et B ------------------------------------------
  if (want_ame) {
    BK_TRY(kernel_contract(ctx, L.d(Zs), u, u, L.d(Xs), n, n, p, sigma, L.d(Bs), q, u, 1, dC, n));     // C = Kn' B*
    hipLaunchKernelGGL(me_cols_kernel, dim3(launch_blocks(n * nj, 4096)), dim3(256), 0, st, (int)n, (int)nj,
                       (const double*)dC, (const double*)L.d(Xs), (const MeCol*)L.d<MeCol>(cols), sigma, dS, (int64_t)0, n,
                       (int64_t)0);
    BK_CHECK_LAUNCH();
    BK_TRY(gemv(ctx, 1, n, nj, 1.0, dS, n, L.d(B), 0.0, L.d(ame)));                                   // S' c
    BK_TRY(gemm(ctx, 1, 0, k, nj, n, 1.0, d_Q, ldq, dS, n, 0.0, dT, k));                               // T = Q' S
    hipLaunchKernelGGL(scale_rows_kernel, dim3(launch_blocks(k * nj, 4096)), dim3(256), 0, st, (int)k, (int)nj,
                       (const double*)L.d(g), dT);
    BK_CHECK_LAUNCH();
    BK_TRY(gemm(ctx, 0, 0, n, nj, k, 1.0, d_Q, ldq, dT, k, 0.0, dBm, n));                              // B = Q diag(g) T
    if (h_unit) BK_TRY(cluster_scores(ctx, n, nj, dBm, n, L.d(et), h_unit, G, dAs, nj));
  }

  // ---- read back (the calls above may have moved the pinned buffer: ask again, after the stream is idle) ---------------------
  const int64_t o_et = 0, o_hat = n, o_num = 2 * n, o_ame = o_num + (want_cook ? U : 0), o_df = o_ame + (want_ame ? nj : 0);
  const int64_t n_df = want_ame ? (h_unit ? nj * U : n * nj) : 0;
  double* pin = nullptr;
  BK_HIP(hipStreamSynchronize(st));
  BK_TRY(pinned_get(ctx, o_df + n_df + 8, &pin));
  BK_HIP(hipMemcpyAsync(pin + o_et, L.d(et), (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  BK_HIP(hipMemcpyAsync(pin + o_hat, L.d(hat), (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (want_cook) BK_HIP(hipMemcpyAsync(pin + o_num, L.d(num), (size_t)U * sizeof(double), hipMemcpyDeviceToHost, st));
  if (want_ame) {
    BK_HIP(hipMemcpyAsync(pin + o_ame, L.d(ame), (size_t)nj * sizeof(double), hipMemcpyDeviceToHost, st));
    BK_HIP(hipMemcpyAsync(pin + o_df, h_unit ? dAs : dBm, (size_t)n_df * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  BK_HIP(hipStreamSynchronize(st));

  // ---- original units -----------------------------------------------------------------------------------------------------------
  const double* etv = pin + o_et;
  double y_mean, y_sd;
  mean_sd(h_y, n, &y_mean, &y_sd);
  if (h_hat) std::memcpy(h_hat, pin + o_hat, (size_t)n * sizeof(double));
  long double see = 0.0L, set = 0.0L, syy = 0.0L;
  for (int64_t i = 0; i < n; ++i) {
    const double ys = (h_y[i] - y_mean) / y_sd;
    see += (long double)h_resid[i] * h_resid[i];
    set += (long double)etv[i] * etv[i];
    syy += (long double)ys * ys;
    if (h_resid_deleted) h_resid_deleted[i] = y_sd * etv[i];
    if (h_fitted_deleted) h_fitted_deleted[i] = h_y[i] - y_sd * etv[i];
  }
  if (h_r2_loo) *h_r2_loo = (double)(1.0L - set / syy);
  if (want_cook) {
    const double den = trH * ((double)see / ((double)n - trH));
    for (int64_t v = 0; v < U; ++v) h_cooks[v] = (h_unit ? pin[o_num + v] : pin[o_num + v] * etv[v] * etv[v]) / den;
  }
  if (want_ame) {
    for (int64_t jj = 0; jj < nj; ++jj) {
      const int64_t j = mp.cols[jj];
      const double dz = (mp.hi[j] - mp.x_mean[j]) / mp.x_sd[j] - (mp.lo[j] - mp.x_mean[j]) / mp.x_sd[j];
      // AME_j = sd(y) a_j S_j' c (csrc/grpeff.hip: a_e with the group all u new points)
      const double a = y_sd * (mp.isbin[j] ? 1.0 / (dz * (double)u * mp.x_sd[j]) : (-2.0 / sigma) / ((double)u * mp.x_sd[j]));
      if (h_ame) h_ame[jj] = a * pin[o_ame + jj];
      long double ss = 0.0L;
      for (int64_t v = 0; v < U; ++v) {
        const double df = a * (h_unit ? pin[o_df + jj + v * nj] : pin[o_df + v + jj * n] * etv[v]);
        if (h_dfame) h_dfame[v + jj * U] = df;
        ss += (long double)df * df;
      }
      // (the reference's factor 2 on the variance of a binary column, src/bigderiv_v3.cpp:85, as everywhere a variance of an
      // AME is reported: with clusters this is robust_vcov(type = CR3)'s var.avgderivatives)
      if (h_var_jack) h_var_jack[jj] = (mp.isbin[j] ? 2.0 : 1.0) * (double)(((long double)(U - 1) / (long double)U) * ss);
    }
  }
  return BIGKRLS_OK;
}

}  // extern "C"
