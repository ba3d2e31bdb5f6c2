// What the post-estimation entries on the modulation m_j(i,l) = r_j[i] + t_j[i] s_j[l] share (csrc/margeff.hip: the
// marginal effects and their standard errors; csrc/inteff.hip: the interaction effects): the per-column constants, the
// row- and column-side finalise of the two contractions (also csrc/grpeff.hip: the group effects), the r / t / s
// kernels, the column dots, the host-side preparation, the operands of the two contractions and the frame of the
// pointwise standard errors. Internal and header-only: every user compiles it inside its own translation unit
// (anonymous namespace), nothing here joins the exported symbols.
#pragma once
#include "hostprep.h"

#include <cstring>
#include <string>
#include <vector>

namespace bk {
namespace {

// Per-column constants of the selected columns (device, 4 per column): is_binary, z0, z1 and the column index.
struct MeCol {
  double bin, z0, z1, col;
};

// out[j] = sum_k S[k,j] T[k,j]; one block per column, fixed order
__global__ __launch_bounds__(256) void me_coldot_kernel(int n, const double* __restrict__ S,
                                                        const double* __restrict__ T, double* __restrict__ out) {
  __shared__ double sh[4];
  const double* s = S + (int64_t)blockIdx.x * n;
  const double* t = T + (int64_t)blockIdx.x * n;
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a = fma(s[i], t[i], a);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// S (n x nj, ld n): s of every selected column -- Xs_kj, or the training group indicator (Xs == z1, as me_cols_kernel)
__global__ void me_se_s_kernel(int n, int nj, const double* __restrict__ Xs, const MeCol* __restrict__ cols,
                               double* __restrict__ S) {
  const int64_t total = (int64_t)n * nj;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(e % n);
    const MeCol cj = cols[e / n];
    const double x = Xs[k + (int64_t)cj.col * n];
    S[e] = cj.bin == 0.0 ? x : (x == cj.z1 ? 1.0 : 0.0);
  }
}

// R, T (rows x nj, ld rows): r and t of one block of new points (Zs: the block's first row, ld ldz). The group of a new
// point in a binary column is Zs == z1: newdata holds one of the two training values there (validated) and is
// standardised by the expression that gives z1.
__global__ void me_se_rt_kernel(int rows, int nj, const double* __restrict__ Zs, int64_t ldz,
                                const MeCol* __restrict__ cols, double sigma, double* __restrict__ R,
                                double* __restrict__ T) {
  const int64_t total = (int64_t)rows * nj;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e % rows);
    const MeCol cj = cols[e / rows];
    const double z = Zs[i + (int64_t)cj.col * ldz];
    double r, t;
    if (cj.bin == 0.0) {
      r = (-2.0 / sigma) * z;
      t = 2.0 / sigma;
    } else {
      const double sd = 1.0 / (cj.z1 - cj.z0);
      const double phi = -1.0 / (sd * sd * sigma);
      const double E = exp(phi), Einv = exp(-phi);
      r = z == cj.z1 ? sd * (1.0 - Einv) : -sd * (1.0 - E);
      t = sd * (Einv - E);
    }
    R[e] = r;
    T[e] = t;
  }
}

// D (u x nj, ld u): row side. R (u x q, ld u) = Kn B, Zs (u x p, ld u), Bs (u x q) = B* (its binary columns are the
// newdata group indicators h_j).
__global__ void me_rows_kernel(int u, int nj, const double* __restrict__ R, const double* __restrict__ Zs,
                               const double* __restrict__ Bs, const MeCol* __restrict__ cols, double sigma,
                               double* __restrict__ D) {
  const int64_t total = (int64_t)u * nj;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(e % u);
    const int jj = (int)(e / u);
    const MeCol cj = cols[jj];
    const double Kc = R[i];
    const double Kvc = R[(int64_t)(1 + jj) * u + i];
    double dv;
    if (cj.bin == 0.0) {
      const double z = Zs[i + (int64_t)cj.col * u];
      dv = (-2.0 / sigma) * (z * Kc - Kvc);
    } else {
      const double sd = 1.0 / (cj.z1 - cj.z0);
      const double phi = -1.0 / (sd * sd * sigma);
      const double E = exp(phi), Einv = exp(-phi);
      const bool hi = Bs[(int64_t)(1 + jj) * u + i] != 0.0;
      const double Sc = hi ? Kvc : Kc - Kvc;     // over the training rows of the point's own group
      const double Oc = hi ? Kc - Kvc : Kvc;     // ... and of the other one
      dv = sd * (hi ? 1.0 : -1.0) * ((1.0 - E) * Sc + (1.0 - Einv) * Oc);
    }
    D[e] = dv;
  }
}

// S: column side. C (n x q, ld n) = Kn' B*, Xs (n x p, ld n). s_k for continuous columns, a_k for binary ones (training
// group of k: Xs == z1, the fit's own test, csrc/deriv.hip). Column jj is written at S + jj s_col. blockIdx.y is a group
// of new points (csrc/grpeff.hip): its block of C starts at c_group doubles per group, its columns of S at s_group; one
// set of new points (csrc/margeff.hip) is gridDim.y = 1, s_col = n.
__global__ void me_cols_kernel(int n, int nj, const double* __restrict__ Cm, const double* __restrict__ Xs,
                               const MeCol* __restrict__ cols, double sigma, double* __restrict__ S, int64_t c_group,
                               int64_t s_col, int64_t s_group) {
  const int64_t total = (int64_t)n * nj;
  Cm += (int64_t)blockIdx.y * c_group;
  S += (int64_t)blockIdx.y * s_group;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(e % n);
    const int jj = (int)(e / n);
    const MeCol cj = cols[jj];
    const double T = Cm[k];                                  // sum_i Kn[i,k]
    const double H = Cm[(int64_t)(1 + jj) * n + k];          // sum_i Kn[i,k] Zs_ij, or over the new points with h = 1
    const double x = Xs[k + (int64_t)cj.col * n];
    double sv;
    if (cj.bin == 0.0) {
      sv = H - x * T;
    } else {
      const double sd = 1.0 / (cj.z1 - cj.z0);
      const double phi = -1.0 / (sd * sd * sigma);
      const double E = exp(phi), Einv = exp(-phi);
      sv = (x == cj.z1) ? (1.0 - E) * H + (Einv - 1.0) * (T - H) : (1.0 - Einv) * H + (E - 1.0) * (T - H);
    }
    S[k + (int64_t)jj * s_col] = sv;
  }
}

// the selected columns (0-based), the training moments and the two-valued columns
struct MePrep {
  std::vector<int64_t> cols;
  std::vector<double> x_mean, x_sd, lo, hi;
  std::vector<char> isbin;
  double y_sd = 0.0;
  MeCol col(int64_t jj) const {
    const int64_t j = cols[jj];
    return MeCol{isbin[j] ? 1.0 : 0.0, (lo[j] - x_mean[j]) / x_sd[j], (hi[j] - x_mean[j]) / x_sd[j], (double)j};
  }
};

int me_prepare(const double* h_X, int64_t n, int64_t p, const double* h_y, const int64_t* h_which, int64_t n_which,
               const double* h_newdata, int64_t u, MePrep* mp) {
  std::vector<int64_t>& cols = mp->cols;
  if (h_which) {
    BK_REQUIRE(n_which > 0, "marginal_effects: which_derivatives is empty");
    for (int64_t i = 0; i < n_which; ++i) {
      BK_REQUIRE(h_which[i] >= 1 && h_which[i] <= p, "which.derivatives must index columns of X");
      cols.push_back(h_which[i] - 1);
    }
  } else {
    for (int64_t j = 0; j < p; ++j) cols.push_back(j);
  }
  for (int64_t i = 0; i < u * p; ++i)
    BK_REQUIRE(std::isfinite(h_newdata[i]), "marginal_effects: newdata contains missing or infinite values");
  std::vector<double>&x_mean = mp->x_mean, &x_sd = mp->x_sd, &lo = mp->lo, &hi = mp->hi;
  std::vector<char>& isbin = mp->isbin;
  x_mean.resize(p); x_sd.resize(p); lo.resize(p); hi.resize(p); isbin.resize(p);
  for (int64_t j = 0; j < p; ++j) {
    mean_sd(h_X + j * n, n, &x_mean[j], &x_sd[j]);
    BK_REQUIRE(x_sd[j] > 0.0, "marginal_effects: training column " + std::to_string(j + 1) + " is constant");
    isbin[j] = two_valued(h_X + j * n, n, &lo[j], &hi[j]);
  }
  for (size_t i = 0; i < cols.size(); ++i) {
    const int64_t j = cols[i];
    if (!isbin[j]) continue;
    const double* z = h_newdata + j * u;
    for (int64_t r = 0; r < u; ++r)
      BK_REQUIRE(z[r] == lo[j] || z[r] == hi[j],
                 "newdata column " + std::to_string(j + 1) +
                     " is binary in the training data; its values must be one of the two training values");
  }
  double y_mean;
  mean_sd(h_y, n, &y_mean, &mp->y_sd);
  BK_REQUIRE(mp->y_sd > 0.0, "marginal_effects: y is a constant");
  return BIGKRLS_OK;
}

// hXs (n x p), hZs (u x p): X and newdata standardised with the training means and sds, as bigkrls_predict
void me_standardise(const MePrep& mp, const double* h_X, int64_t n, int64_t p, const double* h_newdata, int64_t u,
                    double* hXs, double* hZs) {
  for (int64_t j = 0; j < p; ++j) {
    standardise_column(h_X + j * n, n, mp.x_mean[j], mp.x_sd[j], hXs + j * n);
    standardise_column(h_newdata + j * u, u, mp.x_mean[j], mp.x_sd[j], hZs + j * u);
  }
}

// the per-column constants and the weights of the factors, into their staged regions
void me_stage_cols(const MePrep& mp, const Vcov& vc, MeCol* hcols, double* hw) {
  for (size_t jj = 0; jj < mp.cols.size(); ++jj) hcols[jj] = mp.col((int64_t)jj);
  if (vc.cols() > 0) std::memcpy(hw, vc.h_w, (size_t)vc.cols() * sizeof(double));
}

// the operands of the two contractions: hB (n x q) = [c, {x_j o c | b_j o c}_j], hBs (u x q) = [1, {Zs_j | h_j}_j],
// q = 1 + |J|; b_j / h_j: the group indicators of a binary column on the raw training / new values
void me_fill_operands(const MePrep& mp, const double* h_X, int64_t n, const double* h_newdata, int64_t u,
                      const double* h_coeffs, const double* hXs, const double* hZs, double* hB, double* hBs) {
  for (int64_t i = 0; i < n; ++i) hB[i] = h_coeffs[i];
  for (int64_t i = 0; i < u; ++i) hBs[i] = 1.0;
  for (int64_t jj = 0; jj < (int64_t)mp.cols.size(); ++jj) {
    const int64_t j = mp.cols[jj];
    const double* x = h_X + j * n;
    const double* z = h_newdata + j * u;
    double* b = hB + (1 + jj) * n;
    double* bs = hBs + (1 + jj) * u;
    if (mp.isbin[j]) {                                // group membership on the raw values
      for (int64_t i = 0; i < n; ++i) b[i] = (x[i] == mp.hi[j] ? 1.0 : 0.0) * h_coeffs[i];
      for (int64_t i = 0; i < u; ++i) bs[i] = z[i] == mp.hi[j] ? 1.0 : 0.0;
    } else {
      for (int64_t i = 0; i < n; ++i) b[i] = hXs[j * n + i] * h_coeffs[i];
      std::memcpy(bs, hZs + j * u, (size_t)u * sizeof(double));
    }
  }
}

// ---- the pointwise standard errors (bigkrls_marginal_effects_se, bigkrls_interaction_effects_se) -------------------
// One row block of the new points as the per-item body sees it: Kn (rows x n, ld rows), r and t of the block's rows
// (rows x nj, ld rows), s of the training rows (n x nj, ld n), the factors' weights, and P beside the block: rows x k
// (factors) or rows x n (matrix) doubles.
struct SeBlock {
  int64_t rows;
  const double *Kn, *R, *T, *S, *w;
  double* P;
};

// After the entry's checks and me_prepare: the new points in row blocks of the test kernel (at most 1 GiB, or
// block_rows), per block Kn_b once and body(i, block, out) for each of the nout items, which writes the block's
// quadratic forms g' V g of item i to out (rows doubles); h_se[i] = sqrt(max(scale(i) var, 0)), a form that rounds
// below zero being zero. vc is the matrix or the factors.
template <class Body, class Scale>
int me_se_frame(bigkrls_ctx* ctx, const MePrep& mp, const double* h_X, int64_t n, int64_t p, const double* h_newdata,
                int64_t u, double sigma, const Vcov& vc, int64_t block_rows, int64_t nout, Body body, Scale scale,
                double* h_se) {
  const int64_t k = vc.cols(), nj = (int64_t)mp.cols.size();
  // rows per block: beside the b x n block of the test kernel, T = G Q (b x k) or the stored G (b x n)
  const int64_t wide = vc.d_Q ? k : n;
  const int64_t b = std::min(block_rows > 0 ? block_rows : pointwise_block_rows(n, wide), u);

  hipStream_t st = ctx->stream;
  Layout L;
  const Region Xs = L.up(n * p), Zs = L.up(u * p), nx = L.up(n), nz = L.up(u), cols = L.up_records<MeCol>(nj),
               w = L.up(k);
  const Region S = L.dev(n * nj), R = L.dev(b * nj), T = L.dev(b * nj), se = L.down(u * nout);
  BK_TRY(layout_device(ctx, SLOT_ME_SMALL, &L));
  void* pk = nullptr;
  BK_TRY(ws_get(ctx, SLOT_PP_K, b * (n + wide) * (int64_t)sizeof(double), &pk));
  double* dKn = (double*)pk;

  // standardise, squared row norms (the training rows are centred by their standardisation: no further shift), upload
  BK_TRY(layout_pinned(ctx, &L));
  me_standardise(mp, h_X, n, p, h_newdata, u, L.h(Xs), L.h(Zs));
  host_sqnorms(L.h(Xs), n, p, L.h(nx));
  host_sqnorms(L.h(Zs), u, p, L.h(nz));
  me_stage_cols(mp, vc, L.h<MeCol>(cols), L.h(w));
  BK_TRY(layout_upload(ctx, L));
  hipLaunchKernelGGL(me_se_s_kernel, dim3(launch_blocks(n * nj, 4096)), dim3(256), 0, st, (int)n, (int)nj,
                     (const double*)L.d(Xs), (const MeCol*)L.d<MeCol>(cols), L.d(S));
  BK_CHECK_LAUNCH();

  for (int64_t r0 = 0; r0 < u; r0 += b) {
    const int64_t rows = std::min(b, u - r0);
    BK_TRY(kernel_block_centred(ctx, L.d(Zs) + r0, rows, u, L.d(nz) + r0, L.d(Xs), n, n, L.d(nx), p, sigma, dKn, rows, -1));
    hipLaunchKernelGGL(me_se_rt_kernel, dim3(launch_blocks(rows * nj, 4096)), dim3(256), 0, st, (int)rows, (int)nj,
                       (const double*)(L.d(Zs) + r0), u, (const MeCol*)L.d<MeCol>(cols), sigma, L.d(R), L.d(T));
    BK_CHECK_LAUNCH();
    const SeBlock blk{rows, dKn, L.d(R), L.d(T), L.d(S), L.d(w), dKn + b * n};
    for (int64_t i = 0; i < nout; ++i) BK_TRY(body(i, blk, L.d(se) + i * u + r0));
  }
  BK_TRY(layout_download(ctx, L));
  for (int64_t i = 0; i < nout; ++i) {
    const double sc = scale(i);
    const double* v = L.pinned() + i * u;
    for (int64_t r = 0; r < u; ++r) h_se[i * u + r] = std::sqrt(std::max(sc * v[r], 0.0));
  }
  return BIGKRLS_OK;
}

}  // namespace
}  // namespace bk
