// What the post-estimation entries on the modulation m_j(i,l) = r_j[i] + t_j[i] s_j[l] share (csrc/margeff.hip: the
// marginal effects and their standard errors; csrc/inteff.hip: the interaction effects): the per-column constants, the
// row- and column-side finalise of the two contractions (also csrc/grpeff.hip: the group effects), the r / t / s
// kernels, the column dots, the argument checks and the host-side preparation. Internal and header-only: every user
// compiles it inside its own translation unit (anonymous namespace), nothing here joins the exported symbols.
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

int me_check_args(bigkrls_ctx* ctx, const double* h_X, int64_t n, int64_t p, const double* h_y, const double* h_coeffs,
                  double sigma, const double* h_newdata, int64_t u, const void* h_out) {
  BK_TRY(check_ctx(ctx));
  BK_REQUIRE(h_X && h_y && h_coeffs && h_newdata && h_out, "marginal_effects: null argument");
  BK_REQUIRE(n > 1 && p > 0 && u > 0 && n < (1ll << 31) && u < (1ll << 31), "marginal_effects: bad dimensions");
  BK_REQUIRE(sigma > 0.0 && std::isfinite(sigma), "marginal_effects: sigma must be a positive scalar");
  return BIGKRLS_OK;
}

int me_check_factors(const Vcov& vc, int64_t n) {
  if (vc.d_Q) BK_REQUIRE(vc.h_w && vc.k > 0 && vc.k <= n && vc.ldq >= n, "marginal_effects: bad factors of vcov.est.c");
  return BIGKRLS_OK;
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

}  // namespace
}  // namespace bk
