// The host plan of the Shapley weights (csrc/shapley.hip): the Gauss-Legendre rule on [0,1] that integrates the product
// game exactly, the player table (validated, and turned into the column order the kernel reads), the kernel's bucket and
// launch shape, the background chunks that go through LDS and the row blocks of the whole-path entry. Plain C++: no HIP
// call, nothing but the standard library -- what tests/shapplan_check.cpp compiles on its own. Internal and header-only,
// as ktplan.h and delplan.h.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace bk {

constexpr int SHAP_MAX_PLAYERS = 128;                 // the cap on M
constexpr int SHAP_MAX_NODES = SHAP_MAX_PLAYERS / 2;  // G = ceil(M / 2) <= 64
constexpr int64_t SHAP_BG_LDS_BYTES = 16384;          // one chunk of background rows in LDS
constexpr int64_t SHAP_BLOCK_BYTES = 1ll << 30;       // one row block of W

// Gauss-Legendre on [0,1]: G nodes t (ascending, strictly inside (0,1), t[g] + t[G-1-g] = 1) and weights w (sum 1), exact
// for polynomials of degree 2G - 1. Newton on the Legendre recurrence in long double from the Chebyshev guess; only the
// lower half is computed, the upper half is its mirror image. 1 <= G <= SHAP_MAX_NODES (else false).
static inline bool shap_gauss_legendre(int G, double* t, double* w) {
  if (G < 1 || G > SHAP_MAX_NODES) return false;
  const long double pi = 3.14159265358979323846264338327950288L;
  for (int i = 0; i < (G + 1) / 2; ++i) {
    long double x = -std::cos(pi * ((long double)i + 0.75L) / ((long double)G + 0.5L)), dp = 1.0L;
    for (int it = 0; it < 100; ++it) {
      long double p0 = 1.0L, p1 = x;                                   // P_0, P_1 ... P_G at x
      for (int k = 2; k <= G; ++k) {
        const long double pk = ((2.0L * k - 1.0L) * x * p1 - (k - 1.0L) * p0) / (long double)k;
        p0 = p1;
        p1 = pk;
      }
      if (G == 1) p0 = 1.0L;
      dp = (long double)G * (x * p1 - p0) / (x * x - 1.0L);            // P_G'
      const long double dx = p1 / dp;
      x -= dx;
      if (std::fabs((double)dx) < 1e-19) break;
    }
    if (2 * i + 1 == G) x = 0.0L;                                      // the middle node of an odd rule
    {   // P_G' once more at the converged node, for the weight
      long double p0 = 1.0L, p1 = x;
      for (int k = 2; k <= G; ++k) {
        const long double pk = ((2.0L * k - 1.0L) * x * p1 - (k - 1.0L) * p0) / (long double)k;
        p0 = p1;
        p1 = pk;
      }
      if (G == 1) p0 = 1.0L;
      dp = (long double)G * (x * p1 - p0) / (x * x - 1.0L);
    }
    const long double wt = 1.0L / ((1.0L - x * x) * dp * dp);          // (2 / ((1 - x^2) P'^2)) / 2
    t[i] = (double)((1.0L + x) / 2.0L);
    t[G - 1 - i] = (double)((1.0L - x) / 2.0L);
    w[i] = w[G - 1 - i] = (double)wt;
  }
  return true;
}

// nodes for M players: the integrand has degree M - 1
static inline int shap_nodes(int64_t M) { return (int)((M + 1) / 2); }

// The player table. h_players[l] in [0, M) is the player of column l (nullptr: column l is player l, M == p). On success
// perm (p) lists the columns player after player, each player's in ascending order, and pstart (M + 1) where each player's
// begin: the kernel walks perm[pstart[m] .. pstart[m + 1]) for player m, so no register array is indexed by a label.
// On failure *err names the offending argument.
static inline bool shap_player_table(const int64_t* h_players, int64_t p, int64_t M, std::vector<int>* pstart,
                                     std::vector<int>* perm, std::string* err) {
  if (p < 1) {
    *err = "p must be at least 1";
    return false;
  }
  if (M < 1) {
    *err = "M must be at least 1";
    return false;
  }
  if (M > SHAP_MAX_PLAYERS) {
    *err = "M = " + std::to_string(M) + " players; at most " + std::to_string(SHAP_MAX_PLAYERS) + " are supported";
    return false;
  }
  if (M > p) {
    *err = "M = " + std::to_string(M) + " players but only " + std::to_string(p) + " columns: a player would be empty";
    return false;
  }
  if (!h_players && M != p) {
    *err = "players is null, so M must equal p (one player per column)";
    return false;
  }
  std::vector<int> count((size_t)M, 0);
  for (int64_t l = 0; l < p; ++l) {
    const int64_t m = h_players ? h_players[l] : l;
    if (m < 0 || m >= M) {
      *err = "players[" + std::to_string(l) + "] = " + std::to_string(m) + " is outside [0, " + std::to_string(M) + ")";
      return false;
    }
    ++count[(size_t)m];
  }
  pstart->assign((size_t)M + 1, 0);
  for (int64_t m = 0; m < M; ++m) {
    if (count[(size_t)m] == 0) {
      *err = "player " + std::to_string(m) + " owns no column";
      return false;
    }
    (*pstart)[(size_t)m + 1] = (*pstart)[(size_t)m] + count[(size_t)m];
  }
  perm->assign((size_t)p, 0);
  std::vector<int> fill(pstart->begin(), pstart->end() - 1);
  for (int64_t l = 0; l < p; ++l) (*perm)[(size_t)fill[(size_t)(h_players ? h_players[l] : l)]++] = (int)l;
  return true;
}

// The kernel's shape for M players. Buckets of up to 32 players keep every per-player array in registers (loops fully
// unrolled over the bucket, players beyond M padded with the neutral factor 1) and give a thread `rows` explained rows, so
// that the background factors are computed once for all of them; the two buckets above keep the arrays in LDS, one
// explained row per thread. threads: per workgroup (one training row each).
struct ShapShape {
  int bucket = 0, rows = 0, threads = 0;
  bool in_lds = false;
};
static inline ShapShape shap_shape(int64_t M) {
  ShapShape s;
  if (M < 1 || M > SHAP_MAX_PLAYERS) return s;
  s.threads = 64;
  if (M <= 8) s.bucket = 8, s.rows = 6;
  else if (M <= 16) s.bucket = 16, s.rows = 3;
  else if (M <= 20) s.bucket = 20, s.rows = 2;
  else if (M <= 24) s.bucket = 24, s.rows = 1;
  else if (M <= 32) s.bucket = 32, s.rows = 1;
  else {
    s.in_lds = true;
    s.rows = 1;
    s.bucket = M <= 64 ? 64 : 128;
    s.threads = M <= 64 ? 64 : 32;                    // four arrays of M doubles per thread: at most 128 KiB of LDS
  }
  return s;
}

// background rows per LDS chunk (chunk x p doubles within SHAP_BG_LDS_BYTES); 0: one row does not fit (p too large)
static inline int64_t shap_chunk_rows(int64_t B, int64_t p) {
  const int64_t fit = SHAP_BG_LDS_BYTES / (8 * p);
  return std::min(B, fit);
}
static inline int64_t shap_max_columns() { return SHAP_BG_LDS_BYTES / 8; }

// dynamic LDS of one workgroup in bytes: the exponential's table, the chunk, and in the LDS buckets the four arrays; in
// the register buckets the tile's training rows when every player is one column (M == p)
static inline int64_t shap_lds_bytes(const ShapShape& s, int64_t M, int64_t chunk, int64_t p) {
  return 8 * (32 + chunk * p + (s.in_lds ? 4 * M * s.threads : (M == p ? p * s.threads : 0)));
}

// explained rows per block of the whole-path entry: the largest b with 8 b M n <= 2^30 bytes, at least 1, at most u;
// block_rows > 0 overrides it (still at most u)
static inline int64_t shap_block_rows(int64_t u, int64_t n, int64_t M, int64_t block_rows) {
  const int64_t b = block_rows > 0 ? block_rows : std::max<int64_t>(1, SHAP_BLOCK_BYTES / (8 * M * n));
  return std::min(b, u);
}

}  // namespace bk
