// Stand-alone check of the host plan of the Shapley weights (bigkrls_amd/csrc/shapplan.h): the Gauss-Legendre rules on
// [0,1] for every node count the kernel can ask for, the player table, the kernel shapes, the background chunks and the
// row blocks. Plain C++ with its own main; tests/test_shapplan_cpu.py builds it with -fsanitize=address,undefined.
#include "shapplan.h"

#include <cstdio>
#include <cstdlib>

using namespace bk;

static int failures = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                  \
      std::printf("\n");                         \
      ++failures;                                \
    }                                            \
  } while (0)

static void check_rules() {
  double worst = 0.0;
  int worst_G = 0, worst_k = 0;
  for (int G = 1; G <= SHAP_MAX_NODES; ++G) {
    std::vector<double> t((size_t)G + 1, -7.0), w((size_t)G + 1, -7.0);   // one guard entry each
    CHECK(shap_gauss_legendre(G, t.data(), w.data()), "G = %d refused", G);
    CHECK(t[(size_t)G] == -7.0 && w[(size_t)G] == -7.0, "G = %d wrote past its %d entries", G, G);
    for (int g = 0; g < G; ++g) {
      CHECK(t[g] > 0.0 && t[g] < 1.0, "G = %d: node %d = %.17g is not inside (0,1)", G, g, t[g]);
      CHECK(w[g] > 0.0, "G = %d: weight %d = %.17g is not positive", G, g, w[g]);
      if (g > 0) CHECK(t[g] > t[g - 1], "G = %d: nodes %d, %d are not ascending", G, g - 1, g);
      // symmetric about 1/2: both halves are roundings of (1 -+ x) / 2, so their sum is 1 to one unit in the last place
      CHECK(std::fabs((t[g] + t[G - 1 - g]) - 1.0) <= 2.3e-16, "G = %d: nodes %d and %d are not symmetric about 1/2", G, g,
            G - 1 - g);
      CHECK(w[g] == w[G - 1 - g], "G = %d: weights %d and %d differ", G, g, G - 1 - g);
    }
    if (G % 2 == 1) CHECK(t[G / 2] == 0.5, "G = %d: the middle node is %.17g", G, t[G / 2]);
    // exact for the monomials up to degree 2G - 1: int_0^1 t^k dt = 1 / (k + 1)
    for (int k = 0; k <= 2 * G - 1; ++k) {
      long double s = 0.0L;
      for (int g = 0; g < G; ++g) s += (long double)w[g] * std::pow((long double)t[g], (long double)k);
      const double err = (double)std::fabs(s - 1.0L / (long double)(k + 1));
      if (err > worst) worst = err, worst_G = G, worst_k = k;
      CHECK(err <= 1e-14, "G = %d: moment %d is off by %.3g", G, k, err);
    }
  }
  std::printf("rules: G = 1..%d, worst moment error %.3g (G = %d, k = %d)\n", SHAP_MAX_NODES, worst, worst_G, worst_k);
  double t[2], w[2];
  CHECK(!shap_gauss_legendre(0, t, w) && !shap_gauss_legendre(SHAP_MAX_NODES + 1, t, w), "G outside 1..64 accepted");
  CHECK(shap_nodes(1) == 1 && shap_nodes(2) == 1 && shap_nodes(3) == 2 && shap_nodes(7) == 4 && shap_nodes(128) == 64,
        "shap_nodes");
}

static bool table(const std::vector<int64_t>* lab, int64_t p, int64_t M, std::vector<int>* ps, std::vector<int>* pm,
                  std::string* err) {
  return shap_player_table(lab ? lab->data() : nullptr, p, M, ps, pm, err);
}

static void check_players() {
  std::vector<int> ps, pm;
  std::string err;
  // singletons
  CHECK(table(nullptr, 5, 5, &ps, &pm, &err), "singletons refused: %s", err.c_str());
  for (int l = 0; l < 5; ++l) CHECK(pm[l] == l && ps[l] == l, "singletons: position %d", l);
  CHECK(ps[5] == 5, "singletons: end");
  // grouped, columns out of order
  std::vector<int64_t> lab = {2, 0, 1, 0, 2, 2, 1, 0, 3};
  CHECK(table(&lab, 9, 4, &ps, &pm, &err), "grouped refused: %s", err.c_str());
  const int want_ps[5] = {0, 3, 5, 8, 9}, want_pm[9] = {1, 3, 7, 2, 6, 0, 4, 5, 8};
  for (int m = 0; m <= 4; ++m) CHECK(ps[m] == want_ps[m], "grouped: pstart[%d] = %d", m, ps[m]);
  for (int q = 0; q < 9; ++q) CHECK(pm[q] == want_pm[q], "grouped: perm[%d] = %d", q, pm[q]);
  // every table: perm is a permutation, and position q lies in the range of its column's player
  for (int64_t p = 1; p <= 40; ++p)
    for (int64_t M = 1; M <= p; ++M) {
      std::vector<int64_t> l((size_t)p);
      for (int64_t c = 0; c < p; ++c) l[(size_t)c] = c < M ? M - 1 - c : (c * 7 + 3) % M;
      CHECK(table(&l, p, M, &ps, &pm, &err), "p = %ld M = %ld refused: %s", (long)p, (long)M, err.c_str());
      std::vector<int> seen((size_t)p, 0);
      for (int64_t m = 0; m < M; ++m) {
        CHECK(ps[m + 1] > ps[m], "p = %ld M = %ld: player %ld is empty", (long)p, (long)M, (long)m);
        for (int q = ps[m]; q < ps[m + 1]; ++q) {
          CHECK(pm[q] >= 0 && pm[q] < p && l[(size_t)pm[q]] == m, "p = %ld M = %ld: position %d", (long)p, (long)M, q);
          if (q > ps[m]) CHECK(pm[q] > pm[q - 1], "p = %ld M = %ld: player %ld's columns are not ascending", (long)p, (long)M, (long)m);
          ++seen[(size_t)pm[q]];
        }
      }
      for (int64_t c = 0; c < p; ++c) CHECK(seen[(size_t)c] == 1, "p = %ld M = %ld: column %ld", (long)p, (long)M, (long)c);
    }
  // refusals, each naming its argument
  lab = {0, 1, 3};
  CHECK(!table(&lab, 3, 3, &ps, &pm, &err) && err.find("players[2] = 3") != std::string::npos, "index out of range: %s", err.c_str());
  lab = {0, -1, 1};
  CHECK(!table(&lab, 3, 2, &ps, &pm, &err) && err.find("players[1] = -1") != std::string::npos, "negative index: %s", err.c_str());
  lab = {0, 2, 2};
  CHECK(!table(&lab, 3, 3, &ps, &pm, &err) && err.find("player 1 owns no column") != std::string::npos, "empty player: %s", err.c_str());
  std::vector<int64_t> big(200);
  for (int c = 0; c < 200; ++c) big[(size_t)c] = c % 129;
  CHECK(!table(&big, 200, 129, &ps, &pm, &err) && err.find("M = 129") != std::string::npos && err.find("128") != std::string::npos,
        "cap: %s", err.c_str());
  CHECK(table(&big, 200, 129, &ps, &pm, &err) == false, "cap");
  for (int c = 0; c < 200; ++c) big[(size_t)c] = c % 128;
  CHECK(table(&big, 200, 128, &ps, &pm, &err), "M = 128 refused: %s", err.c_str());
  CHECK(!table(nullptr, 4, 3, &ps, &pm, &err) && err.find("M must equal p") != std::string::npos, "null with M != p: %s", err.c_str());
  lab = {0, 0};
  CHECK(!table(&lab, 2, 3, &ps, &pm, &err) && err.find("M = 3") != std::string::npos, "M > p: %s", err.c_str());
  CHECK(!table(&lab, 2, 0, &ps, &pm, &err) && err.find("M must be at least 1") != std::string::npos, "M = 0: %s", err.c_str());
}

static void check_shapes() {
  for (int64_t M = 1; M <= SHAP_MAX_PLAYERS; ++M) {
    const ShapShape s = shap_shape(M);
    CHECK(s.bucket >= M && s.rows >= 1 && (s.threads == 64 || s.threads == 32), "M = %ld: shape", (long)M);
    CHECK(s.in_lds == (M > 32), "M = %ld: in_lds", (long)M);
    if (M > 8) CHECK(shap_shape(M - 1).bucket <= s.bucket, "M = %ld: buckets not monotone", (long)M);
    // the whole workgroup's LDS with the largest chunk stays inside the 160 KiB of a compute unit
    for (int64_t p : {M, (int64_t)2048}) {
      if (p < M) continue;
      const int64_t chunk = shap_chunk_rows(1000, p);
      CHECK(chunk >= 1 && 8 * chunk * p <= SHAP_BG_LDS_BYTES, "M = %ld p = %ld: chunk %ld", (long)M, (long)p, (long)chunk);
      CHECK(shap_lds_bytes(s, M, chunk, p) <= 160 * 1024, "M = %ld p = %ld: %ld bytes of LDS", (long)M, (long)p,
            (long)shap_lds_bytes(s, M, chunk, p));
    }
  }
  CHECK(shap_shape(0).bucket == 0 && shap_shape(129).bucket == 0, "shape outside 1..128");
  CHECK(shap_shape(8).bucket == 8 && shap_shape(9).bucket == 16 && shap_shape(17).bucket == 20 && shap_shape(21).bucket == 24 &&
            shap_shape(25).bucket == 32 && shap_shape(33).bucket == 64 && shap_shape(65).bucket == 128, "bucket edges");
  // chunks: all rows when they fit, never more than B, 0 only when one row does not fit
  CHECK(shap_chunk_rows(5, 2) == 5 && shap_chunk_rows(130, 33) == 62 && shap_chunk_rows(3, 2048) == 1 && shap_chunk_rows(3, 2049) == 0,
        "chunk rows");
  CHECK(shap_max_columns() == 2048, "max columns");
}

static void check_blocks() {
  for (int64_t n : {1, 2, 60, 1000, 20000, 1000000})
    for (int64_t M : {1, 5, 20, 128})
      for (int64_t u : {1, 7, 1000, 100000}) {
        const int64_t b = shap_block_rows(u, n, M, 0);
        CHECK(b >= 1 && b <= u, "n = %ld M = %ld u = %ld: b = %ld", (long)n, (long)M, (long)u, (long)b);
        CHECK(b == 1 || 8 * b * M * n <= SHAP_BLOCK_BYTES, "n = %ld M = %ld u = %ld: block of %ld rows exceeds 2^30 bytes", (long)n,
              (long)M, (long)u, (long)b);
        // the largest such b
        if (b < u) CHECK(8 * (b + 1) * M * n > SHAP_BLOCK_BYTES, "n = %ld M = %ld u = %ld: b = %ld is not the largest", (long)n, (long)M, (long)u, (long)b);
        for (int64_t ov : {1, 3, 128, 1000000}) {
          const int64_t bo = shap_block_rows(u, n, M, ov);
          CHECK(bo == std::min(ov, u), "override %ld at u = %ld gives %ld", (long)ov, (long)u, (long)bo);
        }
      }
  CHECK(shap_block_rows(1000, 20000, 20, 0) == 335, "the flagship block: %ld rows", (long)shap_block_rows(1000, 20000, 20, 0));
}

int main() {
  check_rules();
  check_players();
  check_shapes();
  check_blocks();
  if (failures) {
    std::printf("shapplan_check: %d failures\n", failures);
    return 1;
  }
  std::printf("shapplan_check: ok\n");
  return 0;
}
