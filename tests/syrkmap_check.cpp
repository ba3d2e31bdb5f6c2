// Stand-alone check of the tile map of the mirrored rank-k update (bigkrls_amd/csrc/syrkmap.h), built and run by
// tests/test_syrkmap_cpu.py with -fsanitize=address,undefined. For both tile widths every block id of a launch is decoded
// with the function the kernel runs, and the result must be exactly the set
//     {(tc, tm): c0 <= tc < c1, tc / CPT <= tm < tiles},
// every tile once, with the builder's return value equal to that count. Each map lives in a heap block of its own size,
// so the sanitizer sees a band table that outgrows band_start. The walk of the whole lower tile triangle (lower_tile_of:
// gram_weighted_kernel, gram_reduce_kernel, syrk_lower_kernel) is compared with the plain loop for every T up to 1024.
#include "syrkmap.h"

#include <cstdio>
#include <memory>
#include <vector>

using bk::SyrkMap;

static int failures = 0;
static long long cases = 0, decoded = 0;
static char g_where[160] = "";   // the case a failure belongs to
#define CHECK(cond, ...)                                              \
  do {                                                                \
    if (!(cond)) {                                                    \
      if (++failures <= 20) {                                         \
        std::printf("FAILED %s:%d: %s  [%s", __FILE__, __LINE__, #cond, g_where); \
        std::printf(__VA_ARGS__);                                     \
        std::printf("]\n");                                           \
      }                                                               \
    }                                                                 \
  } while (0)

// One launch: c1 <= CPT * tiles; order_cols and r_override are the builder's two development switches.
template <int BN>
static void check_case(int tiles, int c0, int c1, int k, bool order_cols, int r_override) {
  constexpr int CPT = 128 / BN;
  ++cases;
  std::snprintf(g_where, sizeof g_where, "BN=%d tiles=%d c0=%d c1=%d k=%d cols=%d R_override=%d: ", BN, tiles, c0, c1, k,
                (int)order_cols, r_override);
  std::unique_ptr<SyrkMap> mp(new SyrkMap);
  const int64_t nt = bk::syrk_map_build<BN>(*mp, tiles, c0, c1, k, order_cols, r_override);
  int64_t want = 0;
  for (int tc = c0; tc < c1; ++tc) want += tiles - tc / CPT;
  CHECK(nt == want, "nt=%lld want=%lld", (long long)nt, (long long)want);
  if (nt != want || nt == 0) return;
  CHECK(nt < (1ll << 31), "nt=%lld", (long long)nt);
  CHECK(mp->tiles == tiles && mp->c0 == c0 && mp->c1 == c1, "map fields");
  if (order_cols) {
    CHECK(mp->R == 0, "R=%d", mp->R);
    int64_t before = 0;
    for (int tc = 0; tc < c0; ++tc) before += tiles - tc / CPT;
    CHECK(mp->t_off == before, "t_off=%d want=%lld", mp->t_off, (long long)before);
  } else {
    CHECK(mp->R > 0 && mp->nband >= 1 && mp->nband <= bk::SYRK_MAX_BANDS, "R=%d nband=%d", mp->R, mp->nband);
    if (mp->nband < 1 || mp->nband > bk::SYRK_MAX_BANDS) return;
    if (r_override > 0 && (tiles - c0 / CPT + r_override - 1) / r_override < bk::SYRK_MAX_BANDS)
      CHECK(mp->R == r_override, "R=%d", mp->R);
    if (r_override <= 0 && tiles <= 2 * bk::SYRK_MAX_BANDS) {   // the L2 rule: about 2 MB of A panels per band
      const int64_t byk = (2 << 20) / ((int64_t)128 * 8 * k);
      const int rule = (int)(byk > 32 ? 32 : (byk < 2 ? 2 : byk));
      CHECK(mp->R == rule, "R=%d rule=%d", mp->R, rule);
    }
    CHECK(mp->band_start[0] == 0 && mp->band_start[mp->nband] == nt, "band_start ends");
    for (int b = 0; b < mp->nband; ++b)
      CHECK(mp->band_start[b] <= mp->band_start[b + 1], "band_start[%d] decreases", b);
    CHECK(mp->band0 * mp->R <= c0 / CPT && c0 / CPT < (mp->band0 + 1) * mp->R, "band0=%d", mp->band0);
  }
  std::vector<unsigned char> seen((size_t)(c1 - c0) * (size_t)tiles, 0);
  for (int64_t bid = 0; bid < nt; ++bid) {
    const bk::SyrkTile tile = bk::syrk_map_decode<BN>(*mp, (int)bid, (int)nt);
    const int tc = tile.tc, tm = tile.tm, p = tile.p;
    const bool inside = tc >= c0 && tc < c1 && tm >= tc / CPT && tm < tiles;
    CHECK(inside, "block %lld -> (tc=%d, tm=%d)", (long long)bid, tc, tm);
    if (!inside) return;
    CHECK(p == tc / CPT, "block %lld -> p=%d tc=%d", (long long)bid, p, tc);
    unsigned char& s = seen[(size_t)(tc - c0) * (size_t)tiles + (size_t)tm];
    CHECK(s == 0, "tile (tc=%d, tm=%d) twice, second time by block %lld", tc, tm, (long long)bid);
    if (s) return;
    s = 1;
  }
  decoded += nt;   // nt distinct tiles inside a set of nt: every tile exactly once
}

template <int BN>
static void check_orders(int tiles, int c0, int c1, const std::vector<int>& ks) {
  for (int k : ks) check_case<BN>(tiles, c0, c1, k, false, 0);
  for (int r : {1, 2, 3, 5}) check_case<BN>(tiles, c0, c1, 128, false, r);
  check_case<BN>(tiles, c0, c1, 128, true, 0);
  check_case<BN>(tiles, c0, c1, 128, true, 3);   // the column order wins over a band height
}

template <int BN>
static void check_width() {
  constexpr int CPT = 128 / BN;
  const std::vector<int> ks = {64, 128, 256, 512, 1024, 4096};
  for (int tiles = 1; tiles <= 13; ++tiles)
    for (int c0 = 0; c0 < CPT * tiles; ++c0)
      for (int c1 = c0 + 1; c1 <= CPT * tiles; ++c1) check_orders<BN>(tiles, c0, c1, ks);
  for (int tiles : {40, 157, 318, 319, 330, 700}) {
    const int nc = CPT * tiles;
    for (int c0 : {0, 1, 3, nc / 2, nc - 1})
      for (int c1 : {nc, c0 + 1, c0 + (nc - c0 + 1) / 2}) check_orders<BN>(tiles, c0, c1, ks);
  }
  // empty ranges: nothing to launch
  for (int tiles : {1, 2, 13, 157})
    for (int c : {0, 1, CPT * tiles - 1, CPT * tiles}) {
      check_case<BN>(tiles, c, c, 128, false, 0);
      check_case<BN>(tiles, c, c, 128, true, 0);
    }
}

int main() {
  // xcd_remap is a bijection of [0, n) for every grid size
  for (int n = 1; n <= 600; ++n) {
    std::vector<unsigned char> seen((size_t)n, 0);
    for (int b = 0; b < n; ++b) {
      const int t = bk::xcd_remap(b, n);
      CHECK(t >= 0 && t < n && !seen[(size_t)(t < 0 || t >= n ? 0 : t)], "xcd_remap(%d, %d) = %d", b, n, t);
      if (t >= 0 && t < n) seen[(size_t)t] = 1;
    }
  }
  // ... and gives XCD x (block ids x, x + 8, ...) one contiguous run
  for (int n : {8, 9, 15, 16, 1000, 1001})
    for (int b = 8; b < n; ++b) CHECK(bk::xcd_remap(b, n) == bk::xcd_remap(b - 8, n) + 1, "xcd_remap run at %d of %d", b, n);
  // lower_tile_of (closed form with fix-ups) against the plain column-major walk of the lower tile triangle, for every
  // tile of every grid of 1 to 1024 tile rows
  long long walked = 0;
  for (int T = 1; T <= 1024; ++T) {
    int t = 0;
    for (int tn = 0; tn < T; ++tn)
      for (int tm = tn; tm < T; ++tm, ++t) {
        const bk::LowerTile lt = bk::lower_tile_of(t, T);
        CHECK(lt.tm == tm && lt.tn == tn, "lower_tile_of(%d, %d) = (%d, %d), the walk gives (%d, %d)", t, T, lt.tm, lt.tn, tm, tn);
      }
    CHECK(t == T * (T + 1) / 2, "T=%d: %d tiles", T, t);
    walked += t;
  }
  std::printf("syrkmap_check: %lld lower-triangle tiles walked\n", walked);
  check_width<64>();
  check_width<128>();
  std::printf("syrkmap_check: %lld maps, %lld tiles decoded\n", cases, decoded);
  if (failures == 0) std::printf("syrkmap_check: ok\n");
  else std::printf("syrkmap_check: %d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
