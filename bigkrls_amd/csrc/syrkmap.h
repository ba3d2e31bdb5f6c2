// Tile order of the mirrored rank-k update (syrk_mirror_kernel, csrc/gemm.hip): the map a launch carries, its host-side
// builder and the decode a workgroup runs. Index arithmetic only, no HIP: a plain host compiler can include this file
// (tests/syrkmap_check.cpp enumerates whole grids with it).
//
// R == 0: column by column from tile t_off (consecutive workgroups = consecutive XCDs take consecutive row tiles of one
// tile column, so every XCD streams the whole A operand through its L2 once per tile column). R > 0: XCD-aware,
// L2-blocked: the tiles of the BN-wide columns [c0, c1) are ordered band by band (a band = R consecutive 128-row tiles),
// inside a band column by column, and every XCD takes a contiguous eighth of that sequence (xcd_remap): an XCD keeps the
// R row panels of A of its band in its L2 and walks the columns, so each panel of B is fetched once per band instead of
// each panel of A once per column.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define BK_HD __host__ __device__ __forceinline__
#else
#define BK_HD inline
#endif

namespace bk {

// XCD-aware tile order: consecutive block ids round-robin over the 8 XCDs, so give
// each XCD a contiguous run of tiles (neighbouring tiles share operand panels in
// that XCD's L2). Bijective for any grid size.
BK_HD int xcd_remap(int bid, int nblocks) {
  const int nx = 8;
  const int q = nblocks / nx, rem = nblocks % nx;
  const int x = bid % nx, i = bid / nx;
  // blocks of xcd x: q + (x < rem) of them
  const int start = x * q + (x < rem ? x : rem);
  return start + i;
}

// Column-major walk of the lower triangle of a T x T tile grid: tile t of T (T + 1) / 2 -> (row tm >= column tn). Column
// tn starts at tn T - tn (tn - 1) / 2; tn is the largest integer with that start <= t: the closed form, then fix-ups for
// the rounding of the square root. (gram_weighted_kernel, gram_reduce_kernel, syrk_lower_kernel)
struct LowerTile { int tm, tn; };
BK_HD LowerTile lower_tile_of(int t, int T) {
  int tn = (int)((2.0 * T + 1.0 - sqrt((2.0 * T + 1.0) * (2.0 * T + 1.0) - 8.0 * t)) * 0.5);
  while (tn > 0 && tn * T - tn * (tn - 1) / 2 > t) --tn;
  while ((tn + 1) * T - (tn + 1) * tn / 2 <= t) ++tn;
  return LowerTile{tn + (t - (tn * T - tn * (tn - 1) / 2)), tn};
}

constexpr int SYRK_MAX_BANDS = 159;
struct SyrkMap {
  int tiles;            // 128-row tiles of the matrix
  int c0, c1;           // BN-wide tile columns of this launch
  int R, nband, band0;  // rows per band, number of bands, first band (absolute index)
  int t_off;            // R == 0 only
  int band_start[SYRK_MAX_BANDS + 1];  // band b (relative) starts at sequence index band_start[b]; [nband] = number of tiles
};

#if defined(__HIP_DEVICE_COMPILE__)
BK_HD int syrk_imin(int a, int b) { return min(a, b); }
BK_HD int syrk_imax(int a, int b) { return max(a, b); }
#else
BK_HD int syrk_imin(int a, int b) { return a < b ? a : b; }
BK_HD int syrk_imax(int a, int b) { return a > b ? a : b; }
#endif

// Workgroup `bid` of a grid of `nblocks` -> its tile: BN-wide tile column tc, 128-row tile row tm, and p = tc / CPT, the
// row tile of column tc's diagonal (tm == p: the tile holds a piece of the diagonal).
struct SyrkTile { int tc, tm, p; };
template <int BN>
BK_HD SyrkTile syrk_map_decode(const SyrkMap& map, int bid, int nblocks) {
  int tc, tm, p;
  constexpr int CPT = 128 / BN;   // tile columns per 128-wide column pair
  const int tiles = map.tiles;
  if (map.R == 0) {
    const int t = bid + map.t_off;
    // lower-triangular tiles, column by column; columns come in groups of CPT that share their
    // first row tile p: group p has CPT * (tiles - p) tiles and starts at CPT * (p tiles - p(p-1)/2)
    p = (int)((2.0 * tiles + 1.0 - sqrt((2.0 * tiles + 1.0) * (2.0 * tiles + 1.0) - 8.0 * t / CPT)) * 0.5);
    auto gstart = [&](int q) { return CPT * (q * tiles - q * (q - 1) / 2); };
    while (p > 0 && gstart(p) > t) --p;
    while (gstart(p + 1) <= t) ++p;
    const int rem = t - gstart(p);
    tc = CPT * p + rem / (tiles - p);          // tile column (BN wide)
    tm = p + rem % (tiles - p);                // tile row (128 high)
  } else {
    const int sq = xcd_remap(bid, nblocks);
    int lo = 0, hi = map.nband;                // band_start[lo] <= sq < band_start[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (map.band_start[mid] <= sq) lo = mid; else hi = mid;
    }
    int sp = sq - map.band_start[lo];
    const int r0 = (map.band0 + lo) * map.R, r1 = syrk_imin(r0 + map.R, tiles);
    // columns whose diagonal tile lies at or above r0 hold all r1 - r0 rows of the band ...
    const int cfull = syrk_imax(syrk_imin(map.c1, CPT * (r0 + 1)), map.c0);
    const int nfull = (cfull - map.c0) * (r1 - r0);
    if (sp < nfull) {
      tc = map.c0 + sp / (r1 - r0);
      tm = r0 + sp % (r1 - r0);
    } else {   // ... the columns through the band's diagonal corner hold the rows from their diagonal tile down
      sp -= nfull;
      tc = cfull;
      while (sp >= r1 - tc / CPT) { sp -= r1 - tc / CPT; ++tc; }
      tm = tc / CPT + sp;
    }
    p = tc / CPT;
  }
  return SyrkTile{tc, tm, p};
}

// Host side of SyrkMap: the BN-wide columns [c0, c1) of the lower tile triangle (tile rows from the diagonal down), for
// an inner dimension k. Returns the number of tiles = workgroups of the launch (0: nothing to do). order_cols: the
// column-by-column order (R == 0); r_override > 0: that many rows per band instead of the L2 rule. Both are development
// switches that csrc/gemm.hip reads from the environment.
template <int SBN>
inline int64_t syrk_map_build(SyrkMap& mp, int tiles, int c0, int c1, int k, bool order_cols, int r_override) {
  constexpr int CPT = 128 / SBN;
  mp.tiles = tiles; mp.c0 = c0; mp.c1 = c1; mp.t_off = 0; mp.nband = 0; mp.band0 = 0;
  auto col_first = [&](int64_t c) -> int64_t {   // column-major index of the first tile of BN-wide column c
    const int64_t q = c / CPT;
    if (q >= tiles) return CPT * ((int64_t)tiles * tiles - (int64_t)tiles * (tiles - 1) / 2);
    return CPT * (q * tiles - q * (q - 1) / 2) + (c % CPT) * (tiles - q);
  };
  const int64_t nt = col_first(c1) - col_first(c0);
  if (order_cols || nt <= 0) {
    mp.R = 0;
    mp.t_off = (int)col_first(c0);
    return nt;
  }
  // rows per band: the band's A panels (R x 128 x k doubles) take about 2 MB of the XCD's 4 MB L2
  int R = r_override > 0 ? r_override : (int)std::min<int64_t>(32, std::max<int64_t>(2, (2 << 20) / ((int64_t)128 * 8 * std::max(k, 1))));
  const int first_row = c0 / CPT;
  // bands are cut at multiples of R from row 0, so a range that starts inside a band spans one band more than its
  // tiles - first_row rows need: count the bands themselves
  while ((tiles + R - 1) / R - first_row / R > SYRK_MAX_BANDS) ++R;
  mp.R = R;
  mp.band0 = first_row / R;
  int64_t acc = 0;
  int nb = 0;
  for (int b = mp.band0; b * R < tiles; ++b, ++nb) {
    mp.band_start[nb] = (int)acc;
    const int r0 = b * R, r1 = std::min(r0 + R, tiles);
    for (int tm = r0; tm < r1; ++tm) acc += std::max(0, std::min(c1, CPT * (tm + 1)) - c0);
  }
  mp.band_start[nb] = (int)acc;
  mp.nband = nb;
  return acc;   // == nt
}

}  // namespace bk
