// Host plans of the kernel builds and the fused kernel-tile entry points (csrc/gemm.hip) and of cluster_scores
// (csrc/robust.hip): which kernel, how many tiles, where the loop is cut, in which order the rows and entries go. Integer
// arithmetic only, no HIP: a plain host compiler can include this file (tests/ktplan_check.cpp enumerates the plans
// with it). The structs that travel as kernel arguments live here with their layout pinned; csrc/gemm.hip keeps the
// argument checks, the workspace, the uploads and the launches, and reads the development switches it passes in.
#pragma once
#include "syrkmap.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

namespace bk {

// The KS of the tile kernels for p columns: the MFMA steps of the Gram tile where the fragments fit (p <= 32), else 0.
inline int ks_of(int64_t p) {
  const int steps = (int)((p + 3) / 4);
  return steps <= 8 ? steps : 0;
}
// f(std::integral_constant<int, KS>()) for a runtime ks in 0..8
template <class F>
inline auto with_ks(int ks, F&& f) {
  switch (ks) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    case 5: return f(std::integral_constant<int, 5>());
    case 6: return f(std::integral_constant<int, 6>());
    case 7: return f(std::integral_constant<int, 7>());
    case 8: return f(std::integral_constant<int, 8>());
    default: return f(std::integral_constant<int, 0>());
  }
}

// Loop splits against the wave slots: the time is about (rounds of resident waves) x (loop tiles per wave), so the split
// count minimises ceil(base s / slots) / s for `base` tasks per split -- a last round that is nearly empty costs as much
// as a full one (C3 shape: 313 tiles x 7 splits = 2191 waves on 2048 slots took 1.36 ms). At most 64 splits, each at
// least 16 loop tiles (256 rows), all partial sums together at most 64 MB; fewer splits on a tie (a gain below 2 % does
// not count).
inline int64_t plan_loop_splits(int64_t base, int64_t slots, int64_t ltiles, int64_t bytes_per_split) {
  const int64_t max_split = std::max<int64_t>(1, std::min<int64_t>({(int64_t)64, ltiles / 16, (64ll << 20) / bytes_per_split}));
  int64_t nsplit = 1;
  double best = (double)((base + slots - 1) / slots);
  for (int64_t s = 2; s <= max_split; ++s) {
    const double cost = (double)((base * s + slots - 1) / slots) / (double)s;
    if (cost < best * 0.98) { best = cost; nsplit = s; }
  }
  return nsplit;
}

// ---- rows in group order (kernel_contract_grouped_centred, cluster_scores) ---------------------------------------------
// Stable counting sort of n labels in [0, G): group g holds the sorted rows [off[g], off[g + 1]) and sorted row r is row
// perm[r] of the caller, the rows of one group in their original order. bad: the first row whose label is outside
// [0, G), or -1 (off and perm mean nothing then). perm is EMPTY when the order is the identity.
// Rows that are already grouped are recognised first, in a pass without the counters' store-to-load chains: their
// offsets are the places where the label changes. (The host works while the device centres the operands; at n = 20 000
// the counting passes take longer than that and would show.) A stable sort leaves every row in place (r == i for all i)
// exactly when no label is smaller than the one before it, so "the labels never decrease" is the identity test.
struct GroupOrder {
  std::vector<int64_t> off;
  std::vector<int32_t> perm;
  int64_t bad;
};
inline GroupOrder group_order(const int64_t* labels, int64_t n, int64_t G) {
  GroupOrder o{std::vector<int64_t>((size_t)G + 1, 0), {}, -1};
  if (n == 0) return o;
  bool identity = labels[0] >= 0 && labels[n - 1] < G;
  {
    int64_t decreases = 0;
    for (int64_t i = 1; i < n; ++i) decreases += labels[i] < labels[i - 1];
    identity = identity && decreases == 0;
  }
  if (identity) {
    int64_t prev = -1;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t g = labels[i];
      if (g == prev) continue;
      for (int64_t gg = prev + 1; gg <= g; ++gg) o.off[(size_t)gg] = i;
      prev = g;
    }
    for (int64_t gg = prev + 1; gg <= G; ++gg) o.off[(size_t)gg] = n;
    return o;
  }
  for (int64_t i = 0; i < n; ++i) {
    if (labels[i] < 0 || labels[i] >= G) {
      o.bad = i;
      return o;
    }
    ++o.off[(size_t)labels[i] + 1];
  }
  for (int64_t g = 0; g < G; ++g) o.off[(size_t)g + 1] += o.off[(size_t)g];
  o.perm.resize((size_t)n);
  std::vector<int64_t> pos(o.off.begin(), o.off.end() - 1);
  for (int64_t i = 0; i < n; ++i) o.perm[(size_t)(pos[(size_t)labels[i]]++)] = (int32_t)i;
  return o;
}

// ---- the segments of the grouped pass ----------------------------------------------------------------------------
// One task of kernel_contract_grouped_kernel loops over the rows [l_begin, l_end) of one group (a kernel reads the
// table from device memory: the layout is part of its contract).
struct KcgSeg {
  int l_begin, l_end, group, slot;   // slot < 0: the group's only segment
};
static_assert(sizeof(KcgSeg) == 16 && offsetof(KcgSeg, l_begin) == 0 && offsetof(KcgSeg, l_end) == 4 &&
              offsetof(KcgSeg, group) == 8 && offsetof(KcgSeg, slot) == 12, "KcgSeg is read by the grouped kernel");

// plan_loop_splits' model over all groups together: the time is about (rounds of resident waves) x (loop tiles
// of the longest part). A candidate s cuts the largest group (lt_max loop tiles) into s equal parts and every group
// into parts of about that length, s_g = ceil(lt_g s / lt_max), each part at least 16 loop tiles (s_g <= lt_g / 16) and
// at most 64 parts per group; the slots of the groups with s_g > 1 number at most slot_cap (64 MB of partial sums);
// s minimises ceil(base sum_g s_g / slots) / s, fewer parts on a tie (a gain below 2 % does not count). With G = 1 this
// is plan_loop_splits' rule, cuts included: part k of a group is its loop tiles [lt k / s, lt (k + 1) / s).
// off: group_order's offsets; base: tasks per segment; slots: resident waves. multi holds (group, first slot, segments)
// of the groups that are not one segment, the empty ones with 0 segments.
struct GroupedPlan {
  int64_t nsplit;
  std::vector<KcgSeg> segs;
  std::vector<int32_t> multi;
  int64_t nslots;
};
inline GroupedPlan plan_grouped_segments(const int64_t* off, int64_t G, int64_t base, int64_t slots, int64_t slot_cap) {
  int64_t lt_max = 0, nonempty = 0;
  for (int64_t g = 0; g < G; ++g) {
    const int64_t ng = off[g + 1] - off[g];
    lt_max = std::max(lt_max, (ng + 15) / 16);
    nonempty += ng > 0;
  }
  auto parts_of = [&](int64_t g, int64_t s) {
    const int64_t lt = (off[g + 1] - off[g] + 15) / 16;
    const int64_t most = std::max<int64_t>(1, std::min<int64_t>(64, lt / 16));
    return std::min(most, std::max<int64_t>(1, (lt * s + lt_max - 1) / lt_max));
  };
  const int64_t max_split = std::max<int64_t>(1, std::min<int64_t>(64, lt_max / 16));
  GroupedPlan pl{1, {}, {}, 0};
  double best = (double)((base * nonempty + slots - 1) / slots);
  for (int64_t s = 2; s <= max_split; ++s) {
    int64_t nseg = 0, nslots = 0;
    for (int64_t g = 0; g < G; ++g) {
      if (off[g + 1] == off[g]) continue;
      const int64_t sg = parts_of(g, s);
      nseg += sg;
      if (sg > 1) nslots += sg;
    }
    if (nslots > slot_cap) break;   // (the slots grow with s)
    const double cost = (double)((base * nseg + slots - 1) / slots) / (double)s;
    if (cost < best * 0.98) { best = cost; pl.nsplit = s; }
  }
  for (int64_t g = 0; g < G; ++g) {
    const int64_t b = off[g], t = off[g + 1];
    if (b == t) {
      pl.multi.insert(pl.multi.end(), {(int32_t)g, 0, 0});
      continue;
    }
    const int64_t lt = (t - b + 15) / 16, sg = parts_of(g, pl.nsplit);
    if (sg > 1) pl.multi.insert(pl.multi.end(), {(int32_t)g, (int32_t)pl.nslots, (int32_t)sg});
    for (int64_t k = 0; k < sg; ++k) {
      const int64_t t0 = lt * k / sg, t1 = lt * (k + 1) / sg;
      pl.segs.push_back(KcgSeg{(int)(b + 16 * t0), (int)std::min(b + 16 * t1, t), (int)g, sg > 1 ? (int)pl.nslots++ : -1});
    }
  }
  return pl;
}

// ---- the launches of the leave-out moments -----------------------------------------------------------------------
constexpr int KL_GROUP = 64;   // selected columns (kernel_loo_colsums) or entries (kernel_loo_moments) per launch
struct LooMomentEntries {
  int c[KL_GROUP];           // the column every entry leaves out (one value per chunk)
  int j[KL_GROUP];           // kind 1: the weight's column; kind 2: the second column left out; kind 0: c again
  int kind[KL_GROUP];
  int begin[KL_GROUP + 1];   // chunk cc holds the launch's entries [begin[cc], begin[cc + 1])
};
struct LooMomentDest {
  int d[KL_GROUP];           // the caller's column of every entry of the launch
};
static_assert(sizeof(LooMomentEntries) == 4 * (4 * KL_GROUP + 1) && offsetof(LooMomentEntries, c) == 0 &&
              offsetof(LooMomentEntries, j) == 4 * KL_GROUP && offsetof(LooMomentEntries, kind) == 8 * KL_GROUP &&
              offsetof(LooMomentEntries, begin) == 12 * KL_GROUP, "LooMomentEntries is a kernel argument");
static_assert(sizeof(LooMomentDest) == 4 * KL_GROUP && offsetof(LooMomentDest, d) == 0, "LooMomentDest is a kernel argument");

// entries: n_entries triples (kind, c, j), already checked. An entry that leaves out every column (kind 0 at p = 1,
// kind 2 at p = 2) has the exponent 0 in every term: its sums are the number of loop rows, written as such (from the
// Gram tile the exponent would be rounding noise, and the sum u only to ~1e-16): `trivial`. The others in the order of
// their c (stable): `order`; a launch takes up to KL_GROUP of them and a chunk is a run of up to cw entries of one c.
struct LooLaunch {
  LooMomentEntries le;    // the slots past nc repeat the last entry; begin[nchunks .. KL_GROUP] = nc
  LooMomentDest dest;
  int64_t nc, nchunks;
  int64_t nexp;           // exponentials per row pair (the profile's count)
  int64_t first;          // the caller's column of the launch's first entry
  bool in_place;          // the launch's columns are consecutive columns of out, in order
};
struct LooPlan {
  std::vector<int64_t> trivial, order;
  std::vector<LooLaunch> launches;
};
inline LooPlan plan_loo_moments(const int64_t* entries, int64_t n_entries, int64_t p, int64_t cw) {
  LooPlan pl;
  pl.order.reserve((size_t)n_entries);
  for (int64_t e = 0; e < n_entries; ++e) {
    const int64_t kind = entries[3 * e];
    if ((kind == 0 && p == 1) || (kind == 2 && p == 2)) pl.trivial.push_back(e);
    else pl.order.push_back(e);
  }
  std::stable_sort(pl.order.begin(), pl.order.end(),
                   [entries](int64_t a, int64_t b) { return entries[3 * a + 1] < entries[3 * b + 1]; });
  const int64_t n_sorted = (int64_t)pl.order.size();
  for (int64_t g0 = 0; g0 < n_sorted; g0 += KL_GROUP) {
    LooLaunch ln;
    LooMomentEntries& le = ln.le;
    const int64_t nc = ln.nc = std::min<int64_t>(KL_GROUP, n_sorted - g0);
    ln.first = pl.order[(size_t)g0];
    ln.in_place = true;
    for (int64_t i = 0; i < KL_GROUP; ++i) {
      const int64_t e = pl.order[(size_t)(g0 + std::min(i, nc - 1))];
      le.kind[i] = (int)entries[3 * e];
      le.c[i] = (int)entries[3 * e + 1];
      le.j[i] = le.kind[i] == 0 ? le.c[i] : (int)entries[3 * e + 2];
      ln.dest.d[i] = (int)e;
      if (i < nc && e != ln.first + i) ln.in_place = false;
    }
    // chunks: every run of one c, split evenly into pieces of at most cw entries; the exponentials per row pair
    ln.nchunks = ln.nexp = 0;
    for (int64_t r0 = 0; r0 < nc;) {
      int64_t r1 = r0 + 1;
      while (r1 < nc && le.c[r1] == le.c[r0]) ++r1;
      const int64_t len = r1 - r0, pieces = (len + cw - 1) / cw;
      for (int64_t q = 0; q < pieces; ++q) {
        const int64_t b0 = r0 + len * q / pieces, b1 = r0 + len * (q + 1) / pieces;
        le.begin[ln.nchunks++] = (int)b0;
        bool has01 = false;
        for (int64_t i = b0; i < b1; ++i) {
          if (le.kind[i] == 2) ++ln.nexp; else has01 = true;
        }
        if (has01) ++ln.nexp;
      }
      r0 = r1;
    }
    for (int64_t i = ln.nchunks; i <= KL_GROUP; ++i) le.begin[i] = (int)nc;
    pl.launches.push_back(ln);
  }
  return pl;
}

// ---- the launches of the binned leave-out sums (kernel_loo_binsums) ------------------------------------------------
// labels: u x n_cols column-major, the bin of every loop row under selected column jj, in [0, nbins[jj]). Every column
// has an order of its own: idx (u x n_cols, ld u) holds group_order's stable order of column jj in its column (always
// written out, the identity included: the kernel reads its loop rows through it), counts the rows per bin, all columns'
// bins one after the other (bin_off[jj]: the first of column jj -- the caller's output columns).
// A launch takes a run of selected columns: at most KL_GROUP (their numbers travel as a kernel argument), at most
// KLB_BINS bins (a column with more goes alone) and fewer than 2^31 index entries, so that a position in the launch's
// part of idx is an int. Its bins are the groups of ONE plan_grouped_segments call -- the slots are shared by all of
// the launch's columns, so the split is chosen for all of them together -- over the offsets jl u + off_jl[b] (jl the
// column's place in the launch): a segment's l_begin / l_end are positions in the launch's part of idx, l_begin / u is
// its column's place, and its group is the output column counted from the launch's first bin.
// bad_row >= 0: the first label outside its range, of selected column bad_col (nothing else is filled in then).
constexpr int64_t KLB_BINS = 4096;
struct BinLaunch {
  int64_t col0, ncols;   // the selected columns [col0, col0 + ncols)
  int64_t bin0, nb;      // their bins: the output columns [bin0, bin0 + nb)
  GroupedPlan plan;
};
struct BinPlan {
  int64_t bad_row = -1, bad_col = -1;
  std::vector<int32_t> idx;
  std::vector<int64_t> counts, bin_off;
  std::vector<BinLaunch> launches;
};
inline BinPlan plan_loo_binsums(const int64_t* labels, int64_t u, int64_t n_cols, const int64_t* nbins, int64_t base,
                                int64_t slots, int64_t slot_cap) {
  BinPlan pl;
  pl.bin_off.assign((size_t)n_cols + 1, 0);
  for (int64_t jj = 0; jj < n_cols; ++jj) pl.bin_off[(size_t)jj + 1] = pl.bin_off[(size_t)jj] + nbins[jj];
  pl.idx.resize((size_t)(u * n_cols));
  pl.counts.resize((size_t)pl.bin_off[(size_t)n_cols]);
  for (int64_t jj = 0; jj < n_cols; ++jj) {
    const GroupOrder go = group_order(labels + jj * u, u, nbins[jj]);
    if (go.bad >= 0) {
      pl.bad_row = go.bad;
      pl.bad_col = jj;
      return pl;
    }
    int32_t* ix = pl.idx.data() + jj * u;
    for (int64_t i = 0; i < u; ++i) ix[i] = go.perm.empty() ? (int32_t)i : go.perm[(size_t)i];
    for (int64_t b = 0; b < nbins[jj]; ++b)
      pl.counts[(size_t)(pl.bin_off[(size_t)jj] + b)] = go.off[(size_t)b + 1] - go.off[(size_t)b];
  }
  for (int64_t c0 = 0; c0 < n_cols;) {
    int64_t c1 = c0 + 1;
    while (c1 < n_cols && c1 - c0 < KL_GROUP && pl.bin_off[(size_t)c1 + 1] - pl.bin_off[(size_t)c0] <= KLB_BINS &&
           (c1 - c0 + 1) * u < (1ll << 31))
      ++c1;
    BinLaunch ln;
    ln.col0 = c0;
    ln.ncols = c1 - c0;
    ln.bin0 = pl.bin_off[(size_t)c0];
    ln.nb = pl.bin_off[(size_t)c1] - ln.bin0;
    std::vector<int64_t> off((size_t)ln.nb + 1);
    int64_t g = 0;
    for (int64_t jj = c0; jj < c1; ++jj) {
      int64_t at = (jj - c0) * u;
      for (int64_t b = 0; b < nbins[jj]; ++b) {
        off[(size_t)g++] = at;
        at += pl.counts[(size_t)(pl.bin_off[(size_t)jj] + b)];
      }
    }
    off[(size_t)ln.nb] = ln.ncols * u;
    ln.plan = plan_grouped_segments(off.data(), ln.nb, base, slots, slot_cap);
    pl.launches.push_back(std::move(ln));
    c0 = c1;
  }
  return pl;
}

// ---- the kernel build --------------------------------------------------------------------------------------------
// tile rows per band of the wave kernels' order: the band's rows of X (R x 32 x P doubles) take about 1 MB of an XCD's
// 4 MB L2 (r_env > 0, BIGKRLS_KB_R, overrides; a value >= the number of tile rows gives the plain column-by-column order)
inline int kb_band_rows(int64_t p, int tiles, int r_env) {
  int64_t R = r_env > 0 ? r_env : std::max<int64_t>(8, (1 << 20) / (32 * 8 * std::max<int64_t>(p, 1)));
  R = std::max<int64_t>(1, std::min<int64_t>(R, 1024));
  return (int)std::min<int64_t>(R, std::max(tiles, 1));
}

// Non-temporal stores of the output tiles (the wave kernels; the workgroup-tiled kernel always uses them): the 8 N^2
// bytes of K pass through the write-back L2s and evict the rows of X the tiles are built from; with X larger than an
// XCD's 4 MB L2 the re-fetches stall the waves and non-temporal stores are 13 % faster (N = 50 000: 4.80 -> 4.24 ms,
// 4.17 -> 4.71 TB/s written). At N = 20 000, P = 20 (X = 3.2 MB) a loop over the launch alone prefers ordinary stores
// (0.730 vs 0.775 ms, round 4), but INSIDE the fit -- cold caches, the launch once per fit -- non-temporal stores are
// the faster ones (round 5, same-box A/B in fresh processes: 0.620 / 0.628 ms ordinary, 0.597 / 0.595 ms non-temporal;
// profiles/r05/r05b_knob_ab_C3.log): the threshold is X > 2 MB. nt_env >= 0 (BIGKRLS_KB_NT=0|1) overrides.
inline int kb_nontemporal(int64_t rows, int64_t p, int nt_env) {
  if (nt_env >= 0) return nt_env != 0;
  return rows * p * (int64_t)sizeof(double) > (2ll << 20);    // 2 MB
}

// Which kernel builds out (u x v) from p columns, and its grid.
//   KB_TILED: one workgroup per 128 x 128 tile with the X panels in LDS where it beats the one-wave-per-32x32 kernels:
//     P > 32 (measured, TFLOP/s tiled vs wave: N = 100 000, P = 50: 44.7 vs 38.5; N = 30 000, P = 50: 37.2 vs 33.9;
//     N = 50 000, P = 20: 21.1 vs 20.7; N = 20 000, P = 20: 17.8 vs 19.9; force = +1 | -1, BIGKRLS_KB=tiled|wave, forces
//     either). Symmetric: the lower tiles in bands of 32 tile rows -- the A panels of a band are tiny (128 P doubles
//     each), 32 rows keep them and the streamed B panels far inside the L2 --, which is syrk_map_build<128> over all
//     tile columns with that height (r_env > 0 overrides it; more rows where 159 bands would not do).
//   KB_SYM_WAVE (p <= 128): symmetric Gram matrix (bGaussKernel), lower 32 x 32 wave tiles + mirrored stores.
//   KB_WAVE (p <= 128): one wave per 32 x 32 tile.  KB_GENERIC: 128 x 64 tiles through LDS, any p.
// ntiles: tiles of the launch; grid: its workgroups (four wave tiles each). ks: 1..8 MFMA steps per chunk of the wave
// kernels, minimal padding (0 elsewhere); band_rows, nontemporal: the wave kernels' (0 elsewhere); map: KB_TILED's
// (zeros unless sym).
enum KbArm { KB_TILED = 0, KB_SYM_WAVE = 1, KB_WAVE = 2, KB_GENERIC = 3 };
constexpr int KB_GENERIC_BM = 128, KB_GENERIC_BN = 64;
struct KbPlan {
  int arm, tiles_m, tiles_n;
  int64_t ntiles, grid;
  int ks, band_rows, nontemporal;
  SyrkMap map;
};
inline KbPlan kb_plan(int64_t u, int64_t v, int64_t p, bool sym, int force, int r_env, int nt_env) {
  KbPlan k{};
  const bool big = u >= 1024 && v >= 1024;
  if (force > 0 || (force == 0 && big && p > 32)) {
    k.arm = KB_TILED;
    k.tiles_m = (int)((u + 127) / 128);
    k.tiles_n = (int)((v + 127) / 128);
    k.ntiles = (int64_t)k.tiles_m * k.tiles_n;
    if (sym) k.ntiles = syrk_map_build<128>(k.map, k.tiles_m, 0, k.tiles_m, (int)p, false, r_env > 0 ? r_env : 32);
    k.grid = k.ntiles;
    return k;
  }
  if (p > 128) {
    k.arm = KB_GENERIC;
    k.tiles_m = (int)((u + KB_GENERIC_BM - 1) / KB_GENERIC_BM);
    k.tiles_n = (int)((v + KB_GENERIC_BN - 1) / KB_GENERIC_BN);
    k.grid = k.ntiles = (int64_t)k.tiles_m * k.tiles_n;
    return k;
  }
  k.arm = sym ? KB_SYM_WAVE : KB_WAVE;
  k.tiles_m = (int)((u + 31) / 32);
  k.tiles_n = sym ? k.tiles_m : (int)((v + 31) / 32);
  k.ntiles = sym ? (int64_t)k.tiles_m * (k.tiles_m + 1) / 2 : (int64_t)k.tiles_m * k.tiles_n;
  k.grid = (k.ntiles + 3) / 4;
  const int steps = (int)((p + 3) / 4);
  const int chunks = (steps + 7) / 8;
  k.ks = (steps + chunks - 1) / chunks;
  k.band_rows = kb_band_rows(p, k.tiles_m, r_env);
  k.nontemporal = kb_nontemporal(sym ? u : std::max(u, v), p, nt_env);
  return k;
}

}  // namespace bk
