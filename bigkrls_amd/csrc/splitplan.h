// The deterministic split-K choice of the plain GEMM family (csrc/gemm.hip): one search over a small time model, and the
// three models the family uses side by side. Arithmetic only, no HIP: a plain host compiler can include this file
// (tests/splitplan_check.cpp compares the three models with recorded plans).
//
// The split count is chosen against the workgroups the GPU holds at once: ntile * splits workgroups take
// ceil(ntile * splits / resident) rounds of K / splits k-steps each, plus a cost per split (prologue, partial store,
// reduction). A count that spills a few workgroups into one more round pays that whole round: m = 20 000, n = 64
// (157 tiles): 7 splits 1.02 ms, 6 or 3 splits 0.95 ms; m = 10 000 (79 tiles): 13 splits 0.30 ms, 6 splits 0.26 ms.
#pragma once
#include <algorithm>

namespace bk {

// Rough time model in us.
struct SplitModel {
  int resident;           // workgroups the GPU holds at once (256 CUs times the kernel's occupancy)
  double step_cost;       // a k-step of a workgroup, per unit of K
  double slab_cost;       // per split and output element: the partial slab is written and read again
  double slab_cost_long;  // the same for ntile >= 256 && K >= 16384 (equal to slab_cost: no second rule)
  bool gated;             // split only when ntile < 4096 && K >= 1024 (off: always search)
  bool dev_override;      // the development override of the count applies (products with K >= 16384)
  bool clamp;             // k_chunk >= bk and splits >= 1 are enforced (off: the caller guarantees K > 0)
};

// gemm, gemm_modulated(2), gram_weighted: 16 bytes per output element and split at ~5 TB/s plus a fixed ~0.2 us. Also
// above one round: 782 tiles -- N = 100 000 times a 128-column block -- fill 1.53 rounds unsplit, i.e. run at 76 %; five
// splits fill 7.6 of 8. Long products of many tiles (the block-Lanczos product, 391 tiles x K = 50 000: 5 splits 10.18 ms,
// 9 or 13 splits 9.98 ms, tools/kb_shape_probe.hip): the slab traffic costs half of what the model charged.
constexpr SplitModel split_model_gemm(int occ) { return {256 * occ, 0.06, 3.2e-6, 1.6e-6, true, true, true}; }
// quadform_diag: per split the partials are one double per row and column tile, but the epilogue reads A's m x n again:
// 8 bytes per element of the product instead of the 16 of gemm's partial slabs.
constexpr SplitModel split_model_quadform(int occ) { return {256 * occ, 0.06, 1.6e-6, 1.6e-6, true, false, true}; }
// gemm_nn_skinny48: two workgroups per CU, a cheaper k-step (128 x 48 tile), always through the slabs.
constexpr SplitModel split_model_skinny48() { return {512, 0.045, 3.2e-6, 3.2e-6, false, false, false}; }

struct SplitPlan { int splits, k_chunk; };   // number of k slabs; slab length, a multiple of bk

// ntile tiles of an M x N result over a contraction of K, k-tiles of bk; override_splits > 0: the development override.
inline SplitPlan split_plan(const SplitModel& md, int ntile, int M, int N, int K, int bk, int override_splits) {
  int splits = 1;
  if (!md.gated || (ntile < 4096 && K >= 1024)) {
    const int maxs = std::min(64, std::max(1, K / 256));
    const double per_split = ((ntile >= 256 && K >= 16384) ? md.slab_cost_long : md.slab_cost) * (double)M * (double)N + 0.2;
    double best = 1e30;
    for (int sp = 1; sp <= maxs; ++sp) {
      const int rounds = (ntile * sp + md.resident - 1) / md.resident;
      const double cost = md.step_cost * rounds * ((double)K / sp) + per_split * sp;
      if (cost < best - 1e-9) { best = cost; splits = sp; }
    }
  }
  if (md.dev_override && override_splits > 0 && K >= 16384) splits = override_splits;
  int k_chunk = ((K + splits - 1) / splits + bk - 1) / bk * bk;
  if (md.clamp && k_chunk < bk) k_chunk = bk;
  splits = (K + k_chunk - 1) / k_chunk;
  if (md.clamp && splits < 1) splits = 1;
  return SplitPlan{splits, k_chunk};
}

// ---- thin products: the executed tile width apart from the split plan ------------------------------------------------
// gemm() ties the tile width to the column count (N <= 32: 32, N <= 64: 64, else 128). A product of few tiles and a long
// contraction per tile -- the three products of a step of the stage-1 back-transform: (512 x m0)(m0 x 250) split over K,
// 512 x 512 x 250 and m0 x 512 x 250 -- then runs as a handful of workgroups that each walk a long k loop while most of
// the GPU stands empty. gemm_thin() (csrc/gemm.hip) runs such a product with narrower tiles: every accumulator receives
// the same MFMA sequence over k whatever the width, and the slabs of a split product stay those of gemm(), so the result
// is gemm()'s bit for bit.
struct ThinPlan { int bn_exec, splits, k_chunk; };

// gemm()'s tile width of an N-column result
inline int thin_base_bn(int N) { return N <= 32 ? 32 : (N <= 64 ? 64 : 128); }

// The width rule, a function of the shape alone: a launch that at gemm()'s width has fewer workgroups (tiles * splits)
// than the GPU holds at once (`resident`) runs 32 wide, provided the k loop of a workgroup (K per split) is at least
// thin_min_k long; every other launch keeps gemm()'s width. Measured alone on the GPU (tools/bt1_thin_bench.py,
// profiles/bt1/sweep.txt; us at 128 / 64 / 32 wide): Tb W1 (8 workgroups at 128) 84 / 47 / 33 at every m0;
// Zs -= Vb W2, m0 = 20 000 (314): 151 / 124 / 116, 10 000: 93 / 79 / 67, 2 000: 89 / 49 / 34; Vb' Zs with its reduction,
// m0 = 20 000: 143 / 138 / 146, 5 000: 58 / 56 / 51, 2 000: 56 / 36 / 29; the three in order 371 / 300 / 288,
// 243 / 193 / 177 (10 000), 228 / 132 / 93 (2 000). A 32-wide workgroup alone on a CU is bound by latency (33 us against the
// 22 us a quarter of the 128-wide tile's 89 us would be) and two of them on a CU overlap, so 32 also wins where it makes
// several rounds; 64 wins single shapes by a few us (m0 = 15 000: 81 against 93) and is left to the development switch.
// thin_min_k is split_plan's own floor of a slab (it never cuts K below 256): shorter loops were not measured.
constexpr int thin_min_k = 256;
inline int thin_width(int base_bn, int tiles_m, int N, int splits, int k_per_split, int resident) {
  const long long wgs = (long long)tiles_m * ((N + base_bn - 1) / base_bn) * splits;
  return (k_per_split >= thin_min_k && wgs < resident) ? 32 : base_bn;
}

// (splits, k_chunk): split_plan() under the plain model over gemm()'s own tiling of the M x N result, whatever width
// executes -- the slab boundaries decide the bits (that tiling is the 128-wide one: up to N = 64 either has one tile
// column). occ: workgroups per CU of gemm()'s kernel for this shape; bm: the
// tile height; force_bn = 32, 64 or 128 sets the executed width (development), anything else: the rule.
inline ThinPlan thin_plan(bool /*ta*/, bool /*tb*/, int M, int N, int K, int bm, int bk, int occ, int override_splits,
                          int force_bn = 0) {
  const int base = thin_base_bn(N);
  const int tiles_m = (M + bm - 1) / bm;
  const SplitModel md = split_model_gemm(occ);
  const SplitPlan sp = split_plan(md, tiles_m * ((N + base - 1) / base), M, N, K, bk, override_splits);
  const int bn = (force_bn == 32 || force_bn == 64 || force_bn == 128)
               ? force_bn
               : thin_width(base, tiles_m, N, sp.splits, std::min(K, sp.k_chunk), md.resident);
  return ThinPlan{bn, sp.splits, sp.k_chunk};
}

}  // namespace bk
