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

}  // namespace bk
