// Stand-alone check of thin_plan (bigkrls_amd/csrc/splitplan.h), the plan of gemm_thin: built and run by
// tests/test_thinplan_cpu.py with -fsanitize=address,undefined. Over
//     M in {64, 128, ..., 512}, N in 1 ... 300, all four transposes,
//     K in {1, 15, 16, 17, 255 ... 257, 511 ... 513, 1023 ... 1025, 2047, 2048, 2600, 4095, 4096, 9999, 16383, 16384,
//           19936, 20000} and 1000, 2000, ..., 24000
// it requires
//   * (splits, k_chunk) to equal split_plan() under the plain model over the 128-wide tiling of the result, with the
//     development override off and on, under the rule and under every forced width: the slabs never move with the width;
//   * bn_exec in {32, 64, 128}, the same in two calls (a function of the shape only), and the forced width when one is forced;
//   * N <= 32 to run 32 wide and N <= 64 at most 64 wide: never wider than gemm()'s own choice;
//   * a width below gemm()'s only where the k loop of a workgroup is at least thin_min_k long and the launch fits the
//     workgroups the GPU holds at once (the rule as splitplan.h states it);
//   * the three products of a back-transform step at the benchmark's shapes to get the widths DESIGN.md section 4 records.
#include "splitplan.h"

#include <cstdio>
#include <vector>

int main() {
  const int BM = 128, BK = 16, OCC = 2;
  std::vector<int> Ks = {1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2600, 4095, 4096, 9999,
                         16383, 16384, 19936, 20000};
  for (int K = 1000; K <= 24000; K += 1000) Ks.push_back(K);
  const bk::SplitModel md = bk::split_model_gemm(OCC);
  long long plans = 0, narrowed = 0, multi = 0;
  int failures = 0;
  auto fail = [&](const char* what, int M, int N, int K, const bk::ThinPlan& p) {
    if (++failures <= 20) std::printf("FAILED %s: M=%d N=%d K=%d -> bn %d splits %d k_chunk %d\n", what, M, N, K, p.bn_exec, p.splits, p.k_chunk);
  };
  for (int M = 64; M <= 512; M += 64)
    for (int N = 1; N <= 300; ++N)
      for (int K : Ks)
        for (int ov : {0, 5}) {
          const int tiles_m = (M + BM - 1) / BM;
          const bk::SplitPlan want = bk::split_plan(md, tiles_m * ((N + 127) / 128), M, N, K, BK, ov);
          const int base = N <= 32 ? 32 : (N <= 64 ? 64 : 128);      // with_bn of csrc/gemm.hip
          const bk::ThinPlan p = bk::thin_plan(false, false, M, N, K, BM, BK, OCC, ov);
          ++plans;
          narrowed += p.bn_exec < base;
          multi += p.splits > 1;
          if (p.splits != want.splits || p.k_chunk != want.k_chunk) fail("slabs differ from split_plan on the 128-wide tiling", M, N, K, p);
          if (p.bn_exec != 32 && p.bn_exec != 64 && p.bn_exec != 128) fail("width not 32, 64 or 128", M, N, K, p);
          if (p.bn_exec > base) fail("wider than gemm()'s tile", M, N, K, p);
          if (N <= 32 && p.bn_exec != 32) fail("N <= 32 not 32 wide", M, N, K, p);
          if (p.bn_exec < base) {
            const long long wgs = (long long)tiles_m * ((N + base - 1) / base) * p.splits;
            if (std::min(K, p.k_chunk) < bk::thin_min_k) fail("narrowed with a short k loop", M, N, K, p);
            if (wgs >= md.resident) fail("narrowed a launch that fills the GPU at gemm()'s width", M, N, K, p);
          }
          for (int t = 0; t < 4; ++t) {
            const bk::ThinPlan q = bk::thin_plan(t & 1, t & 2, M, N, K, BM, BK, OCC, ov);
            if (q.bn_exec != p.bn_exec || q.splits != p.splits || q.k_chunk != p.k_chunk) fail("not a function of the shape", M, N, K, q);
          }
          for (int f : {32, 64, 128}) {
            const bk::ThinPlan q = bk::thin_plan(false, false, M, N, K, BM, BK, OCC, ov, f);
            if (q.bn_exec != f || q.splits != want.splits || q.k_chunk != want.k_chunk) fail("forced width", M, N, K, q);
          }
        }
  // a step of the back-transform at the benchmark's shapes (w = 512 rows of reflectors, nv = 250 vectors): Vb' Zs, Tb W1,
  // Zs -= Vb W2 at m0 = 20 000 and 2 000; a short contraction; a launch of 782 tiles, more than the GPU holds at once
  struct { int M, N, K, bn; } pinned[] = {{512, 250, 20000, 32}, {512, 250, 512, 32}, {20000, 250, 512, 32},
                                          {512, 250, 2000, 32},  {2000, 250, 512, 32}, {512, 250, 255, 128},
                                          {512, 60, 255, 64},    {50000, 250, 512, 128}};
  for (const auto& c : pinned) {
    const bk::ThinPlan p = bk::thin_plan(false, false, c.M, c.N, c.K, BM, BK, OCC, 0);
    if (p.bn_exec != c.bn) fail("recorded width", c.M, c.N, c.K, p);
  }
  std::printf("thinplan_check: %lld plans, %lld narrower than gemm()'s tile, %lld with more than one split\n", plans, narrowed, multi);
  if (failures == 0) std::printf("thinplan_check: ok\n");
  else std::printf("thinplan_check: %d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
