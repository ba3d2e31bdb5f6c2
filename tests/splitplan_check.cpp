// Stand-alone check of the split-K plan of the plain GEMM family (bigkrls_amd/csrc/splitplan.h), built and run by
// tests/test_splitplan_cpu.py with -fsanitize=address,undefined. The three models (plain GEMM, quadform, skinny48) are
// evaluated over the grid
//     ntile in {1, 2, 3, 79, 157, 255, 256, 391, 782, 4095, 4096}
//     K     in {1, 15, 16, 17, 255, 256, 1023, 1024, 2100, 16383, 16384, 50000, 100000}
//     (M, N) in {(130, 20), (130, 50), (20000, 64), (50000, 128)}
//     development override off (0) and on (5 splits)
// and (splits, k_chunk) must equal, row for row, tests/golden/split_plans.txt (argv[1]), which was recorded once from the
// three separate searches csrc/gemm.hip had before they became one function (two workgroups per CU: 512 resident).
// Row: model ntile K M N override splits k_chunk.
#include "splitplan.h"

#include <cstdio>
#include <cstring>

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: splitplan_check tests/golden/split_plans.txt\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::printf("splitplan_check: cannot open %s\n", argv[1]); return 2; }
  const int ntiles[] = {1, 2, 3, 79, 157, 255, 256, 391, 782, 4095, 4096};
  const int Ks[] = {1, 15, 16, 17, 255, 256, 1023, 1024, 2100, 16383, 16384, 50000, 100000};
  const int MN[][2] = {{130, 20}, {130, 50}, {20000, 64}, {50000, 128}};
  const char* names[] = {"gemm", "quadform", "skinny48"};
  const bk::SplitModel models[] = {bk::split_model_gemm(2), bk::split_model_quadform(2), bk::split_model_skinny48()};
  int failures = 0, multi = 0;
  long long rows = 0;
  char line[256];
  for (int md = 0; md < 3; ++md)
    for (int nt : ntiles)
      for (int K : Ks)
        for (const auto& mn : MN)
          for (int ov : {0, 5}) {
            do {
              if (!std::fgets(line, sizeof line, f)) { std::printf("splitplan_check: golden file ends after %lld rows\n", rows); return 1; }
            } while (line[0] == '#' || line[0] == '\n');
            char name[32];
            int g_nt, g_K, g_M, g_N, g_ov, g_s, g_kc;
            const int got = std::sscanf(line, "%31s %d %d %d %d %d %d %d", name, &g_nt, &g_K, &g_M, &g_N, &g_ov, &g_s, &g_kc);
            const bk::SplitPlan p = bk::split_plan(models[md], nt, mn[0], mn[1], K, 16, ov);
            ++rows;
            multi += p.splits > 1;
            const bool same_case = got == 8 && !std::strcmp(name, names[md]) && g_nt == nt && g_K == K && g_M == mn[0] &&
                                   g_N == mn[1] && g_ov == ov;
            if (!same_case || p.splits != g_s || p.k_chunk != g_kc) {
              if (++failures <= 20)
                std::printf("FAILED row %lld: %s ntile=%d K=%d M=%d N=%d override=%d -> (%d, %d); golden: %s", rows, names[md],
                            nt, K, mn[0], mn[1], ov, p.splits, p.k_chunk, line);
            }
          }
  while (std::fgets(line, sizeof line, f))
    if (line[0] != '#' && line[0] != '\n') { std::printf("splitplan_check: golden file has rows beyond the grid\n"); ++failures; break; }
  std::fclose(f);
  std::printf("splitplan_check: %lld rows, %d of them with more than one split\n", rows, multi);
  if (failures == 0) std::printf("splitplan_check: ok\n");
  else std::printf("splitplan_check: %d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
