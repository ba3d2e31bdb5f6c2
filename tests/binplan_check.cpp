// Stand-alone check of the host plan of the binned leave-out sums (plan_loo_binsums, bigkrls_amd/csrc/ktplan.h), built
// and run by tests/test_binplan_cpu.py with -fsanitize=address,undefined.
//
//   binplan_check            check the invariants of every plan of the grid below against brute force
//
// What kernel_loo_binsums_kernel relies on: every selected column's index list is the stable order of its labels, a
// permutation of 0 .. u - 1; the launches tile the selected columns in order within their limits; the segments of a
// launch lie inside one bin of one column each, tile every bin in order with cuts at multiples of 16 rows from the bin's
// start, cover every position of the launch's part of the index list exactly once, and carry the output column of
// their bin; a bin of one segment has no slot, the segments of a cut bin have consecutive slots that the multi triples
// name, and an empty bin is a triple with no segment. The first label out of range is reported by row and column.
// The last line printed for the long-bin shape of tests/test_gpu_accumulated_effects.py says how many bins are cut.
#include "ktplan.h"

#include <cstdarg>
#include <cstdio>
#include <numeric>

namespace {

long long g_failures = 0, g_plans = 0, g_cut_plans = 0, g_multi_launch = 0, g_empty_bins = 0, g_bad = 0;

void fail(const char* fmt, ...) {
  if (++g_failures > 20) return;
  va_list ap;
  va_start(ap, fmt);
  std::printf("FAILED: ");
  std::vprintf(fmt, ap);
  std::printf("\n");
  va_end(ap);
}
#define REQUIRE(cond, ...) do { if (!(cond)) fail(__VA_ARGS__); } while (0)

// patterns: 0 sorted, 1 reversed, 2 interleaved, 3 pseudo-random, 4 sorted with the middle bin empty, 5 one row in the
// first and in the last bin and the rest in the middle, 6 / 7 a label = B / -1 somewhere in an interleaved column
void make_labels(int64_t u, int64_t B, int pat, int64_t seed, int64_t* lab) {
  uint64_t s = 88172645463325252ull + (uint64_t)seed * 2654435761ull;
  for (int64_t i = 0; i < u; ++i) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    int64_t b;
    if (pat == 0) b = i * B / u;
    else if (pat == 1) b = B - 1 - i * B / u;
    else if (pat == 3) b = (int64_t)(s % (uint64_t)B);
    else if (pat == 4) { b = i * B / u; if (B >= 3 && b == B / 2) b = B / 2 - 1; }
    else if (pat == 5) b = i == 0 ? 0 : (i == u - 1 ? B - 1 : B / 2);
    else b = i % B;
    lab[i] = b;
  }
  if (pat == 6) lab[u / 2] = B;
  if (pat == 7) lab[u - 1] = -1;
}

// returns the number of cut bins, or -1 for a refused plan
long long check_case(int64_t u, const std::vector<int64_t>& nbins, const std::vector<int>& pats, int64_t base, int64_t slots,
                     int64_t slot_cap) {
  const int64_t nc = (int64_t)nbins.size();
  std::vector<int64_t> lab((size_t)(u * nc));
  for (int64_t jj = 0; jj < nc; ++jj) make_labels(u, nbins[(size_t)jj], pats[(size_t)jj], jj, lab.data() + jj * u);
  const bk::BinPlan pl = bk::plan_loo_binsums(lab.data(), u, nc, nbins.data(), base, slots, slot_cap);
  ++g_plans;
  // the first label out of range, columns first
  int64_t bad_row = -1, bad_col = -1;
  for (int64_t jj = 0; jj < nc && bad_col < 0; ++jj)
    for (int64_t i = 0; i < u; ++i)
      if (lab[(size_t)(i + jj * u)] < 0 || lab[(size_t)(i + jj * u)] >= nbins[(size_t)jj]) { bad_row = i; bad_col = jj; break; }
  REQUIRE(pl.bad_row == bad_row && pl.bad_col == bad_col, "u=%lld nc=%lld: bad label at (%lld, %lld), expected (%lld, %lld)",
          (long long)u, (long long)nc, (long long)pl.bad_row, (long long)pl.bad_col, (long long)bad_row, (long long)bad_col);
  if (bad_col >= 0 || pl.bad_col >= 0) { ++g_bad; return -1; }

  // the index lists and the counts against a stable sort
  int64_t nbt = 0;
  for (int64_t jj = 0; jj < nc; ++jj) {
    REQUIRE(pl.bin_off[(size_t)jj] == nbt, "bin_off of column %lld", (long long)jj);
    std::vector<int32_t> ref((size_t)u);
    std::iota(ref.begin(), ref.end(), 0);
    const int64_t* l = lab.data() + jj * u;
    std::stable_sort(ref.begin(), ref.end(), [&](int32_t a, int32_t b) { return l[a] < l[b]; });
    bool same = true;
    for (int64_t i = 0; i < u; ++i) same = same && pl.idx[(size_t)(i + jj * u)] == ref[(size_t)i];
    REQUIRE(same, "u=%lld column %lld: the index list is not the stable order", (long long)u, (long long)jj);
    std::vector<int64_t> hist((size_t)nbins[(size_t)jj], 0);
    for (int64_t i = 0; i < u; ++i) ++hist[(size_t)l[i]];
    for (int64_t b = 0; b < nbins[(size_t)jj]; ++b) {
      const int64_t c = hist[(size_t)b];
      REQUIRE(pl.counts[(size_t)(nbt + b)] == c, "u=%lld column %lld bin %lld: count", (long long)u, (long long)jj, (long long)b);
      g_empty_bins += c == 0;
    }
    nbt += nbins[(size_t)jj];
  }
  REQUIRE(pl.bin_off[(size_t)nc] == nbt && (int64_t)pl.counts.size() == nbt && (int64_t)pl.idx.size() == u * nc, "sizes");

  // the launches and their segments
  long long cut = 0;
  int64_t next_col = 0;
  for (const bk::BinLaunch& ln : pl.launches) {
    REQUIRE(ln.col0 == next_col && ln.ncols >= 1 && ln.col0 + ln.ncols <= nc, "launch columns");
    REQUIRE(ln.ncols <= bk::KL_GROUP && ln.ncols * u < (1ll << 31), "launch limits");
    REQUIRE(ln.bin0 == pl.bin_off[(size_t)ln.col0] && ln.nb == pl.bin_off[(size_t)(ln.col0 + ln.ncols)] - ln.bin0, "launch bins");
    REQUIRE(ln.ncols == 1 || ln.nb <= bk::KLB_BINS, "launch bin budget");
    if (ln.col0 + ln.ncols < nc)   // greedy: the next column did not fit
      REQUIRE(ln.ncols == bk::KL_GROUP || ln.nb + nbins[(size_t)(ln.col0 + ln.ncols)] > bk::KLB_BINS ||
                  (ln.ncols + 1) * u >= (1ll << 31), "a launch ends before its limits");
    next_col = ln.col0 + ln.ncols;
    const bk::GroupedPlan& gp = ln.plan;
    std::vector<char> covered((size_t)(ln.ncols * u), 0);
    std::vector<int64_t> nseg_of((size_t)ln.nb, 0), next_at((size_t)ln.nb, -1), first_slot((size_t)ln.nb, -1);
    // every group's column (its place in the launch), bin and first position
    std::vector<int64_t> g_col((size_t)ln.nb), g_bin((size_t)ln.nb), g_begin((size_t)ln.nb);
    for (int64_t jl = 0, g = 0; jl < ln.ncols; ++jl) {
      int64_t at = jl * u;
      for (int64_t b = 0; b < nbins[(size_t)(ln.col0 + jl)]; ++b, ++g) {
        g_col[(size_t)g] = jl;
        g_bin[(size_t)g] = b;
        g_begin[(size_t)g] = at;
        at += pl.counts[(size_t)(ln.bin0 + g)];
      }
    }
    for (const bk::KcgSeg& s : gp.segs) {
      REQUIRE(s.group >= 0 && s.group < ln.nb, "segment group");
      if (s.group < 0 || s.group >= ln.nb) continue;
      // the bin of the group: its column's place in the launch and its range of positions
      const int64_t jl = g_col[(size_t)s.group], b = g_bin[(size_t)s.group], begin = g_begin[(size_t)s.group];
      const int64_t end = begin + pl.counts[(size_t)(ln.bin0 + s.group)];
      REQUIRE(s.l_begin < s.l_end && s.l_begin >= begin && s.l_end <= end, "segment outside its bin");
      REQUIRE(s.l_begin / u == jl && (s.l_end - 1) / u == jl, "segment outside its column");
      REQUIRE((s.l_begin - begin) % 16 == 0, "segment cut off a multiple of 16");
      const int64_t want = next_at[(size_t)s.group] < 0 ? begin : next_at[(size_t)s.group];
      REQUIRE(s.l_begin == want, "segments of a bin out of order");
      next_at[(size_t)s.group] = s.l_end;
      if (nseg_of[(size_t)s.group] == 0) first_slot[(size_t)s.group] = s.slot;
      else REQUIRE(s.slot == first_slot[(size_t)s.group] + nseg_of[(size_t)s.group], "slots of a cut bin not consecutive");
      ++nseg_of[(size_t)s.group];
      for (int64_t l = s.l_begin; l < s.l_end && l < (int64_t)covered.size(); ++l) {
        REQUIRE(!covered[(size_t)l], "a position covered twice");
        covered[(size_t)l] = 1;
      }
      // every row the segment reads belongs to its bin
      for (int64_t l = s.l_begin; l < s.l_end; ++l) {
        const int32_t row = pl.idx[(size_t)(ln.col0 * u + l)];
        REQUIRE(row >= 0 && row < u && lab[(size_t)(row + (ln.col0 + jl) * u)] == b, "a segment's row is not of its bin");
      }
    }
    bool all = true;
    for (char c : covered) all = all && c;
    REQUIRE(all, "positions not covered");
    std::vector<char> in_multi((size_t)ln.nb, 0);
    int64_t slots_used = 0;
    for (size_t i = 0; i + 3 <= gp.multi.size(); i += 3) {
      const int g = gp.multi[i], first = gp.multi[i + 1], cnt = gp.multi[i + 2];
      REQUIRE(g >= 0 && g < ln.nb, "multi group");
      if (g < 0 || g >= ln.nb) continue;
      in_multi[(size_t)g] = 1;
      REQUIRE(cnt == nseg_of[(size_t)g] && cnt != 1, "multi count");
      if (cnt > 1) {
        REQUIRE(first == first_slot[(size_t)g] && first == slots_used, "multi first slot");
        slots_used += cnt;
        ++cut;
      }
    }
    REQUIRE(slots_used == gp.nslots && gp.nslots <= slot_cap, "slot count");
    for (int64_t g = 0; g < ln.nb; ++g) {
      REQUIRE((nseg_of[(size_t)g] == 1) == !in_multi[(size_t)g], "multi membership");
      if (nseg_of[(size_t)g] == 1) REQUIRE(first_slot[(size_t)g] < 0, "a whole bin with a slot");
      REQUIRE((nseg_of[(size_t)g] == 0) == (pl.counts[(size_t)(ln.bin0 + g)] == 0), "segments of an empty bin");
    }
  }
  REQUIRE(next_col == nc, "launches do not cover the columns");
  g_cut_plans += cut > 0;
  g_multi_launch += pl.launches.size() > 1;
  return cut;
}

}  // namespace

int main() {
  const int64_t us[] = {1, 2, 15, 17, 33, 65, 130, 700, 4099};
  for (int64_t u : us)
    for (int64_t nc : {(int64_t)1, (int64_t)2, (int64_t)5, (int64_t)65, (int64_t)130})
      for (int pat0 = 0; pat0 < 8; ++pat0)
        for (int64_t bsel = 0; bsel < 4; ++bsel)
          for (int64_t base : {(int64_t)1, (int64_t)9})
            for (int64_t slots : {(int64_t)512, (int64_t)2048, (int64_t)3072}) {
              if (u * nc > 40000 && (pat0 > 3 || slots != 2048 || base != 1)) continue;   // (keep the sanitised run short)
              std::vector<int64_t> nbins((size_t)nc);
              std::vector<int> pats((size_t)nc);
              for (int64_t jj = 0; jj < nc; ++jj) {
                // 1 bin; 2 bins; a different number per column; as many bins as rows
                nbins[(size_t)jj] = bsel == 0 ? 1 : (bsel == 1 ? 2 : (bsel == 2 ? 1 + (jj * 7 + 2) % 5 : std::max<int64_t>(u, 1)));
                pats[(size_t)jj] = pat0 >= 6 ? (jj == nc / 2 ? pat0 : 2) : (int)((pat0 + jj) % 6);
              }
              check_case(u, nbins, pats, base, slots, /*slot_cap=*/(64ll << 20) / (8 * 64 * base));
            }
  // a column with more bins than a launch's budget goes alone; the columns around it share launches
  {
    const int64_t u = 5000;
    std::vector<int64_t> nbins = {3, 5000, 2, 4000, 200};
    std::vector<int> pats = {3, 2, 3, 2, 3};
    check_case(u, nbins, pats, 3, 2048, 1000);
  }
  // no slot for partial sums: nothing may be cut
  {
    std::vector<int64_t> nbins(5, 2);
    std::vector<int> pats(5, 3);
    const long long cut = check_case(4099, nbins, pats, 1, 2048, 0);
    REQUIRE(cut == 0, "bins cut without a slot");
  }
  // the long-bin shape of the GPU test: u = 4099 loop rows, v = 17 (one stationary tile), 5 columns of 2 bins
  {
    std::vector<int64_t> nbins(5, 2);
    std::vector<int> pats(5, 3);
    long long cut = 0;
    for (int64_t slots : {(int64_t)2048, (int64_t)3072}) {
      cut = check_case(4099, nbins, pats, 1, slots, (64ll << 20) / (8 * 17));
      REQUIRE(cut >= 1, "the long bins are not cut (slots %lld)", (long long)slots);
    }
    std::printf("binplan_check: u=4099 v=17 cols=5 bins=2: %lld bins cut into several segments\n", cut);
  }
  std::printf("binplan_check: %lld plans, %lld with cut bins, %lld of several launches, %lld refused for a label, %lld empty bins\n",
              g_plans, g_cut_plans, g_multi_launch, g_bad, g_empty_bins);
  REQUIRE(g_cut_plans > 0 && g_multi_launch > 0 && g_bad > 0 && g_empty_bins > 0, "the grid misses a kind of plan");
  if (g_failures) {
    std::printf("binplan_check: %lld FAILURES\n", g_failures);
    return 1;
  }
  std::printf("binplan_check: ok\n");
  return 0;
}
