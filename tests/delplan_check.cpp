// Stand-alone check of the host plan of the deletion residuals (plan_deletion, bigkrls_amd/csrc/delplan.h), built and
// run by tests/test_delplan_cpu.py with -fsanitize=address,undefined.
//
//   delplan_check            check the invariants of every plan of the grid below against brute force
//
// What deletion_residuals and its kernels rely on: `rows` is the stable order of the labels, a permutation of 0 .. n - 1
// with the rows of a unit in their original order; every unit's size is its count; its class follows from its size and
// the route alone; every non-empty unit is in exactly one list, the list of its class, in label order, with its first
// sorted row and its size; the lists' offsets in the upload are 8-byte aligned, do not overlap and end at index_bytes; the
// workspace of the general route covers its largest unit; a unit over the cap is reported and nothing is sized; the
// first label out of range is reported by row.
#include "delplan.h"

#include <cstdarg>
#include <cstdio>
#include <numeric>

namespace {

long long g_failures = 0, g_plans = 0, g_units = 0, g_empty = 0, g_bad = 0, g_over = 0;

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

uint64_t g_rng = 88172645463325252ull;
uint64_t next_random() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return g_rng;
}

// labels with the given unit sizes, grouped (identity order) or shuffled
std::vector<int64_t> labels_of(const std::vector<int64_t>& sizes, bool shuffled) {
  std::vector<int64_t> lab;
  for (size_t g = 0; g < sizes.size(); ++g) lab.insert(lab.end(), (size_t)sizes[g], (int64_t)g);
  if (shuffled)
    for (size_t i = lab.size(); i > 1; --i) std::swap(lab[i - 1], lab[(size_t)(next_random() % i)]);
  return lab;
}

int brute_class(int64_t m, int route) {
  if (m == 0) return -1;
  if (m == 1) return bk::DEL_SINGLE;
  if (route == 1) return bk::DEL_GENERAL;
  if (m <= 16) return bk::DEL_WAVE;
  if (m <= 64) return bk::DEL_MID;
  if (m <= bk::DEL_MB) return bk::DEL_BLOCK;
  if (m <= bk::DEL_WIDE_MB) return bk::DEL_WIDE;
  return bk::DEL_GENERAL;
}

void check_case(const std::vector<int64_t>& lab, int64_t G, int64_t k, int route, const char* what) {
  const int64_t n = (int64_t)lab.size();
  const bk::DelPlan pl = bk::plan_deletion(lab.data(), n, G, k, route);
  ++g_plans;
  // the first label out of range, by brute force
  int64_t bad = -1;
  for (int64_t i = 0; i < n && bad < 0; ++i)
    if (lab[(size_t)i] < 0 || lab[(size_t)i] >= G) bad = i;
  REQUIRE(pl.bad == bad, "%s: bad row %lld, expected %lld", what, (long long)pl.bad, (long long)bad);
  if (bad >= 0) {
    ++g_bad;
    return;
  }
  // the stable order: unit after unit, original order inside
  std::vector<std::vector<int32_t>> members((size_t)G);
  for (int64_t i = 0; i < n; ++i) members[(size_t)lab[(size_t)i]].push_back((int32_t)i);
  REQUIRE((int64_t)pl.rows.size() == n && (int64_t)pl.off.size() == G + 1 && (int64_t)pl.size.size() == G &&
              (int64_t)pl.cls.size() == G, "%s: sizes of the plan's arrays", what);
  if ((int64_t)pl.rows.size() != n || (int64_t)pl.off.size() != G + 1) return;
  std::vector<char> seen((size_t)n, 0);
  int64_t at = 0, max_general = 0, over_unit = -1;
  double sum_m2 = 0.0;
  size_t next[bk::DEL_CLASSES] = {0, 0, 0, 0, 0, 0};
  const int64_t cap_rows = bk::del_cap_rows();
  REQUIRE(8 * cap_rows * cap_rows <= bk::DEL_CAP_BYTES && 8 * (cap_rows + 1) * (cap_rows + 1) > bk::DEL_CAP_BYTES,
          "%s: cap rows %lld", what, (long long)cap_rows);
  for (int64_t g = 0; g < G; ++g) {
    const std::vector<int32_t>& mem = members[(size_t)g];
    const int64_t m = (int64_t)mem.size();
    REQUIRE(pl.off[(size_t)g] == at && pl.off[(size_t)g + 1] == at + m, "%s: offsets of unit %lld", what, (long long)g);
    REQUIRE(pl.size[(size_t)g] == m, "%s: size of unit %lld", what, (long long)g);
    for (int64_t r = 0; r < m; ++r) {
      const int32_t row = pl.rows[(size_t)(at + r)];
      REQUIRE(row == mem[(size_t)r], "%s: unit %lld position %lld holds row %d, expected %d", what, (long long)g,
              (long long)r, row, mem[(size_t)r]);
      if (row >= 0 && row < n) {
        REQUIRE(!seen[(size_t)row], "%s: row %d listed twice", what, row);
        seen[(size_t)row] = 1;
      }
    }
    const int c = brute_class(m, route);
    REQUIRE(pl.cls[(size_t)g] == c, "%s: class of unit %lld (m = %lld) is %d, expected %d", what, (long long)g,
            (long long)m, (int)pl.cls[(size_t)g], c);
    sum_m2 += (double)m * (double)m;
    ++g_units;
    if (c < 0) {
      ++g_empty;
    } else {
      const std::vector<bk::DelUnit>& list = pl.list[c];
      REQUIRE(next[c] < list.size(), "%s: unit %lld is missing from the list of class %d", what, (long long)g, c);
      if (next[c] < list.size()) {
        const bk::DelUnit& un = list[next[c]++];
        REQUIRE(un.unit == g && un.first == at && un.m == m, "%s: list entry of unit %lld: (%d, %d, %d)", what,
                (long long)g, un.unit, un.first, un.m);
      }
      if (c == bk::DEL_GENERAL) {
        max_general = std::max(max_general, m);
        if (m > cap_rows && over_unit < 0) over_unit = g;
      }
    }
    at += m;
  }
  REQUIRE(at == n, "%s: the units hold %lld rows of %lld", what, (long long)at, (long long)n);
  for (int64_t i = 0; i < n; ++i) REQUIRE(seen[(size_t)i], "%s: row %lld is not listed", what, (long long)i);
  for (int c = 0; c < bk::DEL_CLASSES; ++c)
    REQUIRE(next[c] == pl.list[c].size(), "%s: the list of class %d has %zu entries, %zu units belong there", what, c,
            pl.list[c].size(), next[c]);
  REQUIRE(pl.sum_m2 == sum_m2, "%s: sum of m^2", what);
  REQUIRE(pl.max_general_m == max_general, "%s: largest general unit %lld, expected %lld", what,
          (long long)pl.max_general_m, (long long)max_general);
  REQUIRE(pl.over_unit == over_unit, "%s: unit over the cap %lld, expected %lld", what, (long long)pl.over_unit,
          (long long)over_unit);
  if (over_unit >= 0) {
    ++g_over;
    REQUIRE(pl.over_m == (int64_t)members[(size_t)over_unit].size() && pl.general_doubles == 0,
            "%s: a plan over the cap sizes nothing", what);
  } else if (max_general > 0) {
    REQUIRE(pl.general_doubles == 2 * max_general * k + 2 * max_general * max_general + 4 * max_general,
            "%s: workspace of the general route", what);
  } else {
    REQUIRE(pl.general_doubles == 0, "%s: no general unit, no workspace", what);
  }
  REQUIRE(pl.wide_doubles == std::min<int64_t>((int64_t)pl.list[bk::DEL_WIDE].size(), bk::DEL_WIDE_BATCH) * bk::DEL_WIDE_MB *
                                 (bk::DEL_WIDE_MB + 1), "%s: workspace of the wide instance", what);
  // the upload: rows, then the lists, each 8-byte aligned
  int64_t b = (n * 4 + 7) / 8 * 8;
  for (int c = 0; c < bk::DEL_CLASSES; ++c) {
    REQUIRE(pl.list_off[c] == b && b % 8 == 0, "%s: offset of list %d", what, c);
    b += ((int64_t)pl.list[c].size() * 12 + 7) / 8 * 8;
  }
  REQUIRE(pl.index_bytes == b, "%s: index bytes", what);
}

}  // namespace

int main() {
  const int MB = bk::DEL_MB;
  static_assert(bk::DEL_WIDE_MB == 2 * bk::DEL_MB, "the grid below puts the wide instance's limit at 2 MB");
  // sizes 1 .. 2 MB + 1, one unit of each, grouped and shuffled, both routes
  {
    std::vector<int64_t> sizes;
    for (int64_t m = 1; m <= 2 * MB + 1; ++m) sizes.push_back(m);
    for (int route = 0; route < 2; ++route)
      for (int sh = 0; sh < 2; ++sh)
        check_case(labels_of(sizes, sh != 0), (int64_t)sizes.size(), 7, route, sh ? "sizes 1..2MB+1 shuffled" : "sizes 1..2MB+1 grouped");
    // ... and descending, so that the identity test sees labels that are grouped but the sizes fall
    std::vector<int64_t> rev(sizes.rbegin(), sizes.rend());
    check_case(labels_of(rev, false), (int64_t)rev.size(), 7, 0, "sizes 2MB+1..1 grouped");
  }
  // empty units: at the start, in the middle, at the end, several in a row
  for (int sh = 0; sh < 2; ++sh)
    for (int route = 0; route < 2; ++route) {
      check_case(labels_of({0, 3, 0, 0, 17, 1, 0, 130, 0}, sh != 0), 9, 5, route, "empty units");
      check_case(labels_of({2, 0}, sh != 0), 2, 1, route, "last unit empty");
      check_case(labels_of({0, 2}, sh != 0), 2, 1, route, "first unit empty");
    }
  // all rows in one unit, of every class
  for (int64_t m : {1, 2, 16, 17, 64, 65, MB, MB + 1, 2 * MB, 2 * MB + 1, 1000})
    for (int route = 0; route < 2; ++route) check_case(labels_of({m}, false), 1, 250, route, "one unit");
  // G = n: identity labels and a permutation
  for (int64_t n : {1, 2, 63, 64, 65, 1000})
    for (int sh = 0; sh < 2; ++sh) check_case(labels_of(std::vector<int64_t>((size_t)n, 1), sh != 0), n, 3, 0, "G = n");
  // the class boundaries in one plan, many units each
  for (int sh = 0; sh < 2; ++sh) {
    std::vector<int64_t> sizes;
    for (int rep = 0; rep < 5; ++rep)
      for (int64_t m : {15, 16, 17, 63, 64, 65, MB - 1, MB, MB + 1, 2 * MB - 1, 2 * MB, 2 * MB + 1, 1, 2, 0}) sizes.push_back(m);
    for (int route = 0; route < 2; ++route) check_case(labels_of(sizes, sh != 0), (int64_t)sizes.size(), 33, route, "class boundaries");
  }
  // more wide units than one launch takes
  check_case(labels_of(std::vector<int64_t>(300, 129), false), 300, 4, 0, "300 wide units");
  // random sizes 1 .. 250
  for (int rep = 0; rep < 4; ++rep) {
    std::vector<int64_t> sizes;
    for (int g = 0; g < 200; ++g) sizes.push_back((int64_t)(next_random() % 250) + 1);
    check_case(labels_of(sizes, rep % 2 != 0), 200, 250, 0, "random sizes");
  }
  // a unit over the cap of the general route: refused by the plan, nothing sized
  {
    const int64_t cap = bk::del_cap_rows();
    check_case(labels_of({3, cap + 1, 2}, false), 3, 1, 0, "one unit over the cap");
    check_case(labels_of({3, cap + 1, cap + 2}, true), 3, 1, 1, "two units over the cap");
    check_case(labels_of({cap, 2}, false), 2, 1, 0, "a unit at the cap");
  }
  // a label out of range: below and above, first and last row, grouped and not
  {
    std::vector<int64_t> lab = labels_of({5, 5, 5}, false);
    lab[7] = 3;
    check_case(lab, 3, 2, 0, "label G in the middle");
    lab[7] = 1;
    lab[14] = -1;
    check_case(lab, 3, 2, 0, "label -1 in the last row");
    lab[14] = 2;
    lab[0] = -5;
    check_case(lab, 3, 2, 0, "negative label in the first row");
    lab = labels_of({5, 5, 5}, true);
    lab[3] = 99;
    lab[9] = -1;
    check_case(lab, 3, 2, 1, "two labels out of range, shuffled");
  }
  std::printf("plans %lld, units %lld (%lld empty), refused for a label %lld, over the cap %lld\n", g_plans, g_units,
              g_empty, g_bad, g_over);
  if (g_failures) {
    std::printf("delplan_check: %lld FAILURES\n", g_failures);
    return 1;
  }
  std::printf("delplan_check: ok\n");
  return 0;
}
