// Stand-alone check of the host plans of the kernel builds and the fused kernel-tile entry points
// (bigkrls_amd/csrc/ktplan.h), built and run by tests/test_ktplan_cpu.py with -fsanitize=address,undefined.
//
//   ktplan_check tests/golden/kt_plans.txt      check: invariants of every plan, then equality with the file row for row
//   ktplan_check --print                        print the rows (to compare two versions of the header by hand)
//
// Two layers. The invariants are what the kernels rely on, checked by enumeration over the grids below (brute force
// beside every plan). The golden rows pin the plans themselves: the file was recorded once, by a scratch program that
// held the statements csrc/gemm.hip had before they moved into ktplan.h, verbatim, behind this header's interface.
// A row holds the case and every scalar of its plan; tables (off, perm, segments, multi, the kernel-argument structs,
// the band table) enter as a 32-bit FNV-1a checksum of their integers, in order. The 16 128 cases of kb_plan are folded
// to one row per shape: the plan under the default switches in full, all 18 switch settings in one 64-bit checksum.
#include "ktplan.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>

namespace {

std::FILE* g_golden = nullptr;   // null: print
long long g_rows = 0, g_failures = 0, g_split_rows = 0, g_multi_launch_rows = 0, g_tiled_rows = 0, g_perm_rows = 0, g_kb_cases = 0;

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

struct Fnv {
  uint32_t h = 2166136261u;
  void add(int64_t v) {
    for (int b = 0; b < 8; ++b) { h ^= (uint32_t)((uint64_t)v >> (8 * b)) & 0xffu; h *= 16777619u; }
  }
  template <class It> Fnv& range(It a, It b) { for (; a != b; ++a) add((int64_t)*a); return *this; }
};
template <class V> uint32_t fnv(const V& v) { return Fnv().range(v.begin(), v.end()).h; }

std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  std::vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

void emit(const std::string& row) {
  ++g_rows;
  if (!g_golden) { std::printf("%s\n", row.c_str()); return; }
  char line[1024];
  do {
    if (!std::fgets(line, sizeof line, g_golden)) { fail("the golden file ends before row %lld: %s", g_rows, row.c_str()); return; }
  } while (line[0] == '#' || line[0] == '\n');
  line[std::strcspn(line, "\n")] = 0;
  REQUIRE(row == line, "row %lld: got    %s\n          golden %s", g_rows, row.c_str(), line);
}

// ---- group_order ---------------------------------------------------------------------------------------------------
// patterns 0..5: sorted, reversed, interleaved, an empty group first / in the middle / last (sorted); 6..17: a bad label
// (G or -1) at the first, a middle or the last row of sorted (6..11) or interleaved (12..17) labels
bool make_labels(int64_t n, int64_t G, int pat, std::vector<int64_t>& lab) {
  lab.resize((size_t)n);
  auto sorted_over = [&](int64_t skip) {   // sorted labels that leave group `skip` empty
    const int64_t used = G - 1;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t g = i * used / n;
      lab[(size_t)i] = g >= skip ? g + 1 : g;
    }
  };
  if (pat == 0) for (int64_t i = 0; i < n; ++i) lab[(size_t)i] = i * G / n;
  else if (pat == 1) for (int64_t i = 0; i < n; ++i) lab[(size_t)i] = G - 1 - i * G / n;
  else if (pat == 2) for (int64_t i = 0; i < n; ++i) lab[(size_t)i] = i % G;
  else if (pat <= 5) {
    if (G < 2 || (pat == 4 && G < 3)) return false;
    sorted_over(pat == 3 ? 0 : (pat == 4 ? G / 2 : G - 1));
  } else {
    const int k = pat - 6;
    make_labels(n, G, k < 6 ? 0 : 2, lab);
    const int64_t pos = (k % 3 == 0) ? 0 : (k % 3 == 1 ? n / 2 : n - 1);
    lab[(size_t)pos] = (k % 6) < 3 ? G : -1;
  }
  return true;
}

void check_group_order() {
  const int64_t ns[] = {1, 2, 17, 64, 65};
  std::vector<int64_t> lab;
  for (int64_t n : ns)
    for (int64_t G : {(int64_t)1, (int64_t)2, (int64_t)5, n})
      for (int pat = 0; pat < 18; ++pat) {
        if (!make_labels(n, G, pat, lab)) continue;
        const bk::GroupOrder o = bk::group_order(lab.data(), n, G);
        int64_t bad = -1;
        bool nondecreasing = true;
        for (int64_t i = 0; i < n; ++i) {
          if (bad < 0 && (lab[(size_t)i] < 0 || lab[(size_t)i] >= G)) bad = i;
          if (i > 0 && lab[(size_t)i] < lab[(size_t)i - 1]) nondecreasing = false;
        }
        REQUIRE(o.bad == bad, "group_order n=%lld G=%lld pattern %d: first bad row %lld, expected %lld", (long long)n,
                (long long)G, pat, (long long)o.bad, (long long)bad);
        if (bad >= 0) {
          emit(fmt("group_order %lld %lld %d bad %lld", (long long)n, (long long)G, pat, (long long)o.bad));
          continue;
        }
        // brute force: a stable sort of the row numbers by label
        std::vector<int32_t> ref((size_t)n);
        std::iota(ref.begin(), ref.end(), 0);
        std::stable_sort(ref.begin(), ref.end(), [&](int32_t a, int32_t b) { return lab[(size_t)a] < lab[(size_t)b]; });
        bool ref_identity = true;   // cluster_scores' former test: every row stays where it is
        for (int64_t r = 0; r < n; ++r) ref_identity = ref_identity && ref[(size_t)r] == r;
        REQUIRE(ref_identity == nondecreasing, "identity <=> non-decreasing fails at n=%lld G=%lld pattern %d", (long long)n,
                (long long)G, pat);
        REQUIRE(o.perm.empty() == nondecreasing, "group_order n=%lld G=%lld pattern %d: perm must be empty exactly for labels that never decrease",
                (long long)n, (long long)G, pat);
        REQUIRE(o.perm.empty() || o.perm == ref, "group_order n=%lld G=%lld pattern %d: perm is not the stable order", (long long)n,
                (long long)G, pat);
        bool off_ok = (int64_t)o.off.size() == G + 1 && o.off[0] == 0 && o.off[(size_t)G] == n;
        for (int64_t g = 0; off_ok && g < G; ++g) {
          off_ok = o.off[(size_t)g] <= o.off[(size_t)g + 1];
          for (int64_t r = o.off[(size_t)g]; off_ok && r < o.off[(size_t)g + 1]; ++r) off_ok = lab[(size_t)ref[(size_t)r]] == g;
        }
        REQUIRE(off_ok, "group_order n=%lld G=%lld pattern %d: offsets", (long long)n, (long long)G, pat);
        g_perm_rows += !o.perm.empty();
        emit(fmt("group_order %lld %lld %d ok perm %d off %08x perm %08x", (long long)n, (long long)G, pat, (int)!o.perm.empty(),
                 fnv(o.off), fnv(o.perm)));
      }
}

// ---- plan_grouped_segments -----------------------------------------------------------------------------------------
void check_grouped_segments() {
  std::vector<std::vector<int64_t>> sizes = {{4099, 17}, {1090, 0, 10}, std::vector<int64_t>(200, 2), {}, {16 * 16 * 64 + 5},
                                              {4099}, {1090}};
  for (int g = 0; g < 40; ++g) sizes[3].push_back(g % 6 == 0 ? 100 + 37 * g : 0);   // 7 of 40 groups hold rows
  long long split_rows = 0;
  for (size_t c = 0; c < sizes.size(); ++c) {
    const int64_t G = (int64_t)sizes[c].size();
    std::vector<int64_t> off((size_t)G + 1, 0);
    for (int64_t g = 0; g < G; ++g) off[(size_t)g + 1] = off[(size_t)g] + sizes[c][(size_t)g];
    for (int64_t slots : {1, 512, 2048, 3072})
      for (int64_t base : {1, 2, 10, 313})
        for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)5, (int64_t)1 << 20}) {
          const bk::GroupedPlan pl = bk::plan_grouped_segments(off.data(), G, base, slots, cap);
          const std::string where = fmt("plan_grouped_segments case %zu slots=%lld base=%lld cap=%lld", c, (long long)slots,
                                        (long long)base, (long long)cap);
          size_t si = 0, mi = 0;
          int64_t next_slot = 0;
          bool ok = pl.nsplit >= 1 && pl.nsplit <= 64 && pl.multi.size() % 3 == 0;
          for (int64_t g = 0; ok && g < G; ++g) {
            const int64_t b = off[(size_t)g], t = off[(size_t)g + 1];
            size_t s1 = si;
            while (s1 < pl.segs.size() && pl.segs[s1].group == g) ++s1;
            const int64_t cnt = (int64_t)(s1 - si);
            if (b == t || cnt > 1) {   // the group's multi entry: empty groups (0 segments) and cut ones
              ok = mi + 3 <= pl.multi.size() && pl.multi[mi] == g && pl.multi[mi + 2] == cnt &&
                   pl.multi[mi + 1] == (cnt > 1 ? next_slot : 0);
              mi += 3;
            }
            if (b == t) { ok = ok && cnt == 0; continue; }
            ok = ok && cnt >= 1 && cnt <= 64 && pl.segs[si].l_begin == b && pl.segs[s1 - 1].l_end == t;
            for (size_t s = si; ok && s < s1; ++s) {
              const bk::KcgSeg& sg = pl.segs[s];
              ok = sg.l_begin < sg.l_end && (sg.l_begin - b) % 16 == 0 && (s + 1 == s1 || pl.segs[s + 1].l_begin == sg.l_end) &&
                   sg.slot == (cnt > 1 ? next_slot++ : -1) && (cnt == 1 || (sg.l_end - sg.l_begin + 15) / 16 >= 16);
            }
            si = s1;
          }
          ok = ok && si == pl.segs.size() && mi == pl.multi.size() && next_slot == pl.nslots;
          REQUIRE(ok, "%s: the segments do not tile the groups as they must", where.c_str());
          REQUIRE(pl.nsplit == 1 || pl.nslots <= cap, "%s: %lld slots", where.c_str(), (long long)pl.nslots);
          if (G == 1) {   // plan_loop_splits' rule, cuts included
            const int64_t lt = (off[1] + 15) / 16, bytes = cap > 0 ? (64ll << 20) / cap : (64ll << 20) + 1;
            REQUIRE((64ll << 20) / bytes == cap, "%s: no byte count gives this cap", where.c_str());
            const int64_t s = bk::plan_loop_splits(base, slots, lt, bytes);
            bool same = pl.nsplit == s && (int64_t)pl.segs.size() == s;
            for (int64_t k = 0; same && k < s; ++k)
              same = pl.segs[(size_t)k].l_begin == 16 * (lt * k / s) && pl.segs[(size_t)k].l_end == std::min(16 * (lt * (k + 1) / s), off[1]);
            REQUIRE(same, "%s: differs from plan_loop_splits (%lld splits)", where.c_str(), (long long)s);
          }
          split_rows += pl.nsplit > 1;
          std::vector<int> flat;
          for (const bk::KcgSeg& sg : pl.segs) flat.insert(flat.end(), {sg.l_begin, sg.l_end, sg.group, sg.slot});
          emit(fmt("grouped %zu %lld %lld %lld nsplit %lld nseg %zu nmulti %zu nslots %lld segs %08x multi %08x", c, (long long)slots,
                   (long long)base, (long long)cap, (long long)pl.nsplit, pl.segs.size(), pl.multi.size() / 3,
                   (long long)pl.nslots, fnv(flat), fnv(pl.multi)));
        }
  }
  g_split_rows += split_rows;
  REQUIRE(split_rows > 0, "no grouped plan cuts a group: the grid has shrunk to trivial plans");
}

// ---- plan_loo_moments ----------------------------------------------------------------------------------------------
// tests/_fused_tile_cases.py's loo_entries(p, in_order)
std::vector<int64_t> fused_tile_entries(int64_t p, bool in_order) {
  const int64_t c1 = p - 1, j1 = 1, j2 = p - 2;
  const int64_t ent[9][3] = {{0, 0, 0}, {1, 0, j1}, {2, 0, j2}, {1, 0, j2}, {2, 0, j1}, {0, 1, 0}, {0, c1, 0}, {1, c1, 0}, {2, c1, j1}};
  const int scattered[9] = {6, 0, 5, 2, 7, 1, 8, 3, 4};
  std::vector<int64_t> e;
  for (int i = 0; i < 9; ++i) {
    const int64_t* t = ent[in_order ? i : scattered[i]];
    e.insert(e.end(), t, t + 3);
  }
  return e;
}
// tests/_kt_plan_cases.py's many_entries(): 130 entries over 5 columns, all kinds, in no order
std::vector<int64_t> many_entries() {
  std::vector<int64_t> e;
  for (int64_t i = 0; i < 130; ++i) {
    const int64_t c = (i * 7) % 5;
    e.insert(e.end(), {i % 3, c, (c + 1 + i % 4) % 5});
  }
  return e;
}

void check_loo_moments() {
  struct Case { const char* name; std::vector<int64_t> e; int64_t p; };
  const Case cases[] = {{"fused_p3_in_order", fused_tile_entries(3, true), 3},  {"fused_p3_scattered", fused_tile_entries(3, false), 3},
                        {"fused_p32_in_order", fused_tile_entries(32, true), 32}, {"fused_p32_scattered", fused_tile_entries(32, false), 32},
                        {"trivial_kind0_p1", {0, 0, 0}, 1}, {"trivial_kind2_p2", {2, 0, 1, 0, 1, 1, 2, 1, 0}, 2},
                        {"many_p5", many_entries(), 5}};
  long long multi_launch = 0;
  for (const Case& cs : cases) {
    const int64_t ne = (int64_t)cs.e.size() / 3, cw = bk::ks_of(cs.p) == 8 ? 2 : 3;
    const bk::LooPlan pl = bk::plan_loo_moments(cs.e.data(), ne, cs.p, cw);
    std::vector<int> seen((size_t)ne, 0);
    for (int64_t e : pl.trivial) {
      REQUIRE((cs.e[(size_t)(3 * e)] == 0 && cs.p == 1) || (cs.e[(size_t)(3 * e)] == 2 && cs.p == 2), "%s: entry %lld is not trivial",
              cs.name, (long long)e);
      ++seen[(size_t)e];
    }
    std::string row = fmt("loo_moments %s p %lld cw %lld trivial %zu %08x order %08x launches %zu", cs.name, (long long)cs.p,
                          (long long)cw, pl.trivial.size(), fnv(pl.trivial), fnv(pl.order), pl.launches.size());
    int last_c = -1;
    for (const bk::LooLaunch& ln : pl.launches) {
      const bk::LooMomentEntries& le = ln.le;
      bool ok = ln.nc >= 1 && ln.nc <= bk::KL_GROUP && ln.nchunks >= 1 && ln.nchunks <= ln.nc && le.begin[0] == 0;
      bool consecutive = true;
      for (int64_t i = 0; ok && i < bk::KL_GROUP; ++i) {
        const int64_t s = std::min(i, ln.nc - 1), e = ln.dest.d[i];
        ok = e >= 0 && e < ne && e == ln.dest.d[s] && le.kind[i] == cs.e[(size_t)(3 * e)] && le.c[i] == cs.e[(size_t)(3 * e + 1)] &&
             le.j[i] == (le.kind[i] == 0 ? le.c[i] : cs.e[(size_t)(3 * e + 2)]) && le.c[i] >= last_c;
        if (ok && i < ln.nc) { ++seen[(size_t)e]; last_c = le.c[i]; consecutive = consecutive && e == ln.dest.d[0] + i; }
      }
      int64_t nexp = 0;
      for (int64_t cc = 0; ok && cc < ln.nchunks; ++cc) {
        const int b0 = le.begin[cc], b1 = le.begin[cc + 1];
        ok = b0 < b1 && b1 - b0 <= cw && b1 <= ln.nc;
        bool has01 = false;
        for (int i = b0; ok && i < b1; ++i) {
          ok = le.c[i] == le.c[b0];
          if (le.kind[i] == 2) ++nexp; else has01 = true;
        }
        nexp += has01;
      }
      for (int64_t cc = ln.nchunks; ok && cc <= bk::KL_GROUP; ++cc) ok = le.begin[cc] == ln.nc;
      ok = ok && nexp == ln.nexp && ln.first == ln.dest.d[0] && ln.in_place == consecutive;
      REQUIRE(ok, "%s: a launch of %lld entries breaks the kernel's contract", cs.name, (long long)ln.nc);
      Fnv h;
      h.range(le.c, le.c + bk::KL_GROUP).range(le.j, le.j + bk::KL_GROUP).range(le.kind, le.kind + bk::KL_GROUP).range(le.begin, le.begin + bk::KL_GROUP + 1);
      row += fmt(" | nc %lld nchunks %lld nexp %lld in_place %d first %lld ent %08x dest %08x", (long long)ln.nc, (long long)ln.nchunks,
                 (long long)ln.nexp, (int)ln.in_place, (long long)ln.first, h.h, Fnv().range(ln.dest.d, ln.dest.d + bk::KL_GROUP).h);
    }
    for (int64_t e = 0; e < ne; ++e) REQUIRE(seen[(size_t)e] == 1, "%s: entry %lld appears %d times", cs.name, (long long)e, seen[(size_t)e]);
    multi_launch += pl.launches.size() > 1;
    emit(row);
  }
  g_multi_launch_rows += multi_launch;
  REQUIRE(multi_launch > 0, "no leave-out plan takes more than one launch");
}

// ---- kb_plan -------------------------------------------------------------------------------------------------------
std::string kb_row(int64_t u, int64_t v, int64_t p, int sym, int force, int r_env, int nt_env, const bk::KbPlan& k) {
  std::string row = fmt("kb %lld %lld %lld %d %d %d %d arm %d %d %d %lld %lld %d %d %d", (long long)u, (long long)v, (long long)p, sym,
                        force, r_env, nt_env, k.arm, k.tiles_m, k.tiles_n, (long long)k.ntiles, (long long)k.grid, k.ks, k.band_rows,
                        k.nontemporal);
  const bk::SyrkMap& m = k.map;
  if (k.arm == bk::KB_TILED && sym) {
    row += fmt(" map %d %d %d %d %d %d %d %08x", m.tiles, m.c0, m.c1, m.R, m.nband, m.band0, m.t_off,
               Fnv().range(m.band_start, m.band_start + bk::SYRK_MAX_BANDS + 1).h);
  } else {
    bool zeros = m.tiles == 0 && m.c0 == 0 && m.c1 == 0 && m.R == 0 && m.nband == 0 && m.band0 == 0 && m.t_off == 0;
    for (int b : m.band_start) zeros = zeros && b == 0;
    REQUIRE(zeros, "kb_plan: the map of a launch without one must be zeros");
  }
  return row;
}

// every field of a plan, the map and its band table included
struct Fnv64 {
  uint64_t h = 14695981039346656037ull;
  void add(int64_t v) {
    for (int b = 0; b < 8; ++b) { h ^= ((uint64_t)v >> (8 * b)) & 0xffu; h *= 1099511628211ull; }
  }
  void add(const bk::KbPlan& k) {
    for (int64_t f : {(int64_t)k.arm, (int64_t)k.tiles_m, (int64_t)k.tiles_n, k.ntiles, k.grid, (int64_t)k.ks, (int64_t)k.band_rows,
                      (int64_t)k.nontemporal, (int64_t)k.map.tiles, (int64_t)k.map.c0, (int64_t)k.map.c1, (int64_t)k.map.R,
                      (int64_t)k.map.nband, (int64_t)k.map.band0, (int64_t)k.map.t_off})
      add(f);
    for (int b : k.map.band_start) add((int64_t)b);
  }
};

// One case per shape (u, v, p, sym) and setting of the three switches; one ROW per shape: the plan under the default
// switches (0, 0, -1) in full, and a 64-bit FNV-1a checksum over every field of the shape's 18 plans in the loops' order.
void check_kb_plan() {
  const int64_t uv[] = {1, 31, 32, 33, 1023, 1024, 1153, 50000};
  const int64_t ps[] = {1, 4, 5, 32, 33, 128, 129};
  long long tiled = 0, cases = 0;
  std::vector<char> hit;
  for (int64_t u : uv)
    for (int64_t v : uv)
      for (int64_t p : ps)
        for (int sym = 0; sym < 2; ++sym) {
          Fnv64 all;
          std::string row;
          for (int force : {-1, 0, 1})
            for (int r_env : {0, 7})
              for (int nt_env : {-1, 0, 1}) {
                const bk::KbPlan k = bk::kb_plan(u, v, p, sym != 0, force, r_env, nt_env);
                const bool wave = k.arm == bk::KB_SYM_WAVE || k.arm == bk::KB_WAVE;
                // the wave kernels: the fewest chunks of at most 8 MFMA steps, and the fewest steps per chunk for them
                const int64_t steps = (p + 3) / 4, chunks = (steps + 7) / 8;
                REQUIRE(k.arm >= 0 && k.arm <= 3 && (k.arm != bk::KB_SYM_WAVE || sym) && (wave || k.ks == 0) &&
                        (!wave || (p <= 128 && k.ks >= 1 && k.ks <= 8 && k.ks * chunks >= steps && (k.ks - 1) * chunks < steps)),
                        "kb_plan u=%lld v=%lld p=%lld sym=%d force=%d: arm %d, ks %d", (long long)u, (long long)v, (long long)p, sym, force, k.arm, k.ks);
                REQUIRE(force == 0 || (k.arm == bk::KB_TILED) == (force > 0), "kb_plan: force=%d gives arm %d", force, k.arm);
                if (k.arm == bk::KB_TILED) ++tiled;
                if (k.arm == bk::KB_TILED && sym && k.tiles_m <= 165) {
                  // every workgroup decodes to one lower tile, and every lower tile is taken once
                  hit.assign((size_t)k.tiles_m * k.tiles_m, 0);
                  bool ok = k.ntiles == (int64_t)k.tiles_m * (k.tiles_m + 1) / 2 && k.grid == k.ntiles;
                  for (int bid = 0; ok && bid < (int)k.grid; ++bid) {
                    const bk::SyrkTile t = bk::syrk_map_decode<128>(k.map, bid, (int)k.grid);
                    ok = t.tc >= 0 && t.tc <= t.tm && t.tm < k.tiles_m && t.p == t.tc && !hit[(size_t)t.tm * k.tiles_m + t.tc]++;
                  }
                  REQUIRE(ok, "kb_plan u=%lld p=%lld r_env=%d: the band table does not enumerate the lower tiles", (long long)u,
                          (long long)p, r_env);
                }
                const std::string one = kb_row(u, v, p, sym, force, r_env, nt_env, k);   // (checks the map of the other arms)
                if (force == 0 && r_env == 0 && nt_env == -1) row = one;
                all.add(k);
                ++cases;
              }
          emit(row + fmt(" all18 %016llx", (unsigned long long)all.h));
        }
  // more tile rows than 159 bands of 32: the bands grow
  const int64_t n_big = (int64_t)128 * (159 * 32 + 6);
  const bk::KbPlan k = bk::kb_plan(n_big, n_big, 50, true, 0, 0, -1);
  REQUIRE(k.arm == bk::KB_TILED && k.tiles_m > 159 * 32 && k.map.R > 32 && k.map.nband <= bk::SYRK_MAX_BANDS &&
          k.map.band_start[k.map.nband] == k.ntiles, "kb_plan: the bands of %d tile rows (R = %d, %d bands)", k.tiles_m, k.map.R, k.map.nband);
  emit(kb_row(n_big, n_big, 50, 1, 0, 0, -1, k));
  g_tiled_rows += tiled + 1;
  g_kb_cases += cases + 1;
  REQUIRE(tiled > 0, "no kernel build takes the tiled arm");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: ktplan_check tests/golden/kt_plans.txt | --print\n"); return 2; }
  if (std::strcmp(argv[1], "--print")) {
    g_golden = std::fopen(argv[1], "r");
    if (!g_golden) { std::printf("ktplan_check: cannot open %s\n", argv[1]); return 2; }
  }
  check_group_order();
  check_grouped_segments();
  check_loo_moments();
  check_kb_plan();
  if (!g_golden) return g_failures == 0 ? 0 : 1;
  char line[1024];
  while (std::fgets(line, sizeof line, g_golden))
    if (line[0] != '#' && line[0] != '\n') { fail("the golden file has rows beyond the grid"); break; }
  std::fclose(g_golden);
  REQUIRE(g_perm_rows > 0, "no row orders its rows");
  std::printf("ktplan_check: %lld rows, %lld of them with nsplit > 1, %lld with more than one launch group; %lld kernel-build cases, "
              "%lld of them on the tiled arm\n", g_rows, g_split_rows, g_multi_launch_rows, g_kb_cases, g_tiled_rows);
  if (g_failures == 0) std::printf("ktplan_check: ok\n");
  else std::printf("ktplan_check: %lld failures\n", g_failures);
  return g_failures == 0 ? 0 : 1;
}
