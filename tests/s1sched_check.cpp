// Stand-alone check of bigkrls_amd/csrc/s1sched.h (the schedule of stage 1 of the dense eigensolver) against a literal
// transcription of the predicates stage1_to_band, S1Ops and dist_s1_group_size held while the loop was one function:
// has_panel, resident_qr, agg_ok, quad_ok, the pair loop's condition, the swap condition, the J1 / c1 arithmetic and the
// distributed group size. Every panel of every n from 257 to 24 000 must agree, over BIGKRLS_S1AGG unset / 0 / 2, the
// default thresholds and (9 000, 9 600), 80 and 40 co-resident workgroups, per-column launches off and on, and the
// look-ahead stream its own or the main one. Then the arm counts of the GPU cases of tests/_stage1_cases.py are printed
// (tests/test_s1sched_cpu.py compares them with that file's table) and each case must reach the arms it is there for.
// No HIP; builds with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "s1sched.h"

namespace ref {   // the former code, names and arithmetic unchanged
constexpr int S2_B = 64;
constexpr int S1_AGG_MIN_M = 10752;
constexpr int S1_SWAP_M = 6144;
constexpr int S1_QUAD_MIN_M = 12800;

struct Loop {
  int n;
  int pq_cap;
  bool pq_steps, fused_panel, side_is_main;
  bool have_agg_ws;          // ws.aggPZ1[0] != nullptr
  const char* agg_env;       // getenv("BIGKRLS_S1AGG")
  const char* am;            // getenv("BIGKRLS_S1AGG_MIN")
  const char* qm;            // getenv("BIGKRLS_S1AGG4_MIN")
  int swap_m;

  bool resident_qr(int k) const { return !pq_steps && (n - k - S2_B + 255) / 256 <= std::min(pq_cap, 80); }
  bool has_panel(int k) const { return k + S2_B < n && n - k - S2_B > 1; }

  struct Step { int k, arm, j, c1; };   // arm: 0 quad, 1 pair, 2 two-stream, 3 one-stream, 4 last; c1 after a pair's half 1
  void run(std::vector<Step>& out) const {
    out.clear();
    const int b = S2_B;
    int k0 = 0;
    {
      int AGG_MIN_M = S1_AGG_MIN_M;
      if (am) AGG_MIN_M = std::max(4 * S2_B, atoi(am));
      const bool agg_on = have_agg_ws && fused_panel && !(agg_env && std::string(agg_env) == "0");
      auto agg_ok = [&](int kk) {
        return agg_on && has_panel(kk) && has_panel(kk + b) && resident_qr(kk) && resident_qr(kk + b) &&
               n - kk - b >= AGG_MIN_M;
      };
      int k = 0;
      int c1 = 0;
      if (agg_on && !(agg_env && std::string(agg_env) == "2")) {
        int Q_MIN_M = S1_QUAD_MIN_M;
        if (qm) Q_MIN_M = std::max(AGG_MIN_M, atoi(qm));
        auto quad_ok = [&](int kk) {
          return agg_ok(kk) && agg_ok(kk + b) && agg_ok(kk + 2 * b) && agg_ok(kk + 3 * b) && n - kk - 4 * b >= Q_MIN_M;
        };
        while (quad_ok(k)) {
          for (int j = 0; j < 4; ++j, k += b) out.push_back({k, 0, j, 0});
        }
      }
      while (agg_ok(k) && agg_ok(k + b)) {
        for (int half = 0; half < 2; ++half, k += b) {
          const int m = n - k - b;
          const int mn = m - b;
          if (half == 1) {
            const int ncol64 = (mn + 63) / 64;
            const int J1 = std::min(std::max((int)(ncol64 * 0.2929 + 0.5), 1), ncol64 - 1);
            c1 = (k + 2 * b) + 64 * J1;
          }
          out.push_back({k, 1, half, half == 1 ? c1 : 0});
        }
      }
      k0 = k;
    }
    for (int k = k0; has_panel(k); k += b) {
      const int m = n - k - b;
      const int pw = b;
      const bool panel_in_z = fused_panel && has_panel(k + b) && resident_qr(k + b);
      if (has_panel(k + b) && panel_in_z && m - pw < swap_m && !side_is_main) out.push_back({k, 3, 0, 0});
      else if (has_panel(k + b)) out.push_back({k, 2, 0, 0});
      else out.push_back({k, 4, 0, 0});
    }
  }
};

inline int dist_s1_group_size(int n, int k0, int agg_mode) {
  if (agg_mode == 0) return 0;
  const int env = agg_mode == 2 ? 2 : -1;
  const int b = S2_B;
  auto has_panel = [&](int k) { return k + S2_B < n && n - k - S2_B > 1; };
  auto panels = [&](int g) {
    for (int j = 0; j < g; ++j)
      if (!has_panel((int)(k0 + j * b))) return false;
    return true;
  };
  if (env != 2 && panels(4) && n - k0 - 4 * b >= S1_QUAD_MIN_M) return 4;
  if (panels(2) && n - k0 - 2 * b >= S1_AGG_MIN_M) return 2;
  return 0;
}
}  // namespace ref

static int arm_code(bk::S1Arm a) {
  switch (a) {
    case bk::S1Arm::Quad: return 0;
    case bk::S1Arm::Pair: return 1;
    case bk::S1Arm::TwoStream: return 2;
    case bk::S1Arm::OneStream: return 3;
    default: return 4;
  }
}

// the S1Sched the library would build from the same settings (Stage1::init)
static bk::S1Sched sched_of(const ref::Loop& r) {
  bk::S1Sched s;
  s.n = r.n;
  if (r.am) s.agg_min = std::max(4 * bk::S1_B, atoi(r.am));
  if (r.qm) s.quad_min = std::max(s.agg_min, atoi(r.qm));
  s.swap_m = r.swap_m;
  s.agg_mode = r.agg_env && std::string(r.agg_env) == "0" ? 0 : r.agg_env && std::string(r.agg_env) == "2" ? 2 : -1;
  s.agg_ws = r.have_agg_ws;
  s.fused_panel = r.fused_panel;
  s.cap = r.pq_cap;
  s.pq_steps = r.pq_steps;
  s.side_is_main = r.side_is_main;
  return s;
}

static long long failures = 0;
static void fail(const ref::Loop& r, int k, const char* what) {
  if (++failures <= 20)
    std::printf("s1sched_check: n=%d k=%d S1AGG=%s AGG_MIN=%s cap=%d steps=%d side_is_main=%d: %s differs\n", r.n, k,
                r.agg_env ? r.agg_env : "unset", r.am ? r.am : "default", r.pq_cap, (int)r.pq_steps, (int)r.side_is_main, what);
}

static long long compare(const ref::Loop& r) {
  const bk::S1Sched s = sched_of(r);
  static std::vector<ref::Loop::Step> want;   // (reused: one allocation for the whole grid)
  r.run(want);
  size_t i = 0;
  s.walk([&](int k, bk::S1Step st) {
    if (i >= want.size()) { fail(r, k, "number of panels"); ++i; return; }
    const ref::Loop::Step& w = want[i++];
    if (w.k != k || w.arm != arm_code(st.arm) || w.j != st.j) fail(r, k, "arm");
    if (w.arm == 1 && w.j == 1) {
      const int c1 = bk::s1_piece_c1(k + 2 * bk::S1_B, r.n - k - 2 * bk::S1_B);
      // the three sites: the cut itself, piece a's first column, piece b's width (next group's half 0, or the hand-over)
      if (c1 != w.c1 || bk::s1_piece_cols(c1, k + 2 * bk::S1_B) != (w.c1 - (k + 2 * 64)) / 64 ||
          bk::s1_piece_cols(c1, k + 3 * bk::S1_B) != (w.c1 - (k + 3 * 64)) / 64)
        fail(r, k, "c1");
    }
  });
  if (i != want.size()) fail(r, -1, "number of panels");
  // the plain predicates at every block column, panels or not
  for (int k = 0; k <= r.n + 64; k += 64)
    if (s.has_panel(k) != r.has_panel(k) || s.resident_qr(k) != r.resident_qr(k)) fail(r, k, "has_panel / resident_qr");
  return (long long)want.size();
}

struct GpuCase {
  const char* name;
  int n;
  const char* agg_env; const char* am; const char* qm;
  bool pq_steps, fused_panel;
  int swap_m;
  bool want_quads, want_pairs, want_two, want_one;   // the arms the case is there for
};

int main() {
  const char* modes[3] = {nullptr, "0", "2"};
  long long panels = 0;
  for (int n = 257; n <= 24000; ++n)
    for (const char* mode : modes)
      for (int thr = 0; thr < 2; ++thr)
        for (int cap : {80, 40})
          for (int steps = 0; steps < 2; ++steps)
            for (int sim = 0; sim < 2; ++sim) {
              ref::Loop r{n, cap, steps != 0, true, sim != 0, n >= ref::S1_AGG_MIN_M + 4 * ref::S2_B, mode,
                          thr ? "9000" : nullptr, thr ? "9600" : nullptr, ref::S1_SWAP_M};
              panels += compare(r);
            }
  // the switches the grid above leaves at their defaults: no fused panel update; other swap heights
  for (int n = 257; n <= 24000; n += 7)
    for (int fused = 0; fused < 2; ++fused)
      for (int swap_m : {0, 3000, 6144}) {
        ref::Loop r{n, 80, false, fused != 0, false, n >= ref::S1_AGG_MIN_M + 4 * ref::S2_B, nullptr, nullptr, nullptr, swap_m};
        panels += compare(r);
      }
  long long groups = 0;
  for (int n = 257; n <= 24000; ++n)
    for (int mode : {0, 2, 4})
      for (int k0 = 0; k0 <= n; k0 += 64, ++groups)
        if (bk::s1_dist_group_size(n, k0, mode) != ref::dist_s1_group_size(n, k0, mode)) {
          if (++failures <= 20) std::printf("s1sched_check: n=%d k0=%d mode=%d: distributed group size differs\n", n, k0, mode);
        }
  std::printf("s1sched_check: %lld panels, %lld distributed group starts compared\n", panels, groups);

  const GpuCase cases[] = {
      {"n1100", 1100, nullptr, nullptr, nullptr, false, true, 6144, false, false, false, true},
      {"n1100_pq_steps", 1100, nullptr, nullptr, nullptr, true, true, 6144, false, false, true, false},
      {"n1100_pq_householder", 1100, nullptr, nullptr, nullptr, false, true, 6144, false, false, false, true},
      {"n1100_pq_fused", 1100, nullptr, nullptr, nullptr, false, true, 6144, false, false, false, true},
      {"n1100_s1_gemm", 1100, nullptr, nullptr, nullptr, false, false, 6144, false, false, true, false},
      {"n1100_s1_nopanel", 1100, nullptr, nullptr, nullptr, false, false, 6144, false, false, true, false},
      {"n1100_tpq0", 1100, nullptr, nullptr, nullptr, false, true, 6144, false, false, false, true},
      {"n2100_p2", 2100, nullptr, nullptr, nullptr, false, true, 6144, false, false, false, true},
      {"n2100_p2_tpq0", 2100, nullptr, nullptr, nullptr, false, true, 6144, false, false, false, true},
      {"n7000", 7000, nullptr, nullptr, nullptr, false, true, 6144, false, false, true, true},
      {"n13150", 13150, nullptr, nullptr, nullptr, false, true, 6144, true, true, true, true},
      {"n11300", 11300, nullptr, nullptr, nullptr, false, true, 6144, false, true, true, true},
      {"n11300_agg0", 11300, "0", nullptr, nullptr, false, true, 6144, false, false, true, true},
      {"n11300_agg2", 11300, "2", nullptr, nullptr, false, true, 6144, false, true, true, true},
      {"n11300_low_thresholds", 11300, nullptr, "9000", "9600", false, true, 6144, true, true, true, true},
      {"n1100_swap0", 1100, nullptr, nullptr, nullptr, false, true, 0, false, false, true, false},
  };
  for (const GpuCase& c : cases) {
    ref::Loop r{c.n, 80, c.pq_steps, c.fused_panel, false, c.n >= ref::S1_AGG_MIN_M + 4 * ref::S2_B, c.agg_env, c.am, c.qm, c.swap_m};
    const bk::S1Counts k = sched_of(r).counts();
    std::printf("case %s: %d %d %d %d\n", c.name, k.quads, k.pairs, k.two_stream, k.one_stream);
    if ((k.quads > 0) != c.want_quads || (k.pairs > 0) != c.want_pairs || (k.two_stream > 0) != c.want_two ||
        (k.one_stream > 0) != c.want_one || k.last != 1) {
      std::printf("s1sched_check: case %s does not reach the arms it is there for\n", c.name);
      ++failures;
    }
    if (c.n % 64 == 0) { std::printf("s1sched_check: case %s has no ragged last panel\n", c.name); ++failures; }
  }
  // n = 13 150: one group of four, then 16 pair groups; n = 11 300 with the low thresholds: several groups of four
  {
    ref::Loop a{13150, 80, false, true, false, true, nullptr, nullptr, nullptr, ref::S1_SWAP_M};
    ref::Loop l{11300, 80, false, true, false, true, nullptr, "9000", "9600", ref::S1_SWAP_M};
    const bk::S1Counts ka = sched_of(a).counts(), kl = sched_of(l).counts();
    if (ka.quads != 1 || ka.pairs != 16 || kl.quads < 2) { std::printf("s1sched_check: group counts of the GPU cases\n"); ++failures; }
  }
  if (failures == 0) std::printf("s1sched_check: ok\n");
  else std::printf("s1sched_check: %lld failures\n", failures);
  return failures == 0 ? 0 : 1;
}
