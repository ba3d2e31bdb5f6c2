// The schedule of stage 1 of the dense eigensolver (full matrix to band; Stage1 of csrc/eigen_2stage.inc): which arm of
// the panel loop takes panel k, and where a pair group's update is cut into its two pieces. Host arithmetic only, no
// HIP: a plain host compiler can include this file (tests/s1sched_check.cpp compares it, panel by panel, with the
// predicates the loop had while it was one function). Every condition the loop branches on is written here and nowhere
// else.
//
// Panel k is the block column [k, k + 64). Its step forms Y = A22 W(k), the thin products, and applies (or defers) the
// two-sided update of the trailing matrix of m = n - k - 64 rows; all but the last step also factorise panel k + 64.
//   Quad j        panel j of a group of four whose one k = 512 update is launched at the end of step 3
//   Pair half     panel 0 / 1 of a group of two; the group's k = 256 update runs as two pieces of equal area, the
//                 columns >= c1 at the end of step 1, the columns < c1 at the end of the next group's step 0
//                 (or, after the last pair group, at the hand-over to one update per panel)
//   TwoStream     one update per panel on the main stream, the next factorisation beside it on the look-ahead stream
//   OneStream     fewer than swap_m rows: factorisation and A22 W stay on the main stream, the update goes beside them
//   Last          nothing left to factorise: the update alone
#pragma once
#include <algorithm>

namespace bk {

constexpr int S1_B = 64;   // panel width (== S2_B, the band width)
// trailing-matrix height down to which stage 1 aggregates two panels per update: where the update, not the panel
// factorisation beside it, is the longer launch -- 14 848 with the 64-exchange Householder kernel, 10 752 since pq_chol
// (threshold sweep at N = 20 000: 0.4532 / 0.4498 / 0.4478 / 0.4500 / 0.4520 s at 14 848 / 12 800 / 10 752 / 9 216 / 7 680)
constexpr int S1_AGG_MIN_M = 10752;
constexpr int S1_SWAP_M = 6144;         // trailing-matrix height below which the panel chain stays on one stream
constexpr int S1_QUAD_MIN_M = 12800;    // ... down to which four panels share one update (sweep: 10 752 / 12 800 / 14 000 / 15 000 equal within 1 ms)

enum class S1Arm { Quad, Pair, TwoStream, OneStream, Last };
struct S1Step { S1Arm arm; int j; };                       // j: place in the group (Quad 0..3, Pair 0..1), else 0
struct S1Counts { int quads = 0, pairs = 0, two_stream = 0, one_stream = 0, last = 0; };   // groups, groups, panels, panels, panels

// first column of piece a of the pair group whose second panel's trailing matrix T_{k+1} starts at row0 and has mn rows:
// 64 J1 columns of T_{k+1} are left to piece b, J1 / ncol64 = 1 - 1/sqrt(2) halving the area of the lower triangle
inline int s1_piece_J1(int mn) {
  const int ncol64 = (mn + 63) / 64;
  return std::min(std::max((int)(ncol64 * 0.2929 + 0.5), 1), ncol64 - 1);
}
inline int s1_piece_c1(int row0, int mn) { return row0 + 64 * s1_piece_J1(mn); }
inline int s1_piece_cols(int c1, int row0) { return (c1 - row0) / 64; }   // 64-wide columns of [row0, c1)

struct S1Sched {
  int n = 0;
  int agg_min = S1_AGG_MIN_M, quad_min = S1_QUAD_MIN_M, swap_m = S1_SWAP_M;   // (BIGKRLS_S1AGG_MIN, _S1AGG4_MIN, _S1_SWAP_M)
  int agg_mode = -1;          // BIGKRLS_S1AGG: 0 one update per panel from the start, 2 pairs from the start, else -1
  bool agg_ws = false;        // the workspace of the pending reflector blocks exists (n >= S1_AGG_MIN_M + 256)
  bool fused_panel = true;    // s1_fused_z also updates the next panel's columns (not with BIGKRLS_S1=gemm / nopanel)
  int cap = 80;               // workgroups of pq_resident that can be co-resident
  bool pq_steps = false;      // one launch per column (BIGKRLS_PQ=steps, or after a watchdog)
  bool side_is_main = false;  // the look-ahead stream is the main stream

  bool has_panel(int k) const { return k + S1_B < n && n - k - S1_B > 1; }
  // Above ~80 workgroups the all-to-all of the register-resident factorisation and the CUs its spinning workgroups hold
  // cost more than the 64 launches they replace (measured at N = 50 000)
  bool resident_qr(int k) const { return !pq_steps && (n - k - S1_B + 255) / 256 <= std::min(cap, 80); }
  bool agg_on() const { return agg_ws && fused_panel && agg_mode != 0; }
  bool agg_ok(int k) const {
    return agg_on() && has_panel(k) && has_panel(k + S1_B) && resident_qr(k) && resident_qr(k + S1_B) && n - k - S1_B >= agg_min;
  }
  bool quads_on() const { return agg_on() && agg_mode != 2; }
  bool quad_ok(int k) const {
    return quads_on() && agg_ok(k) && agg_ok(k + S1_B) && agg_ok(k + 2 * S1_B) && agg_ok(k + 3 * S1_B) && n - k - 4 * S1_B >= quad_min;
  }
  bool pair_ok(int k) const { return agg_ok(k) && agg_ok(k + S1_B); }
  // one update per panel: the fused thin products also update the next panel's columns when a register-resident
  // factorisation follows ...
  bool panel_in_z(int k) const { return fused_panel && has_panel(k + S1_B) && resident_qr(k + S1_B); }
  // ... and the arm that takes panel k
  S1Arm single_arm(int k) const {
    if (!has_panel(k + S1_B)) return S1Arm::Last;
    return panel_in_z(k) && n - k - 2 * S1_B < swap_m && !side_is_main ? S1Arm::OneStream : S1Arm::TwoStream;
  }

  // every panel in order: f(k, S1Step). Returns the counts the loop reports under BIGKRLS_VERBOSE.
  template <class F>
  S1Counts walk(F f) const {
    S1Counts c;
    int k = 0;
    for (; quad_ok(k); ++c.quads)
      for (int j = 0; j < 4; ++j, k += S1_B) f(k, S1Step{S1Arm::Quad, j});
    for (; pair_ok(k); ++c.pairs)
      for (int j = 0; j < 2; ++j, k += S1_B) f(k, S1Step{S1Arm::Pair, j});
    for (; has_panel(k); k += S1_B) {
      const S1Arm a = single_arm(k);
      ++(a == S1Arm::OneStream ? c.one_stream : a == S1Arm::TwoStream ? c.two_stream : c.last);
      f(k, S1Step{a, 0});
    }
    return c;
  }
  S1Counts counts() const { return walk([](int, S1Step) {}); }
};

// The row-block distributed stage 1 (dist_s1_group_size of csrc/eigen.hip): panels in the group that may start at k0
// under the mode the ranks agreed on (4: groups of four, then pairs; 2: pairs; 0: none). It differs from quad_ok / pair_ok:
// no residency and no next-panel condition, the compile-time thresholds only, and the pair threshold is on the group's
// second panel -- every rank must reach the same answer whatever its own device and environment say, because the group
// size decides the sequence of collectives.
inline int s1_dist_group_size(int n, int k0, int mode) {
  if (mode == 0) return 0;
  S1Sched s;
  s.n = n;
  const auto panels = [&](int g) {
    for (int j = 0; j < g; ++j)
      if (!s.has_panel(k0 + j * S1_B)) return false;
    return true;
  };
  if (mode != 2 && panels(4) && n - k0 - 4 * S1_B >= S1_QUAD_MIN_M) return 4;
  if (panels(2) && n - k0 - 2 * S1_B >= S1_AGG_MIN_M) return 2;
  return 0;
}

}  // namespace bk
