// The host plan of the deletion residuals (deletion_residuals, csrc/influence.hip): the units (one observation, or one
// cluster of rows) in group_order's stable order (csrc/ktplan.h: the rows of a unit in their original order), every
// unit's size and size class, the per-class lists (unit, first sorted row, m) the kernels walk, and the workspace counts.
// Plain C++: no HIP call, nothing but ktplan.h -- what tests/delplan_check.cpp compiles on its own. Internal and
// header-only, as ktplan.h and s2plan.h.
#pragma once
#include "ktplan.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bk {

// Size classes. A unit of one row has no system to solve (et = e / (1 - h) on the leverage, one vector kernel for all of
// them); classes 1..4 are the instances of the fused kernel (one workgroup per unit: m <= 16 on one wave, m <= 64 and
// m <= DEL_MB on four waves with I - H_SS in LDS, m <= DEL_WIDE_MB on eight waves with I - H_SS in the workspace, where
// it stays in L2); class 5 is the general route through the eigensolver, one unit after the other.
constexpr int DEL_MB = 128;                    // block limit of the LDS instances: I - H_SS at m = 128 is 129 KiB of LDS
constexpr int DEL_WIDE_MB = 256;               // block limit of the wide instance: 514 KiB of workspace per unit in flight
constexpr int DEL_WIDE_BATCH = 128;            // ... and at most this many units per launch
constexpr int DEL_CLASSES = 6;
constexpr int DEL_SINGLE = 0, DEL_WAVE = 1, DEL_MID = 2, DEL_BLOCK = 3, DEL_WIDE = 4, DEL_GENERAL = 5;
constexpr int64_t DEL_CAP_BYTES = 1ll << 30;   // general route: the m x m matrix of one unit, 8 m^2 bytes, at most 1 GiB

// one unit as the kernels read it from device memory: the layout is part of their contract
struct DelUnit {
  int32_t unit, first, m;   // the label; the first of its sorted rows; its rows
};
static_assert(sizeof(DelUnit) == 12 && offsetof(DelUnit, unit) == 0 && offsetof(DelUnit, first) == 4 &&
              offsetof(DelUnit, m) == 8, "DelUnit is read by the deletion kernels");

// route 0: by size; route 1: every unit of two rows or more takes the general route
inline int del_class(int64_t m, int route) {
  if (m <= 0) return -1;
  if (m == 1) return DEL_SINGLE;
  if (route == 1 || m > DEL_WIDE_MB) return DEL_GENERAL;
  return m <= 16 ? DEL_WAVE : (m <= 64 ? DEL_MID : (m <= DEL_MB ? DEL_BLOCK : DEL_WIDE));
}

// the largest m whose 8 m^2 bytes fit the cap
inline int64_t del_cap_rows() {
  int64_t m = 1;
  while (8 * (m + 1) * (m + 1) <= DEL_CAP_BYTES) ++m;   // (at most 11 585 steps)
  return m;
}

struct DelPlan {
  int64_t bad = -1;                       // the first row whose label is outside [0, G), or -1 (nothing else is filled then)
  std::vector<int64_t> off;               // group_order's offsets: unit g holds the sorted rows [off[g], off[g + 1])
  std::vector<int32_t> rows;              // sorted row r is row rows[r] of the caller (always filled, the identity too)
  std::vector<int64_t> size;              // rows of every unit
  std::vector<int8_t> cls;                // class of every unit, -1 for an empty one
  std::vector<DelUnit> list[DEL_CLASSES]; // the units of every class in label order
  int64_t over_unit = -1, over_m = 0;     // the first general-route unit over the cap (nothing may be allocated then)
  int64_t max_general_m = 0;              // the largest unit of the general route
  int64_t general_doubles = 0;            // workspace of the general route: Q_S, Q_S diag(w), A, V, theta, e_S, z, x
  int64_t wide_doubles = 0;               // workspace of the wide instance: one 256 x 257 matrix per unit of a launch
  int64_t index_bytes = 0;                // rows and the per-class lists as they are uploaded (each 8-byte aligned)
  int64_t list_off[DEL_CLASSES] = {0, 0, 0, 0, 0, 0};   // byte offset of every class's list in that upload
  double sum_m2 = 0.0;                    // sum of m_g^2 (the profile's work is 2 k times this)
};

inline DelPlan plan_deletion(const int64_t* labels, int64_t n, int64_t G, int64_t k, int route) {
  DelPlan p;
  GroupOrder go = group_order(labels, n, G);
  p.bad = go.bad;
  if (p.bad >= 0) return p;
  p.off = std::move(go.off);
  p.rows.resize((size_t)n);
  if (go.perm.empty())
    for (int64_t r = 0; r < n; ++r) p.rows[(size_t)r] = (int32_t)r;
  else
    p.rows = std::move(go.perm);
  p.size.resize((size_t)G);
  p.cls.resize((size_t)G);
  const int64_t cap_rows = del_cap_rows();
  for (int64_t g = 0; g < G; ++g) {
    const int64_t m = p.off[(size_t)g + 1] - p.off[(size_t)g];
    const int c = del_class(m, route);
    p.size[(size_t)g] = m;
    p.cls[(size_t)g] = (int8_t)c;
    p.sum_m2 += (double)m * (double)m;
    if (c < 0) continue;
    p.list[c].push_back(DelUnit{(int32_t)g, (int32_t)p.off[(size_t)g], (int32_t)m});
    if (c == DEL_GENERAL) {
      if (m > cap_rows && p.over_unit < 0) {
        p.over_unit = g;
        p.over_m = m;
      }
      p.max_general_m = std::max(p.max_general_m, m);
    }
  }
  if (p.max_general_m > 0 && p.over_unit < 0) {
    const int64_t m = p.max_general_m;
    p.general_doubles = 2 * m * k + 2 * m * m + 4 * m;
  }
  p.wide_doubles = std::min<int64_t>((int64_t)p.list[DEL_WIDE].size(), DEL_WIDE_BATCH) * DEL_WIDE_MB * (DEL_WIDE_MB + 1);
  int64_t at = (n * 4 + 7) / 8 * 8;
  for (int c = 0; c < DEL_CLASSES; ++c) {
    p.list_off[c] = at;
    at += ((int64_t)p.list[c].size() * (int64_t)sizeof(DelUnit) + 7) / 8 * 8;
  }
  p.index_bytes = at;
  return p;
}

}  // namespace bk
