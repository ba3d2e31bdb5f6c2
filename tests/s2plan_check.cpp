// Stand-alone check of the host plan of the dense eigensolver's back half (bigkrls_amd/csrc/s2plan.h), built and run by
// tests/test_s2plan_cpu.py with -fsanitize=address,undefined.
//
//   s2plan_check tests/golden/s2_plans.txt      check: invariants of every plan, then equality with the file row for row
//   s2plan_check --print | --print-full         print the rows (to compare two versions of the header by hand)
//
// Two layers, over n = 1 .. 2 600 and n = 8 000, 8 001, 20 000, 32 768, 40 000 (every n is planned as a two-stage
// decomposition, also those the solver would take in one stage). The invariants are what the kernels rely on, checked
// by brute force beside every plan. The golden rows pin the plans themselves: the file was recorded once, by compiling
// this program against a scratch header that held the statements csrc/eigen.hip and csrc/eigen_2stage.inc had before they
// moved into s2plan.h, verbatim, behind this header's interface. Every n has four rows of figures, in hexadecimal (g, a,
// w, b below). The file holds them in full for n = 259, 1 100, 8 000, 8 001, 20 000, 32 768 and 40 000, and for EVERY n
// one row "n checksum": 64-bit FNV-1a of the four rows' text (--print-full prints all four rows of every n, to find what
// moved when a checksum does):
//   g  n (decimal), then the geometry: nsweep nloc nrefl soff(fnv last) tmax | ngroups ntmax ntasks toff(fnv last) diagonals,
//      tasks launched past the last row, grid of bt2_build_t
//   a  arms under the default switches (bulge chasing at capacities 0, 1, nloc - 1, nloc, 304 and the grid of
//      bc_persistent there; stage-2 back-transform, seg; two_stage by default and under BIGKRLS_EIG=1stage), then ONE 64-bit
//      FNV-1a checksum over every arm choice of every switch combination below, in the loops' order
//   w  slot sizes in bytes (BT VV T2 FLAGS(nv = n) Z-mailbox VBIG TBIG Z(nv = n)) and every region offset but the zeros
//      of the first regions: the regions of SLOT_EIG_BT in doubles, TT, toff, the flag layout at nv = n (total, ticket,
//      bytes cleared), the regions of SLOT_EIG_TBIG (G, tmp in doubles, the table in bytes)
//   b  the stage-1 back-transform's groups for group sizes 2, 4 and 8: groups, vtotal, gmax, maxwork, fnv of the table
#include "s2plan.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

namespace {

std::FILE* g_golden = nullptr;   // null: print
bool g_print_full = false;
long long g_rows = 0, g_failures = 0, g_bc_tasks = 0, g_bt2_tasks = 0, g_bt2_skipped = 0, g_fallbacks = 0, g_chain = 0;

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
};
uint32_t fnv(const std::vector<int64_t>& v) {
  Fnv f;
  for (int64_t x : v) f.add(x);
  return f.h;
}
struct Fnv64 {
  uint64_t h = 14695981039346656037ull;
  void add(int64_t v) {
    for (int b = 0; b < 8; ++b) { h ^= ((uint64_t)v >> (8 * b)) & 0xffu; h *= 1099511628211ull; }
  }
};

uint64_t fnv64(const std::string& row) {   // (of the rows' text: every figure in them)
  Fnv64 f;
  for (unsigned char c : row) { f.h ^= c; f.h *= 1099511628211ull; }
  return f.h;
}

std::string fmt(const char* f, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, f);
  std::vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}
std::string hex(int64_t v) { return fmt(" %llx", (unsigned long long)v); }

void emit(const std::string& row) {
  ++g_rows;
  if (!g_golden) { std::printf("%s\n", row.c_str()); return; }
  char line[2048];
  do {
    if (!std::fgets(line, sizeof line, g_golden)) { fail("the golden file ends before row %lld: %s", g_rows, row.c_str()); return; }
  } while (line[0] == '#' || line[0] == '\n');
  line[std::strcspn(line, "\n")] = 0;
  REQUIRE(row == line, "row %lld: got    %s\n          golden %s", g_rows, row.c_str(), line);
}

constexpr int B = bk::S2_B, G = bk::BT2_G;

bk::S2Plan plan_of(int n, const bk::S2Switches& sw = bk::S2Switches(), bool no_resident = false, bool want_vectors = true) {
  return bk::s2_plan(n, true, want_vectors, no_resident, sw);
}

// ---- the bulge-chasing wavefronts: every task (s, t) with s + 1 + t b <= n - 1 exactly once, nothing else, and both
// predecessors (s, t - 1) and (s - 1, t + 1) on an earlier wavefront; soff is the running count of the sweeps' steps
void check_bulge_chase(const bk::S2Plan& p) {
  const int n = p.n;
  REQUIRE(p.nsweep == std::max(0, n - 2) && (int64_t)p.soff.size() == p.nsweep + 1, "n=%d: %d sweeps", n, p.nsweep);
  int64_t o = 0;
  for (int s = 0; s < p.nsweep; ++s) {
    int steps = 0;
    for (int t = 0; s + 1 + (int64_t)t * B <= n - 1; ++t) ++steps;
    REQUIRE(p.soff[s] == o, "n=%d: soff[%d] = %lld, the sweeps before it have %lld steps", n, s, (long long)p.soff[s], (long long)o);
    if (s == 0) REQUIRE(steps == p.nloc, "n=%d: sweep 0 has %d steps, nloc = %d", n, steps, p.nloc);
    o += steps;
  }
  REQUIRE(p.nrefl == o && p.soff[p.nsweep] == o, "n=%d: nrefl = %lld, the sweeps have %lld steps", n, (long long)p.nrefl, (long long)o);
  if (p.nsweep == 0) return;
  std::vector<int> wave((size_t)p.nrefl, -1);
  int64_t seen = 0;
  const auto steps_of = [&](int s) { return p.soff[s + 1] - p.soff[s]; };
  for (int64_t w = 0; w <= p.bc_tmax() + 3; ++w) {
    const bk::S2Range r = p.bc_wavefront(w);
    REQUIRE(w <= p.bc_tmax() || r.count == 0, "n=%d: wavefront %lld behind tmax has tasks", n, (long long)w);
    for (int64_t s = r.lo; s < r.lo + r.count; ++s) {
      const int64_t t = w - 2 * s;
      if (!(s >= 0 && s < p.nsweep && t >= 0 && t < steps_of((int)s))) {
        fail("n=%d: wavefront %lld launches the invalid task (%lld, %lld)", n, (long long)w, (long long)s, (long long)t);
        continue;
      }
      int& slot = wave[(size_t)(p.soff[s] + t)];
      REQUIRE(slot < 0, "n=%d: task (%lld, %lld) on wavefronts %d and %lld", n, (long long)s, (long long)t, slot, (long long)w);
      slot = (int)w;
      ++seen;
    }
  }
  REQUIRE(seen == p.nrefl, "n=%d: the wavefronts visit %lld of %lld tasks", n, (long long)seen, (long long)p.nrefl);
  for (int s = 0; s < p.nsweep && g_failures == 0; ++s)
    for (int64_t t = 0; t < steps_of(s); ++t) {
      const int w = wave[(size_t)(p.soff[s] + t)];
      if (t > 0) REQUIRE(wave[(size_t)(p.soff[s] + t - 1)] < w, "n=%d: (%d, %lld) not behind (s, t - 1)", n, s, (long long)t);
      if (s > 0 && t + 1 < steps_of(s - 1))
        REQUIRE(wave[(size_t)(p.soff[s - 1] + t + 1)] < w, "n=%d: (%d, %lld) not behind (s - 1, t + 1)", n, s, (long long)t);
    }
  g_bc_tasks += seen;
}

// ---- the stage-2 back-transform's anti-diagonals: every valid (g, t) exactly once; what is launched past the last row
// (the kernels skip it) is counted; toff[g + 1] - toff[g] is the number of valid t of group g
int64_t check_bt2(const bk::S2Plan& p) {
  const int n = p.n;
  REQUIRE(p.ngroups == (p.nsweep + G - 1) / G && p.ntmax == p.nloc, "n=%d: %d groups, ntmax %d", n, p.ngroups, p.ntmax);
  REQUIRE(p.have_t == (n >= 3) && (int64_t)p.toff.size() == (p.have_t ? p.ngroups + 1 : 0), "n=%d: T factors", n);
  if (!p.have_t) return 0;
  const auto valid = [&](int g, int t) {
    const int s_hi = (n - 3) - g * G, s_lo = std::max(0, s_hi - G + 1);   // (as the kernels decode a task)
    return s_lo + 1 + (int64_t)t * B <= n - 1;
  };
  std::vector<char> hit((size_t)p.ngroups * p.ntmax, 0);
  int64_t skipped = 0, visited = 0;
  for (int w = 0; w < p.bt2_diagonals() + 3; ++w) {
    const bk::S2Range r = p.bt2_diagonal(w);
    REQUIRE(w < p.bt2_diagonals() || r.count == 0, "n=%d: anti-diagonal %d behind the last has tasks", n, w);
    for (int64_t g = r.lo; g < r.lo + r.count; ++g) {
      const int64_t t = w - g;
      if (!(g >= 0 && g < p.ngroups && t >= 0 && t < p.ntmax)) {
        fail("n=%d: anti-diagonal %d launches (%lld, %lld) outside the task grid", n, w, (long long)g, (long long)t);
        continue;
      }
      REQUIRE(!hit[(size_t)g * p.ntmax + t]++, "n=%d: task (%lld, %lld) launched twice", n, (long long)g, (long long)t);
      if (valid((int)g, (int)t)) ++visited; else ++skipped;
    }
  }
  for (int g = 0; g < p.ngroups; ++g) {
    int nvalid = 0;
    for (int t = 0; t < p.ntmax; ++t) {
      if (!valid(g, t)) continue;
      REQUIRE(nvalid == t, "n=%d: the valid steps of group %d are not 0 .. count - 1", n, g);   // (toff[g] + t is a slot)
      ++nvalid;
      REQUIRE(hit[(size_t)g * p.ntmax + t] == 1, "n=%d: task (%d, %d) is never launched", n, g, t);
    }
    REQUIRE(p.toff[g + 1] - p.toff[g] == nvalid, "n=%d: group %d has %d valid steps, toff says %lld", n, g, nvalid,
            (long long)(p.toff[g + 1] - p.toff[g]));
  }
  REQUIRE(p.toff[0] == 0 && p.ntasks == p.toff.back() && visited == p.ntasks, "n=%d: %lld tasks visited, ntasks %lld", n,
          (long long)visited, (long long)p.ntasks);
  REQUIRE((int64_t)p.build_t_grid() * 4 >= (int64_t)p.ntmax * p.ngroups && ((int64_t)p.build_t_grid() - 1) * 4 < (int64_t)p.ntmax * p.ngroups,
          "n=%d: bt2_build_t's grid of %u workgroups of four waves", n, p.build_t_grid());
  g_bt2_tasks += visited;
  g_bt2_skipped += skipped;
  return skipped;
}

// ---- the flag words and the ticket of the persistent kernels
void check_flags(const bk::S2Plan& p, int nv) {
  const bk::Bt2Flags f = p.bt2_flags(nv);
  const int64_t words = (int64_t)sizeof(int);
  REQUIRE(f.total == p.ntasks * ((nv + 63) / 64), "n=%d nv=%d: %lld flag words", p.n, nv, (long long)f.total);
  REQUIRE(f.ticket_off >= f.total && (f.ticket_off * words) % 8 == 0, "n=%d nv=%d: the ticket overlaps the flags or is not 8-byte aligned", p.n, nv);
  REQUIRE(f.clear_bytes >= f.ticket_off * words + 8 && f.clear_bytes <= f.slot_bytes, "n=%d nv=%d: the cleared range", p.n, nv);
  REQUIRE(bk::S2Plan::bt2_persistent_grid(0, 256, f.total) == std::min<int64_t>(256, f.total) &&
          bk::S2Plan::bt2_persistent_grid(2, 256, f.total) == std::min<int64_t>(512, f.total), "n=%d nv=%d: the persistent grid", p.n, nv);
}

// ---- regions of one slot: disjoint, in order, ending at `end` (in the regions' unit)
void check_regions(int n, const char* slot, const std::vector<bk::Region>& rs, int64_t end) {
  int64_t at = 0;
  for (size_t i = 0; i < rs.size(); ++i) {
    REQUIRE(rs[i].off == at && rs[i].len >= 0, "n=%d: region %zu of %s starts at %lld, the one before it ends at %lld", n, i, slot,
            (long long)rs[i].off, (long long)at);
    at = rs[i].off + rs[i].len;
  }
  REQUIRE(at == end, "n=%d: the regions of %s end at %lld, the slot at %lld", n, slot, (long long)at, (long long)end);
}

// ---- the merged groups of the stage-1 back-transform: they tile the panels in order, voff contiguous
void check_bt1(int n, const bk::Bt1Plan& bp, int grp) {
  int npan = 0;
  while ((npan + 1) * B < n && n - npan * B - B > 1) ++npan;   // panels k = 64 i with k + 64 < n and more than one row below
  REQUIRE(bp.grp == grp && bp.LT == grp * B, "n=%d grp=%d: plan says grp %d, LT %d", n, grp, bp.grp, bp.LT);
  int next_panel = 0, gmax = 0;
  int64_t voff = 0, maxwork = (int64_t)bp.LT * bp.LT;
  for (size_t q = 0; q < bp.groups.size(); ++q) {
    const bk::Bt1Group& gr = bp.groups[q];
    REQUIRE(gr.k0 == next_panel * B && gr.g >= 1 && gr.g <= grp && (gr.g == grp || q + 1 == bp.groups.size()) && gr.pad == 0,
            "n=%d grp=%d: group %zu starts at column %d with %d panels", n, grp, q, gr.k0, gr.g);
    REQUIRE(gr.m0 == n - gr.k0 - B && gr.voff == voff, "n=%d grp=%d: group %zu: m0 %d, voff %lld", n, grp, q, gr.m0, gr.voff);
    next_panel += gr.g;
    voff += (int64_t)gr.m0 * B * gr.g;
    gmax = std::max(gmax, gr.g);
    maxwork = std::max(maxwork, (int64_t)gr.m0 * B * gr.g);
  }
  REQUIRE(next_panel == npan && bp.vtotal == voff && bp.gmax == gmax && bp.maxwork == maxwork,
          "n=%d grp=%d: %d of %d panels, vtotal %lld", n, grp, next_panel, npan, (long long)bp.vtotal);
  const bk::Bt1Plan::Tbig t = bp.tbig();
  const int64_t dbl = (int64_t)sizeof(double), rec = (int64_t)sizeof(bk::Bt1Group);
  // in bytes: T, G, tmp, 8 doubles, the table with one record to spare, 8 doubles
  check_regions(n, "SLOT_EIG_TBIG", {{t.T.off * dbl, t.T.len * dbl}, {t.G.off * dbl, t.G.len * dbl}, {t.tmp.off * dbl, t.tmp.len * dbl},
                                     {(t.tmp.off + t.tmp.len) * dbl, 8 * dbl}, {t.table_bytes_off, (bp.ng() + 1) * rec},
                                     {t.table_bytes_off + (bp.ng() + 1) * rec, 8 * dbl}}, t.slot_bytes);
  REQUIRE(t.T.len == bp.ng() * bp.LT * bp.LT && t.G.len == t.T.len && t.tmp.len == bp.ng() * bp.LT * B, "n=%d grp=%d: T, G, tmp", n, grp);
  REQUIRE(bp.vbig_bytes() >= bp.vtotal * dbl, "n=%d grp=%d: SLOT_EIG_VBIG", n, grp);
  for (int nv : {1, 65, n}) {
    // (no panel, no group: the panel form's second matrix, 64 rows behind the first)
    REQUIRE(bp.w2_off(nv) == (int64_t)(bp.groups.empty() ? B : bp.LT) * nv && 2 * (int64_t)bp.LT * nv * dbl == bp.z_bytes(nv),
            "n=%d grp=%d: the two scratch matrices", n, grp);
  }
}

std::string bt1_row_part(const bk::Bt1Plan& bp) {
  Fnv f;
  for (const bk::Bt1Group& gr : bp.groups)
    for (int64_t v : {(int64_t)gr.k0, (int64_t)gr.g, (int64_t)gr.m0, (int64_t)gr.pad, (int64_t)gr.voff}) f.add(v);
  return fmt("| %llx %llx %x %llx %08x", (long long)bp.ng(), (long long)bp.vtotal, bp.gmax, (long long)bp.maxwork, f.h);
}

void check_n(int n) {
  const bk::S2Plan p = plan_of(n);
  REQUIRE(p.n == n, "n=%d: the plan says n = %d", n, p.n);
  check_bulge_chase(p);
  const int64_t skipped = check_bt2(p);
  for (int nv : {1, 64, 65, n}) check_flags(p, nv);
  const int64_t dbl = (int64_t)sizeof(double);

  // g
  const std::string g = fmt("g %d", n) + hex(p.nsweep) + hex(p.nloc) + hex(p.nrefl) + fmt(" %08x", fnv(p.soff)) + hex(p.soff.back()) +
       fmt(" %lld|", (long long)(p.nsweep > 0 ? p.bc_tmax() : -1)) + hex(p.ngroups) + hex(p.ntmax) + hex(p.ntasks) + fmt(" %08x", fnv(p.toff)) +
       hex(p.toff.empty() ? 0 : p.toff.back()) + hex(p.bt2_diagonals()) + hex(skipped) +
                        hex(p.build_t_grid());

  // a
  const int caps[] = {0, 1, p.nloc - 1, p.nloc, 304};
  std::string a = "a ";
  for (int cap : caps) a += fmt("%d", (int)p.bc_arm(cap));
  for (int cap : caps) a += hex(p.nsweep > 0 ? p.bc_persistent_grid(cap) : 0);   // (no sweep: nothing is launched)
  a += fmt(" %d %d %d%d", (int)p.bt2_arm, p.seg, (int)bk::s2_two_stage(true, nullptr, n), (int)bk::s2_two_stage(true, "1stage", n));
  REQUIRE(bk::s2_two_stage(false, "1stage", n), "n=%d: the distributed modes are two-stage", n);
  Fnv64 all;
  const char* bcs[] = {nullptr, "resident", "lds", "persistent", "wavefront", "", "other"};
  const char* bcts[] = {nullptr, "256", "512", "x"};
  for (const char* bc : bcs)
    for (const char* bct : bcts)
      for (int no_res = 0; no_res < 2; ++no_res) {
        bk::S2Switches sw;
        sw.bc = bc;
        sw.bc_t = bct;
        const bk::S2Plan q = plan_of(n, sw, no_res != 0);
        const bool lds = bc && !std::strcmp(bc, "lds");
        const bk::BcArm want = no_res ? bk::BcArm::Wavefront
                             : (!bc || !std::strcmp(bc, "resident")) ? bk::BcArm::Regwin
                             : lds ? (bct && !std::strcmp(bct, "256") ? bk::BcArm::Lds256 : bk::BcArm::Lds512)
                             : !std::strcmp(bc, "persistent") ? bk::BcArm::Persistent : bk::BcArm::Wavefront;
        REQUIRE(q.bc_request == want, "n=%d BIGKRLS_BC=%s BIGKRLS_BC_T=%s no_resident=%d: request %d", n, bc ? bc : "(unset)",
                bct ? bct : "(unset)", no_res, (int)q.bc_request);
        for (int cap : caps) {
          const bk::BcArm arm = q.bc_arm(cap);
          // a resident kernel whose locations do not all fit falls back to one launch per wavefront; nothing else moves
          REQUIRE(arm == (bk::bc_is_resident(want) && q.nloc > cap ? bk::BcArm::Wavefront : want), "n=%d: arm %d at capacity %d", n, (int)arm, cap);
          g_fallbacks += arm != want;
          all.add((int64_t)arm);
          all.add(q.nsweep > 0 ? q.bc_persistent_grid(cap) : 0);
        }
      }
  const char* bt2s[] = {nullptr, "seq", "wavefront", "chain", "tasks", "", "other"};
  const char* segs[] = {nullptr, "3", "0", "-2", "x", "32"};
  for (const char* bt2 : bt2s)
    for (const char* seg : segs)
      for (int no_res = 0; no_res < 2; ++no_res)
        for (int vectors = 0; vectors < 2; ++vectors) {
          bk::S2Switches sw;
          sw.bt2 = bt2;
          sw.bt2_seg = seg;
          const bk::S2Plan q = plan_of(n, sw, no_res != 0, vectors != 0);
          const bool seq = bt2 && !std::strcmp(bt2, "seq");
          REQUIRE(q.have_t == (vectors && n >= 3 && !seq) && (q.bt2_arm == bk::Bt2Arm::Seq) == !q.have_t, "n=%d: T factors and the Seq arm", n);
          if (q.have_t) {
            const bk::Bt2Arm want = (no_res || !std::strcmp(bt2 ? bt2 : "", "wavefront")) ? bk::Bt2Arm::WyWavefront
                                  : (bt2 ? !std::strcmp(bt2, "chain") : n > bk::BT2_CHAIN_MIN_N) ? bk::Bt2Arm::Chain : bk::Bt2Arm::Tasks;
            REQUIRE(q.bt2_arm == want, "n=%d BIGKRLS_BT2=%s no_resident=%d: arm %d", n, bt2 ? bt2 : "(unset)", no_res, (int)q.bt2_arm);
            g_chain += !bt2 && q.bt2_arm == bk::Bt2Arm::Chain;
          }
          REQUIRE(q.seg == (seg && std::atoi(seg) > 0 ? std::atoi(seg) : 32), "n=%d BIGKRLS_BT2_SEG=%s: seg %d", n, seg ? seg : "(unset)", q.seg);
          all.add((int64_t)q.bt2_arm);
          all.add(q.seg);
          all.add(q.have_t);
          all.add(q.ntasks);
        }
  for (const char* bt1 : {(const char*)nullptr, "panel", "other"})
    for (int grp_sw : {0, 2, 4, 8, 3, 16})
      for (int vectors = 0; vectors < 2; ++vectors) {
        bk::S2Switches sw;
        sw.bt1 = bt1;
        sw.bt1_grp = grp_sw;
        const bk::S2Plan q = plan_of(n, sw, false, vectors != 0);
        const int grp = grp_sw == 2 || grp_sw == 4 ? grp_sw : 8;
        const bool grouped = vectors && !(bt1 && !std::strcmp(bt1, "panel"));
        REQUIRE(q.bt1.grp == grp && q.bt1.LT == grp * B && (grouped || q.bt1.groups.empty()), "n=%d: the stage-1 back-transform's arm", n);
        if (!grouped) REQUIRE(q.bt1.w2_off(7) == 7 * B && q.bt1.z_bytes(7) == 2 * 7 * grp * B * dbl, "n=%d: the panel form's scratch", n);
        all.add(q.bt1.grp);
        all.add(q.bt1.ng());
        all.add(q.bt1.vtotal);
      }
  a += fmt(" %016llx", (unsigned long long)all.h);

  // w
  const bk::S1Regions r = bk::s1_regions(n);
  check_regions(n, "SLOT_EIG_BT", {r.Vp, r.Vw, r.Tfold, r.Y, r.Y2, r.PZ1, r.PZ2, r.small, r.p.part, r.p.mail, r.p.mail2, r.Tall, r.fpart,
                                   r.pqc, r.taus1, r.AB, r.soff}, r.doubles);
  REQUIRE(r.p.clear_doubles() == r.p.mail.len + r.p.mail2.len && r.p.mail2.off == r.p.mail.off + r.p.mail.len, "n=%d: the mailboxes are cleared as one range", n);
  REQUIRE(r.soff.len >= (int64_t)p.soff.size() && r.pqc.len == bk::PQC_MAIL_DOUBLES && r.taus1.len == 2 * (int64_t)n && r.AB.len == (int64_t)bk::S2_LD * n,
          "n=%d: soff, pqc, taus1, AB", n);
  // SLOT_EIG_VV: VV (64 per reflector), TT (one per reflector), 16 doubles; SLOT_EIG_T2: the T factors, toff, 8 doubles
  check_regions(n, "SLOT_EIG_VV", {{0, p.nrefl * B}, {p.tt_off(), p.nrefl}, {p.tt_off() + p.nrefl, 16}}, p.vv_bytes() / dbl);
  check_regions(n, "SLOT_EIG_T2", {{0, p.ntasks * G * G}, {p.t2_toff_off(), (int64_t)p.toff.size()}, {p.t2_toff_off() + (int64_t)p.toff.size(), 8}},
                p.t2_bytes() / dbl);
  const bk::Bt2Flags fn = p.bt2_flags(n);
  const bk::Bt1Plan::Tbig tb = p.bt1.tbig();
  std::string w = "w" + hex(r.doubles * dbl) + hex(p.vv_bytes()) + hex(p.t2_bytes()) + hex(fn.slot_bytes) + hex(p.bc_mail_doubles() * dbl) +
                  hex(p.bt1.vbig_bytes()) + hex(tb.slot_bytes) + hex(p.bt1.z_bytes(n)) + "|";
  REQUIRE(r.Vp.off == 0 && tb.T.off == 0 && (p.soff.empty() || p.soff.front() == 0), "n=%d: the first regions start their slots", n);
  for (const bk::Region& x : {r.Vw, r.Tfold, r.Y, r.Y2, r.PZ1, r.PZ2, r.small, r.p.part, r.p.mail, r.p.mail2, r.Tall, r.fpart, r.pqc,
                              r.taus1, r.AB, r.soff})
    w += hex(x.off);
  w += "|" + hex(p.tt_off()) + hex(p.t2_toff_off()) + hex(fn.total) + hex(fn.ticket_off) + hex(fn.clear_bytes) + "|" + hex(tb.G.off) + hex(tb.tmp.off) + hex(tb.table_bytes_off);

  // b
  std::string b = "b";
  for (int grp : {2, 4, 8}) {
    const bk::Bt1Plan bp = bk::bt1_plan(n, bk::bt1_grp_for(grp), true);
    check_bt1(n, bp, grp);
    b += bt1_row_part(bp);
  }

  // one row for every n; the four in full for the sizes the tests and the benchmark run at
  emit(fmt("%d %016llx", n, (unsigned long long)fnv64(g + "\n" + a + "\n" + w + "\n" + b)));
  bool full = g_print_full;
  for (int named : {259, 1100, 8000, 8001, 20000, 32768, 40000}) full = full || n == named;
  if (full)
    for (const std::string& row : {g, a, w, b}) emit(row);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: s2plan_check tests/golden/s2_plans.txt | --print | --print-full\n"); return 2; }
  g_print_full = !std::strcmp(argv[1], "--print-full");
  if (std::strcmp(argv[1], "--print") && !g_print_full) {
    g_golden = std::fopen(argv[1], "r");
    if (!g_golden) { std::printf("s2plan_check: cannot open %s\n", argv[1]); return 2; }
  }
  for (int n = 1; n <= 2600; ++n) check_n(n);
  for (int n : {8000, 8001, 20000, 32768, 40000}) check_n(n);
  // the constants the kernels are written for
  static_assert(bk::S2_B == 64 && bk::S2_LD == 128 && bk::BT2_G == 32 && bk::RB_BOX == 130 && bk::S1F_CHUNKS == 2 && bk::PQC_MAXWG == 80, "");
  static_assert(bk::PQC_OFF_SLICES == 80 * 4096 && bk::PQC_OFF_QTOP == 81 * 4096 + 256 && bk::PQC_OFF_FLAGS == 82 * 4096 + 256 &&
                bk::PQC_OFF_RPROD == 82 * 4096 + 256 + 176 && bk::PQC_OFF_SINV == 83 * 4096 + 432 && bk::PQC_MAIL_DOUBLES == 83 * 4096 + 560, "");
  if (!g_golden) return g_failures == 0 ? 0 : 1;
  char line[2048];
  while (std::fgets(line, sizeof line, g_golden))
    if (line[0] != '#' && line[0] != '\n') { fail("the golden file has rows beyond the grid"); break; }
  std::fclose(g_golden);
  REQUIRE(g_fallbacks > 0 && g_chain > 0 && g_bt2_skipped > 0, "the grid no longer reaches a fallback, the size rule of the chain kernel or a skipped task");
  std::printf("s2plan_check: %lld rows; %lld bulge-chasing tasks and %lld back-transform tasks enumerated, %lld launched past the last row; "
              "%lld arm choices fell back to wavefront launches\n", g_rows, g_bc_tasks, g_bt2_tasks, g_bt2_skipped, g_fallbacks);
  if (g_failures == 0) std::printf("s2plan_check: ok\n");
  else std::printf("s2plan_check: %lld failures\n", g_failures);
  return g_failures == 0 ? 0 : 1;
}
