// The host plan of the back half of the dense eigensolver (csrc/eigen.hip, csrc/eigen_2stage.inc): band -> tridiagonal
// by bulge chasing (stage2_to_tridiag), the stage-2 back-transform (bt2_build_t, back_transform_stage2), the stage-1
// back-transform (bt1_precompute, back_transform_stage1_grouped) and the two-stage workspace. Host arithmetic only, no
// HIP and no getenv: a plain host compiler can include this file (tests/s2plan_check.cpp enumerates it and checks by
// brute force what the kernels rely on). Every condition and size the back half branches on is written here and nowhere
// else; one S2Plan is built per decomposition (DenseEig::carve_workspace) and every call site reads it.
//
// Task (s, t) of the bulge chasing is step t of sweep s: one length-b reflector at rows s + 1 + t b .. of the band; it
// exists while s + 1 + t b <= n - 1. Tasks with equal w = 2 s + t are independent (one wavefront). The stage-2
// back-transform applies the reflectors of BT2_G consecutive sweeps at one step as one task (g, t), group 0 holding
// the LAST sweeps; tasks with equal w = g + t are independent (one anti-diagonal).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "layout.h"

namespace bk {

constexpr int S2_B = 64;          // band width == stage-1 panel width
constexpr int S2_LD = 2 * S2_B;   // rows of the band array (bulges reach 2b-1 below the diagonal)
constexpr int BT2_G = 32;         // sweeps per task of the stage-2 back-transform
constexpr int BT2_CHAIN_MIN_N = 8000;   // below, the back-transform is bound by its dependency chain, not by traffic
constexpr int RB_BOX = 2 * (S2_B + 1);  // 8-byte words per message of the resident bulge chasing: (value, value ^ key(sweep)) pairs
constexpr int S1F_CHUNKS = 2;     // 64-row chunks per workgroup of s1_fused_yt

// layout of the pq_chol mailbox (doubles): PQC_MAXWG partial matrices, the summed matrix (+ padding), the top block
// of Q, then the flag words (partials, slices, top block)
constexpr int PQC_MAXWG = 80;
constexpr int PQC_NG = S2_B * S2_B;     // Gram entries
constexpr int64_t PQC_OFF_SLICES = (int64_t)PQC_MAXWG * PQC_NG;
constexpr int64_t PQC_OFF_QTOP = PQC_OFF_SLICES + PQC_NG + 256;
constexpr int64_t PQC_OFF_FLAGS = PQC_OFF_QTOP + PQC_NG;
// ... and what the head of the split factorisation leaves for its tail (pq_tail): L \ U of Q1 - S in the top-block area,
// the product R2 R1, then S and the reciprocals of U's diagonal
constexpr int64_t PQC_OFF_RPROD = PQC_OFF_FLAGS + 2 * PQC_MAXWG + 16;
constexpr int64_t PQC_OFF_SINV = PQC_OFF_RPROD + PQC_NG;
constexpr int64_t PQC_MAIL_DOUBLES = PQC_OFF_SINV + 2 * S2_B;

// The switches of the back half, as the environment gives them (null: not set). DenseEig fills the first group once per
// decomposition and the second once per process.
struct S2Switches {
  const char *eig = nullptr, *bc = nullptr, *bc_t = nullptr, *bt2 = nullptr, *bt2_seg = nullptr, *bt1 = nullptr;
  int bt1_grp = 0;    // BIGKRLS_BT1_GRP as a number (0: not set)
  bool bg = false;    // BIGKRLS_BG=1: the look-ahead work goes to the lowest-priority stream
};
inline bool s2_is(const char* value, const char* what) { return value && std::string(value) == what; }

// two-stage (band) reduction is the default above 4 panels; BIGKRLS_EIG=1stage forces the one-stage (symv) reduction
// (kept for small n and as a cross-check: the tests run both). The distributed modes are always two-stage.
inline bool s2_two_stage(bool full_mode, const char* eig, int n) { return !full_mode || (!s2_is(eig, "1stage") && n > 4 * S2_B); }

// a run of `count` consecutive tasks of one launch, from `lo`; count == 0: nothing to launch
struct S2Range { int64_t lo = 0; int count = 0; };

// ---- bulge chasing: which kernel
// Regwin: the window in registers (bc_regwin), 512 threads per location; Lds512 / Lds256: the LDS-window kernel
// (BIGKRLS_BC=lds; BIGKRLS_BC_T=256 for 256 threads; A/B: 88 -> ~65 ms at n = 20 000); Persistent: flag-synchronised
// sweeps (bc_persistent); Wavefront: one launch per wavefront, also what follows a fired watchdog (no_resident)
enum class BcArm { Regwin, Lds512, Lds256, Persistent, Wavefront };
inline BcArm bc_requested(const char* bc, const char* bc_t, bool no_resident) {
  const std::string mode = no_resident ? "wavefront" : (bc ? bc : "resident");
  if (mode == "resident") return BcArm::Regwin;
  if (mode == "lds") return bc_t && atoi(bc_t) == 256 ? BcArm::Lds256 : BcArm::Lds512;
  return mode == "persistent" ? BcArm::Persistent : BcArm::Wavefront;
}
inline bool bc_is_resident(BcArm a) { return a == BcArm::Regwin || a == BcArm::Lds512 || a == BcArm::Lds256; }

// ---- stage-2 back-transform: which kernel
// Seq: reflector by reflector, no T factors (bt2_block; BIGKRLS_BT2=seq); WyWavefront: compact-WY tasks, one launch per
// anti-diagonal (bt2_wy; BIGKRLS_BT2=wavefront, and after a fired watchdog); Tasks: one ticket per task (bt2_persistent);
// Chain: tickets are segments of `seg` groups at one step (bt2_chain; the default above BT2_CHAIN_MIN_N)
enum class Bt2Arm { Seq, WyWavefront, Tasks, Chain };
inline Bt2Arm bt2_arm_for(const char* bt2, int n, bool no_resident, bool have_t) {
  if (!have_t) return Bt2Arm::Seq;
  if (no_resident || s2_is(bt2, "wavefront")) return Bt2Arm::WyWavefront;
  return (bt2 ? s2_is(bt2, "chain") : n > BT2_CHAIN_MIN_N) ? Bt2Arm::Chain : Bt2Arm::Tasks;
}
inline int bt2_seg_for(const char* bt2_seg) { return bt2_seg && atoi(bt2_seg) > 0 ? atoi(bt2_seg) : 32; }

// flag words of the persistent stage-2 back-transform (one int per task and 64-column slab), the 8-byte ticket counter
// behind them, what is cleared before the launch and what the slot holds
struct Bt2Flags {
  int64_t total = 0, ticket_off = 0, clear_bytes = 0, slot_bytes = 0;
};

// ---- stage-1 back-transform: merged block reflectors
// panels per merged block reflector: eight (until round 6 four above n = 10 000, where the precomputation of the wider
// blocks on the look-ahead stream cost what the faster steps saved: now built in batched launches, N = 20 000 13.0 ->
// 10.9 ms per back-transform, C3 0.4008-0.4012 -> 0.3991-0.4001 s: profiles/r06/r06j_*). BIGKRLS_BT1_GRP = 2, 4 or 8
// overrides.
inline int bt1_grp_for(int bt1_grp_switch) {
  return bt1_grp_switch == 2 || bt1_grp_switch == 4 || bt1_grp_switch == 8 ? bt1_grp_switch : 8;
}
// a merged group as the device reads it: first panel column, panels, rows of its Vb (n - k0 - 64), offset of Vb in the store
struct Bt1Group { int k0, g, m0, pad; long long voff; };
struct Bt1Plan {
  int grp = 0, LT = 0;                 // panels per group and the order grp * 64 of a merged T (set also for BIGKRLS_BT1=panel)
  std::vector<Bt1Group> groups;        // empty: one panel per step (back_transform_stage1)
  int64_t vtotal = 0;
  int gmax = 0;                        // panels of the largest group
  int64_t maxwork = 0;                 // elements of the largest of: a merged T, any group's Vb

  int64_t ng() const { return (int64_t)groups.size(); }
  int64_t vbig_bytes() const { return (vtotal + 16) * (int64_t)sizeof(double); }
  // SLOT_EIG_TBIG. Per group: the merged T (LT x LT), its Gram matrix (LT x LT), the recurrence's scratch (LT x 64);
  // 8 doubles; the group table with one record to spare; 8 doubles
  struct Tbig { Region T, G, tmp; int64_t table_bytes_off = 0, slot_bytes = 0; };
  Tbig tbig() const {
    Layout L;
    Tbig r;
    r.T = L.dev(ng() * LT * LT);
    r.G = L.dev(ng() * LT * LT);
    r.tmp = L.dev(ng() * LT * S2_B);
    L.dev(8);
    r.table_bytes_off = L.total_doubles() * (int64_t)sizeof(double);
    r.slot_bytes = r.table_bytes_off + (ng() + 1) * (int64_t)sizeof(Bt1Group) + 8 * (int64_t)sizeof(double);
    return r;
  }
  // SLOT_EIG_Z of the back-transform of nv columns: two scratch matrices, the second `w2_off` doubles behind the first
  int64_t z_bytes(int nv) const { return 2 * (int64_t)LT * nv * (int64_t)sizeof(double); }
  int64_t w2_off(int nv) const { return (int64_t)(groups.empty() ? S2_B : LT) * nv; }
};
inline Bt1Plan bt1_plan(int n, int grp, bool grouped) {
  Bt1Plan p;
  const int b = S2_B;
  p.grp = grp;
  p.LT = grp * b;
  if (!grouped) return p;
  int npan = 0;
  for (int k = 0; k + b < n && n - k - b > 1; k += b) ++npan;
  p.maxwork = (int64_t)p.LT * p.LT;
  for (int q = 0; q < npan; q += grp) {
    const int g = std::min(grp, npan - q), k0 = q * b;
    p.groups.push_back(Bt1Group{k0, g, n - k0 - b, 0, (long long)p.vtotal});
    p.vtotal += (int64_t)(n - k0 - b) * b * g;
    p.gmax = std::max(p.gmax, g);
    p.maxwork = std::max<int64_t>(p.maxwork, (int64_t)(n - k0 - b) * b * g);
  }
  return p;
}

// ---- the two-stage workspace
// the norm and dot partials of the panel factorisation, then the mailboxes of pq_resident: 2 buffers x workgroups x 64
// word pairs, and 2 buffers x 16 group boxes of its two-level exchange (both zeroed per decomposition, as one range)
struct S1Part {
  Region part, mail, mail2;
  int64_t clear_doubles() const { return mail.len + mail2.len; }
};
inline S1Part s1_part(Layout& L, int64_t N) {
  const int64_t maxb = (N + 255) / 256 + 2;
  S1Part p;
  p.part = L.dev(2 * maxb + 2 * maxb * S2_B + S2_B + S2_B * S2_B + 2 * N);
  p.mail = L.dev(2 * maxb * 2 * S2_B);
  p.mail2 = L.dev(2 * 16 * 2 * S2_B);
  return p;
}
// SLOT_EIG_BT (no slack: the slot is the sum of its regions)
struct S1Regions {
  Region Vp, Vw, Tfold, Y, Y2, PZ1, PZ2, small;
  S1Part p;
  Region Tall, fpart, pqc, taus1, AB, soff;
  int64_t doubles = 0;
};
inline S1Regions s1_regions(int64_t N) {
  const int64_t nb64 = N * S2_B, bb = S2_B * S2_B;
  Layout L;
  S1Regions r;
  r.Vp = L.dev(nb64);
  r.Vw = L.dev(nb64);       // Vw, Tfold: the split panel factorisation
  r.Tfold = L.dev(bb);
  r.Y = L.dev(nb64);
  r.Y2 = L.dev(nb64);
  r.PZ1 = L.dev(2 * nb64);
  r.PZ2 = L.dev(2 * nb64);
  r.small = L.dev(8 * bb);
  r.p = s1_part(L, N);
  r.Tall = L.dev((N / S2_B + 2) * bb);
  r.fpart = L.dev((N / (S1F_CHUNKS * S2_B) + 3) * bb);   // partial V'Y blocks of the fused small products
  r.pqc = L.dev(PQC_MAIL_DOUBLES);                        // pq_chol mailbox
  r.taus1 = L.dev(2 * N);                                 // taus1, scales1
  r.AB = L.dev((int64_t)S2_LD * N);
  r.soff = L.dev(N + 8);                                  // the sweep offsets, as int64
  r.doubles = L.total_doubles();
  return r;
}

// ---- the plan
struct S2Plan {
  int n = 0, nsweep = 0;
  int nloc = 0;                    // steps of sweep 0: locations of the resident bulge chasing, t range of the back-transform's tasks
  // bulge chasing
  std::vector<int64_t> soff;       // reflector slot offset of sweep s
  int64_t nrefl = 0;
  BcArm bc_request = BcArm::Wavefront;
  // stage-2 back-transform
  bool have_t = false;             // T factors of the tasks are built (every arm but Seq)
  int ngroups = 0, ntmax = 0;
  std::vector<int64_t> toff;       // slot of task (g, t)'s T factor: toff[g] + t
  int64_t ntasks = 0;
  Bt2Arm bt2_arm = Bt2Arm::Seq;
  int seg = 32;
  // stage-1 back-transform
  Bt1Plan bt1;

  // -- bulge chasing
  // the arm that runs, given how many workgroups of the requested resident kernel fit on the device at once: too many
  // locations to keep resident means wavefront launches
  BcArm bc_arm(int capacity) const {
    return bc_is_resident(bc_request) && nloc > capacity ? BcArm::Wavefront : bc_request;
  }
  int64_t bc_mail_doubles() const { return (int64_t)(nloc + 1) * 3 * RB_BOX; }   // (bc_regwin: three boxes per location)
  // bc_persistent: grid = min(sweeps in flight, co-resident capacity)
  int bc_persistent_grid(int capacity) const { return std::min(std::min(nsweep, nloc / 2 + 2), capacity); }
  // last wavefront: s = n-3, t = 0 (lo = n-2 <= n-1; t = 1 would need lo = n-2+b > n-1 unless b == 1)
  int64_t bc_tmax() const { return 2ll * (nsweep - 1) + ((n - 1) - (nsweep - 1 + 1)) / S2_B; }
  // sweeps of wavefront w: tasks (s, t), t = w - 2s >= 0, lo = s+1+t b <= n-1, s <= n-3
  S2Range bc_wavefront(int64_t w) const {
    const int b = S2_B;
    const int64_t smax = std::min<int64_t>(w / 2, nsweep - 1);
    // s + 1 + (w - 2s) b <= n - 1  <=>  s (2b - 1) >= w b - n + 2
    const int64_t num = w * b - n + 2;
    const int64_t smin = num > 0 ? (num + (2 * b - 2)) / (2 * b - 1) : 0;
    if (smin > smax) return S2Range{};
    return S2Range{smin, (int)(smax - smin + 1)};
  }
  int64_t vv_bytes() const { return (nrefl * (S2_B + 1) + 16) * (int64_t)sizeof(double); }   // SLOT_EIG_VV: VV, then TT
  int64_t tt_off() const { return nrefl * S2_B; }

  // -- stage-2 back-transform
  // SLOT_EIG_T2: the T factors (BT2_G x BT2_G per task), then toff as int64
  int64_t t2_bytes() const { return (t2_toff_off() + (int64_t)toff.size() + 8) * (int64_t)sizeof(double); }
  int64_t t2_toff_off() const { return ntasks * BT2_G * BT2_G; }
  unsigned build_t_grid() const { return (unsigned)(((int64_t)ntmax * ngroups + 3) / 4); }   // one wave per (g, t), t < ntmax
  int slabs(int nv) const { return (nv + 63) / 64; }
  int bt2_diagonals() const { return ngroups + ntmax - 1; }
  // groups of anti-diagonal w: tasks (g, t = w - g), 0 <= g < ngroups, 0 <= t < ntmax (a task whose window starts past
  // row n - 1 is skipped by the kernel)
  S2Range bt2_diagonal(int w) const {
    const int g_hi = std::min(w, ngroups - 1), g_lo = std::max(0, w - (ntmax - 1));
    if (g_lo > g_hi) return S2Range{};
    return S2Range{g_lo, g_hi - g_lo + 1};
  }
  Bt2Flags bt2_flags(int nv) const {
    Bt2Flags f;
    f.total = ntasks * slabs(nv);
    f.ticket_off = (f.total + 3) / 2 * 2;      // (8-byte aligned) the ticket counter behind the flags
    f.clear_bytes = (f.ticket_off + 4) * (int64_t)sizeof(int);
    f.slot_bytes = (f.ticket_off + 16) * (int64_t)sizeof(int);
    return f;
  }
  static int bt2_persistent_grid(int per_cu, int ncu, int64_t total) {
    return (int)std::min<int64_t>((int64_t)std::max(1, per_cu) * ncu, total);
  }
};

// `two_stage`: s2_two_stage(); `want_vectors`: the caller asked for eigenvectors (n_vecs_max > 0). A one-stage
// decomposition has an empty plan.
inline S2Plan s2_plan(int n, bool two_stage, bool want_vectors, bool no_resident, const S2Switches& sw) {
  S2Plan p;
  if (!two_stage) return p;
  p.n = n;
  p.nsweep = std::max(0, n - 2);
  p.nloc = (n - 2) / S2_B + 1;
  p.soff.resize(p.nsweep + 1);
  int64_t o = 0;
  for (int s = 0; s < p.nsweep; ++s) {
    p.soff[s] = o;
    o += (n - 1 - (s + 1)) / S2_B + 1;   // steps t with s+1+t*b <= n-1
  }
  p.soff[p.nsweep] = o;
  p.nrefl = o;
  p.bc_request = bc_requested(sw.bc, sw.bc_t, no_resident);
  // T factors of the stage-2 back-transform tasks (BIGKRLS_BT2=seq: reflector-by-reflector kernel)
  p.have_t = want_vectors && n >= 3 && !s2_is(sw.bt2, "seq");
  p.ntmax = p.nloc;
  p.ngroups = (p.nsweep + BT2_G - 1) / BT2_G;
  if (p.have_t) {
    p.toff.assign(p.ngroups + 1, 0);
    for (int g = 0; g < p.ngroups; ++g) {
      const int s_hi = (n - 3) - g * BT2_G;
      const int s_lo = std::max(0, s_hi - BT2_G + 1);
      p.toff[g + 1] = p.toff[g] + ((n - 2 - s_lo) / S2_B + 1);   // steps t with s_lo + 1 + t b <= n - 1
    }
    p.ntasks = p.toff.back();
  }
  p.bt2_arm = bt2_arm_for(sw.bt2, n, no_resident, p.have_t);
  p.seg = bt2_seg_for(sw.bt2_seg);
  // merged block reflectors of the stage-1 back-transform (BIGKRLS_BT1=panel: one panel per step)
  p.bt1 = bt1_plan(n, bt1_grp_for(sw.bt1_grp), want_vectors && !s2_is(sw.bt1, "panel"));
  return p;
}

}  // namespace bk
