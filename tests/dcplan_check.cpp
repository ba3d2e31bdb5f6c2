// Stand-alone check of bigkrls_amd/csrc/dcplan.h (the host arithmetic of the divide & conquer of the dense eigensolver):
//   the tree for every n from 1 to 6000 under both BIGKRLS_DCLEAF settings (leaves tile [0, n) in order, no leaf above
//   leaf_max rows, children of m / 2 and m - m / 2 rows, dadj = d - |e[cut]| at both sides of every cut and nowhere else);
//   host_merge on designed pairs of children (well-separated poles, exact ties, clusters of 1e-13 relative width, z = 0,
//   one non-zero z, |z| ~ 1e-150 that reaches the "squares that underflow" form of the deflation test, ecut < 0; n1 from 1
//   to 64, m up to 512) against what the algorithm guarantees: the counts, the permutations, ascending poles, orthogonal
//   rotations, trace and norm preserved, no kept pole below the deflation threshold;
//   the root's ordering / truncation / Kneed / redo decision against a brute-force stable sort on 12 000 random lists
//   with ties, the fallback branch (roots not in descending order) included;
//   the lazy predicate, the uoff / uld / stash offsets and the four boundary-row steps of a factored level against a
//   literal transcription of the expressions the one long function held.
// No HIP; builds with -fsanitize=address,undefined.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "dcplan.h"

using namespace bk;

static int failures = 0;
#define REQUIRE(cond, ...)                                        \
  do {                                                            \
    if (!(cond)) {                                                \
      if (++failures <= 20) {                                     \
        printf("FAILED %s:%d: %s  [", __FILE__, __LINE__, #cond); \
        printf(__VA_ARGS__);                                      \
        printf("]\n");                                            \
      }                                                           \
    }                                                             \
  } while (0)

static const double EPS = 2.220446049250313e-16;

// ---- the tree ------------------------------------------------------------------------------------------------------
static int depth_of(int m, int leaf_max) { return m > leaf_max ? 1 + depth_of(m - m / 2, leaf_max) : 0; }

static void check_tree(int n, const char* env) {
  // d, e multiples of 1/8 of moderate size: every difference below is exact, whatever the order of the cuts
  std::vector<double> hd(n), he(n);
  for (int i = 0; i < n; ++i) {
    hd[i] = ((i * 37) % 101 - 50) / 8.0;
    he[i] = ((i * 53) % 67 - 33) / 8.0;
  }
  const int leaf_max = dc_leaf_max(n, env);
  REQUIRE(leaf_max == ((n > 64 && !(env && std::string(env) == "1")) ? 32 : 1), "n=%d", n);
  DcTree T;
  dc_build_tree(n, hd, he, leaf_max, T);
  std::vector<double> expect = hd;
  std::vector<std::pair<int, int>> leaves;
  int maxdepth = 0, inner = 0;
  for (int id = 0; id < (int)T.nodes.size(); ++id) {
    const Node& nd = T.nodes[id];
    maxdepth = std::max(maxdepth, nd.depth);
    if (nd.left < 0) {
      REQUIRE(nd.right < 0 && nd.m >= 1 && nd.m <= leaf_max, "n=%d leaf m=%d", n, nd.m);
      leaves.push_back({nd.s, nd.m});
      if (nd.m == 1) REQUIRE(nd.dv.size() == 1 && nd.dv[0] == T.dadj[nd.s], "n=%d s=%d", n, nd.s);
      continue;
    }
    ++inner;
    const Node &L = T.nodes[nd.left], &R = T.nodes[nd.right];
    REQUIRE(nd.m > leaf_max, "n=%d m=%d", n, nd.m);
    REQUIRE(L.s == nd.s && L.m == nd.m / 2 && R.s == nd.s + nd.m / 2 && R.m == nd.m - nd.m / 2, "n=%d s=%d m=%d", n, nd.s, nd.m);
    REQUIRE(L.depth == nd.depth + 1 && R.depth == nd.depth + 1, "n=%d", n);
    const int cut = nd.s + nd.m / 2 - 1;
    expect[cut] -= std::fabs(he[cut]);
    expect[cut + 1] -= std::fabs(he[cut]);
  }
  // by_depth lists every inner node once, at its depth
  std::vector<int> listed_at(T.nodes.size(), -1);
  for (int d = 0; d < (int)T.by_depth.size(); ++d)
    for (int id : T.by_depth[d]) {
      REQUIRE(listed_at[id] < 0 && T.nodes[id].depth == d && T.nodes[id].left >= 0, "n=%d id=%d", n, id);
      listed_at[id] = d;
    }
  REQUIRE(T.nodes[0].s == 0 && T.nodes[0].m == n && T.nodes[0].depth == 0, "n=%d", n);
  REQUIRE(T.maxdepth == maxdepth && (int)T.by_depth.size() == maxdepth + 1 && maxdepth == depth_of(n, leaf_max), "n=%d", n);
  size_t listed = 0;
  for (const auto& lev : T.by_depth) listed += lev.size();
  REQUIRE((int)listed == inner, "n=%d", n);
  std::sort(leaves.begin(), leaves.end());
  int at = 0;
  for (const auto& lf : leaves) {
    REQUIRE(lf.first == at, "n=%d leaf at %d, expected %d", n, lf.first, at);
    at = lf.first + lf.second;
  }
  REQUIRE(at == n, "n=%d leaves end at %d", n, at);
  REQUIRE(T.dadj == expect, "n=%d dadj", n);
  // the two lists the driver uploads
  const std::vector<int> ql = dc_ql_leaves(T);
  size_t big = 0;
  for (const auto& lf : leaves) big += lf.second > 1;
  REQUIRE(ql.size() == 2 * big, "n=%d", n);
  if (maxdepth >= 1) {
    const std::vector<int> zb = dc_blocks_at_depth(T, 1);
    REQUIRE(zb.size() == 4 && zb[1] + zb[3] == n, "n=%d", n);
  }
}

// ---- host_merge ----------------------------------------------------------------------------------------------------
enum Kind { SEPARATED, TIES, CLUSTERS, ZERO_Z, ONE_Z, TINY_Z, NKINDS };
static long safe_branch_pairs = 0, rotations_seen = 0, all_deflated = 0, merges_checked = 0;

static void child_values(std::mt19937_64& g, Kind kind, int m, Node& nd) {
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  nd.dv.resize(m);
  for (int t = 0; t < m; ++t) {
    switch (kind) {
      case TIES: nd.dv[t] = (double)(g() % 4); break;
      case CLUSTERS: nd.dv[t] = (1.0 + (double)(g() % 3)) * (1.0 + 1e-13 * U(g)); break;
      case TINY_Z: nd.dv[t] = (g() % 2 ? 1e-160 : 1e-172) * U(g); break;
      default: nd.dv[t] = 3.0 * U(g); break;
    }
  }
  // as the level loop leaves a node: ksorted ascending roots first, then the deflated values in any order (0: a leaf)
  nd.ksorted = (int)(g() % (m + 1));
  std::sort(nd.dv.begin(), nd.dv.begin() + nd.ksorted);
}

static void check_merge(std::mt19937_64& g, Kind kind, int n1, int n2, bool negative, MergeScratch& S) {
  const int m = n1 + n2, s = (int)(g() % 5), len = s + m + 3;
  Node L, R;
  L.s = s; L.m = n1; L.left = L.right = -1; L.depth = 1;
  R.s = s + n1; R.m = n2; R.left = R.right = -1; R.depth = 1;
  child_values(g, kind, n1, L);
  child_values(g, kind, n2, R);
  std::normal_distribution<double> Nrm(0.0, 1.0);
  std::vector<double> zraw(len, 0.0);
  if (kind == ONE_Z) {
    zraw[s + (int)(g() % m)] = 1.0;
  } else if (kind != ZERO_Z) {
    // the last row of the left child's eigenvector matrix, the first row of the right child's: unit vectors
    for (int half = 0; half < 2; ++half) {
      const int a = half ? n1 : 0, b = half ? m : n1;
      double nrm = 0.0;
      for (int t = a; t < b; ++t) { zraw[s + t] = Nrm(g); nrm += zraw[s + t] * zraw[s + t]; }
      for (int t = a; t < b; ++t) zraw[s + t] = (nrm > 0.0) ? zraw[s + t] / std::sqrt(nrm) : 1.0;
    }
    if (kind == TINY_Z) for (int t = 0; t < m; ++t) zraw[s + t] *= 1e-150;
  }
  const double ecut = (negative ? -1.0 : 1.0) * (0.25 + (double)(g() % 8) / 8.0);

  std::vector<double> dlam(len, -7.0), w(len, -7.0);
  std::vector<int> ipole(len, -7), isrc(len, -7), icpos(len, -7), idefsrc(len, -7), idefdst(len, -7);
  LevelArrays A;
  A.dlam = dlam.data(); A.w = w.data();
  A.pole_of_row = ipole.data(); A.srccol = isrc.data(); A.cpos = icpos.data(); A.defsrc = idefsrc.data(); A.defdst = idefdst.data();
  A.rowpos.assign(len, -7);
  const int rot_before = (int)(g() % 3);      // (rotations of earlier merges of the level)
  for (int i = 0; i < rot_before; ++i) { A.ra.push_back(0); A.rb.push_back(0); A.rc.push_back(1.0); A.rs.push_back(0.0); }
  MergeDesc md{};
  std::vector<double> defvals;
  host_merge(L, R, ecut, zraw.data(), md, A, defvals, S);
  ++merges_checked;

  // the inputs as the scan sees them
  const double theta = (ecut >= 0.0) ? 1.0 : -1.0, rho = 2.0 * std::fabs(ecut);
  std::vector<double> D(m), z(m);
  double dmax = 0.0, zmax = 0.0, sumD = 0.0, sumz2 = 0.0;
  for (int t = 0; t < m; ++t) {
    D[t] = t < n1 ? L.dv[t] : R.dv[t - n1];
    z[t] = zraw[s + t] * (t < n1 ? 1.0 : theta) * (1.0 / std::sqrt(2.0));
    dmax = std::max(dmax, std::fabs(D[t]));
    zmax = std::max(zmax, std::fabs(z[t]));
    sumD += D[t];
    sumz2 += z[t] * z[t];
  }
  const double tol = 8.0 * EPS * std::max(dmax, zmax);
  const int K = md.K, ndef = md.ndef;
  REQUIRE(md.s == s && md.n1 == n1 && md.m == m && md.rho == rho && md.Kneed == K, "kind %d", kind);
  REQUIRE(K >= 0 && K + ndef == m && md.k1 + md.k2 + md.k3 == K && (int)defvals.size() == ndef, "kind %d K=%d ndef=%d m=%d", kind, K, ndef, m);
  REQUIRE(md.rot_off == rot_before && (int)A.ra.size() == rot_before + md.nrot, "kind %d", kind);
  // rowpos / pole_of_row: inverse permutations of [0, K); cpos the identity below the root
  std::vector<int> seen(m, 0);
  for (int i = 0; i < K; ++i) {
    const int row = A.rowpos[s + i];
    REQUIRE(row >= 0 && row < K && A.pole_of_row[s + row] == i && A.cpos[s + i] == i, "kind %d i=%d", kind, i);
    if (!(row >= 0 && row < K)) return;
  }
  // srccol[0..K) with defsrc[0..ndef): a permutation of [0, m); the rows are grouped by column type
  for (int i = 0; i < K; ++i) {
    const int t = A.srccol[s + i];
    REQUIRE(t >= 0 && t < m, "kind %d", kind);
    if (!(t >= 0 && t < m)) return;
    ++seen[t];
    if (i < md.k1) REQUIRE(t < n1, "kind %d row %d of type 1 from the right child", kind, i);
    if (i >= md.k1 + md.k2) REQUIRE(t >= n1, "kind %d row %d of type 3 from the left child", kind, i);
  }
  for (int q = 0; q < ndef; ++q) {
    const int t = A.defsrc[s + q];
    REQUIRE(t >= 0 && t < m && A.defdst[s + q] == K + q, "kind %d", kind);
    if (!(t >= 0 && t < m)) return;
    ++seen[t];
  }
  REQUIRE(std::count(seen.begin(), seen.end(), 1) == m, "kind %d: not a permutation", kind);
  // poles ascending
  for (int i = 1; i < K; ++i) REQUIRE(A.dlam[s + i - 1] <= A.dlam[s + i], "kind %d i=%d %.17g > %.17g", kind, i, A.dlam[s + i - 1], A.dlam[s + i]);
  // the rotations: orthogonal, between two entries of this merge
  for (int r = 0; r < md.nrot; ++r) {
    const double c = A.rc[md.rot_off + r], sn = A.rs[md.rot_off + r];
    REQUIRE(std::fabs(c * c + sn * sn - 1.0) <= 4.0 * EPS, "kind %d c=%.17g s=%.17g", kind, c, sn);
    const int a = A.ra[md.rot_off + r], b = A.rb[md.rot_off + r];
    REQUIRE(a >= 0 && a < m && b >= 0 && b < m && a != b, "kind %d", kind);
  }
  rotations_seen += md.nrot;
  all_deflated += (K == 0);
  // trace and norm
  double tr = 0.0, nrm = 0.0;
  for (int i = 0; i < K; ++i) { tr += A.dlam[s + i]; nrm += A.w[s + i] * A.w[s + i]; }
  for (int q = 0; q < ndef; ++q) { tr += defvals[q]; nrm += S.z[A.defsrc[s + q]] * S.z[A.defsrc[s + q]]; }
  REQUIRE(std::fabs(tr - sumD) <= 8.0 * m * EPS * dmax, "kind %d trace %.17g vs %.17g", kind, tr, sumD);
  REQUIRE(std::fabs(nrm - sumz2) <= 8.0 * m * EPS, "kind %d norm %.17g vs %.17g", kind, nrm, sumz2);
  // no kept pole at or below the deflation threshold
  for (int i = 0; i < K; ++i) REQUIRE(rho * std::fabs(A.w[s + i]) > tol, "kind %d i=%d w=%.3g tol=%.3g", kind, i, A.w[s + i], tol);
  if (kind == ZERO_Z) REQUIRE(K == 0 && md.nrot == 0, "K=%d", K);
  if (kind == ONE_Z) REQUIRE(K == 1 && md.nrot == 0, "K=%d", K);
  if (kind == TINY_Z) {
    // every pair the scan compares has squares that underflow: the safe form decides
    REQUIRE(zmax * zmax * 2.0 <= 1e-280 && rho * zmax > tol, "zmax=%.3g", zmax);
    safe_branch_pairs += std::max(0, K + md.nrot - 1);
  }
}

// ---- the root ------------------------------------------------------------------------------------------------------
static long fallback_lists = 0, redo_lists = 0;
static void check_root(std::mt19937_64& g, double keep_thresh, bool unsorted_roots) {
  const int n = 1 + (int)(g() % 200), K = (int)(g() % (n + 1));
  std::vector<double> dv(n);
  for (int t = 0; t < n; ++t) dv[t] = (double)((int)(g() % 21) - 4) / 4.0;      // ties, a few negative
  std::sort(dv.begin(), dv.begin() + K, std::greater<double>());
  if (unsorted_roots && K >= 2) { dv[0] = -3.0; dv[K - 1] = 9.0; }
  const int64_t n_vals = 1 + (int64_t)(g() % n), n_vecs_max = (int64_t)(g() % (n + 1));
  std::vector<double> vals_desc;
  std::vector<int> src_cols;
  int kneed = -1;
  const int64_t nv = dc_select_root(dv, K, n, n_vals, n_vecs_max, keep_thresh, vals_desc, src_cols, kneed);
  // brute force
  std::vector<int> ord(n);
  std::iota(ord.begin(), ord.end(), 0);
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return dv[a] > dv[b]; });
  std::vector<double> ref_vals(n);
  for (int t = 0; t < n; ++t) ref_vals[t] = dv[ord[t]];
  int64_t ref_nv = n_vecs_max;
  if (keep_thresh >= 0.0) {
    int64_t last = 0;
    for (int64_t t = 0; t < n_vals; ++t)
      if (ref_vals[t] >= keep_thresh * ref_vals[0]) last = t + 1;
    ref_nv = std::min<int64_t>(n_vecs_max, std::max<int64_t>(last, 1));
  }
  int ref_kneed = 0;
  for (int64_t t = 0; t < ref_nv; ++t) ref_kneed += ord[t] < K;
  REQUIRE(vals_desc == ref_vals, "n=%d K=%d", n, K);
  REQUIRE(nv == ref_nv && (int64_t)src_cols.size() == ref_nv && kneed == ref_kneed, "n=%d K=%d nv=%lld/%lld kneed=%d/%d", n, K,
          (long long)nv, (long long)ref_nv, kneed, ref_kneed);
  REQUIRE(std::equal(src_cols.begin(), src_cols.end(), ord.begin()), "n=%d K=%d src_cols", n, K);
  REQUIRE(dc_redo_explicit(nv, n) == (ref_nv * 8 > (int64_t)n), "n=%d nv=%lld", n, (long long)nv);
  fallback_lists += !std::is_sorted(dv.begin(), dv.begin() + K, std::greater<double>());
  redo_lists += dc_redo_explicit(nv, n);
}

// ---- the lazy predicate and the stash offsets: the former expressions, names unchanged ------------------------------
namespace ref {
constexpr int LAZY_TOP = 3;
static bool lazy(int n, int maxdepth, double keep_thresh, int64_t n_vecs_max, const char* dc_env, bool allow_lazy) {
  const int64_t N = n;
  const std::string dc_mode = dc_env ? dc_env : "";
  const bool lazy = allow_lazy && maxdepth - 1 > LAZY_TOP && dc_mode != "explicit" &&
                    ((n >= 4096 && (keep_thresh > 0.0 || n_vecs_max * 8 <= N)) ||
                     (dc_mode == "factored" && n >= 128));   // (forced: the tests run small hard spectra)
  return lazy;
}
static void assign_u(std::vector<MergeDesc>& descs, bool u_to_stash, int n, int64_t& stash_used, std::vector<int64_t>& level_stash_off) {
  const int64_t N = n;
  const int nm = (int)descs.size();
  level_stash_off = std::vector<int64_t>(u_to_stash ? nm : 0);
  for (int q = 0; q < nm; ++q) {
    MergeDesc& md = descs[q];
    if (u_to_stash) {
      level_stash_off[q] = stash_used;
      md.uoff = stash_used;
      md.uld = std::max(md.K, 1);
      stash_used += (int64_t)md.K * md.K;
    } else {
      md.uoff = md.s + (int64_t)md.s * N;
      md.uld = n;
    }
  }
}
}  // namespace ref

static long lazy_true = 0;
static void check_lazy(int n) {
  const double thresholds[] = {-1.0, 0.0, 1e-3};
  const int64_t nvecs[] = {0, n / 16, n / 8, n / 8 + 1, n};
  const char* modes[] = {nullptr, "explicit", "factored"};
  const char* leaf_envs[] = {nullptr, "1"};
  for (const char* le : leaf_envs) {
    const int maxdepth = depth_of(n, dc_leaf_max(n, le));
    for (double kt : thresholds)
      for (int64_t nvm : nvecs)
        for (const char* mode : modes)
          for (bool allow : {true, false}) {
            const bool got = dc_lazy(n, maxdepth, kt, nvm, mode, allow);
            REQUIRE(got == ref::lazy(n, maxdepth, kt, nvm, mode, allow), "n=%d maxdepth=%d kt=%g nvm=%lld mode=%s allow=%d", n,
                    maxdepth, kt, (long long)nvm, mode ? mode : "(unset)", (int)allow);
            lazy_true += got;
          }
  }
}

static void check_offsets(std::mt19937_64& g) {
  const int n = 128 + (int)(g() % 30000);
  int64_t used = 0, ref_used = 0;
  for (int level = 0; level < 4; ++level) {
    const int nm = 1 + (int)(g() % 9);
    std::vector<MergeDesc> a(nm), b;
    int at = 0;
    for (MergeDesc& md : a) {
      md = MergeDesc{};
      md.s = at; md.m = 1 + (int)(g() % (n / nm)); md.K = (int)(g() % (md.m + 1));
      at += md.m;
    }
    b = a;
    const bool to_stash = (g() % 2) != 0;
    std::vector<int64_t> off, ref_off;
    dc_assign_u(a, to_stash, n, used, off);
    ref::assign_u(b, to_stash, n, ref_used, ref_off);
    REQUIRE(off == ref_off && used == ref_used, "n=%d level=%d", n, level);
    for (int q = 0; q < nm; ++q) REQUIRE(a[q].uoff == b[q].uoff && a[q].uld == b[q].uld, "n=%d level=%d q=%d", n, level, q);
  }
}

// ---- the boundary rows of one factored level, step by step against the former loops ---------------------------------
static void check_rows(std::mt19937_64& g) {
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  const int nm = 1 + (int)(g() % 4);
  std::vector<MergeDesc> descs(nm);
  int n = 0;
  for (MergeDesc& md : descs) {
    md = MergeDesc{};
    md.s = n; md.n1 = 1 + (int)(g() % 9); md.m = md.n1 + 1 + (int)(g() % 9); md.K = (int)(g() % (md.m + 1));
    n += md.m;
  }
  std::vector<int> srccol(n), defsrc(n);
  LevelArrays A;
  A.srccol = srccol.data(); A.defsrc = defsrc.data();
  for (MergeDesc& md : descs) {
    std::vector<int> perm(md.m);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin(), perm.end(), g);
    for (int i = 0; i < md.K; ++i) srccol[md.s + i] = perm[i];
    for (int t = 0; t < md.m - md.K; ++t) defsrc[md.s + t] = perm[md.K + t];
    md.rot_off = (int)A.ra.size(); md.nrot = (int)(g() % 4);
    for (int r = 0; r < md.nrot; ++r) {
      const int a = (int)(g() % md.m), b = (a + 1 + (int)(g() % (md.m - 1))) % md.m;
      const double ang = 3.0 * U(g);
      A.ra.push_back(a); A.rb.push_back(b); A.rc.push_back(std::cos(ang)); A.rs.push_back(std::sin(ang));
    }
  }
  std::vector<double> bf(n), bl(n), ofh(n), olh(n);
  for (int t = 0; t < n; ++t) { bf[t] = U(g); bl[t] = U(g); ofh[t] = U(g); olh[t] = U(g); }
  std::vector<double> hz(n, 9.0), yf(n, 9.0), yl(n, 9.0), gfh(n, 0.0), glh(n, 0.0);
  std::vector<double> rz = hz, rf = yf, rl = yl, rgf = gfh, rgl = glh, rbf = bf, rbl = bl;
  dc_rows_from_frontier(descs, bf, bl, hz, yf, yl);
  for (int q = 0; q < nm; ++q) {
    const MergeDesc& md = descs[q];
    for (int t = 0; t < md.m; ++t) {
      const bool left = t < md.n1;
      rz[md.s + t] = left ? rbl[md.s + t] : rbf[md.s + t];
      rf[md.s + t] = left ? rbf[md.s + t] : 0.0;
      rl[md.s + t] = left ? 0.0 : rbl[md.s + t];
    }
  }
  REQUIRE(hz == rz && yf == rf && yl == rl, "from_frontier n=%d", n);
  dc_rows_rotate(descs, A, yf, yl);
  for (int q = 0; q < nm; ++q) {
    const MergeDesc& md = descs[q];
    double* f = rf.data() + md.s;
    double* l = rl.data() + md.s;
    for (int t = 0; t < md.nrot; ++t) {
      const int a = A.ra[md.rot_off + t], b = A.rb[md.rot_off + t];
      const double c = A.rc[md.rot_off + t], sn = A.rs[md.rot_off + t];
      const double fa = f[a], fb = f[b], la = l[a], lb = l[b];
      f[a] = c * fa + sn * fb; f[b] = c * fb - sn * fa;
      l[a] = c * la + sn * lb; l[b] = c * lb - sn * la;
    }
  }
  REQUIRE(yf == rf && yl == rl, "rotate n=%d", n);
  dc_rows_gather(descs, A, yf, yl, gfh, glh);
  dc_rows_scatter(descs, A, ofh, olh, yf, yl, bf, bl);
  for (int q = 0; q < nm; ++q) {
    const MergeDesc& md = descs[q];
    for (int i = 0; i < md.K; ++i) {
      rgf[md.s + i] = rf[md.s + A.srccol[md.s + i]];
      rgl[md.s + i] = rl[md.s + A.srccol[md.s + i]];
    }
    for (int j = 0; j < md.K; ++j) { rbf[md.s + j] = ofh[md.s + j]; rbl[md.s + j] = olh[md.s + j]; }
    for (int t = 0; t < md.m - md.K; ++t) {
      rbf[md.s + md.K + t] = rf[md.s + A.defsrc[md.s + t]];
      rbl[md.s + md.K + t] = rl[md.s + A.defsrc[md.s + t]];
    }
  }
  REQUIRE(gfh == rgf && glh == rgl && bf == rbf && bl == rbl, "gather / scatter n=%d", n);
}

int main() {
  {
    std::mt19937_64 gr(7);
    for (int rep = 0; rep < 2000; ++rep) check_rows(gr);
  }
  for (int n = 1; n <= 6000; ++n) {
    check_tree(n, nullptr);
    check_tree(n, "1");
  }
  check_tree(300, "0");      // (only "1" tears down to 1 x 1)
  REQUIRE(dc_leaf_max(64, nullptr) == 1 && dc_leaf_max(65, nullptr) == 32 && dc_leaf_max(65, "1") == 1 && dc_leaf_max(65, "0") == 32, "leaf_max");

  std::mt19937_64 g(20240611);
  MergeScratch S;
  for (int kind = 0; kind < NKINDS; ++kind)
    for (int n1 = 1; n1 <= 64; ++n1) {
      const int n2s[] = {1, n1, n1 + 1, 1 + (int)(g() % 448)};
      for (int n2 : n2s)
        for (int neg = 0; neg < 2; ++neg) check_merge(g, (Kind)kind, n1, n2, neg != 0, S);
    }
  check_merge(g, SEPARATED, 64, 448, false, S);      // m = 512
  check_merge(g, CLUSTERS, 64, 448, true, S);
  check_merge(g, TINY_Z, 64, 448, true, S);
  REQUIRE(safe_branch_pairs > 1000 && rotations_seen > 1000 && all_deflated > 100, "pairs %ld rotations %ld all-deflated %ld",
          safe_branch_pairs, rotations_seen, all_deflated);

  const double keeps[] = {-1.0, 0.0, 1e-3, 1.0};
  for (int rep = 0; rep < 3000; ++rep)
    for (double kt : keeps) check_root(g, kt, rep % 5 == 0);
  REQUIRE(fallback_lists > 500 && redo_lists > 500, "fallback %ld redo %ld", fallback_lists, redo_lists);

  for (int n = 1; n <= 24000; ++n) check_lazy(n);
  REQUIRE(lazy_true > 0, "the predicate was never true");
  for (int rep = 0; rep < 2000; ++rep) check_offsets(g);

  printf("merges %ld (rotations %ld, pairs decided by the safe form %ld, fully deflated %ld); root lists %d (fallback %ld, redo %ld); "
         "lazy settings true %ld\n", merges_checked, rotations_seen, safe_branch_pairs, all_deflated, 3000 * 4, fallback_lists,
         redo_lists, lazy_true);
  if (failures) {
    printf("dcplan_check: %d FAILURES\n", failures);
    return 1;
  }
  printf("dcplan_check: ok\n");
  return 0;
}
