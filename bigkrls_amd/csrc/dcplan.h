// The host arithmetic of the divide & conquer on the tridiagonal matrix (DivideConquer of csrc/eigen.hip): the tree, the
// deflation scan of one merge, which levels stay factored, where a level's secular vectors go, the root's ordering and
// truncation, and the boundary rows of the factored levels. No HIP: a plain host compiler can include this file
// (tests/dcplan_check.cpp checks it on designed inputs). Every floating-point expression here feeds the device bit for
// bit: same operations, same order, same container iteration order as when it was part of one long function.
//
// Everything sits in the unnamed namespace of bk, like the kernels of csrc/eigen.hip that read MergeDesc: their symbol
// names carry the struct's, so moving it to a named namespace would change the device code objects.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

namespace bk {
namespace {

constexpr double DC_EPS = 2.220446049250313e-16;
constexpr int DC_LEAF = 32;       // rows of the largest leaf the QL kernel solves (dc_leaf_ql)
constexpr int DC_LAZY_TOP = 3;    // depths 0 .. DC_LAZY_TOP stay factored when few eigenvectors are wanted

struct MergeDesc {
  int s, n1, m, K;
  int k1, k2, k3, Kneed;
  int rot_off, nrot, ndef, rev;   // rev: columns stored in descending order of the roots (the root of the tree)
  double rho;
  // where the merge's secular vectors go: column c at Ubase + uoff + c * uld -- the block (s, s) of the N x N buffer U
  // (uoff = s + s N, uld = N), or, on a level whose operators stay factored, a contiguous K x K block of the stash
  long long uoff;
  int uld, pad_;
};
// (the kernels read arrays of these as the host lays them out)
static_assert(sizeof(MergeDesc) == 72 && offsetof(MergeDesc, rho) == 48 && offsetof(MergeDesc, uoff) == 56,
              "MergeDesc: layout shared with the kernels");

struct Node {
  int s, m, left, right, depth;
  std::vector<double> dv;  // eigenvalue of storage column s+t
  int ksorted = 0;         // dv[0 .. ksorted) is ascending (the secular roots of the merge that produced the node)
};

// host side of one merge (LAPACK dlaed2's scan, re-derived): fills the packed
// per-level arrays at offset s.
// The n-long arrays are slices of the context's pinned upload arena (PinnedStage::fixed), laid out like their device
// copies -- [dlam | w] and [pole_of_row | srccol | cpos | defsrc | defdst] -- so that a level uploads them with two
// copies straight from where host_merge wrote them.
struct LevelArrays {
  double *dlam = nullptr, *w = nullptr;
  int *pole_of_row = nullptr, *srccol = nullptr, *cpos = nullptr, *defsrc = nullptr, *defdst = nullptr;
  std::vector<int> rowpos;
  std::vector<double> rc, rs;
  std::vector<int> ra, rb;
};

// ---- the tree ------------------------------------------------------------------------------------------------------
// (BIGKRLS_DCLEAF=1: tear down to 1 x 1 leaves, no QL leaf solver)
inline int dc_leaf_max(int n, const char* dcleaf_env) {
  return (n > 2 * DC_LEAF && !(dcleaf_env && std::string(dcleaf_env) == "1")) ? DC_LEAF : 1;
}

struct DcTree {
  int leaf_max = 1, maxdepth = 0;
  std::vector<Node> nodes;                  // a parent before its children, the left subtree after the right one
  std::vector<double> dadj;                 // d minus |e[cut]| at both sides of every cut
  std::vector<std::vector<int>> by_depth;   // the inner nodes of every depth
};

// nodes of more than leaf_max rows are cut into m / 2 and m - m / 2 rows; 1 x 1 leaves know their eigenvalue
inline void dc_build_tree(int n, const std::vector<double>& hd, const std::vector<double>& he, int leaf_max, DcTree& T) {
  T.leaf_max = leaf_max;
  T.nodes.clear();
  T.nodes.reserve(2 * n);
  T.dadj = hd;
  struct Item { int s, m, depth, parent, side; };
  std::vector<Item> stack;
  stack.push_back({0, n, 0, -1, 0});
  while (!stack.empty()) {
    Item it = stack.back();
    stack.pop_back();
    Node nd;
    nd.s = it.s; nd.m = it.m; nd.left = nd.right = -1; nd.depth = it.depth;
    const int id = (int)T.nodes.size();
    T.nodes.push_back(nd);
    if (it.parent >= 0) {
      if (it.side == 0) T.nodes[it.parent].left = id; else T.nodes[it.parent].right = id;
    }
    if (it.m > leaf_max) {
      const int n1 = it.m / 2;
      const int cut = it.s + n1 - 1;  // e[cut] couples rows cut, cut+1
      const double rho = std::fabs(he[cut]);
      T.dadj[cut] -= rho;
      T.dadj[cut + 1] -= rho;
      stack.push_back({it.s, n1, it.depth + 1, id, 0});
      stack.push_back({it.s + n1, it.m - n1, it.depth + 1, id, 1});
    }
  }
  T.maxdepth = 0;
  for (auto& nd : T.nodes) {
    T.maxdepth = std::max(T.maxdepth, nd.depth);
    if (nd.m == 1) nd.dv.assign(1, T.dadj[nd.s]);
  }
  T.by_depth.assign(T.maxdepth + 1, std::vector<int>());
  for (int id = 0; id < (int)T.nodes.size(); ++id)
    if (T.nodes[id].left >= 0) T.by_depth[T.nodes[id].depth].push_back(id);
}

// (s, m) pairs of the leaves the QL kernel solves, in node order
inline std::vector<int> dc_ql_leaves(const DcTree& T) {
  std::vector<int> lf;
  for (const Node& nd : T.nodes)
    if (nd.left < 0 && nd.m > 1) { lf.push_back(nd.s); lf.push_back(nd.m); }
  return lf;
}
// (s, m) pairs of the nodes of one depth, in node order
inline std::vector<int> dc_blocks_at_depth(const DcTree& T, int depth) {
  std::vector<int> zb;
  for (const Node& nd : T.nodes)
    if (nd.depth == depth && nd.m > 0) { zb.push_back(nd.s); zb.push_back(nd.m); }
  return zb;
}

// ---- one merge: the deflation scan ---------------------------------------------------------------------------------
// scratch reused across the merges of a level (thousands of small merges at the bottom of the tree), owned by the caller
struct MergeScratch {
  std::vector<double> z, D;
  std::vector<std::pair<double, int>> keyed, kbuf;
  std::vector<int> order, typ, nd, df;
};

inline void host_merge(const Node& L, const Node& R, double ecut, const double* zraw, MergeDesc& md,
                       LevelArrays& A, std::vector<double>& defvals, MergeScratch& S) {
  const int n1 = L.m, n2 = R.m, m = n1 + n2, s = L.s;
  const double theta = (ecut >= 0.0) ? 1.0 : -1.0;
  const double rho = 2.0 * std::fabs(ecut);
  std::vector<double>&z = S.z, &D = S.D;
  std::vector<std::pair<double, int>>&keyed = S.keyed, &kbuf = S.kbuf;
  std::vector<int>&order = S.order, &typ = S.typ, &nd = S.nd, &df = S.df;
  z.resize(m); D.resize(m); keyed.resize(m); kbuf.resize(m); order.resize(m); typ.resize(m);
  nd.clear(); df.clear();
  const double isq2 = 1.0 / std::sqrt(2.0);
  double dmax = 0.0, zmax = 0.0;
  for (int t = 0; t < m; ++t) {
    z[t] = zraw[s + t] * ((t < n1) ? 1.0 : theta) * isq2;
    D[t] = (t < n1) ? L.dv[t] : R.dv[t - n1];
    keyed[t] = {D[t], t};
    typ[t] = (t < n1) ? 1 : 3;
    dmax = std::max(dmax, std::fabs(D[t]));
    zmax = std::max(zmax, std::fabs(z[t]));
  }
  // ascending in D, ties in storage order: what a stable sort of the indices gives, on (value, index) pairs. Each
  // child's list is its ascending secular roots followed by its deflated values: only the two tails are sorted, the
  // four runs are merged (the root of an N = 20 000 tree: 0.25 instead of 0.7 ms)
  {
    int kl = std::min(L.ksorted, n1), kr = std::min(R.ksorted, m - n1);
    if (!std::is_sorted(keyed.begin(), keyed.begin() + kl)) kl = 0;          // (never seen; costs O(K))
    if (!std::is_sorted(keyed.begin() + n1, keyed.begin() + n1 + kr)) kr = 0;
    std::sort(keyed.begin() + kl, keyed.begin() + n1);
    std::sort(keyed.begin() + n1 + kr, keyed.end());
    // (std::merge into the scratch list and back: std::inplace_merge allocates its buffer at every call -- three calls
    //  per merge, thousands of merges per level)
    std::merge(keyed.begin(), keyed.begin() + kl, keyed.begin() + kl, keyed.begin() + n1, kbuf.begin());
    std::merge(keyed.begin() + n1, keyed.begin() + n1 + kr, keyed.begin() + n1 + kr, keyed.end(), kbuf.begin() + n1);
    std::merge(kbuf.begin(), kbuf.begin() + n1, kbuf.begin() + n1, kbuf.end(), keyed.begin());
  }
  for (int t = 0; t < m; ++t) order[t] = keyed[t].second;
  const double tol = 8.0 * DC_EPS * std::max(dmax, zmax);
  md.s = s; md.n1 = n1; md.m = m; md.rho = rho;
  md.rot_off = (int)A.ra.size(); md.nrot = 0;
  if (rho * zmax <= tol) {
    for (int t : order) df.push_back(t);
  } else {
    int pj = -1;
    for (int t : order) {
      if (rho * std::fabs(z[t]) <= tol) { df.push_back(t); typ[t] = 4; continue; }
      if (pj < 0) { pj = t; continue; }
      double sv = z[pj], cv = z[t];
      const double tt = D[t] - D[pj];
      // dlaed2's test |tt c s| <= tol with c = z_t / tau, s = -z_pj / tau, tau = hypot(z_t, z_pj), in the form that
      // needs neither the root nor the divisions (z is normalised: no overflow): they are only formed for the rare pair
      // that deflates -- the scan visits every non-deflated entry of every level, and hypot + two divisions per entry
      // were most of its time
      const double ss = cv * cv + sv * sv;
      const double tau_safe = (ss > 1e-280) ? 0.0 : std::hypot(cv, sv);     // (squares that underflow: the safe form)
      const bool defl = (ss > 1e-280) ? (std::fabs(tt * cv * sv) <= tol * ss)
                                      : (std::fabs(tt * (cv / tau_safe) * (sv / tau_safe)) <= tol);
      if (defl) {
        const double tau = (ss > 1e-280) ? std::sqrt(ss) : tau_safe;
        cv /= tau; sv = -sv / tau;
        z[t] = tau; z[pj] = 0.0;
        if (typ[t] != typ[pj]) typ[t] = 2;
        typ[pj] = 4;
        A.ra.push_back(pj); A.rb.push_back(t); A.rc.push_back(cv); A.rs.push_back(sv);
        md.nrot++;
        const double tmp = D[pj] * cv * cv + D[t] * sv * sv;
        D[t] = D[pj] * sv * sv + D[t] * cv * cv;
        D[pj] = tmp;
        df.push_back(pj);
        pj = t;
      } else {
        nd.push_back(pj);
        pj = t;
      }
    }
    if (pj >= 0) nd.push_back(pj);
  }
  const int K = (int)nd.size();
  md.K = K; md.Kneed = K; md.ndef = m - K;
  // poles ascending = nd order; rows of U grouped by column type 1,2,3
  int k1 = 0, k2 = 0, k3 = 0;
  for (int t : nd) { if (typ[t] == 1) ++k1; else if (typ[t] == 2) ++k2; else ++k3; }
  md.k1 = k1; md.k2 = k2; md.k3 = k3;
  int p1 = 0, p2 = k1, p3 = k1 + k2;
  for (int i = 0; i < K; ++i) {
    const int t = nd[i];
    A.dlam[s + i] = D[t];
    A.w[s + i] = z[t];
    int row = (typ[t] == 1) ? p1++ : (typ[t] == 2) ? p2++ : p3++;
    A.rowpos[s + i] = row;
    A.pole_of_row[s + row] = i;
    A.srccol[s + row] = t;
    A.cpos[s + i] = i;
  }
  defvals.resize(m - K);
  for (int q = 0; q < m - K; ++q) {
    A.defsrc[s + q] = df[q];
    A.defdst[s + q] = K + q;
    defvals[q] = D[df[q]];
  }
}

// ---- which levels stay factored ------------------------------------------------------------------------------------
// Few eigenvectors wanted (truncation or Neig << N) on a tree deep enough; BIGKRLS_DC=explicit forms every level,
// =factored forces the factored top levels at any size (the tests run small hard spectra); allow_lazy = false: the
// second pass of a decomposition whose root kept too many columns
inline bool dc_lazy(int n, int maxdepth, double keep_thresh, int64_t n_vecs_max, const char* dc_env, bool allow_lazy) {
  const int64_t N = n;
  const std::string dc_mode = dc_env ? dc_env : "";
  return allow_lazy && maxdepth - 1 > DC_LAZY_TOP && dc_mode != "explicit" &&
         ((n >= 4096 && (keep_thresh > 0.0 || n_vecs_max * 8 <= N)) ||
          (dc_mode == "factored" && n >= 128));
}
// a root that keeps more than N/8 columns redoes the divide & conquer explicitly
inline bool dc_redo_explicit(int64_t nv, int64_t N) { return nv * 8 > N; }

// where a level's secular vectors are written: K x K blocks in the stash, one after the other (level_stash_off[q],
// stash_used advanced), or block (s, s) of the N x N buffer U
inline void dc_assign_u(std::vector<MergeDesc>& descs, bool u_to_stash, int n, int64_t& stash_used,
                        std::vector<int64_t>& level_stash_off) {
  const int64_t N = n;
  const int nm = (int)descs.size();
  level_stash_off.assign(u_to_stash ? nm : 0, 0);
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

// ---- the root ------------------------------------------------------------------------------------------------------
// store roots in descending order so that the kept ones are a prefix
inline void dc_root_descending(MergeDesc& md, LevelArrays& A) {
  const int K = md.K, s = md.s;
  for (int j = 0; j < K; ++j) A.cpos[s + j] = K - 1 - j;
  md.rev = 1;
}

// All n values in descending order (vals_desc), the storage columns of the kept vectors (src_cols; returns how many)
// and how many of them are secular vectors of the root (kneed). dv: the root's values in storage order, the K roots
// first. Kept: n_vecs_max columns, or with keep_thresh >= 0 at most max(which(values >= eigtrunc*values[1])) of the
// first n_vals values (at least one).
inline int64_t dc_select_root(const std::vector<double>& dv, int K, int n, int64_t n_vals, int64_t n_vecs_max,
                              double keep_thresh, std::vector<double>& vals_desc, std::vector<int>& src_cols, int& kneed) {
  // descending order of all n values, ties in storage order (= a stable sort of the indices): the K roots are stored
  // in descending order already, so only the deflated tail is sorted and the two runs are merged
  std::vector<int> ord(n);
  std::iota(ord.begin(), ord.end(), 0);
  {
    auto desc = [&](int a, int b) { return dv[a] > dv[b]; };
    const int Kr = K;
    if (std::is_sorted(ord.begin(), ord.begin() + Kr, desc)) {
      std::stable_sort(ord.begin() + Kr, ord.end(), desc);
      std::inplace_merge(ord.begin(), ord.begin() + Kr, ord.end(), desc);
    } else {
      std::stable_sort(ord.begin(), ord.end(), desc);
    }
  }
  vals_desc.resize(n);
  for (int t = 0; t < n; ++t) vals_desc[t] = dv[ord[t]];
  int64_t nv = n_vecs_max;
  if (keep_thresh >= 0.0) {
    int64_t keep = 0;
    const double thr = keep_thresh * vals_desc[0];
    for (int64_t t = 0; t < n_vals; ++t)
      if (vals_desc[t] >= thr) keep = t + 1;   // max(which(values >= eigtrunc*values[1]))
    nv = std::min<int64_t>(nv, std::max<int64_t>(keep, 1));
  }
  src_cols.resize(nv);
  kneed = 0;
  for (int64_t t = 0; t < nv; ++t) {
    src_cols[t] = ord[t];
    if (ord[t] < K) ++kneed;
  }
  return nv;
}

// ---- boundary rows of the factored levels --------------------------------------------------------------------------
// bf / bl: first / last row of the eigenvector matrix of every node of the current frontier, in storage order.
// yf / yl: first / last row of a level's block matrices diag(Q_left, Q_right) (zero in the other child's columns).

// children that are factored themselves: z and yf / yl come from the frontier's rows
inline void dc_rows_from_frontier(const std::vector<MergeDesc>& descs, const std::vector<double>& bf,
                                  const std::vector<double>& bl, std::vector<double>& hz, std::vector<double>& yf,
                                  std::vector<double>& yl) {
  for (const MergeDesc& md : descs) {
    for (int t = 0; t < md.m; ++t) {
      const bool left = t < md.n1;
      hz[md.s + t] = left ? bl[md.s + t] : bf[md.s + t];
      yf[md.s + t] = left ? bf[md.s + t] : 0.0;
      yl[md.s + t] = left ? 0.0 : bl[md.s + t];
    }
  }
}

// the deflation rotations act on the columns of the children's matrices, hence on yf, yl
inline void dc_rows_rotate(const std::vector<MergeDesc>& descs, const LevelArrays& A, std::vector<double>& yf,
                           std::vector<double>& yl) {
  for (const MergeDesc& md : descs) {
    double* f = yf.data() + md.s;
    double* l = yl.data() + md.s;
    for (int t = 0; t < md.nrot; ++t) {
      const int a = A.ra[md.rot_off + t], b = A.rb[md.rot_off + t];
      const double c = A.rc[md.rot_off + t], sn = A.rs[md.rot_off + t];
      const double fa = f[a], fb = f[b], la = l[a], lb = l[b];
      f[a] = c * fa + sn * fb; f[b] = c * fb - sn * fa;
      l[a] = c * la + sn * lb; l[b] = c * lb - sn * la;
    }
  }
}

// the children's first / last rows gathered into the order of the merge's secular-vector rows: dc_vectors pushes
// them through the merge in the pass that writes the vectors
inline void dc_rows_gather(const std::vector<MergeDesc>& descs, const LevelArrays& A, const std::vector<double>& yf,
                           const std::vector<double>& yl, std::vector<double>& gfh, std::vector<double>& glh) {
  for (const MergeDesc& md : descs) {
    for (int i = 0; i < md.K; ++i) {
      gfh[md.s + i] = yf[md.s + A.srccol[md.s + i]];
      glh[md.s + i] = yl[md.s + A.srccol[md.s + i]];
    }
  }
}

// the parents' rows: what dc_vectors pushed through the merge (ofh / olh) in the K non-deflated columns, the
// children's own entries in the deflated ones
inline void dc_rows_scatter(const std::vector<MergeDesc>& descs, const LevelArrays& A, const std::vector<double>& ofh,
                            const std::vector<double>& olh, const std::vector<double>& yf, const std::vector<double>& yl,
                            std::vector<double>& bf, std::vector<double>& bl) {
  for (const MergeDesc& md : descs) {
    for (int j = 0; j < md.K; ++j) { bf[md.s + j] = ofh[md.s + j]; bl[md.s + j] = olh[md.s + j]; }
    for (int t = 0; t < md.m - md.K; ++t) {
      bf[md.s + md.K + t] = yf[md.s + A.defsrc[md.s + t]];
      bl[md.s + md.K + t] = yl[md.s + A.defsrc[md.s + t]];
    }
  }
}

}  // namespace
}  // namespace bk
