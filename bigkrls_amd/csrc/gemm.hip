// fp64 MFMA GEMM core for gfx950 (v_mfma_f64_16x16x4_f64) with pluggable epilogues.
//
// One core serves:
//   * the Gaussian kernel build  K = exp(-(|a_i|^2 + |b_j|^2 - 2 a_i.b_j)/sigma)
//     (replaces the scalar double loops of src/gauss_kernel.cpp:13-30 and
//     src/temp_kernel.cpp:13-30)  -- "NT" product with a fused norm+exp epilogue;
//   * the cross-products of src/crossprod.cpp:13-85 (A'B, A'A, AB', AA');
//   * every GEMM inside the eigensolver, the variance matrices and the
//     marginal-effects pass.
//
// Tiling (CDNA4, wave64): block tile 128 x BN x 16 with 256 threads = 4 waves in a
// 2 x 2 grid; each wave owns 64 x BN/2 as 4 x (BN/32) MFMA tiles of 16 x 16.
// Operands are staged global -> registers -> LDS (double buffered, one barrier per
// k-tile); LDS tiles are k-major with a rotate+xor swizzle so that both the
// fragment reads (ds_read_b64, 16 consecutive doubles per k row) and the
// transposing stores are bank-conflict free.
//
// MFMA operand mapping (f64 16x16x4: lane l supplies A[i=l&15][k=l>>4] and
// B[k=l>>4][j=l&15]; result reg r of lane l is D[i=(l>>4)+4r][j=l&15]):
// we feed the N-side fragment as the MFMA "A" and the M-side fragment as the MFMA
// "B", so that the lane index (l&15) runs along the column-major-contiguous M
// dimension of C and every 16 lanes store one 128-byte segment.
#include "common.h"
#include "ktplan.h"
#include "splitplan.h"
#include "syrkmap.h"
#include <algorithm>
#include <cstring>
#include <type_traits>

namespace bk {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int BM = 128;
constexpr int BK = 16;
constexpr int NT = 256;
#ifndef GEMM_OCC
#define GEMM_OCC 2
#endif

// LDS layouts of one W x BK operand stage (no swizzle: every index is a per-thread base plus a
// compile-time constant, so all fragment reads and staging stores use immediate offsets):
//   contiguous-x operands ("KX"):  [k][x], row stride W + GEMM_KX_PAD doubles. A half-wave of a
//       fragment read covers two k rows x 16 x; with a pad of 16 they land half the banks apart
//       (conflict-free), with 8 half of the lanes pay a 2-way conflict -- not measurable, and the
//       128 x 64 tile then needs 52 KB, so three workgroups fit a CU.
//   k-contiguous operands ("XK"):  [x][k], row stride BK + 2 = 18 doubles. A half-wave reads
//       16 x (18 lm mod 32: the 16 even banks) x 2 k: 32 distinct banks.
constexpr int LDS_XK = BK + 2;
#ifndef GEMM_KX_PAD
#define GEMM_KX_PAD 8
#endif
// plain GEMM kernels with tiles up to this width keep two k-tiles in flight (see gemm_tile)
#ifndef GEMM_DEEP_BN
#define GEMM_DEEP_BN 64
#endif
// ... and keep load issue, MFMAs and staging stores of a half-iteration in that order (0: the compiler's own order)
#ifndef GEMM_DEEP_PIN
#define GEMM_DEEP_PIN 1
#endif
constexpr int lds_stage(int w) {   // room for either layout
  return BK * (w + GEMM_KX_PAD) > w * LDS_XK ? BK * (w + GEMM_KX_PAD) : w * LDS_XK;
}
// one layout only: the 128 x 64 tile of the trailing update (both operands x-contiguous) needs 52 KB with this and
// 54 KB with lds_stage() -- three workgroups fit the 160 KB of a CU only with the former (see syrk_mirror_kernel)
constexpr int lds_stage_of(bool contig_x, int w) { return contig_x ? BK * (w + GEMM_KX_PAD) : w * LDS_XK; }
template <bool CONTIG_X, int W>
__device__ __forceinline__ int lds_at(int k, int x) {
  return CONTIG_X ? k * (W + GEMM_KX_PAD) + x : x * LDS_XK + k;
}

// Load a W x 16 operand tile into registers. Element (x, k) lives at
// src[x*sx + k*sk]; CONTIG_X says which of the two strides is 1.
template <bool CONTIG_X, int W, bool GATHER = false>
__device__ __forceinline__ void tile_load(const double* __restrict__ src, int64_t ld, int x0,
                                          int k0, int xmax, int kmax, double (&r)[W / 16],
                                          const int* __restrict__ kidx = nullptr) {
  // Branch-free and select-free: out-of-range elements read a clamped (valid) address.
  //  * A predicated load puts every load in its own basic block and the compiler then drains
  //    vmcnt to 0 before the first MFMA of the k-tile; a select right after the load does the
  //    same. Either way the whole global latency is exposed once per k-tile.
  //  * Rows/columns past xmax only ever feed accumulator entries that are never stored.
  //  * k past kmax is zeroed by tile_zero_ktail() just before the LDS store of the last tile.
  const int t = threadIdx.x;
  if (CONTIG_X) {
    const int x = t % W;
    const int kb = t / W;
    constexpr int KS = NT / W;
    const int gx = x0 + x;
    const double* base = src + (gx < xmax ? gx : xmax - 1);
#pragma unroll
    for (int q = 0; q < W / 16; ++q) {
      const int gk = k0 + kb + q * KS;
      const int kc = gk < kmax ? gk : kmax - 1;
      const int64_t col = GATHER ? (int64_t)kidx[kc] : (int64_t)kc;
      r[q] = base[col * ld];
    }
  } else {
    const int k = t & 15;
    const int xb = t >> 4;
    const int gk = k0 + k;
    const double* base = src + (gk < kmax ? gk : kmax - 1);
#pragma unroll
    for (int q = 0; q < W / 16; ++q) {
      const int gx = x0 + xb + 16 * q;
      const int xc = gx < xmax ? gx : xmax - 1;
      r[q] = base[(int64_t)xc * ld];
    }
  }
}

// zero the staged elements whose k index lies past kmax (last, partial k-tile only)
template <bool CONTIG_X, int W>
__device__ __forceinline__ void tile_zero_ktail(int k0, int kmax, double (&r)[W / 16]) {
  const int t = threadIdx.x;
  if (CONTIG_X) {
    const int kb = t / W;
    constexpr int KS = NT / W;
#pragma unroll
    for (int q = 0; q < W / 16; ++q)
      if (k0 + kb + q * KS >= kmax) r[q] = 0.0;
  } else {
    if (k0 + (t & 15) >= kmax) {
#pragma unroll
      for (int q = 0; q < W / 16; ++q) r[q] = 0.0;
    }
  }
}

// Fast loader for interior k-tiles: p points at this thread's first element of the tile and
// the remaining elements follow at a fixed stride, so the address math is one 64-bit add each.
template <int W>
__device__ __forceinline__ void tile_load_strided(const double* __restrict__ p, int64_t stride,
                                                  double (&r)[W / 16]) {
#pragma unroll
  for (int q = 0; q < W / 16; ++q) r[q] = p[q * stride];
}

template <bool CONTIG_X, int W>
__device__ __forceinline__ void tile_store(double* __restrict__ lds, const double (&r)[W / 16]) {
  const int t = threadIdx.x;
  if (CONTIG_X) {
    const int x = t % W;
    const int kb = t / W;
    constexpr int KS = NT / W;
#pragma unroll
    for (int q = 0; q < W / 16; ++q) lds[lds_at<true, W>(kb + q * KS, x)] = r[q];
  } else {
    const int k = t & 15;
    const int xb = t >> 4;
#pragma unroll
    for (int q = 0; q < W / 16; ++q) lds[lds_at<false, W>(k, xb + 16 * q)] = r[q];
  }
}

struct GemmOperands {
  const double* A;
  const double* B;
  int64_t lda, ldb;
  int M, N, K;
  const int* kidx;  // optional gather of A's columns (NN only): op(A)(:,k) = A(:, kidx[k])
  const int* run_if = nullptr;  // optional device-side predicate (plain GEMM kernels only): nothing is done while *run_if == 0
};

// Optional modulation of a not-transposed A operand on its way to LDS (gemm_tile<.., MOD = true>, gemm_modulated):
// op(A)(m, k) = A(m, k) (r[m] + t[m] s[k]); r and t have M entries, s has K.
struct GemmMod {
  const double* r;
  const double* t;
  const double* s;
};

// Optional second modulation beside GemmMod (gemm_tile<.., MOD = true, .., MOD2 = true>, gemm_modulated2):
// op(A)(m, k) = A(m, k) fma(fma(t[m], s[k], r[m]), fma(t2[m], s2[k], r2[m]), d); r2 and t2 have M entries, s2 has K.
struct GemmMod2 {
  const double* r2;
  const double* t2;
  const double* s2;
  double d;
};

// Computes the accumulators of the (m0, n0) block tile over k in [kbeg, kend).
// TA/TB: operand is used transposed (op(A) = A' with A stored K x M, etc.).
// MOD: the A operand is modulated (GemmMod) between its staging registers and LDS; off, `mod` is never read.
// MOD2 (with MOD): the factor is the product of two such modulations plus a constant (GemmMod2); off, `mod2` is never read.
// WK: a transposed A operand (k-contiguous) is weighted along the contraction, op(A)(m, k) = A(k, m) wk[k], between its
// staging registers and LDS (gram_weighted: A' diag(wk) B); off, `wk` is never read.
template <bool TA, bool TB, int BN, bool GATHER = false, bool DEEP = false, bool MOD = false, bool WK = false,
          bool MOD2 = false>
__device__ __forceinline__ void gemm_tile(const GemmOperands& g, int m0, int n0, int kbeg,
                                          int kend, double* __restrict__ smem,
                                          d4 (&acc)[4][BN / 32], const GemmMod* mod = nullptr,
                                          const double* __restrict__ wk = nullptr,
                                          const GemmMod2* mod2 = nullptr) {
  static_assert(!MOD2 || MOD, "gemm_tile: the second modulation comes with the first");
  static_assert(!MOD || (!TA && !GATHER), "gemm_tile: the modulated A operand is not transposed and not gathered");
  static_assert(!WK || (TA && !GATHER && !MOD), "gemm_tile: the k-weighted A operand is transposed, not gathered, not modulated");
  constexpr int NJ = BN / 32;
  // A tile: op(A)(m,k). not transposed: A[m + k lda] -> contiguous along m.
  constexpr bool A_CONTIG = !TA;
  // B tile: op(B)(k,n). transposed: B stored N x K, B[n + k ldb] -> contiguous along n.
  constexpr bool B_CONTIG = TB;
  // LDS stage offsets are kept as integers added to `smem` at each use: selecting between
  // pointers (double* As[2]) makes the compiler lose the LDS address space and emit flat loads,
  // whose completion is then tied to the outstanding global loads (vmcnt).
  constexpr int A_STAGE = lds_stage_of(A_CONTIG, BM), B_BASE = 2 * A_STAGE, B_STAGE = lds_stage_of(B_CONTIG, BN);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = (wave & 1) * 64;
  const int wn = (wave >> 1) * (BN / 2);
  const int lm = lane & 15;
  const int lk = lane >> 4;

#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};

  double ra[BM / 16];
  double rb[BN / 16];
  const int ntiles = (kend - kbeg + BK - 1) / BK;
  if (ntiles <= 0) return;

  // Per-thread strided pointers for the fast loader (valid for full k-tiles; an operand whose
  // non-contiguous x range leaves the matrix, or a gathered A, stays on the clamped loader).
  const int tid = threadIdx.x;
  const bool a_fast = !GATHER && (A_CONTIG || m0 + BM <= g.M);
  const bool b_fast = B_CONTIG || n0 + BN <= g.N;
  const double* pa;
  const double* pb;
  int64_t sa, sb, ia, ib;  // element stride inside a tile, pointer advance per k-tile
  if (A_CONTIG) {
    const int gx = m0 + tid % BM;
    pa = g.A + (gx < g.M ? gx : g.M - 1) + (int64_t)(kbeg + tid / BM) * g.lda;
    sa = (NT / BM) * g.lda;
    ia = BK * g.lda;
  } else {
    pa = g.A + (kbeg + (tid & 15)) + (int64_t)(a_fast ? m0 + (tid >> 4) : 0) * g.lda;
    sa = 16 * g.lda;
    ia = BK;
  }
  if (B_CONTIG) {
    const int gx = n0 + tid % BN;
    pb = g.B + (gx < g.N ? gx : g.N - 1) + (int64_t)(kbeg + tid / BN) * g.ldb;
    sb = (NT / BN) * g.ldb;
    ib = BK * g.ldb;
  } else {
    pb = g.B + (kbeg + (tid & 15)) + (int64_t)(b_fast ? n0 + (tid >> 4) : 0) * g.ldb;
    sb = 16 * g.ldb;
    ib = BK;
  }
  // Modulated A (m-contiguous: this thread stages row m0 + tid % BM at the k rows tid / BM + (NT / BM) q of every
  // k-tile): r and t of its row live in two registers; the tile's s values are loaded together with the tile (the same
  // address over a wave: cached broadcast loads), clamped like the tile's own addresses, and the factor is applied in
  // registers just before the LDS store (mod_apply) -- nothing sits between the global loads and the MFMAs.
  // MOD2: r2, t2 of the row in two more registers, the tile's s2 values in the upper half of the same register set
  // (xs[MQ1 + q] beside xs[q]), loaded and clamped with them; the s2 pointer is ps plus a fixed offset.
  constexpr int MQ1 = MOD ? BM / 16 : 1;
  constexpr int MQ = MOD2 ? 2 * MQ1 : MQ1;
  double mod_r = 0.0, mod_t = 0.0, mod_r2 = 0.0, mod_t2 = 0.0, mod_d = 0.0;
  const double* ps = nullptr;
  const double* ps2 = nullptr;
  double rs[MQ];
  if (MOD) {
    const int gx = m0 + tid % BM;
    const int gc = gx < g.M ? gx : g.M - 1;
    mod_r = mod->r[gc];
    mod_t = mod->t[gc];
    ps = mod->s + kbeg + tid / BM;
    if constexpr (MOD2) {
      // (tid / BM is the same over a wave: said so, the s values of both modulations are scalar loads into scalar
      //  registers -- the vector file is full with gemm_modulated's one set)
      const int kb = __builtin_amdgcn_readfirstlane(tid / BM);
      mod_r2 = mod2->r2[gc];
      mod_t2 = mod2->t2[gc];
      mod_d = mod2->d;
      ps = mod->s + kbeg + kb;
      ps2 = mod2->s2 + kbeg + kb;
    }
  }
  // Weighted transposed A (k-contiguous: this thread stages the k row kbeg + (tid & 15) of every k-tile for BM / 16
  // columns): one weight per thread and k-tile, loaded with the tile and clamped like the tile's own addresses.
  if (WK) ps = wk + kbeg + (tid & 15);
  auto mod_load = [&](int k0, double (&xs)[MQ]) {
    constexpr int KS = NT / BM;
    if constexpr (WK) {
      const int gk = k0 + (tid & 15);
      const double* pw = (k0 + BK <= kend) ? ps : wk + (gk < kend ? gk : kend - 1);   // (one load, of a valid address)
      xs[0] = *pw;
    } else if (k0 + BK <= kend) {
#pragma unroll
      for (int q = 0; q < MQ1; ++q) xs[q] = ps[q * KS];
      if constexpr (MOD2) {
#pragma unroll
        for (int q = 0; q < MQ1; ++q) xs[MQ1 + q] = ps2[q * KS];
      }
    } else {
      const int kb = k0 + (MOD2 ? __builtin_amdgcn_readfirstlane(tid / BM) : tid / BM);
#pragma unroll
      for (int q = 0; q < MQ1; ++q) {
        const int gk = kb + q * KS;
        xs[q] = mod->s[gk < kend ? gk : kend - 1];
        if constexpr (MOD2) xs[MQ1 + q] = mod2->s2[gk < kend ? gk : kend - 1];
      }
    }
    ps += BK;
    if constexpr (MOD2) ps2 += BK;
  };
  auto mod_apply = [&](double (&xa)[BM / 16], const double (&xs)[MQ]) {
    if constexpr (WK) {
#pragma unroll
      for (int q = 0; q < BM / 16; ++q) xa[q] *= xs[0];
    } else if constexpr (MOD2) {
#pragma unroll
      for (int q = 0; q < MQ1; ++q)
        xa[q] *= fma(fma(mod_t, xs[q], mod_r), fma(mod_t2, xs[MQ1 + q], mod_r2), mod_d);
    } else {
#pragma unroll
      for (int q = 0; q < MQ; ++q) xa[q] *= fma(mod_t, xs[q], mod_r);
    }
  };
  auto load_tiles = [&](int k0) {
    const bool full = k0 + BK <= kend;
    if (full && a_fast) tile_load_strided<BM>(pa, sa, ra);
    else tile_load<A_CONTIG, BM, GATHER>(g.A, g.lda, m0, k0, g.M, kend, ra, g.kidx);
    if (full && b_fast) tile_load_strided<BN>(pb, sb, rb);
    else tile_load<B_CONTIG, BN>(g.B, g.ldb, n0, k0, g.N, kend, rb);
    if constexpr (MOD || WK) mod_load(k0, rs);
    pa += ia;
    pb += ib;
  };

  auto mfma_tile = [&](int cur) {
    const double* as = smem + cur * A_STAGE;
    const double* bs = smem + B_BASE + cur * B_STAGE;
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      double af[4], bf[NJ];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = as[lds_at<A_CONTIG, BM>(kk + lk, wm + i * 16 + lm)];
#pragma unroll
      for (int j = 0; j < NJ; ++j) bf[j] = bs[lds_at<B_CONTIG, BN>(kk + lk, wn + j * 16 + lm)];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(bf[j], af[i], acc[i][j], 0, 0, 0);
    }
  };

  if (DEEP) {
    // Two k-tiles in flight: the loads of tile t+2 are issued before the MFMAs of tile t, tile t+1
    // waits in the other register set and goes to LDS after them. A thin tile (BN = 64) has only
    // ~1.7 us of MFMA work per k-tile and CU -- less than the HBM latency a single tile in flight
    // would have to hide.
    //
    // What is in flight where (L = loads of one register set: BM / 16 + BN / 16, plus the modulation's; 12 for
    // gemm_kernel<N,N,64>), in the interior loop below:
    //   half 0:  issue L loads of tile t+2 into set 1          outstanding: set 2 (tile t+1), set 1 (tile t+2) = 2 L
    //            MFMAs of tile t from LDS stage 0
    //            stage set 2 (tile t+1) into LDS stage 1       its q-th store needs the q-th oldest load: loads return in
    //                                                          order, so the wait is vmcnt(2 L - 1 - q) ... vmcnt(L) --
    //                                                          never below L, set 1's loads stay outstanding
    //            lgkmcnt(0) (this wave's LDS stores), barrier  outstanding across the barrier: set 1 (tile t+2) = L
    //   half 1:  the same with the sets and the LDS stages swapped, tile t+3 issued, tile t+2 staged.
    // The compiler places these waits itself (the loads are ordinary loads, __syncthreads() with no LDS-DMA outstanding
    // is `s_waitcnt lgkmcnt(0); s_barrier`), but it places them for the worst path that reaches the store: where a half
    // can be entered without its loads having been issued (`if (t + 2 < ntiles) load ...`, the general loop further
    // down), the stores of the other set wait as if nothing had been issued after it -- vmcnt(L - 1) ... vmcnt(0) --
    // and every half ends with nothing in flight: a one-deep pipeline at the registers of a two-deep one.
    // Hence the interior loop: while tiles t+2 and t+3 exist and are full, and both operands are on the strided
    // loader, both halves are straight-line code in which every load is issued on every path. The general loop takes
    // over for the last two to four tiles (two or three full ones and a partial one, if any), for the tiles on the
    // ragged edge of a not-contiguous operand and for a gathered A, in the state the interior loop leaves: tile t in
    // LDS stage 0, tile t+1 in set 2. The k-weighted tile (WK, gram_weighted) never enters the interior loop: it is
    // DEEP only up to 64 columns, and its transposed A operand then never fills the 128 rows of a tile (a_fast is
    // false); the doubly modulated one (MOD2) is kept off it, see below.
    // deep_pin() keeps the compiler from moving the phases of a half across each other: left to itself it hoists the
    // staging stores of half 0 above the MFMAs, sinks the loads below them and runs the MFMAs of both tiles in half 1
    // -- correct, with exact waits, and as slow as the drained loop (GEMM_DEEP_PIN=0).
    // The arithmetic, its order and the LDS images are those of the general loop.
    double ra2[BM / 16];
    double rb2[BN / 16];
    double rs2[MQ];
    auto load_into = [&](int k0, double (&xa)[BM / 16], double (&xb)[BN / 16], double (&xs)[MQ]) {
      const bool full = k0 + BK <= kend;
      if (full && a_fast) tile_load_strided<BM>(pa, sa, xa);
      else tile_load<A_CONTIG, BM, GATHER>(g.A, g.lda, m0, k0, g.M, kend, xa, g.kidx);
      if (full && b_fast) tile_load_strided<BN>(pb, sb, xb);
      else tile_load<B_CONTIG, BN>(g.B, g.ldb, n0, k0, g.N, kend, xb);
      if constexpr (MOD || WK) mod_load(k0, xs);
      pa += ia;
      pb += ib;
    };
    auto stage = [&](int k0, int st, double (&xa)[BM / 16], double (&xb)[BN / 16], const double (&xs)[MQ]) {
      if constexpr (MOD || WK) mod_apply(xa, xs);
      if (k0 + BK > kend) {
        tile_zero_ktail<A_CONTIG, BM>(k0, kend, xa);
        tile_zero_ktail<B_CONTIG, BN>(k0, kend, xb);
      }
      tile_store<A_CONTIG, BM>(smem + st * A_STAGE, xa);
      tile_store<B_CONTIG, BN>(smem + B_BASE + st * B_STAGE, xb);
    };
    load_into(kbeg, ra, rb, rs);
    stage(kbeg, 0, ra, rb, rs);
    if (ntiles > 1) load_into(kbeg + BK, ra2, rb2, rs2);
    __syncthreads();
    int t = 0;
    // (not the doubly modulated tile: with the interior loop gemm_modulated2_kernel<64>, at 256 VGPRs, spills)
    if (!MOD2 && !WK && a_fast && b_fast) {
      auto load_full = [&](double (&xa)[BM / 16], double (&xb)[BN / 16], double (&xs)[MQ]) {
        tile_load_strided<BM>(pa, sa, xa);
        tile_load_strided<BN>(pb, sb, xb);
        if constexpr (MOD) {              // (mod_load's full-tile branch, without its test)
#pragma unroll
          for (int q = 0; q < MQ1; ++q) xs[q] = ps[q * (NT / BM)];
          ps += BK;
        }
        pa += ia;
        pb += ib;
      };
      auto stage_full = [&](int st, double (&xa)[BM / 16], double (&xb)[BN / 16], const double (&xs)[MQ]) {
        if constexpr (MOD) mod_apply(xa, xs);
        tile_store<A_CONTIG, BM>(smem + st * A_STAGE, xa);
        tile_store<B_CONTIG, BN>(smem + B_BASE + st * B_STAGE, xb);
      };
      auto deep_pin = [] {
#if GEMM_DEEP_PIN
        __builtin_amdgcn_sched_barrier(0);
#endif
      };
      const int nfull = (kend - kbeg) / BK;
      for (; t + 3 < nfull; t += 2) {
        load_full(ra, rb, rs);            // tile t+2; in flight: tile t+1 (set 2), tile t+2 (set 1)
        deep_pin();
        mfma_tile(0);
        deep_pin();
        stage_full(1, ra2, rb2, rs2);     // waits for set 2 only: set 1's loads stay outstanding
        __syncthreads();                  // in flight across the barrier: tile t+2
        load_full(ra2, rb2, rs2);         // tile t+3; in flight: tile t+2 (set 1), tile t+3 (set 2)
        deep_pin();
        mfma_tile(1);
        deep_pin();
        stage_full(0, ra, rb, rs);        // waits for set 1 only
        __syncthreads();                  // in flight across the barrier: tile t+3
      }
    }
    for (; t < ntiles; t += 2) {
      // even tile t: LDS stage 0; tile t+1 waits in (ra2, rb2); tile t+2 loads into (ra, rb)
      if (t + 2 < ntiles) load_into(kbeg + (t + 2) * BK, ra, rb, rs);
      mfma_tile(0);
      if (t + 1 < ntiles) stage(kbeg + (t + 1) * BK, 1, ra2, rb2, rs2);
      __syncthreads();
      if (t + 1 >= ntiles) break;
      // odd tile t+1: LDS stage 1; tile t+2 waits in (ra, rb); tile t+3 loads into (ra2, rb2)
      if (t + 3 < ntiles) load_into(kbeg + (t + 3) * BK, ra2, rb2, rs2);
      mfma_tile(1);
      if (t + 2 < ntiles) stage(kbeg + (t + 2) * BK, 0, ra, rb, rs);
      __syncthreads();
    }
    return;
  }

  load_tiles(kbeg);
  if constexpr (MOD || WK) mod_apply(ra, rs);
  if (kbeg + BK > kend) {
    tile_zero_ktail<A_CONTIG, BM>(kbeg, kend, ra);
    tile_zero_ktail<B_CONTIG, BN>(kbeg, kend, rb);
  }
  tile_store<A_CONTIG, BM>(smem, ra);
  tile_store<B_CONTIG, BN>(smem + B_BASE, rb);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    const int k0 = kbeg + (t + 1) * BK;
    if (t + 1 < ntiles) load_tiles(k0);
    mfma_tile(cur);
    if (t + 1 < ntiles) {
      if constexpr (MOD || WK) mod_apply(ra, rs);
      if (k0 + BK > kend) {  // partial last tile: k rows past the end must contribute zeros
        tile_zero_ktail<A_CONTIG, BM>(k0, kend, ra);
        tile_zero_ktail<B_CONTIG, BN>(k0, kend, rb);
      }
      tile_store<A_CONTIG, BM>(smem + (cur ^ 1) * A_STAGE, ra);
      tile_store<B_CONTIG, BN>(smem + B_BASE + (cur ^ 1) * B_STAGE, rb);
    }
    __syncthreads();
  }
}

// Visit every accumulator element owned by this lane: f(m, n, value).
template <int BN, class F>
__device__ __forceinline__ void acc_foreach(const d4 (&acc)[4][BN / 32], int m0, int n0, F f) {
  constexpr int NJ = BN / 32;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = (wave & 1) * 64;
  const int wn = (wave >> 1) * (BN / 2);
  const int lm = lane & 15;
  const int lk = lane >> 4;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm + i * 16 + lm;
        const int n = n0 + wn + j * 16 + lk + 4 * r;
        f(m, n, acc[i][j][r]);
      }
}

// The shared frame of the plain GEMM family. (Scalars arrive by reference: a helper that receives them by value is
// unrolled before it is inlined, which moves the register allocation of the kernels around it.)
// The k slab of a workgroup of a (tiles, splits) grid: slab z = blockIdx.y covers k in [kbeg, kend).
struct KSlab { int z, kbeg, kend; };
__device__ __forceinline__ KSlab k_slab(const int& K, const int& k_chunk) {
  const int z = blockIdx.y;
  const int kbeg = z * k_chunk;
  return KSlab{z, kbeg, min(K, kbeg + k_chunk)};
}
// ... and its tile of the tiles_m x tiles_n grid of 128 x BN tiles, column by column in the XCD-aware order.
struct TileAt { int tn, m0, n0, z, kbeg, kend; };
template <int BN>
__device__ __forceinline__ TileAt tile_at(const GemmOperands& g, const int& tiles_m, const int& tiles_n, const int& k_chunk) {
  const int ntile = tiles_m * tiles_n;
  const int tid = xcd_remap(blockIdx.x, ntile);
  const int tm = tid % tiles_m, tn = tid / tiles_m;
  const int m0 = tm * BM, n0 = tn * BN;
  const KSlab s = k_slab(g.K, k_chunk);
  return TileAt{tn, m0, n0, s.z, s.kbeg, s.kend};
}

// (The stores "m < M && n < N: C or the slab" stay spelled out in each kernel: through a shared helper the compiler
//  schedules them differently, and gemm_modulated2_kernel<128> measured 0.7 % slower)

// Sum of count slabs' entries p[0], p[stride], ... in the fixed order z = 0, 1, ... (deterministic); the loads of four
// slabs are issued together -- with one load in flight per thread a reduction is latency-bound.
__device__ __forceinline__ double slab_sum(const double* __restrict__ p, const int64_t& stride, const int& count) {
  double s = 0.0;
  int z = 0;
  for (; z + 4 <= count; z += 4) {
    const double a0 = p[(int64_t)(z + 0) * stride], a1 = p[(int64_t)(z + 1) * stride];
    const double a2 = p[(int64_t)(z + 2) * stride], a3 = p[(int64_t)(z + 3) * stride];
    s += a0; s += a1; s += a2; s += a3;
  }
  for (; z < count; ++z) s += p[(int64_t)z * stride];
  return s;
}

constexpr size_t smem_bytes(int bn) { return (size_t)(2 * lds_stage(BM) + 2 * lds_stage(bn)) * sizeof(double); }
constexpr size_t smem_bytes_nt(int bn) {   // op(A) = A, op(B) = B': both tiles x-contiguous
  return (size_t)(2 * lds_stage_of(true, BM) + 2 * lds_stage_of(true, bn)) * sizeof(double);
}

// (xcd_remap, the XCD-aware tile order of every kernel here: csrc/syrkmap.h)

// ---------------------------------------------------------------------------
// plain GEMM kernels
// ---------------------------------------------------------------------------
// workgroups per CU of gemm_kernel<TA, TB, BN>: the N,N kernel with 64-wide tiles (A22 V of stage 1, K B_j of the
// block Lanczos) fits three with the layout-exact LDS stages when it gives up the second k-tile in flight
#ifndef GEMM_NN64_OCC
#define GEMM_NN64_OCC 2
#endif
template <bool TA, bool TB, int BN>
constexpr int gemm_occ() { return (!TA && !TB && BN == 64) ? GEMM_NN64_OCC : GEMM_OCC; }
template <bool TA, bool TB, int BN>
constexpr size_t gemm_smem_bytes() {
  return gemm_occ<TA, TB, BN>() > GEMM_OCC
             ? (size_t)(2 * lds_stage_of(!TA, BM) + 2 * lds_stage_of(TB, BN)) * sizeof(double)
             : smem_bytes(BN);
}
template <bool TA, bool TB, int BN>
__global__ __launch_bounds__(NT, (gemm_occ<TA, TB, BN>())) void gemm_kernel(GemmOperands g, double alpha, double beta,
                                                  double* __restrict__ C, int64_t ldc,
                                                  int tiles_m, int tiles_n, int k_chunk,
                                                  double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  if (g.run_if != nullptr && *g.run_if == 0) return;      // (uniform: a scalar load)
  const TileAt at = tile_at<BN>(g, tiles_m, tiles_n, k_chunk);
  const int m0 = at.m0, n0 = at.n0;
  d4 acc[4][BN / 32];
  gemm_tile<TA, TB, BN, false, (BN <= GEMM_DEEP_BN && gemm_occ<TA, TB, BN>() <= GEMM_OCC)>(g, m0, n0, at.kbeg, at.kend, smem, acc);
  const int M = g.M, N = g.N;
  if (partial != nullptr) {
    double* P = partial + (int64_t)at.z * M * N;
    acc_foreach<BN>(acc, m0, n0, [&](int m, int n, double v) {
      if (m < M && n < N) P[(int64_t)m + (int64_t)n * M] = v;
    });
  } else {
    if (beta == 0.0) {
      acc_foreach<BN>(acc, m0, n0, [&](int m, int n, double v) {
        if (m < M && n < N) C[(int64_t)m + (int64_t)n * ldc] = alpha * v;
      });
    } else {
      // read-modify-write: fetch every C value of the lane in one batch, then combine and store
      constexpr int NJ = BN / 32;
      const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
      const int wm = (wave & 1) * 64, wn = (wave >> 1) * (BN / 2);
      const int lm = lane & 15, lk = lane >> 4;
      // one 64 x 16 column strip at a time, software pipelined: the loads of strip j+1 are
      // issued before the stores of strip j (vmcnt is in-order over loads and stores, so loads
      // issued after a strip's stores would also wait for those stores to retire)
      auto load_strip = [&](int j, d4 (&cold)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm + i * 16 + lm, n = n0 + wn + j * 16 + lk + 4 * r;
            cold[i][r] = (m < M && n < N) ? C[(int64_t)m + (int64_t)n * ldc] : 0.0;
          }
      };
      d4 cold[2][4];
      load_strip(0, cold[0]);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (j + 1 < NJ) load_strip(j + 1, cold[(j + 1) & 1]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int m = m0 + wm + i * 16 + lm, n = n0 + wn + j * 16 + lk + 4 * r;
            if (m < M && n < N)
              C[(int64_t)m + (int64_t)n * ldc] = alpha * acc[i][j][r] + beta * cold[j & 1][i][r];
          }
      }
    }
  }
}

__global__ void splitk_reduce_kernel(const double* __restrict__ partial, int splits, int M, int N,
                                     double alpha, double beta, double* __restrict__ C,
                                     int64_t ldc, const int* __restrict__ run_if) {
  if (run_if != nullptr && *run_if == 0) return;
  const int64_t total = (int64_t)M * N;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const double s = slab_sum(partial + e, total, splits);
    const int m = (int)(e % M), n = (int)(e / M);
    const int64_t o = (int64_t)m + (int64_t)n * ldc;
    C[o] = (beta == 0.0) ? alpha * s : alpha * s + beta * C[o];
  }
}

// ---- host frame of the family ---------------------------------------------------------------------------------------
// The deterministic split-K choice (csrc/splitplan.h) of a launch of ntile tiles under one of the three models.
// (development: BIGKRLS_GEMM_SPLITS=<n> overrides the count for products with K >= 16384 under the plain model,
//  tools/kb_shape_probe.hip)
static int gemm_env_splits() {
  static const int env_splits = [] { const char* e = getenv("BIGKRLS_GEMM_SPLITS"); return e ? atoi(e) : 0; }();
  return env_splits;
}
static SplitPlan gemm_split_plan(const SplitModel& md, const GemmOperands& g, int ntile) {
  return split_plan(md, ntile, g.M, g.N, g.K, BK, gemm_env_splits());
}

// GEMMs issued on the look-ahead stream run concurrently with main-stream GEMMs: own partial buffer
static int gemm_split_slot(const bigkrls_ctx* ctx) {
  return (ctx->side_stream && (ctx->stream == ctx->side_stream || ctx->stream == ctx->bg_stream)) ? SLOT_SIDE_SPLITK : SLOT_GEMM_SPLITK;
}

// tile width of an n-column result: f(std::integral_constant<int, BN>), BN = 32, 64 or 128
template <class F>
static auto with_bn(int64_t n, F&& f) {
  if (n <= 32) return f(std::integral_constant<int, 32>());
  if (n <= 64) return f(std::integral_constant<int, 64>());
  return f(std::integral_constant<int, 128>());
}

// the first two checks of every entry (c: a third dimension, or 0)
static int require_dims(const char* who, int64_t a, int64_t b, int64_t c = 0) {
  BK_REQUIRE(a >= 0 && b >= 0 && c >= 0, std::string(who) + ": negative dimension");
  BK_REQUIRE(a < (1ll << 31) && b < (1ll << 31) && c < (1ll << 31), std::string(who) + ": dimension too large");
  return BIGKRLS_OK;
}

__global__ void scale_matrix_kernel(double* C, int64_t ldc, int M, int N, double beta) {
  const int64_t total = (int64_t)M * N;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o = (e % M) + (e / M) * ldc;
    C[o] = (beta == 0.0) ? 0.0 : beta * C[o];
  }
}
// C (m x n) = beta C, C not read for beta == 0
static int scale_matrix(bigkrls_ctx* ctx, double* C, int64_t ldc, int64_t m, int64_t n, double beta) {
  const int blocks = (int)std::min<int64_t>((m * n + 255) / 256, 2048);
  hipLaunchKernelGGL(scale_matrix_kernel, dim3(blocks), dim3(256), 0, ctx->stream, C, ldc, (int)m, (int)n, beta);
  BK_CHECK_LAUNCH();
  return BIGKRLS_OK;
}
// an empty sum
static int zero_fill(bigkrls_ctx* ctx, double* C, int64_t ldc, int64_t m, int64_t n) { return scale_matrix(ctx, C, ldc, m, n, 0.0); }

// partial (splits slabs of m x n) -> C = alpha (sum of the slabs) + beta C
static int launch_splitk_reduce(bigkrls_ctx* ctx, const double* partial, int splits, int m, int n, double alpha, double beta,
                                double* C, int64_t ldc, const int* run_if) {
  const int blocks = (int)std::min<int64_t>(((int64_t)m * n + 255) / 256, 2048);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, ctx->stream, partial, splits, m, n, alpha, beta, C,
                     ldc, run_if);
  BK_CHECK_LAUNCH();
  return BIGKRLS_OK;
}

// One launch of a plain kernel of tile width BN -- gemm_kernel<TA, TB, BN> (pre: alpha, beta) or a modulated kernel
// (TA = TB = false; pre: GemmMod, or GemmMod and GemmMod2) -- over the split plan's (tiles, splits) grid, and for more than
// one split the slabs' reduction C = alpha (sum) + beta C.
// (launch_gemm_planned: the same under a plan made elsewhere -- gemm_thin's, whose slabs are those of another width)
template <bool TA, bool TB, int BN, class Kern, class... Pre>
static int launch_gemm_planned(bigkrls_ctx* ctx, const GemmOperands& g, Kern kern, const SplitPlan& plan, double alpha,
                               double beta, double* C, int64_t ldc, const Pre&... pre);
template <bool TA, bool TB, int BN, class Kern, class... Pre>
static int launch_gemm_splitk(bigkrls_ctx* ctx, const GemmOperands& g, Kern kern, double alpha, double beta, double* C,
                              int64_t ldc, const Pre&... pre) {
  const int ntile = ((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN);
  const SplitPlan plan = gemm_split_plan(split_model_gemm(gemm_occ<TA, TB, BN>()), g, ntile);
  return launch_gemm_planned<TA, TB, BN>(ctx, g, kern, plan, alpha, beta, C, ldc, pre...);
}
template <bool TA, bool TB, int BN, class Kern, class... Pre>
static int launch_gemm_planned(bigkrls_ctx* ctx, const GemmOperands& g, Kern kern, const SplitPlan& plan, double alpha,
                               double beta, double* C, int64_t ldc, const Pre&... pre) {
  const int tiles_m = (g.M + BM - 1) / BM;
  const int tiles_n = (g.N + BN - 1) / BN;
  const int ntile = tiles_m * tiles_n;
  double* partial = nullptr;   // the slabs of the split-K partials (splits x M x N doubles); nullptr for a single split
  if (plan.splits > 1) {
    void* p = nullptr;
    BK_TRY(ws_get(ctx, gemm_split_slot(ctx), (int64_t)plan.splits * g.M * g.N * sizeof(double), &p));
    partial = (double*)p;
  }
  constexpr size_t smem = gemm_smem_bytes<TA, TB, BN>();
  BK_TRY(ensure_dyn_smem(ctx, (const void*)kern, smem));
  hipLaunchKernelGGL(kern, dim3(ntile, plan.splits), dim3(NT), smem, ctx->stream, g, pre..., C, ldc, tiles_m, tiles_n,
                     plan.k_chunk, partial);
  BK_CHECK_LAUNCH();
  if (plan.splits > 1) BK_TRY(launch_splitk_reduce(ctx, partial, plan.splits, g.M, g.N, alpha, beta, C, ldc, g.run_if));
  return BIGKRLS_OK;
}

template <bool TA, bool TB, int BN>
static int launch_gemm(bigkrls_ctx* ctx, const GemmOperands& g, double alpha, double beta, double* C, int64_t ldc) {
  return launch_gemm_splitk<TA, TB, BN>(ctx, g, gemm_kernel<TA, TB, BN>, alpha, beta, C, ldc, alpha, beta);
}

int gemm(bigkrls_ctx* ctx, int ta, int tb, int64_t m, int64_t n, int64_t k, double alpha,
         const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C,
         int64_t ldc) {
  BK_TRY(require_dims("gemm", m, n, k));
  if (m == 0 || n == 0) return BIGKRLS_OK;
  if (k == 0 || alpha == 0.0) return beta == 1.0 ? BIGKRLS_OK : scale_matrix(ctx, C, ldc, m, n, beta);
  BK_REQUIRE(A && B && C, "gemm: null pointer");
  GemmOperands g{A, B, lda, ldb, (int)m, (int)n, (int)k, nullptr, ctx->gemm_run_if};
  return with_bn(n, [&](auto bn) {
    constexpr int BN = decltype(bn)::value;
    if (!ta && !tb) return launch_gemm<false, false, BN>(ctx, g, alpha, beta, C, ldc);
    if (!ta && tb) return launch_gemm<false, true, BN>(ctx, g, alpha, beta, C, ldc);
    if (ta && !tb) return launch_gemm<true, false, BN>(ctx, g, alpha, beta, C, ldc);
    return launch_gemm<true, true, BN>(ctx, g, alpha, beta, C, ldc);
  });
}

// gemm() for a product of few tiles and a long contraction (the stage-1 back-transform's): the same kernels over the same
// k slabs -- thin_plan() (csrc/splitplan.h) keeps gemm()'s (splits, k_chunk) -- with the tile width thin_plan chooses from
// the shape, so that more and shorter workgroups share the arithmetic. Same partial slot, same reduction; bitwise gemm().
// force_bn = 32, 64 or 128: that width (development and tests), else the rule.
template <bool TA, bool TB>
static int launch_gemm_thin(bigkrls_ctx* ctx, const GemmOperands& g, int force_bn, double alpha, double beta, double* C,
                            int64_t ldc) {
  const int occ = with_bn(g.N, [](auto bn) { return gemm_occ<TA, TB, decltype(bn)::value>(); });
  const ThinPlan tp = thin_plan(TA, TB, g.M, g.N, g.K, BM, BK, occ, gemm_env_splits(), force_bn);
  const SplitPlan plan{tp.splits, tp.k_chunk};
  if (tp.bn_exec == 32) return launch_gemm_planned<TA, TB, 32>(ctx, g, gemm_kernel<TA, TB, 32>, plan, alpha, beta, C, ldc, alpha, beta);
  if (tp.bn_exec == 64) return launch_gemm_planned<TA, TB, 64>(ctx, g, gemm_kernel<TA, TB, 64>, plan, alpha, beta, C, ldc, alpha, beta);
  return launch_gemm_planned<TA, TB, 128>(ctx, g, gemm_kernel<TA, TB, 128>, plan, alpha, beta, C, ldc, alpha, beta);
}

int gemm_thin(bigkrls_ctx* ctx, int ta, int tb, int64_t m, int64_t n, int64_t k, double alpha, const double* A, int64_t lda,
              const double* B, int64_t ldb, double beta, double* C, int64_t ldc, int force_bn) {
  BK_TRY(require_dims("gemm_thin", m, n, k));
  if (m == 0 || n == 0) return BIGKRLS_OK;
  if (k == 0 || alpha == 0.0) return beta == 1.0 ? BIGKRLS_OK : scale_matrix(ctx, C, ldc, m, n, beta);
  BK_REQUIRE(A && B && C, "gemm_thin: null pointer");
  GemmOperands g{A, B, lda, ldb, (int)m, (int)n, (int)k, nullptr, ctx->gemm_run_if};
  if (!ta && !tb) return launch_gemm_thin<false, false>(ctx, g, force_bn, alpha, beta, C, ldc);
  if (!ta && tb) return launch_gemm_thin<false, true>(ctx, g, force_bn, alpha, beta, C, ldc);
  if (ta && !tb) return launch_gemm_thin<true, false>(ctx, g, force_bn, alpha, beta, C, ldc);
  return launch_gemm_thin<true, true>(ctx, g, force_bn, alpha, beta, C, ldc);
}

// ---------------------------------------------------------------------------
// C (M x N) = (A o (r 1' + t s')) B, A and B not transposed: the plain N,N kernel of the same width with A modulated
// on its way to LDS (gemm_tile<.., MOD>), so the modulated copy of A -- G_j = Kn o (r 1' + t s') of the pointwise
// standard errors of the marginal effects, csrc/margeff.hip -- is never written. Same tiles, same occupancy, same k
// pipeline and same split-K choice as gemm_kernel<false, false, BN>; the product is linear in the modulated operand,
// so the splits' partials add in slab order as before (splitk_reduce_kernel: no atomics, bitwise reproducible).
// With r = 1, t = 0 the factor is exactly 1 and the result is bitwise gemm()'s.
// ---------------------------------------------------------------------------
// (the one body of gemm_modulated_kernel and gemm_modulated2_kernel; MOD2 off: mod2 is never read)
template <int BN, bool MOD2>
__device__ __forceinline__ void gemm_modulated_body(const GemmOperands& g, const GemmMod& mod, const GemmMod2* mod2,
                                                    double* __restrict__ C, const int64_t& ldc, const int& tiles_m,
                                                    const int& tiles_n, const int& k_chunk, double* __restrict__ partial,
                                                    double* __restrict__ smem) {
  const TileAt at = tile_at<BN>(g, tiles_m, tiles_n, k_chunk);
  d4 acc[4][BN / 32];
  gemm_tile<false, false, BN, false, (BN <= GEMM_DEEP_BN && gemm_occ<false, false, BN>() <= GEMM_OCC), true, false, MOD2>(
      g, at.m0, at.n0, at.kbeg, at.kend, smem, acc, &mod, nullptr, mod2);
  const int M = g.M, N = g.N;
  if (partial != nullptr) {
    double* P = partial + (int64_t)at.z * M * N;
    acc_foreach<BN>(acc, at.m0, at.n0, [&](int m, int n, double v) {
      if (m < M && n < N) P[(int64_t)m + (int64_t)n * M] = v;
    });
  } else {
    acc_foreach<BN>(acc, at.m0, at.n0, [&](int m, int n, double v) {
      if (m < M && n < N) C[(int64_t)m + (int64_t)n * ldc] = v;
    });
  }
}

template <int BN>
__global__ __launch_bounds__(NT, (gemm_occ<false, false, BN>())) void gemm_modulated_kernel(
    GemmOperands g, GemmMod mod, double* __restrict__ C, int64_t ldc, int tiles_m, int tiles_n, int k_chunk,
    double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  gemm_modulated_body<BN, false>(g, mod, nullptr, C, ldc, tiles_m, tiles_n, k_chunk, partial, smem);
}

// the shared host frame of gemm_modulated and gemm_modulated2 (kern(bn): the kernel of tile width bn; mods: its GemmMod,
// or its GemmMod and GemmMod2)
template <class KernOf, class... Mods>
static int gemm_modulated_entry(bigkrls_ctx* ctx, const char* who, int64_t m, int64_t n, int64_t k, const double* A,
                                int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, bool vectors_ok,
                                KernOf kern_of, const Mods&... mods) {
  const std::string name(who);
  BK_TRY(require_dims(who, m, n, k));
  if (m == 0 || n == 0) return BIGKRLS_OK;
  BK_REQUIRE(C && ldc >= m, name + ": null C or ldc < m");
  if (k == 0) return zero_fill(ctx, C, ldc, m, n);   // empty sum
  BK_REQUIRE(A && B && vectors_ok, name + ": null pointer");
  BK_REQUIRE(lda >= m && ldb >= k, name + ": leading dimension of A or B too small");
  const GemmOperands g{A, B, lda, ldb, (int)m, (int)n, (int)k, nullptr};
  BK_TRY(prof_begin(ctx, who, 2.0 * (double)m * (double)n * (double)k));
  BK_TRY(with_bn(n, [&](auto bn) {
    constexpr int BN = decltype(bn)::value;
    return launch_gemm_splitk<false, false, BN>(ctx, g, kern_of(bn), 1.0, 0.0, C, ldc, mods...);
  }));
  BK_TRY(prof_end(ctx, who));
  return BIGKRLS_OK;
}

int gemm_modulated(bigkrls_ctx* ctx, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda, const double* r,
                   const double* t, const double* s, const double* B, int64_t ldb, double* C, int64_t ldc) {
  return gemm_modulated_entry(ctx, "gemm_modulated", m, n, k, A, lda, B, ldb, C, ldc, r && t && s,
                              [](auto bn) { return gemm_modulated_kernel<decltype(bn)::value>; }, GemmMod{r, t, s});
}

// ---------------------------------------------------------------------------
// C (M x N) = (A o F) B, F[i,l] = fma(fma(t1[i], s1[l], r1[i]), fma(t2[i], s2[l], r2[i]), d): gemm_modulated with the
// product of two modulations plus a constant as the factor (gemm_tile<.., MOD, .., MOD2>), so the doubly modulated
// copy of A -- G_jk = Kn o m_j o m_k - (2/sigma) delta_jk Kn of the pointwise standard errors of the interaction
// effects, csrc/inteff.hip -- is never written. Tiles, occupancy, k pipeline and split-K choice are gemm_modulated's;
// per thread two more row scalars and, per k-tile in flight, BM / 16 more s values live across the k loop.
// With r2 = 1, t2 = 0, d = 0 the second factor is exactly 1 and the result is bitwise gemm_modulated's.
// ---------------------------------------------------------------------------
template <int BN>
__global__ __launch_bounds__(NT, (gemm_occ<false, false, BN>())) void gemm_modulated2_kernel(
    GemmOperands g, GemmMod mod, GemmMod2 mod2, double* __restrict__ C, int64_t ldc, int tiles_m, int tiles_n,
    int k_chunk, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  gemm_modulated_body<BN, true>(g, mod, &mod2, C, ldc, tiles_m, tiles_n, k_chunk, partial, smem);
}

int gemm_modulated2(bigkrls_ctx* ctx, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda, const double* r1,
                    const double* t1, const double* s1, const double* r2, const double* t2, const double* s2, double d,
                    const double* B, int64_t ldb, double* C, int64_t ldc) {
  return gemm_modulated_entry(ctx, "gemm_modulated2", m, n, k, A, lda, B, ldb, C, ldc, r1 && t1 && s1 && r2 && t2 && s2,
                              [](auto bn) { return gemm_modulated2_kernel<decltype(bn)::value>; }, GemmMod{r1, t1, s1},
                              GemmMod2{r2, t2, s2, d});
}

// ---------------------------------------------------------------------------
// M (k x k) = A' diag(omega) A, A n x k column-major: the weighted Gram matrix of the sandwich variance
// (csrc/robust.hip). The T,N form of gemm_tile has both operands contiguous along the contraction; the weight is
// applied to the A-side tile in registers on its way to LDS (gemm_tile<.., WK>), so diag(omega) A is never written.
// Only the tiles on or below the diagonal are computed (k <= 64: the one BN-wide tile; else 128 x 128 tiles), and of
// those only the entries with row >= column are used: each is written to (i, j) and to (j, i), inside diagonal tiles
// too, so the result is symmetric bit for bit. The contraction is n long against a handful of tiles, so it is split
// over n by gemm_split_plan, taken over the computed tiles; the slabs (one 128 x BN block per tile and split) are
// summed in slab order by gram_reduce_kernel: no atomics, two calls give the same bits.
// ---------------------------------------------------------------------------
template <int BN>
__global__ __launch_bounds__(NT, (gemm_occ<true, false, BN>())) void gram_weighted_kernel(
    GemmOperands g, const double* __restrict__ omega, double* __restrict__ C, int64_t ldc, int T, int ntile, int k_chunk,
    double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int t = xcd_remap(blockIdx.x, ntile);
  const LowerTile lt = lower_tile_of(t, T);   // csrc/syrkmap.h
  const int m0 = lt.tm * BM, n0 = lt.tn * BN;   // (T > 1 only with BN == BM)
  const KSlab ks = k_slab(g.K, k_chunk);
  d4 acc[4][BN / 32];
  gemm_tile<true, false, BN, false, (BN <= GEMM_DEEP_BN), false, true>(g, m0, n0, ks.kbeg, ks.kend, smem, acc, nullptr, omega);
  const int M = g.M;
  if (partial != nullptr) {
    double* P = partial + ((int64_t)ks.z * ntile + t) * (BM * BN);
    acc_foreach<BN>(acc, m0, n0, [&](int m, int n, double v) {
      if (m < M && n < M && m >= n) P[(m - m0) + (n - n0) * BM] = v;
    });
  } else {
    acc_foreach<BN>(acc, m0, n0, [&](int m, int n, double v) {
      if (m < M && n < M && m >= n) {
        C[(int64_t)m + (int64_t)n * ldc] = v;
        C[(int64_t)n + (int64_t)m * ldc] = v;
      }
    });
  }
}

// BM * bn / 256 workgroups per tile, all in grid.x (the tile count T (T + 1) / 2 passes the 65 535 of grid.y near
// k = 46 000); the slabs of an entry in the fixed order z = 0, 1, ...
__global__ void gram_reduce_kernel(const double* __restrict__ partial, int splits, int ntile, int T, int bn, int M,
                                   double* __restrict__ C, int64_t ldc) {
  const int per_tile = BM * bn;
  const int wg_per_tile = per_tile / 256;
  const int t = blockIdx.x / wg_per_tile;
  const LowerTile lt = lower_tile_of(t, T);
  const int m0 = lt.tm * BM, n0 = lt.tn * bn;
  const int e = (blockIdx.x % wg_per_tile) * 256 + threadIdx.x;
  const int m = m0 + e % BM, n = n0 + e / BM;
  if (m >= M || n >= M || m < n) return;
  const double s = slab_sum(partial + (int64_t)t * per_tile + e, (int64_t)ntile * per_tile, splits);
  C[(int64_t)m + (int64_t)n * ldc] = s;
  C[(int64_t)n + (int64_t)m * ldc] = s;
}

template <int BN>
static int launch_gram_weighted(bigkrls_ctx* ctx, const GemmOperands& g, const double* omega, double* C, int64_t ldc) {
  const int T = (g.M + BN - 1) / BN;            // BN < BM only for g.M <= BN: one tile
  BK_REQUIRE((int64_t)T * (T + 1) / 2 * (BM * BN / 256) < (1ll << 31), "gram_weighted: k too large (too many tiles)");
  const int ntile = T * (T + 1) / 2;
  const SplitPlan plan = gemm_split_plan(split_model_gemm(gemm_occ<true, false, BN>()), g, ntile);
  const int splits = plan.splits;
  double* partial = nullptr;
  if (splits > 1) {
    void* p = nullptr;
    BK_TRY(ws_get(ctx, gemm_split_slot(ctx), (int64_t)splits * ntile * BM * BN * (int64_t)sizeof(double), &p));
    partial = (double*)p;
  }
  auto kern = gram_weighted_kernel<BN>;
  constexpr size_t smem = gemm_smem_bytes<true, false, BN>();
  BK_TRY(ensure_dyn_smem(ctx, (const void*)kern, smem));
  hipLaunchKernelGGL(kern, dim3(ntile, splits), dim3(NT), smem, ctx->stream, g, omega, C, ldc, T, ntile, plan.k_chunk, partial);
  BK_CHECK_LAUNCH();
  if (splits > 1) {
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)(ntile * (BM * BN / 256))), dim3(256), 0, ctx->stream, (const double*)partial,
                       splits, ntile, T, BN, g.M, C, ldc);
    BK_CHECK_LAUNCH();
  }
  return BIGKRLS_OK;
}

int gram_weighted(bigkrls_ctx* ctx, int64_t n, int64_t k, const double* A, int64_t lda, const double* omega, double* M,
                  int64_t ldm) {
  BK_TRY(require_dims("gram_weighted", n, k));
  if (k == 0) return BIGKRLS_OK;
  BK_REQUIRE(M && ldm >= k, "gram_weighted: null M or leading dimension of M too small");
  if (n == 0) return zero_fill(ctx, M, ldm, k, k);   // empty sum
  BK_REQUIRE(A && omega, "gram_weighted: null pointer");
  BK_REQUIRE(lda >= n, "gram_weighted: leading dimension of A too small");
  const GemmOperands g{A, A, lda, lda, (int)k, (int)k, (int)n, nullptr};
  BK_TRY(prof_begin(ctx, "gram_weighted", (double)n * (double)k * ((double)k + 1.0)));
  BK_TRY(with_bn(k, [&](auto bn) { return launch_gram_weighted<decltype(bn)::value>(ctx, g, omega, M, ldm); }));
  BK_TRY(prof_end(ctx, "gram_weighted"));
  return BIGKRLS_OK;
}

// ---------------------------------------------------------------------------
// diagonal of a quadratic form (pointwise predict, bigkrls_predict_pointwise in csrc/fit.hip)
// ---------------------------------------------------------------------------
// out[i] = sum_j (A V)[i,j] A[i,j] = diag(A V A'), A m x n, V n x n general (not assumed symmetric), both column-major.
// The product A V runs through gemm_tile<false, false, BN> exactly as gemm_kernel does; only the epilogue differs. Each
// lane multiplies its accumulators by A at the same (row, column) and sums over its columns; the four lanes that share
// a row (lane >> 4) are added with shuffles and the two waves that share a row half through LDS, in a fixed order.
// Each workgroup writes one partial per row: part[(z tiles_n + tn) M + row]. The dot with A is linear in the product,
// so the k splits' partials are dotted and added like the column tiles' (quadform_reduce_kernel, fixed order: no
// atomics, bitwise reproducible). Extra memory: splits x tiles_n x m doubles, never the m x n product.
template <int BN>
__global__ __launch_bounds__(NT, (gemm_occ<false, false, BN>())) void quadform_diag_kernel(
    GemmOperands g, int tiles_m, int tiles_n, int k_chunk, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const TileAt at = tile_at<BN>(g, tiles_m, tiles_n, k_chunk);
  const int m0 = at.m0, n0 = at.n0, tn = at.tn, z = at.z;
  d4 acc[4][BN / 32];
  gemm_tile<false, false, BN, false, (BN <= GEMM_DEEP_BN && gemm_occ<false, false, BN>() <= GEMM_OCC)>(g, m0, n0, at.kbeg,
                                                                                                       at.kend, smem, acc);
  constexpr int NJ = BN / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave & 1) * 64, wn = (wave >> 1) * (BN / 2);
  const int lm = lane & 15, lk = lane >> 4;
  const int M = g.M, N = g.N;
  // register r of acc[i][j] is (m0 + wm + 16 i + lm, n0 + wn + 16 j + lk + 4 r), as in acc_foreach; columns past N
  // hold products with clamped (finite) operand columns and are weighted by 0, rows past M are never written
  double s[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm + i * 16 + lm;
    const double* arow = g.A + (m < M ? m : M - 1);
    double a[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn + j * 16 + lk + 4 * r;
        a[j][r] = n < N ? arow[(int64_t)n * g.lda] : 0.0;
      }
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) t = fma(acc[i][j][r], a[j][r], t);
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
    s[i] = t;
  }
  // gemm_tile ends on a barrier after its last LDS read; this one is for the early return of an empty k range
  __syncthreads();
  double* red = smem;   // [wave][64 rows of the wave's half]
  if (lk == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave * 64 + i * 16 + lm] = s[i];
  }
  __syncthreads();
  if (threadIdx.x < BM) {
    const int r = threadIdx.x, h = r >> 6, rr = r & 63;       // waves h and h + 2 own rows [64 h, 64 h + 64)
    const int m = m0 + r;
    if (m < M) part[((int64_t)z * tiles_n + tn) * M + m] = red[h * 64 + rr] + red[(h + 2) * 64 + rr];
  }
}

// out[i] = sum over q = z tiles_n + tn of part[q M + i], in the order q = 0, 1, ...
__global__ void quadform_reduce_kernel(const double* __restrict__ part, int nparts, int M, double* __restrict__ out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x)
    out[i] = slab_sum(part + i, M, nparts);
}

template <int BN>
static int launch_quadform_diag(bigkrls_ctx* ctx, const GemmOperands& g, double* out) {
  const int tiles_m = (g.M + BM - 1) / BM;
  const int tiles_n = (g.N + BN - 1) / BN;
  const int ntile = tiles_m * tiles_n;
  const SplitPlan plan = gemm_split_plan(split_model_quadform(gemm_occ<false, false, BN>()), g, ntile);
  const int nparts = plan.splits * tiles_n;
  void* p = nullptr;
  BK_TRY(ws_get(ctx, SLOT_QF_PART, (int64_t)nparts * g.M * (int64_t)sizeof(double), &p));
  auto kern = quadform_diag_kernel<BN>;
  constexpr size_t smem = gemm_smem_bytes<false, false, BN>();
  static_assert(smem >= 4 * 64 * sizeof(double), "quadform_diag_kernel: LDS too small for the row reduction");
  BK_TRY(ensure_dyn_smem(ctx, (const void*)kern, smem));
  hipLaunchKernelGGL(kern, dim3(ntile, plan.splits), dim3(NT), smem, ctx->stream, g, tiles_m, tiles_n, plan.k_chunk,
                     (double*)p);
  BK_CHECK_LAUNCH();
  const int blocks = std::min((g.M + 255) / 256, 2048);
  hipLaunchKernelGGL(quadform_reduce_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const double*)p, nparts, g.M,
                     out);
  BK_CHECK_LAUNCH();
  return BIGKRLS_OK;
}

int quadform_diag(bigkrls_ctx* ctx, int64_t m, int64_t n, const double* A, int64_t lda, const double* V, int64_t ldv,
                  double* out) {
  BK_TRY(require_dims("quadform_diag", m, n));
  if (m == 0) return BIGKRLS_OK;
  BK_REQUIRE(out, "quadform_diag: null pointer");
  if (n == 0) {   // empty sum
    BK_HIP(hipMemsetAsync(out, 0, (size_t)m * sizeof(double), ctx->stream));
    return BIGKRLS_OK;
  }
  BK_REQUIRE(A && V, "quadform_diag: null pointer");
  BK_REQUIRE(lda >= m && ldv >= n, "quadform_diag: leading dimension of A or V too small");
  GemmOperands g{A, V, lda, ldv, (int)m, (int)n, (int)n, nullptr};
  BK_TRY(prof_begin(ctx, "quadform_diag", 2.0 * (double)m * (double)n * (double)n + 2.0 * (double)m * (double)n));
  BK_TRY(with_bn(n, [&](auto bn) { return launch_quadform_diag<decltype(bn)::value>(ctx, g, out); }));
  BK_TRY(prof_end(ctx, "quadform_diag"));
  return BIGKRLS_OK;
}

// ---------------------------------------------------------------------------
// Skinny N,N product C (M x N, N <= 48) = A (M x K, m-contiguous) B (K x N): the marginal-effects pass
// K [1, c, x_j, x_j o c ...] (csrc/deriv.hip), whose 2 + 2P operand columns (42 at P = 20) would pay for 64 in the
// 128 x 64 tile of gemm_kernel. Tile 128 x 48 x 16, four waves of 32 rows x 48 columns (2 x 3 MFMA tiles each), two
// k-tiles in flight, split-K into slabs summed by splitk_reduce_kernel in slab order (deterministic).
// ---------------------------------------------------------------------------
constexpr int SK_BN = 48;
constexpr size_t sk48_smem_bytes() { return (size_t)(2 * lds_stage_of(true, BM) + 2 * lds_stage_of(false, SK_BN)) * sizeof(double); }
__global__ __launch_bounds__(NT, 2) void gemm_nn48_kernel(GemmOperands g, int tiles_m, int k_chunk,
                                                         double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int A_STAGE = lds_stage_of(true, BM), B_BASE = 2 * A_STAGE, B_STAGE = lds_stage_of(false, SK_BN);
  constexpr int NJ = SK_BN / 16;
  const int tm = xcd_remap(blockIdx.x, tiles_m);
  const int m0 = tm * BM;
  const KSlab ks = k_slab(g.K, k_chunk);
  const int z = ks.z, kbeg = ks.kbeg, kend = ks.kend;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave * 32, lm = lane & 15, lk = lane >> 4;
  d4 acc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  const int ntiles = (kend - kbeg + BK - 1) / BK;
  const int tid = threadIdx.x;
  const bool b_fast = g.N >= SK_BN;
  const double* pa;
  const double* pb;
  {
    const int gx = m0 + tid % BM;
    pa = g.A + (gx < g.M ? gx : g.M - 1) + (int64_t)(kbeg + tid / BM) * g.lda;
    pb = g.B + (kbeg + (tid & 15)) + (int64_t)(b_fast ? (tid >> 4) : 0) * g.ldb;
  }
  const int64_t sa = (NT / BM) * g.lda, ia = BK * g.lda, sb = 16 * g.ldb;
  double ra[BM / 16], rb[SK_BN / 16], ra2[BM / 16], rb2[SK_BN / 16];
  auto load_into = [&](int k0, double (&xa)[BM / 16], double (&xb)[SK_BN / 16]) {
    const bool full = k0 + BK <= kend;
    if (full) tile_load_strided<BM>(pa, sa, xa);
    else tile_load<true, BM>(g.A, g.lda, m0, k0, g.M, kend, xa);
    if (full && b_fast) tile_load_strided<SK_BN>(pb, sb, xb);
    else tile_load<false, SK_BN>(g.B, g.ldb, 0, k0, g.N, kend, xb);
    pa += ia;
    pb += BK;
  };
  auto stage = [&](int k0, int st, double (&xa)[BM / 16], double (&xb)[SK_BN / 16]) {
    if (k0 + BK > kend) {
      tile_zero_ktail<true, BM>(k0, kend, xa);
      tile_zero_ktail<false, SK_BN>(k0, kend, xb);
    }
    tile_store<true, BM>(smem + st * A_STAGE, xa);
    tile_store<false, SK_BN>(smem + B_BASE + st * B_STAGE, xb);
  };
  auto mfma_tile = [&](int cur) {
    const double* as = smem + cur * A_STAGE;
    const double* bs = smem + B_BASE + cur * B_STAGE;
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      double af[2], bf[NJ];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = as[lds_at<true, BM>(kk + lk, wm + i * 16 + lm)];
#pragma unroll
      for (int j = 0; j < NJ; ++j) bf[j] = bs[lds_at<false, SK_BN>(kk + lk, j * 16 + lm)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(bf[j], af[i], acc[i][j], 0, 0, 0);
    }
  };
  if (ntiles > 0) {
    load_into(kbeg, ra, rb);
    stage(kbeg, 0, ra, rb);
    if (ntiles > 1) load_into(kbeg + BK, ra2, rb2);
    __syncthreads();
    for (int t = 0; t < ntiles; t += 2) {
      if (t + 2 < ntiles) load_into(kbeg + (t + 2) * BK, ra, rb);
      mfma_tile(0);
      if (t + 1 < ntiles) stage(kbeg + (t + 1) * BK, 1, ra2, rb2);
      __syncthreads();
      if (t + 1 >= ntiles) break;
      if (t + 3 < ntiles) load_into(kbeg + (t + 3) * BK, ra2, rb2);
      mfma_tile(1);
      if (t + 2 < ntiles) stage(kbeg + (t + 2) * BK, 0, ra, rb);
      __syncthreads();
    }
  }
  double* P = partial + (int64_t)z * g.M * g.N;
  const int M = g.M, N = g.N;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int m = m0 + wm + i * 16 + lm, n = j * 16 + lk + 4 * r;
        if (m < M && n < N) P[(int64_t)m + (int64_t)n * M] = acc[i][j][r];
      }
}

int gemm_nn_skinny48(bigkrls_ctx* ctx, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda, const double* B,
                     int64_t ldb, double* C, int64_t ldc) {
  BK_REQUIRE(m > 0 && n > 0 && n <= SK_BN && k > 0 && m < (1ll << 31) && k < (1ll << 31) && A && B && C, "gemm_nn_skinny48: bad arguments");
  GemmOperands g{A, B, lda, ldb, (int)m, (int)n, (int)k, nullptr};
  const int tiles_m = (int)((m + BM - 1) / BM);
  // two workgroups per CU: split K so that the grid fills whole rounds of the 512 slots (or as much of one as K allows)
  const SplitPlan plan = gemm_split_plan(split_model_skinny48(), g, tiles_m);
  void* p = nullptr;
  BK_TRY(ws_get(ctx, gemm_split_slot(ctx), (int64_t)plan.splits * m * n * sizeof(double), &p));
  BK_TRY(ensure_dyn_smem(ctx, (const void*)gemm_nn48_kernel, sk48_smem_bytes()));
  hipLaunchKernelGGL(gemm_nn48_kernel, dim3(tiles_m, plan.splits), dim3(NT), sk48_smem_bytes(), ctx->stream, g, tiles_m,
                     plan.k_chunk, (double*)p);
  BK_CHECK_LAUNCH();
  return launch_splitk_reduce(ctx, (const double*)p, plan.splits, (int)m, (int)n, 1.0, 0.0, C, ldc, nullptr);
}

// ---------------------------------------------------------------------------
// symmetric rank-k update of the lower triangle: C(lower) += alpha * A B'
// (A, B are m x k; used by the tridiagonalisation's trailing update
//  A22 -= [V W][W V]', whose consumers only ever read the lower triangle).
// Only tiles with tile_row >= tile_col are launched.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT, GEMM_OCC) void syrk_lower_kernel(GemmOperands g, double alpha,
                                                        double* __restrict__ C, int64_t ldc,
                                                        int tiles) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  // blockIdx.x enumerates the lower-triangular tiles column by column
  const LowerTile lt = lower_tile_of(blockIdx.x, tiles);   // csrc/syrkmap.h
  const int m0 = lt.tm * BM, n0 = lt.tn * 128;
  d4 acc[4][4];
  gemm_tile<false, true, 128>(g, m0, n0, 0, g.K, smem, acc);
  const int M = g.M;
  acc_foreach<128>(acc, m0, n0, [&](int m, int n, double v) {
    if (m < M && n < M && m >= n) {   // (a diagonal tile holds elements above the diagonal: not part of the update)
      const int64_t o = (int64_t)m + (int64_t)n * ldc;
      C[o] += alpha * v;
    }
  });
}

// Same lower-triangular tile set, but the updated values are also mirrored into the upper
// triangle (through a per-wave 16 x 16 LDS transpose so that the mirrored stores are 128-byte
// segments too): C stays a fully stored, exactly symmetric matrix at half the MFMA work of a
// full GEMM update. Used by the band reduction, whose next step is the plain product A22 V.
// ACCUM = false: C = alpha A B' (nothing of C is read): the N x N variance matrices Q diag(w) Q' of the fit.
// Tile order of the mirrored rank-k update. R == 0: column by column from tile t_off (consecutive workgroups =
// consecutive XCDs take consecutive row tiles of one tile column, so every XCD streams the whole A operand through
// its L2 once per tile column). R > 0: XCD-aware, L2-blocked: the tiles of the BN-wide columns [c0, c1) are ordered
// band by band (a band = R consecutive 128-row tiles), inside a band column by column, and every XCD takes a
// contiguous eighth of that sequence (xcd_remap): an XCD keeps the R row panels of A of its band in its L2 and
// walks the columns, so each panel of B is fetched once per band instead of each panel of A once per column.
#ifdef BK_SYRK_TRACE
// development build only (tools/syrk_trace.sh): per-workgroup time stamps of the trailing update (100 MHz clock)
__device__ unsigned long long* g_syrk_trace = nullptr;
extern "C" __attribute__((visibility("default"))) int bk_syrk_trace_set(unsigned long long* p) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_syrk_trace), &p, sizeof(p));
}
#define BK_TRACE_STAMP(slot)                                                                      \
  if (g_syrk_trace && threadIdx.x == 0) {                                                         \
    g_syrk_trace[(size_t)blockIdx.x * 4 + (slot)] = wall_clock64();                               \
    if ((slot) == 0)                                                                              \
      g_syrk_trace[(size_t)blockIdx.x * 4 + 3] =                                                  \
          ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) | __builtin_amdgcn_s_getreg(63492); \
  }
#else
#define BK_TRACE_STAMP(slot)
#endif

#ifndef SYRK64_OCC
#define SYRK64_OCC 3
#endif
#ifndef SYRK64_DEEP
#define SYRK64_DEEP 0
#endif
#ifndef SYRK64_LDS_EXACT
#define SYRK64_LDS_EXACT 1
#endif
template <int BN, bool ACCUM = true>
__global__ __launch_bounds__(NT, (BN == 64 ? SYRK64_OCC : GEMM_OCC)) void syrk_mirror_kernel(
    GemmOperands g, double alpha, double* __restrict__ C, int64_t ldc, SyrkMap map) {
  // Tiles are 128 x BN. BN = 64 halves the accumulators; its 154 VGPRs let THREE workgroups share a CU with the
  // layout-exact 52 KB of LDS (SYRK64_LDS_EXACT = 1, the default since round 6): 5-7% faster than two in isolation
  // (m = 20 000: k = 128 1 817 -> 1 693 us, k = 256 2 404 -> 2 286). The panel factorisation of the next panel runs
  // beside this kernel, its workgroups need 107 KB of LDS and 256 VGPRs, and with three of these per CU a finished one
  // leaves a hole they do not fit into: the update is therefore launched behind a gate that lets the factorisation
  // become resident first (s1_gate, csrc/eigen_2stage.inc). Without the gate three per CU cost 13-42 ms at C3
  // (profiles/r03/r03m_*, r06/r06b_gate_ab_C3.log: 0.4221 vs 0.4087 s); -DSYRK64_LDS_EXACT=0 builds two per CU.
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int NJ = BN / 32;
  const SyrkTile tile = syrk_map_decode<BN>(map, blockIdx.x, gridDim.x);   // csrc/syrkmap.h
  const int tc = tile.tc, tm = tile.tm, p = tile.p;
  const int m0 = tm * BM, n0 = tc * BN;
  d4 acc[4][NJ];
  BK_TRACE_STAMP(0)
  gemm_tile<false, true, BN, false, (BN == 64 && SYRK64_DEEP)>(g, m0, n0, 0, g.K, smem, acc);  // ends with a block barrier
  BK_TRACE_STAMP(1)
  const int M = g.M;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave & 1) * 64, wn = (wave >> 1) * (BN / 2);
  const int lm = lane & 15, lk = lane >> 4;
  double* buf = smem + wave * (16 * 17);
  const bool diag_tile = (tm == p);
  if (!diag_tile && m0 + BM <= M) {
    // Interior tile (all 128 rows inside, strictly below the diagonal): no predicates. A predicated
    // load or store sits in its own basic block and the compiler waits for memory before each of
    // them, which serialises the whole read-modify-write (16 dependent HBM round trips per strip).
    const double* cb = C + (int64_t)(m0 + wm + lm) + (int64_t)(n0 + wn + lk) * ldc;   // lane's element of sub-tile (0, 0)
    double* cw = C + (int64_t)(m0 + wm + lm) + (int64_t)(n0 + wn + lk) * ldc;
    double* mw = C + (int64_t)(n0 + wn + lm) + (int64_t)(m0 + wm + lk) * ldc;         // its mirror image
    auto load_int = [&](int j, d4 (&cold)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) cold[i][r] = ACCUM ? cb[i * 16 + (int64_t)(j * 16 + 4 * r) * ldc] : 0.0;
    };
    d4 cbuf[2][4];
    load_int(0, cbuf[0]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (j + 1 < NJ) load_int(j + 1, cbuf[(j + 1) & 1]);
      d4 (&cold)[4] = cbuf[j & 1];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double vv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          vv[r] = cold[i][r] + alpha * acc[i][j][r];
          cw[i * 16 + (int64_t)(j * 16 + 4 * r) * ldc] = vv[r];
          buf[(lk + 4 * r) * 17 + lm] = vv[r];   // buf[n_local][m_local]
        }
        double tv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) tv[r] = buf[lm * 17 + (lk + 4 * r)];
#pragma unroll
        for (int r = 0; r < 4; ++r) mw[j * 16 + (int64_t)(i * 16 + 4 * r) * ldc] = tv[r];
      }
    }
    BK_TRACE_STAMP(2)
    return;
  }
  // C is fetched one 64 x 16 column strip at a time, one strip ahead of the stores (vmcnt is
  // in-order over loads and stores: loads issued after a strip's stores would wait for them).
  auto load_strip = [&](int j, d4 (&cold)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm + i * 16 + lm;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn + j * 16 + lk + 4 * r;
        cold[i][r] = (ACCUM && m < M && n < M && m >= n) ? C[(int64_t)m + (int64_t)n * ldc] : 0.0;
      }
    }
  };
  d4 coldbuf[2][4];
  load_strip(0, coldbuf[0]);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (j + 1 < NJ) load_strip(j + 1, coldbuf[(j + 1) & 1]);
    d4 (&cold)[4] = coldbuf[j & 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int mt0 = m0 + wm + i * 16, nt0 = n0 + wn + j * 16;  // 16 x 16 sub-tile origin
      if (diag_tile && mt0 + 15 < nt0) continue;                  // entirely above the diagonal
      const int m = mt0 + lm;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = nt0 + lk + 4 * r;
        double v = 0.0;
        if (m < M && n < M && m >= n) {
          const int64_t o = (int64_t)m + (int64_t)n * ldc;
          v = cold[i][r] + alpha * acc[i][j][r];
          C[o] = v;
        }
        buf[(lk + 4 * r) * 17 + lm] = v;   // buf[n_local][m_local]
      }
      // mirrored store: lane' -> (n' = nt0 + lm, m' = mt0 + lk + 4 r')
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int mm = mt0 + lk + 4 * r, nn = nt0 + lm;
        const double v = buf[lm * 17 + (lk + 4 * r)];
        if (mm < M && nn < M && mm > nn) C[(int64_t)nn + (int64_t)mm * ldc] = v;
      }
    }
  }
  BK_TRACE_STAMP(2)
}

// The map of a launch (csrc/syrkmap.h) with the two development switches: BIGKRLS_SYRK_ORDER=cols is the column-by-column
// order, BIGKRLS_SYRK_R the rows per band.
template <int SBN>
static int64_t syrk_map_build(SyrkMap& mp, int tiles, int c0, int c1, int k) {
  static const int order_cols = [] { const char* e = getenv("BIGKRLS_SYRK_ORDER"); return e && std::string(e) == "cols"; }();
  static const int r_env = [] { const char* e = getenv("BIGKRLS_SYRK_R"); return e ? atoi(e) : 0; }();
  return syrk_map_build<SBN>(mp, tiles, c0, c1, k, order_cols != 0, r_env);
}

// the operands of a rank-k update of an m x m matrix, and its number of 128-row tiles
struct SyrkOperands { GemmOperands g; int tiles; };
static SyrkOperands syrk_operands(int64_t m, int64_t k, const double* A, int64_t lda, const double* B, int64_t ldb) {
  return SyrkOperands{GemmOperands{A, B, lda, ldb, (int)m, (int)m, (int)k, nullptr}, (int)((m + BM - 1) / BM)};
}

template <int SBN, bool ACCUM>
static int launch_syrk_mirror(bigkrls_ctx* ctx, const GemmOperands& g, double alpha, double* C, int64_t ldc,
                              int tiles, int c0, int c1) {
  if (c0 >= c1) return BIGKRLS_OK;
  SyrkMap mp;
  const int64_t nt = syrk_map_build<SBN>(mp, tiles, c0, c1, g.K);
  if (nt <= 0) return BIGKRLS_OK;
  constexpr size_t smem = (SBN == 64 && SYRK64_LDS_EXACT) ? smem_bytes_nt(SBN) : smem_bytes(SBN);
  BK_TRY(ensure_dyn_smem(ctx, (const void*)syrk_mirror_kernel<SBN, ACCUM>, smem));
  hipLaunchKernelGGL((syrk_mirror_kernel<SBN, ACCUM>), dim3((unsigned)nt), dim3(NT), smem, ctx->stream, g,
                     alpha, C, ldc, mp);
  BK_CHECK_LAUNCH();
  return BIGKRLS_OK;
}

int syrk_mirror(bigkrls_ctx* ctx, int64_t m, int64_t k, double alpha, const double* A, int64_t lda,
                const double* B, int64_t ldb, double* C, int64_t ldc, int tn_begin, int tn_end,
                bool narrow_tiles, bool skip_first_column) {
  if (m <= 0 || k <= 0) return BIGKRLS_OK;
  BK_REQUIRE(m < (1ll << 31) && k < (1ll << 31), "syrk_mirror: dimension too large");
  const auto [g, tiles] = syrk_operands(m, k, A, lda, B, ldb);
  if (tn_end < 0 || tn_end > tiles) tn_end = tiles;
  if (tn_begin >= tn_end) return BIGKRLS_OK;
  // 128 x 64 tiles (three workgroups per CU) share the GPU better with a concurrent
  // register-resident panel QR; alone, 128 x 128 tiles are ~6 % faster (N = 20 000: 1.65 vs 1.76 ms)
  BK_REQUIRE(!skip_first_column || narrow_tiles, "syrk_mirror: skip_first_column needs 64-wide tiles");
  // (skip_first_column: the first 64-wide tile column of group tn_begin was updated by the caller)
  if (narrow_tiles)
    return launch_syrk_mirror<64, true>(ctx, g, alpha, C, ldc, tiles, 2 * tn_begin + (skip_first_column ? 1 : 0), 2 * tn_end);
  return launch_syrk_mirror<128, true>(ctx, g, alpha, C, ldc, tiles, tn_begin, tn_end);
}

// C = alpha A B' for a product that is symmetric (A = Q diag(w), B = Q): lower tiles computed, stored twice
int syrk_mirror_set(bigkrls_ctx* ctx, int64_t m, int64_t k, double alpha, const double* A, int64_t lda,
                    const double* B, int64_t ldb, double* C, int64_t ldc) {
  if (m <= 0) return BIGKRLS_OK;
  BK_REQUIRE(k > 0 && m < (1ll << 31) && k < (1ll << 31), "syrk_mirror_set: bad dimensions");
  const auto [g, tiles] = syrk_operands(m, k, A, lda, B, ldb);
  return launch_syrk_mirror<128, false>(ctx, g, alpha, C, ldc, tiles, 0, tiles);
}

// 128 x 64 tiles, columns [c64_begin, c64_end) in units of 64: the lower triangle (with the
// diagonal) of exactly those columns is updated and mirrored.
int syrk_mirror_cols(bigkrls_ctx* ctx, int64_t m, int64_t k, double alpha, const double* A, int64_t lda,
                     const double* B, int64_t ldb, double* C, int64_t ldc, int c64_begin, int c64_end) {
  if (m <= 0 || k <= 0) return BIGKRLS_OK;
  BK_REQUIRE(m < (1ll << 31) && k < (1ll << 31), "syrk_mirror_cols: dimension too large");
  const auto [g, tiles] = syrk_operands(m, k, A, lda, B, ldb);
  // (an odd last column of the matrix: the second column of the last group does not exist, but its
  //  tiles are enumerated; they lie entirely outside the matrix and store nothing)
  if (c64_end < 0 || c64_end > 2 * tiles) c64_end = 2 * tiles;
  if (c64_begin < 0) c64_begin = 0;
  return launch_syrk_mirror<64, true>(ctx, g, alpha, C, ldc, tiles, c64_begin, c64_end);
}

int syrk_lower(bigkrls_ctx* ctx, int64_t m, int64_t k, double alpha, const double* A, int64_t lda,
               const double* B, int64_t ldb, double* C, int64_t ldc) {
  if (m <= 0 || k <= 0) return BIGKRLS_OK;
  BK_REQUIRE(m < (1ll << 31) && k < (1ll << 31), "syrk_lower: dimension too large");
  const auto [g, tiles] = syrk_operands(m, k, A, lda, B, ldb);
  const int64_t nt = (int64_t)tiles * (tiles + 1) / 2;
  BK_TRY(ensure_dyn_smem(ctx, (const void*)syrk_lower_kernel, smem_bytes(128)));
  hipLaunchKernelGGL(syrk_lower_kernel, dim3((unsigned)nt), dim3(NT), smem_bytes(128), ctx->stream, g,
                     alpha, C, ldc, tiles);
  BK_CHECK_LAUNCH();
  return BIGKRLS_OK;
}

// ---------------------------------------------------------------------------
// batched NN GEMM (divide & conquer merges): one descriptor per problem
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT, GEMM_OCC) void gemm_batched_nn_kernel(const GemmDesc* __restrict__ descs,
                                                             int tiles_m_max) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const GemmDesc d = descs[blockIdx.y];
  const int tm = blockIdx.x % tiles_m_max, tn = blockIdx.x / tiles_m_max;
  const int m0 = tm * BM, n0 = tn * 128;
  if (m0 >= d.m || n0 >= d.n) return;
  GemmOperands g{d.A, d.B, d.lda, d.ldb, d.m, d.n, d.k, d.kidx};
  d4 acc[4][4];
  // (uniform over the workgroup. A descriptor without kidx is a plain product: the gathering loader would read through
  //  the null pointer)
  if (d.kidx != nullptr) gemm_tile<false, false, 128, true>(g, m0, n0, 0, d.k, smem, acc);
  else gemm_tile<false, false, 128>(g, m0, n0, 0, d.k, smem, acc);
  double* C = d.C;
  const int64_t ldc = d.ldc;
  const int M = d.m, N = d.n;
  acc_foreach<128>(acc, m0, n0, [&](int m, int n, double v) {
    if (m < M && n < N) C[(int64_t)m + (int64_t)n * ldc] = v;
  });
}

int gemm_batched_nn(bigkrls_ctx* ctx, const GemmDesc* d_descs, int n_batch, int max_m, int max_n) {
  if (n_batch <= 0 || max_m <= 0 || max_n <= 0) return BIGKRLS_OK;
  const int tiles_m = (max_m + BM - 1) / BM, tiles_n = (max_n + 127) / 128;
  BK_TRY(ensure_dyn_smem(ctx, (const void*)gemm_batched_nn_kernel, smem_bytes(128)));
  // grid.y is limited to 65535
  for (int b0 = 0; b0 < n_batch; b0 += 65535) {
    const int nb = std::min(65535, n_batch - b0);
    hipLaunchKernelGGL(gemm_batched_nn_kernel, dim3(tiles_m * tiles_n, nb), dim3(NT),
                       smem_bytes(128), ctx->stream, d_descs + b0, tiles_m);
    BK_CHECK_LAUNCH();
  }
  return BIGKRLS_OK;
}

// ---------------------------------------------------------------------------
// Gaussian kernel block: out[i,j] = exp(-(na_i + nb_j - 2 a_i.b_j)/sigma)
// ---------------------------------------------------------------------------
__device__ __forceinline__ double exp_nonpos(double x);
template <int BN>
__global__ __launch_bounds__(NT) void kernel_block_kernel(GemmOperands g,
                                                          const double* __restrict__ na,
                                                          const double* __restrict__ nb,
                                                          double neg_inv_sigma,
                                                          double* __restrict__ out, int64_t ldo,
                                                          int tiles_m, int tiles_n,
                                                          int64_t diag_shift) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int ntile = tiles_m * tiles_n;
  const int tid = xcd_remap(blockIdx.x, ntile);
  const int tm = tid % tiles_m, tn = tid / tiles_m;
  const int m0 = tm * BM, n0 = tn * BN;
  d4 acc[4][BN / 32];
  gemm_tile<false, true, BN>(g, m0, n0, 0, g.K, smem, acc);
  const int M = g.M, N = g.N;
  acc_foreach<BN>(acc, m0, n0, [&](int m, int n, double v) {
    if (m < M && n < N) {
      double d2 = na[m] + nb[n] - 2.0 * v;
      d2 = d2 > 0.0 ? d2 : 0.0;
      double kv = exp_nonpos(d2 * neg_inv_sigma);
      if (diag_shift >= 0 && (int64_t)m == (int64_t)n + diag_shift) kv = 1.0;
      out[(int64_t)m + (int64_t)n * ldo] = kv;
    }
  });
}

// exp(x) for x <= 0 (the only domain the Gaussian kernel needs), ~20 fp64 VALU ops:
// n = rint(x log2 e), r = x - n ln2 (two-term Cody-Waite), degree-13 Taylor/Horner on
// |r| <= ln2/2 (truncation 4e-18), scale by 2^n with v_ldexp_f64 (gradual underflow to 0).
// The kernel build is VALU-bound on the epilogue (rocprofv3: SQ_ACTIVE_INST_VALU), and the
// library exp() costs ~45 instructions per element.
__device__ __forceinline__ double exp_nonpos(double x) {
  x = fmax(x, -746.0);
  const double n = rint(x * 1.4426950408889634074);
  double r = fma(-n, 6.93147180369123816490e-01, x);
  r = fma(-n, 1.90821492927058770002e-10, r);
  double p = 1.6059043836821613e-10;                   // 1/13!
  p = fma(p, r, 2.08767569878681e-09);                 // 1/12!
  p = fma(p, r, 2.505210838544172e-08);                // 1/11!
  p = fma(p, r, 2.755731922398589e-07);                // 1/10!
  p = fma(p, r, 2.7557319223985893e-06);               // 1/9!
  p = fma(p, r, 2.48015873015873e-05);                 // 1/8!
  p = fma(p, r, 1.984126984126984e-04);                // 1/7!
  p = fma(p, r, 1.388888888888889e-03);                // 1/6!
  p = fma(p, r, 8.333333333333333e-03);                // 1/5!
  p = fma(p, r, 4.1666666666666664e-02);               // 1/4!
  p = fma(p, r, 1.6666666666666666e-01);               // 1/3!
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, (int)n);
}

// The same with a 32-entry table: x log2(e) = (32 q + j + f) / 32, e^x = 2^q 2^(j/32) e^r with |r| <= ln2/64, where a
// degree-6 polynomial has a truncation error of 5e-18 -- 7 fused multiply-adds less per element than exp_nonpos, in
// kernels whose time is the fp64 VALU work of this epilogue. `tab` (LDS, 32 doubles) = 2^(j/32), correctly rounded.
__device__ __constant__ double kExp2Tab32[32] = {
    1.0, 1.0218971486541166, 1.0442737824274138, 1.0671404006768237, 1.0905077326652577, 1.1143867425958924,
    1.1387886347566916, 1.1637248587775775, 1.189207115002721, 1.215247359980469, 1.241857812073484,
    1.2690509571917332, 1.2968395546510096, 1.3252366431597413, 1.3542555469368927, 1.383909881963832,
    1.4142135623730951, 1.4451808069770467, 1.4768261459394993, 1.5091644275934228, 1.5422108254079407,
    1.5759808451078865, 1.6104903319492543, 1.645755478153965, 1.681792830507429, 1.718619298122478,
    1.7562521603732995, 1.7947090750031072, 1.8340080864093424, 1.8741676341103, 1.9152065613971474,
    1.9571441241754002};
__device__ __forceinline__ double exp_nonpos_tab(double x, const double* __restrict__ tab) {
  x = fmax(x, -746.0);
  const double nf = rint(x * 46.166241308446828384);           // 32 / ln 2
  const int n = (int)nf;
  double r = fma(-nf, 6.93147180369123816490e-01 / 32.0, x);    // Cody-Waite: the high part has 21 trailing zero bits
  r = fma(-nf, 1.90821492927058770002e-10 / 32.0, r);
  double p = 1.0 / 720.0;
  p = fma(p, r, 1.0 / 120.0);
  p = fma(p, r, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p *= r;                                                       // e^r - 1
  const double t = tab[n & 31];
  return ldexp(fma(t, p, t), n >> 5);
}

// XCD-aware, L2-blocked order of the one-wave-per-tile kernel builds. Consecutive workgroups round-robin over the 8
// XCDs, so with the plain tile order every XCD walks the whole matrix and streams all of X through its 4 MB L2 again
// and again (X is 8 MB at N = 50 000, P = 20: 1.14 x the algorithmic bytes moved, profiles/r03/r03k_kernel_build_pmc.log).
// Here the tiles are ordered band by band (a band = R consecutive tile rows, whose R x 32 rows of X take ~1 MB),
// inside a band column by column, and every XCD takes one contiguous eighth of that sequence (xcd_remap): it keeps its
// band's row panels in its L2 and streams each column panel once -- the order of the trailing update (SyrkMap), in
// closed form because a launch has up to millions of 32 x 32 tiles.
// Lower triangle of `tiles` tile rows: band b = rows [bR, min((b+1)R, tiles)), columns 0 .. r1-1, column tn holding
// the rows max(r0, tn) .. r1-1. Full bands before b hold R^2 b(b-1)/2 + b R(R+1)/2 tiles.
__device__ __forceinline__ void band_major_lower(int64_t sq, int tiles, int R, int& tm, int& tn) {
  const double Rd = (double)R;
  // start(b) = R^2 b(b-1)/2 + b R(R+1)/2 = (R^2/2) b^2 + (R/2) b  ->  b = floor of the positive root, then corrected
  int b = (int)((-0.5 * Rd + sqrt(0.25 * Rd * Rd + 2.0 * Rd * Rd * (double)sq)) / (Rd * Rd));
  auto start = [&](int q) { return (int64_t)R * R * q * (q - 1) / 2 + (int64_t)q * R * (R + 1) / 2; };
  while (b > 0 && start(b) > sq) --b;
  while ((int64_t)(b + 1) * R < tiles && start(b + 1) <= sq) ++b;
  const int r0 = b * R, r1 = min(r0 + R, tiles), Rb = r1 - r0;
  int64_t sp = sq - start(b);
  const int64_t nfull = (int64_t)r0 * Rb;                 // the columns left of the band's diagonal corner
  if (sp < nfull) {
    tn = (int)(sp / Rb);
    tm = r0 + (int)(sp % Rb);
    return;
  }
  sp -= nfull;                                            // corner: column r0 + c holds Rb - c rows
  int c = (int)(((2.0 * Rb + 1.0) - sqrt((2.0 * Rb + 1.0) * (2.0 * Rb + 1.0) - 8.0 * (double)sp)) * 0.5);
  auto cstart = [&](int q) { return (int64_t)q * Rb - (int64_t)q * (q - 1) / 2; };
  while (c > 0 && cstart(c) > sp) --c;
  while (c + 1 < Rb && cstart(c + 1) <= sp) ++c;
  tn = r0 + c;
  tm = tn + (int)(sp - cstart(c));
}
// rectangle of tiles_m x tiles_n tiles: bands of R tile rows, inside a band column by column
__device__ __forceinline__ void band_major_rect(int64_t sq, int tiles_m, int tiles_n, int R, int& tm, int& tn) {
  const int64_t per_band = (int64_t)R * tiles_n;
  const int b = (int)(sq / per_band);
  const int r0 = b * R, Rb = min(R, tiles_m - r0);
  const int64_t sp = sq - (int64_t)b * per_band;
  tn = (int)(sp / Rb);
  tm = r0 + (int)(sp % Rb);
}

typedef double d2v __attribute__((ext_vector_type(2)));

// Small-P variant (P <= 128: the fit's own regime, P = 5..50): the operands are a few
// MB and live in L2, the output is 8 N^2 bytes, so the kernel is HBM-write bound and the
// only job is to keep many independent store streams in flight. No LDS, no barriers:
// every wave owns one 32 x 32 output tile (2 x 2 MFMA tiles), pulls its fragments
// straight from global/L2 in MFMA operand layout (16 consecutive rows = one 128-byte
// segment per k), runs ceil(P/4) MFMA steps and the exp epilogue, and streams 128-byte
// store segments. ~100 VGPRs -> 4-5 waves per SIMD cover the store latency.
template <int KS>
__global__ __launch_bounds__(NT) void kernel_block_wave_kernel(
    const double* __restrict__ A, int64_t lda, int U, const double* __restrict__ B, int64_t ldb, int V,
    int P, const double* __restrict__ na, const double* __restrict__ nb, double neg_inv_sigma,
    double* __restrict__ out, int64_t ldo, int64_t diag_shift, int tiles_m, int tiles_n, int band_rows,
    int nt_stores, int64_t ntiles) {
  __shared__ double etab[32];
  if (threadIdx.x < 32) etab[threadIdx.x] = kExp2Tab32[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6);
  if (w >= ntiles) return;
  int tm, tn;
  band_major_rect(w, tiles_m, tiles_n, band_rows, tm, tn);
  const int m0 = tm * 32, n0 = tn * 32;
  const int lm = lane & 15, lk = lane >> 4;
  d4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  const int ma0 = min(m0 + lm, U - 1), ma1 = min(m0 + 16 + lm, U - 1);
  const int nb0 = min(n0 + lm, V - 1), nb1 = min(n0 + 16 + lm, V - 1);
  const double* a0p = A + ma0;
  const double* a1p = A + ma1;
  const double* b0p = B + nb0;
  const double* b1p = B + nb1;
  // norms of this lane's output columns / rows: issued first so that their latency hides
  // behind the fragment loads
  double nbv[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) nbv[j][r] = nb[min(n0 + j * 16 + lk + 4 * r, V - 1)];
  double nam[2];
  nam[0] = na[ma0];
  nam[1] = na[ma1];
  // K in chunks of KS MFMA steps (4 k each): all 4*KS fragment loads of a chunk are in
  // flight before the first MFMA; k >= P reads a clamped address and is zeroed.
  for (int kc0 = 0; kc0 < P; kc0 += 4 * KS) {
    double fa0[KS], fa1[KS], fb0[KS], fb1[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = kc0 + 4 * s + lk;
      const int64_t kc = min(k, P - 1);
      fa0[s] = a0p[kc * lda];
      fa1[s] = a1p[kc * lda];
      fb0[s] = b0p[kc * ldb];
      fb1[s] = b1p[kc * ldb];
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const bool kv = (kc0 + 4 * s + lk) < P;
      const double a0 = kv ? fa0[s] : 0.0, a1 = kv ? fa1[s] : 0.0;
      const double b0 = kv ? fb0[s] : 0.0, b1 = kv ? fb1[s] : 0.0;
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(b0, a0, acc[0][0], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(b0, a1, acc[1][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(b1, a0, acc[0][1], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(b1, a1, acc[1][1], 0, 0, 0);
    }
  }

  // 16-byte stores: adjacent lanes (rows 2t, 2t+1) swap one value so that the even lane
  // owns rows (2t, 2t+1) of column n(r) and the odd lane the same rows of column n(r+1).
  const bool odd = (lane & 1) != 0;
  const bool vec_ok = ((ldo & 1) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  // wave-uniform: does this 32 x 32 tile touch the forced-unit diagonal m == n + diag_shift ?
  const bool has_diag = diag_shift >= 0 && (int64_t)m0 < (int64_t)n0 + 32 + diag_shift &&
                        (int64_t)m0 + 32 > (int64_t)n0 + diag_shift;
  const int dsh = (int)diag_shift;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int rp = 0; rp < 4; rp += 2) {
      double kv[2][2];  // [i][r - rp]
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const int n = n0 + j * 16 + lk + 4 * (rp + rr);
        const double nbn = nbv[j][rp + rr];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int m = m0 + i * 16 + lm;
          double d2 = fma(-2.0, acc[i][j][rp + rr], nam[i] + nbn);
          d2 = fmax(d2, 0.0);
          double e = exp_nonpos_tab(d2 * neg_inv_sigma, etab);
          if (has_diag && (m - n) == dsh) e = 1.0;
          kv[i][rr] = e;
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int m = m0 + i * 16 + lm;
        if (vec_ok) {
          const double send = odd ? kv[i][0] : kv[i][1];
          const double recv = __shfl_xor(send, 1, 64);
          const double lo = odd ? recv : kv[i][0];
          const double hi = odd ? kv[i][1] : recv;
          const int mrow = m & ~1;                              // first of the row pair
          const int n = n0 + j * 16 + lk + 4 * (rp + (odd ? 1 : 0));
          if (n < V) {
            double* dst = out + (int64_t)mrow + (int64_t)n * ldo;
            if (mrow + 1 < U) {
              if (nt_stores) {                                  // (uniform; see kb_nontemporal)
                d2v pr;
                pr.x = lo;
                pr.y = hi;
                __builtin_nontemporal_store(pr, reinterpret_cast<d2v*>(dst));
              } else {
                *reinterpret_cast<double2*>(dst) = make_double2(lo, hi);
              }
            } else if (mrow < U) {
              dst[0] = lo;
            }
          }
        } else {
#pragma unroll
          for (int rr = 0; rr < 2; ++rr) {
            const int n = n0 + j * 16 + lk + 4 * (rp + rr);
            if (m < U && n < V) out[(int64_t)m + (int64_t)n * ldo] = kv[i][rr];
          }
        }
      }
    }
}

// kb_store_tile with non-temporal stores
template <bool CHECK>
__device__ __forceinline__ void kbt_store_tile(double* __restrict__ out, int64_t ldo, int U, int V,
                                               int m0, int n0, const double (&e)[2][2][4], bool vec_ok) {
  const int lane = threadIdx.x & 63;
  const int lm = lane & 15, lk = lane >> 4;
  const bool odd = (lane & 1) != 0;
  if (!CHECK) {
    double* base = out + (int64_t)(m0 + (lm & ~1)) + (int64_t)(n0 + lk + (odd ? 4 : 0)) * ldo;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int rp = 0; rp < 4; rp += 2)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const double send = odd ? e[i][j][rp] : e[i][j][rp + 1];
          const double recv = __shfl_xor(send, 1, 64);
          d2v pr;
          pr.x = odd ? recv : e[i][j][rp];
          pr.y = odd ? e[i][j][rp + 1] : recv;
          __builtin_nontemporal_store(pr, reinterpret_cast<d2v*>(base + i * 16 + (int64_t)(j * 16 + 4 * rp) * ldo));
        }
    return;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int rp = 0; rp < 4; rp += 2)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int m = m0 + i * 16 + lm;
        if (vec_ok) {
          const double send = odd ? e[i][j][rp] : e[i][j][rp + 1];
          const double recv = __shfl_xor(send, 1, 64);
          d2v pr;
          pr.x = odd ? recv : e[i][j][rp];
          pr.y = odd ? e[i][j][rp + 1] : recv;
          const int mrow = m & ~1;                              // first of the row pair
          const int n = n0 + j * 16 + lk + 4 * (rp + (odd ? 1 : 0));
          if (n < V) {
            double* dst = out + (int64_t)mrow + (int64_t)n * ldo;
            if (mrow + 1 < U) __builtin_nontemporal_store(pr, reinterpret_cast<d2v*>(dst));
            else if (mrow < U) __builtin_nontemporal_store(pr.x, dst);
          }
        } else {
#pragma unroll
          for (int rr = 0; rr < 2; ++rr) {
            const int n = n0 + j * 16 + lk + 4 * (rp + rr);
            if (m < U && n < V) __builtin_nontemporal_store(e[i][j][rp + rr], out + (int64_t)m + (int64_t)n * ldo);
          }
        }
      }
}

// Paired 16-byte stores of one wave's 32 x 32 tile held in MFMA accumulator layout
// (e[i][j][r] = element (m0 + 16 i + (lane & 15), n0 + 16 j + (lane >> 4) + 4 r)): adjacent lanes
// (rows 2t, 2t+1) swap one value so that the even lane owns rows (2t, 2t+1) of column n(r) and the
// odd lane the same rows of column n(r+1).
template <bool CHECK = true>
__device__ __forceinline__ void kb_store_tile(double* __restrict__ out, int64_t ldo, int U, int V,
                                              int m0, int n0, const double (&e)[2][2][4], bool vec_ok) {
  const int lane = threadIdx.x & 63;
  const int lm = lane & 15, lk = lane >> 4;
  const bool odd = (lane & 1) != 0;
  if (!CHECK) {
    // interior tile, 16-byte aligned output: no predicates (a predicated store sits in a basic block of its own;
    // the 32 x 32 kernels spend a fifth of their instructions on the exec-mask bookkeeping of the general path)
    double* base = out + (int64_t)(m0 + (lm & ~1)) + (int64_t)(n0 + lk + (odd ? 4 : 0)) * ldo;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int rp = 0; rp < 4; rp += 2)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const double send = odd ? e[i][j][rp] : e[i][j][rp + 1];
          const double recv = __shfl_xor(send, 1, 64);
          const double lo = odd ? recv : e[i][j][rp];
          const double hi = odd ? e[i][j][rp + 1] : recv;
          *reinterpret_cast<double2*>(base + i * 16 + (int64_t)(j * 16 + 4 * rp) * ldo) = make_double2(lo, hi);
        }
    return;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int rp = 0; rp < 4; rp += 2)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int m = m0 + i * 16 + lm;
        if (vec_ok) {
          const double send = odd ? e[i][j][rp] : e[i][j][rp + 1];
          const double recv = __shfl_xor(send, 1, 64);
          const double lo = odd ? recv : e[i][j][rp];
          const double hi = odd ? e[i][j][rp + 1] : recv;
          const int mrow = m & ~1;                              // first of the row pair
          const int n = n0 + j * 16 + lk + 4 * (rp + (odd ? 1 : 0));
          if (n < V) {
            double* dst = out + (int64_t)mrow + (int64_t)n * ldo;
            if (mrow + 1 < U) *reinterpret_cast<double2*>(dst) = make_double2(lo, hi);
            else if (mrow < U) dst[0] = lo;
          }
        } else {
#pragma unroll
          for (int rr = 0; rr < 2; ++rr) {
            const int n = n0 + j * 16 + lk + 4 * (rp + rr);
            if (m < U && n < V) out[(int64_t)m + (int64_t)n * ldo] = e[i][j][rp + rr];
          }
        }
      }
}

// Symmetric Gram variant (A == B, square, unit diagonal): only the wave tiles on or below the
// diagonal are computed (half the MFMA, exp and operand traffic); an off-diagonal tile is stored
// twice, the second time transposed through a wave-private LDS buffer so that the mirrored
// stores are the same 16-byte row pairs.
template <int KS>
__global__ __launch_bounds__(NT) void kernel_block_sym_kernel(
    const double* __restrict__ A, int64_t lda, int U, int P, const double* __restrict__ na,
    double neg_inv_sigma, double* __restrict__ out, int64_t ldo, int tiles, int band_rows, int nt_stores,
    int64_t ntiles) {
  __shared__ double tbuf[4][32 * 33];
  __shared__ double etab[32];
  if (threadIdx.x < 32) etab[threadIdx.x] = kExp2Tab32[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * 4 + wave;
  if (w >= ntiles) return;
  int tm, tn;
  band_major_lower(w, tiles, band_rows, tm, tn);
  const int m0 = tm * 32, n0 = tn * 32;
  const int lm = lane & 15, lk = lane >> 4;
  d4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  const int ma0 = min(m0 + lm, U - 1), ma1 = min(m0 + 16 + lm, U - 1);
  const int nb0 = min(n0 + lm, U - 1), nb1 = min(n0 + 16 + lm, U - 1);
  const double* a0p = A + ma0;
  const double* a1p = A + ma1;
  const double* b0p = A + nb0;
  const double* b1p = A + nb1;
  double nbv[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) nbv[j][r] = na[min(n0 + j * 16 + lk + 4 * r, U - 1)];
  double nam[2];
  nam[0] = na[ma0];
  nam[1] = na[ma1];
  for (int kc0 = 0; kc0 < P; kc0 += 4 * KS) {
    double fa0[KS], fa1[KS], fb0[KS], fb1[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = kc0 + 4 * s + lk;
      const int64_t kc = min(k, P - 1);
      fa0[s] = a0p[kc * lda];
      fa1[s] = a1p[kc * lda];
      fb0[s] = b0p[kc * lda];
      fb1[s] = b1p[kc * lda];
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const bool kv = (kc0 + 4 * s + lk) < P;
      const double a0 = kv ? fa0[s] : 0.0, a1 = kv ? fa1[s] : 0.0;
      const double b0 = kv ? fb0[s] : 0.0, b1 = kv ? fb1[s] : 0.0;
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(b0, a0, acc[0][0], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(b0, a1, acc[1][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(b1, a0, acc[0][1], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(b1, a1, acc[1][1], 0, 0, 0);
    }
  }
  const bool vec_ok = ((ldo & 1) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  const bool diag_tile = (tm == tn);
  double e[2][2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + j * 16 + lk + 4 * r;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int m = m0 + i * 16 + lm;
        double d2 = fma(-2.0, acc[i][j][r], nam[i] + nbv[j][r]);
        d2 = fmax(d2, 0.0);
        double v = exp_nonpos_tab(d2 * neg_inv_sigma, etab);
        if (diag_tile && m == n) v = 1.0;
        e[i][j][r] = v;
      }
    }
  const bool interior = vec_ok && m0 + 32 <= U && n0 + 32 <= U;     // (wave-uniform)
  if (interior) { if (nt_stores) kbt_store_tile<false>(out, ldo, U, U, m0, n0, e, true); else kb_store_tile<false>(out, ldo, U, U, m0, n0, e, true); }
  else kb_store_tile<true>(out, ldo, U, U, m0, n0, e, vec_ok);
  if (!diag_tile) {
    // transpose through LDS: E[mloc][nloc], then the mirrored tile's accumulator layout reads
    // element (m' = n0 + 16 i + lm, n' = m0 + 16 j + lk + 4 r) = E[16 j + lk + 4 r][16 i + lm]
    double* tb = tbuf[wave];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) tb[(i * 16 + lm) * 33 + (j * 16 + lk + 4 * r)] = e[i][j][r];
    double et[2][2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) et[i][j][r] = tb[(j * 16 + lk + 4 * r) * 33 + (i * 16 + lm)];
    if (interior) { if (nt_stores) kbt_store_tile<false>(out, ldo, U, U, n0, m0, et, true); else kb_store_tile<false>(out, ldo, U, U, n0, m0, et, true); }
    else kb_store_tile<true>(out, ldo, U, U, n0, m0, et, vec_ok);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Workgroup-tiled kernel build: one workgroup per 128 x 128 output tile. The two 128-row panels of X a tile needs
// are staged ONCE in LDS (k-major, in chunks of 32 columns of X) and shared by the four waves, each of which owns a
// 64 x 64 quarter (4 x 4 MFMA tiles); per byte written the tile reads 1/4 of what the one-wave-per-32x32 kernel
// fetches, which is what that kernel loses at large N (X no longer fits the XCDs' L2s: 4.96 TB/s written at
// N = 20 000, 3.7 at 50 000, 2.9 at 100 000) and at P > 32 (its fragments come straight from global memory).
// Tile order: XCD-aware (symmetric: the band-major order of the trailing update, SyrkMap; rectangular: xcd_remap).
// SYM: the lower tiles are computed, an off-diagonal 32 x 32 piece is stored a second time transposed through a
// wave-private LDS buffer (the panel space, free after the products). Stores are non-temporal 16-byte row pairs:
// the output is written once and must not displace X from the L2.
// ---------------------------------------------------------------------------------------------------------------
constexpr int KBT_KC = 32;            // columns of X staged per chunk
constexpr int KBT_LD = 128 + 8;       // panel row stride in doubles (the k rows of a fragment read half the banks apart)
constexpr size_t kbt_smem_bytes() { return (size_t)(2 * KBT_KC * KBT_LD + 256) * sizeof(double); }

template <bool SYM>
__global__ __launch_bounds__(NT, 2) void kernel_block_tiled_kernel(
    const double* __restrict__ A, int64_t lda, int U, const double* __restrict__ B, int64_t ldb, int V, int P,
    const double* __restrict__ na, const double* __restrict__ nb, double neg_inv_sigma, double* __restrict__ out,
    int64_t ldo, int64_t diag_shift, int tiles_m, int tiles_n, SyrkMap map) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* Xa = smem;
  double* Xb = smem + KBT_KC * KBT_LD;
  double* sna = smem + 2 * KBT_KC * KBT_LD;
  double* snb = sna + 128;
  int tm, tn;
  if (SYM) {
    // band-major, one contiguous eighth per XCD (see SyrkMap; 128-wide columns: CPT = 1)
    const int tiles = map.tiles;
    const int sq = xcd_remap(blockIdx.x, gridDim.x);
    int lo = 0, hi = map.nband;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (map.band_start[mid] <= sq) lo = mid; else hi = mid;
    }
    int sp = sq - map.band_start[lo];
    const int r0 = (map.band0 + lo) * map.R, r1 = min(r0 + map.R, tiles);
    const int cfull = max(min(map.c1, r0 + 1), map.c0);
    const int nfull = (cfull - map.c0) * (r1 - r0);
    if (sp < nfull) {
      tn = map.c0 + sp / (r1 - r0);
      tm = r0 + sp % (r1 - r0);
    } else {
      sp -= nfull;
      tn = cfull;
      while (sp >= r1 - tn) { sp -= r1 - tn; ++tn; }
      tm = tn + sp;
    }
  } else {
    const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    tm = t % tiles_m;
    tn = t / tiles_m;
  }
  const int m0 = tm * 128, n0 = tn * 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
  const int lm = lane & 15, lk = lane >> 4;
  const bool diag_wg = SYM && tm == tn;
  // a wave whose quarter lies entirely above the diagonal of a diagonal tile has nothing to produce (it still
  // stages and keeps the barriers)
  const bool idle = diag_wg && wm < wn;
  __shared__ double etab[32];
  if (tid < 128) sna[tid] = na[min(m0 + tid, U - 1)];
  else snb[tid - 128] = nb[min(n0 + tid - 128, V - 1)];
  if (tid < 32) etab[tid] = kExp2Tab32[tid];
  d4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  const int x = tid & 127, kh = tid >> 7;
  const double* ap = A + min(m0 + x, U - 1);
  const double* bp = B + min(n0 + x, V - 1);
  for (int kc0 = 0; kc0 < P; kc0 += KBT_KC) {
    const int cnt = min(KBT_KC, P - kc0);
    const int cnt4 = (cnt + 3) & ~3;
    double ra[KBT_KC / 2], rb[KBT_KC / 2];
#pragma unroll
    for (int q = 0; q < KBT_KC / 2; ++q) {
      const int k = kh + 2 * q;
      const int64_t kc = kc0 + min(k, cnt - 1);
      ra[q] = ap[kc * lda];
      rb[q] = bp[kc * ldb];
    }
    __syncthreads();                       // (the previous chunk's fragment reads are done)
#pragma unroll
    for (int q = 0; q < KBT_KC / 2; ++q) {
      const int k = kh + 2 * q;
      if (k < cnt4) {
        Xa[k * KBT_LD + x] = k < cnt ? ra[q] : 0.0;
        Xb[k * KBT_LD + x] = k < cnt ? rb[q] : 0.0;
      }
    }
    __syncthreads();
    if (!idle) {
      for (int kk = 0; kk < cnt4; kk += 4) {
        double af[4], bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = Xa[(kk + lk) * KBT_LD + wm + i * 16 + lm];
#pragma unroll
        for (int j = 0; j < 4; ++j) bf[j] = Xb[(kk + lk) * KBT_LD + wn + j * 16 + lm];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(bf[j], af[i], acc[i][j], 0, 0, 0);
      }
    }
  }
  __syncthreads();                         // the panels are dead: their space becomes the transpose buffers
  if (idle) return;
  double* tb = smem + wave * (32 * 33);
  const bool vec_ok = ((ldo & 1) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  const int dsh = (int)diag_shift;
  const bool has_diag = diag_shift >= 0 && (int64_t)m0 < (int64_t)n0 + 128 + diag_shift &&
                        (int64_t)m0 + 128 > (int64_t)n0 + diag_shift;
#pragma unroll
  for (int si = 0; si < 2; ++si)
#pragma unroll
    for (int sj = 0; sj < 2; ++sj) {
      const int pm0 = m0 + wm + 32 * si, pn0 = n0 + wn + 32 * sj;       // this 32 x 32 piece
      if (diag_wg && pm0 < pn0) continue;                               // above the diagonal
      double e[2][2][4];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int nl = wn + 32 * sj + j * 16 + lk + 4 * r;
          const double nbn = snb[nl];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int ml = wm + 32 * si + i * 16 + lm;
            double d2 = fma(-2.0, acc[2 * si + i][2 * sj + j][r], sna[ml] + nbn);
            d2 = fmax(d2, 0.0);
            double v = exp_nonpos_tab(d2 * neg_inv_sigma, etab);
            if (has_diag && (m0 + ml) - (n0 + nl) == dsh) v = 1.0;
            e[i][j][r] = v;
          }
        }
      const bool interior = vec_ok && m0 + 128 <= U && n0 + 128 <= V;    // (workgroup-uniform)
      if (interior) kbt_store_tile<false>(out, ldo, U, V, pm0, pn0, e, true);
      else kbt_store_tile<true>(out, ldo, U, V, pm0, pn0, e, vec_ok);
      if (SYM && pm0 != pn0) {
        // E[mloc][nloc] through LDS; the mirrored piece's accumulator layout reads element
        // (m' = pn0 + 16 i + lm, n' = pm0 + 16 j + lk + 4 r) = E[16 j + lk + 4 r][16 i + lm]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) tb[(i * 16 + lm) * 33 + (j * 16 + lk + 4 * r)] = e[i][j][r];
        double et[2][2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) et[i][j][r] = tb[(j * 16 + lk + 4 * r) * 33 + (i * 16 + lm)];
        if (interior) kbt_store_tile<false>(out, ldo, V, U, pn0, pm0, et, true);
        else kbt_store_tile<true>(out, ldo, V, U, pn0, pm0, et, vec_ok);
      }
    }
}

// Operands of a kernel build moved by one common vector, with their squared row norms. exp(-|a - b|^2 / sigma) depends
// on differences only, but |a|^2 + |b|^2 - 2 a.b cancels on data that are not centred (rows near 1e5: errors of 1e-5 in K),
// so both operands are copied with the column means of A subtracted (col_means, shift_rows_sqnorms in vecops.hip:
// O((u + v) p), no host synchronisation). A row block of A -- the same buffer for the symmetric build, B = A + c0 for
// the column block of a rank -- is served from the copy of A, so it sees bitwise the same rows and norms.
struct CentredOperands {
  const double *A, *B, *na, *nb;
  int64_t lda, ldb;
};
static int centre_operands(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda, const double* B, int64_t v,
                           int64_t ldb, int64_t p, CentredOperands* o) {
  void *pna = nullptr, *pnb = nullptr, *psh = nullptr, *pa = nullptr, *pb = nullptr;
  BK_TRY(ws_get(ctx, SLOT_NORMS_A, u * sizeof(double), &pna));
  BK_TRY(ws_get(ctx, SLOT_KB_SHIFT, p * sizeof(double), &psh));
  BK_TRY(ws_get(ctx, SLOT_KB_A, u * p * (int64_t)sizeof(double), &pa));
  BK_TRY(col_means(ctx, A, u, p, lda, (double*)psh));
  BK_TRY(shift_rows_sqnorms(ctx, A, u, p, lda, (const double*)psh, (double*)pa, (double*)pna));
  o->A = (const double*)pa;
  o->na = (const double*)pna;
  o->lda = u;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(A), b0 = reinterpret_cast<uintptr_t>(B);
  if (lda == ldb && b0 >= a0 && (b0 - a0) / sizeof(double) + (uint64_t)v <= (uint64_t)u) {
    const int64_t r0 = (int64_t)((b0 - a0) / sizeof(double));
    o->B = o->A + r0;
    o->nb = o->na + r0;
    o->ldb = u;
    return BIGKRLS_OK;
  }
  BK_TRY(ws_get(ctx, SLOT_NORMS_B, v * sizeof(double), &pnb));
  BK_TRY(ws_get(ctx, SLOT_KB_B, v * p * (int64_t)sizeof(double), &pb));
  BK_TRY(shift_rows_sqnorms(ctx, B, v, p, ldb, (const double*)psh, (double*)pb, (double*)pnb));
  o->B = (const double*)pb;
  o->nb = (const double*)pnb;
  o->ldb = v;
  return BIGKRLS_OK;
}

int kernel_block(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda, const double* B,
                 int64_t v, int64_t ldb, int64_t p, double sigma, double* out, int64_t ldo,
                 int64_t diag_shift) {
  BK_REQUIRE(u >= 0 && v >= 0 && p > 0, "kernel_block: bad dimensions");
  BK_REQUIRE(u < (1ll << 31) && v < (1ll << 31) && p < (1ll << 31), "kernel_block: too large");
  BK_REQUIRE(sigma > 0.0, "kernel_block: sigma must be > 0");
  if (u == 0 || v == 0) return BIGKRLS_OK;
  BK_REQUIRE(A && B && out, "kernel_block: null pointer");
  BK_REQUIRE(lda >= u && ldb >= v, "kernel_block: leading dimension of A or B too small");
  BK_REQUIRE(ldo >= u, "kernel_block: leading dimension of out too small");
  const bool sym = A == B && u == v && lda == ldb && diag_shift == 0;
  // from here on A and B are the centred copies (the same buffer when they were the same buffer)
  CentredOperands co;
  BK_TRY(centre_operands(ctx, A, u, lda, B, v, ldb, p, &co));
  return kernel_block_centred(ctx, co.A, u, co.lda, co.na, co.B, v, co.ldb, co.nb, p, sigma, out, ldo, diag_shift, sym);
}

int kernel_block_centred(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda, const double* pna, const double* B,
                         int64_t v, int64_t ldb, const double* pnb, int64_t p, double sigma, double* out, int64_t ldo,
                         int64_t diag_shift, bool sym) {
  // the development switches of kb_plan (csrc/ktplan.h), read once per process
  static const int kb_force = [] {
    const char* e = getenv("BIGKRLS_KB");
    return e ? (std::string(e) == "tiled" ? 1 : (std::string(e) == "wave" ? -1 : 0)) : 0;
  }();
  static const int r_env = [] { const char* e = getenv("BIGKRLS_KB_R"); return e ? atoi(e) : 0; }();
  static const int nt_env = [] { const char* e = getenv("BIGKRLS_KB_NT"); return e ? atoi(e) : -1; }();
  // The wave kernels by their KS = 1..8, named one by one: a code object lays its kernels out in the order in which
  // the source first names them, and chosen through with_ks they would be instantiated at the call and move ahead.
  using SymFn = void (*)(const double*, int64_t, int, int, const double*, double, double*, int64_t, int, int, int, int64_t);
  using WaveFn = void (*)(const double*, int64_t, int, const double*, int64_t, int, int, const double*, const double*, double,
                          double*, int64_t, int64_t, int, int, int, int, int64_t);
  const auto tiled_fn = sym ? kernel_block_tiled_kernel<true> : kernel_block_tiled_kernel<false>;
  static constexpr SymFn sym_fns[8] = {kernel_block_sym_kernel<1>, kernel_block_sym_kernel<2>, kernel_block_sym_kernel<3>,
                                       kernel_block_sym_kernel<4>, kernel_block_sym_kernel<5>, kernel_block_sym_kernel<6>,
                                       kernel_block_sym_kernel<7>, kernel_block_sym_kernel<8>};
  static constexpr WaveFn wave_fns[8] = {kernel_block_wave_kernel<1>, kernel_block_wave_kernel<2>, kernel_block_wave_kernel<3>,
                                         kernel_block_wave_kernel<4>, kernel_block_wave_kernel<5>, kernel_block_wave_kernel<6>,
                                         kernel_block_wave_kernel<7>, kernel_block_wave_kernel<8>};
  constexpr auto generic_fn = kernel_block_kernel<KB_GENERIC_BN>;
  static_assert(BM == KB_GENERIC_BM, "kb_plan counts the generic kernel's tiles");

  const KbPlan k = kb_plan(u, v, p, sym, kb_force, r_env, nt_env);
  const bool wave = k.arm == KB_SYM_WAVE || k.arm == KB_WAVE;   // (their ks is 1..8)
  BK_REQUIRE(wave ? k.grid < (1ll << 31) : (k.arm == KB_GENERIC || k.ntiles < (1ll << 31)), "kernel_block: too many tiles");
  if (k.arm == KB_TILED) BK_TRY(ensure_dyn_smem(ctx, (const void*)tiled_fn, kbt_smem_bytes()));
  if (k.arm == KB_GENERIC) BK_TRY(ensure_dyn_smem(ctx, (const void*)generic_fn, smem_bytes(KB_GENERIC_BN)));
  BK_TRY(prof_begin(ctx, "kernel_block", 2.0 * (double)u * (double)v * (double)p));
  const double nis = -1.0 / sigma;
  const dim3 grid((unsigned)k.grid);
  if (k.arm == KB_TILED) {
    hipLaunchKernelGGL(tiled_fn, grid, dim3(NT), kbt_smem_bytes(), ctx->stream, A, lda, (int)u, B, ldb, (int)v, (int)p, pna,
                       pnb, nis, out, ldo, diag_shift, k.tiles_m, k.tiles_n, k.map);
  } else if (k.arm == KB_SYM_WAVE) {   // symmetric Gram matrix (bGaussKernel): lower wave tiles + mirrored stores
    hipLaunchKernelGGL(sym_fns[k.ks - 1], grid, dim3(NT), 0, ctx->stream, A, lda, (int)u, (int)p, pna, nis, out, ldo,
                       k.tiles_m, k.band_rows, k.nontemporal, k.ntiles);
  } else if (k.arm == KB_WAVE) {
    hipLaunchKernelGGL(wave_fns[k.ks - 1], grid, dim3(NT), 0, ctx->stream, A, lda, (int)u, B, ldb, (int)v, (int)p, pna, pnb,
                       nis, out, ldo, diag_shift, k.tiles_m, k.tiles_n, k.band_rows, k.nontemporal, k.ntiles);
  } else {
    GemmOperands g{A, B, lda, ldb, (int)u, (int)v, (int)p, nullptr};
    hipLaunchKernelGGL(generic_fn, dim3(k.tiles_m * k.tiles_n), dim3(NT), smem_bytes(KB_GENERIC_BN), ctx->stream, g, pna, pnb,
                       nis, out, ldo, k.tiles_m, k.tiles_n, diag_shift);
  }
  BK_CHECK_LAUNCH();
  BK_TRY(prof_end(ctx, "kernel_block"));
  return BIGKRLS_OK;
}

// ---------------------------------------------------------------------------
// fused kernel contraction (marginal effects at new data points, csrc/margeff.hip)
// ---------------------------------------------------------------------------
// out (ns x q) = K(S, L) W with K(S, L)[s, l] = exp(-||S_s - L_l||^2 / sigma) and W (nl x q): the kernel tile is
// rebuilt in registers and contracted at once, never written (flash-attention style). K(A, B)' = K(B, A), so
// K(A, B) W (rows of A stationary, loop over B) and K(A, B)' W (rows of B stationary, loop over A) are this one kernel
// with the roles of the operands swapped.
//
// The frame of the tile kernels (kt_*), shared by this kernel, its wide and grouped forms and the two leave-out kernels
// further down: a wave owns MS stationary tiles of 16 rows and a chunk of columns, and walks its share of the loop rows
// 16 at a time:
//   G = L_tile S_tile'  : mfma_f64_16x16x4(L, S), register r of lane holds (l = l0 + (lane >> 4) + 4 r, s = lane & 15)
//   d2 = max(|s|^2 + |l|^2 - 2 G, 0), the epilogue of kernel_block_wave_kernel, in place
// and what a kernel does with d2 is its own: here
//   E = exp(-d2 / sigma)
//   acc += E W_tile     : register r of E is the A operand of k-step r (A[row = lane & 15][k = lane >> 4] = E(s, l))
// so neither the kernel tile nor a transpose of it touches LDS or memory. Rows past an operand's end are read from its
// last row (clamped) and masked or not written by the kernel. When the grid would leave compute units idle (few
// stationary rows) the loop rows are split over several waves whose partial sums are added by contract_reduce_kernel in
// a fixed order: no atomics, the result does not depend on scheduling.
// KS > 0: P <= 4 KS and the stationary fragments stay in registers for the whole loop; KS == 0: any P, fragments
// re-read (from L1 / L2) for every loop tile.

// exp_nonpos_tab's table in LDS (every thread of the block, before a wave without a task leaves)
__device__ __forceinline__ void kt_exp_table(double* etab) {
  if (threadIdx.x < 32) etab[threadIdx.x] = kExp2Tab32[threadIdx.x];
  __syncthreads();
}

// The task of a wave: stationary tile group st (fastest), column chunk cc, and `part`, a loop split or a segment.
struct KtTask {
  int st, cc;
  int64_t part;
};
__device__ __forceinline__ bool kt_task(KtTask& k, int stiles, int nchunks, int64_t ntasks) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= ntasks) return false;
  k.st = (int)(w % stiles);
  k.cc = (int)((w / stiles) % nchunks);
  k.part = w / ((int64_t)stiles * nchunks);
  return true;
}
// loop split sp of nsplit walks the loop tiles [kt_split_begin(sp), kt_split_begin(sp + 1))
__device__ __forceinline__ int kt_split_begin(int ltiles, int sp, int nsplit) { return (int)((int64_t)ltiles * sp / nsplit); }

// column k of the stationary row srow; k >= P zeroed: the loop side then reads a clamped, finite value
__device__ __forceinline__ double kt_fragment(const double* S, int64_t lds, int srow, int k, int P) {
  return k < P ? S[srow + (int64_t)k * lds] : 0.0;
}

// This lane's stationary rows (clamped), their squared norms and, with KS > 0, their resident fragments.
template <int MS, int KS>
__device__ __forceinline__ void kt_stationary(int (&srow)[MS], double (&ns)[MS], double (&sf)[MS][KS > 0 ? KS : 1],
                                              const double* __restrict__ S, int64_t lds, int NS,
                                              const double* __restrict__ nrm_s, int P, int s0) {
  const int lane = threadIdx.x & 63, lm = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int m = 0; m < MS; ++m) {
    srow[m] = min(s0 + 16 * m + lm, NS - 1);
    ns[m] = nrm_s[srow[m]];
  }
  if (KS > 0) {
#pragma unroll
    for (int m = 0; m < MS; ++m)
#pragma unroll
      for (int t = 0; t < (KS > 0 ? KS : 1); ++t) {
        const int k = 4 * t + lk;
        sf[m][t] = kt_fragment(S, lds, srow[m], k, P);
      }
  }
}

// g[m] = L_tile S_tile(m)' for the loop tile whose row `lrow` this lane feeds (MFMA chains in s-then-m order).
// The trip counts ms = MS and ks = max(KS, 1) come BY REFERENCE, from two locals of the kernel: the compiler
// optimises a callee before it inlines it, and with counts it knows it unrolls these loops here, on their own, where the
// kernel's own loops are unrolled after its local arrays have become vectors. The two orders give the same operations in
// another instruction order, and the register allocator then lands elsewhere: of the 27 kernel_contract_kernel
// instantiations (no minimum wave count in their launch bounds) 8 changed occupancy, hence the loop splits and the bits.
// Counts behind a reference are unknown until the call is inlined, and the loops unroll in the kernel as they did when
// the code stood there ("The shared frame", has both resource tables).
template <int MS, int KS>
__device__ __forceinline__ void kt_gram(d4 (&g)[MS], const int (&srow)[MS], const double (&sf)[MS][KS > 0 ? KS : 1],
                                        const double* __restrict__ S, int64_t lds, const double* __restrict__ L,
                                        int64_t ldl, int lrow, int P, const int& ms, const int& ks) {
  const int lk = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int m = 0; m < ms; ++m) g[m] = (d4){0.0, 0.0, 0.0, 0.0};
  if (KS > 0) {
    double lf[KS > 0 ? KS : 1];
#pragma unroll
    for (int s = 0; s < ks; ++s) lf[s] = L[lrow + (int64_t)min(4 * s + lk, P - 1) * ldl];
#pragma unroll
    for (int s = 0; s < ks; ++s)
#pragma unroll
      for (int m = 0; m < ms; ++m) g[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(lf[s], sf[m][s], g[m], 0, 0, 0);
  } else {
    const int steps = (P + 3) / 4;
    for (int s0k = 0; s0k < steps; s0k += 4) {
      double lf[4], sg[MS][4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = 4 * (s0k + s) + lk;
        lf[s] = L[lrow + (int64_t)min(k, P - 1) * ldl];
#pragma unroll
        for (int m = 0; m < ms; ++m) sg[m][s] = kt_fragment(S, lds, srow[m], k, P);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int m = 0; m < ms; ++m) g[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(lf[s], sg[m][s], g[m], 0, 0, 0);
    }
  }
}

// the squared distance from an entry of the Gram tile and the two squared norms
__device__ __forceinline__ double kt_dist2(double g, double ns, double nl) { return fmax(fma(-2.0, g, ns + nl), 0.0); }

// MFMA accumulators to memory: acc[m][c] register r is (s = s0 + 16 m + (lane >> 4) + 4 r, col = c0 + 16 c + (lane & 15));
// ALLCOLS: every column of the chunk exists.
template <int MS, int CT, bool ALLCOLS>
__device__ __forceinline__ void kt_store_tiles(const d4 (&acc)[MS][CT], double* __restrict__ dst, int64_t ld, int s0,
                                               int c0, int NS, int Q) {
  const int lane = threadIdx.x & 63, lm = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int m = 0; m < MS; ++m)
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const int col = c0 + 16 * c + lm;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = s0 + 16 * m + lk + 4 * r;
        if (s < NS && (ALLCOLS || col < Q)) dst[s + (int64_t)col * ld] = acc[m][c][r];
      }
    }
}

// Per-lane sums to memory: the four lane groups (lane >> 4) hold the sums over the loop rows l = (lane >> 4) mod 4 of
// the same stationary rows s0 + 16 m + (lane & 15); they are added with shuffles and group 0 stores column c0 + j, j < ncw.
template <int MS, int CW>
__device__ __forceinline__ void kt_store_lane_sums(const double (&acc)[MS][CW], double* __restrict__ dst, int64_t ld,
                                                   int s0, int c0, int ncw, int NS) {
  const int lane = threadIdx.x & 63, lm = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int j = 0; j < CW; ++j)
#pragma unroll
    for (int m = 0; m < MS; ++m) {
      double a = acc[m][j];
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      const int s = s0 + 16 * m + lm;
      if (lk == 0 && j < ncw && s < NS) dst[s + (int64_t)(c0 + j) * ld] = a;
    }
}

// Each wave of kernel_contract_kernel owns 64 stationary rows (4 MFMA tiles of 16) and 16 CT columns of W.
constexpr int KC_MS = 4;   // 16-row stationary tiles per wave

template <int KS, int CT>
__global__ __launch_bounds__(NT) void kernel_contract_kernel(
    const double* __restrict__ S, int64_t lds, int NS, const double* __restrict__ L, int64_t ldl, int NL, int P,
    const double* __restrict__ nrm_s, const double* __restrict__ nrm_l, double neg_inv_sigma,
    const double* __restrict__ W, int64_t ldw, int Q, double* __restrict__ out, int64_t ldo, int64_t split_stride,
    int stiles, int nchunks, int nsplit, int ltiles, int64_t ntasks) {
  __shared__ double etab[32];
  kt_exp_table(etab);
  KtTask k;
  if (!kt_task(k, stiles, nchunks, ntasks)) return;
  const int sp = (int)k.part;
  const int s0 = k.st * 16 * KC_MS, c0 = k.cc * 16 * CT;
  const int t_begin = kt_split_begin(ltiles, sp, nsplit), t_end = kt_split_begin(ltiles, sp + 1, nsplit);
  const int lane = threadIdx.x & 63, lm = lane & 15, lk = lane >> 4;

  int srow[KC_MS];
  double ns[KC_MS], sf[KC_MS][KS > 0 ? KS : 1];
  kt_stationary<KC_MS, KS>(srow, ns, sf, S, lds, NS, nrm_s, P, s0);
  const int ms = KC_MS, ks = KS > 0 ? KS : 1;   // kt_gram's trip counts (by reference: see there)
  d4 acc[KC_MS][CT];
#pragma unroll
  for (int m = 0; m < KC_MS; ++m)
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[m][c] = (d4){0.0, 0.0, 0.0, 0.0};

  for (int t = t_begin; t < t_end; ++t) {
    const int l0 = t * 16;
    const int lrow = min(l0 + lm, NL - 1);   // this lane's row of the L operand
    double nl[4], wf[CT][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int l = l0 + lk + 4 * r;         // this lane's loop row in accumulator register r
      nl[r] = nrm_l[min(l, NL - 1)];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const int col = c0 + 16 * c + lm;
        wf[c][r] = (l < NL && col < Q) ? W[l + (int64_t)col * ldw] : 0.0;
      }
    }
    d4 g[KC_MS];
    kt_gram<KC_MS, KS>(g, srow, sf, S, lds, L, ldl, lrow, P, ms, ks);
#pragma unroll
    for (int m = 0; m < KC_MS; ++m) {
      d4 e;
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = exp_nonpos_tab(kt_dist2(g[m][r], ns[m], nl[r]) * neg_inv_sigma, etab);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[m][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(e[r], wf[c][r], acc[m][c], 0, 0, 0);
    }
  }
  kt_store_tiles<KC_MS, CT, false>(acc, out + (int64_t)sp * split_stride, ldo, s0, c0, NS, Q);
}

// out[s, c] = sum over the splits, in split order, of part[sp][s, c] (each ns x q, ld ns)
__global__ void contract_reduce_kernel(int NS, int Q, int nsplit, const double* __restrict__ part,
                                       double* __restrict__ out, int64_t ldo) {
  const int64_t total = (int64_t)NS * Q, stride = total;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int k = 0; k < nsplit; ++k) s += part[(int64_t)k * stride + e];
    out[(e % NS) + (e / NS) * ldo] = s;
  }
}

// The same contraction for more than 64 columns of W (the 128-column block of the block Lanczos on an implicit kernel,
// csrc/eigen.hip): one wave builds a kernel tile ONCE and contracts it with up to 128 columns, where the kernel above
// (CT <= 4) would rebuild every tile, exp included, once per 64 columns.
// Tiling: KCW_MS = 2 stationary tiles (32 rows) x KCW_CT = 8 column tiles (128 columns) per wave. Registers per lane
// (a double is two): accumulators 2 x 8 x 4 doubles = 128 (AGPRs), resident fragments sf 2 x KS <= 16 doubles = 32,
// G / E 2 x 4 doubles = 16, one k-step of W 8 doubles = 16 (the compiler keeps two to three of the four in flight),
// loop fragments, norms and addresses about 40: 230 to 256 of the 512 of the unified file, i.e. 2 waves per SIMD
// (__launch_bounds__(NT, 2) holds the allocator to it). Four stationary tiles with 128 columns would take 256
// registers for the accumulators alone and leave one wave per SIMD with nothing to cover the loads of W.
// MFMA 16x16x4 per 32 x 16 kernel tile pair: 2 KS (<= 16) for G and 2 x 4 x 8 = 64 for the contraction.
// Column tiles that lie wholly past q are skipped (wave-uniform), so a last chunk of q mod 128 columns costs its own
// tiles only. Everything else is the frame (kt_*).
constexpr int KCW_MS = 2;   // 16-row stationary tiles per wave
constexpr int KCW_CT = 8;   // 16-column tiles of W per wave

// FULL: the wave's 128 columns all exist (the Lanczos block): column tile c of W sits at the wave-uniform offset
// 16 c ldw from one pointer per lane. Otherwise: a clamped column per tile, tiles wholly past q skipped.
template <int KS, bool FULL>
__device__ __forceinline__ void kcw_body(const double* __restrict__ S, int64_t lds, int NS, const double* __restrict__ L,
                                         int64_t ldl, int NL, int P, const double* __restrict__ nrm_s,
                                         const double* __restrict__ nrm_l, double neg_inv_sigma,
                                         const double* __restrict__ W, int64_t ldw, int Q, double* __restrict__ dst,
                                         int64_t ldo, int s0, int c0, int t_begin, int t_end, const double* etab) {
  const int lane = threadIdx.x & 63;
  const int lm = lane & 15, lk = lane >> 4;
  const int nct = FULL ? KCW_CT : min(KCW_CT, (Q - c0 + 15) / 16);   // column tiles that hold a column (wave-uniform)

  int srow[KCW_MS];
  double ns[KCW_MS], sf[KCW_MS][KS > 0 ? KS : 1];
  kt_stationary<KCW_MS, KS>(srow, ns, sf, S, lds, NS, nrm_s, P, s0);
  const int ms = KCW_MS, ks = KS > 0 ? KS : 1;   // kt_gram's trip counts (by reference: see there)
  d4 acc[KCW_MS][KCW_CT];
#pragma unroll
  for (int m = 0; m < KCW_MS; ++m)
#pragma unroll
    for (int c = 0; c < KCW_CT; ++c) acc[m][c] = (d4){0.0, 0.0, 0.0, 0.0};
  // this lane's column of W in each column tile
  const double* wbase = W + (int64_t)(c0 + lm) * ldw;
  const int64_t wstep = 16 * ldw;

  for (int t = t_begin; t < t_end; ++t) {
    const int l0 = t * 16;
    const int lrow = min(l0 + lm, NL - 1);   // this lane's row of the L operand
    double nl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) nl[r] = nrm_l[min(l0 + lk + 4 * r, NL - 1)];
    d4 g[KCW_MS];
    kt_gram<KCW_MS, KS>(g, srow, sf, S, lds, L, ldl, lrow, P, ms, ks);
    // E in place of G
#pragma unroll
    for (int m = 0; m < KCW_MS; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) g[m][r] = exp_nonpos_tab(kt_dist2(g[m][r], ns[m], nl[r]) * neg_inv_sigma, etab);
    // k-step r of the contraction: loop rows l0 + (lane >> 4) + 4 r, one k-step of W (8 doubles) at a time
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int l = l0 + lk + 4 * r;
      const bool lok = l < NL;
      const int lc = min(l, NL - 1);
      double wf[KCW_CT];
      if (FULL) {
#pragma unroll
        for (int c = 0; c < KCW_CT; ++c) {
          const double v = wbase[c * wstep + lc];
          wf[c] = lok ? v : 0.0;
        }
#pragma unroll
        for (int c = 0; c < KCW_CT; ++c)
#pragma unroll
          for (int m = 0; m < KCW_MS; ++m)
            acc[m][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(g[m][r], wf[c], acc[m][c], 0, 0, 0);
      } else {
#pragma unroll
        for (int c = 0; c < KCW_CT; ++c) {
          const int col = c0 + 16 * c + lm;      // (clamped: a column past q is weighted by 0; the address is
          const double v = W[lc + (int64_t)min(col, Q - 1) * ldw];   //  recomputed to keep 8 pointers out of registers)
          wf[c] = (lok && col < Q) ? v : 0.0;
        }
#pragma unroll
        for (int c = 0; c < KCW_CT; ++c)
          if (c < nct) {
#pragma unroll
            for (int m = 0; m < KCW_MS; ++m)
              acc[m][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(g[m][r], wf[c], acc[m][c], 0, 0, 0);
          }
      }
    }
  }
  kt_store_tiles<KCW_MS, KCW_CT, FULL>(acc, dst, ldo, s0, c0, NS, Q);
}

template <int KS>
__global__ __launch_bounds__(NT, 2) void kernel_contract_wide_kernel(
    const double* __restrict__ S, int64_t lds, int NS, const double* __restrict__ L, int64_t ldl, int NL, int P,
    const double* __restrict__ nrm_s, const double* __restrict__ nrm_l, double neg_inv_sigma,
    const double* __restrict__ W, int64_t ldw, int Q, double* __restrict__ out, int64_t ldo, int64_t split_stride,
    int stiles, int nchunks, int nsplit, int ltiles, int64_t ntasks) {
  __shared__ double etab[32];
  kt_exp_table(etab);
  KtTask k;
  if (!kt_task(k, stiles, nchunks, ntasks)) return;
  const int sp = (int)k.part;
  const int s0 = k.st * 16 * KCW_MS, c0 = k.cc * 16 * KCW_CT;
  const int t_begin = kt_split_begin(ltiles, sp, nsplit), t_end = kt_split_begin(ltiles, sp + 1, nsplit);
  double* dst = out + (int64_t)sp * split_stride;
  if (c0 + 16 * KCW_CT <= Q)
    kcw_body<KS, true>(S, lds, NS, L, ldl, NL, P, nrm_s, nrm_l, neg_inv_sigma, W, ldw, Q, dst, ldo, s0, c0, t_begin, t_end, etab);
  else   // (with resident fragments the partial body would spill: it re-reads them like KS == 0)
    kcw_body<0, false>(S, lds, NS, L, ldl, NL, P, nrm_s, nrm_l, neg_inv_sigma, W, ldw, Q, dst, ldo, s0, c0, t_begin, t_end, etab);
}

// ---- the host side of the frame ----
// (ks_of, with_ks and plan_loop_splits: csrc/ktplan.h)
// the waves of a tile kernel that the device holds at once (2 or 3 per SIMD, by the kernel's registers)
static int wave_slots(bigkrls_ctx* ctx, const void* fn, int64_t* slots) {
  int cap = 0;
  BK_TRY(resident_capacity(ctx, fn, &cap, NT));
  *slots = (int64_t)cap * (NT / 64);
  return BIGKRLS_OK;
}
// One launch over nsplit loop splits and what follows it. launch(dst, ldd, split_stride) starts the tile kernel: a single
// split stores the ns x nc result where it belongs; several store their partial sums (each ns x nc, ld ns) into the
// workspace slot, and contract_reduce_kernel adds them in split order. The result belongs in out (ld ldo), or with
// out == nullptr in a buffer behind the partial sums (ld ns) that *staged returns.
template <class Launch>
static int launch_loop_splits(bigkrls_ctx* ctx, int slot, int64_t nsplit, int64_t ns, int64_t nc, double* out, int64_t ldo,
                              double** staged, Launch&& launch) {
  const int64_t part_doubles = nsplit > 1 ? nsplit * ns * nc : 0, staged_doubles = out ? 0 : ns * nc;
  double* part = nullptr;
  if (part_doubles + staged_doubles > 0) {
    void* pp = nullptr;
    BK_TRY(ws_get(ctx, slot, (part_doubles + staged_doubles) * (int64_t)sizeof(double), &pp));
    part = (double*)pp;
  }
  if (!out) {
    out = *staged = part + part_doubles;
    ldo = ns;
  }
  if (nsplit == 1) BK_TRY(launch(out, ldo, (int64_t)0));
  else BK_TRY(launch(part, ns, ns * nc));
  BK_CHECK_LAUNCH();
  if (nsplit > 1) {
    const int blocks = (int)std::min<int64_t>((ns * nc + 255) / 256, 4096);
    hipLaunchKernelGGL(contract_reduce_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (int)ns, (int)nc, (int)nsplit,
                       (const double*)part, out, ldo);
    BK_CHECK_LAUNCH();
  }
  return BIGKRLS_OK;
}

// out (ns x q, ldo) = K(S, L) W for operands that are already centred, with their squared row norms: what
// kernel_contract runs after centre_operands, and what an implicit kernel operator (KernelOp) runs at every product.
// q <= 64: kernel_contract_kernel; q > 64: kernel_contract_wide_kernel in chunks of 128 columns, profiled under its own
// name. (Measured against the narrow kernel at q = 128: DESIGN.md section 4.)
int kernel_contract_centred(bigkrls_ctx* ctx, const double* S, int64_t ns, int64_t lds, const double* nrm_s,
                            const double* L, int64_t nl, int64_t ldl, const double* nrm_l, int64_t p, double sigma,
                            const double* W, int64_t q, int64_t ldw, double* out, int64_t ldo) {
  BK_REQUIRE(ns > 0 && nl > 0 && p > 0 && q > 0, "kernel_contract: bad dimensions");
  BK_REQUIRE(ns < (1ll << 31) && nl < (1ll << 31) && p < (1ll << 20) && q < (1ll << 20), "kernel_contract: too large");
  BK_REQUIRE(sigma > 0.0, "kernel_contract: sigma must be > 0");
  BK_REQUIRE(S && L && nrm_s && nrm_l && W && out, "kernel_contract: null pointer");
  BK_REQUIRE(lds >= ns && ldl >= nl && ldw >= nl && ldo >= ns, "kernel_contract: leading dimension too small");
  const bool wide = q > 64;
  const int CT = wide ? KCW_CT : (q <= 16 ? 1 : (q <= 32 ? 2 : 4));
  const int MS = wide ? KCW_MS : KC_MS;
  const char* pname = wide ? "kernel_contract_wide" : "kernel_contract";
  using KcFn = void (*)(const double*, int64_t, int, const double*, int64_t, int, int, const double*, const double*,
                        double, const double*, int64_t, int, double*, int64_t, int64_t, int, int, int, int, int64_t);
  const KcFn fn = with_ks(ks_of(p), [&](auto ks) -> KcFn {
    constexpr int KS = decltype(ks)::value;
    if (wide) return kernel_contract_wide_kernel<KS>;
    if (CT == 1) return kernel_contract_kernel<KS, 1>;
    if (CT == 2) return kernel_contract_kernel<KS, 2>;
    return kernel_contract_kernel<KS, 4>;
  });
  const int64_t stiles = (ns + 16 * MS - 1) / (16 * MS);
  const int64_t nchunks = (q + 16 * CT - 1) / (16 * CT);
  const int64_t ltiles = (nl + 15) / 16;
  int64_t slots = 0;
  BK_TRY(wave_slots(ctx, (const void*)fn, &slots));
  const int64_t nsplit = plan_loop_splits(stiles * nchunks, slots, ltiles, ns * q * (int64_t)sizeof(double));
  const int64_t ntasks = stiles * nchunks * nsplit;
  BK_REQUIRE((ntasks + 3) / 4 < (1ll << 31), "kernel_contract: too many tiles");
  BK_TRY(launch_loop_splits(ctx, SLOT_CONTRACT_PART, nsplit, ns, q, out, ldo, nullptr,
                            [&](double* dst, int64_t ldd, int64_t split_stride) -> int {
    BK_TRY(prof_begin(ctx, pname, 2.0 * (double)ns * (double)nl * (double)(p + q)));
    hipLaunchKernelGGL(fn, dim3((unsigned)((ntasks + 3) / 4)), dim3(NT), 0, ctx->stream, S, lds, (int)ns, L, ldl, (int)nl,
                       (int)p, nrm_s, nrm_l, -1.0 / sigma, W, ldw, (int)q, dst, ldd, split_stride, (int)stiles,
                       (int)nchunks, (int)nsplit, (int)ltiles, ntasks);
    return BIGKRLS_OK;
  }));
  BK_TRY(prof_end(ctx, pname));
  return BIGKRLS_OK;
}

int kernel_contract(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda, const double* B, int64_t v,
                    int64_t ldb, int64_t p, double sigma, const double* W, int64_t q, int64_t ldw, int trans,
                    double* out, int64_t ldo) {
  BK_REQUIRE(u > 0 && v > 0 && p > 0 && q > 0, "kernel_contract: bad dimensions");
  BK_REQUIRE(u < (1ll << 31) && v < (1ll << 31) && p < (1ll << 20) && q < (1ll << 20), "kernel_contract: too large");
  BK_REQUIRE(trans == 0 || trans == 1, "kernel_contract: trans must be 0 or 1");
  BK_REQUIRE(sigma > 0.0, "kernel_contract: sigma must be > 0");
  BK_REQUIRE(A && B && W && out, "kernel_contract: null pointer");
  BK_REQUIRE(lda >= u && ldb >= v, "kernel_contract: leading dimension of A or B too small");
  // trans = 0: stationary rows A, loop rows B; trans = 1: the reverse
  const int64_t ns = trans ? v : u, nl = trans ? u : v;
  BK_REQUIRE(ldw >= nl && ldo >= ns, "kernel_contract: leading dimension of W or out too small");
  CentredOperands co;     // both operands moved by the column means of A (see centre_operands)
  BK_TRY(centre_operands(ctx, A, u, lda, B, v, ldb, p, &co));
  if (trans)
    return kernel_contract_centred(ctx, co.B, v, co.ldb, co.nb, co.A, u, co.lda, co.na, p, sigma, W, q, ldw, out, ldo);
  return kernel_contract_centred(ctx, co.A, u, co.lda, co.na, co.B, v, co.ldb, co.nb, p, sigma, W, q, ldw, out, ldo);
}

// ---------------------------------------------------------------------------
// grouped fused kernel contraction (group effects, csrc/grpeff.hip)
// ---------------------------------------------------------------------------
// out[:, g q .. (g + 1) q) = K(S, L[rows of group g])  W[rows of group g] for all groups in ONE launch: the loop rows come
// sorted by group, and a device-side table cuts them into segments (l_begin, l_end, group, partial slot). The kernel is
// kernel_contract_kernel, registers included; what differs is the task, (stationary tile, column chunk, segment) in place
// of (tile, chunk, split), and the loop tiles, which start at l_begin (not at a multiple of 16) and are masked by
// l < l_end (not by NL).
// A segment that is a whole group stores into out; the segments of a longer group store into their slots of `part`
// (each NS x Q, ld NS) and contract_grouped_reduce_kernel adds them in segment order. (KcgSeg: csrc/ktplan.h)
template <int KS, int CT>
__global__ __launch_bounds__(NT) void kernel_contract_grouped_kernel(
    const double* __restrict__ S, int64_t lds, int NS, const double* __restrict__ L, int64_t ldl, int P,
    const double* __restrict__ nrm_s, const double* __restrict__ nrm_l, double neg_inv_sigma,
    const double* __restrict__ W, int64_t ldw, int Q, double* __restrict__ out, int64_t ldo, double* __restrict__ part,
    const KcgSeg* __restrict__ segs, int stiles, int nchunks, int64_t ntasks) {
  __shared__ double etab[32];
  kt_exp_table(etab);
  KtTask k;
  if (!kt_task(k, stiles, nchunks, ntasks)) return;
  const KcgSeg sg = segs[k.part];
  const int s0 = k.st * 16 * KC_MS, c0 = k.cc * 16 * CT;
  const int l_end = sg.l_end, l_last = sg.l_end - 1;
  const int lane = threadIdx.x & 63, lm = lane & 15, lk = lane >> 4;

  int srow[KC_MS];
  double ns[KC_MS], sf[KC_MS][KS > 0 ? KS : 1];
  kt_stationary<KC_MS, KS>(srow, ns, sf, S, lds, NS, nrm_s, P, s0);
  const int ms = KC_MS, ks = KS > 0 ? KS : 1;   // kt_gram's trip counts (by reference: see there)
  d4 acc[KC_MS][CT];
#pragma unroll
  for (int m = 0; m < KC_MS; ++m)
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[m][c] = (d4){0.0, 0.0, 0.0, 0.0};

  for (int l0 = sg.l_begin; l0 < l_end; l0 += 16) {
    const int lrow = min(l0 + lm, l_last);   // this lane's row of the L operand (clamped inside the segment)
    double nl[4], wf[CT][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int l = l0 + lk + 4 * r;         // this lane's loop row in accumulator register r
      nl[r] = nrm_l[min(l, l_last)];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const int col = c0 + 16 * c + lm;
        wf[c][r] = (l < l_end && col < Q) ? W[l + (int64_t)col * ldw] : 0.0;
      }
    }
    d4 g[KC_MS];
    kt_gram<KC_MS, KS>(g, srow, sf, S, lds, L, ldl, lrow, P, ms, ks);
#pragma unroll
    for (int m = 0; m < KC_MS; ++m) {
      d4 e;
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = exp_nonpos_tab(kt_dist2(g[m][r], ns[m], nl[r]) * neg_inv_sigma, etab);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[m][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(e[r], wf[c][r], acc[m][c], 0, 0, 0);
    }
  }
  double* dst = sg.slot < 0 ? out + (int64_t)sg.group * Q * ldo : part + (int64_t)sg.slot * NS * Q;
  kt_store_tiles<KC_MS, CT, false>(acc, dst, sg.slot < 0 ? ldo : (int64_t)NS, s0, c0, NS, Q);
}

// the groups of several segments, and the empty ones (count 0): multi[3 i ..] = (group, first slot, segments);
// out[:, group's columns] = the sum of the group's slots in segment order (blockIdx.y strides over the entries)
__global__ void contract_grouped_reduce_kernel(int NS, int Q, int nmulti, const int* __restrict__ multi,
                                               const double* __restrict__ part, double* __restrict__ out, int64_t ldo) {
  const int64_t total = (int64_t)NS * Q;
  for (int i = blockIdx.y; i < nmulti; i += gridDim.y) {
    const int g = multi[3 * i], first = multi[3 * i + 1], cnt = multi[3 * i + 2];
    const double* p0 = part + (int64_t)first * total;
    double* o = out + (int64_t)g * Q * ldo;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
      double s = 0.0;
      for (int k = 0; k < cnt; ++k) s += p0[(int64_t)k * total + e];
      o[(e % NS) + (e / NS) * ldo] = s;
    }
  }
}

// A table of at most KCG_INLINE_SEGS segments and KCG_INLINE_MULTI multi-segment (or empty) groups travels as a kernel
// argument and is stored by this kernel: a host-to-device copy of a few hundred bytes costs more on the stream (20 to
// 50 us between the centring kernels and the pass) than the launch does.
constexpr int KCG_INLINE_SEGS = 160, KCG_INLINE_MULTI = 32;
struct KcgInline {
  KcgSeg s[KCG_INLINE_SEGS];
  int m[3 * KCG_INLINE_MULTI];
};
__global__ void contract_table_kernel(KcgInline t, int nseg, int nm3, KcgSeg* __restrict__ segs, int* __restrict__ multi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nseg) segs[i] = t.s[i];
  if (i < nm3) multi[i] = t.m[i];
}

// the loop rows in group order: Lg[r, :] = L[perm[r], :], ng[r] = nrm[perm[r]], Wg[r, :] = W[perm[r], :]
__global__ void contract_gather_kernel(int U, int P, int Q, const int* __restrict__ perm, const double* __restrict__ L,
                                       int64_t ldl, const double* __restrict__ nrm, const double* __restrict__ W,
                                       int64_t ldw, double* __restrict__ Lg, double* __restrict__ ng,
                                       double* __restrict__ Wg) {
  const int64_t total = (int64_t)U * (P + Q + 1);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(e % U);
    const int c = (int)(e / U);
    const int src = perm[r];
    if (c < P) Lg[r + (int64_t)c * U] = L[src + (int64_t)c * ldl];
    else if (c < P + Q) Wg[r + (int64_t)(c - P) * U] = W[src + (int64_t)(c - P) * ldw];
    else ng[r] = nrm[src];
  }
}

// The device side of a grouped pass: the table (segments, then the multi triples), the permutation and the gathered
// loop rows, all carved from SLOT_KCG_GATHER in that order, and the partial sums of the cut groups (SLOT_KCG_PART).
struct KcgDevice {
  const KcgSeg* segs;
  const int *multi, *perm;   // perm: only with a permutation
  double *Lg, *ng, *Wg;      // the loop rows, their norms and W in group order (u x p, u, u x q; ld u): likewise
  double* part;
};
// The pinned buffer the tables of the grouped passes (kernel_contract_grouped, kernel_loo_binsums) are uploaded from, at
// least `bytes` long, with its event: the previous upload has left the buffer before the caller overwrites it. A buffer
// of these passes' own, guarded by an event behind the upload: waiting for the STREAM here (the context's shared pinned
// buffer would need it) leaves the device idle between the centring kernels and the pass, 4 % of the whole call at
// u = v = 20 000. kcg_stage_send copies the buffer's bytes [from, to) to the same offsets of dbase and records the event.
static int kcg_stage(bigkrls_ctx* ctx, int64_t bytes, char** hb) {
  if (ctx->ev_kcg) BK_HIP(hipEventSynchronize(ctx->ev_kcg));   // (the previous call's upload has left the buffer)
  else BK_HIP(hipEventCreateWithFlags(&ctx->ev_kcg, hipEventDisableTiming));
  if (ctx->h_kcg_bytes < bytes) {
    if (ctx->h_kcg) BK_HIP(hipHostFree(ctx->h_kcg));
    ctx->h_kcg = nullptr;
    ctx->h_kcg_bytes = 0;
    BK_HIP(hipHostMalloc((void**)&ctx->h_kcg, (size_t)bytes + 4096, hipHostMallocDefault));
    ctx->h_kcg_bytes = bytes + 4096;
  }
  *hb = ctx->h_kcg;
  return BIGKRLS_OK;
}
static int kcg_stage_send(bigkrls_ctx* ctx, char* dbase, int64_t from, int64_t to) {
  BK_HIP(hipMemcpyAsync(dbase + from, ctx->h_kcg + from, (size_t)(to - from), hipMemcpyHostToDevice, ctx->stream));
  BK_HIP(hipEventRecord(ctx->ev_kcg, ctx->stream));
  return BIGKRLS_OK;
}

// Carves the buffers and sends the table and, if there is one, the permutation (perm: group_order's).
static int kcg_upload(bigkrls_ctx* ctx, const GroupedPlan& pl, const std::vector<int32_t>& perm, int64_t u, int64_t v,
                      int64_t p, int64_t q, KcgDevice* d) {
  hipStream_t st = ctx->stream;
  const bool identity = perm.empty();
  const int64_t nseg = (int64_t)pl.segs.size(), nmulti = (int64_t)pl.multi.size() / 3;
  const int64_t b_seg = nseg * (int64_t)sizeof(KcgSeg), b_mu = (nmulti * 12 + 15) / 16 * 16;
  const int64_t b_perm = identity ? 0 : (u * 4 + 15) / 16 * 16, b_idx = b_seg + b_mu + b_perm;
  const int64_t gather_doubles = identity ? 0 : u * (p + q + 1);
  void* pg = nullptr;
  void* ppart = nullptr;
  BK_TRY(ws_get(ctx, SLOT_KCG_GATHER, b_idx + gather_doubles * (int64_t)sizeof(double) + 64, &pg));
  BK_TRY(ws_get(ctx, SLOT_KCG_PART, std::max<int64_t>(pl.nslots, 1) * v * q * (int64_t)sizeof(double), &ppart));
  char* dbase = (char*)pg;
  d->segs = (const KcgSeg*)dbase;
  d->multi = (const int*)(dbase + b_seg);
  d->perm = (const int*)(dbase + b_seg + b_mu);
  d->Lg = (double*)(dbase + b_idx);
  d->ng = d->Lg + u * p;
  d->Wg = d->ng + u;
  d->part = (double*)ppart;
  const bool inline_table = nseg <= KCG_INLINE_SEGS && nmulti <= KCG_INLINE_MULTI;
  if (inline_table) {
    KcgInline t;
    std::memcpy(t.s, pl.segs.data(), (size_t)b_seg);
    if (nmulti > 0) std::memcpy(t.m, pl.multi.data(), (size_t)nmulti * 12);
    hipLaunchKernelGGL(contract_table_kernel, dim3(1), dim3(256), 0, st, t, (int)nseg, (int)(3 * nmulti),
                       (KcgSeg*)dbase, (int*)(dbase + b_seg));
    BK_CHECK_LAUNCH();
  }
  if (inline_table && identity) return BIGKRLS_OK;
  char* hb = nullptr;
  BK_TRY(kcg_stage(ctx, b_idx, &hb));
  const int64_t from = inline_table ? b_seg + b_mu : 0;      // (the table is already there: the permutation alone)
  if (!inline_table) {
    std::memcpy(hb, pl.segs.data(), (size_t)b_seg);
    if (nmulti > 0) std::memcpy(hb + b_seg, pl.multi.data(), (size_t)nmulti * 12);
  }
  if (!identity) std::memcpy(hb + b_seg + b_mu, perm.data(), (size_t)u * 4);
  return kcg_stage_send(ctx, dbase, from, b_idx);
}

// For operands that are already centred and come with their squared row norms (kernel_contract_centred's contract): S the
// stationary rows (v x p, lds), L the loop rows (u x p, ldl) with the labels h_group, W u x q.
int kernel_contract_grouped_centred(bigkrls_ctx* ctx, const double* S, int64_t v, int64_t lds, const double* nrm_s,
                                    const double* L, int64_t u, int64_t ldl, const double* nrm_l, int64_t p, double sigma,
                                    const double* W, int64_t q, int64_t ldw, const int64_t* h_group, int64_t G,
                                    double* out, int64_t ldo) {
  BK_REQUIRE(u > 0 && v > 0 && p > 0 && q > 0, "kernel_contract_grouped: bad dimensions");
  BK_REQUIRE(u < (1ll << 31) && v < (1ll << 31) && p < (1ll << 20) && q < (1ll << 20), "kernel_contract_grouped: too large");
  BK_REQUIRE(sigma > 0.0, "kernel_contract_grouped: sigma must be > 0");
  BK_REQUIRE(S && L && nrm_s && nrm_l && W && out && h_group, "kernel_contract_grouped: null pointer");
  BK_REQUIRE(lds >= v && ldl >= u && ldw >= u && ldo >= v, "kernel_contract_grouped: leading dimension too small");
  BK_REQUIRE(G * q < (1ll << 31) && v * q < (1ll << 40), "kernel_contract_grouped: out too large");
  BK_REQUIRE(G >= 1, "kernel_contract_grouped: G must be at least 1: the label of row 1 is outside [0, G)");
  hipStream_t st = ctx->stream;
  // the rows of one group in their original order (the host works while the device centres the operands)
  const GroupOrder go = group_order(h_group, u, G);
  BK_REQUIRE(go.bad < 0, "kernel_contract_grouped: the label of row " + std::to_string(go.bad + 1) + " is outside [0, G)");
  const bool identity = go.perm.empty();

  const int CT = q <= 16 ? 1 : (q <= 32 ? 2 : 4);
  using KcgFn = void (*)(const double*, int64_t, int, const double*, int64_t, int, const double*, const double*, double,
                         const double*, int64_t, int, double*, int64_t, double*, const KcgSeg*, int, int, int64_t);
  const KcgFn fn = with_ks(ks_of(p), [&](auto ks) -> KcgFn {
    constexpr int KS = decltype(ks)::value;
    if (CT == 1) return kernel_contract_grouped_kernel<KS, 1>;
    if (CT == 2) return kernel_contract_grouped_kernel<KS, 2>;
    return kernel_contract_grouped_kernel<KS, 4>;
  });
  const int64_t stiles = (v + 16 * KC_MS - 1) / (16 * KC_MS);
  const int64_t nchunks = (q + 16 * CT - 1) / (16 * CT);
  int64_t slots = 0;
  BK_TRY(wave_slots(ctx, (const void*)fn, &slots));
  // the slots of the cut groups hold at most 64 MB
  const GroupedPlan pl = plan_grouped_segments(go.off.data(), G, stiles * nchunks, slots,
                                               (64ll << 20) / (v * q * (int64_t)sizeof(double)));
  const int64_t nmulti = (int64_t)pl.multi.size() / 3;
  const int64_t ntasks = stiles * nchunks * (int64_t)pl.segs.size();
  BK_REQUIRE((ntasks + 3) / 4 < (1ll << 31), "kernel_contract_grouped: too many tiles");
  KcgDevice d;
  BK_TRY(kcg_upload(ctx, pl, go.perm, u, v, p, q, &d));

  BK_TRY(prof_begin(ctx, "kernel_contract_grouped", 2.0 * (double)u * (double)v * (double)(p + q)));
  if (!identity) {
    const int blocks = (int)std::min<int64_t>((u * (p + q + 1) + 255) / 256, 8192);
    hipLaunchKernelGGL(contract_gather_kernel, dim3(blocks), dim3(256), 0, st, (int)u, (int)p, (int)q, d.perm, L, ldl, nrm_l,
                       W, ldw, d.Lg, d.ng, d.Wg);
    BK_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(fn, dim3((unsigned)((ntasks + 3) / 4)), dim3(NT), 0, st, S, lds, (int)v, identity ? L : d.Lg,
                     identity ? ldl : u, (int)p, nrm_s, identity ? nrm_l : d.ng, -1.0 / sigma, identity ? W : d.Wg,
                     identity ? ldw : u, (int)q, out, ldo, d.part, d.segs, (int)stiles, (int)nchunks, ntasks);
  BK_CHECK_LAUNCH();
  if (nmulti > 0) {
    const dim3 grid((unsigned)std::min<int64_t>((v * q + 255) / 256, 1024), (unsigned)std::min<int64_t>(nmulti, 1024));
    hipLaunchKernelGGL(contract_grouped_reduce_kernel, grid, dim3(256), 0, st, (int)v, (int)q, (int)nmulti, d.multi,
                       (const double*)d.part, out, ldo);
    BK_CHECK_LAUNCH();
  }
  BK_TRY(prof_end(ctx, "kernel_contract_grouped"));
  return BIGKRLS_OK;
}

int kernel_contract_grouped(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda, const double* B, int64_t v,
                            int64_t ldb, int64_t p, double sigma, const double* W, int64_t q, int64_t ldw,
                            const int64_t* h_group, int64_t G, double* out, int64_t ldo) {
  BK_REQUIRE(u > 0 && v > 0 && p > 0 && q > 0, "kernel_contract_grouped: bad dimensions");
  BK_REQUIRE(u < (1ll << 31) && v < (1ll << 31) && p < (1ll << 20) && q < (1ll << 20), "kernel_contract_grouped: too large");
  BK_REQUIRE(A && B && W && out && h_group, "kernel_contract_grouped: null pointer");
  BK_REQUIRE(lda >= u && ldb >= v, "kernel_contract_grouped: leading dimension of A or B too small");
  // (the labels are checked by the centred entry, on the host while the device centres the operands)
  CentredOperands co;     // both operands moved by the column means of A (see centre_operands)
  BK_TRY(centre_operands(ctx, A, u, lda, B, v, ldb, p, &co));
  return kernel_contract_grouped_centred(ctx, co.B, v, co.ldb, co.nb, co.A, u, co.lda, co.na, p, sigma, W, q, ldw, h_group,
                                         G, out, ldo);
}

// ---------------------------------------------------------------------------
// fused leave-one-column-out column sums (partial dependence, csrc/pdep.hip)
// ---------------------------------------------------------------------------
// out[l, jj] = sum_i exp(-(||A_i - B_l||^2 - (A[i,c] - B[l,c])^2) / sigma), c = cols[jj]: the column sums of the kernel
// of the two operands with column c left out of the distance, for every selected column in ONE pass. The unfused route
// is one kernel_contract(trans = 1, W = ones) per column on copies of the operands without that column: it rebuilds the
// Gram tile per column and spends 16 MFMAs per tile on a contraction with a vector of ones.
// The frame (kt_*) with 64 stationary rows (rows of B, KL_MS = 4 MFMA tiles) and a chunk of KL_CW selected columns per
// wave; d2 is kept, ONCE per tile, in place of G, and then
//   per selected column: dj = L[l,c] - S[s,c],  e = exp(-max(d2 - dj^2, 0) / sigma),  acc[m][j] += e
// The leave-out exponent is evaluated directly: K exp(+dj^2 / sigma) would be 0 * inf for rows that are far apart in
// column c alone. Nothing is contracted by MFMA: a lane adds its own 4 loop rows per tile (one short chain, then one add
// into the accumulator, so the accumulator's chain is nl / 16 long), and the four lane groups of a register (lane >> 4)
// are added with shuffles after the loop. Loop rows past nl are weighted by 0 (mk), stationary rows past ns are computed
// on a clamped row and not written. Loop splits and their fixed-order reduction (contract_reduce_kernel) as
// kernel_contract: no atomics, two calls are bitwise identical.
// Chunk width, registers per lane (a double is two; 512 in the unified file, 256 at two waves per SIMD, which
// __launch_bounds__(NT, 2) holds the allocator to): accumulators 4 x KL_CW doubles and the stationary rows' selected-column
// values, resident for the whole loop, 4 x KL_CW doubles: 16 KL_CW registers; resident Gram fragments sf 4 x KS <= 32
// doubles = 64; d2 16 doubles = 32; the loop rows' values of the column in work and of the next one 8 doubles = 16;
// masks, norms, row indices and addresses about 40; the temporaries of the exponentials in flight about 30. KL_CW = 8:
// 128 + 64 + 32 + 16 + 40 + 30 = 310 > 256 at P = 32 (KS = 8), 286 at P = 20 -- one wave per SIMD, or spills inside the
// loop. KL_CW = 4: 64 + 64 + 32 + 16 + 40 + 30 = 246 (P = 32), 222 (P = 20) -- the compiler reports 251 (KS = 8), 236
// (KS = 5), 229 (KS = 0), no scratch: two waves per SIMD, the second wave's exponentials (fp64 VALU) covering the first
// one's loads and MFMAs. The price of the narrower chunk is the Gram tile:
// it is rebuilt per chunk, 4 KS MFMAs (<= 32) per 64 x 16 tile against 4 x 16 x KL_CW exponentials of ~30 fp64
// instructions each -- with KL_CW = 4 still below a tenth of the wave's issue slots.
// The selected columns travel as a kernel argument (at most KL_GROUP per launch, more columns: more launches), so the
// host's list needs no device copy and no synchronisation.
constexpr int KL_MS = 4;       // 16-row stationary tiles per wave
constexpr int KL_CW = 4;       // selected columns per wave (the chunk width)
struct LooCols {
  int c[KL_GROUP];
};

template <int KS>
__global__ __launch_bounds__(NT, 2) void kernel_loo_colsums_kernel(
    const double* __restrict__ S, int64_t lds, int NS, const double* __restrict__ L, int64_t ldl, int NL, int P,
    const double* __restrict__ nrm_s, const double* __restrict__ nrm_l, double neg_inv_sigma, LooCols cols, int NC,
    double* __restrict__ out, int64_t ldo, int64_t split_stride, int stiles, int nchunks, int nsplit, int ltiles,
    int64_t ntasks) {
  __shared__ double etab[32];
  kt_exp_table(etab);
  KtTask k;
  if (!kt_task(k, stiles, nchunks, ntasks)) return;
  const int sp = (int)k.part, cc = k.cc;
  const int s0 = k.st * 16 * KL_MS;
  // the chunks share the columns evenly (widths differ by at most one, none above KL_CW)
  const int c0 = (int)((int64_t)NC * cc / nchunks), ncw = (int)((int64_t)NC * (cc + 1) / nchunks) - c0;
  const int t_begin = kt_split_begin(ltiles, sp, nsplit), t_end = kt_split_begin(ltiles, sp + 1, nsplit);
  const int lane = threadIdx.x & 63, lm = lane & 15, lk = lane >> 4;

  int srow[KL_MS];
  double ns[KL_MS], sf[KL_MS][KS > 0 ? KS : 1];
  kt_stationary<KL_MS, KS>(srow, ns, sf, S, lds, NS, nrm_s, P, s0);
  const int ms = KL_MS, ks = KS > 0 ? KS : 1;   // kt_gram's trip counts (by reference: see there)
  // the chunk's columns (wave-uniform; one past the chunk's end repeats its last column and is never accumulated) and
  // the stationary rows' values in them
  int64_t coff[KL_CW];
  double sc[KL_MS][KL_CW], acc[KL_MS][KL_CW];
#pragma unroll
  for (int j = 0; j < KL_CW; ++j) {
    const int col = cols.c[c0 + min(j, ncw - 1)];
    coff[j] = (int64_t)col * ldl;
#pragma unroll
    for (int m = 0; m < KL_MS; ++m) {
      sc[m][j] = S[srow[m] + (int64_t)col * lds];
      acc[m][j] = 0.0;
    }
  }

  for (int t = t_begin; t < t_end; ++t) {
    const int l0 = t * 16;
    const int lrow = min(l0 + lm, NL - 1);   // this lane's row of the L operand
    const double* lp[4];                      // this lane's loop row in accumulator register r
    double nl[4], mk[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int l = l0 + lk + 4 * r;
      lp[r] = L + min(l, NL - 1);
      nl[r] = nrm_l[min(l, NL - 1)];
      mk[r] = l < NL ? 1.0 : 0.0;
    }
    double lv[4];                             // the loop rows' values in the first column: in flight behind the MFMAs
#pragma unroll
    for (int r = 0; r < 4; ++r) lv[r] = lp[r][coff[0]];
    d4 g[KL_MS];
    kt_gram<KL_MS, KS>(g, srow, sf, S, lds, L, ldl, lrow, P, ms, ks);
    // the squared distance over ALL columns in place of G, once per tile
#pragma unroll
    for (int m = 0; m < KL_MS; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) g[m][r] = kt_dist2(g[m][r], ns[m], nl[r]);
#pragma unroll
    for (int j = 0; j < KL_CW; ++j) {
      if (j < ncw) {                          // (wave-uniform)
        double lnext[4];
        if (j + 1 < KL_CW) {
#pragma unroll
          for (int r = 0; r < 4; ++r) lnext[r] = lp[r][coff[j + 1]];
        }
#pragma unroll
        for (int m = 0; m < KL_MS; ++m) {
          double tsum = 0.0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double dj = lv[r] - sc[m][j];
            const double x = fmax(fma(-dj, dj, g[m][r]), 0.0);
            tsum = fma(exp_nonpos_tab(x * neg_inv_sigma, etab), mk[r], tsum);
          }
          acc[m][j] += tsum;
        }
        if (j + 1 < KL_CW) {
#pragma unroll
          for (int r = 0; r < 4; ++r) lv[r] = lnext[r];
        }
      }
    }
  }
  kt_store_lane_sums<KL_MS, KL_CW>(acc, out + (int64_t)sp * split_stride, ldo, s0, c0, ncw, NS);
}

// out (ns x n_cols, ldo) for operands that are already centred, with their squared row norms: S the stationary rows
// (the rows the sums belong to), L the loop rows (the rows summed over); h_cols on the host, 0-based, validated here.
static int kernel_loo_colsums_centred(bigkrls_ctx* ctx, const double* S, int64_t ns, int64_t lds, const double* nrm_s,
                                      const double* L, int64_t nl, int64_t ldl, const double* nrm_l, int64_t p,
                                      double sigma, const int64_t* h_cols, int64_t n_cols, double* out, int64_t ldo) {
  using KlFn = void (*)(const double*, int64_t, int, const double*, int64_t, int, int, const double*, const double*,
                        double, LooCols, int, double*, int64_t, int64_t, int, int, int, int, int64_t);
  const KlFn fn = with_ks(ks_of(p), [](auto ks) -> KlFn { return kernel_loo_colsums_kernel<decltype(ks)::value>; });
  int64_t slots = 0;
  BK_TRY(wave_slots(ctx, (const void*)fn, &slots));
  const int64_t stiles = (ns + 16 * KL_MS - 1) / (16 * KL_MS);
  const int64_t ltiles = (nl + 15) / 16;
  for (int64_t g0 = 0; g0 < n_cols; g0 += KL_GROUP) {
    const int64_t nc = std::min<int64_t>(KL_GROUP, n_cols - g0);
    LooCols lc;
    for (int64_t j = 0; j < KL_GROUP; ++j) lc.c[j] = (int)h_cols[g0 + std::min(j, nc - 1)];
    const int64_t nchunks = (nc + KL_CW - 1) / KL_CW;
    const int64_t nsplit = plan_loop_splits(stiles * nchunks, slots, ltiles, ns * nc * (int64_t)sizeof(double));
    const int64_t ntasks = stiles * nchunks * nsplit;
    BK_REQUIRE((ntasks + 3) / 4 < (1ll << 31), "kernel_loo_colsums: too many tiles");
    BK_TRY(launch_loop_splits(ctx, SLOT_LOO_PART, nsplit, ns, nc, out + g0 * ldo, ldo, nullptr,
                              [&](double* dst, int64_t ldd, int64_t split_stride) -> int {
      BK_TRY(prof_begin(ctx, "kernel_loo_colsums", (double)ns * (double)nl * (double)nc));
      hipLaunchKernelGGL(fn, dim3((unsigned)((ntasks + 3) / 4)), dim3(NT), 0, ctx->stream, S, lds, (int)ns, L, ldl,
                         (int)nl, (int)p, nrm_s, nrm_l, -1.0 / sigma, lc, (int)nc, dst, ldd, split_stride, (int)stiles,
                         (int)nchunks, (int)nsplit, (int)ltiles, ntasks);
      return BIGKRLS_OK;
    }));
    BK_TRY(prof_end(ctx, "kernel_loo_colsums"));
  }
  return BIGKRLS_OK;
}

int kernel_loo_colsums(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda, const double* B, int64_t v,
                       int64_t ldb, int64_t p, double sigma, const int64_t* h_cols, int64_t n_cols, double* out,
                       int64_t ldo) {
  BK_REQUIRE(u > 0 && v > 0 && p > 0, "kernel_loo_colsums: bad dimensions");
  BK_REQUIRE(u < (1ll << 31) && v < (1ll << 31) && p < (1ll << 20), "kernel_loo_colsums: too large");
  BK_REQUIRE(sigma > 0.0, "kernel_loo_colsums: sigma must be > 0");
  BK_REQUIRE(A && B && h_cols && out, "kernel_loo_colsums: null pointer");
  BK_REQUIRE(lda >= u && ldb >= v, "kernel_loo_colsums: leading dimension of A or B too small");
  BK_REQUIRE(ldo >= v, "kernel_loo_colsums: leading dimension of out too small");
  BK_REQUIRE(n_cols >= 1 && n_cols < (1ll << 20), "kernel_loo_colsums: n_cols must be at least 1 (and below 2^20)");
  for (int64_t j = 0; j < n_cols; ++j)
    BK_REQUIRE(h_cols[j] >= 0 && h_cols[j] < p, "kernel_loo_colsums: column index " + std::to_string(h_cols[j]) +
                                                    " outside [0, " + std::to_string(p) + ")");
  CentredOperands co;     // both operands moved by the column means of A (see centre_operands)
  BK_TRY(centre_operands(ctx, A, u, lda, B, v, ldb, p, &co));
  // the rows of B are stationary, the rows of A the loop (kernel_contract's trans = 1)
  return kernel_loo_colsums_centred(ctx, co.B, v, co.ldb, co.nb, co.A, u, co.lda, co.na, p, sigma, h_cols, n_cols, out, ldo);
}

// ---------------------------------------------------------------------------
// fused leave-out moments (conditional effects, csrc/condeff.hip)
// ---------------------------------------------------------------------------
// out[l, e] = sum_i wgt exp(-max(d2(i,l) - dc^2 - [kind = 2] dj^2, 0) / sigma), dc = A[i,c] - B[l,c], dj = A[i,j] - B[l,j],
// for entries e = (kind, c, j):  kind 0: wgt = 1 (kernel_loo_colsums' quantity);  kind 1: wgt = B[l,j] - A[i,j];
// kind 2: wgt = 1 and column j left out as well. kernel_loo_colsums_kernel's use of the frame (d2 once per tile,
// lane-group sums) with the chunk redefined: the host sorts the entries by c and a chunk holds up to CW entries of ONE c, so
//   base = max(d2 - dc^2, 0)                        once per chunk and row pair,
//   e01  = exp(-base / sigma)                       once for ALL kind-0 and kind-1 entries of the chunk,
//   kind 0: acc += e01;   kind 1: acc += e01 (S[s,j] - L[l,j])   -- one fused multiply-add on e01, no further exp;
//   kind 2: acc += exp(-max(base - dj^2, 0) / sigma)             -- its own exponential.
// max(max(a, 0) - b, 0) = max(a - b, 0) for b >= 0, so clamping base first changes nothing. The exponents are formed
// directly (never K exp(+dc^2 / sigma)); the weight is the difference of the two centred copies, translation invariant
// (S_j M0 - sum L_j e would cancel where the rows are close in column j). The kinds are wave-uniform (kernel argument).
// Registers per lane beside kernel_loo_colsums_kernel's: the stationary and loop values of column c (4 + 4 doubles) and
// the loop rows' values of all CW entry columns, loaded behind the MFMAs (4 CW doubles instead of 8). The
// compiler's figures per KS and the chunk width they led to: DESIGN.md section 4, "Conditional effects".
constexpr int KM_CW = 3;       // entries per wave (the chunk width) ...
constexpr int KM_CW_KS8 = 2;   // ... and with KS = 8 (29 <= P <= 32), where the resident fragments leave room for two
// (LooMomentEntries, LooMomentDest, and KL_GROUP entries per launch: csrc/ktplan.h)

template <int KS, int CW>
__global__ __launch_bounds__(NT, 2) void kernel_loo_moments_kernel(
    const double* __restrict__ S, int64_t lds, int NS, const double* __restrict__ L, int64_t ldl, int NL, int P,
    const double* __restrict__ nrm_s, const double* __restrict__ nrm_l, double neg_inv_sigma, LooMomentEntries ent,
    double* __restrict__ out, int64_t ldo, int64_t split_stride, int stiles, int nchunks, int nsplit, int ltiles,
    int64_t ntasks) {
  __shared__ double etab[32];
  kt_exp_table(etab);
  KtTask k;
  if (!kt_task(k, stiles, nchunks, ntasks)) return;
  const int sp = (int)k.part;
  const int s0 = k.st * 16 * KL_MS;
  const int e0 = ent.begin[k.cc], ncw = ent.begin[k.cc + 1] - e0;   // (1 <= ncw <= CW)
  const int t_begin = kt_split_begin(ltiles, sp, nsplit), t_end = kt_split_begin(ltiles, sp + 1, nsplit);
  const int lane = threadIdx.x & 63, lm = lane & 15, lk = lane >> 4;

  int srow[KL_MS];
  double ns[KL_MS], sf[KL_MS][KS > 0 ? KS : 1];
  kt_stationary<KL_MS, KS>(srow, ns, sf, S, lds, NS, nrm_s, P, s0);
  const int ms = KL_MS, ks = KS > 0 ? KS : 1;   // kt_gram's trip counts (by reference: see there)
  // the chunk's column c and its entries (wave-uniform; a slot past the chunk's end has kind -1 and is never
  // accumulated), and the stationary rows' values in their columns
  const int ccol = ent.c[e0];
  const int64_t coffc = (int64_t)ccol * ldl;
  double scv[KL_MS];
#pragma unroll
  for (int m = 0; m < KL_MS; ++m) scv[m] = S[srow[m] + (int64_t)ccol * lds];
  int kind[CW];
  int64_t joff[CW];
  double sj[KL_MS][CW], acc[KL_MS][CW];
  bool has01 = false;
#pragma unroll
  for (int j = 0; j < CW; ++j) {
    const int e = e0 + min(j, ncw - 1);
    kind[j] = j < ncw ? ent.kind[e] : -1;
    has01 = has01 || kind[j] == 0 || kind[j] == 1;
    const int col = ent.j[e];
    joff[j] = (int64_t)col * ldl;
#pragma unroll
    for (int m = 0; m < KL_MS; ++m) {
      sj[m][j] = S[srow[m] + (int64_t)col * lds];
      acc[m][j] = 0.0;
    }
  }

  for (int t = t_begin; t < t_end; ++t) {
    const int l0 = t * 16;
    const int lrow = min(l0 + lm, NL - 1);   // this lane's row of the L operand
    const double* lp[4];                      // this lane's loop row in accumulator register r
    double nl[4], mk[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int l = l0 + lk + 4 * r;
      lp[r] = L + min(l, NL - 1);
      nl[r] = nrm_l[min(l, NL - 1)];
      mk[r] = l < NL ? 1.0 : 0.0;
    }
    double lc[4], lv[CW][4];               // the loop rows' values in column c and in the entries' columns:
#pragma unroll                                // in flight behind the MFMAs
    for (int r = 0; r < 4; ++r) lc[r] = lp[r][coffc];
#pragma unroll
    for (int j = 0; j < CW; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) lv[j][r] = lp[r][joff[j]];
    d4 g[KL_MS];
    kt_gram<KL_MS, KS>(g, srow, sf, S, lds, L, ldl, lrow, P, ms, ks);
#pragma unroll
    for (int m = 0; m < KL_MS; ++m) {
      double tsum[CW];
#pragma unroll
      for (int j = 0; j < CW; ++j) tsum[j] = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // the squared distance over all columns, then without column c
        const double d2 = kt_dist2(g[m][r], ns[m], nl[r]);
        const double dc = lc[r] - scv[m];
        const double base = fmax(fma(-dc, dc, d2), 0.0);
        double e01 = 0.0;
        if (has01) e01 = exp_nonpos_tab(base * neg_inv_sigma, etab) * mk[r];   // (wave-uniform)
#pragma unroll
        for (int j = 0; j < CW; ++j) {
          if (kind[j] == 0) {                   // (wave-uniform, as the two below)
            tsum[j] += e01;
          } else if (kind[j] == 1) {
            tsum[j] = fma(e01, sj[m][j] - lv[j][r], tsum[j]);
          } else if (kind[j] == 2) {
            const double dj = lv[j][r] - sj[m][j];
            const double x = fmax(fma(-dj, dj, base), 0.0);
            tsum[j] = fma(exp_nonpos_tab(x * neg_inv_sigma, etab), mk[r], tsum[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < CW; ++j) acc[m][j] += tsum[j];
    }
  }
  kt_store_lane_sums<KL_MS, CW>(acc, out + (int64_t)sp * split_stride, ldo, s0, e0, ncw, NS);
}

// out[s, dest.d[blockIdx.y]] = src[s, blockIdx.y]: a launch's columns (sorted by c) to the caller's entry order
__global__ void loo_moments_scatter_kernel(int NS, const double* __restrict__ src, LooMomentDest dest,
                                           double* __restrict__ out, int64_t ldo) {
  const int e = blockIdx.y;
  double* o = out + (int64_t)dest.d[e] * ldo;
  const double* s = src + (int64_t)e * NS;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < NS; i += gridDim.x * blockDim.x) o[i] = s[i];
}

__global__ void loo_moments_fill_kernel(int NS, double value, double* __restrict__ o) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < NS; i += gridDim.x * blockDim.x) o[i] = value;
}

// every entry (kind, c, j): a known kind, its columns inside [0, p), j another column than c
static int loo_moments_check_entries(const int64_t* h_entries, int64_t n_entries, int64_t p) {
  for (int64_t e = 0; e < n_entries; ++e) {
    const int64_t kind = h_entries[3 * e], c = h_entries[3 * e + 1], j = h_entries[3 * e + 2];
    const std::string where = "kernel_loo_moments: entry " + std::to_string(e) + " (kind " + std::to_string(kind) +
                              ", c " + std::to_string(c) + ", j " + std::to_string(j) + "): ";
    BK_REQUIRE(kind >= 0 && kind <= 2, where + "unknown kind");
    BK_REQUIRE(c >= 0 && c < p, where + "column c outside [0, " + std::to_string(p) + ")");
    if (kind != 0) {
      BK_REQUIRE(j >= 0 && j < p, where + "column j outside [0, " + std::to_string(p) + ")");
      BK_REQUIRE(j != c, where + "j must differ from c");
    }
  }
  return BIGKRLS_OK;
}

int kernel_loo_moments(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda, const double* B, int64_t v,
                       int64_t ldb, int64_t p, double sigma, const int64_t* h_entries, int64_t n_entries, double* out,
                       int64_t ldo) {
  BK_REQUIRE(u > 0 && v > 0 && p > 0, "kernel_loo_moments: bad dimensions");
  BK_REQUIRE(u < (1ll << 31) && v < (1ll << 31) && p < (1ll << 20), "kernel_loo_moments: too large");
  BK_REQUIRE(sigma > 0.0, "kernel_loo_moments: sigma must be > 0");
  BK_REQUIRE(A && B && h_entries && out, "kernel_loo_moments: null pointer");
  BK_REQUIRE(lda >= u && ldb >= v, "kernel_loo_moments: leading dimension of A or B too small");
  BK_REQUIRE(ldo >= v, "kernel_loo_moments: leading dimension of out too small");
  BK_REQUIRE(n_entries >= 1 && n_entries < (1ll << 20), "kernel_loo_moments: n_entries must be at least 1 (and below 2^20)");
  BK_TRY(loo_moments_check_entries(h_entries, n_entries, p));
  // the entries that leave out every column are written as such; the others by c, KL_GROUP per launch (csrc/ktplan.h)
  const int64_t cw = ks_of(p) == 8 ? KM_CW_KS8 : KM_CW;
  const LooPlan pl = plan_loo_moments(h_entries, n_entries, p, cw);
  for (int64_t e : pl.trivial) {
    const int blocks = (int)std::min<int64_t>((v + 255) / 256, 1024);
    hipLaunchKernelGGL(loo_moments_fill_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (int)v, (double)u, out + e * ldo);
    BK_CHECK_LAUNCH();
  }
  if (pl.launches.empty()) return BIGKRLS_OK;

  CentredOperands co;     // both operands moved by the column means of A (see centre_operands)
  BK_TRY(centre_operands(ctx, A, u, lda, B, v, ldb, p, &co));
  // the rows of B are stationary, the rows of A the loop (kernel_contract's trans = 1)
  const double *S = co.B, *L = co.A, *nrm_s = co.nb, *nrm_l = co.na;
  const int64_t ns = v, nl = u, lds = co.ldb, ldl = co.lda;
  using KmFn = void (*)(const double*, int64_t, int, const double*, int64_t, int, int, const double*, const double*,
                        double, LooMomentEntries, double*, int64_t, int64_t, int, int, int, int, int64_t);
  const KmFn fn = with_ks(ks_of(p), [](auto ks) -> KmFn {
    constexpr int KS = decltype(ks)::value;
    return kernel_loo_moments_kernel<KS, KS == 8 ? KM_CW_KS8 : KM_CW>;
  });
  int64_t slots = 0;
  BK_TRY(wave_slots(ctx, (const void*)fn, &slots));
  const int64_t stiles = (ns + 16 * KL_MS - 1) / (16 * KL_MS);
  const int64_t ltiles = (nl + 15) / 16;
  for (const LooLaunch& ln : pl.launches) {
    const int64_t nc = ln.nc, nchunks = ln.nchunks;
    const int64_t nsplit = plan_loop_splits(stiles * nchunks, slots, ltiles, ns * nc * (int64_t)sizeof(double));
    const int64_t ntasks = stiles * nchunks * nsplit;
    BK_REQUIRE((ntasks + 3) / 4 < (1ll << 31), "kernel_loo_moments: too many tiles");
    // the launch's columns go into out at once, or into a staging buffer and are scattered from there afterwards
    double* tmp = nullptr;
    BK_TRY(launch_loop_splits(ctx, SLOT_LOO_PART, nsplit, ns, nc, ln.in_place ? out + ln.first * ldo : nullptr, ldo,
                              &tmp, [&](double* dst, int64_t ldd, int64_t split_stride) -> int {
      BK_TRY(prof_begin(ctx, "kernel_loo_moments", (double)ns * (double)nl * (double)ln.nexp));
      hipLaunchKernelGGL(fn, dim3((unsigned)((ntasks + 3) / 4)), dim3(NT), 0, ctx->stream, S, lds, (int)ns, L, ldl,
                         (int)nl, (int)p, nrm_s, nrm_l, -1.0 / sigma, ln.le, dst, ldd, split_stride, (int)stiles,
                         (int)nchunks, (int)nsplit, (int)ltiles, ntasks);
      return BIGKRLS_OK;
    }));
    if (!ln.in_place) {
      const int blocks = (int)std::min<int64_t>((ns + 255) / 256, 1024);
      hipLaunchKernelGGL(loo_moments_scatter_kernel, dim3(blocks, (unsigned)nc), dim3(256), 0, ctx->stream, (int)ns,
                         (const double*)tmp, ln.dest, out, ldo);
      BK_CHECK_LAUNCH();
    }
    BK_TRY(prof_end(ctx, "kernel_loo_moments"));
  }
  return BIGKRLS_OK;
}

// ---------------------------------------------------------------------------
// fused binned leave-one-column-out column sums (accumulated local effects, csrc/ale.hip)
// ---------------------------------------------------------------------------
// out[l, bin0(jj) + b] = sum over the rows i of A with label[i, jj] = b of exp(-(||A_i - B_l||^2 - (A[i,c] - B[l,c])^2) / sigma),
// c = cols[jj]: kernel_loo_colsums' quantity summed per bin of the left-out column, and the grouping differs per
// column. The frame (kt_*) with 64 stationary rows per wave as kernel_loo_colsums_kernel; the task is (stationary
// tile, segment) and a segment is a run of ONE selected column's loop rows in that column's bin order
// (plan_loo_binsums, csrc/ktplan.h), so a wave handles one column (chunk width 1) and the Gram tile is rebuilt per
// column. The loop rows are not gathered: the operands are column-major, so row idx[r] of column k is L[idx[r] + k ldl],
// and the wave reads its 16 loop rows of a tile through the column's int32 index list -- p gathered copies of A would
// cost u p^2 doubles. As in the grouped contraction the loop tiles start at l_begin (not at a multiple of 16) and are
// masked by l < l_end; a segment that is a whole bin stores into out, the segments of a cut bin into their slots of
// `part` (each NS long), added in segment order by contract_grouped_reduce_kernel with Q = 1, which also zeroes the
// empty bins: no atomics, two calls are bitwise identical.
template <int KS>
__global__ __launch_bounds__(NT, 2) void kernel_loo_binsums_kernel(
    const double* __restrict__ S, int64_t lds, int NS, const double* __restrict__ L, int64_t ldl, int NL, int P,
    const double* __restrict__ nrm_s, const double* __restrict__ nrm_l, double neg_inv_sigma, LooCols cols,
    const int* __restrict__ idx, const KcgSeg* __restrict__ segs, double* __restrict__ out, int64_t ldo,
    double* __restrict__ part, int stiles, int64_t ntasks) {
  __shared__ double etab[32];
  kt_exp_table(etab);
  KtTask k;
  if (!kt_task(k, stiles, 1, ntasks)) return;
  const KcgSeg sg = segs[k.part];
  const int s0 = k.st * 16 * KL_MS;
  const int l_end = sg.l_end, l_last = sg.l_end - 1;
  const int col = cols.c[sg.l_begin / NL];   // (positions in idx: the launch's column jl owns [jl NL, (jl + 1) NL))
  const int64_t coff = (int64_t)col * ldl;
  const int lane = threadIdx.x & 63, lm = lane & 15, lk = lane >> 4;

  int srow[KL_MS];
  double ns[KL_MS], sf[KL_MS][KS > 0 ? KS : 1];
  kt_stationary<KL_MS, KS>(srow, ns, sf, S, lds, NS, nrm_s, P, s0);
  const int ms = KL_MS, ks = KS > 0 ? KS : 1;   // kt_gram's trip counts (by reference: see there)
  double sc[KL_MS], acc[KL_MS][1];
#pragma unroll
  for (int m = 0; m < KL_MS; ++m) {
    sc[m] = S[srow[m] + (int64_t)col * lds];
    acc[m][0] = 0.0;
  }

  for (int l0 = sg.l_begin; l0 < l_end; l0 += 16) {
    const int lrow = idx[min(l0 + lm, l_last)];   // this lane's row of the L operand (clamped inside the segment)
    double nl[4], mk[4], lv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int l = l0 + lk + 4 * r;              // this lane's loop row in accumulator register r
      const int li = idx[min(l, l_last)];
      nl[r] = nrm_l[li];
      lv[r] = L[li + coff];
      mk[r] = l < l_end ? 1.0 : 0.0;
    }
    d4 g[KL_MS];
    kt_gram<KL_MS, KS>(g, srow, sf, S, lds, L, ldl, lrow, P, ms, ks);
#pragma unroll
    for (int m = 0; m < KL_MS; ++m) {
      double tsum = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double dj = lv[r] - sc[m];
        const double x = fmax(fma(-dj, dj, kt_dist2(g[m][r], ns[m], nl[r])), 0.0);
        tsum = fma(exp_nonpos_tab(x * neg_inv_sigma, etab), mk[r], tsum);
      }
      acc[m][0] += tsum;
    }
  }
  double* dst = sg.slot < 0 ? out + (int64_t)sg.group * ldo : part + (int64_t)sg.slot * NS;
  kt_store_lane_sums<KL_MS, 1>(acc, dst, 0, s0, 0, 1, NS);
}

// p = 1: out[s, blockIdx.y] = counts.v[blockIdx.y], up to KLB_FILL bins per launch (the counts as a kernel argument)
constexpr int KLB_FILL = 256;
struct BinCounts {
  double v[KLB_FILL];
};
__global__ void loo_binsums_fill_kernel(int NS, BinCounts counts, double* __restrict__ out, int64_t ldo) {
  const double c = counts.v[blockIdx.y];
  double* o = out + (int64_t)blockIdx.y * ldo;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < NS; i += gridDim.x * blockDim.x) o[i] = c;
}

int kernel_loo_binsums(bigkrls_ctx* ctx, const double* A, int64_t u, int64_t lda, const double* B, int64_t v,
                       int64_t ldb, int64_t p, double sigma, const int64_t* h_cols, int64_t n_cols,
                       const int64_t* h_labels, const int64_t* h_nbins, double* out, int64_t ldo) {
  BK_REQUIRE(u > 0 && v > 0 && p > 0, "kernel_loo_binsums: bad dimensions");
  BK_REQUIRE(u < (1ll << 31) && v < (1ll << 31) && p < (1ll << 20), "kernel_loo_binsums: too large");
  BK_REQUIRE(sigma > 0.0, "kernel_loo_binsums: sigma must be > 0");
  BK_REQUIRE(A && B && h_cols && h_labels && h_nbins && out, "kernel_loo_binsums: null pointer");
  BK_REQUIRE(lda >= u && ldb >= v, "kernel_loo_binsums: leading dimension of A or B too small");
  BK_REQUIRE(ldo >= v, "kernel_loo_binsums: leading dimension of out too small");
  BK_REQUIRE(n_cols >= 1 && n_cols < (1ll << 20), "kernel_loo_binsums: n_cols must be at least 1 (and below 2^20)");
  int64_t nbt = 0;
  for (int64_t j = 0; j < n_cols; ++j) {
    BK_REQUIRE(h_cols[j] >= 0 && h_cols[j] < p, "kernel_loo_binsums: column index " + std::to_string(h_cols[j]) +
                                                    " outside [0, " + std::to_string(p) + ")");
    BK_REQUIRE(h_nbins[j] >= 1 && h_nbins[j] < (1ll << 31), "kernel_loo_binsums: selected column " + std::to_string(j + 1) +
                                                                " must have at least 1 bin (and fewer than 2^31)");
    nbt += h_nbins[j];
  }
  BK_REQUIRE(nbt < (1ll << 31) && u * n_cols < (1ll << 40), "kernel_loo_binsums: too many bins or labels");
  hipStream_t st = ctx->stream;
  CentredOperands co{};   // both operands moved by the column means of ALL of A, not per bin (see centre_operands)
  if (p > 1) BK_TRY(centre_operands(ctx, A, u, lda, B, v, ldb, p, &co));

  using KbFn = void (*)(const double*, int64_t, int, const double*, int64_t, int, int, const double*, const double*,
                        double, LooCols, const int*, const KcgSeg*, double*, int64_t, double*, int, int64_t);
  const KbFn fn = with_ks(ks_of(p), [](auto ks) -> KbFn { return kernel_loo_binsums_kernel<decltype(ks)::value>; });
  int64_t slots = 0;
  BK_TRY(wave_slots(ctx, (const void*)fn, &slots));
  const int64_t stiles = (v + 16 * KL_MS - 1) / (16 * KL_MS);
  // every column's order, the segments and the launches, on the host while the device centres the operands; the slots
  // of the cut bins hold at most 64 MB
  const BinPlan pl = plan_loo_binsums(h_labels, u, n_cols, h_nbins, stiles, slots, (64ll << 20) / (v * (int64_t)sizeof(double)));
  BK_REQUIRE(pl.bad_row < 0, "kernel_loo_binsums: the label of row " + std::to_string(pl.bad_row + 1) + " of selected column " +
                                 std::to_string(pl.bad_col + 1) + " is outside [0, " +
                                 std::to_string(pl.bad_col >= 0 ? h_nbins[pl.bad_col] : 0) + ")");
  if (p == 1) {   // nothing is left of the distance: every term is exp(0), the sums are the bins' counts
    const int blocks = (int)std::min<int64_t>((v + 255) / 256, 1024);
    for (int64_t b0 = 0; b0 < nbt; b0 += KLB_FILL) {
      BinCounts bc;
      const int64_t cnt = std::min<int64_t>(KLB_FILL, nbt - b0);
      for (int64_t b = 0; b < cnt; ++b) bc.v[b] = (double)pl.counts[(size_t)(b0 + b)];
      hipLaunchKernelGGL(loo_binsums_fill_kernel, dim3(blocks, (unsigned)cnt), dim3(256), 0, st, (int)v, bc, out + b0 * ldo, ldo);
      BK_CHECK_LAUNCH();
    }
    return BIGKRLS_OK;
  }

  // ---- one upload for all launches: every column's index list, then per launch its segments and multi triples ----
  const int64_t b_idx = (u * n_cols * 4 + 15) / 16 * 16;
  std::vector<int64_t> seg_at, multi_at;
  int64_t bytes = b_idx, max_slots = 1;
  for (const BinLaunch& ln : pl.launches) {
    BK_REQUIRE((stiles * (int64_t)ln.plan.segs.size() + 3) / 4 < (1ll << 31), "kernel_loo_binsums: too many tiles");
    seg_at.push_back(bytes);
    bytes += (int64_t)ln.plan.segs.size() * (int64_t)sizeof(KcgSeg);
    multi_at.push_back(bytes);
    bytes += ((int64_t)ln.plan.multi.size() * 4 + 15) / 16 * 16;
    max_slots = std::max(max_slots, ln.plan.nslots);
  }
  void *pg = nullptr, *ppart = nullptr;
  BK_TRY(ws_get(ctx, SLOT_KLB_INDEX, bytes + 64, &pg));
  BK_TRY(ws_get(ctx, SLOT_KLB_PART, max_slots * v * (int64_t)sizeof(double), &ppart));
  char* dbase = (char*)pg;
  char* hb = nullptr;   // (kcg_upload's pinned buffer and event: the stream is never waited for)
  BK_TRY(kcg_stage(ctx, bytes, &hb));
  std::memcpy(hb, pl.idx.data(), (size_t)(u * n_cols) * 4);
  for (size_t i = 0; i < pl.launches.size(); ++i) {
    const GroupedPlan& gp = pl.launches[i].plan;
    std::memcpy(hb + seg_at[i], gp.segs.data(), gp.segs.size() * sizeof(KcgSeg));
    if (!gp.multi.empty()) std::memcpy(hb + multi_at[i], gp.multi.data(), gp.multi.size() * 4);
  }
  BK_TRY(kcg_stage_send(ctx, dbase, 0, bytes));

  // the rows of B are stationary, the rows of A the loop (kernel_contract's trans = 1)
  for (size_t i = 0; i < pl.launches.size(); ++i) {
    const BinLaunch& ln = pl.launches[i];
    LooCols lc;
    for (int64_t j = 0; j < KL_GROUP; ++j) lc.c[j] = (int)h_cols[ln.col0 + std::min(j, ln.ncols - 1)];
    const int64_t nseg = (int64_t)ln.plan.segs.size(), nmulti = (int64_t)ln.plan.multi.size() / 3;
    const int64_t ntasks = stiles * nseg;
    double* o = out + ln.bin0 * ldo;
    BK_TRY(prof_begin(ctx, "kernel_loo_binsums", (double)u * (double)v * (double)ln.ncols));
    if (ntasks > 0) {
      hipLaunchKernelGGL(fn, dim3((unsigned)((ntasks + 3) / 4)), dim3(NT), 0, st, co.B, co.ldb, (int)v, co.A, co.lda, (int)u,
                         (int)p, co.nb, co.na, -1.0 / sigma, lc, (const int*)dbase + ln.col0 * u,
                         (const KcgSeg*)(dbase + seg_at[i]), o, ldo, (double*)ppart, (int)stiles, ntasks);
      BK_CHECK_LAUNCH();
    }
    if (nmulti > 0) {
      const dim3 grid((unsigned)std::min<int64_t>((v + 255) / 256, 1024), (unsigned)std::min<int64_t>(nmulti, 1024));
      hipLaunchKernelGGL(contract_grouped_reduce_kernel, grid, dim3(256), 0, st, (int)v, 1, (int)nmulti,
                         (const int*)(dbase + multi_at[i]), (const double*)ppart, o, ldo);
      BK_CHECK_LAUNCH();
    }
    BK_TRY(prof_end(ctx, "kernel_loo_binsums"));
  }
  return BIGKRLS_OK;
}

// ---- the kernel matrix of one data set as an operator (kernel = "implicit": csrc/eigen.hip, csrc/fit.hip) -----------
// The centred copy of X and its squared row norms live in slots of their own, so that they survive every other kernel
// build or contraction of the context until the next kernel_op_prepare.
int kernel_op_prepare(bigkrls_ctx* ctx, const double* X, int64_t n, int64_t ldx, int64_t p, double sigma, KernelOp* op) {
  BK_REQUIRE(X && op && n > 0 && p > 0 && n < (1ll << 31) && p < (1ll << 20), "kernel operator: bad arguments");
  BK_REQUIRE(ldx >= n, "kernel operator: leading dimension of X too small");
  BK_REQUIRE(sigma > 0.0, "kernel operator: sigma must be > 0");
  void *px = nullptr, *pn = nullptr, *psh = nullptr;
  BK_TRY(ws_get(ctx, SLOT_KOP_X, n * p * (int64_t)sizeof(double), &px));
  BK_TRY(ws_get(ctx, SLOT_KOP_NORMS, n * (int64_t)sizeof(double), &pn));
  BK_TRY(ws_get(ctx, SLOT_KB_SHIFT, p * sizeof(double), &psh));
  BK_TRY(col_means(ctx, X, n, p, ldx, (double*)psh));
  BK_TRY(shift_rows_sqnorms(ctx, X, n, p, ldx, (const double*)psh, (double*)px, (double*)pn));
  op->Xc = (const double*)px;
  op->nrm = (const double*)pn;
  op->n = n;
  op->p = p;
  op->sigma = sigma;
  return BIGKRLS_OK;
}

int kernel_op_times(bigkrls_ctx* ctx, const KernelOp& op, const double* W, int64_t q, int64_t ldw, double* out,
                    int64_t ldo) {
  return kernel_contract_centred(ctx, op.Xc, op.n, op.n, op.nrm, op.Xc, op.n, op.n, op.nrm, op.p, op.sigma, W, q, ldw,
                                 out, ldo);
}

}  // namespace bk
