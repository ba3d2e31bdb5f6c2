// Two-stage tridiagonalisation (included inside eigen.hip's anonymous namespace).
//
// One-stage Householder tridiagonalisation streams the whole trailing matrix from HBM
// once per column (4N^3/3 bytes even with the symmetric tiled symv). The two-stage
// reduction moves that half of the work onto MFMA:
//
//   stage 1  full -> band (lower bandwidth b = 64): per block column a tall-skinny
//            Householder QR of the sub-band panel and a two-sided block update
//            A22 <- (I - V T'V') A22 (I - V T V') = A22 - V Z' - Z V',
//            Y = A22 V T,  Z = Y - V (T' V' Y)/2: all GEMMs; A22 is read once per PANEL.
//   stage 2  band -> tridiagonal by column-wise bulge chasing on a 2b x n band array
//            (L2 / Infinity-Cache resident). Task (s,t) = step t of sweep s applies one
//            length-b reflector to a b x b off-diagonal and a b x b diagonal block; tasks
//            with equal 2s + t are independent, so every wavefront is one launch with one
//            workgroup per task (no inter-workgroup communication inside a launch).
//   back-transform  Z <- Q1 (Q2 Z): Q2 sweep by sweep (all steps of a sweep touch
//            disjoint rows), Q1 panel by panel as compact-WY GEMMs.
//
// The algebra was prototyped against dense numpy (residual/orthogonality 1e-15) before
// being written here; tests/test_gpu_level1.py::test_eigen_* run both paths.

// (S2_B = 64, the band width == stage-1 panel width, S2_LD = 2 S2_B rows of the band array and the other plain constants
//  of the host plan: csrc/s2plan.h)
static_assert(S2_B == 64 && S2_LD == 2 * S2_B, "the kernels below are written for a band of 64 and a band array of 128 rows");
constexpr int S1_PROF_STRIDE = 8;   // bench.py's HIP-event sampling brackets every 8th panel (event overhead)

// ---------------------------------------------------------------------------
// stage 1: panel QR (right-looking dgeqr2 on an m x pw panel, ld = N)
// ---------------------------------------------------------------------------
// One launch per panel column. Launch j consumes the block partials produced by launch
// j-1 (norm of column j below its head, unscaled dots d_c = x_j' P[:,c] over rows >= j),
// forms (v_j, tau_j) and w_c = tau (P[j,c] + scale (d_c - alpha P[j,c])), applies the
// rank-1 update to the columns right of j, and -- in the same pass over the updated rows --
// produces the partials column j+1 needs. Row j of the updated columns (a row of R) goes to
// a side buffer so that no block reads P[j,c] while another writes it.
constexpr int PQ_CG = 8;   // columns per workgroup

__device__ __forceinline__ double block_sum4(double v, double* sh4) {
  v = wsum(v);
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
  __syncthreads();
  return r;
}

// partials for column 0 of a panel
__global__ __launch_bounds__(256) void pq_first(const double* __restrict__ P, int64_t ld, int m, int pw,
                                                double* __restrict__ normpart, double* __restrict__ dotpart) {
  __shared__ double sh[4];
  const int tid = threadIdx.x;
  const int r = blockIdx.x * 256 + tid;
  const int c0 = 1 + blockIdx.y * PQ_CG;
  const double x = (r < m) ? P[r] : 0.0;
  if (blockIdx.y == 0) {
    const double ss = block_sum4((r >= 1) ? x * x : 0.0, sh);
    if (tid == 0) normpart[blockIdx.x] = ss;
  }
#pragma unroll
  for (int q = 0; q < PQ_CG; ++q) {
    const int c = c0 + q;
    if (c < pw) {   // uniform
      const double d = block_sum4((r < m) ? x * P[r + (int64_t)c * ld] : 0.0, sh);
      if (tid == 0) dotpart[(int64_t)blockIdx.x * S2_B + c] = d;
    }
  }
}

__global__ __launch_bounds__(256) void pq_step(double* __restrict__ P, int64_t ld, int m, int pw, int j,
                                               const double* __restrict__ normpart,
                                               const double* __restrict__ dotpart, int np,
                                               double* __restrict__ taus, double* __restrict__ scales,
                                               double* __restrict__ betas, double* __restrict__ Rrow,
                                               const double* __restrict__ xcur, int store_xcur,
                                               double* __restrict__ xnext,
                                               double* __restrict__ normpart_next,
                                               double* __restrict__ dotpart_next) {
  // xcur[r] (r >= j) is column j as updated by the previous launch; the updated column j+1 is
  // written to xnext, NOT into P, because the other column groups of this launch still read
  // the old P[:, j+1] to form the same values (an in-place store was a cross-block race).
  __shared__ double s_w[PQ_CG + 1];   // w of this group's columns, [PQ_CG] = w of column j+1
  __shared__ double s_sc[3];
  __shared__ double s_red[4][PQ_CG + 1];
  __shared__ double s_d[PQ_CG + 1];
  const int tid = threadIdx.x;
  const int c0 = j + 1 + blockIdx.y * PQ_CG;
  const double alpha = xcur[j];
  // partial sums of the previous launch, reduced by two waves in parallel
  if (tid < 64) {
    // wave 0: dot partials of the PQ_CG + 1 columns this block needs, 4 lanes per column
    const int slot = tid & 15, part = tid >> 4;
    const int c = (slot < PQ_CG) ? c0 + slot : ((slot == PQ_CG) ? j + 1 : pw);
    double d = 0.0;
    if (c < pw)
      for (int b = part; b < np; b += 4) d += dotpart[(int64_t)b * S2_B + c];
    d += __shfl_xor(d, 16, 64);
    d += __shfl_xor(d, 32, 64);
    if (part == 0 && slot <= PQ_CG) s_d[slot] = d;
  } else if (tid < 128) {
    // wave 1: the norm of column j below its head -> Householder scalars
    double ss = 0.0;
    for (int b = tid - 64; b < np; b += 64) ss += normpart[b];
    ss = wsum(ss);
    if (tid == 64) {
      double beta, t, sc;
      if (ss == 0.0) { beta = alpha; t = 0.0; sc = 0.0; }
      else {
        beta = -copysign(hh_norm(alpha, ss), alpha);
        t = (beta - alpha) / beta;
        sc = 1.0 / (alpha - beta);
      }
      s_sc[0] = sc; s_sc[1] = t; s_sc[2] = beta;
      if (blockIdx.x == 0 && blockIdx.y == 0) { taus[j] = t; scales[j] = sc; betas[j] = beta; }
    }
  }
  __syncthreads();
  const double scale = s_sc[0], tau = s_sc[1];
  if (tid <= PQ_CG) {
    const int c = (tid < PQ_CG) ? c0 + tid : j + 1;
    if (c < pw) {
      const double pjc = P[j + (int64_t)c * ld];
      s_w[tid] = tau * (pjc + scale * (s_d[tid] - alpha * pjc));
    } else {
      s_w[tid] = 0.0;
    }
  }
  __syncthreads();
  const int r = j + blockIdx.x * 256 + tid;
  const bool inr = r < m;
  const double xr = inr ? xcur[r] : 0.0;
  const double v = inr ? ((r == j) ? 1.0 : xr * scale) : 0.0;
  if (store_xcur && blockIdx.y == 0 && inr) P[r + (int64_t)j * ld] = xr;   // column j's final home
  // updated value of column j+1 in this row (every column group recomputes it)
  double xn = 0.0;
  if (inr && j + 1 < pw) xn = P[r + (int64_t)(j + 1) * ld] - v * s_w[PQ_CG];
  const double xd = (r >= j + 1) ? xn : 0.0;   // rows of the next reflector column incl. its head
  double pv[PQ_CG];
#pragma unroll
  for (int q = 0; q < PQ_CG; ++q) pv[q] = (inr && c0 + q < pw) ? P[r + (int64_t)(c0 + q) * ld] : 0.0;
  // one combined block reduction for the PQ_CG dot partials and the norm partial
  double red[PQ_CG + 1];
#pragma unroll
  for (int q = 0; q < PQ_CG; ++q) {
    const int c = c0 + q;
    double contrib = 0.0;
    if (c < pw) {   // uniform
      const double nv = pv[q] - v * s_w[q];
      if (inr) {
        if (r == j) Rrow[j * S2_B + c] = nv;
        else if (c == j + 1) xnext[r] = nv;
        else P[r + (int64_t)c * ld] = nv;
      }
      if (c >= j + 2 && inr) contrib = xd * nv;
    }
    red[q] = wsum(contrib);
  }
  red[PQ_CG] = wsum((blockIdx.y == 0 && inr && r >= j + 2) ? xn * xn : 0.0);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int q = 0; q <= PQ_CG; ++q) s_red[tid >> 6][q] = red[q];
  }
  __syncthreads();
  if (tid <= PQ_CG) {
    const double tot = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
    if (tid < PQ_CG) {
      const int c = c0 + tid;
      if (c < pw && c >= j + 2) dotpart_next[(int64_t)blockIdx.x * S2_B + c] = tot;
    } else if (blockIdx.y == 0) {
      normpart_next[blockIdx.x] = tot;
    }
  }
}

constexpr long BC_SPIN_LIMIT = 4000000;   // watchdog: polls of ~1 us each

// Cross-lane sums on the VALU (DPP) instead of ds_bpermute: a __shfl_xor of a double is two
// dependent LDS-crossbar instructions of ~100 cycles each, a DPP move costs a few. The callers run
// with all 64 lanes active.
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// sum over the 4 lanes of a quad (every lane gets it)
__device__ __forceinline__ double quad_sum(double v) {
  v += dpp_move<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_move<0x4E>(v);   // quad_perm [2,3,0,1]
  return v;
}
__device__ __forceinline__ double lane_value(double v, int lane);
// sum over the wave; every lane holds the identical total
__device__ __forceinline__ double wave_sum(double v) {
  v = quad_sum(v);
  v += dpp_move<0x141>(v);  // row_half_mirror: the other quad of the 8-lane half
  v += dpp_move<0x140>(v);  // row_mirror: the other half of the 16-lane row
  return (lane_value(v, 0) + lane_value(v, 16)) + (lane_value(v, 32) + lane_value(v, 48));
}

// value of `v` in lane `lane` (wave-uniform index) without going through LDS
__device__ __forceinline__ double lane_value(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// Self-validating message words: every value travels as two independent 8-byte words,
// A = bits(v) and B = bits(v) ^ key(seq). The receiver polls both until A ^ B == key(seq).
// No fence, flag or store ordering is needed: a stale A with a fresh B (or vice versa) fails the
// check unless the old and new values are identical, in which case either is the right answer.
__device__ __forceinline__ unsigned long long rb_key(int seq) {
  return (unsigned long long)(unsigned)seq * 0x9E3779B97F4A7C15ull;   // seq >= 1: never 0
}
__device__ __forceinline__ void rb_send(double* box, int i, double v, unsigned long long key) {
  unsigned long long* w = (unsigned long long*)box + 2 * i;
  const unsigned long long a = (unsigned long long)__double_as_longlong(v);
  __hip_atomic_store(w, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(w + 1, a ^ key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// returns false when the watchdog fired (or another workgroup raised err)
__device__ __forceinline__ bool rb_recv(const double* box, int i, unsigned long long key, int* err,
                                        double* out) {
  const unsigned long long* w = (const unsigned long long*)box + 2 * i;
  long spins = 0;
  for (;;) {
    const unsigned long long a = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long b = __hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((a ^ b) == key) {
      *out = __longlong_as_double((long long)a);
      return true;
    }
#ifdef BK_RB_SLEEP      // (experiment build: back off between polls -- fewer uncached reads in the fabric while waiting)
    __builtin_amdgcn_s_sleep(BK_RB_SLEEP);
#endif
    if ((++spins & 255) == 0 &&
        (spins > BC_SPIN_LIMIT || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
      __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
  }
}

// ---------------------------------------------------------------------------
// Register-resident panel QR: ONE launch per panel. Workgroup k keeps rows [256k, 256k+256) of
// the m x 64 panel in registers (one row per thread) for all 64 column steps; every workgroup
// also keeps a private copy of the panel's top 64 x 64 block in LDS (row j of step j and the
// head alpha come from there, so they never have to be broadcast). The only inter-workgroup
// traffic is one all-to-all per column: 64 partial sums per workgroup (the dots of the next
// reflector column with the columns right of it, and its norm below the head), exchanged as
// self-validating message words and summed by everybody in the same fixed order, so all
// workgroups form bit-identical reflectors. Replaces 64 dependent launches per panel.
// ---------------------------------------------------------------------------
constexpr int PQ_FLAT = 27;   // up to this many workgroups the partial sums go all-to-all
constexpr int PQ_GS = 9;      // above: groups of 9 (<= 9 groups for the <= 80 workgroups of a resident panel)

__global__ __launch_bounds__(256, 1) void pq_resident(double* __restrict__ P, int64_t ld, int m,
                                                      double* __restrict__ taus, double* __restrict__ scales,
                                                      double* __restrict__ Vp, double* __restrict__ mail,
                                                      double* __restrict__ mail2, int seq_base,
                                                      int* __restrict__ err, const int* __restrict__ only_if) {
  constexpr int B = S2_B;
  // (behind pq_chol: the Householder factorisation runs only for a panel that kernel left untouched)
  if (only_if != nullptr && *only_if == 0) return;
  __shared__ double top[B][B + 1];
  __shared__ double part[4][B];
  __shared__ double fold[B / 2][256 + 1];   // [slot of the current half][row]: products staged for the column sums
  __shared__ double grp[4][B];
  __shared__ double bsum[B], bsum2[B], sbeta[B], sscale[B];
  __shared__ int s_fail;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = blockIdx.x, np = gridDim.x;
  const int r = blk * 256 + tid;
  const bool valid = r < m;
  double p[B];
#pragma unroll
  for (int c = 0; c < B; ++c) p[c] = valid ? P[r + (int64_t)c * ld] : 0.0;
  for (int e = tid; e < B * B; e += 256) {
    const int rr = e & (B - 1), c = e >> 6;
    top[rr][c] = (rr < m) ? P[rr + (int64_t)c * ld] : 0.0;
  }
  if (tid < B) { sbeta[tid] = 0.0; sscale[tid] = 0.0; }
  if (tid == 0) s_fail = 0;
  __syncthreads();
  const int ncolq = min(B, m);
  const int cc = tid & 63, gg = tid >> 6;   // receive role: column cc, workgroups gg, gg+4, ...
  double x = p[0];
  for (int j = 0; j < ncolq; ++j) {
    const unsigned long long key = rb_key(seq_base + j);
    double* boxes = mail + (int64_t)(j & 1) * np * (2 * B);   // this step's buffer: [np][B] word pairs
    // ---- partial sums over this workgroup's rows: slot c > j: x_j . P[:,c] (rows >= j);
    //      slot j: |x_j|^2 below the head (rows > j) -------------------------------------------
    // (measured per step: a 6-stage ds_bpermute butterfly with per-slot selects costs 7900 cycles.
    //  Here: 64 plain products per thread -- slots <= j are never read by anybody, slot j is the
    //  dot of column j with itself, which is the wanted norm once the head row contributes 0 --
    //  staged through LDS in two halves of 32 slots; 256 threads then add 32 rows each.)
    {
      const double xe = (r >= j) ? x : 0.0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h == 0 && j >= B / 2) continue;   // slots 0..31 are all <= j: nobody reads them (uniform)
        double prod[B / 2];
#pragma unroll
        for (int kk = 0; kk < B / 2; ++kk) prod[kk] = xe * p[h * (B / 2) + kk];
        if (r == j && (j >> 5) == h) {          // one thread: its x^2 must not enter the norm slot
#pragma unroll
          for (int kk = 0; kk < B / 2; ++kk) prod[kk] = (kk == (j & 31)) ? 0.0 : prod[kk];
        }
#pragma unroll
        for (int kk = 0; kk < B / 2; ++kk) fold[kk][tid] = prod[kk];
        __syncthreads();
        {
          // thread (slot = tid & 31, segment = tid >> 5): rows 32 seg .. 32 seg + 31 of that slot
          const int sl = tid & 31, seg = tid >> 5;
          double fv[32];   // all reads first: the compiler otherwise keeps only ~3 in flight
#pragma unroll
          for (int q = 0; q < 32; ++q) fv[q] = fold[sl][seg * 32 + q];
          __builtin_amdgcn_sched_barrier(0);
          double acc = 0.0;
#pragma unroll
          for (int q = 0; q < 32; ++q) acc += fv[q];
          // 8 segments per slot: pairs of segments live in the same wave
          acc += __shfl_xor(acc, 32, 64);
          if ((lane & 32) == 0) part[wave][h * (B / 2) + sl] = acc;
        }
        __syncthreads();
      }
    }
    if (tid < B) {
      const double bs = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
      bsum[tid] = bs;
      rb_send(boxes + (int64_t)blk * (2 * B), tid, bs, key);
    }
    __syncthreads();
    // ---- exchange: everybody ends up with the sums of everybody's partials, formed in the same order.
    // Up to PQ_FLAT workgroups: all-to-all. Above: two levels -- the first workgroup of every group of
    // PQ_GS collects its group (level 1) and publishes the group sums, everybody collects the group
    // sums (level 2): 8 + np/9 boxes to read instead of np, at the price of a second hop
    // (measured flat: 1.3 us at np < 10, 2.4 us at 20-29, 5.4 us at 40-49, 8.6 us at 70-79 per step).
    {
      // Messages are polled in parallel: every pass re-requests all word pairs of the chunk that
      // have not validated yet (waiting for them one after the other would add their latencies).
      // Sums boxes first .. first + count - 1 of `bx` (this thread: column cc, every 4th box from gg).
      auto gather = [&](const double* bx, int first, int count, unsigned long long k, int own,
                        double ownval) -> double {
        double acc = 0.0;
        for (int i0 = gg; i0 < count; i0 += 32) {
          double val[8];
          unsigned pend = 0;
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int i = i0 + 4 * u;
            val[u] = 0.0;
            if (i < count) {
              if (first + i == own) val[u] = ownval;
              else pend |= 1u << u;
            }
          }
          long spins = 0;
          while (pend) {
            unsigned long long wa[8], wb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              wa[u] = 0; wb[u] = 1;
              if (pend & (1u << u)) {
                const unsigned long long* w =
                    (const unsigned long long*)(bx + (int64_t)(first + i0 + 4 * u) * (2 * B)) + 2 * cc;
                wa[u] = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                wb[u] = __hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
              if ((pend & (1u << u)) && (wa[u] ^ wb[u]) == k) {
                val[u] = __longlong_as_double((long long)wa[u]);
                pend &= ~(1u << u);
              }
            if (pend && (++spins & 255) == 0 &&
                (spins > BC_SPIN_LIMIT || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
              __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              s_fail = 1;
              break;
            }
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) acc += val[u];    // fixed order: first + i0, + 4, ...
        }
        return acc;
      };
      if (np <= PQ_FLAT) {
        grp[gg][cc] = gather(boxes, 0, np, key, blk, bsum[cc]);
      } else {
        const int gid = blk / PQ_GS, g0 = gid * PQ_GS, ngr = (np + PQ_GS - 1) / PQ_GS;
        const bool leader = (blk == g0);                                          // uniform
        const unsigned long long key2 = rb_key(seq_base + j + (1 << 24));         // never a level-1 key
        double* boxes2 = mail2 + (int64_t)(j & 1) * ngr * (2 * B);
        if (leader) {
          grp[gg][cc] = gather(boxes, g0, min(PQ_GS, np - g0), key, blk, bsum[cc]);
          __syncthreads();
          if (tid < B) {
            const double gs = (grp[0][tid] + grp[1][tid]) + (grp[2][tid] + grp[3][tid]);
            bsum2[tid] = gs;
            rb_send(boxes2 + (int64_t)gid * (2 * B), tid, gs, key2);
          }
          __syncthreads();
        }
        grp[gg][cc] = gather(boxes2, 0, ngr, key2, leader ? gid : -1, leader ? bsum2[cc] : 0.0);
      }
    }
    __syncthreads();
    if (s_fail) return;   // uniform
    // ---- Householder scalars and w: every WAVE forms them for itself (lane = column), identically,
    //      so that no barrier and no LDS array stand between them and the update; w_c then comes by
    //      readlane from the lane that holds it. (Row j of the private top block is what the waves
    //      read here; the update below leaves it alone -- nobody reads it after this step.)
    double swl, sc;
    {
      const double ss = (grp[0][j] + grp[1][j]) + (grp[2][j] + grp[3][j]);
      const double dc = (grp[0][lane] + grp[1][lane]) + (grp[2][lane] + grp[3][lane]);
      const double alpha = top[j][j];
      double beta, tt;
      if (ss == 0.0) { beta = alpha; tt = 0.0; sc = 0.0; }
      else {
        beta = -copysign(hh_norm(alpha, ss), alpha);
        tt = (beta - alpha) / beta;
        sc = 1.0 / (alpha - beta);
      }
      const double tjc = top[j][lane];
      swl = (lane > j) ? tt * (tjc + sc * (dc - alpha * tjc)) : 0.0;
      if (tid == 0) {
        sbeta[j] = beta;
        sscale[j] = sc;
        if (blk == 0) { taus[j] = tt; scales[j] = sc; }
      }
    }
    // ---- rank-1 update of the rows in registers and of the private top block ------------------------
    {
      const double v = (r == j) ? 1.0 : ((r > j) ? x * sc : 0.0);
      if (j < B / 2 - 1) {   // w_c = 0 for c <= j: the first half is skipped once j >= 31 (uniform)
#pragma unroll
        for (int c = 0; c < B / 2; ++c) p[c] -= v * lane_value(swl, c);
      }
#pragma unroll
      for (int c = B / 2; c < B; ++c) p[c] -= v * lane_value(swl, c);
      const int rr = tid & 63;
      const int cq = __builtin_amdgcn_readfirstlane(tid >> 6);
      const double vt = (rr > j) ? top[rr][j] * sc : 0.0;
      double tv[16];                     // all loads first: the compiler must not serialise them behind the stores
      // unconditional within a half: vt = 0 for rows <= j and w_c = 0 for columns <= j, so those
      // entries are rewritten with their own value (a benign race with the waves still reading row j
      // above); columns 0..31 (q < 8) are all <= j once j >= 31 and are skipped then (uniform)
      if (j < B / 2 - 1) {
#pragma unroll
        for (int q = 0; q < 8; ++q) tv[q] = top[rr][cq + 4 * q];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int c = cq + 4 * q;
          top[rr][c] = tv[q] - vt * lane_value(swl, c);
        }
      }
#pragma unroll
      for (int q = 8; q < 16; ++q) tv[q] = top[rr][cq + 4 * q];
#pragma unroll
      for (int q = 8; q < 16; ++q) {
        const int c = cq + 4 * q;
        top[rr][c] = tv[q] - vt * lane_value(swl, c);
      }
      double xn = 0.0;
      switch (j + 1) {   // j is wave-uniform: a jump instead of a 64-deep select chain
        case 0: xn = p[0]; break;
        case 1: xn = p[1]; break;
        case 2: xn = p[2]; break;
        case 3: xn = p[3]; break;
        case 4: xn = p[4]; break;
        case 5: xn = p[5]; break;
        case 6: xn = p[6]; break;
        case 7: xn = p[7]; break;
        case 8: xn = p[8]; break;
        case 9: xn = p[9]; break;
        case 10: xn = p[10]; break;
        case 11: xn = p[11]; break;
        case 12: xn = p[12]; break;
        case 13: xn = p[13]; break;
        case 14: xn = p[14]; break;
        case 15: xn = p[15]; break;
        case 16: xn = p[16]; break;
        case 17: xn = p[17]; break;
        case 18: xn = p[18]; break;
        case 19: xn = p[19]; break;
        case 20: xn = p[20]; break;
        case 21: xn = p[21]; break;
        case 22: xn = p[22]; break;
        case 23: xn = p[23]; break;
        case 24: xn = p[24]; break;
        case 25: xn = p[25]; break;
        case 26: xn = p[26]; break;
        case 27: xn = p[27]; break;
        case 28: xn = p[28]; break;
        case 29: xn = p[29]; break;
        case 30: xn = p[30]; break;
        case 31: xn = p[31]; break;
        case 32: xn = p[32]; break;
        case 33: xn = p[33]; break;
        case 34: xn = p[34]; break;
        case 35: xn = p[35]; break;
        case 36: xn = p[36]; break;
        case 37: xn = p[37]; break;
        case 38: xn = p[38]; break;
        case 39: xn = p[39]; break;
        case 40: xn = p[40]; break;
        case 41: xn = p[41]; break;
        case 42: xn = p[42]; break;
        case 43: xn = p[43]; break;
        case 44: xn = p[44]; break;
        case 45: xn = p[45]; break;
        case 46: xn = p[46]; break;
        case 47: xn = p[47]; break;
        case 48: xn = p[48]; break;
        case 49: xn = p[49]; break;
        case 50: xn = p[50]; break;
        case 51: xn = p[51]; break;
        case 52: xn = p[52]; break;
        case 53: xn = p[53]; break;
        case 54: xn = p[54]; break;
        case 55: xn = p[55]; break;
        case 56: xn = p[56]; break;
        case 57: xn = p[57]; break;
        case 58: xn = p[58]; break;
        case 59: xn = p[59]; break;
        case 60: xn = p[60]; break;
        case 61: xn = p[61]; break;
        case 62: xn = p[62]; break;
        case 63: xn = p[63]; break;
        default: break;
      }
      x = xn;
    }
    __syncthreads();
  }
  // ---- write back: R on/above the diagonal (beta on it), unscaled reflector columns below, and
  //      the explicit unit-lower-trapezoidal V of the block reflector -------------------------------
  if (blk == 0 && tid >= ncolq && tid < B) { taus[tid] = 0.0; scales[tid] = 0.0; }
  if (valid) {
#pragma unroll
    for (int c = 0; c < B; ++c) {
      const double val = p[c];
      P[r + (int64_t)c * ld] = (r == c && c < ncolq) ? sbeta[c] : val;
      Vp[r + (int64_t)c * m] = (r < c) ? 0.0 : ((r == c) ? 1.0 : val * sscale[c]);
    }
  }
}

// ---------------------------------------------------------------------------
// Panel factorisation by CholeskyQR2 + Householder reconstruction: TWO all-reduces of a 64 x 64 Gram matrix and one
// broadcast of a 64 x 64 block per panel instead of 64 dependent exchanges (pq_resident). The panels of the trailing
// matrix are well conditioned after the first one (kappa 2 ... 60 measured on kernel matrices, 1e2 ... 1e5 for the
// first panel), so P = Q R with R = R2 R1 from two Cholesky passes gives Q orthonormal to rounding; the Householder
// form the rest of stage 1 works with is then reconstructed from Q (Ballard, Demmel, Grigori, Jacquelin, Knight,
// Nguyen: "Reconstructing Householder vectors from TSQR", 2014):
//     Q1 - S = L U  (LU without pivoting, S_i = -sign of the current diagonal entry, subtracted before step i),
//     V = [L; Q2 U^-1],  tau_i = -U_ii S_i = 1 + |a_ii|,  R_householder = S R.
// Thread t of workgroup k owns row 256k + t of the panel: in registers where it is worked on (Gram products on the
// MFMA units, the three triangular substitutions), parked in Vp across the exchanges and factorisations; every
// workgroup factorises the same 64 x 64 matrices itself (bit-identical everywhere: each Gram entry is summed by ONE
// workgroup over the partials in a fixed order and then read by everybody). A Cholesky pivot that is not positive, a
// diagonal ratio below PQC_RATIO or a second-pass Gram matrix far from I make every workgroup leave the panel
// untouched and raise *fallback: the launch of pq_resident that follows does the panel then (and returns at once
// otherwise).
// The big product A22 V that follows a factorisation on the critical path of stage 1 does not need the reconstruction:
// W = Q - [S; 0] = [L U; Q2] = V U gives A22 V T = (A22 W)(U^-1 T). So the kernel is split (pq_chol<true>, the HEAD: the
// two CholeskyQR passes, W left for the product; pq_tail, the TAIL: V, R, tau, T and U^-1 T beside that product);
// pq_chol<false> is the one-kernel form (BIGKRLS_PQ=fused).
// ---------------------------------------------------------------------------
// (the schedule's thresholds S1_AGG_MIN_M, S1_SWAP_M, S1_QUAD_MIN_M: csrc/s1sched.h)
static_assert(S1_B == S2_B, "the schedule's panel width is the band width");
constexpr int PQC_LD = 66;             // LDS row stride of the 64 x 64 matrices and of the staged rows
constexpr double PQC_RATIO = 1e-5;      // min / max diagonal of the first Cholesky factor below which the panel is left
                                        // to the Householder kernel (kappa^2 eps must stay far below 1)
// ... and the largest entry of E = Q1'Q1 - I after the first pass from which it is left to that kernel as well. The diagonal
// of a Cholesky factor does not show its condition number (Kahan's matrix: diagonal >= 0.004, condition 1e12): a first
// factor of a numerically singular Gram matrix that happens to go through passes the ratio, and the second factor of
// the Q1 it gives (condition 30 ... 2000 measured) has its diagonal in [0.65, 1] -- the panel then came back with
// |H'H - I| up to 1e-9 (tests/test_gpu_panel_routes.py). |E|_2 <= 64 max |E| < 1/2 bounds the singular values of Q1 to
// (0.70, 1.23): its condition number is below sqrt(3) and the second pass leaves Q orthonormal to rounding. Kernel
// matrices are far inside (max |E| ~ kappa^2 eps: 1e-6 at kappa = 1e5); panels up to kappa ~ 2e7 still pass.
constexpr double PQC_E2MAX = 0x1p-7;
#ifndef PQC_PARK
#define PQC_PARK 1
#endif
static_assert(PQC_MAXWG == 80 && PQC_NG == S2_B * S2_B, "pq_chol: at most 80 workgroups, 64 x 64 Gram entries (csrc/s2plan.h)");
constexpr size_t PQC_SMEM = (size_t)(3 * S2_B * PQC_LD + 64) * sizeof(double);   // dynamic LDS of pq_chol (sA, sM)

// development builds (tools/pqc_bench.sh): -DPQC_STOP=n compiles the kernel up to phase n only (a build per phase: a
// run-time phase argument changed the register allocation of the whole kernel and made it spill), -DBK_PQC_PROF adds
// the entry point bk_pqc_bench that launches the kernel on a random panel
#ifndef PQC_STOP
#define PQC_STOP 0
#endif
#define PQC_PHASE(n) if ((n) == PQC_STOP) return;
#define PQC_PROF_ARG
#define PQC_PROF_VAL(x)

// poll `cnt` (<= NMAX) self-validating word pairs base[idx[u]] in parallel; false after the watchdog fired
template <int NMAX>
__device__ __forceinline__ bool pqc_poll(const double* base, const int (&idx)[NMAX], int cnt, unsigned long long key,
                                         int* err, double (&out)[NMAX]) {
  unsigned pend = 0;
#pragma unroll
  for (int u = 0; u < NMAX; ++u) {
    out[u] = 0.0;
    if (u < cnt) pend |= 1u << u;
  }
  long spins = 0;
  while (pend) {
    unsigned long long wa[NMAX], wb[NMAX];
#pragma unroll
    for (int u = 0; u < NMAX; ++u) {
      wa[u] = 0; wb[u] = 1;
      if (pend & (1u << u)) {
        const unsigned long long* w = (const unsigned long long*)base + 2 * (int64_t)idx[u];
        wa[u] = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        wb[u] = __hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
#pragma unroll
    for (int u = 0; u < NMAX; ++u)
      if ((pend & (1u << u)) && (wa[u] ^ wb[u]) == key) {
        out[u] = __longlong_as_double((long long)wa[u]);
        pend &= ~(1u << u);
      }
    if (pend && (++spins & 255) == 0 &&
        (spins > BC_SPIN_LIMIT || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
      __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
  }
  return true;
}

// 1/sqrt(x) and 1/x for the pivots of the 64 x 64 factorisations (on their critical path: one or two per step): the
// hardware seed (~2^-26) and two Newton steps instead of the library routines' full special-case handling; x is a
// positive, normal number here (checked before) / |x| >= 1
__device__ __forceinline__ double pqc_rsqrt(double x) {
  double y = __builtin_amdgcn_rsq(x);
  const double hx = 0.5 * x;
  y = y * (1.5 - hx * y * y);
  y = y * (1.5 - hx * y * y);
  return y;
}
__device__ __forceinline__ double pqc_rcp(double x) {
  double y = __builtin_amdgcn_rcp(x);
  y = y * (2.0 - x * y);
  y = y * (2.0 - x * y);
  return y;
}

// The substitution x N = p with N upper triangular 64 x 64 in LDS (rows contiguous, stride PQC_LD) and one row of P per
// thread in registers: x_k = p_k inv[k], p_c -= x_k N[k][c] for c > k. Written as a LOOP over the eight blocks of eight
// unknowns whose body always works on p[0..7] (the current block) and p[8..63] (what is still to be updated), the
// array being rotated by eight places after every block: the 2 016-term form unrolled over static register indices is
// ~25 KB of straight-line code, and beside a trailing update that saturates the memory system every instruction-cache
// miss of it costs microseconds (measured: 1.6 ms for one substitution at m = 20 000 against 4 us alone).
__device__ __forceinline__ void pqc_solve(double (&p)[S2_B], const double* __restrict__ N, const double* __restrict__ inv) {
  constexpr int LD = PQC_LD;
#pragma unroll 1
  for (int cb = 0; cb < 8; ++cb) {
    const double* Nb = N + cb * (8 * LD + 8);     // N[8 cb][8 cb]
    const double* ib = inv + 8 * cb;
    // the 8 x 8 triangle of the current block
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double x = p[u] * ib[u];
      p[u] = x;
#pragma unroll
      for (int v = u + 1; v < 8; ++v) p[v] -= x * Nb[u * LD + v];
    }
    // its eight unknowns into the blocks behind it (block b of the rotated array is columns 8 (cb + b) ...)
#pragma unroll
    for (int b = 1; b < 8; ++b) {
      if (b < 8 - cb) {                            // uniform
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          double nv[8];
#pragma unroll
          for (int v = 0; v < 8; ++v) nv[v] = Nb[u * LD + 8 * b + v];
#pragma unroll
          for (int v = 0; v < 8; ++v) p[8 * b + v] -= p[u] * nv[v];
          if (u & 1) __builtin_amdgcn_sched_barrier(0);   // (the loads of at most two rows in flight: left alone the
                                                          //  compiler hoists all of them and runs out of registers)
        }
      }
    }
    // rotate: the solved block goes to the end, the next one to the front (after eight blocks: the original order)
    double t[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) t[v] = p[v];
#pragma unroll
    for (int c = 0; c < S2_B - 8; ++c) p[c] = p[c + 8];
#pragma unroll
    for (int v = 0; v < 8; ++v) p[S2_B - 8 + v] = t[v];
  }
}

// 16-byte write-through stores and L1-bypassing loads for data handed to other workgroups behind a flag (every byte
// stored sc1, the storing waves drained with s_waitcnt vmcnt(0) before the workgroup barrier that precedes the flag
// store; every load sc1, issued after the flag has been seen and a workgroup barrier)
typedef double bk_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void pqc_st16(double* q, double a, double b) {
  const bk_d2 v = {a, b};
  // (the s_nop: a store of more than 8 bytes followed by a write of its data registers needs wait states the compiler
  //  inserts for its own instructions but cannot for this one -- without them the next store's data, moved into the
  //  same registers, corrupts this one)
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 2" ::"v"(q), "v"(v) : "memory");
}
__device__ __forceinline__ void pqc_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// eight 16-byte loads in flight and the wait for them, as ONE statement: between separate statements the compiler,
// which does not know that the destination registers are still in flight, may copy or spill them
__device__ __forceinline__ void pqc_ld16x8(const double* const (&q)[8], double (&out)[16]) {
  bk_d2 v0, v1, v2, v3, v4, v5, v6, v7;
  asm volatile(
      "global_load_dwordx4 %0, %8, off sc1\n\t"
      "global_load_dwordx4 %1, %9, off sc1\n\t"
      "global_load_dwordx4 %2, %10, off sc1\n\t"
      "global_load_dwordx4 %3, %11, off sc1\n\t"
      "global_load_dwordx4 %4, %12, off sc1\n\t"
      "global_load_dwordx4 %5, %13, off sc1\n\t"
      "global_load_dwordx4 %6, %14, off sc1\n\t"
      "global_load_dwordx4 %7, %15, off sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3), "=&v"(v4), "=&v"(v5), "=&v"(v6), "=&v"(v7)
      : "v"(q[0]), "v"(q[1]), "v"(q[2]), "v"(q[3]), "v"(q[4]), "v"(q[5]), "v"(q[6]), "v"(q[7])
      : "memory");
  out[0] = v0.x; out[1] = v0.y; out[2] = v1.x; out[3] = v1.y; out[4] = v2.x; out[5] = v2.y; out[6] = v3.x; out[7] = v3.y;
  out[8] = v4.x; out[9] = v4.y; out[10] = v5.x; out[11] = v5.y; out[12] = v6.x; out[13] = v6.y; out[14] = v7.x; out[15] = v7.y;
}
__device__ __forceinline__ void pqc_ld16x4(const double* const (&q)[4], double (&out)[8]) {
  bk_d2 v0, v1, v2, v3;
  asm volatile(
      "global_load_dwordx4 %0, %4, off sc1\n\t"
      "global_load_dwordx4 %1, %5, off sc1\n\t"
      "global_load_dwordx4 %2, %6, off sc1\n\t"
      "global_load_dwordx4 %3, %7, off sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
      : "v"(q[0]), "v"(q[1]), "v"(q[2]), "v"(q[3])
      : "memory");
  out[0] = v0.x; out[1] = v0.y; out[2] = v1.x; out[3] = v1.y; out[4] = v2.x; out[5] = v2.y; out[6] = v3.x; out[7] = v3.y;
}
// wait until flag[i] >= seq for i < n (thread i polls flag i; n <= 256); false after the watchdog fired
__device__ __forceinline__ bool pqc_wait_flags(const unsigned long long* flag, int n, unsigned long long seq, int* err) {
  if ((int)threadIdx.x < n) {
    long spins = 0;
    while (__hip_atomic_load(flag + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < seq) {   // (flags only grow)
      if ((++spins & 255) == 0 &&
          (spins > BC_SPIN_LIMIT || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
        __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return false;
      }
    }
  }
  return true;
}

#ifndef PQC_FENCES
#define PQC_FENCES 3
#endif
#define PQC_RELEASE() do { if (PQC_FENCES & 1) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); pqc_drain(); } } while (0)
#define PQC_ACQUIRE() do { if ((PQC_FENCES & 2) && threadIdx.x == 0) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); pqc_drain(); } } while (0)

// (layout of the pq_chol mailbox, PQC_OFF_* and PQC_MAIL_DOUBLES: csrc/s2plan.h)

// The T factor of the block reflector from the reconstruction itself: with Q1 - S = L U and V1 = L one has
// (I - V T V')[I; 0] = Q S  <=>  Q1 S - I = -L T L'  <=>  T = -U S L^-T (same paper). Row i of X = T solves X L' = -U S on
// its own: x_c = -U_ic S_c - sum_{k < c} x_k L_ck, so the 64 rows go to 64 groups of four lanes (16 rows per wave), lane q
// of a group keeping the x_k with k = q (mod 4) and the group's partial sums folded by two quad exchanges per column
// (~2 us for one workgroup). FOLD: also the right-hand side -S instead of -U S, which gives U^-1 T = -S L^-T: the factor
// that takes Y2 = A22 W, W = V U = Q - [S; 0], to Y = A22 V T (the split factorisation, pq_tail) -- the same recurrence,
// its loads of L shared, its chains independent of the first one's. LU: L \ U in LDS (row stride PQC_LD). Both are
// written column-major with the zeros below the diagonal, the layout bt_build_t writes.
template <bool WITH_T, bool FOLD>
__device__ __forceinline__ void pqc_t_factor(const double* __restrict__ LU, const double* __restrict__ sS,
                                             double* __restrict__ Tout, double* __restrict__ Tfold) {
  constexpr int B = S2_B, LD = PQC_LD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ti = 16 * wave + (lane >> 2), q = lane & 3;
  const double* Lq = LU + q;                 // L[c][4 j + q] = Lq[c * LD + 4 j]
  const double* Ui = LU + ti * LD;           // U[ti][c], c >= ti
  double x[B / 4], xf[B / 4];
#pragma unroll
  for (int j = 0; j < B / 4; ++j) { x[j] = 0.0; xf[j] = 0.0; }
#pragma unroll
  for (int c = 0; c < B; ++c) {
    double a4[4] = {0.0, 0.0, 0.0, 0.0};     // (four chains: sixteen dependent multiply-adds per column cost ~6 us in all)
    double f4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < B / 4; ++j) {
      if (4 * j < c) {                                             // (static)
        const double l = Lq[c * LD + 4 * j];
        const double lm = (4 * j + q < c) ? l : 0.0;               // entries k >= c of row c hold U, not L
        if (WITH_T) a4[j & 3] = fma(x[j], lm, a4[j & 3]);
        if (FOLD) f4[j & 3] = fma(xf[j], lm, f4[j & 3]);
      }
    }
    if (WITH_T) {
      double acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
      acc += dpp_move<0xB1>(acc);              // lane ^ 1
      acc += dpp_move<0x4E>(acc);              // lane ^ 2
      const double bic = (c >= ti) ? -Ui[c] * sS[c] : 0.0;
      const double xc = bic - acc;
      if (q == (c & 3)) {
        x[c >> 2] = xc;
        Tout[ti + B * c] = xc;
      }
    }
    if (FOLD) {
      double acc = (f4[0] + f4[1]) + (f4[2] + f4[3]);
      acc += dpp_move<0xB1>(acc);
      acc += dpp_move<0x4E>(acc);
      const double xc = ((c == ti) ? -sS[c] : 0.0) - acc;
      if (q == (c & 3)) {
        xf[c >> 2] = xc;
        Tfold[ti + B * c] = xc;
      }
    }
  }
}

// (launch bounds of TWO workgroups per CU and the LDS arrays as dynamic shared memory, whose size the compiler does
//  not know: 256 registers per lane, vector and accumulation registers together -- with
//  more (the compiler parks values in accumulation registers when it may use 512) a workgroup no longer fits beside a
//  wave of the trailing update and starts only when a CU has emptied completely: the kernel then lasts as long as the update)
// SPLIT: the HEAD of the split factorisation -- the two CholeskyQR passes only. Each thread leaves its row of Q in Vp (here:
// the buffer the big product A22 (.) reads), workgroup 0 factorises its own top block Q1 - S = L U behind its row stores
// (no broadcast, nobody waits for it), subtracts S from the diagonal of the top block -- Vp then holds W = Q - [S; 0] =
// V U -- and publishes L \ U, S and 1 / diag(U); the last workgroup publishes R2 R1. pq_tail does the rest beside A22 W.
template <bool SPLIT>
__global__ __launch_bounds__(256, 2) void pq_chol(double* __restrict__ P, int64_t ld, int m,
                                                  double* __restrict__ taus, double* __restrict__ scales,
                                                  double* __restrict__ Vp, double* __restrict__ mail,
                                                  int seq_base, int* __restrict__ err, int* __restrict__ fallback,
                                                  double* __restrict__ Tout
                                                  PQC_PROF_ARG) {
  constexpr int B = S2_B, LD = PQC_LD;
  extern __shared__ __attribute__((aligned(16))) double pqc_smem[];
  double* sA = pqc_smem;                      // [B * LD + 64] staged rows / reduction scratch (np * chunk <= 4096 + 2 np values) / Q1 -> L \ U
  double (*sM)[B * LD] = (double (*)[B * LD])(pqc_smem + B * LD + 64);   // [2]: Gram matrix -> L (lower) and R = L' (upper) of pass 0, 1
  // (LDS budget: the kernel must fit beside ONE workgroup of the trailing update, 160 KB - 54 KB, like pq_resident:
  //  with more it waits for both update workgroups of a CU to end and starts late on the critical path)
  __shared__ double sInv[B], sS[B], sLU[2][4][B];   // sLU: columns / rows of the current factorisation step
  __shared__ int s_bad, s_fail;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = blockIdx.x, np = gridDim.x;
  const int r = blk * 256 + tid;
  const bool valid = r < m;
  double* boxes = mail;
  double* slices = mail + PQC_OFF_SLICES;
  double* qtop = mail + PQC_OFF_QTOP;
  unsigned long long* fbox = (unsigned long long*)(mail + PQC_OFF_FLAGS);
  unsigned long long* fslice = fbox + PQC_MAXWG;
  unsigned long long* fq = fslice + PQC_MAXWG;
  // every workgroup counts itself as resident: the trailing update that runs beside this kernel is launched behind a
  // gate kernel that waits for the count (s1_gate)
  if (tid == 0) atomicAdd((unsigned long long*)(mail + PQC_OFF_SLICES + PQC_NG + 48), 1ull);
  double p[B];
  {
    unsigned offp = valid ? (unsigned)r * 8u : 0u;
    const unsigned pstride = (unsigned)ld * 8u;
#pragma unroll
    for (int c = 0; c < B; ++c) { const double v = *(const double*)((const char*)P + offp); p[c] = valid ? v : 0.0; offp += pstride; }
    // (the head: the selected values made opaque -- otherwise the compiler keeps the loaded ones as well, for the stores
    //  of park() under `valid`, and the two copies of the row do not fit into 256 registers)
    if constexpr (SPLIT) {
#pragma unroll
      for (int c = 0; c < B; ++c) asm volatile("" : "+v"(p[c]));
    }
  }
  if (tid == 0) { s_bad = 0; s_fail = 0; }
  const int bi = tid >> 4, bj = tid & 15;          // this thread's 4 x 4 block of a 64 x 64 matrix
  const int chunk = 2 * ((PQC_NG / 2 + np - 1) / np);   // Gram entries summed by one workgroup (even: 16-byte loads)
  const int e0 = blk * chunk, e1 = min(PQC_NG, e0 + chunk), len = max(e1 - e0, 0);
  __syncthreads();
  PQC_PHASE(1)

  // this thread's 4 x 4 block of a 64 x 64 matrix in global memory (row-major, 64 doubles per row) <-> registers
  auto store_block = [&](double* dst, const double (&v)[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      double* q = dst + (4 * bi + a) * B + 4 * bj;
      pqc_st16(q, v[a][0], v[a][1]);
      pqc_st16(q + 2, v[a][2], v[a][3]);
    }
  };
  auto load_block_to_lds = [&](const double* src, double* dst) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {               // two rows of the block at a time (register pressure)
      const double* q[4];
#pragma unroll
      for (int a = 0; a < 2; ++a) { q[2 * a] = src + (4 * bi + 2 * h + a) * B + 4 * bj; q[2 * a + 1] = q[2 * a] + 2; }
      double v[8];
      pqc_ld16x4(q, v);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b2 = 0; b2 < 4; ++b2) dst[(4 * bi + 2 * h + a) * LD + 4 * bj + b2] = v[4 * a + b2];
    }
  };

  // The row lives in registers only where it is worked on (Gram products, substitution): across the exchanges and the
  // 64 x 64 factorisations it is parked in Vp (this thread's own row; L2-resident at most panel heights) -- with the row
  // AND the factorisations' blocks live the kernel needs more than 256 registers per lane, and with more than 256 it
  // cannot start beside a wave of the trailing update (see the launch bounds)
  // (32-bit offsets from a uniform base, made opaque at each use: otherwise the compiler forms the 64 column pointers
  //  of every pass over the row once, at the top of the kernel, and keeps -- i.e. spills -- them)
  const unsigned cstride = (unsigned)m * 8u;
  auto park = [&]() {
    unsigned off = (unsigned)r * 8u;
    asm volatile("" : "+v"(off));
    if (valid) {
#pragma unroll
      for (int c = 0; c < B; ++c) { *(double*)((char*)Vp + off) = p[c]; off += cstride; }
    }
  };
  auto unpark = [&]() {
    unsigned off = valid ? (unsigned)r * 8u : 0u;
    asm volatile("" : "+v"(off));
#pragma unroll
    for (int c = 0; c < B; ++c) { const double v = *(const double*)((const char*)Vp + off); p[c] = valid ? v : 0.0; off += cstride; }
  };

  // ---- Q1 - S = L U, right-looking, by the whole workgroup (4 x 4 blocks in registers as in the Cholesky passes; the
  //      current column and row go through LDS); S in sS, the reciprocal pivots in sInv (visible after a barrier) ------
  auto lu_q1 = [&](double (&blkv)[4][4]) {
    // two columns and rows (j, j + 1) per step and barrier
    for (int jb = 0; jb < B / 4; ++jb) {
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        const int jj = 2 * jp, j = 4 * jb + jj;
        double* cb0 = sLU[(jb * 2 + jp) & 1][0];
        double* cb1 = sLU[(jb * 2 + jp) & 1][1];
        double* rb0 = sLU[(jb * 2 + jp) & 1][2];
        double* rb1 = sLU[(jb * 2 + jp) & 1][3];
        if (bj == jb) {
#pragma unroll
          for (int a = 0; a < 4; ++a) { cb0[4 * bi + a] = blkv[a][jj]; cb1[4 * bi + a] = blkv[a][jj + 1]; }
        }
        if (bi == jb) {
#pragma unroll
          for (int b2 = 0; b2 < 4; ++b2) { rb0[4 * bj + b2] = blkv[jj][b2]; rb1[4 * bj + b2] = blkv[jj + 1][b2]; }
        }
        __syncthreads();
        const double a00 = cb0[j];
        const double s0 = (a00 >= 0.0) ? -1.0 : 1.0;
        const double p0 = a00 - s0, p0inv = pqc_rcp(p0);         // |p0| = 1 + |a00|
        const double l10 = cb0[j + 1] * p0inv, u01 = rb0[j + 1];
        const double a11 = cb1[j + 1] - l10 * u01;
        const double s1 = (a11 >= 0.0) ? -1.0 : 1.0;
        const double p1 = a11 - s1, p1inv = pqc_rcp(p1);
        double li0[4], li1[4], uc0[4], uc1[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int i = 4 * bi + a, c = 4 * bj + a;
          const double r0 = cb0[i], r1 = cb1[i], q0 = rb0[c], q1 = rb1[c];
          const double t0 = r0 * p0inv;
          const double t1 = (r1 - t0 * u01) * p1inv, u1 = q1 - l10 * q0;
          li0[a] = (i > j) ? t0 : 0.0;
          li1[a] = (i > j + 1) ? t1 : 0.0;
          uc0[a] = (c > j) ? q0 : 0.0;
          uc1[a] = (c > j + 1) ? u1 : 0.0;
        }
        const bool ocol = (bj == jb);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int i = 4 * bi + a;
#pragma unroll
          for (int b2 = 0; b2 < 4; ++b2) {
            double v = blkv[a][b2] - (li0[a] * uc0[b2] + li1[a] * uc1[b2]);
            if (b2 == jj) v = (ocol && i > j) ? li0[a] : ((ocol && i == j) ? p0 : v);
            if (b2 == jj + 1) v = (ocol && i > j + 1) ? li1[a] : ((ocol && i == j + 1) ? p1 : v);
            blkv[a][b2] = v;
          }
        }
        if (tid == 0) { sS[j] = s0; sS[j + 1] = s1; sInv[j] = p0inv; sInv[j + 1] = p1inv; }
      }
    }
    __syncthreads();
  };
  // ---- R2 R1 on and above the diagonal: thread (bi, bj), bi <= bj, forms its 4 x 4 block from the upper triangles of
  //      sM[1] (R2) and sM[0] (R1) --------------------------------------------------------------------------------------
  auto r_product = [&](double (&rr)[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b2 = 0; b2 < 4; ++b2) rr[a][b2] = 0.0;
    for (int kb = bi; kb <= bj; ++kb) {       // 4 x 4 blocks of R2 (rows of this thread) and R1 (its columns)
      double x2[4][4], x1[4][4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          x2[a][u] = sM[1][(4 * bi + a) * LD + 4 * kb + u];      // R2[i][k]
          x1[u][a] = sM[0][(4 * kb + u) * LD + 4 * bj + a];      // R1[k][c]
        }
      if (kb == bi) {                         // below the diagonal of R2 the array holds L2
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (u < a) x2[a][u] = 0.0;
      }
      if (kb == bj) {                         // ... and below that of R1, L1
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int a = 0; a < 4; ++a)
            if (u > a) x1[u][a] = 0.0;
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b2 = 0; b2 < 4; ++b2)
#pragma unroll
          for (int u = 0; u < 4; ++u) rr[a][b2] += x2[a][u] * x1[u][b2];
    }
  };

  // stage 0, 1: the two CholeskyQR passes (p <- p R^-1); stage 2: the Householder reconstruction (p <- (p - S e_r) U^-1).
  // Each ends in the same substitution over the rows in registers with an upper triangular 64 x 64 factor in LDS
  // (sInv[c]: reciprocal of its diagonal).
#pragma unroll
  for (int stage = 0; stage < (SPLIT ? 2 : 3); ++stage) {
    double* M = sM[stage & 1];
    if (stage < 2) {
      // ---- partial Gram matrix of this workgroup's rows on the f64 MFMA units: 64 rows staged in LDS at a time; wave w
      //      owns the tile row 16 w .. 16 w + 15 of the 64 x 64 result (four 16 x 16 tiles, one A fragment for all four) --
      typedef double pqc_d4 __attribute__((ext_vector_type(4)));
      pqc_d4 gacc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) gacc[t] = (pqc_d4){0.0, 0.0, 0.0, 0.0};
      const int lm = lane & 15, lk = lane >> 4;
      for (int h = 0; h < 4; ++h) {
        if (wave == h) {
#pragma unroll
          for (int c = 0; c < B; ++c) sA[lane * LD + c] = p[c];
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < 64; kk += 4) {
          const double* rowp = sA + (kk + lk) * LD + lm;      // row kk + lk of the staged block, column lm of a tile
          const double ya = rowp[16 * wave];
          double xb[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) xb[t] = rowp[16 * t];
#pragma unroll
          for (int t = 0; t < 4; ++t) gacc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[t], ya, gacc[t], 0, 0, 0);
        }
        __syncthreads();
      }
      // lane (lm, lk) holds G[16 wave + lm][16 t + lk + 4 q]: through LDS (sA is free again) into the 4 x 4 blocks the
      // exchange and the factorisation work with
      {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int q = 0; q < 4; ++q) sA[(16 * wave + lm) * LD + 16 * t + lk + 4 * q] = gacc[t][q];
      }
      __syncthreads();
      double acc[4][4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b2 = 0; b2 < 4; ++b2) acc[a][b2] = sA[(4 * bi + a) * LD + 4 * bj + b2];
      __syncthreads();
      PQC_PHASE(2 + 4 * stage)
      if (PQC_PARK) park();
      // ---- all-reduce: (1) everybody publishes its partial matrix; (2) workgroup w sums entries [e0, e1) over the
      //      workgroups, in their order, and publishes the sums; (3) everybody reads all the sums ------------------
      const unsigned long long seq = (unsigned long long)(seq_base + 4 * stage);
      store_block(boxes + (int64_t)blk * PQC_NG, acc);
      pqc_drain();
      __syncthreads();
      if (tid == 0) { PQC_RELEASE(); __hip_atomic_store(fbox + blk, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
      if (!pqc_wait_flags(fbox, np, seq, err)) s_fail = 1;
      PQC_ACQUIRE();
      __syncthreads();
      if (s_fail) return;   // uniform
      {
        const int half = len >> 1, total = np * half;           // 16-byte pairs to fetch
        for (int base = 0; base < total; base += 256 * 4) {
          const double* q[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int id = min(base + tid + 256 * u, total - 1);   // (clamped: a valid address, the value is dropped)
            q[u] = boxes + (int64_t)(id / half) * PQC_NG + e0 + 2 * (id % half);
          }
          double v[8];
          pqc_ld16x4(q, v);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int id = base + tid + 256 * u;
            if (id < total) {
              sA[(id / half) * len + 2 * (id % half)] = v[2 * u];
              sA[(id / half) * len + 2 * (id % half) + 1] = v[2 * u + 1];
            }
          }
        }
      }
      __syncthreads();
      for (int t = tid; t < len; t += 256) {      // (len > 256 when fewer than 16 workgroups share the matrix)
        double sum = 0.0;
        for (int i = 0; i < np; ++i) sum += sA[i * len + t];
        __hip_atomic_store((unsigned long long*)(slices + e0 + t), (unsigned long long)__double_as_longlong(sum),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      pqc_drain();
      __syncthreads();
      const unsigned long long seq2 = seq + 1;
      if (tid == 0) { PQC_RELEASE(); __hip_atomic_store(fslice + blk, seq2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
      if (!pqc_wait_flags(fslice, np, seq2, err)) s_fail = 1;
      PQC_ACQUIRE();
      __syncthreads();
      if (s_fail) return;   // uniform
      load_block_to_lds(slices, M);
      __syncthreads();
      PQC_PHASE(3 + 4 * stage)
      // ---- Cholesky G = L L', right-looking, by the whole workgroup: thread (bi, bj) keeps its 4 x 4 block in
      //      registers; per step the current column goes through LDS (two buffers: one barrier per step). L ends up in
      //      the lower triangle of M, R = L' in the upper one (rows contiguous: what the substitution reads) -----------
      {
        double blkv[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b2 = 0; b2 < 4; ++b2) blkv[a][b2] = M[(4 * bi + a) * LD + 4 * bj + b2];
        double dmin = 1e300, dmax = 0.0;
        int bad = 0;
        // Second pass on a well-conditioned panel: G = I + E with max |E| < 1e-8 (E ~ kappa^2 eps), and the Cholesky
        // factor of I + E is I + triu(E, 1) + diag(E) / 2 up to O(E^2) < 1e-16: no factorisation steps at all
        int nsteps = B / 4;
        bool far = false;                       // second pass: max |E| >= PQC_E2MAX (uniform)
        if (stage == 1) {
          double emax = 0.0;
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b2 = 0; b2 < 4; ++b2) emax = fmax(emax, fabs(blkv[a][b2] - ((bi == bj && a == b2) ? 1.0 : 0.0)));
          // (2: factorise; 3: too far from I for this method -- the largest wins; a NaN lands at 3)
          if (!(emax < 1e-8)) atomicMax(&s_bad, (emax < PQC_E2MAX) ? 2 : 3);
          __syncthreads();
          const bool near_identity = (s_bad == 0);
          far = (s_bad == 3);
          __syncthreads();
          if (tid == 0) s_bad = 0;
          if (near_identity) {
            nsteps = 0;
            dmin = dmax = 1.0;
            if (bi == bj) {
#pragma unroll
              for (int a = 0; a < 4; ++a) {
                const double d = 1.0 + 0.5 * (blkv[a][a] - 1.0);
                blkv[a][a] = d;
                sInv[4 * bi + a] = 1.0 / d;
              }
            }
          }
        }
        // two columns (j, j + 1) per step and barrier: the 2 x 2 pivot block is factorised by every thread itself
        for (int jb = 0; jb < nsteps; ++jb) {
#pragma unroll
          for (int jp = 0; jp < 2; ++jp) {
            const int jj = 2 * jp, j = 4 * jb + jj;
            double* cb0 = sLU[(jb * 2 + jp) & 1][0];
            double* cb1 = sLU[(jb * 2 + jp) & 1][1];
            if (bj == jb) {
#pragma unroll
              for (int a = 0; a < 4; ++a) { cb0[4 * bi + a] = blkv[a][jj]; cb1[4 * bi + a] = blkv[a][jj + 1]; }
            }
            __syncthreads();
            const double a00 = cb0[j], a10 = cb0[j + 1], a11 = cb1[j + 1];
            if (!(a00 > 0.0) || !(a00 < 1e300)) bad = 1;      // uniform (also across the workgroups)
            const double d0inv = bad ? 1.0 : pqc_rsqrt(a00), d0 = a00 * d0inv;
            const double l10 = a10 * d0inv;
            const double a11u = a11 - l10 * l10;
            if (!(a11u > 0.0) || !(a11u < 1e300)) bad = 1;
            const double d1inv = bad ? 1.0 : pqc_rsqrt(a11u), d1 = a11u * d1inv;
            dmin = fmin(dmin, fmin(d0, d1));
            dmax = fmax(dmax, fmax(d0, d1));
            // (loads and arithmetic unconditional, selects last: a load inside a conditional becomes a branch)
            double li0[4], li1[4], lc0[4], lc1[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
              const int i = 4 * bi + a, c = 4 * bj + a;
              const double r0 = cb0[i], r1 = cb1[i], q0 = cb0[c], q1 = cb1[c];
              const double t0 = r0 * d0inv, u0 = q0 * d0inv;
              const double t1 = (r1 - t0 * l10) * d1inv, u1 = (q1 - u0 * l10) * d1inv;
              li0[a] = (i > j) ? t0 : 0.0;
              li1[a] = (i > j + 1) ? t1 : 0.0;
              lc0[a] = (c > j) ? u0 : 0.0;
              lc1[a] = (c > j + 1) ? u1 : 0.0;
            }
            const bool ocol = (bj == jb), orow = (bi == jb);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
              const int i = 4 * bi + a;
#pragma unroll
              for (int b2 = 0; b2 < 4; ++b2) {
                const int c = 4 * bj + b2;
                double v = blkv[a][b2] - (li0[a] * lc0[b2] + li1[a] * lc1[b2]);
                // columns j, j + 1 of L (with R[j][j+1] = l10 above the diagonal) and rows j, j + 1 of R = L'
                if (b2 == jj) v = (ocol && i > j) ? li0[a] : ((ocol && i == j) ? d0 : v);
                if (b2 == jj + 1) v = (ocol && i > j + 1) ? li1[a] : ((ocol && i == j + 1) ? d1 : ((ocol && i == j) ? l10 : v));
                if (a == jj) v = (orow && c > j + 1) ? lc0[b2] : v;
                if (a == jj + 1) v = (orow && c > j + 1) ? lc1[b2] : v;
                blkv[a][b2] = v;
              }
            }
            if (tid == 0) { sInv[j] = d0inv; sInv[j + 1] = d1inv; }
          }
        }
        // the first factor decides whether the panel is safe for this method; the second Gram matrix must be near I
        if (!bad && stage == 0 && dmin < PQC_RATIO * dmax) bad = 1;
        if (!bad && stage == 1 && (far || dmin < 0.5 || dmax > 2.0)) bad = 1;
        if (tid == 0) s_bad = bad;
        if (tid == 0 && blk == 0) {     // (diagnostics of the decision, read by the host in debug mode)
          double* dbg = mail + PQC_OFF_SLICES + PQC_NG + 8 * stage;
          dbg[0] = (double)bad; dbg[1] = dmin; dbg[2] = dmax;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b2 = 0; b2 < 4; ++b2) M[(4 * bi + a) * LD + 4 * bj + b2] = blkv[a][b2];
      }
      __syncthreads();
      if (s_bad) {            // uniform, and the same in every workgroup
        if (blk == 0 && tid == 0) {
          *fallback = 1;
          mail[PQC_OFF_SLICES + PQC_NG + 32] += 1.0;     // panels left to pq_resident in this decomposition (BIGKRLS_VERBOSE)
        }
        return;
      }
      PQC_PHASE(4 + 4 * stage)
      if (PQC_PARK) unpark();
    } else {
      // ---- the top 64 x 64 block of Q to everybody: rows 0..63 are the first wave of workgroup 0 -------------------
      const unsigned long long seq = (unsigned long long)(seq_base + 2);
      if (blk == 0) {
        if (wave == 0) {
#pragma unroll
          for (int c = 0; c < B; ++c) sA[lane * LD + c] = p[c];
        }
        __syncthreads();
        double v[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b2 = 0; b2 < 4; ++b2) v[a][b2] = sA[(4 * bi + a) * LD + 4 * bj + b2];
        store_block(qtop, v);
        pqc_drain();
        __syncthreads();
        if (tid == 0) { PQC_RELEASE(); __hip_atomic_store(fq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
      }
      if (PQC_PARK) park();
      if (!pqc_wait_flags(fq, 1, seq, err)) s_fail = 1;
      PQC_ACQUIRE();
      __syncthreads();
      if (s_fail) return;   // uniform
      load_block_to_lds(qtop, sA);
      __syncthreads();
      PQC_PHASE(10)
      // ---- Q1 - S = L U; L and U back in place ----------------------------------------------------------------------
      {
        double blkv[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b2 = 0; b2 < 4; ++b2) blkv[a][b2] = sA[(4 * bi + a) * LD + 4 * bj + b2];
        lu_q1(blkv);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b2 = 0; b2 < 4; ++b2) sA[(4 * bi + a) * LD + 4 * bj + b2] = blkv[a][b2];
      }
      __syncthreads();
      PQC_PHASE(11)
      // R = S (R2 R1) on and above the diagonal of the top block (workgroup 0 holds those rows)
      if (blk == 0 && bi <= bj) {
        double rr[4][4];
        r_product(rr);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b2 = 0; b2 < 4; ++b2) {
            const int i = 4 * bi + a, c = 4 * bj + b2;
            if (i <= c && i < m) P[i + (int64_t)c * ld] = sS[i] * rr[a][b2];
          }
      }
      if (PQC_PARK) unpark();
#pragma unroll
      for (int c = 0; c < B; ++c)
        if (r == c) p[c] -= sS[c];
      PQC_PHASE(12)
    }
    // ---- the substitution over the rows in registers: p <- p N^-1, N = R (upper triangle of M) or U (of sA) ------------
    pqc_solve(p, stage < 2 ? M : sA, sInv);
    __syncthreads();
    PQC_PHASE(5 + 4 * stage)
  }
  if constexpr (SPLIT) {
    // ---- the head's results: Q, then (workgroup 0, behind its row stores) the top block's factors and the patch Q1 - S --
    // (the row leaves the registers first: beside it the products and the factorisation below would spill)
    park();
    if (blk == 0 && wave == 0) {
#pragma unroll
      for (int c = 0; c < B; ++c) sA[lane * LD + c] = p[c];
    }
    if (blk == np - 1 && bi <= bj) {
      double rr[4][4];
      r_product(rr);
      double* rprod = mail + PQC_OFF_RPROD;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b2 = 0; b2 < 4; ++b2) {
          const int i = 4 * bi + a, c = 4 * bj + b2;
          if (i <= c) rprod[i * B + c] = rr[a][b2];
        }
    }
    PQC_PHASE(10)
    if (blk != 0) return;
    __syncthreads();
    const double qd = sA[lane * (LD + 1)];     // Q1_ii for thread i < 64
    double blkv[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b2 = 0; b2 < 4; ++b2) blkv[a][b2] = sA[(4 * bi + a) * LD + 4 * bj + b2];
    lu_q1(blkv);
    store_block(qtop, blkv);
    if (tid < B) {
      double* sinv = mail + PQC_OFF_SINV;
      sinv[tid] = sS[tid];
      sinv[B + tid] = sInv[tid];
      Vp[tid + (int64_t)tid * m] = qd - sS[tid];      // (m >= 64: this thread's own row, behind its own store of Q1_ii)
    }
    if (tid == 0) *fallback = 0;
    return;
  }
  // ---- results --------------------------------------------------------------------------------------------------------
  if (blk == 0 && tid == 0) *fallback = 0;
  if (blk == 0 && tid < B) {
    taus[tid] = -sA[tid * LD + tid] * sS[tid];
    scales[tid] = 1.0;
  }
  if (valid) {
    unsigned off = (unsigned)r * 8u, offp = (unsigned)r * 8u;
    asm volatile("" : "+v"(off), "+v"(offp));
    const unsigned pstride = (unsigned)ld * 8u;
#pragma unroll
    for (int c = 0; c < B; ++c) {
      const double v = (r < c) ? 0.0 : ((r == c) ? 1.0 : p[c]);
      *(double*)((char*)Vp + off) = v;
      if (r > c) *(double*)((char*)P + offp) = p[c];
      off += cstride;
      offp += pstride;
    }
  }
  // ---- the T factor of the block reflector, H_1 ... H_64 = I - V T V', from the reconstruction itself (pqc_t_factor):
  //      ~2 us in workgroup 0 behind its stores, instead of the chain V'V (split-K GEMM) -> slab reduction -> dlarft
  //      recurrence behind the kernel (69 us at m = 2 500, on the critical path of every panel below m ~ 6 000). A panel
  //      left to the Householder kernel (s_bad above: this point is not reached) gets its T from that chain, which
  //      Stage1::build_T launches behind a device-side predicate.
  if (Tout != nullptr && blk == 0) pqc_t_factor<true, false>(sA, sS, Tout, nullptr);
}

// ---------------------------------------------------------------------------
// The TAIL of the split factorisation: the Householder reconstruction from what pq_chol<true> left -- W = Q - [S; 0] in
// Vw, L \ U, S, 1 / diag(U) and R2 R1 in the mailbox. A plain kernel with no waits between workgroups, launched behind
// the head (and the Householder kernel's slot) while A22 W runs. Workgroup k < gridDim.x - 1: thread t solves its row of
// V = W U^-1 (the top block comes out as L) and stores it to V and, below the diagonal, into the panel. The LAST
// workgroup, beside them: R = S (R2 R1), tau, T = -U S L^-T (write_T) and Tfold = U^-1 T = -S L^-T, which takes A22 W to
// Y = A22 V T (s1_fused_yt). A panel the head left to the Householder kernel (*fallback != 0) has its V in Vw already:
// copied to V, and T -- built by the chain Stage1::build_T launches in front of this kernel -- to Tfold.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pq_tail(double* __restrict__ P, int64_t ld, int m, double* __restrict__ taus,
                                               double* __restrict__ scales, const double* __restrict__ Vw,
                                               double* __restrict__ V, const double* __restrict__ mail,
                                               const int* __restrict__ fallback, double* __restrict__ T, int write_T,
                                               double* __restrict__ Tfold) {
  constexpr int B = S2_B, LD = PQC_LD;
  __shared__ double sU[B * LD];
  __shared__ double sInv[B], sS[B];
  const int tid = threadIdx.x, blk = blockIdx.x;
  const bool rows = blk < (int)gridDim.x - 1;
  const int r = blk * 256 + tid;
  const bool valid = rows && r < m;
  const unsigned cstride = (unsigned)m * 8u;
  if (*fallback != 0) {     // uniform, and the same in every workgroup
    if (valid) {
      unsigned off = (unsigned)r * 8u;
#pragma unroll 8
      for (int c = 0; c < B; ++c) { *(double*)((char*)V + off) = *(const double*)((const char*)Vw + off); off += cstride; }
    }
    if (!rows && write_T)
      for (int e = tid; e < PQC_NG; e += 256) Tfold[e] = T[e];
    return;
  }
  const double* lu = mail + PQC_OFF_QTOP;
#pragma unroll
  for (int u = 0; u < PQC_NG / 256; ++u) {
    const int e = tid + 256 * u;
    sU[(e >> 6) * LD + (e & 63)] = lu[e];
  }
  if (tid < B) { sS[tid] = mail[PQC_OFF_SINV + tid]; sInv[tid] = mail[PQC_OFF_SINV + B + tid]; }
  if (rows) {
    double p[B];
    {
      unsigned off = valid ? (unsigned)r * 8u : 0u;
#pragma unroll
      for (int c = 0; c < B; ++c) { const double v = *(const double*)((const char*)Vw + off); p[c] = valid ? v : 0.0; off += cstride; }
    }
    __syncthreads();
    pqc_solve(p, sU, sInv);
    if (valid) {
      unsigned off = (unsigned)r * 8u, offp = (unsigned)r * 8u;
      asm volatile("" : "+v"(off), "+v"(offp));
      const unsigned pstride = (unsigned)ld * 8u;
#pragma unroll
      for (int c = 0; c < B; ++c) {
        const double v = (r < c) ? 0.0 : ((r == c) ? 1.0 : p[c]);
        *(double*)((char*)V + off) = v;
        if (r > c) *(double*)((char*)P + offp) = p[c];
        off += cstride;
        offp += pstride;
      }
    }
    return;
  }
  __syncthreads();
  if (tid < B) {
    taus[tid] = -sU[tid * LD + tid] * sS[tid];
    scales[tid] = 1.0;
  }
  {
    const double* rprod = mail + PQC_OFF_RPROD;
#pragma unroll
    for (int u = 0; u < PQC_NG / 256; ++u) {
      const int e = tid + 256 * u, i = e >> 6, c = e & 63;     // (consecutive threads: consecutive entries of a row of R2 R1)
      if (i <= c && i < m) P[i + (int64_t)c * ld] = sS[i] * rprod[e];
    }
  }
  if (write_T) pqc_t_factor<true, true>(sU, sS, T, Tfold);
  else pqc_t_factor<false, true>(sU, sS, nullptr, Tfold);
}

// Tfold = T for a panel the split factorisation left to the Householder kernel (V is then the operand of A22 (.) itself)
__global__ void pq_tfold_copy(const double* __restrict__ T, double* __restrict__ Tfold, const int* __restrict__ run_if) {
  if (*run_if == 0) return;
  for (int e = threadIdx.x; e < S2_B * S2_B; e += blockDim.x) Tfold[e] = T[e];
}

#ifdef BK_PQC_PROF
// development build only (tools/pqc_bench.sh): the panel factorisation on a random m x 64 panel, `reps` launches; returns
// the mean launch time in microseconds. `which` = 0: the head of the split factorisation (pq_chol<true>; its phase is a
// compile-time choice, PQC_STOP), 1: the tail (pq_tail) behind one launch of the head, 2: the one-kernel form
__global__ void pqc_fill(double* p, int64_t n, unsigned seed) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    unsigned x = (unsigned)e * 2654435761u + seed; x ^= x >> 15; x *= 2246822519u; x ^= x >> 13;
    p[e] = (double)(x & 0xffff) / 65536.0 - 0.5;
  }
}
}  // anonymous namespace
}  // namespace bk
extern "C" __attribute__((visibility("default"))) int bk_pqc_bench(bigkrls_ctx* ctx, int m, int reps, int which,
                                                                   double* us, double* dbg_out) {
  using namespace bk;
  hipStream_t st = ctx->stream;
  hipFuncSetAttribute((const void*)pq_chol<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PQC_SMEM);
  hipFuncSetAttribute((const void*)pq_chol<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PQC_SMEM);
  double *P, *P0, *Vp, *Vw, *mail, *tau, *Tt;
  int* flags;
  hipMalloc(&P, (size_t)m * 64 * 8); hipMalloc(&P0, (size_t)m * 64 * 8); hipMalloc(&Vp, (size_t)m * 64 * 8);
  hipMalloc(&Vw, (size_t)m * 64 * 8); hipMalloc(&Tt, 2 * 4096 * 8);
  hipMalloc(&mail, PQC_MAIL_DOUBLES * 8); hipMalloc(&tau, 256 * 8); hipMalloc(&flags, 64);
  hipMemsetAsync(mail, 0, PQC_MAIL_DOUBLES * 8, st); hipMemsetAsync(flags, 0, 64, st);
  pqc_fill<<<512, 256, 0, st>>>(P0, (int64_t)m * 64, 7u);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  float total = 0.f;
  // BK_PQC_LOAD=1: a streaming copy on another stream beside every launch (memory contention like the trailing update's)
  // BK_PQC_LOAD=1: the trailing update of a matrix with m rows (syrk_mirror, k = 128, 128 x 64 tiles) launched on the
  // context's main stream just before every pq_chol launch on a high-priority stream -- the situation of the fit
  const bool load = getenv("BK_PQC_LOAD") != nullptr;
  double *L0 = nullptr, *L1 = nullptr;
  hipStream_t s2 = nullptr;
  if (load) {
    hipMalloc(&L0, (size_t)m * m * 8); hipMalloc(&L1, (size_t)m * 256 * 8);
    hipMemsetAsync(L0, 0, (size_t)m * m * 8, st); hipMemsetAsync(L1, 0, (size_t)m * 256 * 8, st);
    int lo = 0, hi = 0; hipDeviceGetStreamPriorityRange(&lo, &hi);
    hipStreamCreateWithPriority(&s2, hipStreamNonBlocking, hi);
    hipStreamSynchronize(st);
    st = s2;
  }
  for (int r = -1; r < reps; ++r) {
    hipMemcpyAsync(P, P0, (size_t)m * 64 * 8, hipMemcpyDeviceToDevice, st);
    hipStreamSynchronize(st);
    if (load) hipStreamSynchronize(ctx->stream);
    if (load) syrk_mirror(ctx, m, 128, -1.0, L1, m, L1 + (size_t)m * 128, m, L0, m, 0, -1, true);
    if (which == 1)
      hipLaunchKernelGGL(pq_chol<true>, dim3((m + 255) / 256), dim3(256), PQC_SMEM, st, P, (int64_t)m, m, tau, tau + 64, Vw,
                         mail, (r + 2) * 8 + 1, flags, flags + 4, (double*)nullptr);
    hipEventRecord(e0, st);
    if (which == 0)
      hipLaunchKernelGGL(pq_chol<true>, dim3((m + 255) / 256), dim3(256), PQC_SMEM, st, P, (int64_t)m, m, tau, tau + 64, Vw,
                         mail, (r + 2) * 8 + 1, flags, flags + 4, (double*)nullptr);
    else if (which == 1)
      hipLaunchKernelGGL(pq_tail, dim3((m + 255) / 256 + 1), dim3(256), 0, st, P, (int64_t)m, m, tau, tau + 64, (const double*)Vw,
                         Vp, (const double*)mail, (const int*)(flags + 4), Tt, 1, Tt + 4096);
    else
      hipLaunchKernelGGL(pq_chol<false>, dim3((m + 255) / 256), dim3(256), PQC_SMEM, st, P, (int64_t)m, m, tau, tau + 64, Vp,
                         mail, (r + 2) * 8 + 1, flags, flags + 4, (double*)nullptr);
    hipEventRecord(e1, st);
    hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    if (r >= 0) total += ms;
  }
  *us = 1e3 * total / reps;
  if (dbg_out) {
    hipMemcpy(dbg_out, Vp, (size_t)m * 64 * 8, hipMemcpyDeviceToHost);
    hipMemcpy(dbg_out + (size_t)m * 64, P, (size_t)m * 64 * 8, hipMemcpyDeviceToHost);
    hipMemcpy(dbg_out + (size_t)2 * m * 64, tau, 64 * 8, hipMemcpyDeviceToHost);
  }
  int h[8]; hipMemcpy(h, flags, 32, hipMemcpyDeviceToHost);
  if (load) { hipStreamSynchronize(ctx->stream); hipStreamSynchronize(s2); hipFree(L0); hipFree(L1); hipStreamDestroy(s2); }
  hipFree(P); hipFree(P0); hipFree(Vp); hipFree(Vw); hipFree(Tt); hipFree(mail); hipFree(tau); hipFree(flags);
  return h[0] * 100 + h[4];     // watchdog word, fallback word
}
namespace bk {
namespace {
#endif

// write the R factor of the panel (its strict upper triangle came through Rrow, its diagonal
// is beta) back into the panel's top block
__global__ void pq_fix_diag(double* __restrict__ P, int64_t ld, int ncol, int pw,
                            const double* __restrict__ betas, const double* __restrict__ Rrow) {
  for (int e = threadIdx.x; e < ncol * pw; e += blockDim.x) {
    const int j = e / pw, c = e % pw;
    if (c == j) P[j + (int64_t)j * ld] = betas[j];
    else if (c > j) P[j + (int64_t)c * ld] = Rrow[j * S2_B + c];
  }
}

// Vp (m x pw, ld m): explicit unit-lower-trapezoidal reflector block of a stage-1 panel
__global__ void s1_extract_v(const double* __restrict__ P, int64_t ld, int m, int pw,
                             const double* __restrict__ scales, double* __restrict__ Vp) {
  const int64_t total = (int64_t)m * pw;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(e % m), c = (int)(e / m);
    Vp[e] = (r < c) ? 0.0 : (r == c ? 1.0 : P[r + (int64_t)c * ld] * scales[c]);
  }
}

// PZ1 = [V | Z], PZ2 = [Z | V]  with Z = Y - 0.5 V S   (m x pw each, packed m x 2pw)
__global__ void s1_build_vz(const double* __restrict__ Vp, const double* __restrict__ Y,
                            const double* __restrict__ VS, int m, int pw, double* __restrict__ PZ1,
                            double* __restrict__ PZ2) {
  const int64_t total = (int64_t)m * pw;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = e / m, r = e % m;
    const double v = Vp[e];
    const double z = Y[e] - 0.5 * VS[e];
    PZ1[r + c * m] = v;
    PZ1[r + (pw + c) * m] = z;
    PZ2[r + c * m] = z;
    PZ2[r + (pw + c) * m] = v;
  }
}

// ---- the small products of a stage-1 panel, fused ----------------------------------------------
// After Y2 = A22 V the panel needs Y = Y2 T, S = T' (V'Y), Z = Y - 1/2 V S and the packed operands
// [V | Z], [Z | V] of the trailing update: five thin GEMMs (two of them split-K) and a packing pass,
// ~100 us of dependent launches per panel. Three kernels do the same on the MFMA units:
//   s1_fused_yt: Y = Y2 T and the partial products V_blk' Y_blk of 128-row blocks,
//   s1_fused_s : S = T' (sum of the partials)            (one workgroup per column of S),
//   s1_fused_z : Z = Y - 1/2 V S, written straight into [V | Z] and [Z | V].
typedef double s1_d4 __attribute__((ext_vector_type(4)));
constexpr int S1F_LD = S2_B + 2;   // LDS row stride 66 = 2 mod 32: conflict-free MFMA fragment reads
static_assert(S1F_CHUNKS == 2, "s1_fused_yt: two 64-row chunks per workgroup (csrc/s2plan.h sizes fpart by it)");

__global__ __launch_bounds__(256) void s1_fused_yt(const double* __restrict__ Y2, const double* __restrict__ T,
                                                   const double* __restrict__ Vp, int m,
                                                   double* __restrict__ Y, double* __restrict__ partial) {
  constexpr int B = S2_B, LD = S1F_LD;
  extern __shared__ __attribute__((aligned(16))) double s1f_smem[];
  double* sTt = s1f_smem;              // sTt[c * LD + k] = T[k][c]
  double* sY2 = s1f_smem + B * LD;     // sY2[r * LD + k]
  double* sV = s1f_smem + 2 * B * LD;  // sV[i * LD + r]
  double* sYo = s1f_smem + 3 * B * LD; // sYo[c * LD + r]
  const int tid = threadIdx.x, ln = tid & 63, wv = tid >> 6, l16 = ln & 15, lg = ln >> 4;
  {
    double tr[16];   // all loads, then all LDS stores (written as one loop the compiler waits for
                     // every load before its store: 16 dependent round trips)
#pragma unroll
    for (int q = 0; q < 16; ++q) tr[q] = T[ln + (wv + 4 * q) * B];
#pragma unroll
    for (int q = 0; q < 16; ++q) sTt[(wv + 4 * q) * LD + ln] = tr[q];
  }
  s1_d4 pacc[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) pacc[it] = (s1_d4){0.0, 0.0, 0.0, 0.0};
  const int rbase = blockIdx.x * (S1F_CHUNKS * B);
  for (int ch = 0; ch < S1F_CHUNKS; ++ch) {
    const int r0 = rbase + ch * B;
    if (r0 >= m) break;   // uniform
    const bool ok = r0 + ln < m;
    const int64_t rl = ok ? r0 + ln : m - 1;   // clamped, not predicated (see s1_fused_z); zeroed below
    double y2r[16], vr[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = wv + 4 * q;
      y2r[q] = Y2[rl + (int64_t)c * m];
      vr[q] = Vp[rl + (int64_t)c * m];
    }
    if (!ok) {   // rows past the end must not enter the partial V'Y sums
#pragma unroll
      for (int q = 0; q < 16; ++q) { y2r[q] = 0.0; vr[q] = 0.0; }
    }
    __syncthreads();   // the previous chunk's fragment reads are done (and sTt is in place)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = wv + 4 * q;
      sY2[ln * LD + c] = y2r[q];
      sV[c * LD + ln] = vr[q];
    }
    __syncthreads();
    // Y[r][c] = sum_k Y2[r][k] T[k][c]; this wave owns columns 16 wv .. 16 wv + 15
    s1_d4 yacc[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) yacc[rt] = (s1_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kb = 0; kb < B; kb += 8) {   // fragment reads of two k-steps, then their eight MFMAs
      double tk[2], xa[2][4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        tk[u] = sTt[(wv * 16 + l16) * LD + kb + 4 * u + lg];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) xa[u][rt] = sY2[(rt * 16 + l16) * LD + kb + 4 * u + lg];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
          yacc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[u][rt], tk[u], yacc[rt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) sYo[(wv * 16 + l16) * LD + rt * 16 + lg + 4 * q] = yacc[rt][q];
    __syncthreads();
    {
      double yo[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) yo[q] = sYo[(wv + 4 * q) * LD + ln];
      if (ok) {
#pragma unroll
        for (int q = 0; q < 16; ++q) Y[(int64_t)(r0 + ln) + (int64_t)(wv + 4 * q) * m] = yo[q];
      }
    }
    // P[i][c] += sum_r V[r][i] Y[r][c]
#pragma unroll
    for (int rb = 0; rb < B; rb += 8) {
      double yv[2], xv[2][4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        yv[u] = sYo[(wv * 16 + l16) * LD + rb + 4 * u + lg];
#pragma unroll
        for (int it = 0; it < 4; ++it) xv[u][it] = sV[(it * 16 + l16) * LD + rb + 4 * u + lg];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int it = 0; it < 4; ++it)
          pacc[it] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[u][it], yv[u], pacc[it], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  double* po = partial + (int64_t)blockIdx.x * (B * B);
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int q = 0; q < 4; ++q) po[(it * 16 + lg + 4 * q) + B * (wv * 16 + l16)] = pacc[it][q];
}

// S = T' S0, S0 = sum of the nblk partial V'Y blocks; workgroup c forms column c of S: four
// threads per entry of S0[:, c] sum interleaved quarters of the blocks (fixed order: deterministic)
__global__ __launch_bounds__(256) void s1_fused_s(const double* __restrict__ partial, int nblk,
                                                  const double* __restrict__ T, double* __restrict__ S) {
  constexpr int B = S2_B;
  __shared__ double sq[4][B];
  __shared__ double s0[B];
  const int k = threadIdx.x & 63, part = threadIdx.x >> 6, c = blockIdx.x;
  const double* pp = partial + k + B * c;
  double a0 = 0.0, a1 = 0.0;
  int blk = part;
  for (; blk + 28 < nblk; blk += 32) {   // eight loads in flight, two fixed-order running sums
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = pp[(int64_t)(blk + 4 * u) * (B * B)];
#pragma unroll
    for (int u = 0; u < 8; u += 2) { a0 += v[u]; a1 += v[u + 1]; }
  }
  for (; blk + 4 < nblk; blk += 8) {
    a0 += pp[(int64_t)blk * (B * B)];
    a1 += pp[(int64_t)(blk + 4) * (B * B)];
  }
  if (blk < nblk) a0 += pp[(int64_t)blk * (B * B)];
  sq[part][k] = a0 + a1;
  __syncthreads();
  if (part == 0) s0[k] = (sq[0][k] + sq[1][k]) + (sq[2][k] + sq[3][k]);
  __syncthreads();
  if (part == 0) {
    const double* tc = T + k * B;   // column i = k of T: T[kk][i]
    double acc = 0.0;
#pragma unroll 8
    for (int kk = 0; kk < B; ++kk) acc += tc[kk] * s0[kk];
    S[k + B * c] = acc;
  }
}

// Z = Y - 1/2 V S; PZ1 = [V | Z], PZ2 = [Z | V]  (m x 128 each, ld m); one workgroup per 64 rows.
// With A22 != nullptr the workgroup also applies the update A22 -= V Z' + Z V' to its rows of the
// NEXT PANEL's 64 columns (and to the mirrored 64 rows): it forms Z_top = Z(0:64, :) for itself
// (same 64^3 product on the top rows) and U = V_blk Z_top' + Z_blk V_top'. The look-ahead panel QR
// can then start right after this kernel instead of after a separate first-tile-column launch of
// the trailing update (~35 us of a nearly empty GPU per panel).
__global__ __launch_bounds__(256) void s1_fused_z(const double* __restrict__ Vp, const double* __restrict__ Y,
                                                  const double* __restrict__ S, int m,
                                                  double* __restrict__ PZ1, double* __restrict__ PZ2,
                                                  int64_t ldpz, double* __restrict__ A22, int64_t lda) {
  constexpr int B = S2_B, LD = S1F_LD;
  extern __shared__ __attribute__((aligned(16))) double s1f_smem[];
  double* bufA = s1f_smem;              // [r][k]: own V, later V_top
  double* bufS = s1f_smem + B * LD;     // [c][k] = S[k][c], later Z_top as [row][k]
  double* sO = s1f_smem + 2 * B * LD;   // [c][r] = (V S)[r][c]; later own V as [r][k]; later the new block [c][r]
  double* bufD = s1f_smem + 3 * B * LD; // [r][k]: own Z (panel update only)
  const int tid = threadIdx.x, ln = tid & 63, wv = tid >> 6, l16 = ln & 15, lg = ln >> 4;
  const int r0 = blockIdx.x * B;
  const bool ok = r0 + ln < m;
  // rows past the end read a clamped (valid) row instead of being predicated off: a predicated load
  // sits in its own basic block with a memory wait in front; every row only feeds its own outputs,
  // and those of the rows past the end are never stored
  const int64_t rl = ok ? r0 + ln : m - 1;
  double vr[16], sr[16];   // all global loads first, then the LDS stores
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int c = wv + 4 * q;
    vr[q] = Vp[rl + (int64_t)c * m];
    sr[q] = S[ln + c * B];
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    bufS[(wv + 4 * q) * LD + ln] = sr[q];
    bufA[ln * LD + wv + 4 * q] = vr[q];
  }
  __syncthreads();
  // (rows of bufA) x S -> sO[c][r]
  auto times_s = [&]() {
    s1_d4 acc[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[rt] = (s1_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kb = 0; kb < B; kb += 8) {
      double sk[2], xa[2][4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        sk[u] = bufS[(wv * 16 + l16) * LD + kb + 4 * u + lg];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) xa[u][rt] = bufA[(rt * 16 + l16) * LD + kb + 4 * u + lg];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
          acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[u][rt], sk[u], acc[rt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) sO[(wv * 16 + l16) * LD + rt * 16 + lg + 4 * q] = acc[rt][q];
  };
  times_s();
  __syncthreads();
  double zr[16];
  {
    const int64_t r = r0 + ln;
    double yr[16], orr[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      yr[q] = Y[rl + (int64_t)(wv + 4 * q) * m];
      orr[q] = sO[(wv + 4 * q) * LD + ln];
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) zr[q] = yr[q] - 0.5 * orr[q];
    if (ok) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int c = wv + 4 * q;
        PZ1[r + (int64_t)c * ldpz] = vr[q];
        PZ1[r + (int64_t)(B + c) * ldpz] = zr[q];
        PZ2[r + (int64_t)c * ldpz] = zr[q];
        PZ2[r + (int64_t)(B + c) * ldpz] = vr[q];
      }
    }
  }
  if (A22 == nullptr) return;   // uniform
  // ---- the next panel's columns: top rows of V and Z (m >= 64 here) -------------------------------
  double vt[16], yt[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    vt[q] = Vp[(int64_t)ln + (int64_t)(wv + 4 * q) * m];
    yt[q] = Y[(int64_t)ln + (int64_t)(wv + 4 * q) * m];
  }
  __syncthreads();                 // everybody is done with bufA (own V) and sO (V S)
#pragma unroll
  for (int q = 0; q < 16; ++q) bufA[ln * LD + wv + 4 * q] = vt[q];   // V_top as [row][k]
  __syncthreads();
  times_s();                       // V_top S -> sO[c][row]
  __syncthreads();
  {
    double ot[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) ot[q] = sO[(wv + 4 * q) * LD + ln];
    __syncthreads();               // sO and bufS (S) are free now
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = wv + 4 * q;
      bufS[ln * LD + c] = yt[q] - 0.5 * ot[q];   // Z_top as [row][k]
      bufD[ln * LD + c] = zr[q];                 // own Z as [r][k]
      sO[ln * LD + c] = vr[q];                   // own V as [r][k]
    }
  }
  __syncthreads();
  // U[r][c] = sum_k V[r][k] Z_top[c][k] + Z[r][k] V_top[c][k]; this wave: columns 16 wv .. 16 wv + 15
  s1_d4 u[4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) u[rt] = (s1_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const double* xs = pass == 0 ? sO : bufD;
    const double* ys = pass == 0 ? bufS : bufA;
#pragma unroll
    for (int kb = 0; kb < B; kb += 8) {
      double yk[2], xa[2][4];
#pragma unroll
      for (int uu = 0; uu < 2; ++uu) {
        yk[uu] = ys[(wv * 16 + l16) * LD + kb + 4 * uu + lg];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) xa[uu][rt] = xs[(rt * 16 + l16) * LD + kb + 4 * uu + lg];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int uu = 0; uu < 2; ++uu)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
          u[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[uu][rt], yk[uu], u[rt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // u[rt][q] = U[r = 16 rt + lg + 4 q][c = 16 wv + l16]
  const int c_mine = wv * 16 + l16;
  if (r0 > 0) {
    // mirrored block: rows 0..63 of A22, columns r0 + r (16 lanes = 16 consecutive rows c: 128-byte segments)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      double oldv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = r0 + rt * 16 + lg + 4 * q;
        oldv[q] = (r < m) ? A22[(int64_t)c_mine + (int64_t)r * lda] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = r0 + rt * 16 + lg + 4 * q;
        if (r < m) A22[(int64_t)c_mine + (int64_t)r * lda] = oldv[q] - u[rt][q];
      }
    }
  }
  __syncthreads();                 // the products are done: sO is free
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int q = 0; q < 4; ++q) sO[c_mine * LD + rt * 16 + lg + 4 * q] = u[rt][q];   // [c][r]
  __syncthreads();
  if (ok) {
    const int64_t r = r0 + ln;
    double oldv[16], un[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = wv + 4 * q;
      oldv[q] = A22[r + (int64_t)c * lda];
      un[q] = sO[c * LD + ln];
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = wv + 4 * q;
      const double v = oldv[q] - un[q];
      if (r0 > 0) {
        A22[r + (int64_t)c * lda] = v;
      } else if ((int)r >= c) {      // diagonal block: lower triangle computed, mirrored exactly
        A22[r + (int64_t)c * lda] = v;
        A22[(int64_t)c + r * lda] = v;
      }
    }
  }
}

// band array AB[d + c*S2_LD] = A[c+d, c] for 0 <= d <= b (rest zero)
__global__ void s1_extract_band(const double* __restrict__ W, int n, double* __restrict__ AB) {
  const int64_t total = (int64_t)n * S2_LD;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(e % S2_LD), c = (int)(e / S2_LD);
    AB[e] = (d <= S2_B && c + d < n) ? W[(int64_t)(c + d) + (int64_t)c * n] : 0.0;
  }
}

// Holds the stream until `want` workgroups of the panel factorisations launched so far have started (or 50 us have
// passed -- a bound, never a hang): the factorisation's workgroups (107 KB of LDS, 256 VGPRs) are then placed on empty
// CUs BEFORE the trailing update's fill the GPU. That is what makes THREE update workgroups per CU usable (round 6):
// three are 5-7 % faster than two in isolation, but a finished one leaves a 52-KB hole the factorisation does not fit
// into, so without the gate it started late on the critical path (+42 ms at C3, DEAD_ENDS.md); with it C3 goes
// 0.4087-0.4105 -> 0.4041-0.4048 s, same box (profiles/r06/r06b_gate_ab_C3.log). BIGKRLS_S1_GATE=0 launches no gate.
__global__ void s1_gate(const unsigned long long* __restrict__ cnt, unsigned long long want, long long max_ticks) {
  if (threadIdx.x == 0) {
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want &&
           (long long)(wall_clock64() - t0) < max_ticks)
      __builtin_amdgcn_s_sleep(1);
  }
}
struct Stage1Ws {
  double* Vp;     // m x b
  double* Vw = nullptr;     // m x b: W = V U = Q - [S; 0] of the split panel factorisation, the operand of A22 (.)
  double* Tfold = nullptr;  // b x b: U^-1 T of the current panel (Y = (A22 W) Tfold)
  double* Y;      // m x b
  double* Y2;     // m x b
  double* PZ1;    // m x 2b
  double* PZ2;    // m x 2b
  double* small;  // G, T, S, ... 8 b^2
  double* part;   // norm partials (2 x maxb) + dot partials
  double* Tall;   // per-panel T factors (b x b each), kept for the back-transform
  double* fpart;  // partial V'Y blocks of the fused small products: (n/128 + 2) x b x b
  double* mail;   // pq_resident mailboxes: 2 x (n/256 + 1) x 64 word pairs (zeroed per call)
  double* mail2;  // ... of the group sums of its two-level exchange: 2 x 16 x 64 word pairs
  double* pqc = nullptr;   // pq_chol mailboxes: PQC_MAXWG Gram matrices + the summed one + the top block of Q (word pairs)
  int* err;       // watchdog word shared with the bulge-chasing kernel
  int* fallback = nullptr; // raised by pq_chol for a panel it leaves to pq_resident
  // aggregated trailing update (two panels per pass over A22): reflector blocks [V Z V Z] / [Z V Z V]
  // of two panel groups (n x 256 each, leading dimension aggLd) and the small correction factors
  double* aggPZ1[2] = {nullptr, nullptr};
  double* aggPZ2[2] = {nullptr, nullptr};
  int64_t aggLd = 0;
  double* aggC = nullptr;   // 3 x (256 x 64)
};

// ctx->stream pointed at another stream for the host calls of one scope (gemm(), copy_matrix(), syrk_mirror() and the
// profile brackets launch on ctx->stream); restored on every exit
struct StreamScope {
  bigkrls_ctx* ctx;
  hipStream_t saved;
  StreamScope(bigkrls_ctx* c, hipStream_t s) : ctx(c), saved(c->stream) { c->stream = s; }
  ~StreamScope() { ctx->stream = saved; }
  StreamScope(const StreamScope&) = delete;
  StreamScope& operator=(const StreamScope&) = delete;
};

// Stage 1, full matrix to band. The per-panel operations (panel_qr, build_T, small_products*) are shared by the
// single-GPU loop and by the per-panel entry points of the row-block distributed reduction (bigkrls_dev_s1_*, eigen.hip);
// the single-GPU loop is stage1_to_band: one member per phase, the schedule by csrc/s1sched.h.
struct Stage1 {
  bigkrls_ctx* ctx = nullptr;
  double* W = nullptr;
  int n = 0;
  double* taus1 = nullptr;
  Stage1Ws ws{};
  int64_t N = 0;
  int maxb = 0, pq_cap = 1;
  bool pq_chol_on = true;
  // The split factorisation (default; BIGKRLS_PQ=fused: the one-kernel form): panel_qr launches the head (pq_chol<true>),
  // which leaves W = V U in ws.Vw -- all that A22 (.) needs -- and build_T the tail (pq_tail: V, R, tau, T, Tfold), which
  // then runs beside that product. Per panel: Vw(k) is the operand of A22 (.) and of the correction factors U'^T (.) that
  // act on its result, Tyt(k) the factor that takes the product to Y; everything else reads V and T.
  bool pq_split = true;
  bool pq_steps = false, fused_small = true, fused_panel = true;
  size_t yt_smem = 0, z_smem = 0;
  double *normA = nullptr, *normB = nullptr, *dotA = nullptr, *dotB = nullptr, *betas = nullptr, *Rrow = nullptr;
  double* xbuf[2] = {nullptr, nullptr};
  double *G = nullptr, *S0 = nullptr, *S = nullptr;
  unsigned long long pq_started = 0;   // workgroups of all pq_chol launches of this decomposition so far
  // T factors from pq_chol itself (BIGKRLS_S1_TPQ=0: always through the V'V chain, the cross-check): panel_qr records the
  // panel whose T the kernel writes; build_T for that panel then launches the chain behind a device-side predicate
  // (*ws.fallback != 0: the panel was left to the Householder kernel, which forms no T)
  bool t_in_pq = true;
  int t_from_pq_k = -1;
  S1Sched sched;                       // which arm takes which panel (init: n, residency, switches; begin_loop: the rest)
  // ---- state of the loop (run)
  hipStream_t st = nullptr, side = nullptr;   // main stream; look-ahead stream
  int k = 0, gq = 0, gi = 0;           // the panel whose step comes next; groups of four / of two done
  bool t_pending = false;              // ev_join2 (T and the correction factors of panel k, from the look-ahead stream) not waited for yet
  bool panel_in_z = false;             // s1_fused_z has updated the next panel's columns
  bool have_prev = false;              // piece b of the previous pair group is still to run
  int c1 = 0, c1_prev = 0, og = 0, og_prev = 0;   // first column of piece a / first row of the buffers of this / the previous pair group
  S1Counts done;                       // what went down each arm (BIGKRLS_VERBOSE)
  // on ctx->stream: wait until the panel factorisation enqueued last is resident (s1_gate)
  int gate() {
    static const bool on = [] { const char* e = getenv("BIGKRLS_S1_GATE"); return !(e && e[0] == '0'); }();
    if (on && ws.pqc != nullptr && pq_started > 0) {
      hipLaunchKernelGGL(s1_gate, dim3(1), dim3(64), 0, ctx->stream,
                         (const unsigned long long*)(ws.pqc + PQC_OFF_SLICES + PQC_NG + 48), pq_started, 5000LL);
      BK_CHECK_LAUNCH();
    }
    return BIGKRLS_OK;
  }

  int init(bigkrls_ctx* c, double* W_, int n_, double* taus1_, const Stage1Ws& ws_) {
    ctx = c; W = W_; n = n_; taus1 = taus1_; ws = ws_;
    N = n;
    const int b = S2_B;
    maxb = (n + 255) / 256 + 2;
    normA = ws.part;
    normB = normA + maxb;
    dotA = normB + maxb;
    dotB = dotA + (int64_t)maxb * S2_B;
    betas = dotB + (int64_t)maxb * S2_B;
    Rrow = betas + S2_B;
    xbuf[0] = Rrow + S2_B * S2_B;
    xbuf[1] = Rrow + S2_B * S2_B + n;
    G = ws.small;
    S0 = G + 2 * b * b;
    S = S0 + b * b;
    // Panel QR of block column k + the explicit reflector block Vp: one register-resident launch
    // (workgroups exchange partial sums through global mailboxes) when all its workgroups can be
    // co-resident, else one launch per column. BIGKRLS_PQ=steps forces the latter.
    BK_TRY(resident_capacity(ctx, (const void*)pq_resident, &pq_cap));
    BK_TRY(ensure_dyn_smem(ctx, (const void*)pq_chol<false>, PQC_SMEM));
    const char* pq_env = getenv("BIGKRLS_PQ");
    pq_steps = ctx->no_resident || (pq_env && std::string(pq_env) == "steps");
    // BIGKRLS_PQ=householder: the 64-exchange Householder kernel for every panel (cross-check of pq_chol)
    pq_chol_on = !(pq_env && std::string(pq_env) == "householder");
    pq_split = pq_chol_on && !pq_steps && ws.Vw != nullptr && ws.Tfold != nullptr && !(pq_env && std::string(pq_env) == "fused");
    BK_TRY(ensure_dyn_smem(ctx, (const void*)pq_chol<true>, PQC_SMEM));
    // BIGKRLS_S1=gemm: the panel's small products as separate GEMMs (cross-check of the fused kernels)
    const char* s1_env = getenv("BIGKRLS_S1");
    fused_small = !(s1_env && std::string(s1_env) == "gemm");
    yt_smem = (size_t)4 * S2_B * S1F_LD * sizeof(double);
    z_smem = (size_t)4 * S2_B * S1F_LD * sizeof(double);
    // BIGKRLS_S1=nopanel: fused small products, but the next panel's columns by a launch of the trailing update
    fused_panel = fused_small && !(s1_env && std::string(s1_env) == "nopanel");
    {
      const char* tpq = getenv("BIGKRLS_S1_TPQ");
      t_in_pq = !(tpq && tpq[0] == '0');
    }
    if (fused_small) {
      BK_TRY(ensure_dyn_smem(ctx, (const void*)s1_fused_yt, yt_smem));
      BK_TRY(ensure_dyn_smem(ctx, (const void*)s1_fused_z, z_smem));
    }
    sched = S1Sched();
    sched.n = n;
    sched.cap = pq_cap;
    sched.pq_steps = pq_steps;
    sched.fused_panel = fused_panel;
    sched.agg_ws = ws.aggPZ1[0] != nullptr;
    return BIGKRLS_OK;
  }

  bool resident_qr(int k) const { return sched.resident_qr(k); }
  bool has_panel(int k) const { return sched.has_panel(k); }
  double* Tof(int k) const { return ws.Tall + (int64_t)(k / S2_B) * S2_B * S2_B; }
  // the panels pq_chol takes: register-resident, at most PQC_MAXWG workgroups, at least 2 b rows
  bool chol_panel(int k) const {
    const int m = n - k - S2_B;
    return resident_qr(k) && pq_chol_on && ws.pqc != nullptr && (m + 255) / 256 <= PQC_MAXWG && m >= 2 * S2_B;
  }
  bool split_panel(int k) const { return pq_split && chol_panel(k); }
  double* Vw(int k) const { return split_panel(k) ? ws.Vw : ws.Vp; }
  const double* Tyt(int k) const { return split_panel(k) ? ws.Tfold : Tof(k); }

  int panel_qr(int k, hipStream_t ps) {
    const int b = S2_B;
    const int m = n - k - b;
    const int pw = b;
    t_from_pq_k = -1;
    double* P = W + (k + b) + (int64_t)k * N;
#ifdef BK_PQ_STUB
    if (getenv("BIGKRLS_PQ_STUB")) return pq_stub(k, ps);
#endif
    if (resident_qr(k)) {
      // algorithmic bytes: the m x 64 panel read and written once, the explicit V written once
      const bool samp = ctx->profile && (k / b) % S1_PROF_STRIDE == 0;
      if (samp) BK_TRY(prof_begin(ctx, "panel_qr", 24.0 * (double)m * pw, ps));
      const int npq = (m + 255) / 256;
      const bool chol = chol_panel(k), split = split_panel(k);
      static const int pqc_dbg = [] { const char* e = getenv("BIGKRLS_PQC_DEBUG"); return e ? atoi(e) : 0; }();   // (bits: pqc_debug)
      if (chol && (pqc_dbg & 1)) BK_HIP(hipDeviceSynchronize());     // debug: nothing runs beside the kernel
      if (chol) {
        if (split)
          hipLaunchKernelGGL(pq_chol<true>, dim3(npq), dim3(256), PQC_SMEM, ps, P, N, m, taus1 + k, taus1 + n + k, ws.Vw,
                             ws.pqc, (k / b) * 8 + 1, ws.err, ws.fallback, (double*)nullptr PQC_PROF_VAL(0));
        else
          hipLaunchKernelGGL(pq_chol<false>, dim3(npq), dim3(256), PQC_SMEM, ps, P, N, m, taus1 + k, taus1 + n + k, ws.Vp,
                             ws.pqc, (k / b) * 8 + 1, ws.err, ws.fallback, t_in_pq ? Tof(k) : (double*)nullptr PQC_PROF_VAL(0));
        pq_started += (unsigned long long)npq;
        t_from_pq_k = t_in_pq ? k : -1;
      }
      if (chol && (pqc_dbg & 6)) BK_TRY(pqc_debug(k, P, pqc_dbg));
      // (a split panel left to this kernel: its V goes where A22 (.) reads, pq_tail copies it to ws.Vp)
      hipLaunchKernelGGL(pq_resident, dim3(npq), dim3(256), 0, ps, P, N, m, taus1 + k,
                         taus1 + n + k, split ? ws.Vw : ws.Vp, ws.mail, ws.mail2, (k / b) * S2_B + 1, ws.err,
                         chol ? (const int*)ws.fallback : (const int*)nullptr);
      if (samp) BK_TRY(prof_end(ctx, "panel_qr", ps));
      BK_CHECK_LAUNCH();
      return BIGKRLS_OK;
    }
    const int ncolq = std::min(pw, m);
    int np = (m + 255) / 256;
    const int ncg0 = std::max(1, (pw - 1 + PQ_CG - 1) / PQ_CG);
    hipLaunchKernelGGL(pq_first, dim3(np, ncg0), dim3(256), 0, ps, (const double*)P, N, m, pw, normA, dotA);
    double *ncur = normA, *nnxt = normB, *dcur = dotA, *dnxt = dotB;
    for (int j = 0; j < ncolq; ++j) {
      const int nbu = (m - j + 255) / 256;
      const int ncg = std::max(1, (pw - j - 1 + PQ_CG - 1) / PQ_CG);
      const double* xcur = (j == 0) ? (const double*)P : (const double*)xbuf[j & 1];
      hipLaunchKernelGGL(pq_step, dim3(nbu, ncg), dim3(256), 0, ps, P, N, m, pw, j, (const double*)ncur,
                         (const double*)dcur, np, taus1 + k, taus1 + n + k, betas, Rrow, xcur,
                         j == 0 ? 0 : 1, xbuf[(j + 1) & 1], nnxt, dnxt);
      std::swap(ncur, nnxt);
      std::swap(dcur, dnxt);
      np = nbu;
    }
    hipLaunchKernelGGL(pq_fix_diag, dim3(1), dim3(256), 0, ps, P, N, ncolq, pw, (const double*)betas,
                       (const double*)Rrow);
    BK_CHECK_LAUNCH();
    if (ncolq < pw) {
      BK_HIP(hipMemsetAsync(taus1 + k + ncolq, 0, (pw - ncolq) * sizeof(double), ps));
      BK_HIP(hipMemsetAsync(taus1 + n + k + ncolq, 0, (pw - ncolq) * sizeof(double), ps));
    }
    const int blocks = (int)std::min<int64_t>(((int64_t)m * pw + 255) / 256, 4096);
    hipLaunchKernelGGL(s1_extract_v, dim3(blocks), dim3(256), 0, ps, (const double*)P, N, m, pw,
                       (const double*)(taus1 + n + k), ws.Vp);
    BK_CHECK_LAUNCH();
    return BIGKRLS_OK;
  }

  // T factor of the block reflector (G = V'V, forward dlarft recurrence) on the same stream as
  // the panel QR: with look-ahead it, too, hides behind the previous trailing update. gemm()
  // launches on ctx->stream, which is pointed at the panel's stream for the duration.
  int build_T(int k, hipStream_t ps) {
    const int b = S2_B;
    const int m = n - k - b;
    double* T = Tof(k);
    const bool split = split_panel(k);
    // pq_chol has written T itself unless it left the panel to the Householder kernel: the chain then runs behind the
    // device-side predicate *ws.fallback != 0 (three launches that return at once otherwise)
    const int* pred = (t_from_pq_k == k && ws.fallback != nullptr) ? (const int*)ws.fallback : (const int*)nullptr;
    // The tail of the split factorisation (V, R, tau, T and Tfold; for a panel that fell back the copies of V and T) goes
    // BEHIND the predicated chain, whose operand is then ws.Vw -- V itself whenever the chain does anything -- so that
    // nothing but the tail stands between the head and what waits for this stream; with BIGKRLS_S1_TPQ=0 the chain
    // always runs, on the tail's V, and Tfold = T is a launch of its own for a panel that fell back.
    auto tail = [&](bool write_T) {
      hipLaunchKernelGGL(pq_tail, dim3((m + 255) / 256 + 1), dim3(256), 0, ps, W + (k + b) + (int64_t)k * N, N, m, taus1 + k,
                         taus1 + n + k, (const double*)ws.Vw, ws.Vp, (const double*)ws.pqc, (const int*)ws.fallback, T,
                         write_T ? 1 : 0, ws.Tfold);
    };
    if (split && pred == nullptr) tail(false);
    const double* Vchain = (split && pred != nullptr) ? ws.Vw : ws.Vp;
    {
      StreamScope on(ctx, ps);
      ctx->gemm_run_if = pred;
      const int rc = gemm(ctx, 1, 0, b, b, m, 1.0, Vchain, m, Vchain, m, 0.0, G, b);
      ctx->gemm_run_if = nullptr;
      BK_TRY(rc);
    }
    hipLaunchKernelGGL(bt_build_t, dim3(1), dim3(256), 0, ps, (const double*)G, b, (const double*)(taus1 + k), T, pred);
    if (split && pred != nullptr) tail(true);
    else if (split)
      hipLaunchKernelGGL(pq_tfold_copy, dim3(1), dim3(256), 0, ps, (const double*)T, ws.Tfold, (const int*)ws.fallback);
    BK_CHECK_LAUNCH();
    return BIGKRLS_OK;
  }

  // The thin products between Y2 = A22 V and the trailing update, on ctx->stream:
  //   Y = Y2 T, S = T' V'Y, Z = Y - 1/2 V S, packed as PZ1 = [V | Z], PZ2 = [Z | V]  (m x 2b each).
  // Y2 is overwritten when the products run as separate GEMMs. With A22_panel != nullptr the fused
  // kernel also applies the update to the next panel's 64 columns (and mirrored rows) of A22.
  int small_products(int k, double* Y2, double* A22_panel) {
    return small_products_to(k, Y2, A22_panel, ws.PZ1, ws.PZ2, n - k - S2_B);
  }
  // ... with [V | Z] and [Z | V] written to pz1 / pz2 (leading dimension ldpz >= m)
  int small_products_to(int k, double* Y2, double* A22_panel, double* pz1, double* pz2, int64_t ldpz) {
    hipStream_t st = ctx->stream;
    const int b = S2_B, pw = S2_B;
    const int m = n - k - b;
    double* T = Tof(k);
    if (fused_small) {
      const int nblk = (m + S1F_CHUNKS * S2_B - 1) / (S1F_CHUNKS * S2_B);
      hipLaunchKernelGGL(s1_fused_yt, dim3(nblk), dim3(256), yt_smem, st, (const double*)Y2, Tyt(k),
                         (const double*)ws.Vp, m, ws.Y, ws.fpart);                   // Y = A22 V T, partial V'Y
      hipLaunchKernelGGL(s1_fused_s, dim3(pw), dim3(256), 0, st, (const double*)ws.fpart, nblk,
                         (const double*)T, S);                                       // S = T'V'Y
      hipLaunchKernelGGL(s1_fused_z, dim3((m + pw - 1) / pw), dim3(256), z_smem, st, (const double*)ws.Vp,
                         (const double*)ws.Y, (const double*)S, m, pz1, pz2, ldpz, A22_panel, N);   // [V | Z], [Z | V]
      BK_CHECK_LAUNCH();
    } else {
      BK_REQUIRE(pz1 == ws.PZ1 && ldpz == m, "stage 1: separate small products write the compact buffers only");
      const int blocks = (int)std::min<int64_t>(((int64_t)m * pw + 255) / 256, 4096);
      BK_TRY(gemm(ctx, 0, 0, m, pw, pw, 1.0, Y2, m, Tyt(k), pw, 0.0, ws.Y, m));            // Y = A22 V T
      BK_TRY(gemm(ctx, 1, 0, pw, pw, m, 1.0, ws.Vp, m, ws.Y, m, 0.0, S0, pw));        // V'Y
      BK_TRY(gemm(ctx, 1, 0, pw, pw, pw, 1.0, T, pw, S0, pw, 0.0, S, pw));            // S = T'V'Y
      BK_TRY(gemm(ctx, 0, 0, m, pw, pw, 1.0, ws.Vp, m, S, pw, 0.0, Y2, m));           // V S
      hipLaunchKernelGGL(s1_build_vz, dim3(blocks), dim3(256), 0, st, (const double*)ws.Vp,
                         (const double*)ws.Y, (const double*)Y2, m, pw, ws.PZ1, ws.PZ2);
      BK_CHECK_LAUNCH();
    }
    return BIGKRLS_OK;
  }

  // debug bodies, out of line (below): behind the same conditions and at the same points as ever
  int pq_stub(int k, hipStream_t ps);                        // BK_PQ_STUB builds with BIGKRLS_PQ_STUB
  int pqc_debug(int k, const double* P, int bits);           // BIGKRLS_PQC_DEBUG bits 4 and 2, after pq_chol's launch
  int trace_duplicate_run(int k);                            // BIGKRLS_TRACE_FINE: the thin products once more, compared
  // fine diagnostic trace (BIGKRLS_TRACE_FINE with BIGKRLS_TRACE_DIR): both streams drained, then hashes of the panel's
  // factors and of the whole working matrix -- serialises the loop, for hunting a nondeterminism only
  int fine(const char* tag, const double* p, int64_t count, int k) {
    if (!trace_fine()) return BIGKRLS_OK;
    BK_HIP(hipStreamSynchronize(side));
    return trace_point(ctx, st, tag, p, count, k);
  }

  // ---- the loop: helpers ---------------------------------------------------------------------------------------
  double* A22(int k) const { return W + (k + S2_B) + (int64_t)(k + S2_B) * N; }   // trailing matrix of panel k
  bool samp(int k) const { return ctx->profile && (k / S2_B) % S1_PROF_STRIDE == 0; }   // HIP-event sampling: every 8th panel
  static double piece_flops(double mm, double ca, double cb, double kk) {   // columns [ca, cb) of the lower triangle
    return 2.0 * kk * ((cb - ca) * mm - 0.5 * (cb * cb - ca * ca));
  }
  // Y2 = A22 W(k) on the main stream (A22 possibly stale: the callers correct the product), then the wait for the T
  // factor and the correction factors that were built on the look-ahead stream beside it
  int av(int k) {
    const int b = S2_B, m = n - k - b;
    if (samp(k)) BK_TRY(prof_begin(ctx, "band_av", 2.0 * (double)m * (double)m * b));
    BK_TRY(gemm(ctx, 0, 0, m, b, m, 1.0, A22(k), N, Vw(k), m, 0.0, ws.Y2, m));
    if (samp(k)) BK_TRY(prof_end(ctx, "band_av"));
    if (t_pending) {
      BK_HIP(hipStreamWaitEvent(st, ctx->ev_join2, 0));
      t_pending = false;
    }
    return BIGKRLS_OK;
  }
  // Look-ahead: panel kn is final once the step's thin products have updated its columns, so its latency-bound
  // factorisation runs on the side stream beside the throughput-bound update the caller launches next. ev_join: V (W) of
  // panel kn is ready; ev_join2: its T factor and factors() -- the caller's correction-factor products U'^T W(kn), with
  // ctx->stream on the side stream -- which only the step after A22 W(kn) needs.
  template <class F>
  int fork_panel(int kn, F factors) {
    BK_HIP(hipEventRecord(ctx->ev_fork, st));
    BK_HIP(hipStreamWaitEvent(side, ctx->ev_fork, 0));
    BK_TRY(panel_qr(kn, side));
    BK_HIP(hipEventRecord(ctx->ev_join, side));
    BK_TRY(build_T(kn, side));
    { StreamScope on(ctx, side); BK_TRY(factors()); }
    BK_HIP(hipEventRecord(ctx->ev_join2, side));
    t_pending = true;
    return BIGKRLS_OK;
  }
  int join() { BK_HIP(hipStreamWaitEvent(st, ctx->ev_join, 0)); return BIGKRLS_OK; }
  // One piece of a pair group's k = 256 update: the 64-wide columns [j0, j1) (j1 < 0: to the end) of the trailing matrix
  // that starts at row0, from buffer set `set` whose first row is og_
  int piece(int row0, int set, int og_, int j0, int j1, bool bracket) {
    const int b = S2_B, rows = n - row0;
    const int64_t off = row0 - og_;
    if (bracket) BK_TRY(prof_begin(ctx, "band_update2", piece_flops(rows, 64.0 * j0, j1 < 0 ? (double)rows : 64.0 * j1, 4.0 * b)));
    BK_TRY(syrk_mirror_cols(ctx, rows, 4 * b, -1.0, ws.aggPZ1[set] + off, ws.aggLd, ws.aggPZ2[set] + off, ws.aggLd,
                            W + row0 + (int64_t)row0 * N, N, j0, j1));
    if (bracket) BK_TRY(prof_end(ctx, "band_update2"));
    return BIGKRLS_OK;
  }

  // ---- the loop: phases (DESIGN.md section 4, "Stage 1: phases of one struct") ------------------------------------
  // the per-call switches of the schedule and the streams (the loop state starts as a fresh Stage1 has it)
  int begin_loop() {
    if (const char* am = getenv("BIGKRLS_S1AGG_MIN")) sched.agg_min = std::max(4 * S2_B, atoi(am));   // (development: threshold sweep)
    const char* agg_env = getenv("BIGKRLS_S1AGG");   // =0: one trailing update per panel from the start; =2: pairs from the start
    sched.agg_mode = agg_env && std::string(agg_env) == "0" ? 0 : agg_env && std::string(agg_env) == "2" ? 2 : -1;
    if (sched.quads_on())
      if (const char* qm = getenv("BIGKRLS_S1AGG4_MIN")) sched.quad_min = std::max(sched.agg_min, atoi(qm));
    static const int swap_m = [] { const char* e = getenv("BIGKRLS_S1_SWAP_M"); return e ? atoi(e) : S1_SWAP_M; }();
    sched.swap_m = swap_m;
    st = ctx->stream;
    BK_TRY(side_stream_get(ctx));
    side = ctx->side_stream;
    sched.side_is_main = ctx->side_is_main;
    return BIGKRLS_OK;
  }
  int first_panel() {
    if (!has_panel(0)) return BIGKRLS_OK;
    BK_TRY(panel_qr(0, st));
    return build_T(0, st);
  }

  // ---- aggregated phases: several panels per pass over A22 ------------------------------------------------------
  // At k = 128 the trailing update sits on the ridge between the MFMA and the HBM roof and reaches neither
  // (read-modify-write of 12 m^2 bytes per 128 ranks); applied for two panels at once (k = 256) it runs at 0.60 of the
  // MFMA peak instead of 0.41, for four (k = 512) at 0.73. Until a deferred update has run the bulk of A22 is stale, and
  // what reads it is corrected by thin products with the pending reflector blocks U = [V_a Z_a V_b Z_b ...],
  // U' = [Z_a V_a Z_b V_b ...]:
  //   Y = A22 V  =  A22_stale V  -  U (U'^T V)  (+  P1 U (U'^T P1 V)      P1: rows in R1, where a pair's piece a is applied)
  //   the next panel's 64 columns (never covered by a deferred update) get  - U U'[those rows]^T  explicitly.
  // The factors U'^T V only need the next panel's V: they are formed on the look-ahead stream right after its QR.
  //
  // Groups of FOUR panels, one k = 512 update per group, while the trailing matrix has >= 12 800 rows. No pieces here: the
  // whole update of a group is launched at the end of its fourth step (beside the next group's first panel
  // factorisation); the three factorisations inside a group run alone, which costs little -- beside an update they only
  // overlap by a quarter of their length. Panel j of a group corrects its product with the j pending blocks and updates
  // the next panel's columns with them explicitly. Stage 1 at N = 20 000: 285.7 -> 283.0 ms (same box; BIGKRLS_S1AGG=2:
  // pairs from the start).
  int run_quads() {
    for (; sched.quad_ok(k); ++gq, ++done.quads) {
      const int ogq = k + S2_B;
      for (int j = 0; j < 4; ++j, k += S2_B) BK_TRY(quad_step(j, ogq));
    }
    return BIGKRLS_OK;
  }
  int quad_step(int j, int ogq) {
    const int b = S2_B, m = n - k - b, mn = m - b;
    const int64_t ldg = ws.aggLd;
    double *PZ1q = ws.aggPZ1[0], *PZ2q = ws.aggPZ1[1];           // n x 8b each: the allocation's four 4b-wide blocks
    double* Cfull = ws.aggC;
    BK_TRY(av(k));
    const int64_t off = (k + b) - ogq;
    if (j > 0) {
      BK_TRY(gemm(ctx, 0, 0, m, b, 2 * b * j, -1.0, PZ1q + off, ldg, Cfull, 2 * b * j, 1.0, ws.Y2, m));
      BK_TRY(gemm(ctx, 0, 1, m, b, 2 * b * j, -1.0, PZ1q + off, ldg, PZ2q + off, ldg, 1.0, A22(k), N));
    }
    const int64_t roff = off + (int64_t)j * 2 * b * ldg;
    BK_TRY(small_products_to(k, ws.Y2, A22(k), PZ1q + roff, PZ2q + roff, ldg));
    BK_TRY(fork_panel(k + b, [&] {
      return j < 3 ? gemm(ctx, 1, 0, 2 * b * (j + 1), b, mn, 1.0, PZ2q + off + b, ldg, Vw(k + b), mn, 0.0, Cfull, 2 * b * (j + 1))
                   : BIGKRLS_OK;
    }));
    if (j == 3) {
      const bool samp4 = ctx->profile && (gq & 1) == 0;      // (bench.py: every second group's update bracketed)
      BK_TRY(gate());
      if (samp4) BK_TRY(prof_begin(ctx, "band_update4", piece_flops(mn, 0.0, (double)mn, 8.0 * b)));
      BK_TRY(syrk_mirror_cols(ctx, mn, 8 * b, -1.0, PZ1q + off + b, ldg, PZ2q + off + b, ldg, A22(k + b), N, 0, -1));
      if (samp4) BK_TRY(prof_end(ctx, "band_update4"));
    }
    return join();
  }

  // Groups of TWO panels down to AGG_MIN_M rows. The update of a group is applied in two pieces of equal area, one per
  // panel step, so that every step still has a throughput-bound launch to hide the next panel's latency-bound QR behind:
  //   piece a, launched at the end of the group's second step: the columns >= c1 of the trailing matrix (lower triangle +
  //            mirror = the square R1 x R1, R1 = [c1, n));
  //   piece b, launched at the end of the next group's first step (or by hand_over): the columns < c1.
  // Below AGG_MIN_M the panel QR (~0.8 ms while it shares the GPU with an update), not the piece, is the longer of the two
  // concurrent launches and the ~0.1 ms of thin correction products per step no longer pay (measured per step,
  // N = 20 000: -0.2 ms at m = 19 000, 0 at m = 14 500).
  int run_pairs() {
    for (; sched.pair_ok(k); ++gi, ++done.pairs) {
      og = k + S2_B;                                        // first row held by this group's buffers
      for (int half = 0; half < 2; ++half, k += S2_B) BK_TRY(pair_step(half));
      have_prev = true;
      c1_prev = c1;
      og_prev = og;
    }
    return BIGKRLS_OK;
  }
  int pair_step(int half) {
    const int b = S2_B, m = n - k - b, mn = m - b;          // rows of the trailing matrices T_k, T_{k+1}
    const int64_t ldg = ws.aggLd;
    const int set = gi & 1;
    double *PZ1g = ws.aggPZ1[set], *PZ2g = ws.aggPZ2[set], *PZ1p = ws.aggPZ1[set ^ 1], *PZ2p = ws.aggPZ2[set ^ 1];
    double *Cfull = ws.aggC, *CR1 = Cfull + 4 * b * b, *Ca = CR1 + 4 * b * b;
    BK_TRY(av(k));
    if (half == 0 && have_prev) {
      const int64_t off = (k + b) - og_prev;
      const int64_t r1 = c1_prev - (k + b);
      BK_TRY(gemm(ctx, 0, 0, m, b, 4 * b, -1.0, PZ1p + off, ldg, Cfull, 4 * b, 1.0, ws.Y2, m));
      if (r1 < m)
        BK_TRY(gemm(ctx, 0, 0, m - r1, b, 4 * b, 1.0, PZ1p + off + r1, ldg, CR1, 4 * b, 1.0, ws.Y2 + r1, m));
      // the next panel's columns: the previous group's update (no piece covers them)
      BK_TRY(gemm(ctx, 0, 1, m, b, 4 * b, -1.0, PZ1p + off, ldg, PZ2p + off, ldg, 1.0, A22(k), N));
    } else if (half == 1) {
      const int64_t off = (k + b) - og;
      BK_TRY(gemm(ctx, 0, 0, m, b, 2 * b, -1.0, PZ1g + off, ldg, Ca, 2 * b, 1.0, ws.Y2, m));
      BK_TRY(gemm(ctx, 0, 1, m, b, 2 * b, -1.0, PZ1g + off, ldg, PZ2g + off, ldg, 1.0, A22(k), N));
    }
    // Z of this panel into the group's blocks; s1_fused_z also applies this panel's own update to the next panel's columns
    const int64_t roff = (k + b) - og + (int64_t)half * 2 * b * ldg;
    BK_TRY(small_products_to(k, ws.Y2, A22(k), PZ1g + roff, PZ2g + roff, ldg));
    // correction factors of the next step: U'^T W_{next} (and its part over R1) -- they act on Y2 = A22 W_{next}, which
    // Tfold takes to Y as a whole (W = V U row by row, so the part over R1 is in the same space)
    BK_TRY(fork_panel(k + b, [&] {
      if (half == 0) return gemm(ctx, 1, 0, 2 * b, b, mn, 1.0, PZ2g + b, ldg, Vw(k + b), mn, 0.0, Ca, 2 * b);
      c1 = s1_piece_c1(k + 2 * b, mn);
      const int64_t r1n = c1 - (k + 2 * b);
      BK_TRY(gemm(ctx, 1, 0, 4 * b, b, mn, 1.0, PZ2g + 2 * b, ldg, Vw(k + b), mn, 0.0, Cfull, 4 * b));
      return gemm(ctx, 1, 0, 4 * b, b, mn - r1n, 1.0, PZ2g + 2 * b + r1n, ldg, Vw(k + b) + r1n, mn, 0.0, CR1, 4 * b);
    }));
    // the throughput-bound launch of this step, concurrent with the panel QR
    if (half == 0 && have_prev) {
      BK_TRY(gate());
      BK_TRY(piece(k + 2 * b, set ^ 1, og_prev, 0, s1_piece_cols(c1_prev, k + 2 * b), samp(k)));
    } else if (half == 1) {
      BK_TRY(gate());
      BK_TRY(piece(k + 2 * b, set, og, s1_piece_cols(c1, k + 2 * b), -1, samp(k)));
    }
    return join();
  }
  // hand-over to one update per panel: piece b of the last pair group on the whole of T_k
  int hand_over() {
    if (!have_prev) return BIGKRLS_OK;
    return piece(k + S2_B, (gi - 1) & 1, og_prev, 0, s1_piece_cols(c1_prev, k + S2_B), false);
  }

  // ---- one update per panel -------------------------------------------------------------------------------------
  int run_single() {
    for (; has_panel(k); k += S2_B) {
      BK_TRY(single_products());
      switch (sched.single_arm(k)) {
        case S1Arm::OneStream: ++done.one_stream; BK_TRY(single_one_stream()); break;
        case S1Arm::TwoStream: ++done.two_stream; BK_TRY(single_two_stream()); break;
        default: ++done.last; BK_TRY(single_last()); break;
      }
    }
    return BIGKRLS_OK;
  }
  // what every arm starts with: A22 W, the thin products and, when a register-resident panel QR follows, the update of
  // the next panel's columns by s1_fused_z
  int single_products() {
    const int b = S2_B, m = n - k - b;
    BK_TRY(fine("R:s1_W", W, N * N, k));
    BK_TRY(fine("R:s1_V", ws.Vp, (int64_t)m * b, k));
    BK_TRY(fine("R:s1_tau", taus1 + k, b, k));
    BK_TRY(av(k));
    panel_in_z = sched.panel_in_z(k);
    BK_TRY(fine("R:s1_Y2", ws.Y2, (int64_t)m * b, k));
    BK_TRY(fine("R:s1_T", Tof(k), b * b, k));
    BK_TRY(small_products(k, ws.Y2, panel_in_z ? A22(k) : (double*)nullptr));
    BK_TRY(fine("R:s1_PZ1", ws.PZ1, (int64_t)m * 2 * b, k));
    BK_TRY(fine("R:s1_PZ2", ws.PZ2, (int64_t)m * 2 * b, k));
    if (trace_fine()) BK_TRY(trace_duplicate_run(k));
    return BIGKRLS_OK;
  }
  // algorithmic flops of the bracketed update: without the first 64 columns when s1_fused_z has already updated them
  double single_flops() const {
    const double mu = (double)(n - k - S2_B - (panel_in_z ? S2_B : 0));
    return mu * (mu + 1.0) * 2.0 * S2_B;
  }
  // the two-sided update A22 -= V Z' + Z V' of panel k: tile columns [c0, c1) (c1 < 0: to the end)
  int single_update(int c0, int c1_, bool narrow, bool skip_first = false) {
    return syrk_mirror(ctx, n - k - S2_B, 2 * S2_B, -1.0, ws.PZ1, n - k - S2_B, ws.PZ2, n - k - S2_B, A22(k), N, c0, c1_, narrow, skip_first);
  }
  // Small trailing matrices (below S1_SWAP_M rows; round 6): the chain fused products -> panel factorisation -> A22 V
  // -> fused products IS the critical path there (the update is the shorter of the two concurrent launches), and
  // each of its two stream changes cost 12-15 us (from the end of a kernel on one stream to the start of its
  // dependant on the other; profiles/r05/r05b_C2_panel_chain_timeline.log). So the chain stays on the main stream --
  // the factorisation (which now writes its T factor itself) starts right behind s1_fused_z, A22 V right behind it --
  // and the trailing update moves to the look-ahead stream, joined before A22 V reads the matrix. The tail of the split
  // factorisation follows the update there (behind ev_pq): the update is the shorter of the two launches, so the tail
  // starts with A22 W and ends before s1_fused_yt needs V and Tfold wherever that product is the longer one.
  int single_one_stream() {
    BK_HIP(hipEventRecord(ctx->ev_fork, st));
    BK_HIP(hipStreamWaitEvent(side, ctx->ev_fork, 0));
    {
      StreamScope on(ctx, side);
      if (samp(k)) BK_TRY(prof_begin(ctx, "band_update", single_flops()));
      BK_TRY(single_update(0, -1, true, true));
      if (samp(k)) BK_TRY(prof_end(ctx, "band_update"));
    }
    BK_HIP(hipEventRecord(ctx->ev_join, side));     // the update is done
    BK_TRY(panel_qr(k + S2_B, st));
    BK_HIP(hipEventRecord(ctx->ev_pq, st));
    BK_HIP(hipStreamWaitEvent(side, ctx->ev_pq, 0));
    BK_TRY(build_T(k + S2_B, side));                // (the factorisation's tail, beside A22 W; the T chain of a panel that fell back)
    BK_HIP(hipEventRecord(ctx->ev_join2, side));
    t_pending = true;
    return join();
  }
  // the update on the main stream, the next factorisation beside all of it but the next panel's own tile column
  int single_two_stream() {
    const bool narrow = resident_qr(k + S2_B);   // tile shape that shares the GPU best with the concurrent QR
    if (samp(k)) BK_TRY(prof_begin(ctx, "band_update", single_flops()));
    if (!panel_in_z) BK_TRY(single_update(0, 1, narrow));   // next panel's tiles
    BK_TRY(fork_panel(k + S2_B, [] { return (int)BIGKRLS_OK; }));
    BK_TRY(gate());
    if (panel_in_z) BK_TRY(single_update(0, -1, narrow, true));   // everything but the first 64-wide tile column (done by s1_fused_z)
    else BK_TRY(single_update(1, -1, narrow));                     // the rest
    if (samp(k)) BK_TRY(prof_end(ctx, "band_update"));
    return join();
  }
  int single_last() {
    if (samp(k)) BK_TRY(prof_begin(ctx, "band_update", single_flops()));
    BK_TRY(single_update(0, -1, false));        // A22 -= VZ' + ZV'
    if (samp(k)) BK_TRY(prof_end(ctx, "band_update"));
    return BIGKRLS_OK;
  }

};

// fine diagnostic trace only: element-wise comparison of two runs of the same kernels on the same inputs.
// out[0] = number of differing entries, out[1] = first differing index, out[2] = largest |a - b| (as bits, via atomicMax on
// the non-negative double's integer image), out[3] = number of differing 64-row blocks touched (approximate: per block flag)
__global__ void s1_dbg_compare(const double* __restrict__ a, const double* __restrict__ b, int64_t rows, int64_t cols, int64_t ld,
                               unsigned long long* __restrict__ out, unsigned int* __restrict__ blockflag) {
  const int64_t total = rows * cols;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e % rows, c = e / rows;
    const double x = a[r + c * ld], y = b[r + c * ld];
    if (__double_as_longlong(x) != __double_as_longlong(y)) {
      atomicAdd(out, 1ull);
      atomicMin(out + 1, (unsigned long long)e);
      const double d = fabs(x - y);
      atomicMax(out + 2, (unsigned long long)__double_as_longlong(d == d ? d : 1e300));
      if (atomicExch(blockflag + (r / 64) * 4 + (c / 64 < 3 ? c / 64 : 3), 1u) == 0u) atomicAdd(out + 3, 1ull);
    }
  }
}

// experiment build only (BK_PQ_STUB, tools/pq_exposure.py): no panel QR at all -- tau = 0, V = 0: the decomposition is
// garbage but finite, and its stage-1 time is what a free panel factorisation would leave
inline int Stage1::pq_stub(int k, hipStream_t ps) {
  const int pw = S2_B, m = n - k - S2_B;
  BK_HIP(hipMemsetAsync(taus1 + k, 0, pw * sizeof(double), ps));
  BK_HIP(hipMemsetAsync(taus1 + n + k, 0, pw * sizeof(double), ps));
  BK_HIP(hipMemsetAsync(ws.Vp, 0, (size_t)m * pw * sizeof(double), ps));
  return BIGKRLS_OK;
}

// BIGKRLS_PQC_DEBUG, after pq_chol's launch for panel k (P: its m x 64 block, leading dimension N). Bit 4: the panel as
// the kernel will see it, for bit 2: report the panels left to pq_resident (and the mailbox's Gram matrix against the host's)
inline int Stage1::pqc_debug(int k, const double* P, int bits) {
  const int b = S2_B, m = n - k - b;
  std::vector<double> dbgP;
  if (bits & 4) {
    BK_HIP(hipDeviceSynchronize());
    dbgP.resize((size_t)m * b);
    BK_HIP(hipMemcpy2D(dbgP.data(), (size_t)m * 8, P, (size_t)N * 8, (size_t)m * 8, b, hipMemcpyDeviceToHost));
  }
  if (!(bits & 2)) return BIGKRLS_OK;
  BK_HIP(hipDeviceSynchronize());
  if (!dbgP.empty()) {
    std::vector<double> Gd(PQC_NG);
    BK_HIP(hipMemcpy(Gd.data(), ws.pqc + PQC_OFF_SLICES, PQC_NG * sizeof(double), hipMemcpyDeviceToHost));
    double worst = 0.0, gmax = 0.0; int wi = 0, wc = 0, nanc = 0;
    for (int i = 0; i < b; ++i)
      for (int c = 0; c < b; ++c) {
        long double sum = 0.0L;
        for (int r = 0; r < m; ++r) sum += (long double)dbgP[r + (size_t)i * m] * dbgP[r + (size_t)c * m];
        const double g = Gd[i * b + c];
        if (!(g == g)) ++nanc;
        const double d = fabs(g - (double)sum);
        gmax = std::max(gmax, fabs((double)sum));
        if (d > worst || !(d == d)) { worst = d; wi = i; wc = c; }
      }
    fprintf(stderr, "[bigkrls] panel k=%d: summed Gram matrix in the mailbox vs host: max diff %.3e at (%d,%d), |G| max %.3e, NaNs %d\n", k, worst, wi, wc, gmax, nanc);
  }
  int fb = 0;
  BK_HIP(hipMemcpy(&fb, ws.fallback, sizeof(int), hipMemcpyDeviceToHost));
  double dbg[16];
  BK_HIP(hipMemcpy(dbg, ws.pqc + PQC_OFF_SLICES + PQC_NG, sizeof(dbg), hipMemcpyDeviceToHost));
  if (fb) fprintf(stderr, "[bigkrls] pq_chol left panel k=%d (m=%d) to the Householder kernel: pass 0 bad=%g dmin=%.3e dmax=%.3e; pass 1 bad=%g dmin=%.3e dmax=%.3e\n", k, m, dbg[0], dbg[1], dbg[2], dbg[8], dbg[9], dbg[10]);
  return BIGKRLS_OK;
}

// BIGKRLS_TRACE_FINE: the same three kernels once more on the same inputs (without the update of the next panel's
// columns), into a second pair of buffers: any difference is a nondeterminism caught in the act -- where, how much, how many
inline int Stage1::trace_duplicate_run(int k) {
  const int pw = S2_B, m = n - k - S2_B;
  void* pdup = nullptr;
  BK_TRY(ws_get(ctx, SLOT_DERIV_B, (4 * (int64_t)N * pw + 2 * (N / 64 + 2) * 4 + 64) * (int64_t)sizeof(double), &pdup));
  double* d1 = (double*)pdup;
  double* d2 = d1 + 2 * (int64_t)N * pw;
  unsigned long long* dout = (unsigned long long*)(d2 + 2 * (int64_t)N * pw);
  unsigned int* dflag = (unsigned int*)(dout + 8);
  BK_TRY(small_products_to(k, ws.Y2, nullptr, d1, d2, m));
  for (int which = 0; which < 2; ++which) {
    BK_HIP(hipMemsetAsync(dout, 0, 8 * sizeof(unsigned long long), st));
    BK_HIP(hipMemsetAsync(dout + 1, 0xff, sizeof(unsigned long long), st));
    BK_HIP(hipMemsetAsync(dflag, 0, (size_t)(N / 64 + 2) * 4 * sizeof(unsigned int), st));
    hipLaunchKernelGGL(s1_dbg_compare, dim3(512), dim3(256), 0, st, (const double*)(which ? ws.PZ2 : ws.PZ1),
                       (const double*)(which ? d2 : d1), (int64_t)m, (int64_t)2 * pw, (int64_t)m, dout, dflag);
    BK_CHECK_LAUNCH();
    unsigned long long h[4] = {0, 0, 0, 0};
    PinnedFetch pfc(ctx, 4);
    BK_TRY(pfc.add(h, dout, 4 * sizeof(unsigned long long)));
    BK_TRY(pfc.finish());
    if (h[0] != 0) {
      double md;
      memcpy(&md, &h[2], sizeof md);
      // (count in `count`, first differing row in `extra`; the hash field carries the largest difference's bits)
      fprintf(stderr, "[bigkrls] NONDETERMINISM caught: panel k=%d, %s of two runs of s1_fused_yt/s/z on the same inputs differ in %llu of %lld "
                      "entries, first at (row %lld, column %lld), largest difference %.3e, %llu distinct 64 x 64 blocks\n",
              k, which ? "[Z | V]" : "[V | Z]", h[0], (long long)m * 2 * pw, (long long)(h[1] % m), (long long)(h[1] / m), md, h[3]);
      BK_TRY(trace_host(which ? "X:dup_PZ2" : "X:dup_PZ1", h, 4, k));
    }
  }
  return BIGKRLS_OK;
}

int stage1_to_band(bigkrls_ctx* ctx, double* W, int n, double* taus1, const Stage1Ws& ws) {
  Stage1 s1;
  BK_TRY(s1.init(ctx, W, n, taus1, ws));
  BK_TRY(s1.begin_loop());
  BK_TRY(s1.first_panel());
  BK_TRY(s1.run_quads());
  BK_TRY(s1.run_pairs());
  BK_TRY(s1.hand_over());
  BK_TRY(s1.run_single());
  if (verbose())
    fprintf(stderr, "[bigkrls] stage 1 schedule: n=%d: %d groups of four, %d pair groups, %d two-stream panels, %d one-stream panels\n",
            n, s1.done.quads, s1.done.pairs, s1.done.two_stream, s1.done.one_stream);
  return BIGKRLS_OK;
}

// ---------------------------------------------------------------------------
// stage 2: bulge chasing. Task (s,t): index block I_t = [s+1+t b, min(s+(t+1)b, n-1)].
// ---------------------------------------------------------------------------
__device__ __forceinline__ double& band_at(double* AB, int r, int c) {
  return AB[(r - c) + (int64_t)c * S2_LD];
}

// Band accesses of the persistent kernel go through agent-scope relaxed atomics (sc1 loads and
// write-through stores): workgroups on different XCDs exchange band data inside one launch and
// the per-XCD L2s are not coherent with each other for ordinary accesses.
template <bool COH>
__device__ __forceinline__ double band_ld(const double* p) {
  return COH ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}
template <bool COH>
__device__ __forceinline__ void band_st(double* p, double v) {
  if (COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

struct BcShared {
  double* sW; double* sD; double* sv; double* svp; double* sy; double* su; double* sp; double* sz;
  double* sq; double* s_sc;
};

// One bulge-chasing task (s,t). VP_LOCAL: the previous reflector of the sweep (task (s,t-1))
// is still in this workgroup's LDS (sv / s_sc[0]) instead of being read back from VV / TT.
template <bool COH, bool VP_LOCAL>
__device__ __forceinline__ void bc_task(double* __restrict__ AB, int n, int s, int t,
                                        const int64_t* __restrict__ soff, double* __restrict__ VV,
                                        double* __restrict__ TT, const BcShared& sh) {
  // With W the off-diagonal block (rows I_t, cols I_{t-1}), D the
  // diagonal block, (v_p, tau_p) the previous reflector of the sweep and (v, tau) the new one:
  //   y = tau_p W v_p ;  x = W[:,0] - y v_p[0]  -> v, tau, beta
  //   z = tau (v'W - (v'y) v_p') ;  W' = W - y v_p' - v z'   (one pass, straight to memory)
  //   p = tau D v ;  K = tau/2 p'v ;  q = p - K v ;  D' = D - v q' - q v'
  constexpr int B = S2_B;
  constexpr int LDW = B + 1;
  double* sW = sh.sW; double* sD = sh.sD; double* sv = sh.sv; double* svp = sh.svp; double* sy = sh.sy;
  double* su = sh.su; double* sp = sh.sp; double* sz = sh.sz; double* sq = sh.sq; double* s_sc = sh.s_sc;
  const int tid = threadIdx.x;
  const int lo = s + 1 + t * B;
  const int hi = min(s + (t + 1) * B, n - 1);
  const int len = hi - lo + 1;  // 1..B
  const int plo = lo - B;
  const int64_t ridx = soff[s] + t;
  const int i = tid & 63, j0 = tid >> 6;
  // ---- loads: everything is issued before the first LDS write -----------------------------
  double wreg[16], dreg[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int j = j0 + 4 * q;
    wreg[q] = (t > 0 && i < len) ? band_ld<COH>(&band_at(AB, lo + i, plo + j)) : 0.0;
    dreg[q] = (i < len && j < len && i >= j) ? band_ld<COH>(&band_at(AB, lo + i, lo + j)) : 0.0;
  }
  double x0 = 0.0, vpv = 0.0;
  if (tid < B) {
    if (t > 0) vpv = VP_LOCAL ? sv[tid] : VV[(ridx - 1) * B + tid];
    else if (tid < len) x0 = band_ld<COH>(&band_at(AB, lo + tid, s));
  }
  if (tid == 0) s_sc[2] = (t > 0) ? (VP_LOCAL ? s_sc[0] : TT[ridx - 1]) : 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int j = j0 + 4 * q;
    sW[i + j * LDW] = wreg[q];
    if (i >= j) {
      sD[i + j * LDW] = dreg[q];
      if (i > j) sD[j + i * LDW] = dreg[q];
    }
  }
  if (tid < B) svp[tid] = vpv;
  __syncthreads();
  const int idx = tid >> 2, qq = tid & 3;  // 4 threads per row / column
  // ---- y = tau_p W v_p ------------------------------------------------------------------
  if (t > 0) {
    double acc = 0.0;
    // lanes (idx, qq) of a half-wave hit bank (idx + j) mod 32: j = 32h + 8qq + i keeps them distinct
#pragma unroll
    for (int h = 0; h < B / 32; ++h)
#pragma unroll
      for (int i2 = 0; i2 < 8; ++i2) {
        const int j = 32 * h + 8 * qq + i2;
        acc += sW[idx + j * LDW] * svp[j];
      }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    if (qq == 0) sy[idx] = acc * s_sc[2];
    __syncthreads();
  }
  // ---- reflector ----------------------------------------------------------------------------
  if (tid < 64) {
    double x = 0.0;
    if (tid < len) x = (t > 0) ? sW[tid] - sy[tid] * svp[0] : x0;
    double ss = (tid >= 1) ? x * x : 0.0;
    ss = wsum(ss);
    const double alpha = __shfl(x, 0, 64);
    double beta, tt, sc;
    if (ss == 0.0) { beta = alpha; tt = 0.0; sc = 0.0; }
    else {
      beta = -copysign(hh_norm(alpha, ss), alpha);
      tt = (beta - alpha) / beta;
      sc = 1.0 / (alpha - beta);
    }
    const double v = (tid == 0) ? 1.0 : x * sc;
    sv[tid] = v;
    VV[ridx * B + tid] = v;
    if (tid == 0) { s_sc[0] = tt; s_sc[1] = beta; TT[ridx] = tt; }
  }
  __syncthreads();
  const double tau = s_sc[0];
  // ---- u = v'W (per column), p = tau D v (per row) ----------------------------------------------
  {
    double au = 0.0, ap = 0.0;
#pragma unroll
    for (int h = 0; h < B / 32; ++h)
#pragma unroll
      for (int i2 = 0; i2 < 8; ++i2) {
        const int k = 32 * h + 8 * qq + i2;
        const double vk = sv[k];
        au += vk * sW[k + idx * LDW];
        ap += sD[idx + k * LDW] * vk;
      }
    au += __shfl_xor(au, 1, 64);
    au += __shfl_xor(au, 2, 64);
    ap += __shfl_xor(ap, 1, 64);
    ap += __shfl_xor(ap, 2, 64);
    if (qq == 0) { su[idx] = au; sp[idx] = ap * tau; }
  }
  __syncthreads();
  if (tid < 64) {
    const double cc = (t > 0) ? wsum(sv[tid] * sy[tid]) : 0.0;
    const double kk = 0.5 * tau * wsum(sp[tid] * sv[tid]);
    sz[tid] = tau * (su[tid] - cc * svp[tid]);
    sq[tid] = sp[tid] - kk * sv[tid];
  }
  __syncthreads();
  // ---- write-out ---------------------------------------------------------------------------------
  const double vi = sv[i], qi = sq[i];
  const double yi = (t > 0) ? sy[i] : 0.0;
  if (i < len) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int j = j0 + 4 * q;
      if (t > 0) {
        double w = wreg[q] - yi * svp[j] - vi * sz[j];
        if (j == 0) w = (i == 0) ? s_sc[1] : 0.0;
        band_st<COH>(&band_at(AB, lo + i, plo + j), w);
      }
      if (i >= j) band_st<COH>(&band_at(AB, lo + i, lo + j), dreg[q] - vi * sq[j] - qi * sv[j]);
    }
    if (t == 0 && j0 == 0) band_st<COH>(&band_at(AB, lo + i, s), (i == 0) ? s_sc[1] : 0.0);
  }
}

#define BC_SHARED_DECL                                                        \
  __shared__ double sW[S2_B * (S2_B + 1)];                                    \
  __shared__ double sD[S2_B * (S2_B + 1)];                                    \
  __shared__ double sv[S2_B], svp[S2_B], sy[S2_B], su[S2_B], sp[S2_B], sz[S2_B], sq[S2_B]; \
  __shared__ double s_sc[4]; /* tau, beta, tau_p */                           \
  const BcShared sh{sW, sD, sv, svp, sy, su, sp, sz, sq, s_sc};

// One launch per anti-diagonal wavefront 2s + t = wave_t: one workgroup per task.
__global__ __launch_bounds__(256) void bc_wavefront(double* __restrict__ AB, int n, int wave_t, int s_min,
                                                    const int64_t* __restrict__ soff,
                                                    double* __restrict__ VV, double* __restrict__ TT) {
  BC_SHARED_DECL
  const int s = s_min + blockIdx.x;
  bc_task<false, false>(AB, n, s, wave_t - 2 * s, soff, VV, TT, sh);
}

// Persistent variant: ONE launch for the whole stage. Workgroup k owns sweeps k, k+G, k+2G, ...
// and walks each of them down the band; task (s,t) may start once sweep s-1 has finished task
// t+1 (progress[s-1] >= t+2, or sweep s-1 is complete). progress[] is published with a
// release fence + barrier + agent-scope store, polled with agent-scope loads. Every sweep only
// waits on a lower-numbered sweep and G never exceeds the number of co-resident workgroups, so
// the lowest unfinished sweep can always run. A bounded spin (watchdog) turns any scheduling
// surprise into an error code instead of a hang.
__global__ __launch_bounds__(256, 2) void bc_persistent(double* __restrict__ AB, int n,
                                                     const int64_t* __restrict__ soff,
                                                     double* __restrict__ VV, double* __restrict__ TT,
                                                     int* __restrict__ progress, int* __restrict__ err,
                                                     int nsweep) {
  BC_SHARED_DECL
  __shared__ int s_ok;
  const int tid = threadIdx.x;
  for (int s = blockIdx.x; s < nsweep; s += gridDim.x) {
    const int T_s = (n - 2 - s) / S2_B + 1;      // tasks of this sweep
    const int T_prev = (n - 1 - s) / S2_B + 1;   // tasks of sweep s-1
    for (int t = 0; t < T_s; ++t) {
      if (s > 0) {
        if (tid == 0) {
          const int need = min(t + 2, T_prev);
          long spins = 0;
          int ok = 1;
          while (__hip_atomic_load(progress + (s - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) {
            __builtin_amdgcn_s_sleep(1);
            if ((++spins & 255) == 0 &&
                (spins > BC_SPIN_LIMIT ||
                 __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
              __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              ok = 0;
              break;
            }
          }
          s_ok = ok;
        }
        __syncthreads();
        if (!s_ok) return;   // uniform
      }
      bc_task<true, true>(AB, n, s, t, soff, VV, TT, sh);
      // every thread makes its own stores visible device-wide, then one thread publishes
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      __syncthreads();
      if (tid == 0) __hip_atomic_store(progress + s, t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---------------------------------------------------------------------------
// LDS-resident bulge chasing: workgroup t owns band LOCATION t for the whole stage.
//
// At sweep s it holds columns I_t(s) = [s+1+tb, s+(t+1)b] of the band (each column from its
// diagonal down to the end of I_{t+1}(s): up to 2b rows) in LDS, as a circular buffer indexed
// by column mod b. Its task for sweep s, given the reflector (v, tau) on rows I_t(s):
//     D = A[I_t, I_t]      <- H D H                       (two-sided)
//     W = A[I_{t+1}, I_t]  <- H' (W H),  H' = new reflector zeroing (W H)[1:, 0]
// and it then passes (v', tau') down to location t+1 and its first column (which leaves
// I_t(s+1)) up to location t-1, whose window gains it as the new last column. Location 0
// keeps the leaving column itself: it is the next sweep's column to annihilate, and its head
// is the finished diagonal entry. So after the initial load the band never touches global
// memory again; only 65-double messages cross workgroups (agent-scope write-through stores,
// a release fence, a flag; polled with agent-scope loads). Per sweep a location waits for
// (s, t-1) and (s-1, t+1): the same dependency DAG as the wavefront kernel.
// All n/b locations must be co-resident (two workgroups per CU): the host checks the occupancy
// and falls back to the wavefront kernel otherwise; every poll is bounded (watchdog).
// ---------------------------------------------------------------------------
#ifdef BK_BC_PROF
// (profiling builds: where one middle location spends its sweep, in shader clocks, tools/bc_prof.py)
__device__ long long bc_prof_acc[8];
__device__ unsigned long long bc_prof_stamp[4];   // send times (100 MHz) of the reflector / column that the profiled location awaits
// timeline of a few locations over a few sweeps (100 MHz stamps): bc_trace[loc][sweep - BC_TR_S0][event]
constexpr int BC_TR_LOCS = 6, BC_TR_SW = 12, BC_TR_EV = 10, BC_TR_S0 = 2000;
__device__ unsigned long long bc_trace[BC_TR_LOCS * BC_TR_SW * BC_TR_EV];
#define BC_TRACE(ev, cond)                                                                                   \
  if (bc_tr_loc >= 0 && s >= BC_TR_S0 && s < BC_TR_S0 + BC_TR_SW && (cond))                                   \
    bc_trace[(bc_tr_loc * BC_TR_SW + (s - BC_TR_S0)) * BC_TR_EV + (ev)] = wall_clock64();
#define BC_TICK(slot)                                                   \
  if (bc_prof_on) {                                                     \
    const long long now_ = clock64();                                   \
    bc_prof_acc[slot] += now_ - bc_prof_t;                              \
    bc_prof_t = now_;                                                   \
  }
#else
#define BC_TICK(slot)
#define BC_TRACE(ev, cond)
#endif
constexpr int RB_LDC = 2 * S2_B + 9;   // window column stride; mod 32 == 9 keeps the 4-lanes-per-row matvec reads conflict-free
static_assert(RB_BOX == 2 * (S2_B + 1), "a message of the resident bulge chasing: 65 (value, value ^ key(sweep)) pairs");

// NTH threads (256 or 512): the matvecs use NTH / 64 lanes per row, the update NTH / 64 column groups. With 512 a SIMD
// holds two waves of the workgroup, which hides the LDS round trips a single wave per SIMD waits out (the kernel is
// bound by the busy time of a location per sweep, tools/bc_prof.py, not by the hops).
template <int NTH>
__global__ __launch_bounds__(NTH, NTH / 128) void bc_resident(const double* __restrict__ AB, int n,
                                                      const int64_t* __restrict__ soff,
                                                      double* __restrict__ VV, double* __restrict__ TT,
                                                      double* __restrict__ dvec, double* __restrict__ evec,
                                                      double* __restrict__ mail, int* __restrict__ err) {
  constexpr int B = S2_B, LDC = RB_LDC;
  constexpr int PARTS = NTH / 64;      // lanes per row (matvecs) / column groups (update)
  constexpr int NJ = B / PARTS;        // columns per lane / per group
  __shared__ double win[B * LDC];
  __shared__ double sv[B], svn[B], sy[B], sp[B], su[B], sz[B], sq[B];
  __shared__ double xcol[B + 1];
  __shared__ double s_sc[4];   // tau, taun, betan
  __shared__ int s_fail;
  const int t = blockIdx.x, tid = threadIdx.x;
  double* vbox = mail + (int64_t)t * 2 * RB_BOX;   // inbound: reflector from location t-1
  double* cbox = vbox + RB_BOX;                    // inbound: column from location t+1
  if (tid == 0) s_fail = 0;
  // ---- initial window: columns 1 + tB .. of the band ------------------------------------------
  for (int e = tid; e < B * LDC; e += NTH) win[e] = 0.0;
  if (tid <= B) xcol[tid] = 0.0;
  __syncthreads();
  {
    const int lo0 = 1 + t * B;
    for (int e = tid; e < B * (B + 1); e += NTH) {
      const int j = e / (B + 1), d = e % (B + 1), c = lo0 + j;
      if (c < n && c + d < n) win[(c & (B - 1)) * LDC + d] = AB[d + (int64_t)c * S2_LD];
    }
    if (t == 0 && tid <= B && tid < n) xcol[tid] = AB[tid];   // column 0: head + the rows to annihilate
  }
  __syncthreads();
  const int i4 = tid / PARTS, qq = tid % PARTS;
  auto part_sum = [](double v) {       // over the PARTS adjacent lanes of a row
    v = quad_sum(v);
    if (PARTS == 8) v += dpp_move<0x141>(v);   // row_half_mirror: the other quad of the 8-lane half
    return v;
  };
#ifdef BK_BC_PROF
  const bool bc_prof_on = (t == (int)gridDim.x / 3) && tid == 128;   // a thread that takes part in every phase
  long long bc_prof_t = clock64();
#endif
  for (int s = 0; s <= n - 3; ++s) {
    const int lo = s + 1 + t * B;
    if (lo > n - 1) break;
    BC_TICK(7)   // loop overhead / end-of-sweep barrier
    const int cnew = lo + B - 1;                    // column entering the window at this sweep
    const bool need_col = (s > 0) && (cnew <= n - 1);
    // ---- inbound: the entering column (threads 128..) and the reflector (threads 0..64) ---------
    // (zeros enter instead when the window has reached the end of the matrix)
    const unsigned long long key = rb_key(s + 1);
    // The entering column is waited for AFTER the products with the rest of the window: it only contributes
    // W[:, B-1] v_{B-1} to y and D[B-1][B-1] v_{B-1} to p (one multiply-add per row, folded into the next
    // phase), so its arrival -- one of the two hops of the inter-workgroup cycle -- is followed by the reflector
    // generation directly instead of by the whole matvec.
    const bool entering = (s > 0);                  // (zeros enter once the window has reached the end of the matrix)
    const int sl_new = (cnew & (B - 1)) * LDC;
    if (t == 0) {
      if (tid < 64) {
        // annihilate column s below its first sub-diagonal entry: x = A[s+1 .. s+b, s]
        const double x = xcol[1 + tid];
        double ss = (tid >= 1) ? x * x : 0.0;
        ss = wave_sum(ss);
        const double alpha = lane_value(x, 0);
        double beta, tt, sc;
        if (ss == 0.0) { beta = alpha; tt = 0.0; sc = 0.0; }
        else {
          beta = -copysign(hh_norm(alpha, ss), alpha);
          tt = (beta - alpha) / beta;
          sc = 1.0 / (alpha - beta);
        }
        const double v = (tid == 0) ? 1.0 : x * sc;
        sv[tid] = v;
        const int64_t ridx = soff[s];
        VV[ridx * B + tid] = v;
        if (tid == 0) { s_sc[0] = tt; TT[ridx] = tt; dvec[s] = xcol[0]; evec[s] = beta; }
      }
    } else if (tid <= B) {
      double v = 0.0;
      if (!rb_recv(vbox, tid, key, err, &v)) s_fail = 1;
      if (tid < B) sv[tid] = v;
      else s_sc[0] = v;
    }
    __syncthreads();
    BC_TICK(0)   // wait for the reflector
    if (s_fail) return;   // uniform
    const double tau = s_sc[0];
    // element (row lo + i, col lo + j) of D (i >= j): win[slot(j)][i - j];
    // element (row lo + B + i, col lo + j) of W:     win[slot(j)][B + i - j]
    // ---- p = tau D v, y = tau W v (4 lanes per row, interleaved columns) ---------------------
    {
      // all 48 LDS reads first, then the sums: left to itself the compiler emits read -> wait -> FMA
      // 32 times in a row (measured 1.37 us for this phase, which is on the inter-workgroup cycle)
      double ap = 0.0, ay = 0.0;
      const int sl_i = ((lo + i4) & (B - 1)) * LDC;
      double vj[NJ], dij[NJ], wij[NJ];
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) {
        const int j = qq + PARTS * jj;
        const int sl_j = ((lo + j) & (B - 1)) * LDC;
        const bool stale = entering && j == B - 1;   // the slot of the entering column still holds the column that left
        vj[jj] = sv[j];
        dij[jj] = (stale && i4 == B - 1) ? 0.0 : win[(i4 >= j) ? sl_j + (i4 - j) : sl_i + (j - i4)];
        wij[jj] = stale ? 0.0 : win[sl_j + (B + i4 - j)];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) {
        ap += dij[jj] * vj[jj];
        ay += wij[jj] * vj[jj];
      }
      ap = part_sum(ap);
      ay = part_sum(ay);
      if (qq == 0) { sp[i4] = ap * tau; sy[i4] = ay * tau; }
    }
    BC_TICK(1)   // partial products
    if (entering && tid >= 128 && tid < 256) {
      const int d = tid - 128;   // 0 .. 127
      double v = 0.0;
      if (need_col && d <= B && !rb_recv(cbox, d, rb_key(s), err, &v)) s_fail = 1;
      win[sl_new + d] = v;
    }
    __syncthreads();
    BC_TICK(2)   // wait for the entering column
    if (s_fail) return;   // uniform
    // ---- wave 0: new reflector from x = (W H)[:, 0]; wave 1: q = p - (tau/2 p'v) v ------------
    // (both first add the entering column's term to their row of y / p)
    // Outbound straight from the wave that produced it, before the barrier: (v_n, tau_n) down and the head of
    // W's first column up from wave 0, the updated first column D[:, 0] - v q_0 - q v_0 up from wave 1. The
    // neighbours start while this workgroup still updates its window (off the inter-workgroup critical path).
    const bool has_below = (lo + B <= n - 1);
    double* obox = mail + (int64_t)(t + 1) * 2 * RB_BOX;
    double* upbox = mail + (int64_t)(t - 1) * 2 * RB_BOX + RB_BOX;   // (t > 0)
    if (tid < 64) {
      double yi = sy[tid];
      if (entering) {
        yi = fma(tau * sv[B - 1], win[sl_new + 1 + tid], yi);
        sy[tid] = yi;
      }
      const double x = win[(lo & (B - 1)) * LDC + (B + tid)] - yi * sv[0];
      double ss = (tid >= 1) ? x * x : 0.0;
      ss = wave_sum(ss);
      const double alpha = lane_value(x, 0);
      double beta, tt, sc;
      if (ss == 0.0) { beta = alpha; tt = 0.0; sc = 0.0; }
      else {
        beta = -copysign(hh_norm(alpha, ss), alpha);
        tt = (beta - alpha) / beta;
        sc = 1.0 / (alpha - beta);
      }
      const double vnew = (tid == 0) ? 1.0 : x * sc;
      if (has_below) {
        rb_send(obox, tid, vnew, key);
        if (tid == 0) rb_send(obox, B, tt, key);
      }
      if (tid == 0) {
        if (t == 0) xcol[B] = beta;
        else rb_send(upbox, B, beta, key);
        s_sc[1] = tt;
        s_sc[2] = beta;
      }
      svn[tid] = vnew;
      if (has_below) {
        VV[(soff[s] + t + 1) * B + tid] = vnew;
        if (tid == 0) TT[soff[s] + t + 1] = tt;
      }
    } else if (tid < 128) {
      const int i = tid - 64;
      double pi = sp[i];
      if (entering && i == B - 1) pi = fma(tau * sv[B - 1], win[sl_new], pi);
      const double vi = sv[i];
      const double kk = 0.5 * tau * wave_sum(pi * vi);
      const double qi = pi - kk * vi;
      // updated first column: D[i][0] - v_i q_0 - q_i v_0
      const double cu = win[(lo & (B - 1)) * LDC + i] - (vi * lane_value(qi, 0) + qi * lane_value(vi, 0));
      if (t == 0) xcol[i] = cu;
      else rb_send(upbox, i, cu, key);
      sq[i] = qi;
    }
    __syncthreads();
    BC_TICK(3)   // reflector generation / q / sends
    const double taun = s_sc[1];
    // ---- u = v_n' W (4 lanes per column) -----------------------------------------------------------
    {
      double au = 0.0;
      const int sl_j = ((lo + i4) & (B - 1)) * LDC + B - i4;   // i4 plays the column index here
      double vn[NJ], wc[NJ];                                   // (reads first, see above)
#pragma unroll
      for (int ii = 0; ii < NJ; ++ii) {
        const int i = qq + PARTS * ii;
        vn[ii] = svn[i];
        wc[ii] = win[sl_j + i];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ii = 0; ii < NJ; ++ii) au += vn[ii] * wc[ii];
      au = part_sum(au);
      if (qq == 0) su[i4] = au;
    }
    __syncthreads();
    if (tid < 64) {
      const double cc = wave_sum(svn[tid] * sy[tid]);
      sz[tid] = taun * (su[tid] - cc * sv[tid]);
    }
    __syncthreads();
    // ---- in-place update ------------------------------------------------------------------------
    // (the kernel is bound by the number of LDS instructions a CU can issue, not by LDS bandwidth:
    //  v_j, q_j, z_j of the wave-uniform column j come from the lane that already holds them in a
    //  register (readlane) instead of three broadcast LDS reads per column)
    {
      const int i = tid & 63;
      const int jq = __builtin_amdgcn_readfirstlane(tid >> 6);
      const double vi = sv[i], qi = sq[i], yi = sy[i], vni = svn[i], zi = sz[i];
      // all reads of the window before the first write (the compiler cannot prove that the columns
      // do not alias and would otherwise wait for every store before the next load)
      double wv[NJ], dv[NJ];
      const double beta_n = s_sc[2];
#pragma unroll
      for (int q = 0; q < NJ; ++q) {
        const int j = jq + PARTS * q;
        const double* col = win + ((lo + j) & (B - 1)) * LDC;
        wv[q] = col[B + i - j];
        dv[q] = (i >= j) ? col[i - j] : 0.0;
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < NJ; ++q) {
        const int j = jq + PARTS * q;
        const double svj = lane_value(vi, j), sqj = lane_value(qi, j), szj = lane_value(zi, j);
        double* col = win + ((lo + j) & (B - 1)) * LDC;
        double w = wv[q] - yi * svj - vni * szj;
        if (j == 0) w = (i == 0) ? beta_n : 0.0;
        col[B + i - j] = w;
        if (i >= j) col[i - j] = dv[q] - (vi * sqj + qi * svj);
      }
    }
    BC_TICK(4)   // u, z, update
    __syncthreads();   // the window slot / xcol / svn are reused by the next sweep
    if (s == n / 2) { BC_TICK(5) }   // (count marker: unused)
  }
  // ---- location 0: the last two diagonal entries and the last off-diagonal ------------------------
  if (t == 0 && tid == 0) {
    // after sweep n-3 the leaving column is n-2 (kept in xcol); column n-1 is still in the window
    dvec[n - 2] = xcol[0];
    evec[n - 2] = xcol[1];
    dvec[n - 1] = win[((n - 1) & (B - 1)) * LDC];
    evec[n - 1] = 0.0;
  }
}

// The same self-validating words as ONE 16-byte transaction per lane (value, value ^ key side by side): one store and
// one load instruction per word pair instead of two, full 128-byte lines per wave store. The pair is still validated
// word against word, so nothing depends on the 16 bytes arriving together.
__device__ __forceinline__ void rb_send16(double* box, int i, double v, unsigned long long key) {
  const unsigned long long a = (unsigned long long)__double_as_longlong(v);
  pqc_st16(box + 2 * i, v, __longlong_as_double((long long)(a ^ key)));
}
__device__ __forceinline__ bool rb_recv16(const double* box, int i, unsigned long long key, int* err, double* out) {
  const double* q = box + 2 * i;
  long spins = 0;
  for (;;) {
    bk_d2 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(q) : "memory");
    const unsigned long long a = (unsigned long long)__double_as_longlong(v.x);
    const unsigned long long b = (unsigned long long)__double_as_longlong(v.y);
    if ((a ^ b) == key) {
      *out = v.x;
      return true;
    }
    if ((++spins & 255) == 0 &&
        (spins > BC_SPIN_LIMIT || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
      __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
  }
}

// ---------------------------------------------------------------------------
// bc_regwin: the same location-resident bulge chasing with the band window in REGISTERS.
//
// bc_resident keeps the 64 x 128 window in LDS and every phase of a sweep is a round of LDS reads and of the index
// arithmetic of its circular buffer. Here thread (lane l, wave w) of the 512-thread workgroup holds, for each of the
// wave's eight column slots sigma = 8w + q (column c lives in slot c mod 64 for as long as it is in the window), two
// elements of column c:
//     d[q] = A[rho, c]        rho = the row of [lo, lo + 64) congruent to l (mod 64)   -- row l' = (l - lo) mod 64 of D,
//     w[q] = A[rho + 64, c]                                                             -- row l' of W,
// lo the first column of the window; both triangles of the symmetric diagonal block D are kept. When the window slides
// by one, exactly one lane changes its rows (its D row leaves, its W row becomes the new last row of D, a zero row
// enters W): d <- w, w <- 0 in that lane; the slot of the column that left is refilled -- w and the diagonal from the
// column that location t+1 sends up, the rest of d from the new last row of D, transposed through LDS. No other data
// moves and no access needs a select.
// Per sweep: y = tau W v and p = tau D v are 16 multiply-adds per thread (v_j of the wave's eight consecutive columns
// by broadcast LDS reads) + one cross-wave reduction through LDS; u = v_n' W is a column sum, i.e. a lane reduction
// inside the owning wave (a butterfly over 8 values: DPP for lane distances 1, 2, 4, 8, ds_bpermute for 16, 32), so z
// needs no exchange at all; the rank-2 updates are four multiply-adds per element on registers. Four barriers per
// sweep instead of seven. The messages, their keys and the reflector store are exactly bc_resident's.
// ---------------------------------------------------------------------------
template <int CTRL, int BANK>
__device__ __forceinline__ double dpp_into(double v, double old) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, 0xF, BANK, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, 0xF, BANK, false);
  return __hiloint2double(hi, lo);
}
// value of lane (l ^ 4): lanes with bit 2 clear read l + 4 (row_shl:4, banks 0 and 2), the others l - 4
__device__ __forceinline__ double lane_xor4(double v) {
  return dpp_into<0x114, 0xA>(v, dpp_into<0x104, 0x5>(v, v));
}
__device__ __forceinline__ double lane_xor_far(double v, int lane_x) {   // lane_x = l ^ 16 or l ^ 32
  const int lo = __builtin_amdgcn_ds_bpermute(lane_x << 2, __double2loint(v));
  const int hi = __builtin_amdgcn_ds_bpermute(lane_x << 2, __double2hiint(v));
  return __hiloint2double(hi, lo);
}
// a[q], q = 0..7: returns, in every lane whose low bits are (b0, b1, b2) with q = 4 b0 + 2 b1 + b2, the sum of a[q]
// over the 64 lanes (reduce-scatter over lane distances 1, 2, 4, then all-reduce over 8, 16, 32)
__device__ __forceinline__ double colsum8(const double (&a)[8], int lane) {
  const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
  double k4[4], k2[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double keep = b0 ? a[k + 4] : a[k], give = b0 ? a[k] : a[k + 4];
    k4[k] = keep + dpp_move<0xB1>(give);
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double keep = b1 ? k4[k + 2] : k4[k], give = b1 ? k4[k] : k4[k + 2];
    k2[k] = keep + dpp_move<0x4E>(give);
  }
  const double keep = b2 ? k2[1] : k2[0], give = b2 ? k2[0] : k2[1];
  double v = keep + lane_xor4(give);
  v += dpp_move<0x128>(v);             // row_ror:8 = lane ^ 8
  v += lane_xor_far(v, lane ^ 16);
  v += lane_xor_far(v, lane ^ 32);
  return v;
}
__host__ __device__ constexpr int colsum8_lane(int q) { return (q >> 2) | (((q >> 1) & 1) << 1) | ((q & 1) << 2); }

// (-DBK_BC_MSG16: one 16-byte transaction per word pair instead of two 8-byte ones -- measured: no difference,
//  62.9-63.2 vs 61.6-63.3 ms at N = 20 000: the hop does not depend on the number of memory instructions)
#ifdef BK_BC_MSG16
#define RB_SEND rb_send16
#define RB_RECV rb_recv16
#else
#define RB_SEND rb_send
#define RB_RECV rb_recv
#endif
__global__ __launch_bounds__(512, 4) void bc_regwin(const double* __restrict__ AB, int n,
                                                    const int64_t* __restrict__ soff,
                                                    double* __restrict__ VV, double* __restrict__ TT,
                                                    double* __restrict__ dvec, double* __restrict__ evec,
                                                    double* __restrict__ mail, int* __restrict__ err) {
  constexpr int B = S2_B;
  // vectors indexed by the row / column relative to the window; sv2, sq2 twice in a row so that the eight consecutive
  // (mod 64) entries a wave needs are one run
  __shared__ __attribute__((aligned(16))) double sv2[2 * B], sq2[2 * B];
  __shared__ double svn[B], sy[B];
  __shared__ double redP[8][B], redY[8][B];               // the waves' partial products
  __shared__ double col0D[B], col0W[B];                   // first column of the window before the sweep's update
  __shared__ double rowbuf[B];                            // last row of D for the slot that is refilled
  __shared__ double colbuf[2 * B];                        // the entering column, offsets 0 .. 64 from its diagonal
  __shared__ double xcol[B + 1];                          // location 0: the column that left (next one to annihilate)
  __shared__ double s_sc[4];                              // tau, tau_n, beta_n
  __shared__ int s_fail;
  const int t = blockIdx.x, tid = threadIdx.x;
  const int ln = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  // Mailboxes of location t: the reflector from location t-1, and TWO boxes for the column from location t+1, used
  // in turn by sweep parity: the two waves that consume the column read their words independently, and the reflector
  // this location sends on as soon as ONE of them is done lets location t+1 produce the next column -- which must
  // not land on words the other wave has yet to read.
  double* vbox = mail + (int64_t)t * 3 * RB_BOX;
  if (tid == 0) s_fail = 0;
  if (tid <= B) xcol[tid] = 0.0;
  double d[8], w[8];
  // ---- initial window: columns 1 + tB .. tB + 64 of the band (stored by sub-diagonal offset 0 .. 64) ------------------
  {
    const int lo0 = 1 + t * B;
    const int lp0 = (ln - lo0) & 63;
    const int row = lo0 + lp0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int sig = 8 * wv + q;
      const int j = (sig - lo0) & 63, c = lo0 + j;
      double dv = 0.0, wv_ = 0.0;
      if (c < n && row < n)
        dv = (lp0 >= j) ? AB[(lp0 - j) + (int64_t)c * S2_LD] : AB[(j - lp0) + (int64_t)row * S2_LD];
      if (c < n && lp0 <= j && row + B < n) wv_ = AB[(B + lp0 - j) + (int64_t)c * S2_LD];
      d[q] = dv;
      w[q] = wv_;
    }
    if (t == 0 && tid <= B && tid < n) xcol[tid] = AB[tid];   // column 0: head + the rows to annihilate
    if (wv == ((lo0 & 63) >> 3)) {
      switch (lo0 & 7) {
#define BK_RW_EXPORT0(Q) case Q: col0D[lp0] = d[Q]; col0W[lp0] = w[Q]; break;
        BK_RW_EXPORT0(0) BK_RW_EXPORT0(1) BK_RW_EXPORT0(2) BK_RW_EXPORT0(3)
        BK_RW_EXPORT0(4) BK_RW_EXPORT0(5) BK_RW_EXPORT0(6) BK_RW_EXPORT0(7)
#undef BK_RW_EXPORT0
      }
    }
  }
  __syncthreads();
#ifdef BK_BC_PROF
  const bool bc_prof_on = (t == (int)gridDim.x / 3) && tid == 128;   // a thread that takes part in every phase
  long long bc_prof_t = clock64();
  // traced locations (tools/bc_trace.py): 0, 1, 2, 3 and two in the middle
  const int bc_tr_loc = (t < 4) ? t : ((t == (int)gridDim.x / 3) ? 4 : ((t == (int)gridDim.x / 3 + 1) ? 5 : -1));
#endif
  for (int s = 0; s <= n - 3; ++s) {
    const int lo = s + 1 + t * B;
    if (lo > n - 1) break;
    BC_TICK(7)   // loop overhead / end-of-sweep barrier
    BC_TRACE(0, tid == 0)                       // top of the sweep
    const int base = lo & 63;                       // slot of the window's first column
    const int lp = (ln - base) & 63;                // this lane's row relative to the window
    const int j0 = (8 * wv - base) & 63;            // relative column of the wave's first slot (the others follow, mod 64)
    const bool entering = (s > 0);                  // (zeros enter once the window has reached the end of the matrix)
    const int cnew = lo + B - 1;
    const bool need_col = entering && (cnew <= n - 1);
    const int snew = (base + 63) & 63;              // slot that is refilled at this sweep
    const unsigned long long key = rb_key(s + 1);
    const double* cbox = vbox + RB_BOX * (1 + (s & 1));   // inbound: the column location t+1 sent during its sweep s-1
    // the refilled slot: zero but for the new last row of D, transposed at the end of the previous sweep
    if (entering && wv == (snew >> 3)) {
      const double rb = (lp < B - 1) ? rowbuf[lp] : 0.0;
      switch (snew & 7) {
#define BK_RW_REFILL(Q) case Q: d[Q] = rb; w[Q] = 0.0; break;
        BK_RW_REFILL(0) BK_RW_REFILL(1) BK_RW_REFILL(2) BK_RW_REFILL(3)
        BK_RW_REFILL(4) BK_RW_REFILL(5) BK_RW_REFILL(6) BK_RW_REFILL(7)
#undef BK_RW_REFILL
      }
    }
    // ---- inbound reflector ---------------------------------------------------------------------------------------
    if (t == 0) {
      if (tid < 64) {
        const double x = xcol[1 + tid];
        double ss = (tid >= 1) ? x * x : 0.0;
        ss = wave_sum(ss);
        const double alpha = lane_value(x, 0);
        double beta, tt, sc;
        if (ss == 0.0) { beta = alpha; tt = 0.0; sc = 0.0; }
        else {
          beta = -copysign(hh_norm(alpha, ss), alpha);
          tt = (beta - alpha) / beta;
          sc = 1.0 / (alpha - beta);
        }
        const double v = (tid == 0) ? 1.0 : x * sc;
        sv2[tid] = v;
        sv2[tid + B] = v;
        const int64_t ridx = soff[s];
        VV[ridx * B + tid] = v;
        if (tid == 0) { s_sc[0] = tt; TT[ridx] = tt; dvec[s] = xcol[0]; evec[s] = beta; }
      }
    } else if (tid <= B) {
      double v = 0.0;
      if (!RB_RECV(vbox, tid, key, err, &v)) s_fail = 1;
#ifdef BK_BC_PROF
      if (tid == 0 && t == (int)gridDim.x / 3)     // slot 6: send -> receipt of the reflector, in 10-ns ticks
        bc_prof_acc[6] += (long long)(wall_clock64() - __hip_atomic_load(&bc_prof_stamp[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#endif
      if (tid < B) { sv2[tid] = v; sv2[tid + B] = v; }
      else s_sc[0] = v;
    }
    BC_TRACE(1, tid == 0)                       // reflector in (wave 0 has its words / has generated it)
    __syncthreads();
    BC_TICK(0)   // wait for the reflector
    BC_TRACE(2, tid == 0)                       // behind the barrier
    if (s_fail) return;   // uniform
    const double tau = s_sc[0];
    const double vi = sv2[lp];
    double vj[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) vj[q] = sv2[j0 + q];         // wave-uniform addresses: broadcast reads
    // ---- partial products over the wave's eight columns --------------------------------------------------------------
    {
      double ap = 0.0, ay = 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        ap = fma(d[q], vj[q], ap);
        ay = fma(w[q], vj[q], ay);
      }
      redP[wv][lp] = ap;
      redY[wv][lp] = ay;
    }
    BC_TICK(1)   // partial products
    __syncthreads();
    BC_TICK(2)   // barrier after the partial products
    BC_TRACE(3, tid == 0)                       // partial products done (behind the barrier)
    // ---- wave 0: y and the new reflector; wave 1: p, q and the column that goes up. Everything that does not need the
    //      entering column is done BEFORE its words are awaited (the sums over the waves' partials, x0 = W[:,0] - y0 v_0,
    //      p0'v): the column is the last thing to arrive on the cycle that sets the rate of the stage -- location t cannot
    //      send its reflector before location t+1 has answered the previous sweep --, so what follows its arrival is kept
    //      to one multiply-add per row, the norm and the divisions (wave 0) / a few scalar operations (wave 1). The two
    //      waves await their words of the message themselves, straight into registers: no barrier after the arrival.
    const bool has_below = (lo + B <= n - 1);
    double* obox = mail + (int64_t)(t + 1) * 3 * RB_BOX;
    double* upbox = mail + (int64_t)(t - 1) * 3 * RB_BOX + RB_BOX * (1 + ((s + 1) & 1));   // (t > 0) read at sweep s+1
    if (tid < 64) {
      const int i = tid;
      double yi = ((redY[0][i] + redY[1][i]) + (redY[2][i] + redY[3][i])) +
                  ((redY[4][i] + redY[5][i]) + (redY[6][i] + redY[7][i]));
      yi *= tau;
      const double v0 = sv2[0];
      double x = col0W[i] - yi * v0;
      if (entering) {
        double ce = 0.0;                                            // entry 1 + i of the entering column: W[i, 63]
        BC_TRACE(4, tid == 0)                     // wave 0 starts to await the column
        if (need_col && !RB_RECV(cbox, 1 + i, rb_key(s), err, &ce)) s_fail = 1;
        BC_TRACE(5, tid == 0)                     // column in
#ifdef BK_BC_PROF
        if (i == 0 && t == (int)gridDim.x / 3)     // (no free slot: the column's flight time goes to a second counter)
          bc_prof_stamp[3] += wall_clock64() - __hip_atomic_load(&bc_prof_stamp[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
        colbuf[1 + i] = ce;
        const double e = tau * sv2[B - 1] * ce;
        yi += e;
        x = fma(-e, v0, x);
      }
      sy[i] = yi;
      double ss = (i >= 1) ? x * x : 0.0;
      ss = wave_sum(ss);
      const double alpha = lane_value(x, 0);
      double beta, tt, sc;
      if (ss == 0.0) { beta = alpha; tt = 0.0; sc = 0.0; }
      else {
        beta = -copysign(hh_norm(alpha, ss), alpha);
        tt = (beta - alpha) / beta;
        sc = 1.0 / (alpha - beta);
      }
      const double vnew = (i == 0) ? 1.0 : x * sc;
      BC_TRACE(6, tid == 0)                       // new reflector ready: sends follow
#ifdef BK_BC_PROF
      if (i == 0 && t + 1 == (int)gridDim.x / 3)
        __hip_atomic_store(&bc_prof_stamp[0], wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
      if (has_below) {
        RB_SEND(obox, i, vnew, key);
        if (i == 0) RB_SEND(obox, B, tt, key);
      }
      if (i == 0) {
        if (t == 0) xcol[B] = beta;
        else RB_SEND(upbox, B, beta, key);
        s_sc[1] = tt;
        s_sc[2] = beta;
      }
      svn[i] = vnew;
      if (has_below) {
        VV[(soff[s] + t + 1) * B + i] = vnew;
        if (i == 0) TT[soff[s] + t + 1] = tt;
      }
    } else if (tid < 128) {
      const int i = tid - 64;
      double pi = ((redP[0][i] + redP[1][i]) + (redP[2][i] + redP[3][i])) +
                  ((redP[4][i] + redP[5][i]) + (redP[6][i] + redP[7][i]));
      pi *= tau;
      const double vv = sv2[i];
      const double v0 = lane_value(vv, 0), v63 = lane_value(vv, B - 1);
      double pv = wave_sum(pi * vv);                                // p0'v: all of it but the entering column's term
      const double c0d = col0D[i];
      if (entering) {
        double ce = 0.0;                                            // entry 0: the diagonal D[63, 63]
        if (i == 0 && need_col && !RB_RECV(cbox, 0, rb_key(s), err, &ce)) s_fail = 1;
        ce = lane_value(ce, 0);
        if (i == 0) colbuf[0] = ce;
        const double e = tau * v63 * ce;                            // p_63 += e
        if (i == B - 1) pi += e;
        pv = fma(e, v63, pv);
      }
      const double kk = 0.5 * tau * pv;
      const double qi = pi - kk * vv;
      const double cu = c0d - (vv * lane_value(qi, 0) + qi * v0);
      BC_TRACE(7, tid == 64)                      // column for location t-1 ready: sends follow
#ifdef BK_BC_PROF
      if (i == 0 && t - 1 == (int)gridDim.x / 3)
        __hip_atomic_store(&bc_prof_stamp[1], wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
      if (t == 0) xcol[i] = cu;
      else RB_SEND(upbox, i, cu, key);
      sq2[i] = qi;
      sq2[i + B] = qi;
    }
    __syncthreads();
    if (s_fail) return;   // uniform
    // the entering column into the registers of the slot's wave: its diagonal and the block below it
    if (entering && wv == (snew >> 3)) {
      const double c0v = colbuf[0], cw = colbuf[lp + 1];
      switch (snew & 7) {
#define BK_RW_ENTER(Q) case Q: d[Q] = (lp == B - 1) ? c0v : d[Q]; w[Q] = cw; break;
        BK_RW_ENTER(0) BK_RW_ENTER(1) BK_RW_ENTER(2) BK_RW_ENTER(3)
        BK_RW_ENTER(4) BK_RW_ENTER(5) BK_RW_ENTER(6) BK_RW_ENTER(7)
#undef BK_RW_ENTER
      }
    }
    BC_TICK(3)   // reflector generation / q / sends
    BC_TRACE(8, tid == 0)                       // behind the barrier after the generation
    const double taun = s_sc[1];
    const double qi = sq2[lp], yi = sy[lp], vni = svn[lp];
    // ---- u = v_n' W over the wave's columns (lane reduction), z, and the rank-2 updates --------------------------------
    {
      double a[8], qj[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        a[q] = vni * w[q];
        qj[q] = sq2[j0 + q];
      }
      const double usum = colsum8(a, ln);
      const double cc = wave_sum(vni * yi);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const double zj = taun * (lane_value(usum, colsum8_lane(q)) - cc * vj[q]);
        d[q] = fma(-vi, qj[q], fma(-qi, vj[q], d[q]));
        w[q] = fma(-yi, vj[q], fma(-vni, zj, w[q]));
      }
    }
    BC_TICK(4)   // u, z, update
    // ---- the window slides: the lane of relative row 0 takes its W row as the new last row of D, a zero row enters W.
    //      (The first column leaves with the sweep -- its updated entries went up in the message -- and its slot is
    //      refilled at the top of the next sweep; its first-column special case W'[:, 0] = beta e_0 is never read.)
    {
      const bool wraps = (lp == 0);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        d[q] = wraps ? w[q] : d[q];
        w[q] = wraps ? 0.0 : w[q];
      }
      // for the next sweep: the new last row of D (now in the d registers of that lane) for the slot to be refilled,
      // and the new first column
      const int nbase = (base + 1) & 63;
      if (wraps) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int jn = (j0 + q - 1) & 63;                 // column index in the next window (63: the slot that leaves)
          rowbuf[jn] = d[q];                                 // (entry 63 is written and never read)
        }
      }
      if (wv == (nbase >> 3)) {
        const int lpn = (ln - nbase) & 63;
        switch (nbase & 7) {
#define BK_RW_EXPORT(Q) case Q: col0D[lpn] = d[Q]; col0W[lpn] = w[Q]; break;
          BK_RW_EXPORT(0) BK_RW_EXPORT(1) BK_RW_EXPORT(2) BK_RW_EXPORT(3)
          BK_RW_EXPORT(4) BK_RW_EXPORT(5) BK_RW_EXPORT(6) BK_RW_EXPORT(7)
#undef BK_RW_EXPORT
        }
      }
    }
    BC_TICK(5)   // slide, transposition of the new last row, export of the new first column
    BC_TRACE(9, tid == 0)                       // update, slide and exports done
    __syncthreads();   // rowbuf / col0 / xcol / the reduction buffers are reused by the next sweep
  }
  // ---- location 0: the last two diagonal entries and the last off-diagonal ------------------------
  if (t == 0 && tid == 0) {
    // after sweep n-3 the leaving column is n-2 (kept in xcol); column n-1 is the window's first column
    dvec[n - 2] = xcol[0];
    evec[n - 2] = xcol[1];
    dvec[n - 1] = col0D[0];
    evec[n - 1] = 0.0;
  }
}

#undef RB_SEND
#undef RB_RECV
__global__ void s2_extract_de(const double* __restrict__ AB, int n, double* __restrict__ d,
                              double* __restrict__ e) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n) {
    d[c] = AB[(int64_t)c * S2_LD];
    e[c] = (c < n - 1) ? AB[1 + (int64_t)c * S2_LD] : 0.0;
  }
}

// (sweep offsets, arm, grid, mailbox and wavefront ranges: S2Plan of csrc/s2plan.h)
int stage2_to_tridiag(bigkrls_ctx* ctx, const S2Plan& plan, double* AB, const int64_t* d_soff, double* VV, double* TT,
                      double* d, double* e, int* progress, int* err) {
  hipStream_t st = ctx->stream;
  const int b = S2_B, n = plan.n;
  BcArm arm = plan.bc_request;
  const void* resident = arm == BcArm::Regwin ? (const void*)bc_regwin
                                              : arm == BcArm::Lds512 ? (const void*)bc_resident<512> : (const void*)bc_resident<256>;
  const int threads = arm == BcArm::Lds256 ? 256 : 512;
  if (plan.nsweep > 0 && bc_is_resident(arm)) {
    int rcap = 1;
    BK_TRY(resident_capacity(ctx, resident, &rcap, threads));
    arm = plan.bc_arm(rcap);
  }
  if (plan.nsweep > 0 && bc_is_resident(arm)) {
    void* pm = nullptr;
    const int64_t mail_doubles = plan.bc_mail_doubles();
    BK_TRY(ws_get(ctx, SLOT_EIG_Z, mail_doubles * sizeof(double), &pm));
    double* mail = (double*)pm;
    BK_HIP(hipMemsetAsync(mail, 0, (size_t)mail_doubles * sizeof(double), st));   // A ^ B == 0: no valid message
    // algorithmic HBM bytes: the band read once (16 n b) + the stored reflectors (8 b per task)
    BK_TRY(prof_begin(ctx, "bulge_chase", 16.0 * (double)n * b + 8.0 * b * ((double)n * n / (2.0 * b))));
    if (arm == BcArm::Regwin)
      hipLaunchKernelGGL(bc_regwin, dim3(plan.nloc), dim3(512), 0, st, (const double*)AB, n, d_soff, VV, TT, d, e,
                         mail, err);
    else if (arm == BcArm::Lds512)
      hipLaunchKernelGGL(bc_resident<512>, dim3(plan.nloc), dim3(512), 0, st, (const double*)AB, n, d_soff, VV, TT, d, e,
                         mail, err);
    else
      hipLaunchKernelGGL(bc_resident<256>, dim3(plan.nloc), dim3(256), 0, st, (const double*)AB, n, d_soff, VV, TT, d, e,
                         mail, err);
    BK_TRY(prof_end(ctx, "bulge_chase"));
    BK_CHECK_LAUNCH();
    return BIGKRLS_OK;
  }
  if (plan.nsweep > 0 && arm == BcArm::Persistent) {
    int cap = 1;
    BK_TRY(resident_capacity(ctx, (const void*)bc_persistent, &cap));
    BK_HIP(hipMemsetAsync(progress, 0, (size_t)plan.nsweep * sizeof(int), st));
    hipLaunchKernelGGL(bc_persistent, dim3(plan.bc_persistent_grid(cap)), dim3(256), 0, st, AB, n, d_soff, VV, TT, progress,
                       err, plan.nsweep);
    BK_CHECK_LAUNCH();
  } else if (plan.nsweep > 0) {
    for (int64_t w = 0; w <= plan.bc_tmax(); ++w) {
      const S2Range r = plan.bc_wavefront(w);
      if (r.count == 0) continue;
      const bool sample = ctx->profile && (w % 64) == 32;
      if (sample) {
        // algorithmic bytes of this launch: every task reads and writes its len x b off-diagonal
        // block (t > 0) and the lower triangle of its len x len diagonal block
        double bytes = 0.0;
        for (int64_t s = r.lo; s < r.lo + r.count; ++s) {
          const int64_t t = w - 2 * s, lo = s + 1 + t * b;
          const double len = (double)(std::min<int64_t>(s + (t + 1) * b, n - 1) - lo + 1);
          bytes += 16.0 * (len * (len + 1.0) * 0.5 + (t > 0 ? len * b : len));
        }
        BK_TRY(prof_begin(ctx, "bulge_chase", bytes));
      }
      hipLaunchKernelGGL(bc_wavefront, dim3(r.count), dim3(256), 0, st, AB, n, (int)w, (int)r.lo, d_soff, VV, TT);
      if (sample) BK_TRY(prof_end(ctx, "bulge_chase"));
    }
    BK_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(s2_extract_de, dim3((n + 255) / 256), dim3(256), 0, st, (const double*)AB, n, d, e);
  BK_CHECK_LAUNCH();
  return BIGKRLS_OK;
}

// ---------------------------------------------------------------------------
// back-transforms
// ---------------------------------------------------------------------------
// one sweep of Q2: every step t of sweep s acts on its own rows of Z (n x nv, ldz)
__global__ __launch_bounds__(256) void bt2_sweep(double* __restrict__ Z, int64_t ldz, int n, int nv, int s,
                                                 const int64_t* __restrict__ soff,
                                                 const double* __restrict__ VV,
                                                 const double* __restrict__ TT) {
  constexpr int B = S2_B;
  __shared__ double sv[B];
  __shared__ double sp[4][64];
  const int t = blockIdx.x;
  const int lo = s + 1 + t * B;
  const int len = min(B, n - lo);
  const int64_t ridx = soff[s] + t;
  const double tau = TT[ridx];
  if (tau == 0.0) return;
  const int tid = threadIdx.x;
  if (tid < B) sv[tid] = (tid < len) ? VV[ridx * B + tid] : 0.0;
  __syncthreads();
  const int cl = tid & 63, part = tid >> 6;       // 64 columns per block, 4 row parts of 16
  const int col = blockIdx.y * 64 + cl;
  double* z = Z + lo + (int64_t)col * ldz;
  double acc = 0.0;
  double zr[16];
  if (col < nv) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = part * 16 + i;
      zr[i] = (r < len) ? z[r] : 0.0;
      acc += sv[r] * zr[i];
    }
  }
  sp[part][cl] = acc;
  __syncthreads();
  const double dot = tau * ((sp[0][cl] + sp[1][cl]) + (sp[2][cl] + sp[3][cl]));
  if (col < nv) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = part * 16 + i;
      if (r < len) z[r] = zr[i] - dot * sv[r];
    }
  }
}

// Blocked application of Q2. Sweeps are taken in groups of BT2_G (group 0 = the highest
// sweeps, which must be applied first). Task (g, t) applies the reflectors (s, t), s = s_hi
// .. s_lo of its group (descending) to the row window [s_lo+1+t b, s_hi+(t+1)b] of a
// 64-column slab of Z held in LDS, so Z moves through HBM once per GROUP instead of once
// per sweep. Reordering is legal because reflectors with disjoint rows commute:
//   (g,t) needs (g,t-1) and (g-1,t) done; tasks with equal g + t are independent.
static_assert(BT2_G == 32, "the stage-2 back-transform's tasks: 32 sweeps (csrc/s2plan.h)");
__global__ __launch_bounds__(256) void bt2_block(double* __restrict__ Z, int64_t ldz, int n, int nv,
                                                 int wave_idx, int g_min, const int64_t* __restrict__ soff,
                                                 const double* __restrict__ VV,
                                                 const double* __restrict__ TT) {
  constexpr int B = S2_B;
  constexpr int WR = B + BT2_G - 1;  // rows of the window
  // column c of the slab at sZ[c * LDZ + r]; LDZ odd so that the 64 lanes (one per column)
  // of a ds_read_b64 fall on distinct bank pairs (WR + 1 = 96 would be a 32-way conflict)
  constexpr int LDZ = (WR % 2 == 0) ? WR + 1 : WR + 2;
  __shared__ double sZ[64 * LDZ];
  __shared__ double sV[BT2_G * B];   // all reflectors of the task, fetched up front
  __shared__ double stau[BT2_G];
  __shared__ double sp[4][64];
  const int tid = threadIdx.x;
  const int g = g_min + blockIdx.x;
  const int t = wave_idx - g;
  const int s_hi = (n - 3) - g * BT2_G;
  const int s_lo = max(0, s_hi - BT2_G + 1);
  const int r0 = s_lo + 1 + t * B;
  if (r0 > n - 1) return;
  const int r1 = min(n - 1, s_hi + (t + 1) * B);
  const int wr = r1 - r0 + 1;
  const int c0 = blockIdx.y * 64;
  // All global loads of the task are independent and issued up front (fixed trip counts,
  // fully unrolled): 8 reflector slices + 32 window elements per thread.
  const int ln = tid & 63, wv = tid >> 6;
  // reflectors: slot k <-> sweep s_hi - k ; thread -> element ln of slots wv, wv+4, ...
  double vreg[BT2_G / 4];
#pragma unroll
  for (int q = 0; q < BT2_G / 4; ++q) {
    const int k = wv + 4 * q;
    const int s = s_hi - k;
    const int lo = s + 1 + t * B;
    double v = 0.0;
    if (s >= s_lo && lo <= n - 1 && ln < min(B, n - lo)) v = VV[(soff[s] + t) * B + ln];
    vreg[q] = v;
  }
  if (tid < BT2_G) {
    const int s = s_hi - tid;
    const int lo = s + 1 + t * B;
    stau[tid] = (s >= s_lo && lo <= n - 1) ? TT[soff[s] + t] : 0.0;
  }
  // window: lanes run down the rows (coalesced), waves over columns
  double zreg[16][2];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int c = wv + 4 * q;
    const double* zp = Z + (int64_t)r0 + (int64_t)(c0 + c) * ldz;
    const bool cok = (c0 + c) < nv;
    zreg[q][0] = (cok && ln < wr) ? zp[ln] : 0.0;
    zreg[q][1] = (cok && ln + 64 < wr) ? zp[ln + 64] : 0.0;
  }
#pragma unroll
  for (int q = 0; q < BT2_G / 4; ++q) sV[(wv + 4 * q) * B + ln] = vreg[q];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int c = wv + 4 * q;
    sZ[c * LDZ + ln] = zreg[q][0];
    if (ln + 64 < WR) sZ[c * LDZ + ln + 64] = zreg[q][1];  // rows past the window stay zero
  }
  __syncthreads();
  const int cl = tid & 63, part = tid >> 6;
  for (int k = 0; k < BT2_G; ++k) {
    const double tau = stau[k];
    if (tau == 0.0) continue;             // uniform: missing step or H = I
    const int s = s_hi - k;
    const int off = (s + 1 + t * B) - r0;  // first window row this reflector touches
    const double* vk = sV + k * B + part * 16;
    double* zc = sZ + cl * LDZ + off + part * 16;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc += vk[i] * zc[i];
    sp[part][cl] = acc;
    __syncthreads();
    const double dot = tau * ((sp[0][cl] + sp[1][cl]) + (sp[2][cl] + sp[3][cl]));
#pragma unroll
    for (int i = 0; i < 16; ++i) zc[i] -= dot * vk[i];
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int c = wv + 4 * q;
    if (c0 + c < nv) {
      double* zp = Z + (int64_t)r0 + (int64_t)(c0 + c) * ldz;
      if (ln < wr) zp[ln] = sZ[c * LDZ + ln];
      if (ln + 64 < wr) zp[ln + 64] = sZ[c * LDZ + ln + 64];
    }
  }
}

// ---- compact-WY form of a task --------------------------------------------------------------
// The BT2_G reflectors of task (g, t) are applied in the order k = 0 .. G-1, i.e. the task is
//   Z_w <- H_{G-1} ... H_0 Z_w = (I - V T' V') Z_w,   T = dlarft(forward, columnwise) of (v_0 .. v_{G-1}),
// with V the 95 x 32 parallelogram of the reflectors in window rows. T depends only on the
// reflectors, so all tasks' T factors are built in ONE launch (bt2_build_t) as soon as the bulge
// chasing has finished; the dependent chain of 32 reflector steps per task (2 barriers each)
// then becomes three small MFMA products per task (bt2_wy).
constexpr int BT2_LDW = BT2_G + S2_B + 2;   // 98: LDS stride of window columns / reflector rows, = 2 mod 32
typedef double d4 __attribute__((ext_vector_type(4)));

// (slot of task (g, t)'s T factor, toff[g] + t: S2Plan::toff of csrc/s2plan.h)
// One WAVE per task (round 6; it was one workgroup per task, whose 32-step recurrence ran on at most 32 of its 256
// threads between two workgroup barriers per step: 6 ms at N = 20 000 for 97 000 tasks, on the stream that shares the GPU
// with the divide & conquer). The Gram products V_k' V_j of the task's 32 reflectors (length 64, shifted by one window
// row per reflector: a 32 x 96 operand) go to the f64 MFMA units -- three 16 x 16 tiles, the upper triangle --; row r of
// T then depends on the Gram matrix and on row r alone, T(r, i) = -tau_i sum_{m < i} T(r, m) G(m, i), so 32 lanes keep
// one row each in registers and run the recurrence without any exchange. No workgroup barrier anywhere: the four waves
// of a workgroup work on four tasks independently (a wave's LDS accesses are ordered among themselves).
constexpr size_t BT2T_SMEM = (size_t)4 * (BT2_G * BT2_LDW + BT2_G * (BT2_G + 1)) * sizeof(double);
__global__ __launch_bounds__(256) void bt2_build_t(int n, const int64_t* __restrict__ soff,
                                                   const double* __restrict__ VV,
                                                   const double* __restrict__ TT,
                                                   const int64_t* __restrict__ toff,
                                                   double* __restrict__ Tst, int ntmax, int ngroups) {
  constexpr int B = S2_B, G = BT2_G, LDW = BT2_LDW, LDG = BT2_G + 1;
  static_assert(G == 32 && B == 64, "bt2_build_t: two 16-row tiles of reflectors, one wave per reflector");
  extern __shared__ __attribute__((aligned(16))) double bt2t_smem[];
  const int tid = threadIdx.x, ln = tid & 63, wv = tid >> 6;
  double* sV = bt2t_smem + (size_t)wv * (G * LDW + G * LDG);     // reflector k in window rows: sV[k * LDW + r]
  double* sG = sV + G * LDW;                                      // sG[k * LDG + j] = v_k' v_j, k < j
  const int64_t task = (int64_t)blockIdx.x * 4 + wv;
  if (task >= (int64_t)ntmax * ngroups) return;                   // (whole waves leave; nothing below spans waves)
  const int g = (int)(task / ntmax), t = (int)(task % ntmax);
  const int s_hi = (n - 3) - g * G;
  const int s_lo = max(0, s_hi - G + 1);
  const int r0 = s_lo + 1 + t * B;
  if (r0 > n - 1) return;
  auto wave_sync = [] {         // the wave's earlier LDS writes are visible to all of its lanes
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  };
  for (int e = ln; e < G * LDW; e += 64) sV[e] = 0.0;
  wave_sync();
  double tau = 0.0;             // lane k < G: tau of reflector k
#pragma unroll 4
  for (int k = 0; k < G; ++k) {
    const int s = s_hi - k;
    const int lo = s + 1 + t * B;
    if (s >= s_lo && lo <= n - 1) {                               // (uniform)
      if (ln < min(B, n - lo)) sV[k * LDW + (lo - r0) + ln] = VV[(soff[s] + t) * B + ln];
      if (ln == k) tau = TT[soff[s] + t];
    }
  }
  wave_sync();
  // ---- Gram matrix, upper tiles (a, b) = (0,0), (0,1), (1,1): lane (lm, lk) ends up with G[16 a + lm][16 b + lk + 4 q] --
  {
    typedef double bt2_d4 __attribute__((ext_vector_type(4)));
    const int lm = ln & 15, lk = ln >> 4;
    bt2_d4 acc00 = {0.0, 0.0, 0.0, 0.0}, acc01 = acc00, acc11 = acc00;
#pragma unroll 4
    for (int kk = 0; kk < B + G; kk += 4) {
      const double v0 = sV[lm * LDW + kk + lk];                   // reflector lm, window row kk + lk
      const double v1 = sV[(16 + lm) * LDW + kk + lk];            // reflector 16 + lm
      acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(v0, v0, acc00, 0, 0, 0);
      acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(v1, v0, acc01, 0, 0, 0);
      acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(v1, v1, acc11, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sG[lm * LDG + lk + 4 * q] = acc00[q];
      sG[lm * LDG + 16 + lk + 4 * q] = acc01[q];
      sG[(16 + lm) * LDG + 16 + lk + 4 * q] = acc11[q];
    }
  }
  wave_sync();
  // ---- row ln of T: T(ln, ln) = tau_ln, T(ln, i) = -tau_i sum_{m < i} T(ln, m) G(m, i) for i > ln (T(ln, m) = 0 for m < ln) ----
  double Trow[G];
#pragma unroll
  for (int i = 0; i < G; ++i) Trow[i] = 0.0;
#pragma unroll
  for (int i = 0; i < G; ++i) {
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int m = 0; m < i; ++m) {
      const double gmi = sG[m * LDG + i];                         // (uniform address: a broadcast read)
      if (m & 1) a1 = fma(Trow[m], gmi, a1);
      else a0 = fma(Trow[m], gmi, a0);
    }
    const double ti = lane_value(tau, i);
    Trow[i] = (ln < i) ? -ti * (a0 + a1) : ((ln == i) ? ti : 0.0);
  }
  if (ln < G) {
    double* To = Tst + (toff[g] + t) * (int64_t)(G * G) + (int64_t)ln * G;   // row-major T[l][i]
#pragma unroll
    for (int i = 0; i < G; ++i) To[i] = Trow[i];
  }
}

// Task (g, t) on a 64-column slab: W = V' Z_w, W2 = T' W, Z_w -= V W2 on the f64 MFMA units. Every
// wave owns 16 columns of the slab through all three products (the accumulator layout of one
// product is the B-operand layout of the next when the k index runs over lane/16 + 4q).
// COH (the persistent kernel): the window travels between workgroups -- possibly on different XCDs, whose L2s are not
// coherent with each other for ordinary accesses -- inside ONE launch, so it is read and written with agent-scope
// accesses (sc1 loads, write-through stores), like the band of bc_persistent.
// `ready()` is called (by all threads, uniformly) after the loads that do not depend on other tasks -- the reflectors
// and the T factor -- have been issued and before the first access to Z: the persistent kernel waits for the task's
// predecessors there; it returns false to abandon the task.
template <bool COH, class Ready>
__device__ __forceinline__ bool bt2_wy_task(double* __restrict__ Z, int64_t ldz, int n, int nv, int g, int t,
                                            int c0, const int64_t* __restrict__ soff,
                                            const double* __restrict__ VV,
                                            const int64_t* __restrict__ toff,
                                            const double* __restrict__ Tst, double* smem_wy, Ready ready) {
  constexpr int B = S2_B, G = BT2_G;
  constexpr int LD = BT2_LDW;
  double* sZ = smem_wy;             // sZ[c * LD + r]: window rows r < 96 of slab column c
  double* sV = smem_wy + 64 * LD;   // sV[k * LD + r]: reflector k in window rows
  const int tid = threadIdx.x;
  const int s_hi = (n - 3) - g * G;
  const int s_lo = max(0, s_hi - G + 1);
  const int r0 = s_lo + 1 + t * B;
  const int r1 = min(n - 1, s_hi + (t + 1) * B);
  const int wr = r1 - r0 + 1;
  const int ln = tid & 63, wv = tid >> 6;
  // global loads first: reflector slices, T entries of this lane, window
  double vreg[G / 4];
  int voff[G / 4];
#pragma unroll
  for (int q = 0; q < G / 4; ++q) {
    const int k = wv + 4 * q;
    const int s = s_hi - k;
    const int lo = s + 1 + t * B;
    double v = 0.0;
    if (s >= s_lo && lo <= n - 1 && ln < min(B, n - lo)) v = VV[(soff[s] + t) * B + ln];
    vreg[q] = v;
    voff[q] = (s >= s_lo) ? (s - s_lo) : 0;     // first window row of reflector k
  }
  const int l16 = ln & 15, lg = ln >> 4;
  const double* Tg = Tst + (toff[g] + t) * (int64_t)(G * G);
  double treg[2][4][2];   // T[kt*16 + lg + 4q][it*16 + l16]
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int it = 0; it < 2; ++it) treg[kt][q][it] = Tg[(kt * 16 + lg + 4 * q) * G + it * 16 + l16];
  if (!ready()) return false;
  double zreg[16][2];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int c = wv + 4 * q;
    const double* zp = Z + (int64_t)r0 + (int64_t)(c0 + c) * ldz;
    const bool cok = (c0 + c) < nv;
    zreg[q][0] = (cok && ln < wr) ? band_ld<COH>(zp + ln) : 0.0;
    zreg[q][1] = (cok && ln + 64 < wr) ? band_ld<COH>(zp + ln + 64) : 0.0;
  }
  // zero the reflector array (each reflector covers 64 of the 96 rows), then place the slices
  for (int e = tid; e < G * LD; e += 256) sV[e] = 0.0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < G / 4; ++q) sV[(wv + 4 * q) * LD + voff[q] + ln] = vreg[q];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int c = wv + 4 * q;
    sZ[c * LD + ln] = zreg[q][0];
    if (ln < 32) sZ[c * LD + ln + 64] = zreg[q][1];   // rows 64..95 (row 95 and rows >= wr are zero)
  }
  __syncthreads();
  const int ct = wv;                       // this wave's 16 columns of the slab
  const double* zc = sZ + (ct * 16 + l16) * LD;
  // ---- W = V' Z_w (32 x 16 per wave): k runs over the 96 window rows ---------------------------
  // (fragment reads of four k-steps are issued together, then their eight MFMAs: left alone the
  //  compiler waits for every read right before the MFMA that uses it)
  d4 w[2] = {(d4){0.0, 0.0, 0.0, 0.0}, (d4){0.0, 0.0, 0.0, 0.0}};
#pragma unroll
  for (int rb = 0; rb < B + G; rb += 16) {
    double zy[4], x0[4], x1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = rb + 4 * u;
      zy[u] = zc[r + lg];
      x0[u] = sV[l16 * LD + r + lg];
      x1[u] = sV[(16 + l16) * LD + r + lg];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      w[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[u], zy[u], w[0], 0, 0, 0);
      w[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[u], zy[u], w[1], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  // ---- W2 = T' W: W2[i][c] = sum_l T[l][i] W[l][c], l = kt*16 + lg + 4q is exactly what w[kt][q] holds
  d4 w2[2] = {(d4){0.0, 0.0, 0.0, 0.0}, (d4){0.0, 0.0, 0.0, 0.0}};
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      w2[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(treg[kt][q][0], w[kt][q], w2[0], 0, 0, 0);
      w2[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(treg[kt][q][1], w[kt][q], w2[1], 0, 0, 0);
    }
  // ---- Z_w -= V W2 (96 x 16 per wave), k runs over the 32 reflectors ---------------------------------
#pragma unroll
  for (int rt = 0; rt < (B + G) / 16; ++rt) {
    double xv[8], zold[4];
    double* zo = sZ + (ct * 16 + l16) * LD + rt * 16 + lg;
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int q = 0; q < 4; ++q) xv[it * 4 + q] = sV[(it * 16 + lg + 4 * q) * LD + rt * 16 + l16];
#pragma unroll
    for (int q = 0; q < 4; ++q) zold[q] = zo[4 * q];
    __builtin_amdgcn_sched_barrier(0);
    d4 u = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int q = 0; q < 4; ++q) u = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[it * 4 + q], w2[it][q], u, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) zo[4 * q] = zold[q] - u[q];
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();
  // window back to HBM: all LDS reads, then all stores
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int c = wv + 4 * q;
    zreg[q][0] = sZ[c * LD + ln];
    zreg[q][1] = (ln < 32) ? sZ[c * LD + ln + 64] : 0.0;
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int c = wv + 4 * q;
    if (c0 + c < nv) {
      double* zp = Z + (int64_t)r0 + (int64_t)(c0 + c) * ldz;
      if (ln < wr) band_st<COH>(zp + ln, zreg[q][0]);
      if (ln + 64 < wr) band_st<COH>(zp + ln + 64, zreg[q][1]);
    }
  }
  return true;
}

// one launch per anti-diagonal g + t = wave_idx (BIGKRLS_BT2=wavefront, and the fallback after a fired watchdog)
__global__ __launch_bounds__(256, 2) void bt2_wy(double* __restrict__ Z, int64_t ldz, int n, int nv,
                                                 int wave_idx, int g_min, const int64_t* __restrict__ soff,
                                                 const double* __restrict__ VV,
                                                 const int64_t* __restrict__ toff,
                                                 const double* __restrict__ Tst) {
  extern __shared__ __attribute__((aligned(16))) double smem_wy[];
  const int g = g_min + blockIdx.x;
  const int t = wave_idx - g;
  const int s_hi = (n - 3) - g * BT2_G;
  const int s_lo = max(0, s_hi - BT2_G + 1);
  if (s_lo + 1 + t * S2_B > n - 1) return;
  bt2_wy_task<false>(Z, ldz, n, nv, g, t, blockIdx.y * 64, soff, VV, toff, Tst, smem_wy, [] { return true; });
}

// ONE launch for the whole stage-2 back-transform. The tasks (g, t, slab) are numbered along the anti-diagonals
// w = g + t (then g, then slab) and handed out in that order by a ticket counter: a workgroup that is running takes
// the next number. A task starts when its two predecessors on the same slab -- (g, t-1) and (g-1, t), both on
// earlier anti-diagonals, i.e. with smaller numbers -- have raised their flags, instead of when the whole previous
// anti-diagonal has drained: 937 dependent launches of ~24 us at N = 20 000 become a chain of 937 tasks with the
// other tasks packed around it. Numbers are only ever held by workgroups that are running, and the holder of the
// lowest unfinished number waits for nothing, so the kernel makes progress with ANY number of resident workgroups:
// it needs no co-residency (two contexts may run it side by side on one GPU, each with part of the CUs) and its
// bounded waits (watchdog -> the caller redoes the decomposition with per-wavefront launches) are a safety net only.
__global__ __launch_bounds__(256, 2) void bt2_persistent(double* __restrict__ Z, int64_t ldz, int n, int nv,
                                                         int ngroups, int ntmax, const int64_t* __restrict__ soff,
                                                         const double* __restrict__ VV,
                                                         const int64_t* __restrict__ toff,
                                                         const double* __restrict__ Tst, int* __restrict__ flags,
                                                         long long ntickets_off, int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) double smem_wy[];
  __shared__ int s_ok;
  __shared__ long long s_ticket;
  constexpr int B = S2_B, G = BT2_G;
  const int nslab = (nv + 63) / 64;
  const int tid = threadIdx.x;
  int w = 0;
  long long woff = 0;                       // first task number of anti-diagonal w
  auto wave_count = [&](int ww) {
    const int g_hi = min(ww, ngroups - 1), g_lo = max(0, ww - (ntmax - 1));
    return (long long)max(0, g_hi - g_lo + 1) * nslab;
  };
  const int nwaves = ngroups + ntmax - 1;
  unsigned long long* ticket = (unsigned long long*)(flags + ntickets_off);
  long long next_k = 0;                     // (thread 0) the next number, requested while the current task runs
  if (tid == 0) next_k = (long long)__hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    if (tid == 0) s_ticket = next_k;
    __syncthreads();
    const long long k = s_ticket;
    __syncthreads();                          // (everybody has read it before thread 0 may write the next one)
    while (w < nwaves && k >= woff + wave_count(w)) { woff += wave_count(w); ++w; }
    if (w >= nwaves) break;
    const int idx = (int)(k - woff);
    const int g = max(0, w - (ntmax - 1)) + idx / nslab, slab = idx % nslab;
    const int t = w - g;
    const int s_hi = (n - 3) - g * G;
    const int s_lo = max(0, s_hi - G + 1);
    if (s_lo + 1 + t * B > n - 1) {                             // no such task (uniform)
      if (tid == 0) next_k = (long long)__hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    // predecessors: (g, t-1) always exists for t > 0; (g-1, t) exists when its first row is inside the matrix
    auto ready = [&]() -> bool {
      if (tid == 0) {
        int ok = 1;
        const int* f1 = (t > 0) ? flags + (toff[g] + t - 1) * nslab + slab : nullptr;
        const int* f2 = nullptr;
        if (g > 0) {
          const int sp_hi = (n - 3) - (g - 1) * G, sp_lo = max(0, sp_hi - G + 1);
          if (sp_lo + 1 + t * B <= n - 1) f2 = flags + (toff[g - 1] + t) * nslab + slab;
        }
        long spins = 0;
        while ((f1 && __hip_atomic_load(f1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) ||
               (f2 && __hip_atomic_load(f2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)) {
          if ((++spins & 255) == 0 &&
              (spins > BC_SPIN_LIMIT || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
            __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = 0;
            break;
          }
        }
        s_ok = ok;
      }
      __syncthreads();
      return s_ok != 0;   // uniform
    };
    if (!bt2_wy_task<true>(Z, ldz, n, nv, g, t, slab * 64, soff, VV, toff, Tst, smem_wy, ready)) return;
    // every thread's window stores device-visible, then one thread raises the flag. The stores are agent-scope
    // write-through stores already: waiting for their completion (vmcnt counts stores on gfx9) is the whole release --
    // a release fence would add a write-back of this XCD's entire L2 (buffer_wbl2) per task.
    // (the next task number is requested here: memory operations return in order, so its round trip would delay
    //  whatever this wave loads after it -- behind the stores it only overlaps with their drain)
    if (tid == 0) next_k = (long long)__hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0)
      __hip_atomic_store(flags + (toff[g] + t) * nslab + slab, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- the stage-2 back-transform as chains along the sweep groups ---------------------------------------------
// The windows of (g, t) and (g + 1, t) share 63 of their 95 rows (the next group's window starts 32 rows higher), and
// nobody else touches those rows in between: a workgroup that walks g -> g + 1 at a fixed location t keeps them in
// LDS, fetches only the 32 rows that enter at the top and writes only the 32 rows that leave at the bottom -- 64
// instead of 190 window rows of agent-scope traffic per task. The window lives in LDS at row (logical + base) mod 96
// with base a multiple of 32, so the shift is a change of `base`; the products run over the logical rows in the same
// order as bt2_wy_task (bit-identical results). A ticket is a SEGMENT of `seg` consecutive groups at one (t, slab),
// handed out in the order in which the segments become runnable (see below): its predecessors -- (g, t-1) for every step, (g-1, t) for its
// first step -- belong to tickets with smaller numbers, so the progress argument of bt2_persistent holds unchanged.
// The per-task flags stay: the chain at t follows the chain at t - 1 one step behind.
__device__ __forceinline__ int bt2_rot(int i, int base) {
  const int x = i + base;
  return x >= 96 ? x - 96 : x;
}

__global__ __launch_bounds__(256, 2) void bt2_chain(double* __restrict__ Z, int64_t ldz, int n, int nv,
                                                    int ngroups, int ntmax, int seg,
                                                    const int64_t* __restrict__ soff,
                                                    const double* __restrict__ VV,
                                                    const int64_t* __restrict__ toff,
                                                    const double* __restrict__ Tst, int* __restrict__ flags,
                                                    long long ntickets_off, int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) double smem_wy[];
  __shared__ int s_ok;
  __shared__ long long s_ticket;
  constexpr int B = S2_B, G = BT2_G, LD = BT2_LDW;
  static_assert(B + G == 96 && G == 32, "the window rotation assumes 96 rows and a shift of 32");
  double* sZ = smem_wy;             // sZ[c * LD + physical row]
  double* sV = smem_wy + 64 * LD;   // sV[k * LD + physical row]
  const int nslab = (nv + 63) / 64;
  const int nseg = (ngroups + seg - 1) / seg;
  const int tid = threadIdx.x, ln = tid & 63, wv = tid >> 6;
  const int l16 = ln & 15, lg = ln >> 4;
  const int ri = tid & 31, cg = tid >> 5;      // the 32-row pieces: row ri, columns cg + 8 q
  int w = 0;
  long long woff = 0;
  // tickets in the order of the key w = S seg + t, the step at which segment (S, t) can start (then S, then slab):
  // the segments that are runnable together are then consecutive numbers -- ordered by S + t most of the resident
  // workgroups would hold segments whose turn comes much later
  auto seg_lo = [&](int ww) { const int x = ww - (ntmax - 1); return x <= 0 ? 0 : (x + seg - 1) / seg; };
  auto wave_count = [&](int ww) {
    const int s_hi2 = min(ww / seg, nseg - 1), s_lo2 = seg_lo(ww);
    return (long long)max(0, s_hi2 - s_lo2 + 1) * nslab;
  };
  const int nwaves = (nseg - 1) * seg + ntmax;
  unsigned long long* ticket = (unsigned long long*)(flags + ntickets_off);
  auto first_row = [&](int g) {                 // first window row of task (g, t = 0)
    const int s_hi = (n - 3) - g * G;
    return max(0, s_hi - G + 1) + 1;
  };
  long long next_k = 0;
  if (tid == 0) next_k = (long long)__hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    if (tid == 0) s_ticket = next_k;
    __syncthreads();
    const long long k = s_ticket;
    __syncthreads();
    while (w < nwaves && k >= woff + wave_count(w)) { woff += wave_count(w); ++w; }
    if (w >= nwaves) break;
    const int idx = (int)(k - woff);
    const int S = seg_lo(w) + idx / nslab, slab = idx % nslab;
    const int t = w - S * seg;
    const int c0 = slab * 64;
    int g0 = S * seg;
    const int g1 = min(ngroups, g0 + seg);
    while (g0 < g1 && first_row(g0) + t * B > n - 1) ++g0;      // (a task exists from some g on: the windows move up)
    if (g0 >= g1) {                                              // no task in this segment (uniform)
      if (tid == 0) next_k = (long long)__hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    int base = 0;
    bool fresh = true;                                           // the window is not in LDS yet
    for (int g = g0; g < g1; ++g) {
      const int s_hi = (n - 3) - g * G;
      const int s_lo = max(0, s_hi - G + 1);
      const int r0 = s_lo + 1 + t * B;
      const int r1 = min(n - 1, s_hi + (t + 1) * B);
      const int wr = r1 - r0 + 1;
      // ---- loads that depend on nobody: reflector slices and T entries of this lane --------------------------------
      double vreg[G / 4];
      int voff[G / 4];
#pragma unroll
      for (int q = 0; q < G / 4; ++q) {
        const int kk = wv + 4 * q;
        const int s = s_hi - kk;
        const int lo = s + 1 + t * B;
        double v = 0.0;
        if (s >= s_lo && lo <= n - 1 && ln < min(B, n - lo)) v = VV[(soff[s] + t) * B + ln];
        vreg[q] = v;
        voff[q] = (s >= s_lo) ? (s - s_lo) : 0;
      }
      const double* Tg = Tst + (toff[g] + t) * (int64_t)(G * G);
      double treg[2][4][2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int it = 0; it < 2; ++it) treg[kt][q][it] = Tg[(kt * 16 + lg + 4 * q) * G + it * 16 + l16];
      // ---- predecessors: (g, t-1) wrote the rows that enter; (g-1, t) is this workgroup's own previous step unless
      //      the window is fetched afresh -----------------------------------------------------------------------------
      if (tid == 0) {
        int ok = 1;
        const int* f1 = (t > 0) ? flags + (toff[g] + t - 1) * nslab + slab : nullptr;
        const int* f2 = nullptr;
        if (fresh && g == g0 && g > 0 && first_row(g - 1) + t * B <= n - 1) f2 = flags + (toff[g - 1] + t) * nslab + slab;
        long spins = 0;
        while ((f1 && __hip_atomic_load(f1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) ||
               (f2 && __hip_atomic_load(f2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)) {
          if ((++spins & 255) == 0 &&
              (spins > BC_SPIN_LIMIT || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
            __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = 0;
            break;
          }
        }
        s_ok = ok;
      }
      __syncthreads();
      if (s_ok == 0) return;                    // uniform
      // ---- the window: all 95 rows, or the 32 that enter at the top -------------------------------------------------
      if (fresh) {
        base = 0;
        double zreg[16][2];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int c = wv + 4 * q;
          const double* zp = Z + (int64_t)r0 + (int64_t)(c0 + c) * ldz;
          const bool cok = (c0 + c) < nv;
          zreg[q][0] = (cok && ln < wr) ? band_ld<true>(zp + ln) : 0.0;
          zreg[q][1] = (cok && ln + 64 < wr) ? band_ld<true>(zp + ln + 64) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int c = wv + 4 * q;
          sZ[c * LD + ln] = zreg[q][0];
          if (ln < 32) sZ[c * LD + ln + 64] = zreg[q][1];
        }
      } else {
        base = (base >= 32) ? base - 32 : base + 64;          // logical row 0 moved up by 32 rows
        double znew[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int c = cg + 8 * q;
          const double* zp = Z + (int64_t)r0 + (int64_t)(c0 + c) * ldz;
          znew[q] = ((c0 + c) < nv && ri < wr) ? band_ld<true>(zp + ri) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) sZ[(cg + 8 * q) * LD + base + ri] = znew[q];     // (base + 31 <= 95: no wrap)
      }
      // reflector k: its 64 entries from logical row voff on, zero in the 32 other rows of its line (which are the
      // logical rows voff + 64 ... voff + 95 taken modulo 96)
#pragma unroll
      for (int q = 0; q < G / 4; ++q) {
        double* line = sV + (wv + 4 * q) * LD;
        int x = voff[q] + ln;
        line[bt2_rot(x, base)] = vreg[q];
        if (ln < 32) {
          x += 64;
          if (x >= 96) x -= 96;
          line[bt2_rot(x, base)] = 0.0;
        }
      }
      __syncthreads();
      // physical start of the six logical 16-row blocks
      int pbk[6];
      {
        const int bb = __builtin_amdgcn_readfirstlane(base) >> 4;
#pragma unroll
        for (int j = 0; j < 6; ++j) { const int x = j + bb; pbk[j] = ((x >= 6) ? x - 6 : x) * 16; }
      }
      const int ct = wv;
      const double* zc = sZ + (ct * 16 + l16) * LD;
      d4 wacc[2] = {(d4){0.0, 0.0, 0.0, 0.0}, (d4){0.0, 0.0, 0.0, 0.0}};
#pragma unroll
      for (int rbk = 0; rbk < 6; ++rbk) {
        double zy[4], x0[4], x1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int r = pbk[rbk] + 4 * u;
          zy[u] = zc[r + lg];
          x0[u] = sV[l16 * LD + r + lg];
          x1[u] = sV[(16 + l16) * LD + r + lg];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          wacc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[u], zy[u], wacc[0], 0, 0, 0);
          wacc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[u], zy[u], wacc[1], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      d4 w2[2] = {(d4){0.0, 0.0, 0.0, 0.0}, (d4){0.0, 0.0, 0.0, 0.0}};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          w2[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(treg[kt][q][0], wacc[kt][q], w2[0], 0, 0, 0);
          w2[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(treg[kt][q][1], wacc[kt][q], w2[1], 0, 0, 0);
        }
#pragma unroll
      for (int rt = 0; rt < 6; ++rt) {
        double xv[8], zold[4];
        double* zo = sZ + (ct * 16 + l16) * LD + pbk[rt] + lg;
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
          for (int q = 0; q < 4; ++q) xv[it * 4 + q] = sV[(it * 16 + lg + 4 * q) * LD + pbk[rt] + l16];
#pragma unroll
        for (int q = 0; q < 4; ++q) zold[q] = zo[4 * q];
        __builtin_amdgcn_sched_barrier(0);
        d4 u = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
          for (int q = 0; q < 4; ++q) u = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[it * 4 + q], w2[it][q], u, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) zo[4 * q] = zold[q] - u[q];
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
      // ---- what leaves: the bottom 32 rows when the next group's window continues this one, everything otherwise ------
      const bool cont = (g + 1 < g1) && (r0 - (first_row(g + 1) + t * B) == 32);
      if (cont) {
        double zout[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) zout[q] = sZ[(cg + 8 * q) * LD + bt2_rot(63 + ri, base)];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int c = cg + 8 * q;
          if ((c0 + c) < nv && 63 + ri < wr) band_st<true>(Z + (int64_t)r0 + 63 + ri + (int64_t)(c0 + c) * ldz, zout[q]);
        }
        // logical row 63 becomes the padding row 95 of the next window
        if (ri == 0) {
#pragma unroll
          for (int q = 0; q < 8; ++q) sZ[(cg + 8 * q) * LD + bt2_rot(63, base)] = 0.0;
        }
        fresh = false;
      } else {
        double zreg[16][2];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int c = wv + 4 * q;
          zreg[q][0] = sZ[c * LD + bt2_rot(ln, base)];
          zreg[q][1] = (ln < 32) ? sZ[c * LD + bt2_rot(ln + 64, base)] : 0.0;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int c = wv + 4 * q;
          if (c0 + c < nv) {
            double* zp = Z + (int64_t)r0 + (int64_t)(c0 + c) * ldz;
            if (ln < wr) band_st<true>(zp + ln, zreg[q][0]);
            if (ln + 64 < wr) band_st<true>(zp + ln + 64, zreg[q][1]);
          }
        }
        fresh = true;
      }
      // (the next number only when this segment is all but done: a number taken early would sit with a busy workgroup
      //  while idle ones wait for the segment it stands for)
      if (tid == 0 && g + 1 == g1)
        next_k = (long long)__hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0)
        __hip_atomic_store(flags + (toff[g] + t) * nslab + slab, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// (arm, task geometry, flag layout, grid and anti-diagonal ranges: S2Plan of csrc/s2plan.h. d_toff, Tst and err exist
//  on every arm but Seq)
int back_transform_stage2(bigkrls_ctx* ctx, const S2Plan& plan, const int64_t* d_soff, const double* VV,
                          const double* TT, double* Z, int64_t ldz, int nv, const int64_t* d_toff, const double* Tst,
                          int* err) {
  hipStream_t st = ctx->stream;
  const int n = plan.n;
  if (n < 3 || nv <= 0) return BIGKRLS_OK;
  const dim3 block(256);
  const size_t wy_smem = (size_t)(64 + BT2_G) * BT2_LDW * sizeof(double);
  if (plan.have_t) BK_TRY(ensure_dyn_smem(ctx, (const void*)bt2_wy, wy_smem));
  if (plan.bt2_arm == Bt2Arm::Tasks || plan.bt2_arm == Bt2Arm::Chain) {
    const bool chain = plan.bt2_arm == Bt2Arm::Chain;
    const void* fn = chain ? (const void*)bt2_chain : (const void*)bt2_persistent;
    BK_TRY(ensure_dyn_smem(ctx, fn, wy_smem));
    int per_cu = 0, ncu = 0;
    BK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, wy_smem));
    BK_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device));
    const Bt2Flags fl = plan.bt2_flags(nv);
    const int grid = S2Plan::bt2_persistent_grid(per_cu, ncu, fl.total);
    void* pf = nullptr;
    BK_TRY(ws_get(ctx, SLOT_EIG_FLAGS, fl.slot_bytes, &pf));
    BK_HIP(hipMemsetAsync(pf, 0, (size_t)fl.clear_bytes, st));
    if (chain)
      hipLaunchKernelGGL(bt2_chain, dim3(grid), block, wy_smem, st, Z, ldz, n, nv, plan.ngroups, plan.ntmax, plan.seg, d_soff,
                         VV, d_toff, Tst, (int*)pf, (long long)fl.ticket_off, err);
    else
      hipLaunchKernelGGL(bt2_persistent, dim3(grid), block, wy_smem, st, Z, ldz, n, nv, plan.ngroups, plan.ntmax, d_soff, VV,
                         d_toff, Tst, (int*)pf, (long long)fl.ticket_off, err);
    BK_CHECK_LAUNCH();
    return BIGKRLS_OK;
  }
  for (int w = 0; w < plan.bt2_diagonals(); ++w) {
    const S2Range r = plan.bt2_diagonal(w);
    if (r.count == 0) continue;
    if (plan.bt2_arm == Bt2Arm::WyWavefront)
      hipLaunchKernelGGL(bt2_wy, dim3(r.count, plan.slabs(nv)), block, wy_smem, st, Z, ldz, n, nv, w, (int)r.lo, d_soff, VV,
                         d_toff, Tst);
    else
      hipLaunchKernelGGL(bt2_block, dim3(r.count, plan.slabs(nv)), block, 0, st, Z, ldz, n, nv, w, (int)r.lo, d_soff, VV, TT);
  }
  BK_CHECK_LAUNCH();
  return BIGKRLS_OK;
}

// ---- stage-1 back-transform with Bt1Plan::grp panels per step (csrc/s2plan.h) ---------------------------
// Q1 = H(0) H(1) ... with one 64-column block reflector per panel. Consecutive panels are merged:
//   H(p) ... H(p+g-1) = I - Vb Tb Vb',  Vb = [V_p | V_{p+1} | ...] (later panels zero-padded on top),
//   Tb(0:64j, j-th block) = -Tb(0:64j, 0:64j) (V_{0:j}' V_j) T_j   (block form of dlarft),
// so that the n/64 dependent steps of three thin GEMMs become n/256 steps of GEMMs with a 256-deep
// inner dimension. Vb and Tb depend only on stage 1: they are built on the look-ahead stream while
// the main stream does the bulge chasing and the divide & conquer.

// Vb (m0 x 64 g, ld m0): panel i's unit-lower-trapezoidal reflector block in rows >= 64 i
__global__ void s1_extract_vbig(const double* __restrict__ W, int64_t N, int k0, int g, int m0,
                                const double* __restrict__ scales_all, double* __restrict__ Vb) {
  const int64_t total = (int64_t)m0 * S2_B * g;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(e % m0), c = (int)(e / m0);
    const int i = c / S2_B, cc = c % S2_B;
    const int rr = r - S2_B * i;
    const int kp = k0 + S2_B * i;
    double v = 0.0;
    if (rr == cc) v = 1.0;
    else if (rr > cc) v = W[(int64_t)(kp + S2_B + rr) + (int64_t)(kp + cc) * N] * scales_all[kp + cc];
    Vb[e] = v;
  }
}

// ---- the merged blocks of ALL groups, batched (round 6) ---------------------------------------------------------------
// The groups are independent, and per group the work was a chain of 14 small launches (extract, memset, four 2-D copies,
// V'V and its slab reduction, six tiny products): ~1 100 launches of ~14 us at N = 20 000 on the look-ahead stream, which
// under the divide & conquer and the stage-2 back-transform beside them took until after both -- the stage-1
// back-transform waited 5 ms for them. Now: ONE launch builds every group's V block and the block diagonal of its T,
// the Gram products stay one GEMM per group (they are the flops), and every step of the T recurrence is two launches
// over all groups: 1 + 2 ngroups + 2 (g - 1) launches.
// (the group record Bt1Group { k0, g, m0, pad, voff }: csrc/s2plan.h)
static_assert(sizeof(Bt1Group) == 24, "the group table as the kernels read it");

// grid (blocks, ngroups): Vb_q (m0 x 64 g, ld m0) as s1_extract_vbig builds it, and Tb_q = blockdiag(T_{q,0} ... T_{q,g-1})
// in an LT x LT matrix that is zero elsewhere
__global__ __launch_bounds__(256) void bt1_extract_all(const Bt1Group* __restrict__ groups, const double* __restrict__ W,
                                                       int64_t N, const double* __restrict__ scales_all,
                                                       const double* __restrict__ Tall, int LT,
                                                       double* __restrict__ Vstore, double* __restrict__ Tstore) {
  const Bt1Group gr = groups[blockIdx.y];
  const int64_t total = (int64_t)gr.m0 * S2_B * gr.g;
  double* Vb = Vstore + gr.voff;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(e % gr.m0), c = (int)(e / gr.m0);
    const int i = c / S2_B, cc = c % S2_B;
    const int rr = r - S2_B * i;
    const int kp = gr.k0 + S2_B * i;
    double v = 0.0;
    if (rr == cc) v = 1.0;
    else if (rr > cc) v = W[(int64_t)(kp + S2_B + rr) + (int64_t)(kp + cc) * N] * scales_all[kp + cc];
    Vb[e] = v;
  }
  double* Tb = Tstore + (int64_t)blockIdx.y * LT * LT;
  const int64_t tt = (int64_t)LT * LT;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < tt; e += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(e % LT), c = (int)(e / LT);
    const int bi = r / S2_B, bj = c / S2_B;
    double v = 0.0;
    if (bi == bj && bi < gr.g)
      v = Tall[(int64_t)(gr.k0 / S2_B + bi) * S2_B * S2_B + (r % S2_B) + (int64_t)(c % S2_B) * S2_B];
    Tb[e] = v;
  }
}

// One step j of the recurrence T(0:64j, j) = -T(0:64j, 0:64j) (V_{0:j}' V_j) T_j for all groups, as two launches:
//   mode 0: tmp_q (64 j x 64, ld LT) = Gb_q[0:64j, 64j : 64j + 64] T_{q,j}
//   mode 1: Tb_q[0:64j, 64j : 64j + 64] = -Tb_q[0:64j, 0:64j] tmp_q
// grid (j, ngroups): one workgroup per 64 x 64 output tile; thread (tx, ty) owns a 4 x 4 block; operands through LDS in
// k-chunks of 32. A group with g <= j has nothing to do.
__global__ __launch_bounds__(256) void bt1_merge_step(const Bt1Group* __restrict__ groups, int j, int mode, int LT,
                                                      const double* __restrict__ Tall, double* __restrict__ Tstore,
                                                      const double* __restrict__ Gstore, double* __restrict__ tmpstore) {
  constexpr int B = S2_B, KC = 32;
  __shared__ double sA[KC][B + 1];   // sA[k][r]
  __shared__ double sB[KC][B + 1];   // sB[k][c]
  const Bt1Group gr = groups[blockIdx.y];
  if (gr.g <= j) return;
  const int rt = blockIdx.x;                                  // row tile: rows 64 rt .. 64 rt + 63 (< 64 j)
  const int64_t q = blockIdx.y;
  double* Tb = Tstore + q * LT * LT;
  const double* Gb = Gstore + q * LT * LT;
  double* tmp = tmpstore + q * LT * B;
  const double* A;  const double* Bm;  double* C;
  int64_t lda, ldb, ldc;
  int K;
  double alpha;
  if (mode == 0) {
    A = Gb + (int64_t)(B * j) * LT + B * rt; lda = LT;
    Bm = Tall + (int64_t)(gr.k0 / B + j) * B * B; ldb = B;
    C = tmp + B * rt; ldc = LT;
    K = B; alpha = 1.0;
  } else {
    A = Tb + B * rt; lda = LT;
    Bm = tmp; ldb = LT;
    C = Tb + (int64_t)(B * j) * LT + B * rt; ldc = LT;
    K = B * j; alpha = -1.0;
  }
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = 0.0;
  for (int k0 = 0; k0 < K; k0 += KC) {
    for (int e = tid; e < KC * B; e += 256) {
      const int r = e % B, k = e / B;
      sA[k][r] = A[r + (int64_t)(k0 + k) * lda];
    }
    for (int e = tid; e < KC * B; e += 256) {
      const int k = e % KC, c = e / KC;
      sB[k][c] = Bm[(k0 + k) + (int64_t)c * ldb];
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < KC; ++k) {
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = sA[k][4 * ty + a];
#pragma unroll
      for (int c = 0; c < 4; ++c) bv[c] = sB[k][4 * tx + c];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = fma(av[a], bv[c], acc[a][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) C[(4 * ty + a) + (int64_t)(4 * tx + c) * ldc] = alpha * acc[a][c];
}

// Builds every group's Vb and Tb on `ps`. Gstore: one LT x LT Gram matrix per group, tmpstore: LT x 64 per group,
// d_groups: room for the plan's group table (uploaded here from the context's pinned plan buffer).
int bt1_precompute(bigkrls_ctx* ctx, const double* W, int n, const double* taus1, const double* Tall,
                   const Bt1Plan& plan, double* Vstore, double* Tstore, double* Gstore, double* tmpstore,
                   Bt1Group* d_groups, hipStream_t ps) {
  const int64_t N = n;
  const int LT = plan.LT;
  const int ng = (int)plan.ng();
  if (ng == 0) return BIGKRLS_OK;
  // the group table through a pinned buffer of its own (the upload arena belongs to the divide & conquer, which runs
  // on the host while this is still queued)
  const size_t tbytes = (size_t)ng * sizeof(Bt1Group);
  if (ctx->h_plan_bytes < (int64_t)tbytes) {
    BK_HIP(hipStreamSynchronize(ps));
    BK_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->h_plan) BK_HIP(hipHostFree(ctx->h_plan));
    ctx->h_plan = nullptr;
    ctx->h_plan_bytes = 0;
    BK_HIP(hipHostMalloc((void**)&ctx->h_plan, tbytes + 4096, hipHostMallocDefault));
    ctx->h_plan_bytes = (int64_t)tbytes + 4096;
  }
  memcpy(ctx->h_plan, plan.groups.data(), tbytes);
  BK_HIP(hipMemcpyAsync(d_groups, ctx->h_plan, tbytes, hipMemcpyHostToDevice, ps));
  const int blocks = (int)std::min<int64_t>((plan.maxwork + 255) / 256, 1024);
  hipLaunchKernelGGL(bt1_extract_all, dim3(blocks, ng), dim3(256), 0, ps, (const Bt1Group*)d_groups, W, N,
                     (const double*)(taus1 + n), Tall, LT, Vstore, Tstore);
  BK_CHECK_LAUNCH();
  for (int q = 0; q < ng; ++q) {
    StreamScope on(ctx, ps);   // gemm() launches on ctx->stream
    const Bt1Group& gr = plan.groups[q];
    const int w = S2_B * gr.g;
    const double* Vb = Vstore + gr.voff;
    if (gr.g > 1) BK_TRY(gemm(ctx, 1, 0, w, w, gr.m0, 1.0, Vb, gr.m0, Vb, gr.m0, 0.0, Gstore + (int64_t)q * LT * LT, LT));   // Gb = Vb' Vb
  }
  for (int j = 1; j < plan.gmax; ++j)
    for (int mode = 0; mode < 2; ++mode)
      hipLaunchKernelGGL(bt1_merge_step, dim3(j, ng), dim3(256), 0, ps, (const Bt1Group*)d_groups, j, mode, LT, Tall,
                         Tstore, (const double*)Gstore, tmpstore);
  BK_CHECK_LAUNCH();
  return BIGKRLS_OK;
}

// Z <- Q1 Z with the merged block reflectors (W1, W2: LT x nv scratch each). The three products of a step have few
// tiles and long k loops: gemm_thin runs them with the tile width its plan chooses from the shape, bitwise as gemm().
// (development: BIGKRLS_BT1_TILE=128|64|32 fixes the width, read per call)
int back_transform_stage1_grouped(bigkrls_ctx* ctx, const Bt1Plan& plan, const double* Vstore, const double* Tstore,
                                  double* Z, int64_t ldz, int nv, double* W1, double* W2) {
  const int LT = plan.LT;
  const char* tile_env = getenv("BIGKRLS_BT1_TILE");
  const int bn = tile_env ? atoi(tile_env) : 0;
  for (int q = (int)plan.ng() - 1; q >= 0; --q) {
    const Bt1Group& gr = plan.groups[q];
    const int w = S2_B * gr.g;
    const double* Vb = Vstore + gr.voff;
    const double* Tb = Tstore + (int64_t)q * LT * LT;
    double* Zs = Z + (gr.k0 + S2_B);
    BK_TRY(gemm_thin(ctx, 1, 0, w, nv, gr.m0, 1.0, Vb, gr.m0, Zs, ldz, 0.0, W1, LT, bn));
    BK_TRY(gemm_thin(ctx, 0, 0, w, nv, w, 1.0, Tb, LT, W1, LT, 0.0, W2, LT, bn));
    BK_TRY(gemm_thin(ctx, 0, 0, gr.m0, nv, w, -1.0, Vb, gr.m0, W2, LT, 1.0, Zs, ldz, bn));
  }
  return BIGKRLS_OK;
}

int back_transform_stage1(bigkrls_ctx* ctx, const double* W, int n, const double* taus1, double* Z,
                          int64_t ldz, int nv, double* Vp, const double* Tall, double* W1, double* W2) {
  hipStream_t st = ctx->stream;
  const int64_t N = n;
  const int b = S2_B;
  int klast = -1;
  for (int k = 0; k + b < n; k += b) {
    if (n - k - b <= 1) break;
    klast = k;
  }
  for (int k = klast; k >= 0; k -= b) {
    const int m = n - k - b;
    const int pw = b;
    const double* P = W + (k + b) + (int64_t)k * N;
    int blocks = (int)std::min<int64_t>(((int64_t)m * pw + 255) / 256, 4096);
    hipLaunchKernelGGL(s1_extract_v, dim3(blocks), dim3(256), 0, st, P, N, m, pw, taus1 + n + k, Vp);
    BK_CHECK_LAUNCH();
    const double* T = Tall + (int64_t)(k / b) * b * b;
    double* Zs = Z + (k + b);
    BK_TRY(gemm(ctx, 1, 0, pw, nv, m, 1.0, Vp, m, Zs, ldz, 0.0, W1, pw));
    BK_TRY(gemm(ctx, 0, 0, pw, nv, pw, 1.0, T, pw, W1, pw, 0.0, W2, pw));
    BK_TRY(gemm(ctx, 0, 0, m, nv, pw, -1.0, Vp, m, W2, pw, 1.0, Zs, ldz));
  }
  return BIGKRLS_OK;
}
