// exp(x) for x <= 0, the only domain the Gaussian kernel needs, for kernels outside csrc/gemm.hip that form per-column
// factors of kernel entries (csrc/shapley.hip): exp_nonpos_tab and its table exactly as csrc/gemm.hip defines them for
// its own kernels (the same constants and operations, so a factor here and a kernel entry there round alike). Device
// code only; header-only; the table has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

namespace bk {

// exp(x) with a 32-entry table: x log2(e) = (32 q + j + f) / 32, e^x = 2^q 2^(j/32) e^r with |r| <= ln2/64, where a
// degree-6 polynomial has a truncation error of 5e-18 -- 7 fused multiply-adds less per element than the table-free form, in
// kernels whose time is the fp64 VALU work of this epilogue. `tab` (LDS, 32 doubles) = 2^(j/32), correctly rounded.
static __device__ __constant__ double kExp2Tab32[32] = {
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

}  // namespace bk
