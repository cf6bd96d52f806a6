// lnshare_dev.hpp -- ln of a share a / (a + b) from the small side, in fast mode's arithmetic:
// what k_expect_walk (kernels_expect.hip) and k_bylength_walk (kernels_bylength.hip) share.
// With x = min / max of the pair, the larger entry's ln share is -log1p(x) and the smaller one's
// ln(x) - log1p(x); log1p(x) = 2 atanh(x / (2 + x)) and ln(x) from the same odd series on the
// mantissa: a share next to 1 (ln share ~ -1e-6) keeps its relative accuracy.
#pragma once

#include "fast_dev.hpp"

namespace nghmm {

#define NGH_NEG_INF (-__builtin_huge_val())

constexpr double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;

// 2 atanh(s) = ln((1 + s) / (1 - s)) for |s| <= 0.1716, i.e. s = (m - 1) / (m + 1) with m in
// [sqrt(1/2), sqrt(2)]: the odd series to s^19 (the first dropped term, s^20 / 21, is below 2.3e-17
// of the result).  Relative accuracy for every s, however small.
__device__ __forceinline__ double atanh2(double s) {
  const double z = s * s;
  double p = 1.0 / 19.0;
  p = fma(p, z, 1.0 / 17.0);
  p = fma(p, z, 1.0 / 15.0);
  p = fma(p, z, 1.0 / 13.0);
  p = fma(p, z, 1.0 / 11.0);
  p = fma(p, z, 1.0 / 9.0);
  p = fma(p, z, 1.0 / 7.0);
  p = fma(p, z, 1.0 / 5.0);
  p = fma(p, z, 1.0 / 3.0);
  const double t = s + s;
  return fma(t * z, p, t);
}

// log1p(x) for x in [0, 1], to relative accuracy: ln(1 + x) = 2 atanh(x / (2 + x)), formed from x
// itself (1 + x is never rounded); above sqrt(2) - 1 the argument is halved first,
// ln(1 + x) = ln 2 + 2 atanh((x - 1) / (x + 3)).
__device__ __forceinline__ double log1p_unit(double x) {
  const bool up = x > 0.41421356237309515;
  const double s = (up ? x - 1.0 : x) * rcp_nr2(up ? x + 3.0 : x + 2.0);
  const double t = atanh2(s);
  return up ? LN2_HI + (LN2_LO + t) : t;
}

// ln(x) for x in (0, 1]: mantissa in [sqrt(1/2), sqrt(2)) through the same series, the exponent
// times ln 2 in two parts; ln(0) = -inf
__device__ __forceinline__ double ln_unit(double x) {
  double m = __builtin_amdgcn_frexp_mant(x);   // [0.5, 1)
  int e = __builtin_amdgcn_frexp_exp(x);
  const bool low = m < 0.70710678118654752;
  m = low ? m + m : m;
  e = low ? e - 1 : e;
  const double s = (m - 1.0) * rcp_nr2(m + 1.0);
  const double de = (double)e;
  const double r = fma(de, LN2_HI, fma(de, LN2_LO, atanh2(s)));
  return x > 0.0 ? r : NGH_NEG_INF;
}

// la = ln(a / (a + b)), lb = ln(b / (a + b)) for a, b >= 0, both from the small side: with
// x = min / max, the larger share is -log1p(x) and the smaller ln(x) - log1p(x) (no cancellation:
// both terms are <= 0).  A share of 0 gives -inf, 0/0 included.
__device__ __forceinline__ void ln_shares(double a, double b, double& la, double& lb) {
  const bool big = b <= a;
  const double hi = big ? a : b, lo = big ? b : a;
  const double x = lo * rcp_nr2(hi);   // in [0, 1]; hi == 0: NaN, unused
  const double l1p = log1p_unit(x);
  const double l_hi = hi > 0.0 ? -l1p : NGH_NEG_INF;
  const double l_lo = lo > 0.0 ? ln_unit(x) - l1p : NGH_NEG_INF;
  la = big ? l_hi : l_lo;
  lb = big ? l_lo : l_hi;
}

// ---- exact mode: the same in log space through detmath.h ----
// gen_func.cpp:135-151 for two values
__device__ __forceinline__ double lsum2(double a0, double a1) {
  const double M = (a1 >= a0) ? a1 : a0;
  if (M == NGH_NEG_INF) return NGH_NEG_INF;
  return det_log(det_exp(a0 - M) + det_exp(a1 - M)) + M;
}

// ln(A / (A + B)) from la = ln A, lb = ln B; A == 0 gives -inf
__device__ __forceinline__ double ln_share_log(double la, double lb) {
  if (!(la > NGH_NEG_INF)) return NGH_NEG_INF;
  const bool big = lb <= la;
  const double x = det_exp(big ? lb - la : la - lb);   // in [0, 1]
  const double u = 1.0 + x;
  const double l1p = u == 1.0 ? x : det_log(u) * x / (u - 1.0);
  return big ? -l1p : (la - lb) - l1p;
}

__device__ __forceinline__ double exp0(double l) { return l > NGH_NEG_INF ? det_exp(l) : 0.0; }

}  // namespace nghmm
