// kernels_long_moments.hip -- mean and covariance of (A_k, C_k | y): the total length and the number
// of the IBD runs of a region that reach L_k, exactly, per individual, region and threshold
// (include/nghmm.h: nghmm_ibd_long_moments has the definition).
//
// k_count_fwd (kernels_count.hip) walks the posterior chain with one mass per count level.  Here a
// mass class carries, instead of levels, the six moments (1, A, C, A^2, AC, C^2) of (A - oA, C - oC)
// on it, (oA, oC) being the lane's offset pair: N (z = 0), V (inside a run that has not reached L_k)
// and R (inside a run that has reached L_k and is counted).  A run that resolves adds its length so
// far and one to the count, R grows by delta_s at every site it survives.  The planes (the backward
// walks are kernels_longest.hip's), the table of window ends, the rule for Q and the ring are
// k_count_fwd's; a ring entry holds (Q_a, oA_a, oC_a, tau_a[6]).  Every 8 sites of a part the three
// vectors are re-centred on the mean so far, which is what keeps the closing
// E[x^2] - E[x]^2 from cancelling at 10^5 sites and more.
//   k_lmom_fwd<EXACT>  one lane per (individual, segment, threshold), a wave 64 adjacent individuals:
//                   the arrangement kernels_longest.hpp records as the faster one for walks bound by
//                   the latency of a site's dependent chain; four sites' loads in flight together.
// No atomics, one order of operations: the same bits on every call, whatever else is asked for.
#include "fast_dev.hpp"
#include "kernels.hpp"
#include "kernels_long_moments.hpp"

namespace nghmm {

namespace {

struct LmomArgs {
  const uint64_t* __restrict__ seg;
  uint64_t S, I;
  uint32_t K;
  const uint32_t* __restrict__ btab;
  const LongestPart* __restrict__ part;
  uint64_t n_part;
  LongestPlanes pl;
  const double2* __restrict__ piseg;
  CountRings rings;
  const double* __restrict__ cum;
  const double* __restrict__ step;
  double len_add;
  LongMomentRec* __restrict__ rec;
  int* __restrict__ overflow;     // raised if a ring is ever full at a push
};

template <bool EXACT>
__device__ __forceinline__ double exp_le0(double x) {
  const double y = x < 0.0 ? x : 0.0;
  if constexpr (EXACT) return det_exp(y);
  else return exp_nonpos(y);
}

// the moments (1, A, C, A^2, AC, C^2) of one mass class
struct Mom {
  double m0, a, c, aa, ac, cc;
};

__device__ __forceinline__ Mom mom_zero() { return Mom{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }
__device__ __forceinline__ Mom mom_scale(const Mom& m, double w) {
  return Mom{m.m0 * w, m.a * w, m.c * w, m.aa * w, m.ac * w, m.cc * w};
}
__device__ __forceinline__ Mom mom_add(const Mom& x, const Mom& y) {
  return Mom{x.m0 + y.m0, x.a + y.a, x.c + y.c, x.aa + y.aa, x.ac + y.ac, x.cc + y.cc};
}
__device__ __forceinline__ Mom mom_sub(const Mom& x, const Mom& y) {
  return Mom{x.m0 - y.m0, x.a - y.a, x.c - y.c, x.aa - y.aa, x.ac - y.ac, x.cc - y.cc};
}
// Sh(m; l, c): the moments of (A + l, C + c)
__device__ __forceinline__ Mom mom_shift(const Mom& m, double l, double c) {
  Mom o;
  o.m0 = m.m0;
  o.a = m.a + l * m.m0;
  o.c = m.c + c * m.m0;
  o.aa = (m.aa + (2.0 * l) * m.a) + (l * l) * m.m0;
  o.ac = ((m.ac + l * m.c) + c * m.a) + (l * c) * m.m0;
  o.cc = (m.cc + (2.0 * c) * m.c) + (c * c) * m.m0;
  return o;
}

constexpr int kBatch = 4;          // sites whose loads are in flight together, as k_count_fwd
constexpr uint32_t kEntry = kLongMomentEntry;
constexpr uint32_t kRecentre = 8;  // sites of a part between two re-centrings

template <bool EXACT>
__global__ void __launch_bounds__(64)
k_lmom_fwd(const LmomArgs A) {
  const uint64_t nib = (A.I + 63) / 64;
  const uint32_t K = A.K;
  const uint64_t gk = blockIdx.x / nib;
  const uint64_t g = gk / K;
  const uint32_t k = (uint32_t)(gk % K);
  const uint64_t i = (blockIdx.x % nib) * 64 + threadIdx.x;
  if (i >= A.I) return;
  const uint64_t a = A.seg[g], b = A.seg[g + 1], I = A.I;
  const uint32_t cap = A.rings.cap[g * K + k];
  double* const ring = A.rings.ring + A.rings.off[g * K + k] * kEntry * I + i;
  const uint32_t* const bt = A.btab + (uint64_t)k * A.S;

  double pi0, pi1, Q = 0.0, oA = 0.0, oC = 0.0;
  uint32_t ap = 0, cnt = 0, hd = 0;   // the oldest unresolved start, the ring's live entries, its head
  Mom N = mom_zero(), V = mom_zero(), R = mom_zero();
  {
    const double2 p = A.piseg[g * I + i];
    pi0 = p.x;
    pi1 = p.y;
  }
  // the first part that ends behind the segment's first site
  uint64_t p;
  {
    uint64_t lo = 0, hi = A.n_part;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (A.part[mid].end <= a) lo = mid + 1;
      else hi = mid;
    }
    p = lo;
  }
  uint64_t pb = ~0ull, pe = 0;
  if (p < A.n_part) {
    pb = A.part[p].begin;
    pe = A.part[p].end;
  }
  for (uint64_t s0 = a; s0 < b; s0 += kBatch) {
    double r00[kBatch], r01[kBatch], r10[kBatch], r11[kBatch], lr[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const uint64_t s = s0 + u;
      r00[u] = r01[u] = r10[u] = r11[u] = 0.0;
      lr[u] = 1.0;                 // in the ln rho plane: blocked (ln rho <= 0, so 1.0 is no value)
      if (s < b) {
        const uint64_t o = s * I + i;
        r00[u] = A.pl.r00[o];
        r01[u] = A.pl.r01[o];
        r10[u] = A.pl.r10[o];
        r11[u] = A.pl.r11[o];
        lr[u] = A.pl.lnrho[o];
      }
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const uint64_t s = s0 + u;
      if (s >= b) continue;
      if (s != a) {
        const double n0 = pi0 * r00[u] + pi1 * r10[u];
        const double n1 = pi0 * r01[u] + pi1 * r11[u];
        pi0 = n0;
        pi1 = n1;
      }
      if (s < pb || s >= pe) continue;
      const bool begin = s == pb;
      const bool blocked = lr[u] > 0.0;
      const double rho = blocked ? 0.0 : r11[u];
      Q = (begin || blocked) ? 0.0 : Q + lr[u];
      Mom tau, Nn, Vr, Rr;
      if (begin) {
        oA = oC = 0.0;
        tau = Nn = Vr = Rr = mom_zero();
        // (an excluded IBD state: pi(0) is 1, without the roundings the propagated pair carries)
        Nn.m0 = (pi1 == 0.0 && pi0 > 0.0) ? 1.0 : pi0;
        tau.m0 = pi1;
        cnt = 0;
      } else {
        tau = mom_scale(N, r01[u]);
        Nn = mom_add(mom_add(mom_scale(N, r00[u]), mom_scale(V, r10[u])), mom_scale(R, r10[u]));
        Vr = mom_scale(V, rho);
        Rr = mom_scale(R, rho);
        if (blocked) cnt = 0;      // those starts can never reach L_k
      }
      const bool push = bt[s] != kLongestNone;
      if (push && cnt >= cap) *A.overflow = 1;   // (never: the host sized the ring)
      if (push && cnt < cap) {
        if (cnt == 0) {
          hd = 0;
          ap = (uint32_t)s;
        }
        uint32_t sl = hd + cnt;
        sl = sl >= cap ? sl - cap : sl;
        double* const e = ring + (uint64_t)sl * kEntry * I;
        e[0] = Q;
        e[I] = oA;
        e[2 * I] = oC;
        e[3 * I] = tau.m0;
        e[4 * I] = tau.a;
        e[5 * I] = tau.c;
        e[6 * I] = tau.aa;
        e[7 * I] = tau.ac;
        e[8 * I] = tau.cc;
        ++cnt;
      }
      Mom G = mom_zero(), Gs = mom_zero();
      const double cs = A.cum[s];
      while (cnt > 0 && bt[ap] == (uint32_t)s) {   // the starts that resolve at s, oldest first
        const double* const e = ring + (uint64_t)hd * kEntry * I;
        const double w = exp_le0<EXACT>(Q - e[0]);
        const Mom t{e[3 * I] * w, e[4 * I] * w, e[5 * I] * w, e[6 * I] * w, e[7 * I] * w, e[8 * I] * w};
        const Mom ga = mom_shift(t, e[I] - oA, e[2 * I] - oC);   // at the lane's current offsets
        G = mom_add(G, ga);
        Gs = mom_add(Gs, mom_shift(ga, (cs - A.cum[ap]) + A.len_add, 1.0));
        hd = hd + 1 == cap ? 0 : hd + 1;
        --cnt;
        ++ap;
      }
      V = mom_sub(mom_add(Vr, tau), G);
      if (!(V.m0 > 0.0)) V = mom_zero();
      R = mom_add(begin ? Rr : mom_shift(Rr, A.step[s], 0.0), Gs);
      N = Nn;
      if (((s - pb) & (kRecentre - 1)) == kRecentre - 1) {
        const double t0 = (N.m0 + V.m0) + R.m0;
        if (t0 > 0.0) {
          const double dA = ((N.a + V.a) + R.a) / t0, dC = ((N.c + V.c) + R.c) / t0;
          N = mom_shift(N, -dA, -dC);
          V = mom_shift(V, -dA, -dC);
          R = mom_shift(R, -dA, -dC);
          oA += dA;
          oC += dC;
        }
      }
      if (s + 1 == pe) {   // the part is complete
        const Mom t = mom_add(mom_add(N, V), R);
        LongMomentRec out{0.0, 0.0, 0.0, 0.0, 0.0};
        if (t.m0 > 0.0) {
          const double mA = t.a / t.m0, mC = t.c / t.m0;
          const double va = t.aa / t.m0 - mA * mA, vt = t.cc / t.m0 - mC * mC;
          out.mean_a = oA + mA;
          out.mean_t = oC + mC;
          out.var_a = va > 0.0 ? va : 0.0;
          out.cov_at = t.ac / t.m0 - mA * mC;
          out.var_t = vt > 0.0 ? vt : 0.0;
        }
        A.rec[(i * A.n_part + p) * K + k] = out;
        cnt = 0;
        ++p;
        pb = ~0ull;
        pe = 0;
        if (p < A.n_part) {
          pb = A.part[p].begin;
          pe = A.part[p].end;
        }
      }
    }
  }
}

}  // namespace

bool long_moments_fwd(hipStream_t st, bool exact, const uint64_t* d_seg, uint64_t n_seg, uint64_t S, uint64_t I,
                      uint32_t K, const uint32_t* d_btab, const LongestPart* d_part, uint64_t n_part,
                      const LongestPlanes& pl, const double* d_piseg, const CountRings& rings, const double* d_cum,
                      const double* d_step, double len_add, LongMomentRec* d_rec, int* d_overflow) {
  if (K < 1 || K > kLongestMaxK) return false;
  const uint64_t grid = n_seg * K * ((I + 63) / 64);
  if (n_seg == 0 || grid > 0x7fffffffull) return false;
  LmomArgs A;
  A.seg = d_seg;
  A.S = S;
  A.I = I;
  A.K = K;
  A.btab = d_btab;
  A.part = d_part;
  A.n_part = n_part;
  A.pl = pl;
  A.piseg = reinterpret_cast<const double2*>(d_piseg);
  A.rings = rings;
  A.cum = d_cum;
  A.step = d_step;
  A.len_add = len_add;
  A.rec = d_rec;
  A.overflow = d_overflow;
  if (exact) hipLaunchKernelGGL((k_lmom_fwd<true>), dim3(grid), dim3(64), 0, st, A);
  else hipLaunchKernelGGL((k_lmom_fwd<false>), dim3(grid), dim3(64), 0, st, A);
  return hipGetLastError() == hipSuccess;
}

}  // namespace nghmm
