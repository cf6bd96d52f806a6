// kernels_count.hip -- P(exactly c IBD runs of a region reach L_k | y), c = 0 .. M - 1, and P(M or
// more do), exactly, per individual, region and threshold (include/nghmm.h: nghmm_ibd_count has the
// definition).
//
// k_longest_fwd (kernels_longest.hip) absorbs a run into Hit the moment it reaches L_k.  Here that
// mass stays alive: it enters R_{c+1}, the mass inside a run that has reached L_k and is counted,
// and falls back to N_{c+1} when the run ends; only the mass that reaches level M is absorbed, in
// Top.  So the recursion is k_longest_fwd's with one more index, on the same planes (the backward
// walks are kernels_longest.hip's), the same table of window ends, the same rule for Q, and a ring
// whose entries hold (Q_a, tau_{a,0}, .., tau_{a,M-1}).
//   k_count_fwd<EXACT, CAP>  one lane per (individual, segment, threshold), a wave 64 adjacent
//                   individuals: the arrangement kernels_longest.hpp records as the faster one for
//                   walks bound by the latency of a site's dependent chain.  CAP in {4, 8, 16} is
//                   the number of levels the lane holds in registers, the smallest >= M; M is a
//                   runtime bound inside the unrolled loops.  Level 0 is ordered as k_longest_fwd
//                   orders its N, V, Hit, so that M = 1 gives nghmm_ibd_longest's p_none and p_any.
// No atomics, one order of operations: the same bits on every call, whatever else is asked for.
#include "fast_dev.hpp"
#include "kernels.hpp"
#include "kernels_count.hpp"

namespace nghmm {

namespace {

constexpr double kBlocked = 1.0;   // in the ln rho plane: ln rho <= 0, so 1.0 is no value

struct CountArgs {
  const uint64_t* __restrict__ seg;
  uint64_t S, I;
  uint32_t K, M;
  const uint32_t* __restrict__ btab;
  const LongestPart* __restrict__ part;
  uint64_t n_part;
  LongestPlanes pl;
  const double2* __restrict__ piseg;
  CountRings rings;
  double* __restrict__ prob;
  int* __restrict__ overflow;     // raised if a ring is ever full at a push
};

template <bool EXACT>
__device__ __forceinline__ double exp_le0(double x) {
  const double y = x < 0.0 ? x : 0.0;
  if constexpr (EXACT) return det_exp(y);
  else return exp_nonpos(y);
}

constexpr int kBatch = 4;          // sites whose loads are in flight together, as k_longest_fwd

template <bool EXACT, int CAP>
__global__ void __launch_bounds__(64)
k_count_fwd(const CountArgs A) {
  const uint64_t nib = (A.I + 63) / 64;
  const uint32_t K = A.K, M = A.M, W = A.M + 1;
  const uint64_t gk = blockIdx.x / nib;
  const uint64_t g = gk / K;
  const uint32_t k = (uint32_t)(gk % K);
  const uint64_t i = (blockIdx.x % nib) * 64 + threadIdx.x;
  if (i >= A.I) return;
  const uint64_t a = A.seg[g], b = A.seg[g + 1], I = A.I;
  const uint32_t cap = A.rings.cap[g * K + k];
  double* const ring = A.rings.ring + A.rings.off[g * K + k] * W * I + i;
  const uint32_t* const bt = A.btab + (uint64_t)k * A.S;

  CountLane<CAP> L;
  {
    const double2 p = A.piseg[g * I + i];
    L.pi0 = p.x;
    L.pi1 = p.y;
  }
  L.Q = 0.0;
  L.top = 0.0;
  L.ap = L.cnt = L.hd = 0;
#pragma unroll
  for (int c = 0; c < CAP; ++c) L.N[c] = L.V[c] = L.R[c] = 0.0;
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
      lr[u] = kBlocked;
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
        const double n0 = L.pi0 * r00[u] + L.pi1 * r10[u];
        const double n1 = L.pi0 * r01[u] + L.pi1 * r11[u];
        L.pi0 = n0;
        L.pi1 = n1;
      }
      if (s < pb || s >= pe) continue;
      const bool begin = s == pb;
      const bool blocked = lr[u] > 0.0;
      const double rho = blocked ? 0.0 : r11[u];
      L.Q = (begin || blocked) ? 0.0 : L.Q + lr[u];
      double tau[CAP], Nn[CAP], Vr[CAP], Rr[CAP], G[CAP];
#pragma unroll
      for (int c = 0; c < CAP; ++c) {
        tau[c] = Nn[c] = Vr[c] = Rr[c] = G[c] = 0.0;
        if ((uint32_t)c < M) {
          if (begin) {
            if (c == 0) {
              // (an excluded IBD state: pi(0) is 1, without the roundings the propagated pair carries)
              Nn[c] = (L.pi1 == 0.0 && L.pi0 > 0.0) ? 1.0 : L.pi0;
              tau[c] = L.pi1;
            }
          } else {
            tau[c] = L.N[c] * r01[u];
            Nn[c] = L.N[c] * r00[u] + L.V[c] * r10[u];
            if (c > 0) Nn[c] = Nn[c] + L.R[c] * r10[u];
            Vr[c] = L.V[c] * rho;
            Rr[c] = L.R[c] * rho;
          }
        }
      }
      if (begin) {
        L.top = 0.0;
        L.cnt = 0;
      } else if (blocked) {
        L.cnt = 0;   // those starts can never reach L_k
      }
      const bool push = bt[s] != kLongestNone;
      if (push && L.cnt >= cap) *A.overflow = 1;   // (never: the host sized the ring)
      if (push && L.cnt < cap) {
        if (L.cnt == 0) {
          L.hd = 0;
          L.ap = (uint32_t)s;
        }
        uint32_t sl = L.hd + L.cnt;
        sl = sl >= cap ? sl - cap : sl;
        double* const e = ring + (uint64_t)sl * W * I;
        e[0] = L.Q;
#pragma unroll
        for (int c = 0; c < CAP; ++c)
          if ((uint32_t)c < M) e[(uint64_t)(c + 1) * I] = tau[c];
        ++L.cnt;
      }
      while (L.cnt > 0 && bt[L.ap] == (uint32_t)s) {   // the starts that resolve at s, oldest first
        const double* const e = ring + (uint64_t)L.hd * W * I;
        const double w = exp_le0<EXACT>(L.Q - e[0]);
#pragma unroll
        for (int c = 0; c < CAP; ++c)
          if ((uint32_t)c < M) G[c] += e[(uint64_t)(c + 1) * I] * w;
        L.hd = L.hd + 1 == cap ? 0 : L.hd + 1;
        --L.cnt;
        ++L.ap;
      }
#pragma unroll
      for (int c = 0; c < CAP; ++c) {
        if ((uint32_t)c < M) {
          if ((uint32_t)c + 1 == M) L.top += G[c];
          const double v = (Vr[c] + tau[c]) - G[c];
          L.V[c] = v > 0.0 ? v : 0.0;
          L.N[c] = Nn[c];
          if (c > 0) L.R[c] = Rr[c] + G[c - 1];
        }
      }
      if (s + 1 == pe) {   // the part is complete
        double* const out = A.prob + ((i * A.n_part + p) * K + k) * W;
#pragma unroll
        for (int c = 0; c < CAP; ++c) {
          if ((uint32_t)c < M) out[c] = c > 0 ? L.N[c] + L.V[c] + L.R[c] : L.N[c] + L.V[c];
        }
        out[M] = L.top;
        L.cnt = 0;
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

template <bool EXACT>
void launch(uint32_t M, unsigned grid, hipStream_t st, const CountArgs& A) {
  if (M <= 4) hipLaunchKernelGGL((k_count_fwd<EXACT, 4>), dim3(grid), dim3(64), 0, st, A);
  else if (M <= 8) hipLaunchKernelGGL((k_count_fwd<EXACT, 8>), dim3(grid), dim3(64), 0, st, A);
  else hipLaunchKernelGGL((k_count_fwd<EXACT, 16>), dim3(grid), dim3(64), 0, st, A);
}

}  // namespace

bool count_fwd(hipStream_t st, bool exact, const uint64_t* d_seg, uint64_t n_seg, uint64_t S, uint64_t I,
               uint32_t K, uint32_t M, const uint32_t* d_btab, const LongestPart* d_part, uint64_t n_part,
               const LongestPlanes& pl, const double* d_piseg, const CountRings& rings, double* d_prob,
               int* d_overflow) {
  if (K < 1 || K > kLongestMaxK || M < 1 || M > kCountMaxM) return false;
  const uint64_t grid = n_seg * K * ((I + 63) / 64);
  if (n_seg == 0 || grid > 0x7fffffffull) return false;
  CountArgs A;
  A.seg = d_seg;
  A.S = S;
  A.I = I;
  A.K = K;
  A.M = M;
  A.btab = d_btab;
  A.part = d_part;
  A.n_part = n_part;
  A.pl = pl;
  A.piseg = reinterpret_cast<const double2*>(d_piseg);
  A.rings = rings;
  A.prob = d_prob;
  A.overflow = d_overflow;
  if (exact) launch<true>(M, (unsigned)grid, st, A);
  else launch<false>(M, (unsigned)grid, st, A);
  return hipGetLastError() == hipSuccess;
}

}  // namespace nghmm
