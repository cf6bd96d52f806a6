// kernels_longest.hip -- P(some IBD run of a region reaches L_k | y) and P(none does), exactly, per
// individual, region and threshold (include/nghmm.h: nghmm_ibd_longest has the definition).
//
// Given the data the path is a Markov chain with the steps r_s(k, l) = P(z_s = l | z_{s-1} = k, y).
// The recursion carries, per threshold, the mass N that is outside a run with no hit yet, the mass
// V inside a run that has not reached L_k, and the absorbed mass Hit; the mass that reaches L_k
// at site s left N at the run's first site a, b_k(a) = s, and stayed IBD since: tau_a W(a, s).  That
// delay of L sites keeps the recursion from being a product of 2 x 2 operators, so the walks are
// plain vector recursions, one site after the other, in the shape of k_freq_fwd / k_freq_bwd
// (kernels_freqinfo.hip): one lane per (individual, segment), a wave 64 adjacent individuals, every
// plane read and written as 512 contiguous bytes per site, the loads of a batch in flight together.
//   k_longest_bwd   right to left: beta (rescaled by powers of two after every site); per cell the
//                   four steps, each from its own product, and ln rho from the small side
//                   (lnshare_dev.hpp), 1.0 where the step is blocked; pi at a chromosome's first site
//   k_longest_fwd   left to right: pi propagated, pi_s(l) = pi_{s-1}(0) r_s(0, l) + pi_{s-1}(1) r_s(1, l);
//                   at every part's first site (N, V, Hit, Q, ring) restart; the K thresholds are a
//                   loop inside the lane, so the planes are read once -- or, as long as all their
//                   waves are resident at once, lanes of their own (longest_split_lanes: faster,
//                   the walk being bound by latency), with the same operations on the same values.  A lane's ring of threshold k
//                   holds (tau_a, Q_a) of the starts a in [ap, s], a queue in device scratch with the
//                   individual as the fastest index; b_k is non-decreasing, so the starts resolve
//                   from the front.
// Exact mode: k_longest_bwd_exact, one lane per individual in log space through detmath.h, and the
// same forward walk with W through det_exp.
// No atomics, one order of operations: the same bits on every call, whatever else is asked for.
#include "fast_dev.hpp"
#include "kernels.hpp"
#include "kernels_longest.hpp"
#include "lnshare_dev.hpp"

namespace nghmm {

namespace {

constexpr double kBlocked = 1.0;   // in the ln rho plane: ln rho <= 0, so 1.0 is no value
constexpr int kBatch = 4;          // sites whose loads are in flight together

// the two emissions of a cell at frequency f (kernels_freqinfo.hip)
__device__ __forceinline__ void emissions(double p0, double p1, double p2, double f, double& e0, double& e1) {
  const double om = 1 - f;
  e0 = fma(p0, om * om, fma(p1, 2 * (om * f), p2 * (f * f)));
  e1 = fma(p0, om, p2 * f);
}

__device__ __forceinline__ void rescale2(double& v0, double& v1) {
  int ex = 0;
  renorm2(v0, v1, ex);
}

struct BwdArgs {
  GlView gl;
  const double* __restrict__ freq;
  const double* __restrict__ pos;
  const uint64_t* __restrict__ seg;
  uint64_t S, I;
  const double* __restrict__ indF;
  const double* __restrict__ alpha;
  uint32_t first_is_start;
  const double* __restrict__ win;
  double* __restrict__ wout;
  LongestPlanes pl;
  double2* __restrict__ piseg;
  int* __restrict__ flags;
};

__global__ void __launch_bounds__(64)
k_longest_bwd(const BwdArgs A) {
  const uint64_t nib = (A.I + 63) / 64;
  const uint64_t g = blockIdx.x / nib;
  const uint64_t i = (blockIdx.x % nib) * 64 + threadIdx.x;
  if (i >= A.I) return;
  const uint64_t a = A.seg[g], b = A.seg[g + 1], I = A.I;
  const double f = A.indF[i], al = A.alpha[i];
  const double q0 = 1 - f, q1 = f;
  double w0 = 1.0, w1 = 1.0;   // the data's end, or a chromosome start at site b
  if (b == A.S && A.win) {
    w0 = A.win[i * 2];
    w1 = A.win[i * 2 + 1];
  }
  bool bad = false;
  for (uint64_t hi = b; hi > a;) {   // batches as in k_freq_bwd, right to left
    const uint64_t lo = hi - a >= (uint64_t)kBatch ? hi - kBatch : a;
    double cc[kBatch], e0[kBatch], e1[kBatch];
    bool start[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const uint64_t s = lo + u;
      cc[u] = e0[u] = e1[u] = 0.0;
      start[u] = true;
      if (s < hi) {
        const double d = A.pos[s];
        start[u] = !(d < kDStart) || (s == 0 && A.first_is_start);
        if (!start[u]) cc[u] = coanc(al, d);
        double p0, p1, p2;
        gl_fetch(A.gl, s * I + i, p0, p1, p2);
        emissions(p0, p1, p2, A.freq[s], e0[u], e1[u]);
      }
    }
#pragma unroll
    for (int u = kBatch - 1; u >= 0; --u) {
      const uint64_t s = lo + u;
      if (s < hi) {
        const double om = 1 - cc[u];   // (a chromosome start: c = 0, both rows are q e beta)
        const double u0 = e0[u] * w0, u1 = e1[u] * w1;
        const double m00 = fma(om, q0, cc[u]) * u0, m01 = om * q1 * u1;
        const double m10 = om * q0 * u0, m11 = fma(om, q1, cc[u]) * u1;
        const double s0 = m00 + m01, s1 = m10 + m11;
        bad |= (s0 != s0) | (s1 != s1);
        const double z0 = rcp_nr2(s0), z1 = rcp_nr2(s1);
        const bool ok0 = s0 > 0.0, ok1 = s1 > 0.0;
        const double r00 = ok0 ? m00 * z0 : 0.0, r01 = ok0 ? m01 * z0 : 0.0;
        const double r10 = ok1 ? m10 * z1 : 0.0, r11 = ok1 ? m11 * z1 : 0.0;
        double L10, L11;
        ln_shares(m10, m11, L10, L11);
        const bool blocked = start[u] || !(r11 > 0.0) || !(L11 > NGH_NEG_INF);
        const uint64_t o = s * I + i;
        A.pl.r00[o] = r00;
        A.pl.r01[o] = r01;
        A.pl.r10[o] = r10;
        A.pl.r11[o] = r11;
        A.pl.lnrho[o] = blocked ? kBlocked : L11;
        if (start[u]) {
          if (s == a) A.piseg[g * I + i] = double2{r00, r01};
          w0 = w1 = 1.0;
        } else {
          w0 = s0;
          w1 = s1;
          rescale2(w0, w1);
        }
      }
    }
    hi = lo;
  }
  if (a == 0 && A.wout) {
    A.wout[i * 2] = w0;
    A.wout[i * 2 + 1] = w1;
  }
  if (bad) A.flags[FLAG_INVALID_LKL] = 1;
}

// the two log emissions of a cell of LOG likelihoods at frequency f (kernels_freqinfo.hip)
__device__ __forceinline__ void log_emissions(const GlView& gl, uint64_t cell, double f, double& le0,
                                              double& le1) {
  double g0, g1, g2, e0, e1;
  gl_fetch(gl, cell, g0, g1, g2);
  emissions(det_exp(g0), det_exp(g1), det_exp(g2), f, e0, e1);
  le0 = e0 > 0.0 ? det_log(e0) : (e0 == 0.0 ? NGH_NEG_INF : e0 * 0.0 / 0.0);
  le1 = e1 > 0.0 ? det_log(e1) : (e1 == 0.0 ? NGH_NEG_INF : e1 * 0.0 / 0.0);
}

// exp(m - n) for n = lsum2(m, .): 0 where m or n is -inf
__device__ __forceinline__ double share(double m, double n) {
  return (m > NGH_NEG_INF && n > NGH_NEG_INF) ? det_exp(m - n) : 0.0;
}

__global__ void __launch_bounds__(64)
k_longest_bwd_exact(const GlView gl, const double* __restrict__ freq, const double* __restrict__ pos,
                    uint64_t S, uint64_t I, uint64_t n_seg, const double* __restrict__ indF,
                    const double* __restrict__ alpha, const LongestPlanes pl, double2* __restrict__ piseg,
                    int* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  const double f = indF[i], al = alpha[i];
  const double q0 = 1 - f, q1 = f;
  bool bad = false;
  uint64_t g = n_seg;
  double b0 = 0.0, b1 = 0.0;   // log beta of the last site
  for (uint64_t s = S; s-- > 0;) {
    const double d = pos[s];
    const bool start = !(d < kDStart) || s == 0;
    const double cs = (d < kDStart && s != 0) ? det_exp(-al * d) : 0.0;
    const double a = 1 - cs;
    const double t00 = det_log(a * q0 + cs), t01 = det_log(a * q1);
    const double t10 = det_log(a * q0), t11 = det_log(a * q1 + cs);
    double le0, le1;
    log_emissions(gl, s * I + i, freq[s], le0, le1);
    const double u0 = le0 + b0, u1 = le1 + b1;
    const double m00 = t00 + u0, m01 = t01 + u1, m10 = t10 + u0, m11 = t11 + u1;
    const double n0 = lsum2(m00, m01), n1 = lsum2(m10, m11);
    bad |= (n0 != n0) | (n1 != n1);
    const double r00 = share(m00, n0), r01 = share(m01, n0);
    const double r10 = share(m10, n1), r11 = share(m11, n1);
    const double L11 = ln_share_log(m11, m10);
    const bool blocked = start || !(r11 > 0.0) || !(L11 > NGH_NEG_INF);
    const uint64_t o = s * I + i;
    pl.r00[o] = r00;
    pl.r01[o] = r01;
    pl.r10[o] = r10;
    pl.r11[o] = r11;
    pl.lnrho[o] = blocked ? kBlocked : L11;
    if (start) {
      --g;
      piseg[g * I + i] = double2{r00, r01};
      b0 = b1 = 0.0;
    } else {
      const double M = (n1 >= n0) ? n1 : n0;
      const bool fin = M > NGH_NEG_INF;
      b0 = fin ? n0 - M : n0;
      b1 = fin ? n1 - M : n1;
    }
  }
  if (bad) flags[FLAG_INVALID_LKL] = 1;
}

struct FwdArgs {
  const uint64_t* __restrict__ seg;
  uint64_t S, I, base, S_tot;
  uint32_t K;
  const uint32_t* __restrict__ btab;
  const LongestPart* __restrict__ part;
  uint64_t n_part;
  LongestPlanes pl;
  const double2* __restrict__ piseg;
  LongestRings rings;
  const LongestCarry* __restrict__ cin;
  LongestRingIn rin;
  LongestCarry* __restrict__ cout;
  LongestRec* __restrict__ rec;
  uint32_t split;                 // a lane per (individual, segment, threshold)
  int* __restrict__ overflow;     // raised if a ring is ever full at a push
};

template <bool EXACT>
__device__ __forceinline__ double exp_le0(double x) {
  const double y = x < 0.0 ? x : 0.0;
  if constexpr (EXACT) return det_exp(y);
  else return exp_nonpos(y);
}

template <bool EXACT>
__global__ void __launch_bounds__(64)
k_longest_fwd(const FwdArgs A) {
  const uint64_t nib = (A.I + 63) / 64;
  const uint32_t K = A.K;
  // the thresholds [klo, khi) are this lane's: all K, or one when the thresholds have lanes of
  // their own (the same operations on the same values either way)
  const uint64_t gk = blockIdx.x / nib;
  const uint64_t g = A.split ? gk / K : gk;
  const uint32_t klo = A.split ? (uint32_t)(gk % K) : 0u, khi = A.split ? klo + 1 : K;
  const uint64_t i = (blockIdx.x % nib) * 64 + threadIdx.x;
  if (i >= A.I) return;
  const uint64_t a = A.seg[g], b = A.seg[g + 1], I = A.I;
  const bool cont = a == 0 && A.cin != nullptr;   // goes on from the shard before

  double pi0, pi1, Q = 0.0;
  double N[kLongestMaxK], V[kLongestMaxK], H[kLongestMaxK];
  uint32_t ap[kLongestMaxK], cnt[kLongestMaxK], hd[kLongestMaxK], cap[kLongestMaxK];
  double2* ring[kLongestMaxK];
#pragma unroll
  for (uint32_t k = 0; k < kLongestMaxK; ++k) {
    N[k] = V[k] = H[k] = 0.0;
    ap[k] = cnt[k] = hd[k] = 0;
    cap[k] = 1;
    ring[k] = nullptr;
    if (k >= klo && k < khi) {
      cap[k] = A.rings.cap[g * K + k];
      ring[k] = A.rings.ring + A.rings.off[g * K + k] * I + i;
    }
  }
  if (cont) {
    const LongestCarry& c = A.cin[i];
    pi0 = c.pi0;
    pi1 = c.pi1;
    Q = c.q;
#pragma unroll
    for (uint32_t k = 0; k < kLongestMaxK; ++k) {
      if (k >= klo && k < khi) {
        N[k] = c.n[k];
        V[k] = c.v[k];
        H[k] = c.hit[k];
        ap[k] = c.ap[k];
        if (c.cnt[k] > cap[k]) *A.overflow = 1;            // (never: the host sized the ring)
        cnt[k] = c.cnt[k] <= cap[k] ? c.cnt[k] : cap[k];
        const double2* src = A.rin.ring + A.rin.off[k] * I + i;
        uint32_t sl = c.hd[k];
        for (uint32_t j = 0; j < cnt[k]; ++j) {
          ring[k][(uint64_t)j * I] = src[(uint64_t)sl * I];
          sl = sl + 1 == A.rin.cap[k] ? 0 : sl + 1;
        }
      }
    }
  } else {
    const double2 p = A.piseg[g * I + i];
    pi0 = p.x;
    pi1 = p.y;
  }
  // the first part that ends behind the segment's first site
  uint64_t p;
  {
    uint64_t lo = 0, hi = A.n_part;
    const uint64_t ga = A.base + a;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (A.part[mid].end <= ga) lo = mid + 1;
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
      const uint64_t gs = A.base + s;
      if (s != a || cont) {
        const double n0 = pi0 * r00[u] + pi1 * r10[u];
        const double n1 = pi0 * r01[u] + pi1 * r11[u];
        pi0 = n0;
        pi1 = n1;
      }
      if (gs < pb || gs >= pe) continue;
      const bool begin = gs == pb;
      const bool blocked = lr[u] > 0.0;
      const double rho = blocked ? 0.0 : r11[u];
      Q = (begin || blocked) ? 0.0 : Q + lr[u];
#pragma unroll
      for (uint32_t k = 0; k < kLongestMaxK; ++k) {
        if (k >= klo && k < khi) {
          double tau, Nn, Vr;
          if (begin) {
            Nn = pi0;
            tau = pi1;
            Vr = 0.0;
            H[k] = 0.0;
            cnt[k] = 0;
          } else {
            tau = N[k] * r01[u];
            Nn = N[k] * r00[u] + V[k] * r10[u];
            Vr = V[k] * rho;
            if (blocked) cnt[k] = 0;   // those starts can never reach L_k
          }
          const uint32_t* bt = A.btab + (uint64_t)k * A.S_tot;
          const bool push = bt[gs] != kLongestNone;
          if (push && cnt[k] >= cap[k]) *A.overflow = 1;   // (never: the host sized the ring)
          if (push && cnt[k] < cap[k]) {
            if (cnt[k] == 0) {
              hd[k] = 0;
              ap[k] = (uint32_t)gs;
            }
            uint32_t sl = hd[k] + cnt[k];
            sl = sl >= cap[k] ? sl - cap[k] : sl;
            ring[k][(uint64_t)sl * I] = double2{tau, Q};
            ++cnt[k];
          }
          double G = 0.0;
          while (cnt[k] > 0 && bt[ap[k]] == (uint32_t)gs) {
            const double2 e = ring[k][(uint64_t)hd[k] * I];
            G += e.x * exp_le0<EXACT>(Q - e.y);
            hd[k] = hd[k] + 1 == cap[k] ? 0 : hd[k] + 1;
            --cnt[k];
            ++ap[k];
          }
          H[k] += G;
          const double v = (Vr + tau) - G;
          V[k] = v > 0.0 ? v : 0.0;
          N[k] = Nn;
        }
      }
      if (gs + 1 == pe) {   // the part is complete
#pragma unroll
        for (uint32_t k = 0; k < kLongestMaxK; ++k) {
          if (k >= klo && k < khi) {
            A.rec[(i * A.n_part + p) * K + k] = LongestRec{H[k], N[k] + V[k]};
            cnt[k] = 0;
          }
        }
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
  if (b == A.S && A.cout) {
    LongestCarry& c = A.cout[i];
    if (klo == 0) {
      c.pi0 = pi0;
      c.pi1 = pi1;
      c.q = Q;
    }
#pragma unroll
    for (uint32_t k = 0; k < kLongestMaxK; ++k) {
      if (k < klo || k >= khi) continue;
      c.n[k] = N[k];
      c.v[k] = V[k];
      c.hit[k] = H[k];
      c.ap[k] = ap[k];
      c.cnt[k] = cnt[k];
      c.hd[k] = hd[k];
    }
  }
}

}  // namespace

bool longest_fast_bwd(hipStream_t st, const GlView& gl_lin, const double* d_freq, const double* d_pos,
                      const uint64_t* d_seg, uint64_t n_seg, uint64_t S, uint64_t I, const double* d_indF,
                      const double* d_alpha, bool first_is_start, const double* d_win, double* d_wout,
                      const LongestPlanes& pl, double* d_piseg, int* d_flags) {
  const uint64_t grid = n_seg * ((I + 63) / 64);
  if (n_seg == 0 || grid > 0x7fffffffull) return false;
  BwdArgs A;
  A.gl = gl_lin;
  A.freq = d_freq;
  A.pos = d_pos;
  A.seg = d_seg;
  A.S = S;
  A.I = I;
  A.indF = d_indF;
  A.alpha = d_alpha;
  A.first_is_start = first_is_start ? 1u : 0u;
  A.win = d_win;
  A.wout = d_wout;
  A.pl = pl;
  A.piseg = reinterpret_cast<double2*>(d_piseg);
  A.flags = d_flags;
  hipLaunchKernelGGL(k_longest_bwd, dim3((unsigned)grid), dim3(64), 0, st, A);
  return hipGetLastError() == hipSuccess;
}

void launch_longest_bwd_exact(hipStream_t st, const GlView& gl_log, const double* d_freq, const double* pos,
                              uint64_t S, uint64_t I, uint64_t n_seg, const double* d_indF, const double* d_alpha,
                              const LongestPlanes& pl, double* d_piseg, int* d_flags) {
  hipLaunchKernelGGL(k_longest_bwd_exact, dim3((unsigned)((I + 63) / 64)), dim3(64), 0, st, gl_log, d_freq, pos,
                     S, I, n_seg, d_indF, d_alpha, pl, reinterpret_cast<double2*>(d_piseg), d_flags);
}

bool longest_fwd(hipStream_t st, bool exact, bool split, const uint64_t* d_seg, uint64_t n_seg,
                 uint64_t S, uint64_t I, uint64_t base, uint64_t S_tot, uint32_t K, const uint32_t* d_btab,
                 const LongestPart* d_part, uint64_t n_part, const LongestPlanes& pl, const double* d_piseg,
                 const LongestRings& rings, const LongestCarry* d_cin, const LongestRingIn& rin,
                 LongestCarry* d_cout, LongestRec* d_rec, int* d_overflow) {
  if (K < 1 || K > kLongestMaxK) return false;
  const uint64_t grid = n_seg * (split ? K : 1) * ((I + 63) / 64);
  if (n_seg == 0 || grid > 0x7fffffffull) return false;
  FwdArgs A;
  A.split = split ? 1u : 0u;
  A.overflow = d_overflow;
  A.seg = d_seg;
  A.S = S;
  A.I = I;
  A.base = base;
  A.S_tot = S_tot;
  A.K = K;
  A.btab = d_btab;
  A.part = d_part;
  A.n_part = n_part;
  A.pl = pl;
  A.piseg = reinterpret_cast<const double2*>(d_piseg);
  A.rings = rings;
  A.cin = d_cin;
  A.rin = rin;
  A.cout = d_cout;
  A.rec = d_rec;
  if (exact) hipLaunchKernelGGL((k_longest_fwd<true>), dim3((unsigned)grid), dim3(64), 0, st, A);
  else hipLaunchKernelGGL((k_longest_fwd<false>), dim3((unsigned)grid), dim3(64), 0, st, A);
  return hipGetLastError() == hipSuccess;
}

bool longest_split_lanes(uint64_t n_seg, uint64_t I, uint32_t K) {
  return K > 1 && n_seg * ((I + 63) / 64) * K <= kLongestSplitWaves;
}

}  // namespace nghmm
