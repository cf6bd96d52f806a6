// kernels_support.hip -- the joint posterior probability that a whole run of sites [a, b] of one
// individual is in one state (include/nghmm.h: nghmm_tract_support has the definition).
//
// The walk uses the backward ("mirror") form of the conditional product,
//   P(z_a..b = k | y) = P(z_a = k | y) prod_{s = a+1..b} g_s(k),
//   g_s(k) = P(z_s = k | z_{s-1} = k, y_s..) = T_s(k, k) e_s(k) beta_s(k) / beta_{s-1}(k),
// because numerator and denominator of g_s are by-products of the beta step the backward sweep
// makes anyway (beta_{s-1}(k) = c u_k + (1 - c) (q . u), u = e_s beta_s; the numerator is
// (c + (1 - c) q_k) u_k) and T_s is the site's OWN transition: no look at the site to the right,
// so a lane-chunk, and a site shard, needs nothing from its neighbour but the two boundary
// vectors.  Every factor is scale-free; a common factor of the two emissions cancels, so the
// stored ratios rho = e1 / e0 serve.
//   k_support_bounds  the backward vector entering every lane-chunk from the right (the backward
//                     half of k_fast_bounds; the forward half is k_sample_bounds); a site shard
//                     continues the vector of the shard after it;
//   k_support_walk    every lane-chunk that holds a site of a range recomputes its forward vectors
//                     block by block from the checkpoints, as k_fast_bwd_recompute does, carries
//                     the backward vector right to left, and reduces each range's sites inside
//                     the lane-chunk to a PIECE: the two products and the smallest posterior;
//   k_support_finish  one lane per range: its pieces added in site order.
// The products are carried as a double in [0.5, 1) and an integer exponent, rescaled after every
// factor (a factor may be as small as an emission ratio, so eight of them need not fit a double);
// one logarithm per piece and state.  A factor 0 makes the product 0 and the piece -inf; a 0/0
// factor (a state the data already exclude) counts as 0.
// No float atomics: a range is the sum of its pieces in site order, the minimum is taken in site
// order with ties to the lowest site -- the same bits on every call, whatever else is asked for.
// Exact mode: k_support_exact, one lane per individual in log space through detmath.h, with a forward
// array of its own (normalised at every site; see there).
#include "fast_dev.hpp"
#include "kernels_support.hpp"

namespace nghmm {

namespace {

constexpr double LN2 = 0.6931471805599453094;
#define NGH_NEG_INF (-__builtin_huge_val())

__global__ void __launch_bounds__(64)
k_support_bounds(const double* __restrict__ lane_ops, uint64_t J, uint32_t C,
                 const double* __restrict__ win, double* __restrict__ bound,
                 double* __restrict__ wout) {
  const uint64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  const double x0 = win ? win[i * 2] : 1.0, x1 = win ? win[i * 2 + 1] : 1.0;
  const double* ops = lane_ops + (i * J + (uint64_t)lane * C) * 5;
  double* bd = bound + (i * J + (uint64_t)lane * C) * 4;
  constexpr uint32_t PF = 8;
  Op L{1.0, 0.0, 0.0, 1.0, 0};
  for (uint32_t k0 = 0; k0 < C; k0 += PF) {
    Op o[PF];
#pragma unroll
    for (uint32_t u = 0; u < PF; ++u)
      o[u] = op_load(ops + (uint64_t)(k0 + u < C ? k0 + u : C - 1) * 5);
#pragma unroll
    for (uint32_t u = 0; u < PF; ++u)
      if (k0 + u < C) L = op_mul(L, o[u]);
  }
  // product of the lanes to the right
  Op Sx = L;
  for (int off = 1; off < 64; off <<= 1) {
    const Op o = op_shfl_down(Sx, off);
    if (lane + off < 64) Sx = op_mul(Sx, o);
  }
  Op X = op_shfl_down(Sx, 1);
  if (lane == 63) X = Op{1.0, 0.0, 0.0, 1.0, 0};
  double w0 = fma(X.a00, x0, X.a01 * x1), w1 = fma(X.a10, x0, X.a11 * x1);
  int ex = 0;   // (the scale of a boundary vector does not enter a score)
  renorm2(w0, w1, ex);
  for (uint32_t kk0 = C; kk0 > 0; kk0 = kk0 > PF ? kk0 - PF : 0) {
    Op o[PF];  // operators kk0-1, kk0-2, ...
#pragma unroll
    for (uint32_t u = 0; u < PF; ++u)
      o[u] = op_load(ops + (uint64_t)(kk0 > u ? kk0 - 1 - u : 0) * 5);
#pragma unroll
    for (uint32_t u = 0; u < PF; ++u) {
      if (kk0 > u) {
        const uint32_t k = kk0 - 1 - u;
        bd[(uint64_t)k * 4 + 2] = w0;
        bd[(uint64_t)k * 4 + 3] = w1;
        const double n0 = fma(o[u].a00, w0, o[u].a01 * w1);
        const double n1 = fma(o[u].a10, w0, o[u].a11 * w1);
        w0 = n0;
        w1 = n1;
        renorm2(w0, w1, ex);
      }
    }
  }
  if (wout && lane == 0) {
    wout[i * 2] = w0;
    wout[i * 2 + 1] = w1;
  }
}

// a product of factors in [0, 1] as m 2^ex, m in [0.5, 1) or 0
struct LogProd {
  double P = 1.0;
  int ex = 0;
  __device__ __forceinline__ void mul(double f) {
    P *= (f == f) ? f : 0.0;   // 0/0: a state that is excluded already
    const int e = exp_of(P);
    P = __builtin_ldexp(P, -e);
    ex += e;
  }
  __device__ __forceinline__ double log_value() const { return log(P) + (double)ex * LN2; }
  __device__ __forceinline__ void reset() {
    P = 1.0;
    ex = 0;
  }
};

struct WalkArgs {
  const double* __restrict__ e_il;
  const double* __restrict__ pos_il;
  uint64_t T, S;
  uint32_t C;
  const double* __restrict__ indF;
  const double* __restrict__ alpha;
  const double* __restrict__ bound;
  const double2* __restrict__ ckpt;
  const uint64_t* __restrict__ ioff;
  const SupportRange* __restrict__ rec;
  SupportScore* __restrict__ piece;
};

__global__ void __launch_bounds__(64)
k_support_walk(const WalkArgs A) {
  const uint64_t i = blockIdx.x / A.C;
  const uint32_t c = blockIdx.x % A.C;
  const int lane = threadIdx.x;
  const uint64_t T = A.T, S = A.S;
  const uint64_t J = (uint64_t)A.C * 64;
  const uint64_t j = (uint64_t)c * 64 + lane;
  const uint64_t s_base = j * T;

  // the last range of the individual that starts at or in front of the lane-chunk's last site
  const uint64_t r_lo = A.ioff[i], r_hi = A.ioff[i + 1];
  uint64_t r = r_lo;   // ranges [r_lo, r) start in front of the lane-chunk's end
  bool active = false;
  uint64_t rfirst = 0, rlast = 0, rpiece = 0;
  bool rcont = false;
  if (s_base < S && r_lo < r_hi) {
    const uint64_t s_end = (S - s_base < T ? S : s_base + T) - 1;
    uint64_t lo = r_lo, hi = r_hi;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (A.rec[mid].first <= s_end) lo = mid + 1;
      else hi = mid;
    }
    r = lo;
    if (r > r_lo) {
      const SupportRange R = A.rec[r - 1];
      active = R.last >= s_base;
      rfirst = R.first;
      rlast = R.last;
      rpiece = R.piece0;
      rcont = R.cont != 0;
    }
  }
  if (!NGH_ANY(active)) return;   // (no range in any of the wave's 64 lane-chunks)

  const double f = A.indF[i], al = A.alpha[i];
  const double q0 = 1 - f, q1 = f;
  const double* bd = A.bound + (i * J + j) * 4;
  const double vin0 = bd[0], vin1 = bd[1];
  double w0 = bd[2], w1 = bd[3];
  const double* ep = A.e_il + ((i * A.C + c) * T) * 64 + lane;
  const double* dp = A.pos_il + ((uint64_t)c * T) * 64 + lane;
  const uint64_t nblk = T / CK;
  const double2* ck = A.ckpt + ((i * A.C + c) * nblk * 2) * 64 + lane;

  LogProd acc0, acc1;
  double pmin = __builtin_huge_val();
  uint64_t psite = 0;

  double ecur[CK], enxt[CK], dcur[CK], dnxt[CK];
  double2 r0c, r1c, r0n, r1n;
  {
    const uint64_t b = nblk - 1;
#pragma unroll
    for (int u = 0; u < CK; ++u) {
      ecur[u] = ep[(b * CK + u) * 64];
      dcur[u] = dp[(b * CK + u) * 64];
    }
    r0c = b ? ck[(b * 2) * 64] : double2{1.0, 0.0};
    r1c = b ? ck[(b * 2 + 1) * 64] : double2{0.0, 1.0};
  }
  for (uint64_t b = nblk;;) {
    --b;
    if (b > 0) {
      const uint64_t bn = b - 1;
#pragma unroll
      for (int u = 0; u < CK; ++u) {
        enxt[u] = ep[(bn * CK + u) * 64];
        dnxt[u] = dp[(bn * CK + u) * 64];
      }
      r0n = bn ? ck[(bn * 2) * 64] : double2{1.0, 0.0};
      r1n = bn ? ck[(bn * 2 + 1) * 64] : double2{0.0, 1.0};
    }
    // forward vectors of the block's sites, from the checkpoint (as k_fast_bwd_recompute)
    double v0 = fma(vin0, r0c.x, vin1 * r1c.x);
    double v1 = fma(vin0, r0c.y, vin1 * r1c.y);
    double f0[CK], f1[CK], cc[CK];
#pragma unroll
    for (int u = 0; u < CK; ++u) {
      cc[u] = coanc(al, dcur[u]);
      const double a = 1 - cc[u];
      const double sm = v0 + v1;
      v0 = fma(a * q0, sm, cc[u] * v0);
      v1 = fma(a * q1, sm, cc[u] * v1) * ecur[u];
      if (u == CK / 2 - 1) {
        int dummy = 0;
        renorm2(v0, v1, dummy);
      }
      f0[u] = v0;
      f1[u] = v1;
    }
    // backward through the block: the beta step, and in a range its two factors and the posterior
#pragma unroll
    for (int u = CK - 1; u >= 0; --u) {
      const uint64_t s = s_base + b * CK + u;
      const double a = 1 - cc[u];
      const double u0 = w0, u1 = ecur[u] * w1;
      const double sq = a * fma(q0, u0, q1 * u1);
      const double n0 = fma(cc[u], u0, sq), n1 = fma(cc[u], u1, sq);
      if (active && s <= rlast) {   // (s >= rfirst: the range is left as soon as rfirst is done)
        const double x0 = f0[u] * w0, x1 = f1[u] * w1;
        const double rx = rcp_nr2(x0 + x1);
        const double p0 = x0 * rx, p1 = x1 * rx;
        const bool start = s == rfirst && !rcont;
        // T_s(k, k) e_s(k) beta_s(k) / beta_{s-1}(k)
        const double g0 = start ? p0 : fma(a, q0, cc[u]) * u0 * rcp_nr2(n0);
        const double g1 = start ? p1 : fma(a, q1, cc[u]) * u1 * rcp_nr2(n1);
        acc0.mul(g0);
        acc1.mul(g1);
        if (p1 <= pmin) {   // right to left: a tie goes to the lower site
          pmin = p1;
          psite = s;
        }
        if (s == rfirst || s == s_base) {   // the piece is complete
          SupportScore pc;
          pc.log_ibd = acc1.log_value();
          pc.log_non = acc0.log_value();
          pc.post_min = pmin;
          pc.post_min_site = psite;
          A.piece[rpiece + (j - rfirst / T)] = pc;
          acc0.reset();
          acc1.reset();
          pmin = __builtin_huge_val();
          if (s == rfirst) {   // the range in front, if it reaches into the lane-chunk
            --r;
            active = false;
            if (r > r_lo) {
              const SupportRange R = A.rec[r - 1];
              active = R.last >= s_base;
              rfirst = R.first;
              rlast = R.last;
              rpiece = R.piece0;
              rcont = R.cont != 0;
            }
          } else {
            active = false;
          }
        }
      }
      w0 = n0;
      w1 = n1;
    }
    {
      int dummy = 0;
      renorm2(w0, w1, dummy);
    }
    if (b == 0 || !NGH_ANY(active)) break;
#pragma unroll
    for (int u = 0; u < CK; ++u) {
      ecur[u] = enxt[u];
      dcur[u] = dnxt[u];
    }
    r0c = r0n;
    r1c = r1n;
  }
}

// one lane per range: the pieces in site order
__global__ void __launch_bounds__(64)
k_support_finish(const SupportRange* __restrict__ rec, uint64_t n, uint64_t T,
                 const SupportScore* __restrict__ piece, SupportScore* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const SupportRange R = rec[k];
  const uint64_t np = support_pieces(R.first, R.last, T);
  SupportScore acc = piece[R.piece0];
  for (uint64_t p = 1; p < np; ++p) {
    const SupportScore pc = piece[R.piece0 + p];
    acc.log_ibd += pc.log_ibd;
    acc.log_non += pc.log_non;
    if (pc.post_min < acc.post_min) {   // ascending sites: a tie stays with the lower one
      acc.post_min = pc.post_min;
      acc.post_min_site = pc.post_min_site;
    }
  }
  out[k] = acc;
}

// gen_func.cpp:135-151 for two values, through detmath.h
__device__ __forceinline__ double lsum2(double a0, double a1) {
  const double M = (a1 >= a0) ? a1 : a0;
  if (M == NGH_NEG_INF) return NGH_NEG_INF;
  return det_log(det_exp(a0 - M) + det_exp(a1 - M)) + M;
}
__device__ __forceinline__ double nan_to_minf(double v) { return v == v ? v : NGH_NEG_INF; }

// a sum of logarithms with its rounding error carried along (TwoSum): a range of a thousand sites
// adds a thousand terms to a sum of a few hundred, and plain addition would lose ulp(sum) each time.
// A term -inf (or NaN: 0/0, a state that is excluded already) makes the sum -inf.
struct LogSum {
  double s = 0.0, c = 0.0;
  bool dead = false;
  __device__ __forceinline__ void add(double v) {
    if (!(v > NGH_NEG_INF)) {
      dead = true;
      return;
    }
    const double t = s + v, bv = t - s;
    c += (s - (t - bv)) + (v - bv);
    s = t;
  }
  __device__ __forceinline__ double value() const { return dead ? NGH_NEG_INF : s + c; }
};

// exact mode: eprob [S][I][2] log emissions; fw [S + 1][I][2] is scratch for the forward values
// (fw[s + 1] = site s).  The lane first fills its own column of fw with the log-space forward
// recursion of k_forward_exact, but with the larger of the two entries subtracted after every site,
// and carries the backward vector the same way.  The unnormalised array of launch_forward_exact will
// not do here: its entries reach ln f = -thousands, so each carries a rounding error of
// ulp(|ln f|) ~ 1e-12 that the difference of the two states, which is all a posterior needs, keeps.
// With both vectors normalised every term below is a sum of numbers of the size of one emission.
__global__ void __launch_bounds__(64)
k_support_exact(const double* __restrict__ eprob, const double* __restrict__ pos,
                double* __restrict__ fw, uint64_t S, uint64_t I,
                const double* __restrict__ indF, const double* __restrict__ alpha,
                const uint64_t* __restrict__ ioff, const SupportRange* __restrict__ rec,
                SupportScore* __restrict__ out, int* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  const uint64_t r_lo = ioff[i];
  uint64_t r = ioff[i + 1];
  if (r == r_lo) return;
  const double f = indF[i], al = alpha[i];
  const double q0 = 1 - f, q1 = f;
  SupportRange R = rec[r - 1];
  const uint64_t s_stop = rec[r_lo].first, s_top = R.last;
  {
    double p0 = det_log(q0), p1 = det_log(q1);
    bool bad = false;
    for (uint64_t s = 0; s <= s_top; ++s) {
      const double d = pos[s];
      const double cs = d < kDStart ? det_exp(-al * d) : 0.0;   // (as k_sample_exact)
      const double a = 1 - cs;
      const double t00 = det_log(a * q0 + cs), t01 = det_log(a * q1);
      const double t10 = det_log(a * q0), t11 = det_log(a * q1 + cs);
      double c0 = lsum2(p0 + t00, p1 + t10) + eprob[(s * I + i) * 2];
      double c1 = lsum2(p0 + t01, p1 + t11) + eprob[(s * I + i) * 2 + 1];
      bad |= (c0 != c0) | (c1 != c1);
      const double M = (c1 >= c0) ? c1 : c0;
      if (M > NGH_NEG_INF) {
        c0 -= M;
        c1 -= M;
      }
      fw[((s + 1) * I + i) * 2] = c0;
      fw[((s + 1) * I + i) * 2 + 1] = c1;
      p0 = c0;
      p1 = c1;
    }
    if (bad) flags[FLAG_INVALID_LKL] = 1;
  }
  double b0 = 0.0, b1 = 0.0;   // log beta of the last site
  LogSum sum0, sum1;
  double pmin = __builtin_huge_val();
  uint64_t psite = 0;
  for (uint64_t s = S; s-- > s_stop;) {
    const double d = pos[s];
    const double cs = d < kDStart ? det_exp(-al * d) : 0.0;
    const double a = 1 - cs;
    const double t00 = det_log(a * q0 + cs), t01 = det_log(a * q1);
    const double t10 = det_log(a * q0), t11 = det_log(a * q1 + cs);
    const double u0 = eprob[(s * I + i) * 2] + b0, u1 = eprob[(s * I + i) * 2 + 1] + b1;
    const double n0 = lsum2(t00 + u0, t01 + u1);
    const double n1 = lsum2(t10 + u0, t11 + u1);
    if (r > r_lo && s <= R.last) {
      const double l0 = fw[((s + 1) * I + i) * 2] + b0, l1 = fw[((s + 1) * I + i) * 2 + 1] + b1;
      const double lz = lsum2(l0, l1);
      const bool start = s == R.first;
      sum0.add(start ? l0 - lz : t00 + u0 - n0);
      sum1.add(start ? l1 - lz : t11 + u1 - n1);
      const double p1 = det_exp(l1 - lz);
      if (p1 <= pmin) {
        pmin = p1;
        psite = s;
      }
      if (start) {
        out[r - 1] = SupportScore{sum1.value(), sum0.value(), pmin, psite};
        sum0 = LogSum{};
        sum1 = LogSum{};
        pmin = __builtin_huge_val();
        --r;
        if (r > r_lo) R = rec[r - 1];
      }
    }
    const double M = (n1 >= n0) ? n1 : n0;
    const bool fin = M > NGH_NEG_INF;
    b0 = fin ? n0 - M : n0;
    b1 = fin ? n1 - M : n1;
  }
}

}  // namespace

bool support_fast_bounds(FastState& fs, hipStream_t st, const double* d_win, double* d_wout) {
  hipLaunchKernelGGL(k_support_bounds, dim3((unsigned)fs.I), dim3(64), 0, st, fs.lane_ops, fs.J, fs.C,
                     d_win, fs.bound, d_wout);
  return hipGetLastError() == hipSuccess;
}

bool support_fast_walk(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                       const uint64_t* d_ioff, const SupportRange* d_rec, uint64_t n,
                       SupportScore* d_piece, SupportScore* d_out) {
  if (n == 0) return true;
  if (fs.T == 0 || fs.T % CK != 0) return false;
  WalkArgs A;
  A.e_il = fs.e_il;
  A.pos_il = fs.pos_il;
  A.T = fs.T;
  A.S = fs.S;
  A.C = fs.C;
  A.indF = d_indF;
  A.alpha = d_alpha;
  A.bound = fs.bound;
  A.ckpt = reinterpret_cast<const double2*>(fs.ckpt);
  A.ioff = d_ioff;
  A.rec = d_rec;
  A.piece = d_piece;
  hipLaunchKernelGGL(k_support_walk, dim3((unsigned)(fs.I * fs.C)), dim3(64), 0, st, A);
  hipLaunchKernelGGL(k_support_finish, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, d_rec, n, fs.T,
                     d_piece, d_out);
  return hipGetLastError() == hipSuccess;
}

void launch_support_exact(hipStream_t st, const double* eprob, const double* pos, double* fw,
                          uint64_t S, uint64_t I, const double* d_indF, const double* d_alpha,
                          const uint64_t* d_ioff, const SupportRange* d_rec, SupportScore* d_out,
                          int* d_flags) {
  hipLaunchKernelGGL(k_support_exact, dim3((unsigned)((I + 63) / 64)), dim3(64), 0, st, eprob, pos, fw,
                     S, I, d_indF, d_alpha, d_ioff, d_rec, d_out, d_flags);
}

}  // namespace nghmm
