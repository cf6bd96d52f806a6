// kernels_freqinfo.hip -- the log-likelihood of the cohort as a function of ONE site's allele
// frequency, everything else held at the handle's current values (include/nghmm.h:
// nghmm_freq_info has the definition).
//
// Z_i is linear in the two emissions of site s: Z_i = C_i [(1 - c_is) e0_is(f) + c_is e1_is(f)] with
// the CAVITY probability c_is = P(z_is = 1 | all data of i except site s's), which is
// (alpha_{s-1} T_s)(k) beta_s(k) normalised over k: the forward prediction BEFORE the site's own
// emission is applied, times the backward vector.
//
// The results are the same BITS however the sites are cut into shards and whatever the handle's
// layout is.  That rules out the lane-chunk operators and checkpoints of the E-step (a vector that
// is a product of 2 x 2 operators is rounded along the grouping of that product, which belongs to
// a layout), so the two walks here are plain vector recursions, one site after the other, in
// linear space on the site-major likelihoods and frequencies:
//   k_freq_fwd    one lane per (individual, SEGMENT); a segment is the part of a chromosome that
//                 the handle holds.  A chromosome's first site restarts the recursion exactly -- its
//                 prediction is DEFINED as (1 - F, F), the scale of a vector being free --, so the
//                 segments are independent, and a segment that goes on from the shard before starts
//                 from that shard's last vector, bit for bit.  Leaves every site's prediction.
//   k_freq_bwd    the same lanes right to left: beta in front of a chromosome start is DEFINED as
//                 (1, 1); per cell the two weights (1 - c, c), each from its own product
//                 prediction(k) beta(k) (neither is 1 minus the other), in place of the prediction.
// Both vectors are rescaled after every site by the power of two that brings their larger entry
// into [0.5, 1): exact, and decided by the values alone, so a shard's vectors are the single
// handle's including their scale, and prediction(k) beta(k) cannot underflow.
//   k_freq_sites  the site pass: a wave owns 8 adjacent sites and goes through the individuals in
//                 blocks of 64, weights and likelihoods both site-major (64 adjacent cells per
//                 site).  Per cell the two brackets' values and derivatives and one logarithm per
//                 level.  A site's sums: within a block of 64 individuals (filled up with zeros) a
//                 butterfly -- x_i += x_{i ^ 32}, then ^ 16, 8, 4, 2, 1 --, the blocks added in
//                 order, the first one's value first (the rule of nghmm_ibd_summary's post_sum).
// No atomics, one order of operations: the same bits on every call, whatever is asked for.
// Exact mode: k_freq_exact, one lane per individual in log space through detmath.h with the
// normalised forward array of k_support_exact; the same site pass.
#include "fast_dev.hpp"
#include "kernels_freqinfo.hpp"

namespace nghmm {

namespace {

#define NGH_NEG_INF (-__builtin_huge_val())

// the two emissions of a cell at frequency f: e0 = p0 (1 - f)^2 + 2 p1 f (1 - f) + p2 f^2 and
// e1 = p0 (1 - f) + p2 f (calc_emission with calc_HWE's F = 0 and F = 1, in linear space)
__device__ __forceinline__ void emissions(double p0, double p1, double p2, double f, double& e0, double& e1) {
  const double om = 1 - f;
  e0 = fma(p0, om * om, fma(p1, 2 * (om * f), p2 * (f * f)));
  e1 = fma(p0, om, p2 * f);
}

// the larger entry into [0.5, 1): a power of two, so exact, and decided by the values alone
__device__ __forceinline__ void rescale2(double& v0, double& v1) {
  int ex = 0;
  renorm2(v0, v1, ex);
}

constexpr int kBatch = 8;   // sites whose loads are in flight together

struct SeqArgs {
  GlView gl;                          // linear likelihoods, site-major [S][I] cells
  const double* __restrict__ freq;    // [S]
  const double* __restrict__ pos;     // [S] distances; +inf: a chromosome start
  const uint64_t* __restrict__ seg;   // [n_seg + 1] first sites of the segments, then S
  uint64_t S, I;
  const double* __restrict__ indF;
  const double* __restrict__ alpha;
  const double* __restrict__ vin;     // [I][2] or null
  double* __restrict__ vout;          // [I][2] or null
  double2* __restrict__ cav;          // [S][I]
  int* __restrict__ flags;
};

// vin: the forward vector after the last site of the shard before (null: the handle holds the first
// site of the data, and the recursion starts from (1 - F, F)); vout: the one after this handle's
// last site
__global__ void __launch_bounds__(64)
k_freq_fwd(const SeqArgs A) {
  const uint64_t nib = (A.I + 63) / 64;
  const uint64_t g = blockIdx.x / nib;
  const uint64_t i = (blockIdx.x % nib) * 64 + threadIdx.x;
  if (i >= A.I) return;
  const uint64_t a = A.seg[g], b = A.seg[g + 1], I = A.I;
  const double f = A.indF[i], al = A.alpha[i];
  const double q0 = 1 - f, q1 = f;
  double v0 = q0, v1 = q1;
  if (a == 0 && A.vin) {
    v0 = A.vin[i * 2];
    v1 = A.vin[i * 2 + 1];
  }
  // kBatch sites at a time: everything that does not depend on the vector -- the loads, the
  // coancestry, the two emissions -- first, so that the loads of a batch are in flight together
  // and the dependent chain of a site is the transition, two products and the rescaling.  The
  // operations of a site and their order do not depend on where a batch begins.
  for (uint64_t s0 = a; s0 < b; s0 += kBatch) {
    double cc[kBatch], e0[kBatch], e1[kBatch];
    bool start[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const uint64_t s = s0 + u;
      cc[u] = e0[u] = e1[u] = 0.0;
      start[u] = true;
      if (s < b) {
        const double d = A.pos[s];
        start[u] = !(d < kDStart);
        if (!start[u]) cc[u] = coanc(al, d);
        double p0, p1, p2;
        gl_fetch(A.gl, s * I + i, p0, p1, p2);
        emissions(p0, p1, p2, A.freq[s], e0[u], e1[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const uint64_t s = s0 + u;
      if (s < b) {
        double n0 = q0, n1 = q1;   // a chromosome start
        if (!start[u]) {
          const double om = 1 - cc[u], sm = v0 + v1;
          n0 = fma(om * q0, sm, cc[u] * v0);
          n1 = fma(om * q1, sm, cc[u] * v1);
        }
        A.cav[s * I + i] = double2{n0, n1};
        v0 = n0 * e0[u];
        v1 = n1 * e1[u];
        rescale2(v0, v1);
      }
    }
  }
  if (b == A.S && A.vout) {
    A.vout[i * 2] = v0;
    A.vout[i * 2 + 1] = v1;
  }
}

// vin here: the backward vector at the handle's last site (null: (1, 1)); vout: the one at the
// last site of the shard before, (1, 1) where this handle's first site starts a chromosome
__global__ void __launch_bounds__(64)
k_freq_bwd(const SeqArgs A) {
  const uint64_t nib = (A.I + 63) / 64;
  const uint64_t g = blockIdx.x / nib;
  const uint64_t i = (blockIdx.x % nib) * 64 + threadIdx.x;
  if (i >= A.I) return;
  const uint64_t a = A.seg[g], b = A.seg[g + 1], I = A.I;
  const double f = A.indF[i], al = A.alpha[i];
  const double q0 = 1 - f, q1 = f;
  double w0 = 1.0, w1 = 1.0;   // the data's end, or a chromosome start at site b
  if (b == A.S && A.vin) {
    w0 = A.vin[i * 2];
    w1 = A.vin[i * 2 + 1];
  }
  bool bad = false;
  for (uint64_t hi = b; hi > a;) {   // batches as in k_freq_fwd, right to left
    const uint64_t lo = hi - a >= (uint64_t)kBatch ? hi - kBatch : a;
    double cc[kBatch], e0[kBatch], e1[kBatch];
    double2 pr[kBatch];
    bool start[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const uint64_t s = lo + u;
      cc[u] = e0[u] = e1[u] = 0.0;
      pr[u] = double2{0.0, 0.0};
      start[u] = true;
      if (s < hi) {
        pr[u] = A.cav[s * I + i];
        const double d = A.pos[s];
        start[u] = !(d < kDStart);
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
        const double x0 = pr[u].x * w0, x1 = pr[u].y * w1;
        const double rx = rcp_nr2(x0 + x1);
        const double c0 = x0 * rx, c1 = x1 * rx;
        bad |= (c0 != c0) | (c1 != c1);
        A.cav[s * I + i] = double2{c0, c1};
        if (!start[u]) {
          const double om = 1 - cc[u];
          const double u0 = e0[u] * w0, u1 = e1[u] * w1;
          const double sq = om * fma(q0, u0, q1 * u1);
          w0 = fma(cc[u], u0, sq);
          w1 = fma(cc[u], u1, sq);
          rescale2(w0, w1);
        } else {
          w0 = w1 = 1.0;
        }
      }
    }
    hi = lo;
  }
  if (a == 0 && A.vout) {
    A.vout[i * 2] = w0;
    A.vout[i * 2 + 1] = w1;
  }
  if (bad) A.flags[FLAG_INVALID_LKL] = 1;
}

// gen_func.cpp:135-151 for two values, through detmath.h (as kernels_support.hip)
__device__ __forceinline__ double lsum2(double a0, double a1) {
  const double M = (a1 >= a0) ? a1 : a0;
  if (M == NGH_NEG_INF) return NGH_NEG_INF;
  return det_log(det_exp(a0 - M) + det_exp(a1 - M)) + M;
}

// the two log emissions of a cell of LOG likelihoods at frequency f, through detmath.h: formed
// here from the current frequencies, so that the walk and the site pass see the same ones
__device__ __forceinline__ void log_emissions(const GlView& gl, uint64_t cell, double f, double& le0,
                                              double& le1) {
  double g0, g1, g2, e0, e1;
  gl_fetch(gl, cell, g0, g1, g2);
  emissions(det_exp(g0), det_exp(g1), det_exp(g2), f, e0, e1);
  le0 = e0 > 0.0 ? det_log(e0) : (e0 == 0.0 ? NGH_NEG_INF : e0 * 0.0 / 0.0);
  le1 = e1 > 0.0 ? det_log(e1) : (e1 == 0.0 ? NGH_NEG_INF : e1 * 0.0 / 0.0);
}

// exact mode: gl the LOG likelihoods [S][I] cells; fw [S + 1][I][2] is scratch for the forward
// values (fw[s + 1] = site s), normalised at every site like the backward vector (k_support_exact
// says why).  cav [S][I] cells.
__global__ void __launch_bounds__(64)
k_freq_exact(const GlView gl, const double* __restrict__ freq, const double* __restrict__ pos,
             double* __restrict__ fw, uint64_t S, uint64_t I, const double* __restrict__ indF,
             const double* __restrict__ alpha, double2* __restrict__ cav, int* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  const double f = indF[i], al = alpha[i];
  const double q0 = 1 - f, q1 = f;
  const double lq0 = det_log(q0), lq1 = det_log(q1);
  bool bad = false;
  {
    double p0 = lq0, p1 = lq1;
    for (uint64_t s = 0; s < S; ++s) {
      const double d = pos[s];
      const double cs = d < kDStart ? det_exp(-al * d) : 0.0;   // (as k_sample_exact)
      const double a = 1 - cs;
      const double t00 = det_log(a * q0 + cs), t01 = det_log(a * q1);
      const double t10 = det_log(a * q0), t11 = det_log(a * q1 + cs);
      double le0, le1;
      log_emissions(gl, s * I + i, freq[s], le0, le1);
      double c0 = lsum2(p0 + t00, p1 + t10) + le0;
      double c1 = lsum2(p0 + t01, p1 + t11) + le1;
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
  }
  double b0 = 0.0, b1 = 0.0;   // log beta of the last site
  for (uint64_t s = S; s-- > 0;) {
    const double d = pos[s];
    const double cs = d < kDStart ? det_exp(-al * d) : 0.0;
    const double a = 1 - cs;
    const double t00 = det_log(a * q0 + cs), t01 = det_log(a * q1);
    const double t10 = det_log(a * q0), t11 = det_log(a * q1 + cs);
    // the prediction of site s from the forward vector of the site before
    const double p0 = s ? fw[(s * I + i) * 2] : lq0, p1 = s ? fw[(s * I + i) * 2 + 1] : lq1;
    const double l0 = lsum2(p0 + t00, p1 + t10) + b0, l1 = lsum2(p0 + t01, p1 + t11) + b1;
    const double lz = lsum2(l0, l1);
    const double c0 = det_exp(l0 - lz), c1 = det_exp(l1 - lz);
    bad |= (c0 != c0) | (c1 != c1);
    cav[s * I + i] = double2{c0, c1};
    double le0, le1;
    log_emissions(gl, s * I + i, freq[s], le0, le1);
    const double u0 = le0 + b0, u1 = le1 + b1;
    const double n0 = lsum2(t00 + u0, t01 + u1);
    const double n1 = lsum2(t10 + u0, t11 + u1);
    const double M = (n1 >= n0) ? n1 : n0;
    const bool fin = M > NGH_NEG_INF;
    b0 = fin ? n0 - M : n0;
    b1 = fin ? n1 - M : n1;
  }
  if (bad) flags[FLAG_INVALID_LKL] = 1;
}

// ---- the site pass ----
constexpr int kSitesPerWave = 8;
constexpr int kNVal = 3 + (int)FREQINFO_MAX_LEVELS;   // ll, score, info, the curve

struct SiteArgs {
  const double2* __restrict__ cav;
  GlView gl;
  const double* __restrict__ freq;
  uint64_t S, I;
  FreqLevels lv;
  FreqStat* __restrict__ stats;
  double* __restrict__ curve;
};

__device__ __forceinline__ double bracket(double w0, double w1, double p0, double p1, double p2, double f) {
  double e0, e1;
  emissions(p0, p1, p2, f, e0, e1);
  return fma(w0, e0, w1 * e1);
}

// A wave per 8 adjacent sites.  LOGGL: the view holds log likelihoods.  The running sums of the
// wave's sites live in LDS (lane 0 adds a block's butterfly sum to them), so that the loop over the
// levels need not be unrolled.
template <bool LOGGL>
__global__ void __launch_bounds__(64)
k_freq_sites(const SiteArgs A) {
  __shared__ double acc[kSitesPerWave][kNVal];
  const uint32_t lane = threadIdx.x;
  const uint64_t S = A.S, I = A.I;
  const uint64_t s_first = (uint64_t)blockIdx.x * kSitesPerWave;
  const uint64_t nib = (I + 63) / 64;
  for (uint64_t ib = 0; ib < nib; ++ib) {
    const uint64_t i = ib * 64 + lane;
    const bool live = i < I;
#pragma unroll 1
    for (uint32_t l = 0; l < (uint32_t)kSitesPerWave; ++l) {
      const uint64_t s = s_first + l;
      if (s >= S) break;   // (wave-uniform)
      const double f = A.freq[s];
      double p0 = 0.0, p1 = 0.0, p2 = 0.0;
      double2 w{0.0, 0.0};
      if (live) {
        gl_fetch(A.gl, s * I + i, p0, p1, p2);
        if (LOGGL) {
          p0 = exp(p0);
          p1 = exp(p1);
          p2 = exp(p2);
        }
        w = A.cav[s * I + i];
      }
      // the block's butterfly sum of one quantity (a lane past the last individual adds 0), added
      // to the site's running sum: the blocks in order, the first one's value first
      auto put = [&](uint32_t q, double v) {
        const double sum = wave_sum(live ? v : 0.0);
        if (lane == 0) acc[l][q] = ib == 0 ? sum : acc[l][q] + sum;
      };
      const double om = 1 - f;
      const double B = bracket(w.x, w.y, p0, p1, p2, f);
      // d/df and d2/df2 of the two emissions (e1'' = 0)
      const double d0 = 2 * fma(p2, f, fma(p1, om - f, -(p0 * om)));
      const double d1 = p2 - p0;
      const double dd0 = 2 * ((p0 + p2) - 2 * p1);
      const double u = fma(w.x, d0, w.y * d1) / B;
      put(0, log(B));
      put(1, u);
      put(2, fma(u, u, -(w.x * dd0 / B)));
#pragma unroll 1
      for (uint32_t k = 0; k < A.lv.n; ++k)
        put(3 + k, log(bracket(w.x, w.y, p0, p1, p2, A.lv.f[k]) / B));
    }
  }
  __syncthreads();
  if (lane < (uint32_t)kSitesPerWave) {
    const uint64_t s = s_first + lane;
    if (s < S) {
      // a bracket that is 0 at the current frequency: ll = -inf, and nothing else is defined
      const double ll = acc[lane][0];
      const bool dead = ll == NGH_NEG_INF;   // (a NaN is not hidden: it stays in the record)
      const double nan = __builtin_nan("");
      A.stats[s] = FreqStat{A.freq[s], dead ? NGH_NEG_INF : ll, dead ? nan : acc[lane][1],
                            dead ? nan : acc[lane][2]};
      for (uint32_t k = 0; k < A.lv.n; ++k) A.curve[s * A.lv.n + k] = dead ? nan : acc[lane][3 + k];
    }
  }
}

// out [I][S] = the second weight of cav [S][I]: a 32 x 32 tile through LDS, so that the 16 B reads
// run along the individuals and the 8 B writes along the sites
__global__ void __launch_bounds__(256)
k_freq_cavity_out(const double2* __restrict__ cav, uint64_t S, uint64_t I, double* __restrict__ out) {
  __shared__ double tile[32][33];
  const uint64_t nti = (I + 31) / 32;
  const uint64_t s0 = (blockIdx.x / nti) * 32, i0 = (blockIdx.x % nti) * 32;
  const uint32_t x = threadIdx.x % 32, y = threadIdx.x / 32;   // y < 8
  for (uint32_t r = y; r < 32; r += 8)
    if (s0 + r < S && i0 + x < I) tile[r][x] = cav[(s0 + r) * I + i0 + x].y;
  __syncthreads();
  for (uint32_t r = y; r < 32; r += 8)
    if (i0 + r < I && s0 + x < S) out[(i0 + r) * S + s0 + x] = tile[x][r];
}

}  // namespace

bool freqinfo_fast_walks(hipStream_t st, const GlView& gl_lin, const double* d_freq, const double* d_pos,
                         const uint64_t* d_seg, uint64_t n_seg, uint64_t S, uint64_t I,
                         const double* d_indF, const double* d_alpha, const double* d_vin,
                         double* d_vout, const double* d_win, double* d_wout, double* d_cav,
                         int* d_flags, bool backward) {
  const uint64_t grid = n_seg * ((I + 63) / 64);
  if (n_seg == 0 || grid > 0x7fffffffull) return false;
  SeqArgs A;
  A.gl = gl_lin;
  A.freq = d_freq;
  A.pos = d_pos;
  A.seg = d_seg;
  A.S = S;
  A.I = I;
  A.indF = d_indF;
  A.alpha = d_alpha;
  A.cav = reinterpret_cast<double2*>(d_cav);
  A.flags = d_flags;
  if (!backward) {
    A.vin = d_vin;
    A.vout = d_vout;
    hipLaunchKernelGGL(k_freq_fwd, dim3((unsigned)grid), dim3(64), 0, st, A);
  } else {
    A.vin = d_win;
    A.vout = d_wout;
    hipLaunchKernelGGL(k_freq_bwd, dim3((unsigned)grid), dim3(64), 0, st, A);
  }
  return hipGetLastError() == hipSuccess;
}

void launch_freqinfo_exact(hipStream_t st, const GlView& gl_log, const double* d_freq, const double* pos,
                           double* fw, uint64_t S, uint64_t I, const double* d_indF,
                           const double* d_alpha, double* d_cav, int* d_flags) {
  hipLaunchKernelGGL(k_freq_exact, dim3((unsigned)((I + 63) / 64)), dim3(64), 0, st, gl_log, d_freq, pos, fw, S, I,
                     d_indF, d_alpha, reinterpret_cast<double2*>(d_cav), d_flags);
}

bool freqinfo_sites(hipStream_t st, const double* d_cav, const GlView& gl, bool log_gl,
                    const double* d_freq, uint64_t S, uint64_t I, const FreqLevels& lv,
                    FreqStat* d_stats, double* d_curve) {
  if (lv.n > FREQINFO_MAX_LEVELS) return false;
  SiteArgs A;
  A.cav = reinterpret_cast<const double2*>(d_cav);
  A.gl = gl;
  A.freq = d_freq;
  A.S = S;
  A.I = I;
  A.lv = lv;
  A.stats = d_stats;
  A.curve = d_curve;
  const uint64_t grid = (S + kSitesPerWave - 1) / kSitesPerWave;
  if (grid > 0x7fffffffull) return false;
  if (log_gl) hipLaunchKernelGGL((k_freq_sites<true>), dim3((unsigned)grid), dim3(64), 0, st, A);
  else hipLaunchKernelGGL((k_freq_sites<false>), dim3((unsigned)grid), dim3(64), 0, st, A);
  return hipGetLastError() == hipSuccess;
}

bool freqinfo_cavity_out(hipStream_t st, const double* d_cav, uint64_t S, uint64_t I, double* d_out) {
  const uint64_t g = ((S + 31) / 32) * ((I + 31) / 32);
  if (g == 0 || g > 0x7fffffffull) return false;
  const dim3 grid((unsigned)g);
  hipLaunchKernelGGL(k_freq_cavity_out, grid, dim3(256), 0, st, reinterpret_cast<const double2*>(d_cav), S, I,
                     d_out);
  return hipGetLastError() == hipSuccess;
}

}  // namespace nghmm
