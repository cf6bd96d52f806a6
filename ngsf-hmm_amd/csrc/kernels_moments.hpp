// kernels_moments.hpp -- exact posterior means and covariances of (IBD sites or IBD Mb, number of
// tracts) per individual and region (kernels_moments.hip): the centred jet, what closes a region,
// and the host interface.  include/nghmm.h (nghmm_ibd_moments) has the definition.
//
// The likelihood tilted by the two path statistics, Z(t) = sum_z P(z, y) exp(t_A A(z) + t_T T(z)),
// is a product of 2x2 operators like the likelihood itself, and the t-derivatives of a site's
// operator are entrywise masks of it.  The product rule to second order in two variables is the Jet
// of kernels_info.hpp, read as (V, V_A, V_T, V_AA, V_AT, V_TT).  A plain jet loses digits when it is
// closed (Z_AA / Z - (Z_A / Z)^2 cancels like eps E[A]^2 / Var), so a piece carries, next to its
// jet, an OFFSET (d_A, d_T): the jet is that of the statistics minus the offsets.  A product adds
// the offsets and re-centres (cjet_recentre) wherever jet_renorm runs, which keeps the first-order
// components of the order of the statistics' spread times the value.  Closing gives the means as
// offset + Z_a / Z and the covariances unchanged.  Everything that forms a product or closes it is
// __host__ __device__: a chain's host multiplies its shards' jets with the routine the device uses.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_fast.hpp"
#include "kernels_info.hpp"

namespace nghmm {

enum { CJ_V = JET_V, CJ_A = JET_F, CJ_T = JET_A, CJ_AA = JET_FF, CJ_AT = JET_FA, CJ_TT = JET_AA };

struct CJet {
  Jet j;
  double da, dt;   // the offsets of the two statistics
};
// a centred jet in memory: the jet (24 entries, the exponent), the two offsets
constexpr int kCJetDoubles = kJetDoubles + 2;

// the five doubles of nghmm_moment_region
struct MomentRec {
  double mean_a, mean_t, var_a, cov_at, var_t;
};
static_assert(sizeof(MomentRec) == 40, "nghmm_moment_region is 40 bytes");

__host__ __device__ inline CJet cjet_identity() {
  CJet c;
  c.j = jet_identity();
  c.da = c.dt = 0.0;
  return c;
}

// moves the offsets by the first-order components' share of the value (sums over the four
// entries): the statistics' means under equal weights at both ends
__host__ __device__ inline void cjet_recentre(CJet& c) {
  double (*m)[4] = c.j.m;
  const double sv = (m[CJ_V][0] + m[CJ_V][1]) + (m[CJ_V][2] + m[CJ_V][3]);
  if (!(sv > 0.0)) return;   // (a piece no path passes: nothing to centre)
  const double iv = 1.0 / sv;
  const double ua = ((m[CJ_A][0] + m[CJ_A][1]) + (m[CJ_A][2] + m[CJ_A][3])) * iv;
  const double ut = ((m[CJ_T][0] + m[CJ_T][1]) + (m[CJ_T][2] + m[CJ_T][3])) * iv;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double v = m[CJ_V][q], a = m[CJ_A][q], t = m[CJ_T][q];
    m[CJ_AA][q] = fma(ua * ua, v, fma(-2.0 * ua, a, m[CJ_AA][q]));
    m[CJ_AT][q] = fma(ua * ut, v, fma(-ua, t, fma(-ut, a, m[CJ_AT][q])));
    m[CJ_TT][q] = fma(ut * ut, v, fma(-2.0 * ut, t, m[CJ_TT][q]));
    m[CJ_A][q] = fma(-ua, v, a);
    m[CJ_T][q] = fma(-ut, v, t);
  }
  c.da += ua;
  c.dt += ut;
}

// L applied first, then R
__host__ __device__ inline CJet cjet_mul(const CJet& L, const CJet& R) {
  CJet o;
  o.j = jet_mul(L.j, R.j);
  o.da = L.da + R.da;
  o.dt = L.dt + R.dt;
  cjet_recentre(o);
  return o;
}

// p[(k) * stride], k < kCJetDoubles
__host__ __device__ inline CJet cjet_load(const double* p, uint64_t stride) {
  CJet c;
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) c.j.m[k][q] = p[(uint64_t)(k * 4 + q) * stride];
  c.j.ex = (int)p[24 * stride];
  c.da = p[25 * stride];
  c.dt = p[26 * stride];
  return c;
}
__host__ __device__ inline void cjet_store(double* p, uint64_t stride, const CJet& c) {
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) p[(uint64_t)(k * 4 + q) * stride] = c.j.m[k][q];
  p[24 * stride] = (double)c.j.ex;
  p[25 * stride] = c.da;
  p[26 * stride] = c.dt;
}

// The record of a region's product P between the forward vector f before the region and the
// backward vector b after it (any scale): Z_x = f P_x b, mean = offset + Z_a / Z,
// cov_ab = Z_ab / Z - (Z_a / Z)(Z_b / Z); a variance that rounds below 0 is 0.
__host__ __device__ inline MomentRec cjet_close(const CJet& P, double f0, double f1, double b0, double b1) {
  double z[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double* m = P.j.m[k];
    z[k] = fma(f0, fma(m[0], b0, m[1] * b1), f1 * fma(m[2], b0, m[3] * b1));
  }
  MomentRec r{P.da, P.dt, 0.0, 0.0, 0.0};
  if (!(z[CJ_V] > 0.0)) return r;
  const double iz = 1.0 / z[CJ_V];
  const double ga = z[CJ_A] * iz, gt = z[CJ_T] * iz;
  r.mean_a = P.da + ga;
  r.mean_t = P.dt + gt;
  r.var_a = fma(-ga, ga, z[CJ_AA] * iz);
  r.cov_at = fma(-ga, gt, z[CJ_AT] * iz);
  r.var_t = fma(-gt, gt, z[CJ_TT] * iz);
  if (!(r.var_a > 0.0)) r.var_a = 0.0;
  if (!(r.var_t > 0.0)) r.var_t = 0.0;
  return r;
}

// v M for the value component, scaled to entries that add up to 1 (left as it is when they
// vanish): how the forward and backward vectors pass a segment
__host__ __device__ inline void moments_fwd(const Jet& P, double& f0, double& f1) {
  const double* m = P.m[CJ_V];
  const double g0 = fma(f0, m[0], f1 * m[2]), g1 = fma(f0, m[1], f1 * m[3]);
  const double s = g0 + g1;
  const double is = s > 0.0 ? 1.0 / s : 1.0;
  f0 = g0 * is;
  f1 = g1 * is;
}
__host__ __device__ inline void moments_bwd(const Jet& P, double& b0, double& b1) {
  const double* m = P.m[CJ_V];
  const double g0 = fma(m[0], b0, m[1] * b1), g1 = fma(m[2], b0, m[3] * b1);
  const double s = g0 + g1;
  const double is = s > 0.0 ? 1.0 / s : 1.0;
  b0 = g0 * is;
  b1 = g1 * is;
}

// One individual's records from the centred jets of its segments, seg[(k * kCJetDoubles + e) *
// stride] (segment k, entry e): the backward vectors at the segments' begins from the last segment
// to the first into bw[(k * 2 + l) * stride] (k <= n_seg), then the forward vectors from the first
// segment to the last, closing every segment that is a region (seg_region[k] >= 0) into
// out[seg_region[k]].  q = (1 - F, F) enters on the left, 1 on the right.
__host__ __device__ inline void moments_scan_close(const double* seg, double* bw, uint64_t stride,
                                                   uint32_t n_seg, const int32_t* seg_region, double F,
                                                   MomentRec* out) {
  double b0 = 1.0, b1 = 1.0;
  bw[((uint64_t)n_seg * 2) * stride] = b0;
  bw[((uint64_t)n_seg * 2 + 1) * stride] = b1;
  for (uint32_t k = n_seg; k-- > 0;) {
    Jet P;
#pragma unroll
    for (int q = 0; q < 4; ++q) P.m[CJ_V][q] = seg[((uint64_t)k * kCJetDoubles + q) * stride];
    moments_bwd(P, b0, b1);
    bw[((uint64_t)k * 2) * stride] = b0;
    bw[((uint64_t)k * 2 + 1) * stride] = b1;
  }
  double f0 = 1 - F, f1 = F;
  for (uint32_t k = 0; k < n_seg; ++k) {
    const double* p = seg + (uint64_t)k * kCJetDoubles * stride;
    const int32_t r = seg_region[k];
    if (r >= 0) {
      const CJet P = cjet_load(p, stride);
      out[r] = cjet_close(P, f0, f1, bw[((uint64_t)(k + 1) * 2) * stride], bw[((uint64_t)(k + 1) * 2 + 1) * stride]);
      moments_fwd(P.j, f0, f1);
    } else {
      Jet P;
#pragma unroll
      for (int q = 0; q < 4; ++q) P.m[CJ_V][q] = p[(uint64_t)q * stride];
      moments_fwd(P, f0, f1);
    }
  }
}

// ---- host interface ----
// Fast mode.  The site axis [0, Spad) is partitioned into segments (the regions and the gaps
// between them), the segments into pieces at the lane-chunk edges.  Tables (device):
//   chunk_piece [J + 1]   the first piece of every lane-chunk; a wave whose 64 lane-chunks lie in
//                         one segment makes ONE piece (all 64 entries equal), the ordered product
//                         of its lanes
//   piece_end   [P]       the site behind a piece's last
//   seg_piece   [n_seg+1] the first piece of every segment
//   seg_region  [n_seg]   the region a segment is, or -1
struct MomentsTables {
  const uint32_t* chunk_piece;
  const uint64_t* piece_end;
  const uint32_t* seg_piece;
  const int32_t* seg_region;
  uint32_t n_pieces, n_seg;
};
// the walk and the segment products: d_piece [I][P][27], d_seg [n_seg][27][I]
//   mb          A = IBD Mb (else IBD sites)
//   has_vin     the handle continues a site shard: its first site is an ordinary site
bool moments_fast_segments(const FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                           bool mb, bool has_vin, const MomentsTables& tb, double* d_piece, double* d_seg);
// one lane per individual: d_bw [n_seg + 1][2][I] scratch, d_out [I][n_reg]
void launch_moments_close(hipStream_t st, const double* d_seg, double* d_bw, uint64_t I, uint32_t n_seg,
                          const int32_t* d_seg_region, const double* d_indF, uint64_t n_reg,
                          MomentRec* d_out);
// exact mode: one lane per individual over the materialised log emissions eprob [S][I][2], pos [S]
// (+inf at a chromosome start): a backward pass that keeps the backward vectors at the region ends
// in d_bw [n_reg][2][I], then a forward pass that carries the forward vector and the centred
// row-jet of the current region and closes at its end.  d_reg [n_reg][2] = (begin, end).
void launch_moments_exact(hipStream_t st, const double* eprob, const double* pos, uint64_t S, uint64_t I,
                          const double* d_indF, const double* d_alpha, bool mb, const uint64_t* d_reg,
                          uint64_t n_reg, double* d_bw, MomentRec* d_out);

}  // namespace nghmm
