// kernels_moments.hip -- exact posterior means and covariances of (IBD sites or IBD Mb, number of
// tracts) per individual and region, from the likelihood tilted by the two path statistics and
// carried through one forward pass as a centred second-order jet (include/nghmm.h:
// nghmm_ibd_moments has the definition; kernels_moments.hpp the centred jet and the closing).
//
// A site is M_s = (c I + a 1 q^T) diag(e), a = 1 - c.  The tilt multiplies its entry (k, l) by
// exp(t_A phiA(k, l) + t_T phiT(k, l)), and both phi vanish outside column l = 1:
//   phiA = 1 (sites) or d_s [k = 1], 0 at a chromosome start (Mb);   phiT = [k = 0], 1 at a start.
// So with y_0 = x_0 M(0, 1), y_1 = x_1 M(1, 1) -- what a row x sends into column 1 from either
// state -- every derivative of x M is (0, w_0 y_0 + w_1 y_1) with the weights (w_0, w_1):
//   M_A, M_AA  (1, 1) | (0, d), (0, d^2)     M_T, M_TT  (1, st)     M_AT  (1, st) | (0, d st) = 0
// (st = 1 at a chromosome start, else 0): a site step is six row-times-matrix products and a few
// additions, no second operator.
//   k_moments_walk      a wave per (individual, chunk) in k_info_walk's shape and with its prefetch
//                       of e_il / pos_il -- the one read of 8 B per cell: every lane walks its T
//                       sites carrying a centred jet, rescaled and re-centred every RENORM sites.
//                       At a segment edge inside its lane-chunk a lane stores the finished piece
//                       and restarts from the identity; a wave that lies in one segment stores the
//                       ordered shuffle-tree product of its 64 lanes as one piece.
//   k_moments_segments  a wave per (individual, segment): lane l multiplies the pieces l K ..
//                       l K + K - 1 of the segment, the shuffle tree the lanes' (k_info_finish's
//                       grouping: it depends on the segment and the layout alone).
//   k_moments_close     a lane per individual: moments_scan_close.
// No atomics: one order of operations, the same bits on every call.
// Exact mode: k_moments_exact, one lane per individual over the materialised log emissions.
#include "fast_dev.hpp"
#include "kernels_moments.hpp"

namespace nghmm {

namespace {

// one site applied to the rows [0, ROWS) of every component; e = the two emissions (any common
// factor), dd = the distance (0 at a chromosome start), st = 1 at a chromosome start, else 0
template <bool MB, int ROWS>
__device__ __forceinline__ void moments_site(Jet& J, double a, double c, double q0, double q1, double e0,
                                             double e1, double dd, double st) {
  const double g0 = a * q0 * e0, g1 = a * q1 * e1;
  const double m00 = fma(c, e0, g0), m10 = g0, m01 = g1, m11 = fma(c, e1, g1);
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int i0 = 2 * r, i1 = 2 * r + 1;
    double y0[6], y1[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double x0 = J.m[k][i0], x1 = J.m[k][i1];
      y0[k] = x0 * m01;
      y1[k] = x1 * m11;
      J.m[k][i0] = fma(x0, m00, x1 * m10);
    }
    const double nV = y0[CJ_V] + y1[CJ_V];
    const double tV = fma(st, y1[CJ_V], y0[CJ_V]);   // x M_T
    const double tA = fma(st, y1[CJ_A], y0[CJ_A]);   // x_A M_T
    const double tT = fma(st, y1[CJ_T], y0[CJ_T]);   // x_T M_T
    J.m[CJ_V][i1] = nV;
    J.m[CJ_T][i1] = (y0[CJ_T] + y1[CJ_T]) + tV;
    J.m[CJ_TT][i1] = fma(2.0, tT, y0[CJ_TT] + y1[CJ_TT]) + tV;
    if constexpr (MB) {
      const double aV = dd * y1[CJ_V];               // x M_A
      J.m[CJ_A][i1] = (y0[CJ_A] + y1[CJ_A]) + aV;
      J.m[CJ_AA][i1] = fma(2.0 * dd, y1[CJ_A], y0[CJ_AA] + y1[CJ_AA]) + dd * aV;
      J.m[CJ_AT][i1] = fma(dd, y1[CJ_T], y0[CJ_AT] + y1[CJ_AT]) + tA;
    } else {
      const double nA = y0[CJ_A] + y1[CJ_A];
      J.m[CJ_A][i1] = nA + nV;
      J.m[CJ_AA][i1] = fma(2.0, nA, y0[CJ_AA] + y1[CJ_AA]) + nV;
      J.m[CJ_AT][i1] = ((y0[CJ_AT] + y1[CJ_AT]) + tA) + ((y0[CJ_T] + y1[CJ_T]) + tV);
    }
  }
}

// a = 1 - c in the form jet_site uses: for x = alpha d <= 2^-6 as expm1(x) c
__device__ __forceinline__ double one_minus_c(double x, double c) {
  return x <= 0.015625 ? expm1_over_x_tiny(x) * x * c : 1 - c;
}

__device__ __forceinline__ CJet cjet_shfl_down(const CJet& c, int off) {
  CJet o;
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) o.j.m[k][q] = __shfl_down(c.j.m[k][q], off);
  o.j.ex = __shfl_down(c.j.ex, off);
  o.da = __shfl_down(c.da, off);
  o.dt = __shfl_down(c.dt, off);
  return o;
}

// ordered product of the lanes [0, n) of a wave (n uniform); lane 0 holds it
__device__ __forceinline__ CJet cjet_wave_product(CJet m, int lane, int n) {
  for (int off = 1; off < n; off <<= 1) {
    const CJet o = cjet_shfl_down(m, off);
    if ((lane & (2 * off - 1)) == 0 && lane + off < n) m = cjet_mul(m, o);
  }
  return m;
}

template <bool MB>
__global__ void __launch_bounds__(64)
k_moments_walk(const double* __restrict__ e_il, const double* __restrict__ pos_il, uint64_t T, uint32_t C,
               const double* __restrict__ F, const double* __restrict__ A, uint32_t has_vin,
               const uint32_t* __restrict__ chunk_piece, const uint64_t* __restrict__ piece_end,
               uint32_t n_pieces, double* __restrict__ piece) {
  // chunk-major, as k_info_walk
  const uint32_t n_i = gridDim.x / C;
  const uint64_t i = blockIdx.x % n_i;
  const uint32_t c = blockIdx.x / n_i;
  const int lane = threadIdx.x;
  const double f = F[i], al = A[i];
  const double q0 = 1 - f, q1 = f;
  const double* ep = e_il + ((i * C + c) * T) * 64 + lane;
  const double* dp = pos_il + ((uint64_t)c * T) * 64 + lane;
  const uint32_t pb = chunk_piece[c * 64u];
  const bool whole = chunk_piece[c * 64u + 64u] - pb == 1;   // the wave lies in one segment
  uint32_t p = chunk_piece[c * 64u + (uint32_t)lane];
  // (piece_end has a sentinel behind its last entry)
  uint64_t next = whole ? ~0ull : piece_end[p];
  const uint64_t s0 = ((uint64_t)c * 64 + (uint64_t)lane) * T;
  double* const pi = piece + i * (uint64_t)n_pieces * kCJetDoubles;
  CJet J = cjet_identity();
  double rc[RENORM], dc[RENORM], rn[RENORM], dn[RENORM];
#pragma unroll
  for (int u = 0; u < RENORM; ++u) {
    rc[u] = ep[(uint64_t)u * 64];
    dc[u] = dp[(uint64_t)u * 64];
  }
  for (uint64_t t0 = 0; t0 < T; t0 += RENORM) {   // T is a multiple of RENORM
    const bool more = t0 + RENORM < T;
#pragma unroll
    for (int u = 0; u < RENORM; ++u) {
      rn[u] = more ? ep[(t0 + RENORM + u) * 64] : 1.0;
      dn[u] = more ? dp[(t0 + RENORM + u) * 64] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < RENORM; ++u) {
      const uint64_t s = s0 + t0 + u;
      const double d = dc[u];
      const bool start = !(d < kDStart) || (s == 0 && !has_vin);
      const double cc = start ? 0.0 : coanc(al, d);
      const double a = start ? 1.0 : one_minus_c(al * d, cc);
      moments_site<MB, 2>(J.j, a, cc, q0, q1, 1.0, rc[u], start ? 0.0 : d, start ? 1.0 : 0.0);
      if (s + 1 == next) {   // a segment ends here (or the lane-chunk does)
        jet_renorm(J.j);
        cjet_recentre(J);
        if (p < n_pieces) cjet_store(pi + (uint64_t)p * kCJetDoubles, 1, J);
        ++p;
        next = piece_end[p < n_pieces ? p : n_pieces];
        J = cjet_identity();
      }
    }
    jet_renorm(J.j);
    cjet_recentre(J);
#pragma unroll
    for (int u = 0; u < RENORM; ++u) {
      rc[u] = rn[u];
      dc[u] = dn[u];
    }
  }
  if (whole) {
    J = cjet_wave_product(J, lane, 64);
    if (lane == 0 && pb < n_pieces) cjet_store(pi + (uint64_t)pb * kCJetDoubles, 1, J);
  }
}

__global__ void __launch_bounds__(64)
k_moments_segments(const double* __restrict__ piece, uint32_t n_pieces, const uint32_t* __restrict__ seg_piece,
                   uint32_t n_seg, uint64_t I, double* __restrict__ seg) {
  const uint64_t i = blockIdx.x % I;
  const uint32_t k = (uint32_t)(blockIdx.x / I);
  const int lane = threadIdx.x;
  const uint32_t p0 = seg_piece[k], p1 = min(seg_piece[k + 1], n_pieces);
  const uint32_t n = p1 > p0 ? p1 - p0 : 0;
  const uint32_t K = (n + 63) / 64;
  const uint32_t nl = K ? (n + K - 1) / K : 0;   // lanes that hold pieces
  const double* pj = piece + (i * (uint64_t)n_pieces + p0) * kCJetDoubles;
  CJet m = cjet_identity();
  if ((uint32_t)lane < nl) {
    const uint32_t b = (uint32_t)lane * K, e = min(b + K, n);
    m = cjet_load(pj + (uint64_t)b * kCJetDoubles, 1);
    for (uint32_t u = b + 1; u < e; ++u) m = cjet_mul(m, cjet_load(pj + (uint64_t)u * kCJetDoubles, 1));
  }
  m = cjet_wave_product(m, lane, (int)nl);
  if (lane == 0) cjet_store(seg + (uint64_t)k * kCJetDoubles * I + i, I, m);
}

__global__ void __launch_bounds__(64)
k_moments_close(const double* __restrict__ seg, double* __restrict__ bw, uint64_t I, uint32_t n_seg,
                const int32_t* __restrict__ seg_region, const double* __restrict__ F, uint64_t n_reg,
                MomentRec* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  moments_scan_close(seg + i, bw + i, I, n_seg, seg_region, F[i], out + i * n_reg);
}

// exact mode: eprob [S][I][2] log emissions, pos [S] (+inf at a chromosome start)
template <bool MB>
__global__ void __launch_bounds__(64)
k_moments_exact(const double* __restrict__ eprob, const double* __restrict__ pos, uint64_t S, uint64_t I,
                const double* __restrict__ F, const double* __restrict__ A, const uint64_t* __restrict__ reg,
                uint64_t n_reg, double* __restrict__ bw, MomentRec* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  const double f = F[i], al = A[i];
  const double q0 = 1 - f, q1 = f;
  const double2* e2 = reinterpret_cast<const double2*>(eprob);
  // the backward vectors behind every region's last site
  {
    double b0 = 1.0, b1 = 1.0;
    uint64_t r = n_reg;
    for (uint64_t s = S; s-- > 0;) {
      if (r > 0 && s + 1 == reg[2 * (r - 1) + 1]) {
        --r;
        bw[(r * 2) * I + i] = b0;
        bw[(r * 2 + 1) * I + i] = b1;
      }
      if (r == 0) break;
      const double2 le = e2[s * I + i];
      const double mx = fmax(le.x, le.y);
      const bool fin = mx > -__builtin_huge_val();
      const double u0 = (fin ? det_exp(le.x - mx) : 0.0) * b0, u1 = (fin ? det_exp(le.y - mx) : 0.0) * b1;
      const double d = pos[s];
      const bool start = !(d < kDStart) || s == 0;
      const double cc = start ? 0.0 : det_exp(-al * d);
      const double a = start ? 1.0 : one_minus_c(al * d, cc);
      const double mix = a * fma(q0, u0, q1 * u1);
      const double n0 = fma(cc, u0, mix), n1 = fma(cc, u1, mix);
      const double sum = n0 + n1;
      const double is = sum > 0.0 ? 1.0 / sum : 1.0;
      b0 = n0 * is;
      b1 = n1 * is;
    }
  }
  // forward: row 0 of the jet is f times the region's centred jet, row 1 stays 0
  CJet J = cjet_identity();
  J.j.m[CJ_V][0] = q0;
  J.j.m[CJ_V][1] = q1;
  J.j.m[CJ_V][3] = 0.0;
  uint64_t r = 0;
  uint64_t rb = n_reg ? reg[0] : ~0ull, re = n_reg ? reg[1] : ~0ull;
  for (uint64_t s = 0; s < S && r < n_reg; ++s) {
    if (s == rb) {   // the region begins: the statistics start from 0 on the forward vector
#pragma unroll
      for (int k = 1; k < 6; ++k) J.j.m[k][0] = J.j.m[k][1] = 0.0;
      J.da = J.dt = 0.0;
    }
    const double2 le = e2[s * I + i];
    const double mx = fmax(le.x, le.y);
    const bool fin = mx > -__builtin_huge_val();
    const double d = pos[s];
    const bool start = !(d < kDStart) || s == 0;
    const double cc = start ? 0.0 : det_exp(-al * d);
    const double a = start ? 1.0 : one_minus_c(al * d, cc);
    moments_site<MB, 1>(J.j, a, cc, q0, q1, fin ? det_exp(le.x - mx) : 0.0, fin ? det_exp(le.y - mx) : 0.0,
                        start ? 0.0 : d, start ? 1.0 : 0.0);
    const bool last = s + 1 == re;
    if (last || (s & (RENORM - 1)) == RENORM - 1) {
      jet_renorm(J.j);
      cjet_recentre(J);
    }
    if (last) {
      out[i * n_reg + r] = cjet_close(J, 1.0, 0.0, bw[(r * 2) * I + i], bw[(r * 2 + 1) * I + i]);
      ++r;
      rb = r < n_reg ? reg[2 * r] : ~0ull;
      re = r < n_reg ? reg[2 * r + 1] : ~0ull;
    }
  }
}

}  // namespace

bool moments_fast_segments(const FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                           bool mb, bool has_vin, const MomentsTables& tb, double* d_piece, double* d_seg) {
  if (fs.T % RENORM != 0 || fs.C == 0 || tb.n_seg == 0 || tb.n_pieces == 0) return false;
  const dim3 grid((unsigned)(fs.I * fs.C)), block(64);
  if (mb)
    hipLaunchKernelGGL(k_moments_walk<true>, grid, block, 0, st, fs.e_il, fs.pos_il, fs.T, fs.C, d_indF, d_alpha,
                       has_vin ? 1u : 0u, tb.chunk_piece, tb.piece_end, tb.n_pieces, d_piece);
  else
    hipLaunchKernelGGL(k_moments_walk<false>, grid, block, 0, st, fs.e_il, fs.pos_il, fs.T, fs.C, d_indF, d_alpha,
                       has_vin ? 1u : 0u, tb.chunk_piece, tb.piece_end, tb.n_pieces, d_piece);
  hipLaunchKernelGGL(k_moments_segments, dim3((unsigned)(fs.I * tb.n_seg)), block, 0, st, d_piece, tb.n_pieces,
                     tb.seg_piece, tb.n_seg, fs.I, d_seg);
  return hipGetLastError() == hipSuccess;
}

void launch_moments_close(hipStream_t st, const double* d_seg, double* d_bw, uint64_t I, uint32_t n_seg,
                          const int32_t* d_seg_region, const double* d_indF, uint64_t n_reg,
                          MomentRec* d_out) {
  hipLaunchKernelGGL(k_moments_close, dim3((unsigned)((I + 63) / 64)), dim3(64), 0, st, d_seg, d_bw, I, n_seg,
                     d_seg_region, d_indF, n_reg, d_out);
}

void launch_moments_exact(hipStream_t st, const double* eprob, const double* pos, uint64_t S, uint64_t I,
                          const double* d_indF, const double* d_alpha, bool mb, const uint64_t* d_reg,
                          uint64_t n_reg, double* d_bw, MomentRec* d_out) {
  const dim3 grid((unsigned)((I + 63) / 64)), block(64);
  if (mb)
    hipLaunchKernelGGL(k_moments_exact<true>, grid, block, 0, st, eprob, pos, S, I, d_indF, d_alpha, d_reg, n_reg,
                       d_bw, d_out);
  else
    hipLaunchKernelGGL(k_moments_exact<false>, grid, block, 0, st, eprob, pos, S, I, d_indF, d_alpha, d_reg,
                       n_reg, d_bw, d_out);
}

}  // namespace nghmm
