// kernels_expect.hip -- exact expectations over IBD paths: the expected number of tracts, IBD
// sites and Mb, state switches, the entropy of the path posterior and the posterior probability
// of the decoded path, per individual and region and per site over the cohort
// (include/nghmm.h: nghmm_ibd_expect has the definition of every term).
//
// All of them are sums over the sites of functions of the pairwise marginals
//   xi_s(k, l) = f_{s-1}(k) m_s(k, l) / Z_s,   m_s(k, l) = T_s(k, l) e_s(l) beta_s(l),
// and of the posterior chain's own transition r_s(k, l) = m_s(k, l) / (m_s(k, 0) + m_s(k, 1)).
// The four m_s are by-products of the beta step the backward sweep makes anyway
// (beta_{s-1}(k) = m_s(k, 0) + m_s(k, 1)), every factor is scale-free and a common factor of the
// two emissions cancels, so the stored ratios rho = e1 / e0 serve.
//   k_expect_walk     one wave per (individual, chunk of 64 lane-chunks), like k_support_walk but
//                     over EVERY cell: a lane recomputes its forward vectors block by block from
//                     the checkpoints, carries beta right to left, forms the four products and the
//                     terms per site, keeps lane-private sums for the region piece it is in and
//                     stores one piece per (lane-chunk, region overlap); with site records asked
//                     for it also stores (on, off, ibd, h) of every cell, tile-major
//                     [c T + t][i][4][64] (512 B wave stores);
//   k_expect_finish   one lane per (individual, region): its pieces added in site order;
//   k_expect_sites    one wave per (tile row, term): per block of 64 individuals the butterfly
//                     tree x_i += x_{i ^ 32}, ^ 16, ..., ^ 1 in registers (coalesced loads: the
//                     lanes are the row's 64 sites), the blocks in order.
// ln r comes from the small side: with x = min / max of the pair m(k, 0), m(k, 1), the larger
// entry's ln r is -log1p(x) and the smaller one's ln(x) - log1p(x).  Exact mode: log1p is the
// classic correction u = 1 + x, u == 1 ? x : det_log(u) x / (u - 1).  Fast mode: log1p(x) =
// 2 atanh(x / (2 + x)) and ln(x) from the same odd series on the mantissa (log1p_unit, ln_unit
// below): four calls of the device library's log were four fifths of the walk's instructions.
// No float atomics: every sum has one order -- the same bits on every call.
// Exact mode: k_expect_exact, one lane per individual in log space through detmath.h, with the
// forward array filled and normalised as k_support_exact does it.
#include "fast_dev.hpp"
#include "kernels_expect.hpp"
#include "lnshare_dev.hpp"

namespace nghmm {

namespace {

struct WalkArgs {
  const double* __restrict__ e_il;
  const double* __restrict__ pos_il;
  uint64_t T, S, I;
  uint32_t C;
  uint32_t has_vin;
  const double* __restrict__ indF;
  const double* __restrict__ alpha;
  const double* __restrict__ bound;
  const double2* __restrict__ ckpt;
  const uint8_t* __restrict__ path16;
  const uint8_t* __restrict__ prev_state;
  const ExpectRegion* __restrict__ reg;
  uint64_t n_reg, n_pieces;
  ExpectRec* __restrict__ piece;
  double* __restrict__ cell;
};

__global__ void __launch_bounds__(64, 2)
k_expect_walk(const WalkArgs A) {
  const uint64_t i = blockIdx.x / A.C;
  const uint32_t c = blockIdx.x % A.C;
  const int lane = threadIdx.x;
  const uint64_t T = A.T, S = A.S;
  const uint64_t J = (uint64_t)A.C * 64;
  const uint64_t j = (uint64_t)c * 64 + lane;
  const uint64_t s_base = j * T;
  const bool VIT = A.path16 != nullptr, CELLS = A.cell != nullptr;

  // the last region that begins at or in front of the lane-chunk's last site: found once, then
  // the lane steps down
  uint64_t r = 0;   // regions [0, r) begin in front of the lane-chunk's end
  uint64_t rb = ~0ull, re = 0, rp = 0;   // (re = 0: no region)
  if (s_base < S && A.n_reg) {
    const uint64_t s_end = (S - s_base < T ? S : s_base + T) - 1;
    uint64_t lo = 0, hi = A.n_reg;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (A.reg[mid].begin <= s_end) lo = mid + 1;
      else hi = mid;
    }
    r = lo;
    if (r > 0) {
      const ExpectRegion R = A.reg[r - 1];
      if (R.end > s_base) {
        rb = R.begin;
        re = R.end;
        rp = R.piece0;
      }
    }
  }

  const double f = A.indF[i], al = A.alpha[i];
  const double q0 = 1 - f, q1 = f;
  const double* bd = A.bound + (i * J + j) * 4;
  const double vin0 = bd[0], vin1 = bd[1];
  double w0 = bd[2], w1 = bd[3];
  const double* ep = A.e_il + ((i * A.C + c) * T) * 64 + lane;
  const double* dp = A.pos_il + ((uint64_t)c * T) * 64 + lane;
  const uint64_t nblk = T / CK;
  const double2* ck = A.ckpt + ((i * A.C + c) * nblk * 2) * 64 + lane;
  ExpectRec* const pc_out = A.piece + i * A.n_pieces;

  double a_ibd = 0.0, a_st = 0.0, a_sw = 0.0, a_mb = 0.0, a_h = 0.0, a_lp = 0.0;

  double ecur[CK], enxt[CK], dcur[CK];
  double2 r0c, r1c;
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
      }
    }
    const uint64_t s_blk = s_base + b * CK;
    if (b + 1 < nblk) {
#pragma unroll
      for (int u = 0; u < CK; ++u) dcur[u] = dp[(b * CK + u) * 64];
      r0c = b ? ck[(b * 2) * 64] : double2{1.0, 0.0};
      r1c = b ? ck[(b * 2 + 1) * 64] : double2{0.0, 1.0};
    }
    // the decoded states of the block's sites (bit u) and of the site in front of it (bit 8)
    uint32_t zbits = 0;
    if (VIT && s_blk < S) {
      const uint64_t w = *reinterpret_cast<const uint64_t*>(A.path16 + ((s_blk >> 4) * A.I + i) * 16 +
                                                            (s_blk & 15));
#pragma unroll
      for (int u = 0; u < CK; ++u) zbits |= (((w >> (8 * u)) & 0xffu) != 0 ? 1u : 0u) << u;
      uint32_t zp = 0;
      if (s_blk > 0) {
        const uint64_t sp = s_blk - 1;
        zp = A.path16[((sp >> 4) * A.I + i) * 16 + (sp & 15)] != 0 ? 1u : 0u;
      } else if (A.prev_state) {
        zp = A.prev_state[i] != 0 ? 1u : 0u;
      }
      zbits |= zp << 8;
    }
    // forward vectors of the block's sites, from the checkpoint (as k_fast_bwd_recompute);
    // fp[u] = the vector of the site in front of site u
    double v0 = fma(vin0, r0c.x, vin1 * r1c.x);
    double v1 = fma(vin0, r0c.y, vin1 * r1c.y);
    double fp0[CK], fp1[CK], cc[CK];
#pragma unroll
    for (int u = 0; u < CK; ++u) {
      fp0[u] = v0;
      fp1[u] = v1;
      cc[u] = coanc(al, dcur[u]);
      const double a = 1 - cc[u];
      const double sm = v0 + v1;
      v0 = fma(a * q0, sm, cc[u] * v0);
      v1 = fma(a * q1, sm, cc[u] * v1) * ecur[u];
      if (u == CK / 2 - 1) {
        int dummy = 0;
        renorm2(v0, v1, dummy);
      }
    }
    // backward through the block: the four products, the terms, the beta step
#pragma unroll
    for (int u = CK - 1; u >= 0; --u) {
      const uint64_t s = s_blk + u;
      const double a = 1 - cc[u];
      const double u0 = w0, u1 = ecur[u] * w1;
      const double m00 = fma(a, q0, cc[u]) * u0, m01 = a * q1 * u1;
      const double m10 = a * q0 * u0, m11 = fma(a, q1, cc[u]) * u1;
      const bool want = CELLS ? s < S : (s < re);
      if (NGH_ANY(want)) {
        const bool start = !(dcur[u] < kDStart) || (s == 0 && !A.has_vin);
        const double n00 = fp0[u] * m00, n01 = fp0[u] * m01;
        const double n10 = fp1[u] * m10, n11 = fp1[u] * m11;
        const double rz = rcp_nr2((n00 + n01) + (n10 + n11));
        const double x00 = n00 * rz, x01 = n01 * rz, x10 = n10 * rz, x11 = n11 * rz;
        const double p0 = x00 + x10, p1 = x01 + x11;
        // chromosome start: the site enters through pi_s alone
        double L00, L01, L10, L11;
        ln_shares(start ? n00 + n10 : m00, start ? n01 + n11 : m01, L00, L01);
        ln_shares(m10, m11, L10, L11);
        const double g00 = start ? p0 : x00, g01 = start ? p1 : x01;
        const double g10 = start ? 0.0 : x10, g11 = start ? 0.0 : x11;
        double hs = g00 > 0.0 ? g00 * L00 : 0.0;
        hs += g01 > 0.0 ? g01 * L01 : 0.0;
        hs += g10 > 0.0 ? g10 * L10 : 0.0;
        hs += g11 > 0.0 ? g11 * L11 : 0.0;
        hs = -hs;
        const double t_on = start ? 0.0 : x01, t_off = start ? 0.0 : x10;
        if (CELLS && s < S) {
          double* o = A.cell + (((uint64_t)c * T + b * CK + u) * A.I + i) * 256 + lane;
          o[0] = t_on;
          o[64] = t_off;
          o[128] = p1;
          o[192] = hs;
        }
        if (s < re) {   // (s >= rb: the region is left as soon as rb is done)
          a_ibd += p1;
          a_st += start ? p1 : x01;
          a_sw += t_on + t_off;
          a_mb += start ? 0.0 : dcur[u] * x11;
          a_h += hs;
          if (VIT) {
            const uint32_t z = (zbits >> u) & 1u, zp = start ? 0u : (zbits >> (u ? u - 1 : 8)) & 1u;
            a_lp += zp ? (z ? L11 : L10) : (z ? L01 : L00);
          }
          if (s == rb || s == s_base) {   // the piece is complete
            ExpectRec pc;
            pc.ibd = a_ibd;
            pc.starts = a_st;
            pc.switches = a_sw;
            pc.ibd_mb = a_mb;
            pc.entropy = a_h;
            pc.log_p_path = a_lp;
            pc_out[rp + (j - rb / T)] = pc;
            a_ibd = a_st = a_sw = a_mb = a_h = a_lp = 0.0;
            if (s == rb) {   // the region in front, if it reaches into the lane-chunk
              --r;
              rb = ~0ull;
              re = 0;
              if (r > 0) {
                const ExpectRegion R = A.reg[r - 1];
                if (R.end > s_base) {
                  rb = R.begin;
                  re = R.end;
                  rp = R.piece0;
                }
              }
            } else {
              re = 0;
            }
          }
        }
      }
      w0 = m00 + m01;
      w1 = m10 + m11;
    }
    {
      int dummy = 0;
      renorm2(w0, w1, dummy);
    }
    if (b == 0) break;
#pragma unroll
    for (int u = 0; u < CK; ++u) {
      ecur[u] = enxt[u];
    }
  }
}

__device__ __forceinline__ void rec_add(ExpectRec& t, const ExpectRec& a) {
  t.ibd += a.ibd;
  t.starts += a.starts;
  t.switches += a.switches;
  t.ibd_mb += a.ibd_mb;
  t.entropy += a.entropy;
  t.log_p_path += a.log_p_path;
}

// one lane per (individual, region): the pieces in site order, the first one's value first
__global__ void __launch_bounds__(64)
k_expect_finish(const ExpectRegion* __restrict__ reg, uint64_t n_reg, uint64_t I, uint64_t T,
                uint64_t n_pieces, const ExpectRec* __restrict__ piece, ExpectRec* __restrict__ out) {
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_reg * I) return;
  const uint64_t i = x / n_reg, k = x % n_reg;
  const ExpectRegion R = reg[k];
  const uint64_t np = expect_pieces(R.begin, R.end, T);
  const ExpectRec* p = piece + i * n_pieces + R.piece0;
  ExpectRec acc = p[0];
  for (uint64_t n = 1; n < np; ++n) rec_add(acc, p[n]);
  out[x] = acc;
}

// fast mode: one wave per (tile row c T + t, term), lane l = site (c 64 + l) T + t.  Per block of
// 64 individuals (filled up with zeros) the butterfly tree in registers, the blocks in order.
__global__ void __launch_bounds__(64)
k_expect_sites(const double* __restrict__ cell, uint64_t T, uint64_t S, uint64_t I,
               ExpectSite* __restrict__ out) {
  const uint64_t row = blockIdx.x;
  const uint32_t k = blockIdx.y;   // on, off, ibd, entropy
  const int lane = threadIdx.x;
  const uint64_t s = ((row / T) * 64 + lane) * T + row % T;
  double tot = 0.0;
#pragma unroll 1
  for (uint64_t i0 = 0; i0 < I; i0 += 64) {
    const double* p = cell + ((row * I + i0) * 4 + k) * 64 + lane;
    const uint64_t left = I - i0;
    double v[32];
    if (left >= 64) {
#pragma unroll
      for (int n = 0; n < 32; ++n) v[n] = p[n * 256] + p[(n + 32) * 256];
    } else {
#pragma unroll
      for (int n = 0; n < 32; ++n)
        v[n] = ((uint64_t)n < left ? p[n * 256] : 0.0) + ((uint64_t)(n + 32) < left ? p[(n + 32) * 256] : 0.0);
    }
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1)
#pragma unroll
      for (int n = 0; n < m; ++n) v[n] += v[n + m];
    tot = i0 ? tot + v[0] : v[0];
  }
  if (s < S) reinterpret_cast<double*>(out + s)[k] = tot;
}

// exact mode's cells are site-major [S][I][4]: one wave per site, the lanes are the individuals
__global__ void __launch_bounds__(64)
k_expect_sites_rows(const double* __restrict__ cell, uint64_t I, ExpectSite* __restrict__ out) {
  const uint64_t s = blockIdx.x;
  const int lane = threadIdx.x;
  double tot[4] = {0.0, 0.0, 0.0, 0.0};
  for (uint64_t i0 = 0; i0 < I; i0 += 64) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double v = i0 + lane < I ? cell[(s * I + i0 + lane) * 4 + k] : 0.0;
      const double t = wave_sum(v);
      tot[k] = i0 ? tot[k] + t : t;
    }
  }
  if (lane == 0) out[s] = ExpectSite{tot[0], tot[1], tot[2], tot[3]};
}

// exact mode: eprob [S][I][2] log emissions; fw [S + 1][I][2] is scratch for the forward values
// (fw[s + 1] = site s), filled as k_support_exact fills it: the larger of the two entries
// subtracted after every site.  Then the backward recursion right to left; a region is the sum of
// its sites' terms added to 0 from its last site to its first.
__global__ void __launch_bounds__(64)
k_expect_exact(const double* __restrict__ eprob, const double* __restrict__ pos,
               double* __restrict__ fw, uint64_t S, uint64_t I, const double* __restrict__ indF,
               const double* __restrict__ alpha, const uint8_t* __restrict__ path16,
               const ExpectRegion* __restrict__ reg, uint64_t n_reg, ExpectRec* __restrict__ out,
               double* __restrict__ cell, int* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  const double f = indF[i], al = alpha[i];
  const double q0 = 1 - f, q1 = f;
  const double lq0 = det_log(q0), lq1 = det_log(q1);
  {
    double p0 = lq0, p1 = lq1;
    bool bad = false;
    for (uint64_t s = 0; s < S; ++s) {
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
  uint64_t r = n_reg;
  ExpectRegion R{0, 0, 0, 0};
  if (r) R = reg[r - 1];
  ExpectRec acc{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (uint64_t s = S; s-- > 0;) {
    const double d = pos[s];
    const bool start = !(d < kDStart) || s == 0;
    const double cs = d < kDStart ? det_exp(-al * d) : 0.0;
    const double a = 1 - cs;
    const double t00 = det_log(a * q0 + cs), t01 = det_log(a * q1);
    const double t10 = det_log(a * q0), t11 = det_log(a * q1 + cs);
    const double u0 = eprob[(s * I + i) * 2] + b0, u1 = eprob[(s * I + i) * 2 + 1] + b1;
    const double m00 = t00 + u0, m01 = t01 + u1, m10 = t10 + u0, m11 = t11 + u1;
    const bool inreg = r > 0 && s < R.end;   // (s >= R.begin: the region is left once begin is done)
    if (cell || inreg) {
      const double lf0 = s ? fw[(s * I + i) * 2] : lq0, lf1 = s ? fw[(s * I + i) * 2 + 1] : lq1;
      const double n00 = lf0 + m00, n01 = lf0 + m01, n10 = lf1 + m10, n11 = lf1 + m11;
      const double P0 = lsum2(n00, n10), P1 = lsum2(n01, n11);
      const double lz = lsum2(P0, P1);
      const double x00 = exp0(n00 - lz), x01 = exp0(n01 - lz), x10 = exp0(n10 - lz), x11 = exp0(n11 - lz);
      const double p0 = x00 + x10, p1 = x01 + x11;
      const double L00 = start ? ln_share_log(P0, P1) : ln_share_log(m00, m01);
      const double L01 = start ? ln_share_log(P1, P0) : ln_share_log(m01, m00);
      const double L10 = ln_share_log(m10, m11), L11 = ln_share_log(m11, m10);
      const double g00 = start ? p0 : x00, g01 = start ? p1 : x01;
      const double g10 = start ? 0.0 : x10, g11 = start ? 0.0 : x11;
      double hs = g00 > 0.0 ? g00 * L00 : 0.0;
      hs += g01 > 0.0 ? g01 * L01 : 0.0;
      hs += g10 > 0.0 ? g10 * L10 : 0.0;
      hs += g11 > 0.0 ? g11 * L11 : 0.0;
      hs = -hs;
      const double t_on = start ? 0.0 : x01, t_off = start ? 0.0 : x10;
      if (cell) {
        double* o = cell + (s * I + i) * 4;
        o[0] = t_on;
        o[1] = t_off;
        o[2] = p1;
        o[3] = hs;
      }
      if (inreg) {
        acc.ibd += p1;
        acc.starts += start ? p1 : x01;
        acc.switches += t_on + t_off;
        acc.ibd_mb += start ? 0.0 : d * x11;
        acc.entropy += hs;
        if (path16) {
          const uint32_t z = path16[((s >> 4) * I + i) * 16 + (s & 15)] != 0 ? 1u : 0u;
          const uint32_t zp = start ? 0u : (path16[(((s - 1) >> 4) * I + i) * 16 + ((s - 1) & 15)] != 0 ? 1u : 0u);
          acc.log_p_path += zp ? (z ? L11 : L10) : (z ? L01 : L00);
        }
        if (s == R.begin) {
          out[i * n_reg + (r - 1)] = acc;
          acc = ExpectRec{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
          --r;
          if (r) R = reg[r - 1];
        }
      }
    }
    const double n0 = lsum2(m00, m01), n1 = lsum2(m10, m11);
    const double M = (n1 >= n0) ? n1 : n0;
    const bool fin = M > NGH_NEG_INF;
    b0 = fin ? n0 - M : n0;
    b1 = fin ? n1 - M : n1;
  }
}

}  // namespace

uint64_t expect_cell_doubles(const FastState* fs, uint64_t S, uint64_t I) {
  return fs ? (uint64_t)fs->C * fs->T * I * 256 : S * I * 4;
}

bool expect_fast_walk(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                      bool has_vin, const uint8_t* path16, const uint8_t* prev_state,
                      const ExpectRegion* d_reg, uint64_t n_reg, uint64_t n_pieces,
                      ExpectRec* d_piece, ExpectRec* d_out, double* d_cell, ExpectSite* d_sites) {
  if (fs.T == 0 || fs.T % CK != 0) return false;
  WalkArgs A;
  A.e_il = fs.e_il;
  A.pos_il = fs.pos_il;
  A.T = fs.T;
  A.S = fs.S;
  A.I = fs.I;
  A.C = fs.C;
  A.has_vin = has_vin ? 1u : 0u;
  A.indF = d_indF;
  A.alpha = d_alpha;
  A.bound = fs.bound;
  A.ckpt = reinterpret_cast<const double2*>(fs.ckpt);
  A.path16 = path16;
  A.prev_state = prev_state;
  A.reg = d_reg;
  A.n_reg = n_reg;
  A.n_pieces = n_pieces;
  A.piece = d_piece;
  A.cell = d_cell;
  const dim3 grid((unsigned)(fs.I * fs.C)), block(64);
  hipLaunchKernelGGL(k_expect_walk, grid, block, 0, st, A);
  if (n_reg)
    hipLaunchKernelGGL(k_expect_finish, dim3((unsigned)((n_reg * fs.I + 63) / 64)), block, 0, st, d_reg,
                       n_reg, fs.I, fs.T, n_pieces, d_piece, d_out);
  if (d_cell)
    hipLaunchKernelGGL(k_expect_sites, dim3((unsigned)((uint64_t)fs.C * fs.T), 4), block, 0, st, d_cell,
                       fs.T, fs.S, fs.I, d_sites);
  return hipGetLastError() == hipSuccess;
}

void launch_expect_exact(hipStream_t st, const double* eprob, const double* pos, double* fw,
                         uint64_t S, uint64_t I, const double* d_indF, const double* d_alpha,
                         const uint8_t* path16, const ExpectRegion* d_reg, uint64_t n_reg,
                         ExpectRec* d_out, double* d_cell, ExpectSite* d_sites, int* d_flags) {
  hipLaunchKernelGGL(k_expect_exact, dim3((unsigned)((I + 63) / 64)), dim3(64), 0, st, eprob, pos, fw,
                     S, I, d_indF, d_alpha, path16, d_reg, n_reg, d_out, d_cell, d_flags);
  if (d_cell)
    hipLaunchKernelGGL(k_expect_sites_rows, dim3((unsigned)S), dim3(64), 0, st, d_cell, I, d_sites);
}

}  // namespace nghmm
