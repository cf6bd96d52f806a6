// kernels_bylength.hip -- expected number and expected length of the IBD tracts of at least L_k,
// exactly, per individual and region (include/nghmm.h: nghmm_ibd_by_length has the definition).
//
// Given the data the path is a Markov chain: a tract begins at a and covers a..b with probability
// sigma_a W(a, b), W the product of the chain's stay-IBD probabilities rho_s = r_s(1, 1) over
// a < s <= b, and the run goes on beyond b for M_b further sites (D_b Mb) in expectation,
// M_s = rho_{s+1} (1 + M_{s+1}).  Fast mode, in the layout of the other walks (a lane owns a
// lane-chunk of T consecutive sites; per-cell planes tile-major):
//   k_bylength_walk   the shape of k_expect_walk: per cell sigma_s, ln rho_s (from the small side,
//                     lnshare_dev.hpp; a blocked step -- rho_s = 0, a chromosome start -- as the flag
//                     1.0) and rho_s; per lane-chunk the affine maps of the M and D recursions,
//                     the sum of ln rho behind its last blocked step and its blocked count;
//   k_bylength_scan   one wave per individual: the maps composed right to left (64 lanes in a
//                     Hillis-Steele tree with the steps 1, 2, .., 32, the waves in order), the sums
//                     and counts left to right the same way;
//   k_bylength_fill   a lane per lane-chunk: M_s and D_s backward from the chunk-end value, then
//                     the prefix Q_s (restarted at every blocked step) and the count n_s forward;
//   k_bylength_terms  a lane per lane-chunk from its last site to its first, per start site the K
//                     thresholds: W(a, b) = n_b == n_a ? exp(Q_b - Q_a) : 0 gathered at b_k(a),
//                     one piece per (lane-chunk, region overlap) as k_expect_walk;
//   k_bylength_finish one lane per (individual, region, threshold): its pieces in site order.
// Exact mode: k_bylength_exact, one lane per individual in log space through detmath.h.
// No float atomics: every sum has one order -- the same bits on every call.
#include "fast_dev.hpp"
#include "kernels_bylength.hpp"
#include "lnshare_dev.hpp"

namespace nghmm {

namespace {

constexpr double kBlocked = 1.0;   // in the q plane before the fill: ln rho <= 0, so 1.0 is no value

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
  double* __restrict__ sigma;
  double* __restrict__ q;
  double* __restrict__ m;
  double* __restrict__ map;
  double* __restrict__ qtail;
  uint32_t* __restrict__ nblk;
  double* __restrict__ pi;   // (PI only) the posterior of the IBD state, a plane like sigma
};

// The forward recomputation, the beta step and the four products are k_expect_walk's.  PI: the
// posterior x01 + x11, which the walk forms anyway, goes to a plane of its own (kernels_long.hip);
// without it the kernel is what it was.
template <bool PI>
__global__ void __launch_bounds__(64, 2)
k_bylength_walk(const WalkArgs A) {
  const uint64_t i = blockIdx.x / A.C;
  const uint32_t c = blockIdx.x % A.C;
  const int lane = threadIdx.x;
  const uint64_t T = A.T, S = A.S;
  const uint64_t J = (uint64_t)A.C * 64;
  const uint64_t j = (uint64_t)c * 64 + lane;
  const uint64_t s_base = j * T;

  const double f = A.indF[i], al = A.alpha[i];
  const double q0 = 1 - f, q1 = f;
  const double* bd = A.bound + (i * J + j) * 4;
  const double vin0 = bd[0], vin1 = bd[1];
  double w0 = bd[2], w1 = bd[3];
  const double* ep = A.e_il + ((i * A.C + c) * T) * 64 + lane;
  const double* dp = A.pos_il + ((uint64_t)c * T) * 64 + lane;
  const uint64_t nblk = T / CK;
  const double2* ck = A.ckpt + ((i * A.C + c) * nblk * 2) * 64 + lane;

  double mA = 1.0, mBM = 0.0, mBD = 0.0;   // the map of the sites walked so far
  double qt = 0.0;                         // ln rho behind the last blocked step, last site first
  uint32_t nb = 0;

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
      for (int u = 0; u < CK; ++u) enxt[u] = ep[(bn * CK + u) * 64];
    }
    const uint64_t s_blk = s_base + b * CK;
    if (b + 1 < nblk) {
#pragma unroll
      for (int u = 0; u < CK; ++u) dcur[u] = dp[(b * CK + u) * 64];
      r0c = b ? ck[(b * 2) * 64] : double2{1.0, 0.0};
      r1c = b ? ck[(b * 2 + 1) * 64] : double2{0.0, 1.0};
    }
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
#pragma unroll
    for (int u = CK - 1; u >= 0; --u) {
      const uint64_t s = s_blk + u;
      const double a = 1 - cc[u];
      const double u0 = w0, u1 = ecur[u] * w1;
      const double m00 = fma(a, q0, cc[u]) * u0, m01 = a * q1 * u1;
      const double m10 = a * q0 * u0, m11 = fma(a, q1, cc[u]) * u1;
      const bool real = s < S;
      const bool start = !(dcur[u] < kDStart) || (s == 0 && !A.has_vin);
      const double n00 = fp0[u] * m00, n01 = fp0[u] * m01;
      const double n10 = fp1[u] * m10, n11 = fp1[u] * m11;
      const double rz = rcp_nr2((n00 + n01) + (n10 + n11));
      const double x01 = n01 * rz, x11 = n11 * rz;
      const double sg = start ? x01 + x11 : x01;
      double L10, L11;
      ln_shares(m10, m11, L10, L11);
      const double rho = m11 * rcp_nr2(m10 + m11);
      const bool blocked = start || !(rho > 0.0) || !(L11 > NGH_NEG_INF);
      {
        const uint64_t o = (((uint64_t)c * T + b * CK + u) * A.I + i) * 64 + lane;
        A.sigma[o] = real ? sg : 0.0;
        A.q[o] = (real && !blocked) ? L11 : kBlocked;
        A.m[o] = (real && !blocked) ? rho : 0.0;
        if (PI) A.pi[o] = real ? x01 + x11 : 0.0;
      }
      if (real) {   // (a padding site is the identity)
        if (blocked) {
          mA = 0.0;
          mBM = 0.0;
          mBD = 0.0;
          ++nb;
        } else {
          mA *= rho;
          mBM = rho * (1.0 + mBM);
          mBD = rho * (dcur[u] + mBD);
          qt += nb ? 0.0 : L11;
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
    for (int u = 0; u < CK; ++u) ecur[u] = enxt[u];
  }
  double* mo = A.map + (i * J + j) * 3;
  mo[0] = mA;
  mo[1] = mBM;
  mo[2] = mBD;
  A.qtail[i * J + j] = qt;
  A.nblk[i * J + j] = nb;
}

// One wave per individual.  Right to left: F_l = f_l o f_{l+1} o .. o f_63 of a wave's 64 maps in
// a Hillis-Steele tree (steps 1, 2, 4, .., 32), the value at a lane-chunk's last site = F_{l+1} of
// the wave's incoming value, the waves in order.  Left to right: (tail sum, count) the same way
// under (L, R) -> (R.n ? R.q : L.q + R.q, L.n + R.n).
__global__ void __launch_bounds__(64)
k_bylength_scan(uint32_t C, const double* __restrict__ map, const double* __restrict__ qtail,
                const uint32_t* __restrict__ nblk, const double* __restrict__ carry_in,
                double* __restrict__ carry_out, double* __restrict__ endM, double* __restrict__ endD,
                double* __restrict__ q0, uint32_t* __restrict__ n0) {
  const uint64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  const uint64_t J = (uint64_t)C * 64;
  double xM = carry_in ? carry_in[i * 2] : 0.0, xD = carry_in ? carry_in[i * 2 + 1] : 0.0;
  for (uint32_t c = C; c-- > 0;) {
    const uint64_t o = i * J + (uint64_t)c * 64 + lane;
    double a = map[o * 3], bm = map[o * 3 + 1], bd = map[o * 3 + 2];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double a2 = __shfl_down(a, off), bm2 = __shfl_down(bm, off), bd2 = __shfl_down(bd, off);
      if (lane + off < 64) {
        bm = fma(a, bm2, bm);
        bd = fma(a, bd2, bd);
        a *= a2;
      }
    }
    const double ea = __shfl_down(a, 1), ebm = __shfl_down(bm, 1), ebd = __shfl_down(bd, 1);
    endM[o] = lane < 63 ? fma(ea, xM, ebm) : xM;
    endD[o] = lane < 63 ? fma(ea, xD, ebd) : xD;
    const double a0 = __shfl(a, 0), bm0 = __shfl(bm, 0), bd0 = __shfl(bd, 0);
    xM = fma(a0, xM, bm0);
    xD = fma(a0, xD, bd0);
  }
  if (carry_out && lane == 0) {
    carry_out[i * 2] = xM;
    carry_out[i * 2 + 1] = xD;
  }
  double cq = 0.0;
  uint32_t cn = 0;
  for (uint32_t c = 0; c < C; ++c) {
    const uint64_t o = i * J + (uint64_t)c * 64 + lane;
    double q = qtail[o];
    uint32_t n = nblk[o];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double q2 = __shfl_up(q, off);
      const uint32_t n2 = __shfl_up(n, off);
      if (lane >= off) {
        q = n ? q : q2 + q;
        n += n2;
      }
    }
    // what enters lane l: the carry and the lanes in front of it
    const double pq = __shfl_up(q, 1);
    const uint32_t pn = __shfl_up(n, 1);
    q0[o] = lane ? (pn ? pq : cq + pq) : cq;
    n0[o] = lane ? cn + pn : cn;
    const double lq = __shfl(q, 63);
    const uint32_t ln = __shfl(n, 63);
    cq = ln ? lq : cq + lq;
    cn += ln;
  }
}

// A lane per lane-chunk.  Backward: M_s and D_s from the chunk-end value (rho is read from the m
// plane before M goes there).  Forward: Q_s and n_s.  A padding site keeps what it is handed.
__global__ void __launch_bounds__(64)
k_bylength_fill(uint64_t T, uint64_t S, uint64_t I, uint32_t C, int mb, const double* __restrict__ pos_il,
                const ByLenCells cl, const double* __restrict__ endM, const double* __restrict__ endD,
                const double* __restrict__ q0, const uint32_t* __restrict__ n0,
                double* __restrict__ qmax) {
  const uint64_t i = blockIdx.x / C;
  const uint32_t c = blockIdx.x % C;
  const int lane = threadIdx.x;
  const uint64_t J = (uint64_t)C * 64, j = (uint64_t)c * 64 + lane, s_base = j * T;
  const double* dp = pos_il + ((uint64_t)c * T) * 64 + lane;
  const uint64_t cell0 = (((uint64_t)c * T) * I + i) * 64 + lane, step = I * 64;
  double x = endM[i * J + j], y = endD[i * J + j];
#pragma unroll 8
  for (uint64_t t = T; t-- > 0;) {
    const uint64_t o = cell0 + t * step;
    const double rho = cl.m[o], d = dp[t * 64];
    cl.m[o] = x;
    if (mb) cl.d[o] = y;
    if (s_base + t < S) {
      const bool go = rho > 0.0;
      x = go ? rho * (1.0 + x) : 0.0;
      y = go ? rho * (d + y) : 0.0;
    }
  }
  // Q_s = (what the lane is handed) + (the lane's own running sum): the terms are added where
  // they are small and each Q_s is rounded once at its full magnitude, so that the error of
  // Q_b - Q_a does not grow with the sites per lane (a running sum at |Q| ~ 4e4 loses 4e-12 per
  // site: over lanes of 256 sites that showed as 2e-12 relative in `length` against lanes of 32)
  double base = q0[i * J + j], loc = 0.0, q = base, big = 0.0;
  uint32_t n = n0[i * J + j];
#pragma unroll 8
  for (uint64_t t = 0; t < T; ++t) {
    const uint64_t o = cell0 + t * step;
    const double lr = cl.q[o];
    if (s_base + t < S) {
      const bool blk = lr > 0.0;
      loc = blk ? 0.0 : loc + lr;
      base = blk ? 0.0 : base;
      q = base + loc;
      n += blk ? 1u : 0u;
    }
    cl.q[o] = q;
    cl.n[o] = n;
    big = -q > big ? -q : big;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double z = __shfl_xor(big, off);
    big = z > big ? z : big;
  }
  if (lane == 0) qmax[blockIdx.x] = big;
}

__global__ void __launch_bounds__(64)
k_bylength_halo(uint64_t T, uint64_t I, uint64_t H, const double* __restrict__ q,
                const uint32_t* __restrict__ n, const double* __restrict__ rem, double* __restrict__ hq,
                uint32_t* __restrict__ hn, double* __restrict__ hrem) {
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= I * H) return;
  const uint64_t i = x / H, h = x % H;
  const uint64_t j = h / T, t = h % T;
  const uint64_t o = (((j >> 6) * T + t) * I + i) * 64 + (j & 63);
  hq[x] = q[o];
  hn[x] = n[o];
  hrem[x] = rem[o];
}

struct TermArgs {
  uint64_t T, S, I, H;
  uint32_t C, K;
  int mb;
  const double* __restrict__ sigma;
  const double* __restrict__ q;
  const uint32_t* __restrict__ n;
  const double* __restrict__ rem;
  const uint32_t* __restrict__ btab;
  const double* __restrict__ cum;
  const double* __restrict__ cum_halo;
  const double* __restrict__ hq;
  const uint32_t* __restrict__ hn;
  const double* __restrict__ hrem;
  const ExpectRegion* __restrict__ reg;
  uint64_t n_reg, n_pieces;
  ByLenRec* __restrict__ piece;
};

// the two terms of start site a (plane offset oa, table offset ta) and threshold k
__device__ __forceinline__ void bylength_term(const TermArgs& A, uint64_t i, uint64_t a, uint32_t b,
                                              double sg, double qa, uint32_t na, double ca, double qlast,
                                              uint32_t nlast, double& tr, double& ln) {
  double dq, rem, cb = 0.0;
  bool ok;
  if (b < A.S) {
    const uint32_t T32 = (uint32_t)A.T;
    const uint32_t jb = b / T32, tb = b - jb * T32;
    const uint64_t row = (uint64_t)(jb >> 6) * A.T + tb;
    const uint64_t o = (row * A.I + i) * 64 + (jb & 63);
    dq = A.q[o] - qa;
    ok = A.n[o] == na;
    rem = A.rem[o];
    if (A.mb) cb = A.cum[row * 64 + (jb & 63)];
  } else {   // in the right neighbour's first sites: through the handle's last site
    const uint64_t h = b - A.S;
    dq = (qlast - qa) + A.hq[i * A.H + h];
    ok = nlast == na && A.hn[i * A.H + h] == 0;
    rem = A.hrem[i * A.H + h];
    if (A.mb) cb = A.cum_halo[h];
  }
  const double w = ok ? exp_nonpos(dq < 0.0 ? dq : 0.0) : 0.0;
  const double len = A.mb ? cb - ca : (double)(b - (uint32_t)a + 1u);
  tr = sg * w;
  ln = tr * (len + rem);
}

__global__ void __launch_bounds__(64)
k_bylength_terms(const TermArgs A) {
  const uint64_t i = blockIdx.x / A.C;
  const uint32_t c = blockIdx.x % A.C;
  const int lane = threadIdx.x;
  const uint64_t T = A.T, S = A.S;
  const uint64_t j = (uint64_t)c * 64 + lane;
  const uint64_t s_base = j * T;
  if (s_base >= S || !A.n_reg) return;
  const uint64_t s_end = (S - s_base < T ? S : s_base + T) - 1;
  // the last region that begins at or in front of the lane-chunk's last site (k_expect_walk)
  uint64_t r;
  uint64_t rb = ~0ull, re = 0, rp = 0;
  {
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
  double qlast = 0.0;
  uint32_t nlast = 0;
  if (A.H) {
    const uint64_t jl = (S - 1) / T, tl = (S - 1) % T;
    const uint64_t o = (((jl >> 6) * T + tl) * A.I + i) * 64 + (jl & 63);
    qlast = A.q[o];
    nlast = A.n[o];
  }
  const uint64_t CT = (uint64_t)A.C * T;
  ByLenRec* const pc_out = A.piece + i * A.n_pieces * A.K;
  double at[kByLenMaxK], al[kByLenMaxK];
#pragma unroll
  for (uint32_t k = 0; k < kByLenMaxK; ++k) at[k] = al[k] = 0.0;
  for (uint64_t t = s_end - s_base + 1; t-- > 0;) {
    const uint64_t s = s_base + t;
    if (re == 0) break;   // no region in front of here reaches into the lane-chunk
    if (s >= re) continue;
    const uint64_t row = (uint64_t)c * T + t;
    const uint64_t o = (row * A.I + i) * 64 + lane;
    const double sg = A.sigma[o], qa = A.q[o];
    const uint32_t na = A.n[o];
    const double ca = A.mb ? A.cum[row * 64 + lane] : 0.0;
#pragma unroll
    for (uint32_t k = 0; k < kByLenMaxK; ++k) {
      if (k < A.K) {
        const uint32_t b = A.btab[((uint64_t)k * CT + row) * 64 + lane];
        if (b != kByLenNone && sg > 0.0) {
          double tr, ln;
          bylength_term(A, i, s, b, sg, qa, na, ca, qlast, nlast, tr, ln);
          at[k] += tr;
          al[k] += ln;
        }
      }
    }
    if (s == rb || s == s_base) {   // the piece is complete
      ByLenRec* po = pc_out + (rp + (j - rb / T)) * A.K;
#pragma unroll
      for (uint32_t k = 0; k < kByLenMaxK; ++k) {
        if (k < A.K) po[k] = ByLenRec{at[k], al[k]};
        at[k] = al[k] = 0.0;
      }
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

// one lane per (individual, region, threshold): the pieces in site order, the first one's value first
__global__ void __launch_bounds__(64)
k_bylength_finish(const ExpectRegion* __restrict__ reg, uint64_t n_reg, uint64_t I, uint64_t T, uint32_t K,
                  uint64_t n_pieces, const ByLenRec* __restrict__ piece, ByLenRec* __restrict__ out) {
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_reg * I * K) return;
  const uint64_t k = x % K, g = (x / K) % n_reg, i = x / K / n_reg;
  const ExpectRegion R = reg[g];
  const uint64_t np = expect_pieces(R.begin, R.end, T);
  const ByLenRec* p = piece + (i * n_pieces + R.piece0) * K + k;
  ByLenRec acc = p[0];
  for (uint64_t n = 1; n < np; ++n) {
    acc.tracts += p[n * K].tracts;
    acc.length += p[n * K].length;
  }
  out[x] = acc;
}

// exact mode: the forward array as k_expect_exact fills it; the backward recursion right to left
// with sigma_s, ln rho_s and rem_s per site; Q_s and n_s left to right; then every region's terms
// added to 0 from its last site to its first.  PI: x01 + x11 per site goes to the plane pi [S][I].
template <bool PI>
__global__ void __launch_bounds__(64)
k_bylength_exact(const double* __restrict__ eprob, const double* __restrict__ pos, double* __restrict__ fw,
                 uint64_t S, uint64_t I, const double* __restrict__ indF, const double* __restrict__ alpha,
                 int mb, uint32_t K, const ByLenCells cl, const uint32_t* __restrict__ btab,
                 const double* __restrict__ cum, const ExpectRegion* __restrict__ reg, uint64_t n_reg,
                 ByLenRec* __restrict__ out, double* __restrict__ qmax, int* __restrict__ flags,
                 double* __restrict__ pi) {
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
      const double cs = d < kDStart ? det_exp(-al * d) : 0.0;
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
  double b0 = 0.0, b1 = 0.0, x = 0.0;   // log beta and rem of the last site
  for (uint64_t s = S; s-- > 0;) {
    const double d = pos[s];
    const bool start = !(d < kDStart) || s == 0;
    const double cs = d < kDStart ? det_exp(-al * d) : 0.0;
    const double a = 1 - cs;
    const double t00 = det_log(a * q0 + cs), t01 = det_log(a * q1);
    const double t10 = det_log(a * q0), t11 = det_log(a * q1 + cs);
    const double u0 = eprob[(s * I + i) * 2] + b0, u1 = eprob[(s * I + i) * 2 + 1] + b1;
    const double m00 = t00 + u0, m01 = t01 + u1, m10 = t10 + u0, m11 = t11 + u1;
    const double lf0 = s ? fw[(s * I + i) * 2] : lq0, lf1 = s ? fw[(s * I + i) * 2 + 1] : lq1;
    const double n00 = lf0 + m00, n01 = lf0 + m01, n10 = lf1 + m10, n11 = lf1 + m11;
    const double lz = lsum2(lsum2(n00, n10), lsum2(n01, n11));
    const double x01 = exp0(n01 - lz), x11 = exp0(n11 - lz);
    const double L11 = ln_share_log(m11, m10);
    const double rho = (start || !(L11 > NGH_NEG_INF)) ? 0.0 : det_exp(L11);
    const bool blocked = !(rho > 0.0);
    cl.sigma[s * I + i] = start ? x01 + x11 : x01;
    if (PI) pi[s * I + i] = x01 + x11;
    cl.q[s * I + i] = blocked ? kBlocked : L11;
    cl.m[s * I + i] = x;
    x = blocked ? 0.0 : rho * ((mb ? d : 1.0) + x);
    const double n0 = lsum2(m00, m01), n1 = lsum2(m10, m11);
    const double M = (n1 >= n0) ? n1 : n0;
    const bool fin = M > NGH_NEG_INF;
    b0 = fin ? n0 - M : n0;
    b1 = fin ? n1 - M : n1;
  }
  {
    double q = 0.0, big = 0.0;
    uint32_t n = 0;
    for (uint64_t s = 0; s < S; ++s) {
      const double lr = cl.q[s * I + i];
      const bool blk = lr > 0.0;
      q = blk ? 0.0 : q + lr;
      n += blk ? 1u : 0u;
      cl.q[s * I + i] = q;
      cl.n[s * I + i] = n;
      big = -q > big ? -q : big;
    }
    qmax[i] = big;
  }
  for (uint64_t r = n_reg; r-- > 0;) {
    const ExpectRegion R = reg[r];
    double at[kByLenMaxK], ln[kByLenMaxK];
#pragma unroll
    for (uint32_t k = 0; k < kByLenMaxK; ++k) at[k] = ln[k] = 0.0;
    for (uint64_t s = R.end; s-- > R.begin;) {
      const double sg = cl.sigma[s * I + i], qa = cl.q[s * I + i];
      const uint32_t na = cl.n[s * I + i];
      const double ca = mb ? cum[s] : 0.0;
#pragma unroll
      for (uint32_t k = 0; k < kByLenMaxK; ++k) {
        if (k < K) {
          const uint32_t b = btab[(uint64_t)k * S + s];
          if (b != kByLenNone && sg > 0.0) {
            const double dq = cl.q[(uint64_t)b * I + i] - qa;
            const double w = cl.n[(uint64_t)b * I + i] == na ? det_exp(dq < 0.0 ? dq : 0.0) : 0.0;
            const double len = mb ? cum[b] - ca : (double)(b - (uint32_t)s + 1u);
            const double tr = sg * w;
            at[k] += tr;
            ln[k] += tr * (len + cl.m[(uint64_t)b * I + i]);
          }
        }
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < kByLenMaxK; ++k)
      if (k < K) out[(i * n_reg + r) * K + k] = ByLenRec{at[k], ln[k]};
  }
}

}  // namespace

uint64_t bylength_cell_count(const FastState* fs, uint64_t S, uint64_t I) {
  return fs ? (uint64_t)fs->C * fs->T * I * 64 : S * I;
}

bool bylength_fast_cells(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                         bool has_vin, bool mb, const ByLenCells& cells, const ByLenChunks& ch,
                         const double* carry_in, double* carry_out, double* qmax, double* pi) {
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
  A.sigma = cells.sigma;
  A.q = cells.q;
  A.m = cells.m;
  A.map = ch.map;
  A.qtail = ch.qtail;
  A.nblk = ch.nblk;
  A.pi = pi;
  const dim3 grid((unsigned)(fs.I * fs.C)), block(64);
  if (pi) hipLaunchKernelGGL(k_bylength_walk<true>, grid, block, 0, st, A);
  else hipLaunchKernelGGL(k_bylength_walk<false>, grid, block, 0, st, A);
  hipLaunchKernelGGL(k_bylength_scan, dim3((unsigned)fs.I), block, 0, st, fs.C, ch.map, ch.qtail, ch.nblk,
                     carry_in, carry_out, ch.endM, ch.endD, ch.q0, ch.n0);
  hipLaunchKernelGGL(k_bylength_fill, grid, block, 0, st, fs.T, fs.S, fs.I, fs.C, mb ? 1 : 0, fs.pos_il,
                     cells, ch.endM, ch.endD, ch.q0, ch.n0, qmax);
  return hipGetLastError() == hipSuccess;
}

void bylength_fast_halo(FastState& fs, hipStream_t st, bool mb, const ByLenCells& cells, uint64_t H,
                        double* q, uint32_t* n, double* rem) {
  hipLaunchKernelGGL(k_bylength_halo, dim3((unsigned)((fs.I * H + 63) / 64)), dim3(64), 0, st, fs.T, fs.I, H,
                     cells.q, cells.n, mb ? cells.d : cells.m, q, n, rem);
}

bool bylength_fast_terms(FastState& fs, hipStream_t st, bool mb, uint32_t K, const ByLenCells& cells,
                         const uint32_t* btab, const double* cum, const double* cum_halo,
                         const ByLenHalo& halo, const ExpectRegion* d_reg, uint64_t n_reg,
                         uint64_t n_pieces, ByLenRec* d_piece, ByLenRec* d_out) {
  if (!n_reg) return true;
  TermArgs A;
  A.T = fs.T;
  A.S = fs.S;
  A.I = fs.I;
  A.H = halo.H;
  A.C = fs.C;
  A.K = K;
  A.mb = mb ? 1 : 0;
  A.sigma = cells.sigma;
  A.q = cells.q;
  A.n = cells.n;
  A.rem = mb ? cells.d : cells.m;
  A.btab = btab;
  A.cum = cum;
  A.cum_halo = cum_halo;
  A.hq = halo.q;
  A.hn = halo.n;
  A.hrem = halo.rem;
  A.reg = d_reg;
  A.n_reg = n_reg;
  A.n_pieces = n_pieces;
  A.piece = d_piece;
  hipLaunchKernelGGL(k_bylength_terms, dim3((unsigned)(fs.I * fs.C)), dim3(64), 0, st, A);
  hipLaunchKernelGGL(k_bylength_finish, dim3((unsigned)((n_reg * fs.I * K + 63) / 64)), dim3(64), 0, st,
                     d_reg, n_reg, fs.I, fs.T, K, n_pieces, d_piece, d_out);
  return hipGetLastError() == hipSuccess;
}

void launch_bylength_exact(hipStream_t st, const double* eprob, const double* pos, double* fw, uint64_t S,
                           uint64_t I, const double* d_indF, const double* d_alpha, bool mb, uint32_t K,
                           const ByLenCells& cells, const uint32_t* btab, const double* cum,
                           const ExpectRegion* d_reg, uint64_t n_reg, ByLenRec* d_out, double* qmax,
                           int* d_flags, double* pi) {
  const dim3 grid((unsigned)((I + 63) / 64)), block(64);
  if (pi)
    hipLaunchKernelGGL(k_bylength_exact<true>, grid, block, 0, st, eprob, pos, fw, S, I, d_indF, d_alpha,
                       mb ? 1 : 0, K, cells, btab, cum, d_reg, n_reg, d_out, qmax, d_flags, pi);
  else
    hipLaunchKernelGGL(k_bylength_exact<false>, grid, block, 0, st, eprob, pos, fw, S, I, d_indF, d_alpha,
                       mb ? 1 : 0, K, cells, btab, cum, d_reg, n_reg, d_out, qmax, d_flags, pi);
}

}  // namespace nghmm
