// kernels_bounds.hip -- credible bounds of the two ends of an IBD tract (include/nghmm.h:
// nghmm_tract_bounds has the definition).
//
// With the factors of kernels_support.hip, g_t = T_t(1,1) e_t(1) beta_t(1) / beta_{t-1}(1), the run
// through an anchor c reaches up to s with probability H(s) = prod_{t = c+1..s} g_t and down to s
// with G(s) = P(z_s = 1 | y) prod_{t = s+1..c} g_t / P(z_c = 1 | y).  Between two anchors lo < hi
// (a STRETCH: the sites lo + 1 .. hi) one set of factors serves H of lo and G of hi.  Three walks
// of the shape of k_support_walk (forward vectors recomputed block by block from the checkpoints,
// the backward vector carried right to left, products as a double in [0.5, 1) and an exponent):
//   anchor  over the cores: per lane-chunk piece the smallest P(z = 0 | y) -- formed directly, it
//           keeps its relative precision where P(z = 1 | y) saturates -- and its lowest site;
//   sum     over the stretches: per piece ln prod g (and the part in front of the lowest factor 0);
//           the host, which adds the shards' parts in rank order anyway, scans the pieces in site
//           order and hands every piece the value at its edge;
//   locate  over the stretches again: with the edge values every site's ln G and ln H is one
//           logarithm away; per level the piece keeps the first failing site from the anchor
//           outwards (G: the highest failing site; H: the lowest), and k_bounds_finish, one lane
//           per range, the one of its pieces nearest the anchor.
// A factor 0 ends a search exactly: G sees it as a product 0; for H, whose local product runs from
// the far edge, the product restarts at a factor 0 and the site fails by itself -- a site above a
// factor 0 of its piece is compared with a value that is too large, but the 0 below it fails at a
// lower site, and only the lowest counts.  0/0 factors count as 0.  No atomics: every piece is
// written by one lane.
// Exact mode: k_bounds_exact, one lane per individual in log space through detmath.h with the
// normalised forward array of k_support_exact; a range is a single piece.
#include "fast_dev.hpp"
#include "kernels_bounds.hpp"

namespace nghmm {

namespace {

constexpr double LN2 = 0.6931471805599453094;
#define NGH_NEG_INF (-__builtin_huge_val())

// a product of factors in [0, 1] as m 2^ex, m in [0.5, 1) or 0 (as kernels_support.hip)
struct LogProd {
  double P = 1.0;
  int ex = 0;
  __device__ __forceinline__ void mul(double f) {
    P *= f;
    const int e = exp_of(P);
    P = __builtin_ldexp(P, -e);
    ex += e;
  }
  __device__ __forceinline__ double log_value() const { return log(P) + (double)ex * LN2; }
  // ln (x * product)
  __device__ __forceinline__ double log_times(double x) const { return log(x * P) + (double)ex * LN2; }
  __device__ __forceinline__ void reset() {
    P = 1.0;
    ex = 0;
  }
};

enum { PASS_ANCHOR = 0, PASS_SUM = 1, PASS_LOCATE = 2 };

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
  const BoundRange* __restrict__ rec;
  const BoundOff* __restrict__ off;
  void* __restrict__ piece;
  BoundLevels lv;
};

template <int PASS>
__global__ void __launch_bounds__(64)
k_bounds_walk(const WalkArgs A) {
  const uint64_t i = blockIdx.x / A.C;
  const uint32_t c = blockIdx.x % A.C;
  const int lane = threadIdx.x;
  const uint64_t T = A.T, S = A.S;
  const uint64_t J = (uint64_t)A.C * 64;
  const uint64_t j = (uint64_t)c * 64 + lane;
  const uint64_t s_base = j * T;

  // the last range of the individual that starts at or in front of the lane-chunk's last site
  const uint64_t r_lo = A.ioff[i], r_hi = A.ioff[i + 1];
  uint64_t r = r_lo;
  bool active = false;
  uint64_t rfirst = 0, rlast = 0, rslot = 0;
  bool rnofact = false, has_h = false, has_g = false;
  double off_g = 0.0, off_h = 0.0;
  auto take = [&](uint64_t k) {   // range k, if it reaches into the lane-chunk
    const BoundRange R = A.rec[k];
    active = R.last >= s_base;
    rfirst = R.first;
    rlast = R.last;
    rslot = R.piece0 + (j - R.first / T);
    rnofact = R.nofact != 0;
    has_h = (R.search & 1u) != 0;
    has_g = (R.search & 2u) != 0;
    if (PASS == PASS_LOCATE && active) {
      const BoundOff o = A.off[rslot];
      off_g = o.off_g;
      off_h = o.off_h;
    }
  };
  if (s_base < S && r_lo < r_hi) {
    const uint64_t s_end = (S - s_base < T ? S : s_base + T) - 1;
    uint64_t lo = r_lo, hi = r_hi;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (A.rec[mid].first <= s_end) lo = mid + 1;
      else hi = mid;
    }
    r = lo;
    if (r > r_lo) take(r - 1);
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

  // anchor
  double pmin = __builtin_huge_val(), pmin_p1 = 0.0;
  uint64_t psite = 0;
  // sum, locate: the product of the piece's factors above the site; the same from its lowest factor 0
  LogProd acc_g, acc_h;
  bool zero = false;
  double lp1_first = 0.0;
  uint64_t fg[BOUNDS_MAX_LEVELS], fh[BOUNDS_MAX_LEVELS];
#pragma unroll
  for (uint32_t m = 0; m < BOUNDS_MAX_LEVELS; ++m) fg[m] = fh[m] = BOUNDS_NONE;

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
    // forward vectors of the block's sites, from the checkpoint (as k_support_walk)
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
        double p0 = x0 * rx, p1 = x1 * rx;
        if (!(p0 == p0) || !(p1 == p1) || x1 == 0.0) {   // neither state can fill the site; IBD cannot:
          p0 = 1.0;                                      // exactly 1, so that equal sites tie
          p1 = 0.0;
        }
        if (PASS == PASS_ANCHOR) {
          if (p0 <= pmin) {   // right to left: a tie goes to the lower site
            pmin = p0;
            pmin_p1 = p1;
            psite = s;
          }
        } else {
          const bool skip = rnofact && s == rfirst;
          double g1 = fma(a, q1, cc[u]) * u1 * rcp_nr2(n1);
          g1 = (g1 == g1) ? g1 : 0.0;   // 0/0: a state that is excluded already
          if (PASS == PASS_LOCATE && !skip) {
            if (has_g) {
              const double G = acc_g.log_times(p1) + off_g;
#pragma unroll
              for (uint32_t m = 0; m < BOUNDS_MAX_LEVELS; ++m)
                if (m < A.lv.n && G < A.lv.ln[m] && fg[m] == BOUNDS_NONE) fg[m] = s;
            }
            if (has_h) {
              const double H = off_h - acc_h.log_value();
              const bool z = g1 == 0.0;
#pragma unroll
              for (uint32_t m = 0; m < BOUNDS_MAX_LEVELS; ++m)
                if (m < A.lv.n && (z || H < A.lv.ln[m])) fh[m] = s;
            }
          }
          if (PASS == PASS_SUM && s == rfirst) lp1_first = log(p1);
          if (!skip) {
            acc_g.mul(g1);
            if (g1 == 0.0) {
              acc_h.reset();
              zero = true;
            } else {
              acc_h.mul(g1);
            }
          }
        }
        if (s == rfirst || s == s_base) {   // the piece is complete
          if (PASS == PASS_ANCHOR) {
            static_cast<BoundAnchor*>(A.piece)[rslot] = BoundAnchor{pmin, pmin_p1, psite, 0};
            pmin = __builtin_huge_val();
          } else if (PASS == PASS_SUM) {
            static_cast<BoundSum*>(A.piece)[rslot] =
                BoundSum{acc_g.log_value(), acc_h.log_value(), lp1_first, zero ? 1ull : 0ull};
          } else {
            BoundFail* o = static_cast<BoundFail*>(A.piece) + rslot;
#pragma unroll
            for (uint32_t m = 0; m < BOUNDS_MAX_LEVELS; ++m) {
              o->g[m] = fg[m];
              o->h[m] = fh[m];
              fg[m] = fh[m] = BOUNDS_NONE;
            }
          }
          acc_g.reset();
          acc_h.reset();
          zero = false;
          if (s == rfirst) {   // the range in front, if it reaches into the lane-chunk
            --r;
            active = false;
            if (r > r_lo) take(r - 1);
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

// one lane per range: of its pieces' failing sites the one nearest the anchor, per level
__global__ void __launch_bounds__(64)
k_bounds_finish(const BoundRange* __restrict__ rec, uint64_t n, uint64_t T,
                const BoundFail* __restrict__ piece, BoundFail* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const BoundRange R = rec[k];
  const uint64_t np = support_pieces(R.first, R.last, T);
  BoundFail acc = piece[R.piece0];
  for (uint64_t p = 1; p < np; ++p) {   // ascending sites: H keeps its first failure, G its last
    const BoundFail* f = piece + R.piece0 + p;
#pragma unroll
    for (uint32_t m = 0; m < BOUNDS_MAX_LEVELS; ++m) {
      const uint64_t fh = f->h[m], fg = f->g[m];
      if (acc.h[m] == BOUNDS_NONE) acc.h[m] = fh;
      if (fg != BOUNDS_NONE) acc.g[m] = fg;
    }
  }
  out[k] = acc;
}

// gen_func.cpp:135-151 for two values, through detmath.h (as kernels_support.hip)
__device__ __forceinline__ double lsum2(double a0, double a1) {
  const double M = (a1 >= a0) ? a1 : a0;
  if (M == NGH_NEG_INF) return NGH_NEG_INF;
  return det_log(det_exp(a0 - M) + det_exp(a1 - M)) + M;
}

// a sum of logarithms with its rounding error carried along (TwoSum); a term -inf or NaN makes
// the sum -inf (as kernels_support.hip)
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

// exact mode: eprob [S][I][2] log emissions; fw [S + 1][I][2] is scratch for the forward values,
// normalised at every site (k_support_exact says why).  The same three passes, one lane per
// individual; a range is one piece, slot = its index.
template <int PASS>
__global__ void __launch_bounds__(64)
k_bounds_exact(const double* __restrict__ eprob, const double* __restrict__ pos,
               double* __restrict__ fw, uint64_t S, uint64_t I,
               const double* __restrict__ indF, const double* __restrict__ alpha,
               const uint64_t* __restrict__ ioff, const BoundRange* __restrict__ rec,
               const BoundOff* __restrict__ off, const BoundLevels lv, void* __restrict__ out,
               int* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  const uint64_t r_lo = ioff[i];
  uint64_t r = ioff[i + 1];
  if (r == r_lo) return;
  const double f = indF[i], al = alpha[i];
  const double q0 = 1 - f, q1 = f;
  BoundRange R = rec[r - 1];
  const uint64_t s_stop = rec[r_lo].first, s_top = R.last;
  {
    double p0 = det_log(q0), p1 = det_log(q1);
    bool bad = false;
    for (uint64_t s = 0; s <= s_top; ++s) {
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
  double b0 = 0.0, b1 = 0.0;   // log beta of the last site
  double pmin = __builtin_huge_val(), pmin_p1 = 0.0;
  uint64_t psite = 0;
  LogSum acc_g, acc_h;
  bool zero = false;
  double lp1_first = 0.0;
  BoundFail fail;
#pragma unroll
  for (uint32_t m = 0; m < BOUNDS_MAX_LEVELS; ++m) fail.g[m] = fail.h[m] = BOUNDS_NONE;
  BoundOff o{0.0, 0.0};
  if (PASS == PASS_LOCATE) o = off[r - 1];
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
      double lp0 = l0 - lz, lp1 = l1 - lz;
      if (!(lp0 == lp0) || !(lp1 == lp1)) {   // a site neither state can fill
        lp0 = 0.0;
        lp1 = NGH_NEG_INF;
      }
      if (PASS == PASS_ANCHOR) {
        const double p0 = det_exp(lp0);
        if (p0 <= pmin) {
          pmin = p0;
          pmin_p1 = det_exp(lp1);
          psite = s;
        }
      } else {
        const bool skip = R.nofact && s == R.first;
        double lg = t11 + u1 - n1;
        lg = (lg == lg) ? lg : NGH_NEG_INF;   // 0/0
        if (PASS == PASS_LOCATE && !skip) {
          if (R.search & 2u) {
            const double G = lp1 + acc_g.value() + o.off_g;
#pragma unroll
            for (uint32_t m = 0; m < BOUNDS_MAX_LEVELS; ++m)
              if (m < lv.n && G < lv.ln[m] && fail.g[m] == BOUNDS_NONE) fail.g[m] = s;
          }
          if (R.search & 1u) {
            const double H = o.off_h - acc_h.value();
            const bool z = !(lg > NGH_NEG_INF);
#pragma unroll
            for (uint32_t m = 0; m < BOUNDS_MAX_LEVELS; ++m)
              if (m < lv.n && (z || H < lv.ln[m])) fail.h[m] = s;
          }
        }
        if (s == R.first) lp1_first = lp1;
        if (!skip) {
          acc_g.add(lg);
          if (!(lg > NGH_NEG_INF)) {
            acc_h = LogSum{};
            zero = true;
          } else {
            acc_h.add(lg);
          }
        }
      }
      if (s == R.first) {
        if (PASS == PASS_ANCHOR) {
          static_cast<BoundAnchor*>(out)[r - 1] = BoundAnchor{pmin, pmin_p1, psite, 0};
          pmin = __builtin_huge_val();
        } else if (PASS == PASS_SUM) {
          static_cast<BoundSum*>(out)[r - 1] =
              BoundSum{acc_g.value(), acc_h.value(), lp1_first, zero ? 1ull : 0ull};
        } else {
          static_cast<BoundFail*>(out)[r - 1] = fail;
#pragma unroll
          for (uint32_t m = 0; m < BOUNDS_MAX_LEVELS; ++m) fail.g[m] = fail.h[m] = BOUNDS_NONE;
        }
        acc_g = LogSum{};
        acc_h = LogSum{};
        zero = false;
        --r;
        if (r > r_lo) {
          R = rec[r - 1];
          if (PASS == PASS_LOCATE) o = off[r - 1];
        }
      }
    }
    const double M = (n1 >= n0) ? n1 : n0;
    const bool fin = M > NGH_NEG_INF;
    b0 = fin ? n0 - M : n0;
    b1 = fin ? n1 - M : n1;
  }
}

template <int PASS>
bool walk(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
          const uint64_t* d_ioff, const BoundRange* d_rec, const BoundOff* d_off,
          const BoundLevels* lv, void* d_piece) {
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
  A.off = d_off;
  A.piece = d_piece;
  A.lv = lv ? *lv : BoundLevels{};
  hipLaunchKernelGGL(k_bounds_walk<PASS>, dim3((unsigned)(fs.I * fs.C)), dim3(64), 0, st, A);
  return hipGetLastError() == hipSuccess;
}

}  // namespace

bool bounds_fast_anchor(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                        const uint64_t* d_ioff, const BoundRange* d_rec, BoundAnchor* d_piece) {
  return walk<PASS_ANCHOR>(fs, st, d_indF, d_alpha, d_ioff, d_rec, nullptr, nullptr, d_piece);
}

bool bounds_fast_sum(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                     const uint64_t* d_ioff, const BoundRange* d_rec, BoundSum* d_piece) {
  return walk<PASS_SUM>(fs, st, d_indF, d_alpha, d_ioff, d_rec, nullptr, nullptr, d_piece);
}

bool bounds_fast_locate(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                        const uint64_t* d_ioff, const BoundRange* d_rec, const BoundOff* d_off,
                        const BoundLevels& lv, BoundFail* d_fail, uint64_t n, BoundFail* d_out) {
  if (!walk<PASS_LOCATE>(fs, st, d_indF, d_alpha, d_ioff, d_rec, d_off, &lv, d_fail)) return false;
  hipLaunchKernelGGL(k_bounds_finish, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, d_rec, n, fs.T, d_fail,
                     d_out);
  return hipGetLastError() == hipSuccess;
}

void launch_bounds_exact(int pass, hipStream_t st, const double* eprob, const double* pos, double* fw,
                         uint64_t S, uint64_t I, const double* d_indF, const double* d_alpha,
                         const uint64_t* d_ioff, const BoundRange* d_rec, const BoundOff* d_off,
                         const BoundLevels& lv, void* d_out, int* d_flags) {
  const dim3 grid((unsigned)((I + 63) / 64)), block(64);
  if (pass == PASS_ANCHOR)
    hipLaunchKernelGGL(k_bounds_exact<PASS_ANCHOR>, grid, block, 0, st, eprob, pos, fw, S, I, d_indF,
                       d_alpha, d_ioff, d_rec, d_off, lv, d_out, d_flags);
  else if (pass == PASS_SUM)
    hipLaunchKernelGGL(k_bounds_exact<PASS_SUM>, grid, block, 0, st, eprob, pos, fw, S, I, d_indF,
                       d_alpha, d_ioff, d_rec, d_off, lv, d_out, d_flags);
  else
    hipLaunchKernelGGL(k_bounds_exact<PASS_LOCATE>, grid, block, 0, st, eprob, pos, fw, S, I, d_indF,
                       d_alpha, d_ioff, d_rec, d_off, lv, d_out, d_flags);
}

}  // namespace nghmm
