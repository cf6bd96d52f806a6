// kernels_long.hip -- P_k(s) = P(site s lies in an IBD tract of length >= L_k | y), exactly, per
// individual, site and threshold (include/nghmm.h: nghmm_ibd_long has the definition).
//
// The cells are kernels_bylength.hip's: sigma_s, the prefix Q_s, the blocked count n_s and, from
// the same walk, the posterior pi_s.  With T_k(a) = sigma_a W(a, b_k(a)) and lo = lo_k(s),
//   P_k(s) = pi_lo W(lo, s) + sum of T_k(a) over lo < a <= s      (from s's chromosome start if no lo)
// A term T_k(a) with a blocked step in (a, s] is exactly 0 (its window reaches beyond s), so the
// sum is a difference of the prefix U of T_k that restarts at every blocked step, where Q does:
//   n_lo == n_s:  P = pi_lo exp(Q_s - Q_lo) + max(U_s - U_lo, 0);   else  P = U_s;   P = min(P, pi_s).
// One threshold at a time, so that the scratch does not grow with K.  Fast mode (a lane owns a
// lane-chunk of T consecutive sites; planes tile-major):
//   k_long_terms    a lane per lane-chunk, first site to last: T_k(a) (the gather at b_k(a) is
//                   k_bylength_terms') into a plane, the lane's own running sum, restarted at every
//                   blocked step, into the packed records; per lane-chunk the sum behind its last
//                   blocked step and whether it has one;
//   k_long_scan     one wave per individual: what enters every lane-chunk, as k_bylength_scan forms
//                   the Q that enters it (Hillis-Steele steps 1, 2, .., 32, the waves in site order);
//   k_long_prefix   U_s = (what enters the lane-chunk, if no blocked step since) + (the lane's sum);
//   k_long_p        P_k(s) from one packed record at lo_k(s) and the site's own;
//   k_long_pieces / k_long_finish   the region records, pieces at the lane-chunk edges added from
//                   their last site to their first, the pieces in site order (k_bylength_terms);
//   k_long_sites    a wave per tile row (64 sites), the individuals in index order;
//   k_long_post     tile-major -> [I][S] through LDS.
// Exact mode: one lane per individual, serial over the sites, planes [S][I].
// No float atomics: every sum has one order -- the same bits on every call.
#include "fast_dev.hpp"
#include "kernels_long.hpp"
#include "lnshare_dev.hpp"

namespace nghmm {

namespace {

__global__ void __launch_bounds__(256)
k_long_pack(uint64_t cells, const double* __restrict__ pi, const double* __restrict__ q,
            const uint32_t* __restrict__ n, LongCell* __restrict__ rec) {
  const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= cells) return;
  LongCell r;
  r.pi = pi[o];
  r.q = q[o];
  r.u = 0.0;
  r.n = n[o];
  r.pad = 0;
  rec[o] = r;
}

struct TermArgs {
  uint64_t T, S, I, H;
  uint32_t C;
  const double* __restrict__ hq;     // Q and n of the right neighbour's first H sites, [I][H]
  const uint32_t* __restrict__ hn;
  const double* __restrict__ sigma;
  const double* __restrict__ q;
  const uint32_t* __restrict__ n;
  const uint32_t* __restrict__ n0;   // per lane-chunk: n at the site in front of its first
  const uint32_t* __restrict__ btab;
  double* __restrict__ tk;
  LongCell* __restrict__ rec;
  double* __restrict__ utail;
  uint32_t* __restrict__ ublk;
};

__global__ void __launch_bounds__(64)
k_long_terms(const TermArgs A) {
  const uint64_t i = blockIdx.x / A.C;
  const uint32_t c = blockIdx.x % A.C;
  const int lane = threadIdx.x;
  const uint64_t T = A.T, S = A.S;
  const uint64_t J = (uint64_t)A.C * 64, j = (uint64_t)c * 64 + lane, s_base = j * T;
  const uint64_t cell0 = (((uint64_t)c * T) * A.I + i) * 64 + lane, step = A.I * 64;
  const uint32_t T32 = (uint32_t)T;
  const uint32_t n_first = A.n0[i * J + j];
  uint32_t n_prev = n_first;
  double loc = 0.0;
  double qlast = 0.0;
  uint32_t nlast = 0;
  if (A.H) {
    const uint64_t jl = (S - 1) / T, tl = (S - 1) % T;
    const uint64_t ol = (((jl >> 6) * T + tl) * A.I + i) * 64 + (jl & 63);
    qlast = A.q[ol];
    nlast = A.n[ol];
  }
  for (uint64_t t = 0; t < T; ++t) {
    const uint64_t o = cell0 + t * step;
    double tk = 0.0;
    if (s_base + t < S) {
      const double sg = A.sigma[o], qa = A.q[o];
      const uint32_t na = A.n[o];
      const uint32_t b = A.btab[((uint64_t)c * T + t) * 64 + lane];
      if (b != kByLenNone && sg > 0.0) {
        double dq = 0.0;
        bool ok = false;
        if (b < S) {
          const uint32_t jb = b / T32, tb = b - jb * T32;
          const uint64_t ob = (((uint64_t)(jb >> 6) * T + tb) * A.I + i) * 64 + (jb & 63);
          dq = A.q[ob] - qa;
          ok = A.n[ob] == na;
        } else if (b - S < A.H) {   // in the right neighbour's first sites: through the handle's last site
          const uint64_t h = b - S;
          dq = (qlast - qa) + A.hq[i * A.H + h];
          ok = nlast == na && A.hn[i * A.H + h] == 0;
        }
        tk = ok ? sg * exp_nonpos(dq < 0.0 ? dq : 0.0) : 0.0;
      }
      loc = na != n_prev ? tk : loc + tk;
      n_prev = na;
    }
    A.tk[o] = tk;
    A.rec[o].u = loc;
  }
  A.utail[i * J + j] = loc;
  A.ublk[i * J + j] = n_prev != n_first ? 1u : 0u;
}

// One wave per individual, left to right: (tail sum, blocked) under
// (L, R) -> (R.n ? R.q : L.q + R.q, L.n + R.n), as k_bylength_scan.
__global__ void __launch_bounds__(64)
k_long_scan(uint32_t C, const double* __restrict__ utail, const uint32_t* __restrict__ ublk,
            double* __restrict__ u0) {
  const uint64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  const uint64_t J = (uint64_t)C * 64;
  double cq = 0.0;
  for (uint32_t c = 0; c < C; ++c) {
    const uint64_t o = i * J + (uint64_t)c * 64 + lane;
    double q = utail[o];
    uint32_t n = ublk[o];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double q2 = __shfl_up(q, off);
      const uint32_t n2 = __shfl_up(n, off);
      if (lane >= off) {
        q = n ? q : q2 + q;
        n += n2;
      }
    }
    const double pq = __shfl_up(q, 1);
    const uint32_t pn = __shfl_up(n, 1);
    u0[o] = lane ? (pn ? pq : cq + pq) : cq;
    const double lq = __shfl(q, 63);
    const uint32_t ln = __shfl(n, 63);
    cq = ln ? lq : cq + lq;
  }
}

__global__ void __launch_bounds__(64)
k_long_prefix(uint64_t T, uint64_t I, uint32_t C, const uint32_t* __restrict__ n0,
              const double* __restrict__ u0, LongCell* __restrict__ rec) {
  const uint64_t i = blockIdx.x / C;
  const uint32_t c = blockIdx.x % C;
  const int lane = threadIdx.x;
  const uint64_t J = (uint64_t)C * 64, j = (uint64_t)c * 64 + lane;
  const uint64_t cell0 = (((uint64_t)c * T) * I + i) * 64 + lane, step = I * 64;
  const uint32_t nin = n0[i * J + j];
  const double base = u0[i * J + j];
#pragma unroll 8
  for (uint64_t t = 0; t < T; ++t) {
    LongCell* r = rec + cell0 + t * step;
    r->u = (r->n == nin ? base : 0.0) + r->u;
  }
}

// What a site shard takes from its left neighbour, h = 0 at the neighbour's last site and counting
// back from there, [I][H] each: pi, the sum of ln rho from the site to the cut, the blocked steps
// from the site to the cut, the sum of T_k over the sites behind it (suf, this threshold's); and
// all [I], the neighbour's U at its last site.
struct LeftHalo {
  uint64_t H;
  uint32_t has_left;
  const double* __restrict__ pi;
  const double* __restrict__ qc;
  const uint32_t* __restrict__ nc;
  const double* __restrict__ suf;
  const double* __restrict__ all;
};

template <bool EXACT>
__device__ __forceinline__ double long_exp(double dq) {
  return EXACT ? det_exp(dq < 0.0 ? dq : 0.0) : exp_nonpos(dq < 0.0 ? dq : 0.0);
}

// P of a site from its own record and the one at lo (none: null)
template <bool EXACT>
__device__ __forceinline__ double long_p(const LongCell& r, const LongCell* g) {
  double a = 0.0, b = r.u;
  if (g) {
    if (g->n == r.n) {
      a = g->pi * long_exp<EXACT>(r.q - g->q);
      b = r.u - g->u;
      b = b > 0.0 ? b : 0.0;
    }
  }
  const double p = a + b;
  return p < r.pi ? p : r.pi;
}

__global__ void __launch_bounds__(64)
k_long_p(uint64_t T, uint64_t S, uint64_t I, uint32_t C, const LongCell* __restrict__ rec,
         const uint32_t* __restrict__ lotab, const LeftHalo L, double* __restrict__ P) {
  const uint64_t i = blockIdx.x / C;
  const uint32_t c = blockIdx.x % C;
  const int lane = threadIdx.x;
  const uint64_t j = (uint64_t)c * 64 + lane, s_base = j * T;
  const uint64_t cell0 = (((uint64_t)c * T) * I + i) * 64 + lane, step = I * 64;
  const uint32_t T32 = (uint32_t)T;
  for (uint64_t t = 0; t < T; ++t) {
    const uint64_t o = cell0 + t * step;
    double p = 0.0;
    if (s_base + t < S) {
      const LongCell r = rec[o];
      const uint32_t lo = lotab[((uint64_t)c * T + t) * 64 + lane];
      if (lo != kByLenNone && lo < S) {
        const uint32_t jl = lo / T32, tl = lo - jl * T32;
        const LongCell g = rec[(((uint64_t)(jl >> 6) * T + tl) * I + i) * 64 + (jl & 63)];
        p = long_p<false>(r, &g);
      } else if (L.has_left && r.n == 0) {
        // no blocked step from the cut to s: the window and the late starts go on in the left
        // neighbour, whose parts are products and sums of non-negative terms
        double a = 0.0, b = r.u;
        if (lo == kByLenNone) {
          b = L.all[i] + r.u;
        } else if (lo - S < L.H) {
          const uint64_t x = i * L.H + (lo - S);
          a = L.nc[x] == 0 ? L.pi[x] * long_exp<false>(L.qc[x] + r.q) : 0.0;
          b = L.suf[x] + r.u;
        }
        p = a + b;
        p = p < r.pi ? p : r.pi;
      } else {
        p = long_p<false>(r, nullptr);
      }
    }
    P[o] = p;
  }
}

// the left halo a shard gives: x = i (H + 1) + h; h < H the site S - 1 - h, h == H the prefix at the
// last site
__global__ void __launch_bounds__(64)
k_long_halo_left(uint64_t T, uint64_t S, uint64_t I, uint64_t H, const LongCell* __restrict__ rec,
                 const double* __restrict__ tk, double* __restrict__ hpi, double* __restrict__ hqc,
                 uint32_t* __restrict__ hnc, double* __restrict__ ht, double* __restrict__ hall) {
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= I * (H + 1)) return;
  const uint64_t i = x / (H + 1), h = x % (H + 1);
  const uint64_t jl = (S - 1) / T, tl = (S - 1) % T;
  const LongCell last = rec[(((jl >> 6) * T + tl) * I + i) * 64 + (jl & 63)];
  if (h == H) {
    hall[i] = last.u;
    return;
  }
  const uint64_t s = S - 1 - h, j = s / T, t = s % T;
  const uint64_t o = (((j >> 6) * T + t) * I + i) * 64 + (j & 63);
  const LongCell r = rec[o];
  hpi[i * H + h] = r.pi;
  hqc[i * H + h] = last.q - r.q;
  hnc[i * H + h] = last.n - r.n;
  ht[i * H + h] = tk[o];
}

struct PieceArgs {
  uint64_t T, S, I;
  uint32_t C, has_vin;
  const double* __restrict__ pos_il;
  const double* __restrict__ p;
  const double* __restrict__ tk;
  const ExpectRegion* __restrict__ reg;
  uint64_t n_reg, n_pieces;
  LongRec* __restrict__ piece;
};

// a site's two terms: P, and d_s (P - T_k(s)) off a chromosome start (never below 0)
__device__ __forceinline__ void long_site_terms(double p, double tk, double d, bool start, double& a, double& b) {
  const double joint = p - tk;
  a = p;
  b = (start || !(joint > 0.0)) ? 0.0 : d * joint;
}

// The region logic is k_bylength_terms': a lane per lane-chunk from its last site to its first, one
// piece per (lane-chunk, region overlap).
__global__ void __launch_bounds__(64)
k_long_pieces(const PieceArgs A) {
  const uint64_t i = blockIdx.x / A.C;
  const uint32_t c = blockIdx.x % A.C;
  const int lane = threadIdx.x;
  const uint64_t T = A.T, S = A.S;
  const uint64_t j = (uint64_t)c * 64 + lane;
  const uint64_t s_base = j * T;
  if (s_base >= S || !A.n_reg) return;
  const uint64_t s_end = (S - s_base < T ? S : s_base + T) - 1;
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
  LongRec* const pc_out = A.piece + i * A.n_pieces;
  double as = 0.0, am = 0.0;
  for (uint64_t t = s_end - s_base + 1; t-- > 0;) {
    const uint64_t s = s_base + t;
    if (re == 0) break;   // no region in front of here reaches into the lane-chunk
    if (s >= re) continue;
    const uint64_t row = (uint64_t)c * T + t;
    const uint64_t o = (row * A.I + i) * 64 + lane;
    const double d = A.pos_il[row * 64 + lane];
    double a, b;
    long_site_terms(A.p[o], A.tk[o], d, !(d < kDStart) || (s == 0 && !A.has_vin), a, b);
    as += a;
    am += b;
    if (s == rb || s == s_base) {   // the piece is complete
      pc_out[rp + (j - rb / T)] = LongRec{as, am};
      as = am = 0.0;
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

// one lane per (individual, region): the pieces in site order, the first one's value first
__global__ void __launch_bounds__(64)
k_long_finish(const ExpectRegion* __restrict__ reg, uint64_t n_reg, uint64_t I, uint64_t T, uint32_t K,
              uint32_t k, uint64_t n_pieces, const LongRec* __restrict__ piece, LongRec* __restrict__ out) {
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_reg * I) return;
  const uint64_t g = x % n_reg, i = x / n_reg;
  const ExpectRegion R = reg[g];
  const uint64_t np = expect_pieces(R.begin, R.end, T);
  const LongRec* p = piece + i * n_pieces + R.piece0;
  LongRec acc = p[0];
  for (uint64_t n = 1; n < np; ++n) {
    acc.sites += p[n].sites;
    acc.mb += p[n].mb;
  }
  out[x * K + k] = acc;
}

// A wave per tile row: its 64 sites, the individuals in index order.
__global__ void __launch_bounds__(64)
k_long_sites(uint64_t T, uint64_t S, uint64_t I, const double* __restrict__ P, double thr, uint32_t K,
             uint32_t k, LongSite* __restrict__ out) {
  const uint64_t row = blockIdx.x;   // c T + t
  const int lane = threadIdx.x;
  const uint64_t c = row / T, t = row % T;
  const uint64_t s = (c * 64 + lane) * T + t;
  const double* p = P + row * I * 64 + lane;
  double sum = 0.0;
  uint64_t cnt = 0;
  for (uint64_t i = 0; i < I; ++i) {
    const double v = p[i * 64];
    sum += v;
    cnt += v >= thr ? 1u : 0u;
  }
  if (s < S) out[s * K + k] = LongSite{sum, cnt};
}

// Tile-major [c T + t][i][64] to [I][S]: a block moves the 64 lanes x 64 rows t0 .. t0 + 63 of one
// (individual, wave) through LDS; both sides run along their contiguous index.
constexpr int kTr = 64;
__global__ void __launch_bounds__(256)
k_long_post(uint64_t T, uint64_t S, uint64_t I, uint32_t C, uint32_t tiles, const double* __restrict__ P,
            double* __restrict__ post) {
  __shared__ double tile[kTr][kTr + 1];
  const uint64_t x = blockIdx.x;
  const uint32_t tt = (uint32_t)(x % tiles);
  const uint32_t c = (uint32_t)((x / tiles) % C);
  const uint64_t i = x / tiles / C;
  const int lane = threadIdx.x & 63, y = threadIdx.x >> 6;
  const uint64_t t0 = (uint64_t)tt * kTr;
  for (int r = y; r < kTr; r += 4) {
    const uint64_t t = t0 + r;
    if (t < T) tile[r][lane] = P[(((uint64_t)c * T + t) * I + i) * 64 + lane];
  }
  __syncthreads();
  for (int l = y; l < kTr; l += 4) {   // lane-chunk l of the wave, its sites t0 + lane
    const uint64_t t = t0 + lane;
    const uint64_t s = ((uint64_t)c * 64 + l) * T + t;
    if (t < T && s < S) post[i * S + s] = tile[lane][l];
  }
}

// ---- exact mode: planes [S][I] ----

__global__ void __launch_bounds__(64)
k_long_exact(uint64_t S, uint64_t I, const double* __restrict__ sigma, const double* __restrict__ q,
             const uint32_t* __restrict__ n, const uint32_t* __restrict__ btab,
             const uint32_t* __restrict__ lotab, double* __restrict__ tkp, LongCell* __restrict__ rec,
             double* __restrict__ P) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  double u = 0.0;
  uint32_t n_prev = 0;
  for (uint64_t s = 0; s < S; ++s) {
    const uint64_t o = s * I + i;
    const double sg = sigma[o], qa = q[o];
    const uint32_t na = n[o];
    const uint32_t b = btab[s];
    double tk = 0.0;
    if (b != kByLenNone && b < S && sg > 0.0) {
      const double dq = q[(uint64_t)b * I + i] - qa;
      const double w = n[(uint64_t)b * I + i] == na ? det_exp(dq < 0.0 ? dq : 0.0) : 0.0;
      tk = sg * w;
    }
    u = na != n_prev ? tk : u + tk;
    n_prev = na;
    tkp[o] = tk;
    LongCell r = rec[o];
    r.u = u;
    rec[o] = r;
    const uint32_t lo = lotab[s];
    if (lo != kByLenNone && lo <= s) {
      const LongCell g = rec[(uint64_t)lo * I + i];
      P[o] = long_p<true>(r, &g);
    } else {
      P[o] = long_p<true>(r, nullptr);
    }
  }
}

// one lane per (individual, region): its sites' terms added to 0 from its last site to its first
__global__ void __launch_bounds__(64)
k_long_exact_regions(uint64_t S, uint64_t I, const double* __restrict__ pos, const double* __restrict__ P,
                     const double* __restrict__ tk, const ExpectRegion* __restrict__ reg, uint64_t n_reg,
                     uint32_t K, uint32_t k, LongRec* __restrict__ out) {
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_reg * I) return;
  const uint64_t i = x % I, g = x / I;
  const ExpectRegion R = reg[g];
  double as = 0.0, am = 0.0;
  for (uint64_t s = R.end; s-- > R.begin;) {
    const double d = pos[s];
    double a, b;
    long_site_terms(P[s * I + i], tk[s * I + i], d, !(d < kDStart) || s == 0, a, b);
    as += a;
    am += b;
  }
  out[(i * n_reg + g) * K + k] = LongRec{as, am};
}

__global__ void __launch_bounds__(64)
k_long_exact_sites(uint64_t S, uint64_t I, const double* __restrict__ P, double thr, uint32_t K, uint32_t k,
                   LongSite* __restrict__ out) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  double sum = 0.0;
  uint64_t cnt = 0;
  for (uint64_t i = 0; i < I; ++i) {
    const double v = P[s * I + i];
    sum += v;
    cnt += v >= thr ? 1u : 0u;
  }
  out[s * K + k] = LongSite{sum, cnt};
}

// [S][I] to [I][S] in 64 x 64 tiles through LDS
__global__ void __launch_bounds__(256)
k_long_exact_post(uint64_t S, uint64_t I, uint64_t tiles_i, const double* __restrict__ P,
                  double* __restrict__ post) {
  __shared__ double tile[kTr][kTr + 1];
  const uint64_t s0 = (blockIdx.x / tiles_i) * kTr, i0 = (blockIdx.x % tiles_i) * kTr;
  const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
  for (int r = y; r < kTr; r += 4)
    if (s0 + r < S && i0 + x < I) tile[r][x] = P[(s0 + r) * I + i0 + x];
  __syncthreads();
  for (int r = y; r < kTr; r += 4)
    if (i0 + r < I && s0 + x < S) post[(i0 + r) * S + s0 + x] = tile[x][r];
}

}  // namespace

void long_pack(hipStream_t st, uint64_t cells, const ByLenCells& cl, LongCell* rec) {
  hipLaunchKernelGGL(k_long_pack, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, cells, cl.d, cl.q, cl.n,
                     rec);
}

bool long_fast_threshold(FastState& fs, hipStream_t st, const ByLenCells& cl, const ByLenChunks& ch,
                         const LongPlanes& pl, const LongChunks& lc, const uint32_t* btab,
                         const uint32_t* lotab, const ByLenHalo& right, const LongLeft& left) {
  if (fs.T == 0 || fs.T >= 0xffffffffull) return false;
  TermArgs A;
  A.T = fs.T;
  A.S = fs.S;
  A.I = fs.I;
  A.H = right.H;
  A.hq = right.q;
  A.hn = right.n;
  A.C = fs.C;
  A.sigma = cl.sigma;
  A.q = cl.q;
  A.n = cl.n;
  A.n0 = ch.n0;
  A.btab = btab;
  A.tk = cl.m;
  A.rec = pl.rec;
  A.utail = lc.utail;
  A.ublk = lc.ublk;
  const dim3 grid((unsigned)(fs.I * fs.C)), block(64);
  hipLaunchKernelGGL(k_long_terms, grid, block, 0, st, A);
  hipLaunchKernelGGL(k_long_scan, dim3((unsigned)fs.I), block, 0, st, fs.C, lc.utail, lc.ublk, lc.u0);
  hipLaunchKernelGGL(k_long_prefix, grid, block, 0, st, fs.T, fs.I, fs.C, ch.n0, lc.u0, pl.rec);
  LeftHalo L;
  L.H = left.H;
  L.has_left = left.has_left ? 1u : 0u;
  L.pi = left.pi;
  L.qc = left.qc;
  L.nc = left.nc;
  L.suf = left.suf;
  L.all = left.all;
  hipLaunchKernelGGL(k_long_p, grid, block, 0, st, fs.T, fs.S, fs.I, fs.C, pl.rec, lotab, L, pl.p);
  return hipGetLastError() == hipSuccess;
}

bool long_fast_regions(FastState& fs, hipStream_t st, const ByLenCells& cl, const LongPlanes& pl,
                       bool has_vin, const ExpectRegion* d_reg, uint64_t n_reg, uint64_t n_pieces,
                       LongRec* d_piece, uint32_t K, uint32_t k, LongRec* d_out) {
  if (!n_reg) return true;
  PieceArgs A;
  A.T = fs.T;
  A.S = fs.S;
  A.I = fs.I;
  A.C = fs.C;
  A.has_vin = has_vin ? 1u : 0u;
  A.pos_il = fs.pos_il;
  A.p = pl.p;
  A.tk = cl.m;
  A.reg = d_reg;
  A.n_reg = n_reg;
  A.n_pieces = n_pieces;
  A.piece = d_piece;
  hipLaunchKernelGGL(k_long_pieces, dim3((unsigned)(fs.I * fs.C)), dim3(64), 0, st, A);
  hipLaunchKernelGGL(k_long_finish, dim3((unsigned)((n_reg * fs.I + 63) / 64)), dim3(64), 0, st, d_reg, n_reg,
                     fs.I, fs.T, K, k, n_pieces, d_piece, d_out);
  return hipGetLastError() == hipSuccess;
}

void long_fast_sites(FastState& fs, hipStream_t st, const LongPlanes& pl, double thr, uint32_t K, uint32_t k,
                     LongSite* d_site) {
  hipLaunchKernelGGL(k_long_sites, dim3((unsigned)(fs.C * fs.T)), dim3(64), 0, st, fs.T, fs.S, fs.I, pl.p, thr, K,
                     k, d_site);
}

void long_fast_post(FastState& fs, hipStream_t st, const LongPlanes& pl, double* d_post) {
  const uint32_t tiles = (uint32_t)((fs.T + kTr - 1) / kTr);
  hipLaunchKernelGGL(k_long_post, dim3((unsigned)(fs.I * fs.C * tiles)), dim3(256), 0, st, fs.T, fs.S, fs.I, fs.C,
                     tiles, pl.p, d_post);
}

void long_fast_halo_left(FastState& fs, hipStream_t st, const ByLenCells& cl, const LongPlanes& pl, uint64_t H,
                         double* hpi, double* hqc, uint32_t* hnc, double* ht, double* hall) {
  hipLaunchKernelGGL(k_long_halo_left, dim3((unsigned)((fs.I * (H + 1) + 63) / 64)), dim3(64), 0, st, fs.T, fs.S,
                     fs.I, H, pl.rec, cl.m, hpi, hqc, hnc, ht, hall);
}

void long_exact_threshold(hipStream_t st, uint64_t S, uint64_t I, const ByLenCells& cl, const LongPlanes& pl,
                          const uint32_t* btab, const uint32_t* lotab) {
  hipLaunchKernelGGL(k_long_exact, dim3((unsigned)((I + 63) / 64)), dim3(64), 0, st, S, I, cl.sigma, cl.q, cl.n,
                     btab, lotab, cl.m, pl.rec, pl.p);
}

void long_exact_regions(hipStream_t st, uint64_t S, uint64_t I, const double* pos, const ByLenCells& cl,
                        const LongPlanes& pl, const ExpectRegion* d_reg, uint64_t n_reg, uint32_t K, uint32_t k,
                        LongRec* d_out) {
  if (!n_reg) return;
  hipLaunchKernelGGL(k_long_exact_regions, dim3((unsigned)((n_reg * I + 63) / 64)), dim3(64), 0, st, S, I, pos,
                     pl.p, cl.m, d_reg, n_reg, K, k, d_out);
}

void long_exact_sites(hipStream_t st, uint64_t S, uint64_t I, const LongPlanes& pl, double thr, uint32_t K,
                      uint32_t k, LongSite* d_site) {
  hipLaunchKernelGGL(k_long_exact_sites, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, S, I, pl.p, thr, K, k,
                     d_site);
}

void long_exact_post(hipStream_t st, uint64_t S, uint64_t I, const LongPlanes& pl, double* d_post) {
  const uint64_t ti = (I + kTr - 1) / kTr, ts = (S + kTr - 1) / kTr;
  hipLaunchKernelGGL(k_long_exact_post, dim3((unsigned)(ti * ts)), dim3(256), 0, st, S, I, ti, pl.p, d_post);
}

}  // namespace nghmm
