// kernels_sample.hip -- whole IBD paths drawn from P(z | data, theta) by forward filtering and
// backward sampling (include/nghmm.h: nghmm_sample_paths has the definition of a draw).
//
// Given its uniform u_s, site s is a MAP from the state of site s + 1 to its own: two bits (its
// value for z_{s+1} = 0 and for z_{s+1} = 1; constant 0, constant 1, identity or swap), and maps
// compose associatively.  So the backward recursion over 10^6 sites is what the E-step is with
// 2x2 operators, with 2-bit maps in their place:
//   k_sample_bounds   the forward vector entering every lane-chunk (the forward half of
//                     k_fast_bounds; a site shard continues the vector of the shard before);
//   k_sample_walk<0>  every lane-chunk recomputes its forward vectors block by block from the
//                     checkpoints, as k_fast_bwd_recompute does, and composes the maps of its
//                     sites right to left, for up to kSampleBatch draws at once: the loads and the
//                     forward recomputation are shared, the draws differ in u alone;
//   k_sample_scan     one wave per (draw, individual): ordered suffix scan of the 64 C lane-chunk
//                     maps (a lane composes its C chunks, shuffles combine the lanes) -> the
//                     state entering every lane-chunk from the right;
//   k_sample_walk<1>  the same walk again, now with that state: writes the sites (eight per
//                     64-bit store) and reduces each lane-chunk to its run statistics;
//   k_sample_fold     the lane-chunk statistics of a (draw, individual) merged in site order.
// The per-site maps are RECOMPUTED in the second walk, not stored: kept, they are 0.25 B per site
// and draw of scratch that is written once and read once -- at 1000 x 1M and 64 draws 16 GB of
// traffic and as much memory -- where the second walk re-reads the 12 B per cell that the first
// one read (shared by the batch's draws) and repeats arithmetic.
// No float atomics anywhere: every sum has one fixed order, the same bits on every call.
// Exact mode: k_sample_exact, one lane per (draw, individual) over the log-space forward array.
#include "fast_dev.hpp"
#include "kernels_sample.hpp"
#include "philox.h"

namespace nghmm {

namespace {

constexpr int RB = (int)kSampleBatch;

// statistics of one lane-chunk of one draw (k_sample_walk<1> -> k_sample_fold)
struct ChunkSeg {
  uint32_t ones, head, tail, inner_n, inner_longest, full;
  double mb;
};
static_assert(sizeof(ChunkSeg) == 32, "ChunkSeg");

// run bookkeeping of a walk from the last site of a range to its first
struct DrawAcc {
  uint32_t ones = 0, cur = 0, tail = 0, inner_n = 0, longest = 0;
  bool at_end = false;   // every site so far is 1 and in the run of the range's last site
  double mb = 0.0;
  // site with state z; brk: the site to its right starts a chromosome; dn: that site's distance
  __device__ __forceinline__ void site(bool first, uint32_t z, bool brk, double dn) {
    if (first) {
      cur = z;
      at_end = z != 0;
    } else if (z && cur && !brk) {
      ++cur;
      mb += dn;
    } else {
      if (cur) {
        if (at_end) tail = cur;
        else {
          ++inner_n;
          longest = cur > longest ? cur : longest;
        }
      }
      at_end = false;
      cur = z;
    }
    ones += z;
  }
  __device__ __forceinline__ uint32_t tail_final() const { return at_end ? cur : tail; }
};

// thresholds of one site: z = 1 iff u * s_l < t_l, l = the state of the site to the right;
// n_k = a(k) T(k, l), T(k, l) = (1 - c) q_l + [k == l] c.  open: no site to the right, or it starts
// a chromosome -- T does not depend on k and the site is drawn from its forward vector alone.
struct Thr {
  double s0, t0, s1, t1;
};
__device__ __forceinline__ Thr site_thr(double a0, double a1, double q0, double q1, double c, bool open) {
  const double an = 1 - c;
  const double A0 = open ? 1.0 : an * q0, A1 = open ? 1.0 : an * q1, cc = open ? 0.0 : c;
  const double n00 = a0 * (A0 + cc), n10 = a1 * A0;   // l = 0
  const double n01 = a0 * A1, n11 = a1 * (A1 + cc);   // l = 1
  return Thr{n00 + n10, n10, n01 + n11, n11};
}

// maps: bit l = the state for input l.  L after R.
__device__ __forceinline__ uint32_t map_comp(uint32_t L, uint32_t R) {
  return ((L >> (R & 1u)) & 1u) | (((L >> ((R >> 1) & 1u)) & 1u) << 1);
}
constexpr uint32_t MAP_ID = 2u;

__device__ __forceinline__ Op op_shfl_up(const Op& m, int off) {
  Op o;
  o.a00 = __shfl_up(m.a00, off);
  o.a01 = __shfl_up(m.a01, off);
  o.a10 = __shfl_up(m.a10, off);
  o.a11 = __shfl_up(m.a11, off);
  o.ex = __shfl_up(m.ex, off);
  return o;
}

// the forward half of k_fast_bounds: bound[i][j][0..1] = the vector entering lane-chunk j
__global__ void __launch_bounds__(64)
k_sample_bounds(const double* __restrict__ lane_ops, uint64_t J, uint32_t C,
                const double* __restrict__ indF, const double* __restrict__ vin,
                double* __restrict__ bound, double* __restrict__ vout) {
  const uint64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  const double f = indF[i];
  const double q0 = vin ? vin[i * 2] : 1 - f, q1 = vin ? vin[i * 2 + 1] : f;
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
  Op P = L;
  for (int off = 1; off < 64; off <<= 1) {
    const Op o = op_shfl_up(P, off);
    if (lane >= off) P = op_mul(o, P);
  }
  Op E = op_shfl_up(P, 1);
  if (lane == 0) E = Op{1.0, 0.0, 0.0, 1.0, 0};
  double v0 = fma(q0, E.a00, q1 * E.a10), v1 = fma(q0, E.a01, q1 * E.a11);
  int ex = 0;
  renorm2(v0, v1, ex);
  for (uint32_t k0 = 0; k0 < C; k0 += PF) {
    Op o[PF];
#pragma unroll
    for (uint32_t u = 0; u < PF; ++u)
      o[u] = op_load(ops + (uint64_t)(k0 + u < C ? k0 + u : C - 1) * 5);
#pragma unroll
    for (uint32_t u = 0; u < PF; ++u) {
      const uint32_t k = k0 + u;
      if (k < C) {
        bd[(uint64_t)k * 4 + 0] = v0;
        bd[(uint64_t)k * 4 + 1] = v1;
        const double n0 = fma(v0, o[u].a00, v1 * o[u].a10);
        const double n1 = fma(v0, o[u].a01, v1 * o[u].a11);
        v0 = n0;
        v1 = n1;
        renorm2(v0, v1, ex);
      }
    }
  }
  if (vout && lane == 63) {
    vout[i * 2] = v0;
    vout[i * 2 + 1] = v1;
  }
}

struct WalkArgs {
  const double* __restrict__ e_il;
  const double* __restrict__ pos_il;
  uint64_t T, S, I, pitch;
  uint32_t C;
  const double* __restrict__ indF;
  const double* __restrict__ alpha;
  const double* __restrict__ bound;
  const double2* __restrict__ ckpt;
  uint64_t seed, site0;
  uint32_t draw0, nd, n_paths;
  int last;
  double d_after;
  uint8_t* __restrict__ maps;
  ChunkSeg* __restrict__ chunk;
  uint8_t* __restrict__ paths;
};

// PASS 0: compose the lane-chunk's maps.  PASS 1: apply them from the state entering on the right.
template <int PASS>
__global__ void __launch_bounds__(64)
k_sample_walk(const WalkArgs A) {
  const uint64_t i = blockIdx.x / A.C;
  const uint32_t c = blockIdx.x % A.C;
  const int lane = threadIdx.x;
  const uint64_t T = A.T, I = A.I, S = A.S;
  const double f = A.indF[i], al = A.alpha[i];
  const double q0 = 1 - f, q1 = f;
  const uint64_t J = (uint64_t)A.C * 64;
  const uint64_t j = (uint64_t)c * 64 + lane;
  const double* bd = A.bound + (i * J + j) * 4;
  const double vin0 = bd[0], vin1 = bd[1];
  const double* ep = A.e_il + ((i * A.C + c) * T) * 64 + lane;
  const double* dp = A.pos_il + ((uint64_t)c * T) * 64 + lane;
  const uint64_t nblk = T / CK;
  const double2* ck = A.ckpt + ((i * A.C + c) * nblk * 2) * 64 + lane;
  const uint64_t s_base = j * T;
  // the site to the right of the lane-chunk: the first of lane-chunk j + 1 (padding past the last)
  double dright = (j + 1 < J) ? A.pos_il[(((j + 1) >> 6) * T) * 64 + ((j + 1) & 63)] : 0.0;
  double cright = coanc(al, dright);
  // T is a multiple of 8: the sites (2k, 2k + 1) of a block share a Philox call iff site0 is even
  const bool aligned = (A.site0 & 1) == 0;
  const uint32_t nd = A.nd;

  uint32_t st[RB];     // PASS 0: the composed map; PASS 1: the state of the site to the right
  DrawAcc acc[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if constexpr (PASS == 0) st[r] = MAP_ID;
    else st[r] = (uint32_t)r < nd ? A.maps[((uint64_t)r * I + i) * J + j] : 0u;
  }
  bool started = false;   // a real (not padding) site has been walked

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
    double f0[CK], f1[CK], cc[CK + 1], dd[CK + 1];
#pragma unroll
    for (int u = 0; u < CK; ++u) {
      cc[u] = coanc(al, dcur[u]);
      dd[u] = dcur[u];
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
    cc[CK] = cright;
    dd[CK] = dright;
    // the thresholds of the block's sites: shared by the draws
    Thr th[CK];
    bool brk[CK];
    double dn[CK];
#pragma unroll
    for (int u = 0; u < CK; ++u) {
      const uint64_t s = s_base + b * CK + u;
      double d = dd[u + 1], cn = cc[u + 1];
      if (s + 1 == S) {   // the handle's last site: nothing follows, or the next shard's first
        d = A.last ? kDStart : A.d_after;
        cn = coanc(al, d < kDStart ? d : kDStart);
      }
      brk[u] = !(d < kDStart);
      dn[u] = d;
      th[u] = site_thr(f0[u], f1[u], q0, q1, cn, brk[u]);
    }
    uint64_t word[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) word[r] = 0;
#pragma unroll
    for (int up = CK / 2 - 1; up >= 0; --up) {
      const uint64_t s_lo = s_base + b * CK + 2 * up;   // local; s_lo + 1 is walked first
      const uint64_t g_lo = A.site0 + s_lo;
      const bool real1 = s_lo + 1 < S;   // (s_lo + 1 real implies s_lo real)
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        if ((uint32_t)r < nd) {
          double uu[2];
          if (aligned) {
            const ngh_philox4 w = ngh_sample_words(A.seed, A.draw0 + r, (uint32_t)i, g_lo >> 1);
            uu[0] = ngh_sample_uniform(w, g_lo);
            uu[1] = ngh_sample_uniform(w, g_lo + 1);
          } else {
            uu[0] = ngh_sample_uniform(ngh_sample_words(A.seed, A.draw0 + r, (uint32_t)i, g_lo >> 1), g_lo);
            uu[1] = ngh_sample_uniform(
                ngh_sample_words(A.seed, A.draw0 + r, (uint32_t)i, (g_lo + 1) >> 1), g_lo + 1);
          }
#pragma unroll
          for (int h = 1; h >= 0; --h) {
            const int u = 2 * up + h;
            const bool pad = s_lo + h >= S;
            const uint32_t z0 = uu[h] * th[u].s0 < th[u].t0 ? 1u : 0u;
            const uint32_t z1 = uu[h] * th[u].s1 < th[u].t1 ? 1u : 0u;
            if constexpr (PASS == 0) {
              const uint32_t m = pad ? MAP_ID : (z0 | (z1 << 1));
              st[r] = map_comp(m, st[r]);
            } else {
              if (!pad) {   // (padding passes the state on and is no site of the path)
                const uint32_t z = st[r] ? z1 : z0;
                st[r] = z;
                acc[r].site(!started && (h == 1 || !real1), z, brk[u], dn[u]);
                word[r] |= (uint64_t)z << (8 * u);
              }
            }
          }
        }
      }
      if constexpr (PASS == 1) started = started || s_lo < S;
    }
    if constexpr (PASS == 1) {
#pragma unroll
      for (int r = 0; r < RB; ++r)
        if ((uint32_t)r < A.n_paths)
          *reinterpret_cast<uint64_t*>(A.paths + ((uint64_t)r * I + i) * A.pitch + s_base + b * CK) = word[r];
    }
    if (b == 0) break;
    dright = dcur[0];
    cright = cc[0];
#pragma unroll
    for (int u = 0; u < CK; ++u) {
      ecur[u] = enxt[u];
      dcur[u] = dnxt[u];
    }
    r0c = r0n;
    r1c = r1n;
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if ((uint32_t)r < nd) {
      const uint64_t o = ((uint64_t)r * I + i) * J + j;
      if constexpr (PASS == 0) {
        A.maps[o] = (uint8_t)st[r];
      } else {
        ChunkSeg cs;
        cs.ones = acc[r].ones;
        cs.head = acc[r].cur;
        cs.tail = acc[r].tail_final();
        cs.inner_n = acc[r].inner_n;
        cs.inner_longest = acc[r].longest;
        cs.full = acc[r].at_end ? 1u : 0u;
        cs.mb = acc[r].mb;
        A.chunk[o] = cs;
      }
    }
  }
}

// one wave per (draw, individual): maps[j] (the lane-chunk's map) -> the state entering
// lane-chunk j from the right; state_out = the state of the handle's first site
__global__ void __launch_bounds__(64)
k_sample_scan(uint8_t* __restrict__ maps, uint64_t J, uint32_t C, const uint8_t* __restrict__ state_in,
              uint8_t* __restrict__ state_out) {
  const uint64_t w = blockIdx.x;   // draw * I + individual
  const int lane = threadIdx.x;
  uint8_t* m = maps + w * J + (uint64_t)lane * C;
  uint32_t M = MAP_ID;
  for (uint32_t k = C; k-- > 0;) M = map_comp(m[k], M);
  uint32_t Sx = M;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_down(Sx, off);
    if (lane + off < 64) Sx = map_comp(Sx, o);
  }
  uint32_t X = __shfl_down(Sx, 1);
  if (lane == 63) X = MAP_ID;
  const uint32_t zin = state_in ? (state_in[w] & 1u) : 0u;
  uint32_t cur = (X >> zin) & 1u;
  for (uint32_t k = C; k-- > 0;) {
    const uint32_t mk = m[k];
    m[k] = (uint8_t)cur;
    cur = (mk >> cur) & 1u;
  }
  if (lane == 0) state_out[w] = (uint8_t)cur;
}

// one lane per (draw, individual): its lane-chunks' statistics merged in site order
__global__ void __launch_bounds__(64)
k_sample_fold(const ChunkSeg* __restrict__ chunk, const double* __restrict__ pos_il, uint64_t J,
              uint64_t T, uint64_t S, uint64_t n, SampleSeg* __restrict__ seg) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  SampleSeg acc{0, 0, 0, 0, 0, 0, 0.0, 0};
  for (uint64_t j = 0; j < J; ++j) {
    const uint64_t lo = j * T;
    if (lo >= S) break;
    const ChunkSeg cs = chunk[w * J + j];
    const SampleSeg B{S - lo < T ? S - lo : T, cs.ones, cs.head, cs.tail, cs.inner_n, cs.inner_longest,
                      cs.mb, cs.full};
    if (j == 0) {
      acc = B;
    } else {
      const double d = pos_il[((j >> 6) * T) * 64 + (j & 63)];
      acc = seg_merge(acc, B, !(d < kDStart), d);
    }
  }
  seg[w] = acc;
}

// exact mode: fw [S + 1][I][2] log-space forward values (fw[s + 1] = site s)
__global__ void __launch_bounds__(64)
k_sample_exact(const double* __restrict__ fw, const double* __restrict__ pos, uint64_t S, uint64_t I,
               const double* __restrict__ indF, const double* __restrict__ alpha, uint64_t seed,
               uint32_t draw0, uint32_t nd, uint32_t n_paths, uint64_t pitch,
               uint8_t* __restrict__ paths, SampleSeg* __restrict__ seg) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= (uint64_t)nd * I) return;
  const uint32_t r = (uint32_t)(w / I);
  const uint64_t i = w % I;
  const double f = indF[i], al = alpha[i];
  const double q0 = 1 - f, q1 = f;
  DrawAcc acc;
  uint32_t z = 0;
  ngh_philox4 words{};
  for (uint64_t s = S; s-- > 0;) {
    const double l0 = fw[((s + 1) * I + i) * 2], l1 = fw[((s + 1) * I + i) * 2 + 1];
    // a(1) / a(0), or its inverse, whichever is at most 1
    const bool up = l1 > l0;
    const double ratio = det_exp(up ? l0 - l1 : l1 - l0);
    const double a0 = up ? ratio : 1.0, a1 = up ? 1.0 : ratio;
    const double d = s + 1 < S ? pos[s + 1] : kDStart;
    const bool brk = !(d < kDStart);
    const double cn = brk ? 0.0 : det_exp(-al * d);
    const Thr th = site_thr(a0, a1, q0, q1, cn, brk);
    if (s + 1 == S || (s & 1)) words = ngh_sample_words(seed, draw0 + r, (uint32_t)i, s >> 1);
    const double u = ngh_sample_uniform(words, s);
    z = z ? (u * th.s1 < th.t1 ? 1u : 0u) : (u * th.s0 < th.t0 ? 1u : 0u);
    acc.site(s + 1 == S, z, brk, d);
    if (r < n_paths) paths[w * pitch + s] = (uint8_t)z;
  }
  seg[w] = SampleSeg{S, acc.ones, acc.cur, acc.tail_final(), acc.inner_n, acc.longest, acc.mb,
                     acc.at_end ? 1ull : 0ull};
}

uint64_t align256(uint64_t n) { return (n + 255) & ~255ull; }

}  // namespace

uint64_t sample_scratch_bytes(uint64_t I, uint64_t J, uint64_t pitch, uint32_t n_paths) {
  const uint64_t n = (uint64_t)kSampleBatch * I, jj = J ? J : 1;
  return align256(n * jj) + align256(n * jj * sizeof(ChunkSeg)) + align256(n * sizeof(SampleSeg)) +
         2 * align256(n) + align256((uint64_t)n_paths * I * pitch + 8);
}

SampleScratch sample_scratch_carve(uint8_t* base, uint64_t I, uint64_t J, uint64_t pitch) {
  const uint64_t n = (uint64_t)kSampleBatch * I;
  SampleScratch s;
  s.maps = base;
  base += align256(n * (J ? J : 1));
  s.chunk = base;
  base += align256(n * (J ? J : 1) * sizeof(ChunkSeg));
  s.seg = reinterpret_cast<SampleSeg*>(base);
  base += align256(n * sizeof(SampleSeg));
  s.state_in = base;
  base += align256(n);
  s.state_out = base;
  base += align256(n);
  s.paths = base;
  s.pitch = pitch;
  return s;
}

bool sample_fast_forward(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                         const double* d_vin, double* d_vout) {
  if (!fast_forward_ops(fs, st, d_indF, d_alpha)) return false;
  hipLaunchKernelGGL(k_sample_bounds, dim3((unsigned)fs.I), dim3(64), 0, st, fs.lane_ops, fs.J, fs.C,
                     d_indF, d_vin, fs.bound, d_vout);
  return hipGetLastError() == hipSuccess;
}

bool sample_fast_backward(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                          uint64_t seed, uint32_t draw0, uint32_t nd, uint64_t site0, bool last,
                          double d_after, uint32_t n_paths, const SampleScratch& scr) {
  if (nd == 0 || nd > kSampleBatch || n_paths > nd) return false;
  WalkArgs A;
  A.e_il = fs.e_il;
  A.pos_il = fs.pos_il;
  A.T = fs.T;
  A.S = fs.S;
  A.I = fs.I;
  A.pitch = scr.pitch;
  A.C = fs.C;
  A.indF = d_indF;
  A.alpha = d_alpha;
  A.bound = fs.bound;
  A.ckpt = reinterpret_cast<const double2*>(fs.ckpt);
  A.seed = seed;
  A.site0 = site0;
  A.draw0 = draw0;
  A.nd = nd;
  A.n_paths = n_paths;
  A.last = last ? 1 : 0;
  A.d_after = d_after;
  A.maps = scr.maps;
  A.chunk = static_cast<ChunkSeg*>(scr.chunk);
  A.paths = scr.paths;
  const dim3 grid((unsigned)(fs.I * fs.C)), block(64);
  hipLaunchKernelGGL(k_sample_walk<0>, grid, block, 0, st, A);
  hipLaunchKernelGGL(k_sample_scan, dim3((unsigned)(nd * fs.I)), block, 0, st, scr.maps, fs.J, fs.C,
                     last ? nullptr : scr.state_in, scr.state_out);
  hipLaunchKernelGGL(k_sample_walk<1>, grid, block, 0, st, A);
  const uint64_t n = (uint64_t)nd * fs.I;
  hipLaunchKernelGGL(k_sample_fold, dim3((unsigned)((n + 63) / 64)), block, 0, st,
                     static_cast<const ChunkSeg*>(scr.chunk), fs.pos_il, fs.J, fs.T, fs.S, n, scr.seg);
  return hipGetLastError() == hipSuccess;
}

void launch_sample_exact(hipStream_t st, const double* fw, const double* pos, uint64_t S, uint64_t I,
                         const double* d_indF, const double* d_alpha, uint64_t seed, uint32_t draw0,
                         uint32_t nd, uint32_t n_paths, const SampleScratch& scr) {
  const uint64_t n = (uint64_t)nd * I;
  hipLaunchKernelGGL(k_sample_exact, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, fw, pos, S, I,
                     d_indF, d_alpha, seed, draw0, nd, n_paths, scr.pitch, scr.paths, scr.seg);
}

}  // namespace nghmm
