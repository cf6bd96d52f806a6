// kernels_sharing.hip -- pairwise IBD sharing: for every pair of individuals (i, j) the number of
// sites at which both are IBD (by the decoded path, by a posterior threshold) and the expected
// number, sum over sites of marg[s][i] * marg[s][j].  All three are X^T X of an array that lies
// site-major, so a row piece of 16 individuals is one coalesced read and is the A and the B
// operand of the matrix instruction as it stands, without a transpose:
//   posteriors  [S][I] doubles          v_mfma_f64_16x16x4_f64: lane l carries marg[s + (l >> 4)][c + (l & 15)]
//   0/1 bytes   [S/16][I][16] (the path v_mfma_i32_16x16x64_i8: lane l carries the 16 bytes of
//               as the decode leaves it)  individual c + (l & 15) in block b + (l >> 4)
// (the int8 instruction's own order of the 64 k inside a step does not matter here: both operands
// are read the same way, so whatever k a byte gets, its partner at the same site gets it too).
//
// One wave per (block of 64 x 64 pairs with column block >= row block, K-split): 16 tiles of
// 16 x 16 in registers, operands straight from global memory (each row piece is used by four
// MFMAs, the next step's are requested before this step's MFMAs), no LDS.  A split's partial
// tile goes to scratch; the finish kernels add the splits in site order and mirror the upper
// triangle.  No atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_sharing.hpp"

namespace nghmm {

namespace {

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef int i4_t __attribute__((ext_vector_type(4)));

// blockIdx.x -> the block pair (rb, cb), cb >= rb, of nb blocks a side (row by row)
__device__ inline void block_pair(uint32_t t, uint32_t nb, uint32_t* rb, uint32_t* cb) {
  uint32_t r = 0;
  while (t >= nb - r) {
    t -= nb - r;
    ++r;
  }
  *rb = r;
  *cb = r + t;
}

__global__ void __launch_bounds__(64)
k_sharing_prod(const double* __restrict__ marg, uint64_t I, uint64_t begin, uint64_t end,
               uint64_t first, uint64_t len, double* __restrict__ part) {
  const uint32_t nb = (uint32_t)((I + 63) / 64);
  uint32_t rb, cb;
  block_pair(blockIdx.x, nb, &rb, &cb);
  const uint64_t split = blockIdx.y;
  const uint64_t e0 = first + split * len, e1 = e0 + len;
  const uint64_t lo = e0 > begin ? e0 : begin, hi = e1 < end ? e1 : end;
  const uint32_t lane = threadIdx.x, m = lane & 15, k = lane >> 4;
  const bool diag = rb == cb;
  // a row of marg is exactly I doubles: a column past I would read the next site
  uint64_t ca[4], cc[4];
  bool oa[4], oc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    ca[t] = (uint64_t)rb * 64 + t * 16 + m;
    cc[t] = (uint64_t)cb * 64 + t * 16 + m;
    oa[t] = ca[t] < I;
    oc[t] = cc[t] < I;
  }
  d4_t acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = d4_t{0.0, 0.0, 0.0, 0.0};
  double a[4], b[4], na[4], nb_[4];
  {
    const uint64_t s = lo + k;
    const bool ok = s < hi;
    const double* row = marg + s * I;
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = ok && oa[t] ? row[ca[t]] : 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) b[t] = diag ? a[t] : (ok && oc[t] ? row[cc[t]] : 0.0);
  }
  for (uint64_t s0 = lo; s0 < hi; s0 += 4) {
    {   // the next four sites (past the split's end: zeros, never loaded)
      const uint64_t s = s0 + 4 + k;
      const bool ok = s < hi;
      const double* row = marg + s * I;
#pragma unroll
      for (int t = 0; t < 4; ++t) na[t] = ok && oa[t] ? row[ca[t]] : 0.0;
#pragma unroll
      for (int t = 0; t < 4; ++t) nb_[t] = diag ? na[t] : (ok && oc[t] ? row[cc[t]] : 0.0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], b[c], acc[r][c], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a[t] = na[t];
      b[t] = nb_[t];
    }
  }
  // the f64 C/D map: column = lane & 15, row = (lane >> 4) + 4 * register
  double* out = part + split * I * I;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint64_t j = (uint64_t)cb * 64 + c * 16 + m;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint64_t i = (uint64_t)rb * 64 + r * 16 + k + 4 * g;
        if (i < I && j < I) out[i * I + j] = acc[r][c][g];
      }
    }
}

// 0x01 in every byte v of word q of a block of 16 sites whose site, 4 q + v past the block's
// first, is in [u0, u1)
__device__ inline uint32_t mask_word(uint32_t q, uint32_t u0, uint32_t u1) {
  uint32_t x = 0;
#pragma unroll
  for (uint32_t v = 0; v < 4; ++v) x |= (4 * q + v >= u0 && 4 * q + v < u1 ? 1u : 0u) << (8 * v);
  return x;
}

// ... of the block that begins at site0, for the sites in [lo, hi)
__device__ inline uint4 site_mask(uint64_t site0, uint64_t lo, uint64_t hi) {
  const uint32_t u0 = lo > site0 ? (uint32_t)(lo - site0 < 16 ? lo - site0 : 16) : 0u;
  const uint32_t u1 = hi > site0 ? (uint32_t)(hi - site0 < 16 ? hi - site0 : 16) : 0u;
  return uint4{mask_word(0, u0, u1), mask_word(1, u0, u1), mask_word(2, u0, u1), mask_word(3, u0, u1)};
}

// the 16 bytes at p (ok) or zeros (not loaded), the sites outside the mask cleared
__device__ inline i4_t load_masked(const uint8_t* p, bool ok, uint4 mk) {
  uint32_t x = 0, y = 0, z = 0, w = 0;
  if (ok) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    x = v.x;
    y = v.y;
    z = v.z;
    w = v.w;
  }
  return i4_t{(int)(x & mk.x), (int)(y & mk.y), (int)(z & mk.z), (int)(w & mk.w)};
}

__global__ void __launch_bounds__(64)
k_sharing_count(const uint8_t* __restrict__ bytes16, uint64_t block0, uint64_t I, uint64_t begin,
                uint64_t end, uint64_t first, uint64_t len, int32_t* __restrict__ part) {
  const uint32_t nb = (uint32_t)((I + 63) / 64);
  uint32_t rb, cb;
  block_pair(blockIdx.x, nb, &rb, &cb);
  const uint64_t split = blockIdx.y;
  const uint64_t e0 = first + split * len, e1 = e0 + len;
  const uint64_t lo = e0 > begin ? e0 : begin, hi = e1 < end ? e1 : end;
  const uint32_t lane = threadIdx.x, m = lane & 15, k = lane >> 4;
  const bool diag = rb == cb;
  uint64_t ca[4], cc[4];
  bool oa[4], oc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    ca[t] = (uint64_t)rb * 64 + t * 16 + m;
    cc[t] = (uint64_t)cb * 64 + t * 16 + m;
    oa[t] = ca[t] < I;
    oc[t] = cc[t] < I;
  }
  i4_t acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = i4_t{0, 0, 0, 0};
  // steps of 64 sites = 4 blocks of 16, lane group k takes block k of the step; e0 is a
  // multiple of 64, so a step never lies across a split edge; a block with no site in [lo, hi)
  // (before begin, behind end, behind the handle's last block) is not loaded
  for (uint64_t g0 = e0; g0 < hi; g0 += 64) {
    const uint64_t site0 = g0 + 16 * k;
    const bool ok = site0 + 16 > lo && site0 < hi;
    const uint4 mk = site_mask(site0, lo, hi);
    const uint8_t* blk = bytes16 + (site0 / 16 - block0) * I * 16;
    i4_t a[4], b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      a[t] = load_masked(blk + ca[t] * 16, ok && oa[t], mk);
#pragma unroll
    for (int t = 0; t < 4; ++t)
      b[t] = diag ? a[t] : load_masked(blk + cc[t] * 16, ok && oc[t], mk);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        acc[r][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[r], b[c], acc[r][c], 0, 0, 0);
  }
  // the C/D map of every 16 x 16 shape but f64: column = lane & 15, row = 4 * (lane >> 4) + register
  int32_t* out = part + split * I * I;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint64_t j = (uint64_t)cb * 64 + c * 16 + m;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint64_t i = (uint64_t)rb * 64 + r * 16 + 4 * k + g;
        if (i < I && j < I) out[i * I + j] = acc[r][c][g];
      }
    }
}

// one thread per (block of 16 sites, individual): 16 coalesced reads along the individuals, one
// 16-byte store
__global__ void __launch_bounds__(256)
k_sharing_threshold(const double* __restrict__ marg, uint64_t I, uint64_t begin, uint64_t end,
                    double thr, uint8_t* __restrict__ out16) {
  const uint64_t b0 = begin / 16, nblk = (end + 15) / 16 - b0, n = nblk * I;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n;
       x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t b = b0 + x / I, i = x % I;
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const uint64_t s = b * 16 + u;
      const bool in = s >= begin && s < end;
      const double p = in ? marg[s * I + i] : 0.0;
      w[u >> 2] |= (in && p >= thr ? 1u : 0u) << (8 * (u & 3));
    }
    *reinterpret_cast<uint4*>(out16 + x * 16) = uint4{w[0], w[1], w[2], w[3]};
  }
}

template <typename T, typename U>
__global__ void __launch_bounds__(256)
k_sharing_finish(const T* __restrict__ part, uint64_t n_splits, uint64_t I, U* __restrict__ out) {
  const uint64_t n = I * I;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n;
       x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = x / I, j = x % I;
    const uint64_t at = i <= j ? i * I + j : j * I + i;
    U t = (U)part[at];
    for (uint64_t k = 1; k < n_splits; ++k) t += (U)part[k * n + at];
    out[x] = t;
  }
}

uint32_t grid_for(uint64_t n, uint64_t per_block) {
  const uint64_t g = (n + per_block - 1) / per_block;
  return (uint32_t)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

dim3 pair_grid(uint64_t I, const SharingPlan& plan) {
  const uint64_t nb = (I + 63) / 64;
  return dim3((uint32_t)(nb * (nb + 1) / 2), (uint32_t)plan.n);
}

}  // namespace

void launch_sharing_prod(hipStream_t st, const double* marg, uint64_t I, uint64_t begin,
                         uint64_t end, SharingPlan plan, double* part) {
  hipLaunchKernelGGL(k_sharing_prod, pair_grid(I, plan), dim3(64), 0, st, marg, I, begin, end,
                     plan.first, plan.len, part);
}

void launch_sharing_count(hipStream_t st, const uint8_t* bytes16, uint64_t block0, uint64_t I,
                          uint64_t begin, uint64_t end, SharingPlan plan, int32_t* part) {
  hipLaunchKernelGGL(k_sharing_count, pair_grid(I, plan), dim3(64), 0, st, bytes16, block0, I, begin,
                     end, plan.first, plan.len, part);
}

void launch_sharing_threshold(hipStream_t st, const double* marg, uint64_t I, uint64_t begin,
                              uint64_t end, double thr, uint8_t* out16) {
  const uint64_t n = ((end + 15) / 16 - begin / 16) * I;
  hipLaunchKernelGGL(k_sharing_threshold, dim3(grid_for(n, 256)), dim3(256), 0, st, marg, I, begin,
                     end, thr, out16);
}

void launch_sharing_finish_prod(hipStream_t st, const double* part, uint64_t n_splits, uint64_t I,
                                double* out) {
  hipLaunchKernelGGL((k_sharing_finish<double, double>), dim3(grid_for(I * I, 256)), dim3(256), 0, st,
                     part, n_splits, I, out);
}

void launch_sharing_finish_count(hipStream_t st, const int32_t* part, uint64_t n_splits,
                                 uint64_t I, uint64_t* out) {
  hipLaunchKernelGGL((k_sharing_finish<int32_t, uint64_t>), dim3(grid_for(I * I, 256)), dim3(256), 0,
                     st, part, n_splits, I, out);
}

}  // namespace nghmm
