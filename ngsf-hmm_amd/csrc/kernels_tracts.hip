// kernels_tracts.hip -- IBD tracts (maximal runs of the IBD state within one chromosome) called on
// the device from the decoded path or from thresholded posteriors: what scripts/convert_ibd.pl
// does on the .ibd file (convert_ibd.pl:99-130), without the file.
//
// One lane per individual, one wave per (64 individuals x segment of kTractSeg sites).  Count
// pass: tract starts per (individual, segment); exclusive scan in (individual, segment) order =
// the index of each individual's tracts in (ind, first_site) order.  Emit pass: every lane
// writes the first site of the tracts that start in its segment and the last site of those
// that end there, and one partial posterior sum per tract piece.  Finish pass: a tract adds its
// pieces in segment order (no atomics: the sums are the same bits on every call).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace nghmm {

namespace {

constexpr uint32_t kScanTile = 2048;   // elements per block of the scan (256 threads x 8)

// bit u of mask[b]: site 16 b + u starts a chromosome (distance +inf) or is site 0
__global__ void __launch_bounds__(256)
k_tract_chrom_mask(const double* __restrict__ pos, uint64_t S, uint32_t* __restrict__ mask) {
  const uint64_t nblk = (S + 15) / 16;
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nblk;
       b += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t m = 0;
    for (int u = 0; u < 16; ++u) {
      const uint64_t s = b * 16 + u;
      if (s < S && (s == 0 || __builtin_isinf(pos[s]))) m |= 1u << u;
    }
    mask[b] = m;
  }
}

// In-state bits of one lane's 16-site block b (bits of sites >= S are 0).  VITERBI: the path
// bytes of the blocked layout [S/16][I][16] (one 16-byte load); POSTERIOR: marg[s][i] >= thr,
// the values kept in p[] for the posterior sums.
template <int SRC>
__device__ __forceinline__ uint32_t in_bits(const uint8_t* __restrict__ path16,
                                            const double* __restrict__ marg, double thr,
                                            uint64_t S, uint64_t I, uint64_t i, uint64_t b,
                                            double* p) {
  const uint32_t nvalid = (uint32_t)(S - b * 16 < 16 ? S - b * 16 : 16);
  uint32_t m = 0;
  if (SRC == TRACTS_SRC_VITERBI) {
    const uint4 v = *reinterpret_cast<const uint4*>(path16 + (b * I + i) * 16);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int u = 0; u < 16; ++u) m |= (((w[u >> 2] >> (8 * (u & 3))) & 0xffu) != 0 ? 1u : 0u) << u;
  } else {
#pragma unroll
    for (int u = 0; u < 16; ++u) p[u] = (uint32_t)u < nvalid ? marg[(b * 16 + u) * I + i] : 0.0;
#pragma unroll
    for (int u = 0; u < 16; ++u) m |= (p[u] >= thr ? 1u : 0u) << u;
  }
  return nvalid == 16 ? m : m & ((1u << nvalid) - 1u);
}

template <int SRC>
__device__ __forceinline__ bool in_site(const uint8_t* __restrict__ path16,
                                        const double* __restrict__ marg, double thr, uint64_t I,
                                        uint64_t i, uint64_t s) {
  if (SRC == TRACTS_SRC_VITERBI) return path16[((s / 16) * I + i) * 16 + (s & 15)] != 0;
  return marg[s * I + i] >= thr;
}

// counts[i * nseg + seg] = tracts of individual i that start in segment seg
template <int SRC>
__global__ void __launch_bounds__(64)
k_tract_count(const uint8_t* __restrict__ path16, const double* __restrict__ marg, double thr,
              const uint32_t* __restrict__ cmask, uint64_t S, uint64_t I, uint64_t nseg,
              uint64_t* __restrict__ counts) {
  const uint64_t nib = (I + 63) / 64;
  const uint64_t seg = blockIdx.x / nib;
  const uint64_t i = (blockIdx.x % nib) * 64 + threadIdx.x;
  if (i >= I) return;
  const uint64_t s0 = seg * kTractSeg;
  const uint64_t b0 = s0 / 16, b1 = min((S + 15) / 16, (s0 + kTractSeg) / 16);
  uint32_t carry = s0 > 0 && in_site<SRC>(path16, marg, thr, I, i, s0 - 1) ? 1u : 0u;
  uint64_t n = 0;
  double p[16];
  for (uint64_t b = b0; b < b1; ++b) {
    const uint32_t in = in_bits<SRC>(path16, marg, thr, S, I, i, b, p);
    const uint32_t prev = (in << 1) | carry;   // bit u: site u - 1 is in state
    n += __builtin_popcount(in & (~prev | cmask[b]));
    carry = in >> 15;
  }
  counts[i * nseg + seg] = n;
}

// Emit pass: rec[k].first_site for every tract k that starts in the lane's segment, its last
// site (kept in rec[k].n_sites until the finish pass) for every tract that ends there,
// rec[k].post_sum = the sum over the tract's sites in its first segment; carry[i * nseg + seg] =
// the sum over the sites in this segment of the tract that was open when the segment began (0
// if none).  off = the exclusive scan of the count pass.
template <int SRC>
__global__ void __launch_bounds__(64)
k_tract_emit(const uint8_t* __restrict__ path16, const double* __restrict__ marg, double thr,
             const uint32_t* __restrict__ cmask, uint64_t S, uint64_t I, uint64_t nseg,
             const uint64_t* __restrict__ off, TractRec* __restrict__ rec,
             double* __restrict__ carry) {
  const uint64_t nib = (I + 63) / 64;
  const uint64_t seg = blockIdx.x / nib;
  const uint64_t i = (blockIdx.x % nib) * 64 + threadIdx.x;
  if (i >= I) return;
  const uint64_t s0 = seg * kTractSeg;
  const uint64_t b0 = s0 / 16, b1 = min((S + 15) / 16, (s0 + kTractSeg) / 16);
  bool open = s0 > 0 && in_site<SRC>(path16, marg, thr, I, i, s0 - 1);
  const bool had_carry = open;
  bool carried = open;             // the open piece belongs to a tract of an earlier segment
  uint64_t k = off[i * nseg + seg] - (open ? 1 : 0);   // the open tract (if open)
  uint64_t next = off[i * nseg + seg];                 // the next tract to start
  double sum = 0.0;
  double p[16];
  for (uint64_t b = b0; b < b1; ++b) {
    const uint32_t in = in_bits<SRC>(path16, marg, thr, S, I, i, b, p);
    const uint32_t cs = cmask[b];
    if (SRC == TRACTS_SRC_VITERBI) {
      if (!open && in == 0) continue;   // nothing starts, nothing is open
      // the posteriors of the block's sites in state, 16 independent loads in flight
#pragma unroll
      for (int u = 0; u < 16; ++u) p[u] = (in >> u) & 1u ? marg[(b * 16 + u) * I + i] : 0.0;
      if (open && in == 0xffffu && cs == 0) {   // the open run goes through the whole block
#pragma unroll
        for (int u = 0; u < 16; ++u) sum += p[u];
        continue;
      }
    }
    for (int u = 0; u < 16; ++u) {
      const bool c = (in >> u) & 1u;
      const bool start = (cs >> u) & 1u;
      if (open && (!c || start)) {   // the open tract ended at the site before
        rec[k].n_sites = b * 16 + u - 1;
        if (carried) carry[i * nseg + seg] = sum;
        else rec[k].post_sum = sum;
        carried = false;
        open = false;
      }
      if (c && !open) {
        k = next++;
        rec[k].first_site = b * 16 + u;
        rec[k].ind = (uint32_t)i;
        rec[k].reserved = 0;
        sum = 0.0;
        open = true;
      }
      if (c) sum += p[u];
    }
  }
  if (open) {   // runs on into the next segment, or ends at the last site
    if (s0 + kTractSeg >= S) rec[k].n_sites = S - 1;
    if (carried) carry[i * nseg + seg] = sum;
    else rec[k].post_sum = sum;
  }
  if (!had_carry) carry[i * nseg + seg] = 0.0;
}

// Finish pass: n_sites from the last site, post_sum = the first piece plus every later
// segment's carried piece, in site order; keep[k] = (n_sites >= min_sites)
__global__ void __launch_bounds__(256)
k_tract_finish(TractRec* __restrict__ rec, uint64_t n, const double* __restrict__ carry,
               uint64_t nseg, uint64_t min_sites, uint64_t* __restrict__ keep) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
       k += (uint64_t)gridDim.x * blockDim.x) {
    TractRec r = rec[k];
    const uint64_t last = r.n_sites;
    double sum = r.post_sum;
    const double* c = carry + (uint64_t)r.ind * nseg;
    for (uint64_t seg = r.first_site / kTractSeg + 1; seg <= last / kTractSeg; ++seg) sum += c[seg];
    r.n_sites = last - r.first_site + 1;
    r.post_sum = sum;
    rec[k] = r;
    if (keep) keep[k] = r.n_sites >= min_sites ? 1 : 0;
  }
}

__global__ void __launch_bounds__(256)
k_tract_compact(const TractRec* __restrict__ rec, uint64_t n, uint64_t min_sites,
                const uint64_t* __restrict__ off, TractRec* __restrict__ out) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n;
       k += (uint64_t)gridDim.x * blockDim.x)
    if (rec[k].n_sites >= min_sites) out[off[k]] = rec[k];
}

// Exclusive scan of one tile of kScanTile elements in place; tsum[blockIdx] = the tile's total.
// One tile only: d[n] = the total.
__global__ void __launch_bounds__(256)
k_scan_tile(uint64_t* __restrict__ d, uint64_t n, uint64_t* __restrict__ tsum) {
  __shared__ uint64_t part[256];
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * 8;
  uint64_t v[8], t = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = base + j < n ? d[base + j] : 0;
    t += v[j];
  }
  part[threadIdx.x] = t;
  __syncthreads();
  for (int w = 1; w < 256; w <<= 1) {   // inclusive Hillis-Steele scan of the thread totals
    const uint64_t x = threadIdx.x >= (unsigned)w ? part[threadIdx.x - w] : 0;
    __syncthreads();
    part[threadIdx.x] += x;
    __syncthreads();
  }
  uint64_t run = part[threadIdx.x] - t;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (base + j < n) d[base + j] = run;
    run += v[j];
  }
  if (threadIdx.x == 255) {
    tsum[blockIdx.x] = part[255];
    if (gridDim.x == 1) d[n] = part[255];
  }
}

// adds the scanned tile totals (tsum[nt] = the grand total) to every tile; d[n] = the total
__global__ void __launch_bounds__(256)
k_scan_add(uint64_t* __restrict__ d, uint64_t n, const uint64_t* __restrict__ tsum, uint64_t nt) {
  const uint64_t add = tsum[blockIdx.x];
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (base + j < n) d[base + j] += add;
  if (blockIdx.x == 0 && threadIdx.x == 0) d[n] = tsum[nt];
}

uint64_t grid_for(uint64_t n, uint64_t per_block) {
  const uint64_t g = (n + per_block - 1) / per_block;
  return g < 1 ? 1 : (g > 65536 ? 65536 : g);
}

}  // namespace

uint64_t tract_scan_scratch(uint64_t n) {
  uint64_t total = 1;
  while (n > kScanTile) {
    n = (n + kScanTile - 1) / kScanTile;
    total += n + 1;
  }
  return total + 1;
}

void launch_tract_scan(hipStream_t st, uint64_t* d, uint64_t n, uint64_t* scratch) {
  if (n == 0) {
    (void)hipMemsetAsync(d, 0, sizeof(uint64_t), st);
    return;
  }
  const uint64_t nt = (n + kScanTile - 1) / kScanTile;
  hipLaunchKernelGGL(k_scan_tile, dim3((uint32_t)nt), dim3(256), 0, st, d, n, scratch);
  if (nt == 1) return;
  launch_tract_scan(st, scratch, nt, scratch + nt + 1);
  hipLaunchKernelGGL(k_scan_add, dim3((uint32_t)nt), dim3(256), 0, st, d, n, scratch, nt);
}

uint64_t tract_segments(uint64_t S) { return (S + kTractSeg - 1) / kTractSeg; }

void launch_tract_chrom_mask(hipStream_t st, const double* pos, uint64_t S, uint32_t* mask) {
  hipLaunchKernelGGL(k_tract_chrom_mask, dim3((uint32_t)grid_for((S + 15) / 16, 256)), dim3(256), 0,
                     st, pos, S, mask);
}

void launch_tract_count(hipStream_t st, int src, const uint8_t* path16, const double* marg,
                        double thr, const uint32_t* cmask, uint64_t S, uint64_t I,
                        uint64_t* counts) {
  const uint64_t nseg = tract_segments(S);
  const dim3 grid((uint32_t)(nseg * ((I + 63) / 64)));
  if (src == TRACTS_SRC_VITERBI)
    hipLaunchKernelGGL(k_tract_count<TRACTS_SRC_VITERBI>, grid, dim3(64), 0, st, path16, marg, thr,
                       cmask, S, I, nseg, counts);
  else
    hipLaunchKernelGGL(k_tract_count<TRACTS_SRC_POSTERIOR>, grid, dim3(64), 0, st, path16, marg,
                       thr, cmask, S, I, nseg, counts);
}

void launch_tract_emit(hipStream_t st, int src, const uint8_t* path16, const double* marg,
                       double thr, const uint32_t* cmask, uint64_t S, uint64_t I,
                       const uint64_t* off, TractRec* rec, double* carry) {
  const uint64_t nseg = tract_segments(S);
  const dim3 grid((uint32_t)(nseg * ((I + 63) / 64)));
  if (src == TRACTS_SRC_VITERBI)
    hipLaunchKernelGGL(k_tract_emit<TRACTS_SRC_VITERBI>, grid, dim3(64), 0, st, path16, marg, thr,
                       cmask, S, I, nseg, off, rec, carry);
  else
    hipLaunchKernelGGL(k_tract_emit<TRACTS_SRC_POSTERIOR>, grid, dim3(64), 0, st, path16, marg,
                       thr, cmask, S, I, nseg, off, rec, carry);
}

void launch_tract_finish(hipStream_t st, TractRec* rec, uint64_t n, const double* carry,
                         uint64_t S, uint64_t min_sites, uint64_t* keep) {
  hipLaunchKernelGGL(k_tract_finish, dim3((uint32_t)grid_for(n, 256)), dim3(256), 0, st, rec, n,
                     carry, tract_segments(S), min_sites, keep);
}

void launch_tract_compact(hipStream_t st, const TractRec* rec, uint64_t n, uint64_t min_sites,
                          const uint64_t* off, TractRec* out) {
  hipLaunchKernelGGL(k_tract_compact, dim3((uint32_t)grid_for(n, 256)), dim3(256), 0, st, rec, n,
                     min_sites, off, out);
}

}  // namespace nghmm
