// kernels_summary.hip -- IBD per region and per site: the share of a region that an individual
// has in state IBD (F_ROH per chromosome or window) and the number of individuals that are IBD at
// a site (ROH islands), from the decoded path and the posteriors where the run left them.
//
// One pass.  One lane per individual, one wave per (64 individuals x segment of kSummarySeg
// sites); a lane loads its 16 path bytes and its 16 posteriors of a block of 16 sites once, and
// every cell feeds both sides:
//   along the sites       lane-private accumulators of the region the (wave-uniform) site index
//                         is in, written out as one PIECE per (region, segment) when the site
//                         index reaches the piece's end;
//   along the individuals per site two ballots and population counts and one butterfly of
//                         shuffles over the wave's 64 lanes (xor 32, 16, 8, 4, 2, 1), lane u
//                         keeping site u's record, so that a block of 16 sites leaves as one
//                         store of 16 records.
// Finish kernels add an (individual, region)'s pieces in site order and a site's per-wave records
// in block order.  No atomics: every double is added in one order, the same bits on every call.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_summary.hpp"

namespace nghmm {

namespace {

template <int WHAT, bool SITES>
__global__ void __launch_bounds__(64)
k_summary_pass(const uint8_t* __restrict__ path16, const double* __restrict__ marg,
               const double* __restrict__ pos, const uint8_t* __restrict__ prev_state, double thr,
               uint64_t S, uint64_t I, const SummaryPiece* __restrict__ pieces,
               const uint32_t* __restrict__ seg_piece, RegionRec* __restrict__ piece_out,
               SiteRec* __restrict__ site_part) {
  constexpr bool VIT = (WHAT & SUMMARY_VITERBI) != 0, POST = (WHAT & SUMMARY_POSTERIOR) != 0;
  const uint64_t nib = (I + 63) / 64;
  const uint64_t seg = blockIdx.x / nib, ib = blockIdx.x % nib;
  const uint32_t lane = threadIdx.x;
  const uint64_t i = ib * 64 + lane;
  // (no early return: the lanes past the last individual take part in the ballots and shuffles,
  // with state 0 and posterior 0, and load and store nothing)
  const bool live = i < I;
  const uint64_t s0 = seg * kSummarySeg;
  const uint64_t b0 = s0 / 16, b1 = min((S + 15) / 16, (s0 + kSummarySeg) / 16);
  uint32_t prev = 0;   // the state at the site before
  if (VIT && live) {
    if (s0 > 0) prev = path16[((b0 - 1) * I + i) * 16 + 15] != 0 ? 1u : 0u;
    else if (prev_state) prev = prev_state[i] != 0 ? 1u : 0u;
  }
  // the piece the site index is in or comes to next (wave-uniform)
  uint32_t k = seg_piece[seg];
  const uint32_t kend = seg_piece[seg + 1];
  uint64_t lo = ~0ull, hi = ~0ull;
  bool first = false, inreg = false;
  if (k < kend) {
    lo = pieces[k].lo;
    hi = pieces[k].hi;
    first = pieces[k].first != 0;
  }
  uint64_t a_vit = 0, a_post = 0;
  double a_sum = 0.0, a_mb = 0.0;
  for (uint64_t b = b0; b < b1; ++b) {
    const uint32_t nvalid = (uint32_t)(S - b * 16 < 16 ? S - b * 16 : 16);
    uint32_t bits = 0;
    double p[16];
    if (VIT && live) {
      const uint4 v = *reinterpret_cast<const uint4*>(path16 + (b * I + i) * 16);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int u = 0; u < 16; ++u) bits |= (((w[u >> 2] >> (8 * (u & 3))) & 0xffu) != 0 ? 1u : 0u) << u;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u)
      p[u] = POST && live && (uint32_t)u < nvalid ? marg[(b * 16 + u) * I + i] : 0.0;
    SiteRec mine = {0, 0, 0.0};   // lane u: the record of site 16 b + u
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if ((uint32_t)u < nvalid) {
        const uint64_t s = b * 16 + u;
        const uint32_t c = VIT ? (bits >> u) & 1u : 0u;
        const double pv = p[u];
        const bool q = POST && pv >= thr;
        if (SITES) {
          const uint32_t nv = VIT ? (uint32_t)__popcll(__ballot(c != 0)) : 0u;
          const uint32_t np = POST ? (uint32_t)__popcll(__ballot(q)) : 0u;
          double t = pv;
          if (POST) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
          }
          if (lane == (uint32_t)u) {
            mine.vit_count = nv;
            mine.post_count = np;
            mine.post_sum = t;
          }
        }
        if (s == lo) {
          inreg = true;
          a_vit = a_post = 0;
          a_sum = a_mb = 0.0;
        }
        if (inreg) {
          if (VIT) {
            a_vit += c;
            const double d = pos[s];
            if ((c & prev) != 0 && !(first && s == lo) && __builtin_isfinite(d)) a_mb += d;
          }
          if (POST) {
            a_post += q ? 1u : 0u;
            a_sum += pv;
          }
        }
        if (VIT) prev = c;
        if (s + 1 == hi) {
          if (live) {
            RegionRec r;
            r.vit_sites = a_vit;
            r.post_sites = a_post;
            r.post_sum = a_sum;
            r.vit_mb = a_mb;
            piece_out[(uint64_t)k * I + i] = r;
          }
          inreg = false;
          ++k;
          lo = hi = ~0ull;
          if (k < kend) {
            lo = pieces[k].lo;
            hi = pieces[k].hi;
            first = pieces[k].first != 0;
          }
        }
      }
    }
    if (SITES && lane < nvalid) site_part[ib * S + b * 16 + lane] = mine;
  }
}

__global__ void __launch_bounds__(256)
k_summary_finish_regions(const RegionRec* __restrict__ piece_out,
                         const uint32_t* __restrict__ piece_first, uint64_t n_regions, uint64_t I,
                         RegionRec* __restrict__ out) {
  const uint64_t n = n_regions * I;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n;
       x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = x / I, i = x % I;
    const uint32_t ka = piece_first[r], kb = piece_first[r + 1];
    RegionRec t = piece_out[(uint64_t)ka * I + i];
    for (uint32_t k = ka + 1; k < kb; ++k) {
      const RegionRec a = piece_out[(uint64_t)k * I + i];
      t.vit_sites += a.vit_sites;
      t.post_sites += a.post_sites;
      t.post_sum += a.post_sum;
      t.vit_mb += a.vit_mb;
    }
    out[i * n_regions + r] = t;
  }
}

__global__ void __launch_bounds__(256)
k_summary_finish_sites(const SiteRec* __restrict__ site_part, uint64_t n_blocks, uint64_t S,
                       SiteRec* __restrict__ out) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S;
       s += (uint64_t)gridDim.x * blockDim.x) {
    SiteRec t = site_part[s];
    for (uint64_t ib = 1; ib < n_blocks; ++ib) {
      const SiteRec a = site_part[ib * S + s];
      t.vit_count += a.vit_count;
      t.post_count += a.post_count;
      t.post_sum += a.post_sum;
    }
    out[s] = t;
  }
}

__global__ void __launch_bounds__(256)
k_summary_last_state(const uint8_t* __restrict__ path16, uint64_t S, uint64_t I,
                     uint8_t* __restrict__ out) {
  const uint64_t s = S - 1;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < I;
       i += (uint64_t)gridDim.x * blockDim.x)
    out[i] = path16[((s / 16) * I + i) * 16 + (s & 15)] != 0 ? 1 : 0;
}

uint32_t grid_for(uint64_t n, uint64_t per_block) {
  const uint64_t g = (n + per_block - 1) / per_block;
  return (uint32_t)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

template <int WHAT>
void launch_pass(hipStream_t st, dim3 grid, const uint8_t* path16, const double* marg,
                 const double* pos, const uint8_t* prev_state, double thr, uint64_t S, uint64_t I,
                 const SummaryPiece* pieces, const uint32_t* seg_piece, RegionRec* piece_out,
                 SiteRec* site_part) {
  if (site_part)
    hipLaunchKernelGGL((k_summary_pass<WHAT, true>), grid, dim3(64), 0, st, path16, marg, pos,
                       prev_state, thr, S, I, pieces, seg_piece, piece_out, site_part);
  else
    hipLaunchKernelGGL((k_summary_pass<WHAT, false>), grid, dim3(64), 0, st, path16, marg, pos,
                       prev_state, thr, S, I, pieces, seg_piece, piece_out, site_part);
}

}  // namespace

void launch_summary_pass(hipStream_t st, int what, const uint8_t* path16, const double* marg,
                         const double* pos, const uint8_t* prev_state, double thr, uint64_t S,
                         uint64_t I, const SummaryPiece* pieces, const uint32_t* seg_piece,
                         RegionRec* piece_out, SiteRec* site_part) {
  const dim3 grid((uint32_t)(summary_segments(S) * ((I + 63) / 64)));
  if (what == SUMMARY_VITERBI)
    launch_pass<SUMMARY_VITERBI>(st, grid, path16, marg, pos, prev_state, thr, S, I, pieces,
                                 seg_piece, piece_out, site_part);
  else if (what == SUMMARY_POSTERIOR)
    launch_pass<SUMMARY_POSTERIOR>(st, grid, path16, marg, pos, prev_state, thr, S, I, pieces,
                                   seg_piece, piece_out, site_part);
  else
    launch_pass<SUMMARY_VITERBI | SUMMARY_POSTERIOR>(st, grid, path16, marg, pos, prev_state, thr,
                                                     S, I, pieces, seg_piece, piece_out, site_part);
}

void launch_summary_finish_regions(hipStream_t st, const RegionRec* piece_out,
                                   const uint32_t* piece_first, uint64_t n_regions, uint64_t I,
                                   RegionRec* out) {
  hipLaunchKernelGGL(k_summary_finish_regions, dim3(grid_for(n_regions * I, 256)), dim3(256), 0, st,
                     piece_out, piece_first, n_regions, I, out);
}

void launch_summary_finish_sites(hipStream_t st, const SiteRec* site_part, uint64_t n_blocks,
                                 uint64_t S, SiteRec* out) {
  hipLaunchKernelGGL(k_summary_finish_sites, dim3(grid_for(S, 256)), dim3(256), 0, st, site_part,
                     n_blocks, S, out);
}

void launch_summary_last_state(hipStream_t st, const uint8_t* path16, uint64_t S, uint64_t I,
                               uint8_t* out) {
  hipLaunchKernelGGL(k_summary_last_state, dim3(grid_for(I, 256)), dim3(256), 0, st, path16, S, I,
                     out);
}

}  // namespace nghmm
