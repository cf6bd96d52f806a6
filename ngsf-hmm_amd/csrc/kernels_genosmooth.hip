// kernels_genosmooth.hip -- genotype posteriors under the HMM (include/nghmm.h: nghmm_geno_smooth
// has the definition): per cell the joint posterior of genotype and IBD state given ALL data of
// the individual, from the cell's two cavity weights (1 - c, c) -- which the walks of
// kernels_freqinfo.hip leave --, its three likelihoods and the site's frequency:
//     J[z][g] = w_z h_z[g] p_g,  h_0 = ((1 - f)^2, 2 f (1 - f), f^2),  h_1 = (1 - f, 0, f),
// everything else a sum of the six products over their total B.
//
// One pass, of the shape of kernels_summary.hip's: one lane per individual, one wave per (64
// individuals x segment of kSummarySeg sites), weights and likelihoods both site-major (64
// adjacent cells per site).  Every cell feeds both sides:
//   along the individuals  per site a butterfly of the block's 64 values per field -- x_i +=
//                          x_{i ^ 32}, then ^ 16, 8, 4, 2, 1, a lane past the last individual
//                          adding 0 --, one record per (block, site); a finish kernel adds the
//                          blocks in order, the first one's value first (k_freq_sites' rule);
//   along the sites        lane-private sums of the piece the (wave-uniform) site index is in,
//                          from 0 in site order, written when the site index reaches the piece's
//                          end; a finish kernel adds a region's pieces in site order
//                          (nghmm_ibd_summary's rule for post_sum).
// No atomics, and ONE sequence of operations per cell whatever is asked for (the outputs differ
// only in what is stored): the same bits on every call.  The loads of kBatch sites are in flight
// together.
#include "fast_dev.hpp"
#include "kernels_genosmooth.hpp"

namespace nghmm {

namespace {

constexpr int kBatch = 4;   // sites whose loads are in flight together

struct CellArgs {
  const double2* __restrict__ cav;   // [S][I]
  GlView gl;
  const double* __restrict__ freq;   // [S]
  uint64_t S, I;
  const SummaryPiece* __restrict__ pieces;
  const uint32_t* __restrict__ seg_piece;
  double* __restrict__ post;         // [S][I][3] or null
  uint8_t* __restrict__ call;        // [S][I] or null
  GenoSiteRec* __restrict__ site_part;    // [nib][S] or null
  GenoRegionRec* __restrict__ piece_out;  // [n_pieces][I] or null
};

struct Cell {
  double P0, P1, P2, het_prior, ibd, non, alt, B;
};

// The six products and what is made of them.  Not contracted: every product is rounded before it
// is added, so a called genotype -- one p_g = 1, the others 0 -- has B equal to its one numerator
// and the posterior x / x = 1 exactly.
__device__ __forceinline__ Cell cell_posterior(double w0, double w1, double p0, double p1, double p2, double f) {
#pragma clang fp contract(off)
  const double om = 1 - f, hh = 2 * (om * f);
  const double j00 = (w0 * (om * om)) * p0, j01 = (w0 * hh) * p1, j02 = (w0 * (f * f)) * p2;
  const double j10 = (w1 * om) * p0, j12 = (w1 * f) * p2;
  const double n0 = j00 + j10, n2 = j02 + j12;
  Cell c;
  c.B = (n0 + j01) + n2;
  c.P0 = n0 / c.B;
  c.P1 = j01 / c.B;
  c.P2 = n2 / c.B;
  c.het_prior = w0 * hh;
  c.ibd = (j10 + j12) / c.B;
  c.non = ((j00 + j01) + j02) / c.B;
  c.alt = j12 / c.B;
  return c;
}

template <bool LOGGL>
__global__ void __launch_bounds__(64)
k_geno_cells(const CellArgs A) {
  const uint64_t S = A.S, I = A.I;
  const uint64_t nib = (I + 63) / 64;
  const uint64_t seg = blockIdx.x / nib, ib = blockIdx.x % nib;
  const uint32_t lane = threadIdx.x;
  const uint64_t i = ib * 64 + lane;
  // (no early return: the lanes past the last individual take part in the butterflies, with 0,
  // and load and store nothing)
  const bool live = i < I;
  const uint64_t s0 = seg * kSummarySeg;
  const uint64_t s1 = S - s0 < kSummarySeg ? S : s0 + kSummarySeg;
  // the piece the site index is in or comes to next (wave-uniform)
  uint32_t k = 0, kend = 0;
  uint64_t lo = ~0ull, hi = ~0ull;
  if (A.piece_out) {
    k = A.seg_piece[seg];
    kend = A.seg_piece[seg + 1];
    if (k < kend) {
      lo = A.pieces[k].lo;
      hi = A.pieces[k].hi;
    }
  }
  bool inreg = false;
  double a_het = 0.0, a_hp = 0.0, a_non = 0.0, a_dos = 0.0;
  for (uint64_t sb = s0; sb < s1; sb += kBatch) {
    double2 w[kBatch];
    double p0[kBatch], p1[kBatch], p2[kBatch], fr[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const uint64_t s = sb + u;
      w[u] = double2{0.0, 0.0};
      p0[u] = p1[u] = p2[u] = fr[u] = 0.0;
      if (s < s1) {
        fr[u] = A.freq[s];
        if (live) {
          w[u] = A.cav[s * I + i];
          gl_fetch(A.gl, s * I + i, p0[u], p1[u], p2[u]);
          if (LOGGL) {
            p0[u] = exp(p0[u]);
            p1[u] = exp(p1[u]);
            p2[u] = exp(p2[u]);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const uint64_t s = sb + u;
      if (s < s1) {   // (wave-uniform)
        const Cell c = cell_posterior(w[u].x, w[u].y, p0[u], p1[u], p2[u], fr[u]);
        if (live) {
          if (A.post) {
            double* o = A.post + (s * I + i) * 3;
            o[0] = c.P0;
            o[1] = c.P1;
            o[2] = c.P2;
          }
          if (A.call) {
            // the largest, ties to the lowest genotype; 3: no posterior
            uint32_t g = 0;
            double m = c.P0;
            if (c.P1 > m) {
              g = 1;
              m = c.P1;
            }
            if (c.P2 > m) g = 2;
            if (!(c.B > 0.0) || c.P0 != c.P0 || c.P1 != c.P1 || c.P2 != c.P2) g = 3;
            A.call[s * I + i] = (uint8_t)g;
          }
        }
        if (A.site_part) {
          const double t0 = wave_sum(live ? c.P0 : 0.0), t1 = wave_sum(live ? c.P1 : 0.0);
          const double t2 = wave_sum(live ? c.P2 : 0.0), t3 = wave_sum(live ? c.het_prior : 0.0);
          const double t4 = wave_sum(live ? c.ibd : 0.0), t5 = wave_sum(live ? c.alt : 0.0);
          // every lane holds the six sums: lane q stores field q of the record
          const double v = lane == 0 ? t0 : lane == 1 ? t1 : lane == 2 ? t2 : lane == 3 ? t3 : lane == 4 ? t4 : t5;
          if (lane < 6) reinterpret_cast<double*>(A.site_part + (ib * S + s))[lane] = v;
        }
        if (s == lo) {
          inreg = true;
          a_het = a_hp = a_non = a_dos = 0.0;
        }
        if (inreg) {
          a_het += c.P1;
          a_hp += c.het_prior;
          a_non += c.non;
          a_dos += c.P1 + 2 * c.P2;
        }
        if (s + 1 == hi) {
          if (live) A.piece_out[(uint64_t)k * I + i] = GenoRegionRec{a_het, a_hp, a_non, a_dos};
          inreg = false;
          ++k;
          lo = hi = ~0ull;
          if (k < kend) {
            lo = A.pieces[k].lo;
            hi = A.pieces[k].hi;
          }
        }
      }
    }
  }
}

__global__ void __launch_bounds__(256)
k_geno_finish_regions(const GenoRegionRec* __restrict__ piece_out, const uint32_t* __restrict__ piece_first,
                      uint64_t n_regions, uint64_t I, GenoRegionRec* __restrict__ out) {
  const uint64_t n = n_regions * I;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n;
       x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = x / I, i = x % I;
    const uint32_t ka = piece_first[r], kb = piece_first[r + 1];
    GenoRegionRec t = piece_out[(uint64_t)ka * I + i];
    for (uint32_t k = ka + 1; k < kb; ++k) {
      const GenoRegionRec a = piece_out[(uint64_t)k * I + i];
      t.het += a.het;
      t.het_prior += a.het_prior;
      t.non_ibd += a.non_ibd;
      t.dosage += a.dosage;
    }
    out[i * n_regions + r] = t;
  }
}

__global__ void __launch_bounds__(256)
k_geno_finish_sites(const GenoSiteRec* __restrict__ site_part, uint64_t n_blocks, uint64_t S,
                    GenoSiteRec* __restrict__ out) {
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S;
       s += (uint64_t)gridDim.x * blockDim.x) {
    GenoSiteRec t = site_part[s];
    for (uint64_t ib = 1; ib < n_blocks; ++ib) {
      const GenoSiteRec a = site_part[ib * S + s];
      t.n0 += a.n0;
      t.n1 += a.n1;
      t.n2 += a.n2;
      t.het_prior += a.het_prior;
      t.ibd += a.ibd;
      t.alt_ibd += a.alt_ibd;
    }
    out[s] = t;
  }
}

uint32_t grid_for(uint64_t n, uint64_t per_block) {
  const uint64_t g = (n + per_block - 1) / per_block;
  return (uint32_t)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

}  // namespace

bool genosmooth_cells(hipStream_t st, const double* d_cav, const GlView& gl, bool log_gl,
                      const double* d_freq, uint64_t S, uint64_t I, const SummaryPiece* d_pieces,
                      const uint32_t* d_seg_piece, double* d_post, uint8_t* d_call,
                      GenoSiteRec* d_site_part, GenoRegionRec* d_piece_out) {
  const uint64_t grid = summary_segments(S) * ((I + 63) / 64);
  if (grid == 0 || grid > 0x7fffffffull) return false;
  CellArgs A;
  A.cav = reinterpret_cast<const double2*>(d_cav);
  A.gl = gl;
  A.freq = d_freq;
  A.S = S;
  A.I = I;
  A.pieces = d_pieces;
  A.seg_piece = d_seg_piece;
  A.post = d_post;
  A.call = d_call;
  A.site_part = d_site_part;
  A.piece_out = d_piece_out;
  if (log_gl) hipLaunchKernelGGL((k_geno_cells<true>), dim3((unsigned)grid), dim3(64), 0, st, A);
  else hipLaunchKernelGGL((k_geno_cells<false>), dim3((unsigned)grid), dim3(64), 0, st, A);
  return hipGetLastError() == hipSuccess;
}

bool genosmooth_finish_regions(hipStream_t st, const GenoRegionRec* d_piece_out,
                               const uint32_t* d_piece_first, uint64_t n_regions, uint64_t I,
                               GenoRegionRec* d_out) {
  hipLaunchKernelGGL(k_geno_finish_regions, dim3(grid_for(n_regions * I, 256)), dim3(256), 0, st,
                     d_piece_out, d_piece_first, n_regions, I, d_out);
  return hipGetLastError() == hipSuccess;
}

bool genosmooth_finish_sites(hipStream_t st, const GenoSiteRec* d_site_part, uint64_t n_blocks,
                             uint64_t S, GenoSiteRec* d_out) {
  hipLaunchKernelGGL(k_geno_finish_sites, dim3(grid_for(S, 256)), dim3(256), 0, st, d_site_part,
                     n_blocks, S, d_out);
  return hipGetLastError() == hipSuccess;
}

}  // namespace nghmm
