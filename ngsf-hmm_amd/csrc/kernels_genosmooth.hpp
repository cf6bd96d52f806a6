// kernels_genosmooth.hpp -- genotype posteriors under the HMM (kernels_genosmooth.hip): host
// interface.  include/nghmm.h (nghmm_geno_smooth) has the definition of every output.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "glview.hpp"
#include "kernels_summary.hpp"

namespace nghmm {

// laid out as nghmm_geno_site_stat and nghmm_geno_region_stat (include/nghmm.h)
struct GenoSiteRec {
  double n0, n1, n2, het_prior, ibd, alt_ibd;
};
static_assert(sizeof(GenoSiteRec) == 48, "nghmm_geno_site_stat is 48 bytes");
struct GenoRegionRec {
  double het, het_prior, non_ibd, dosage;
};
static_assert(sizeof(GenoRegionRec) == 32, "nghmm_geno_region_stat is 32 bytes");

// The cell pass: the weights d_cav [S][I][2] (kernels_freqinfo.hpp) and the likelihoods gl,
// site-major [S][I] cells (log_gl: their logarithms), at the frequencies d_freq [S].  Every output
// may be null and is then not written; what is written does not depend on which are.
//   d_post [S][I][3], d_call [S][I]
//   d_site_part [ceil(I / 64)][S]: per site the butterfly sum of every block of 64 individuals
//   d_piece_out [n_pieces][I]: the sums of every piece (kernels_summary.hpp: a region cut at the
//   multiples of kSummarySeg; `first` is not read), pieces and seg_piece as launch_summary_pass
//   takes them; null when there are no pieces
bool genosmooth_cells(hipStream_t st, const double* d_cav, const GlView& gl, bool log_gl,
                      const double* d_freq, uint64_t S, uint64_t I, const SummaryPiece* d_pieces,
                      const uint32_t* d_seg_piece, double* d_post, uint8_t* d_call,
                      GenoSiteRec* d_site_part, GenoRegionRec* d_piece_out);
// out[i][r] (r < n_regions) = the pieces piece_first[r] .. piece_first[r + 1] - 1 added in that
// order, the first one's value first
bool genosmooth_finish_regions(hipStream_t st, const GenoRegionRec* d_piece_out,
                               const uint32_t* d_piece_first, uint64_t n_regions, uint64_t I,
                               GenoRegionRec* d_out);
// out[s] = site_part[0][s] + site_part[1][s] + ... in block order (n_blocks >= 2)
bool genosmooth_finish_sites(hipStream_t st, const GenoSiteRec* d_site_part, uint64_t n_blocks,
                             uint64_t S, GenoSiteRec* d_out);

}  // namespace nghmm
