// kernels_support.hpp -- joint posterior of whole runs of sites (kernels_support.hip): host
// interface.  include/nghmm.h (nghmm_tract_support) has the definition of a score.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_fast.hpp"

namespace nghmm {

// A range of one handle, in handle-local sites.  The records of an individual are contiguous and
// ordered by first site (ioff[i] .. ioff[i + 1]); ranges of one individual do not overlap.
struct SupportRange {
  uint64_t first, last;   // closed
  uint64_t piece0;        // fast mode: slot of the range's first piece (one piece per lane-chunk it touches)
  uint64_t cont;          // 1: the range goes on from the site shard before (its first site is no range start)
};
static_assert(sizeof(SupportRange) == 32, "SupportRange");

// What a piece of a range contributes, and what a range ends up with: laid out as
// nghmm_tract_score (include/nghmm.h)
struct SupportScore {
  double log_ibd, log_non, post_min;
  uint64_t post_min_site;
};
static_assert(sizeof(SupportScore) == 32, "nghmm_tract_score is 32 bytes");

// pieces of a range [first, last] in a layout of T sites per lane (one per lane-chunk it touches)
__host__ __device__ inline uint64_t support_pieces(uint64_t first, uint64_t last, uint64_t T) {
  return last / T - first / T + 1;
}

// fast mode, backward half of the boundary vectors (the forward half is sample_fast_forward's):
// fs.bound[..][2..3] = the backward vector entering every lane-chunk from the right.  d_win [I][2]
// = the backward vector at the handle's last site (null: (1, 1)); d_wout [I][2] (may be null)
// receives the one at the last site of the shard before.
bool support_fast_bounds(FastState& fs, hipStream_t st, const double* d_win, double* d_wout);

// fast mode: the walk over the lane-chunks that hold a range, then every range's pieces added in
// site order.  d_ioff [I + 1], d_rec [n], d_piece [pieces], d_out [n]
bool support_fast_walk(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                       const uint64_t* d_ioff, const SupportRange* d_rec, uint64_t n,
                       SupportScore* d_piece, SupportScore* d_out);

// exact mode: one lane per individual over the log emissions eprob [S][I][2]: a log-space forward
// array normalised at every site, written into fw [S + 1][I][2] (the handle's forward array, which
// every user recomputes before reading), then the backward recursion on the fly.  A NaN in the
// forward values raises d_flags[FLAG_INVALID_LKL], as launch_forward_exact does.
void launch_support_exact(hipStream_t st, const double* eprob, const double* pos, double* fw,
                          uint64_t S, uint64_t I, const double* d_indF, const double* d_alpha,
                          const uint64_t* d_ioff, const SupportRange* d_rec, SupportScore* d_out,
                          int* d_flags);

}  // namespace nghmm
