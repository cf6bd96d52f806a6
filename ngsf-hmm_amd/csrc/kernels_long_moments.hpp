// kernels_long_moments.hpp -- mean and covariance of (total length, number) of the long IBD tracts
// (kernels_long_moments.hip): host interface.  include/nghmm.h (nghmm_ibd_long_moments) has the
// definition of a record.  The backward walk, the planes, the table of window ends and the parts
// are kernels_longest.hpp's; the rings are kernels_count.hpp's with kLongMomentEntry doubles an entry.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_count.hpp"
#include "kernels_longest.hpp"

namespace nghmm {

// laid out as nghmm_long_moment_stat (include/nghmm.h)
struct LongMomentRec {
  double mean_a, mean_t, var_a, cov_at, var_t;
};
static_assert(sizeof(LongMomentRec) == 40, "nghmm_long_moment_stat is 40 bytes");

// a ring entry: (Q_a, oA_a, oC_a, tau_a[6]); double j of entry e of individual i lies at
// ring[(e * kLongMomentEntry + j) * I + i] -- CountRings' row layout with 9 in place of M + 1
constexpr uint32_t kLongMomentEntry = 9;
inline uint64_t long_moment_ring_bytes(uint64_t entries, uint64_t I) {
  return entries * kLongMomentEntry * I * sizeof(double);
}

// The forward walk, one lane per (individual, segment, threshold) left to right over the planes of
// longest_fast_bwd / launch_longest_bwd_exact: pi, and per part the three moment vectors N, V, R,
// the offset pair and the ring.  d_seg, d_btab [K][S] window ends, d_part [n_part] sorted, d_piseg
// as count_fwd's (one handle: base 0).  d_cum [S]: cum_s in Mb, or the site index as a double;
// len(a, s) = (d_cum[s] - d_cum[a]) + len_add (1 in sites, 0 in Mb).  d_step [S]: delta_s, 1 in
// sites and d_s in Mb (0 at a chromosome start).  d_rec [I][n_part][K].  exact: W through det_exp.
// *d_overflow is raised if a ring is ever full at a push: the records are then not to be used.
bool long_moments_fwd(hipStream_t st, bool exact, const uint64_t* d_seg, uint64_t n_seg, uint64_t S, uint64_t I,
                      uint32_t K, const uint32_t* d_btab, const LongestPart* d_part, uint64_t n_part,
                      const LongestPlanes& pl, const double* d_piseg, const CountRings& rings, const double* d_cum,
                      const double* d_step, double len_add, LongMomentRec* d_rec, int* d_overflow);

}  // namespace nghmm
