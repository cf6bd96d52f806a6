// kernels_count.hpp -- the distribution of the number of long IBD tracts (kernels_count.hip): host
// interface.  include/nghmm.h (nghmm_ibd_count) has the definition of a record.  The backward walk,
// the planes, the table of window ends and the parts are kernels_longest.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_longest.hpp"

namespace nghmm {

constexpr uint32_t kCountMaxM = 16;   // the largest n_counts

// The state of one forward lane, (individual, segment, threshold), with CAP >= n_counts levels:
// all of it, so that a chain twin can hand it across a cut as LongestCarry is handed.  R[0] stays 0.
template <int CAP>
struct CountLane {
  double pi0, pi1, Q;
  double N[CAP], V[CAP], R[CAP], top;
  uint32_t ap, cnt, hd;   // the oldest unresolved start (a GLOBAL site), the ring's live entries, its head
};

// the rings of one handle: segment g, threshold k owns cap[g * K + k] entries from entry
// off[g * K + k]; an entry is the M + 1 doubles (Q_a, tau_{a,0}, .., tau_{a,M-1}); double j of entry e
// of individual i lies at ring[(e * (M + 1) + j) * I + i], so a wave moves one level of one entry as
// one row of 512 contiguous bytes
struct CountRings {
  double* ring;
  const uint64_t* off;
  const uint32_t* cap;
};
inline uint64_t count_ring_bytes(uint64_t entries, uint64_t I, uint32_t M) {
  return entries * (M + 1) * I * sizeof(double);
}

// The forward walk, one lane per (individual, segment, threshold) left to right over the planes of
// longest_fast_bwd / launch_longest_bwd_exact: pi, and per part (N_c, V_c, R_c, Top, ring).  d_seg,
// d_btab [K][S] window ends, d_part [n_part] sorted, d_piseg as longest_fwd's (one handle: base 0).
// d_prob [I][n_part][K][M + 1].  exact: W through det_exp.  *d_overflow is raised if a ring is ever
// full at a push (the host's sizing would be wrong): the records are then not to be used.
bool count_fwd(hipStream_t st, bool exact, const uint64_t* d_seg, uint64_t n_seg, uint64_t S, uint64_t I,
               uint32_t K, uint32_t M, const uint32_t* d_btab, const LongestPart* d_part, uint64_t n_part,
               const LongestPlanes& pl, const double* d_piseg, const CountRings& rings, double* d_prob,
               int* d_overflow);

}  // namespace nghmm
