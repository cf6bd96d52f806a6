// kernels_sample.hpp -- sampling IBD paths from the joint posterior (kernels_sample.hip): host
// interface.  include/nghmm.h (nghmm_sample_paths) has the definition of a draw.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_fast.hpp"

namespace nghmm {

// draws that share one walk over the emissions (their per-draw state lives in registers)
constexpr uint32_t kSampleBatch = 8;

// What a contiguous range of sites of one sampled path contributes to nghmm_path_stats, in a form
// that two adjacent ranges merge: the run of 1 at its first site (head), the one at its last
// (tail; the same run when the range is `full`: all sites 1, no chromosome start after the
// first), the maximal runs that touch neither end (inner), the sum of the distances inside runs.
struct SampleSeg {
  uint64_t len, ones, head, tail, inner_n, inner_longest;
  double mb;
  uint64_t full;
};
static_assert(sizeof(SampleSeg) == 64, "SampleSeg");

// A followed by B; b_starts_chrom: B's first site starts a chromosome; d_first_b: its distance
__host__ __device__ inline SampleSeg seg_merge(const SampleSeg& A, const SampleSeg& B,
                                               bool b_starts_chrom, double d_first_b) {
  const bool joined = A.tail > 0 && B.head > 0 && !b_starts_chrom;
  SampleSeg o;
  o.len = A.len + B.len;
  o.ones = A.ones + B.ones;
  o.mb = joined ? (A.mb + d_first_b) + B.mb : A.mb + B.mb;
  o.inner_n = A.inner_n + B.inner_n;
  o.inner_longest = A.inner_longest > B.inner_longest ? A.inner_longest : B.inner_longest;
  o.full = (A.full && B.full && joined) ? 1 : 0;
  o.head = (A.full && joined) ? A.head + B.head : A.head;
  o.tail = (B.full && joined) ? A.tail + B.tail : B.tail;
  // the runs that end up touching neither end of the merged range
  uint64_t mid[2] = {0, 0};
  if (joined) {
    if (!A.full && !B.full) mid[0] = A.tail + B.head;
  } else {
    if (!A.full) mid[0] = A.tail;
    if (!B.full) mid[1] = B.head;
  }
  for (int k = 0; k < 2; ++k)
    if (mid[k]) {
      ++o.inner_n;
      if (mid[k] > o.inner_longest) o.inner_longest = mid[k];
    }
  return o;
}

// fast mode, forward half of a call on one handle: lane-chunk operators and checkpoints at the
// current parameters (kernels_fast_estep.hip), then the vector entering every lane-chunk from
// the left into fs.bound.  d_vin [I][2] = the forward vector entering the handle's first site
// (null: the initial distribution (1 - F, F)); d_vout [I][2] receives the one leaving its last.
bool sample_fast_forward(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                         const double* d_vin, double* d_vout);

struct SampleScratch {
  uint8_t* maps;        // [kSampleBatch][I][J]: lane-chunk maps, then the state entering each from the right
  void* chunk;          // [kSampleBatch][I][J] x 32 B: lane-chunk statistics
  SampleSeg* seg;       // [kSampleBatch][I]
  uint8_t* state_in;    // [kSampleBatch][I]: state at the site after the handle's last (shards)
  uint8_t* state_out;   // [kSampleBatch][I]: state at the handle's first site
  uint8_t* paths;       // [n_paths][I][pitch]
  uint64_t pitch;
};
// J lane-chunks per individual (0: exact mode), path rows of `pitch` bytes for n_paths draws
uint64_t sample_scratch_bytes(uint64_t I, uint64_t J, uint64_t pitch, uint32_t n_paths);
SampleScratch sample_scratch_carve(uint8_t* base, uint64_t I, uint64_t J, uint64_t pitch);

// fast mode, backward half for the draws [draw0, draw0 + nd), nd <= kSampleBatch: maps, scan,
// apply.  site0 = global index of the handle's first site; last = nothing follows the handle's
// last site (else d_after = the distance of the site that follows and scr.state_in its states);
// the first n_paths draws of the batch leave their sites in scr.paths.
bool sample_fast_backward(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                          uint64_t seed, uint32_t draw0, uint32_t nd, uint64_t site0, bool last,
                          double d_after, uint32_t n_paths, const SampleScratch& scr);

// exact mode: one lane per (individual, draw) over the stored log-space forward array
// fw [S + 1][I][2] (launch_forward_exact)
void launch_sample_exact(hipStream_t st, const double* fw, const double* pos, uint64_t S, uint64_t I,
                         const double* d_indF, const double* d_alpha, uint64_t seed, uint32_t draw0,
                         uint32_t nd, uint32_t n_paths, const SampleScratch& scr);

}  // namespace nghmm
