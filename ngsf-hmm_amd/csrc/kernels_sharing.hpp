// kernels_sharing.hpp -- launch interface of the pairwise IBD sharing (kernels_sharing.hip): the
// [I][I] matrices  sum over sites of x[i][s] * x[j][s]  of the posteriors (FP64 matrix cores), of
// the decoded path and of the thresholded posteriors (int8 matrix cores on 0/1 bytes).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace nghmm {

enum { SHARING_VITERBI = 1, SHARING_POSTERIOR = 2 };   // = NGHMM_SHARING_* (a bit mask)

// The site range of a call is cut into K-splits, each added up by one wave per block of 64 x 64
// pairs; the splits' partial matrices are added in site order afterwards.  The cut is a function
// of (I, site_begin, site_end) alone, which fixes the order every double is added in.
//   kSharingSplit          the least sites per split (a multiple of 64: the int8 instruction's K);
//                          ngsf-hmm_amd/hmm.py states the same number as SHARING_SPLIT_SITES
//   kSharingMaxSplits      the cap on the number of splits
//   kSharingScratchBytes   ... and on the partial matrices, I * I * 8 bytes each (at least one)
constexpr uint64_t kSharingSplit = 1024;
constexpr uint64_t kSharingMaxSplits = 1024;
constexpr uint64_t kSharingScratchBytes = 256ull << 20;

// Split k holds the sites [max(begin, first + k * len), min(end, first + (k + 1) * len)); first
// and len are multiples of 64, so no block of 16 path bytes and no int8 step lies across an edge.
struct SharingPlan {
  uint64_t first, len, n;
};
inline SharingPlan sharing_plan(uint64_t I, uint64_t begin, uint64_t end) {
  SharingPlan p;
  p.first = begin / 64 * 64;
  const uint64_t span = end - p.first;
  uint64_t cap = kSharingScratchBytes / (I * I * 8);
  cap = cap < 1 ? 1 : (cap > kSharingMaxSplits ? kSharingMaxSplits : cap);
  uint64_t n = (span + kSharingSplit - 1) / kSharingSplit;
  if (n > cap) n = cap;
  p.len = ((span + n - 1) / n + 63) / 64 * 64;
  p.n = (span + p.len - 1) / p.len;
  return p;
}

// part[k][i][j] (doubles; written for j's block of 64 >= i's block only) = sum over split k's
// sites of marg[s][i] * marg[s][j], marg [S][I]: v_mfma_f64_16x16x4_f64, four sites a step in
// ascending order
void launch_sharing_prod(hipStream_t st, const double* marg, uint64_t I, uint64_t begin,
                         uint64_t end, SharingPlan plan, double* part);
// part[k][i][j] (int32; same blocks) = the sites of split k at which bytes of i and of j are both
// 1.  bytes16: 0/1 bytes blocked [..][I][16], its first block the sites 16 * block0 ..:
// v_mfma_i32_16x16x64_i8, 64 sites a step
void launch_sharing_count(hipStream_t st, const uint8_t* bytes16, uint64_t block0, uint64_t I,
                          uint64_t begin, uint64_t end, SharingPlan plan, int32_t* part);
// out16[b - block0][i][u] = marg[16 b + u][i] >= thr (0 for sites outside [begin, end)), for the
// blocks b = begin / 16 .. (end - 1) / 16
void launch_sharing_threshold(hipStream_t st, const double* marg, uint64_t I, uint64_t begin,
                              uint64_t end, double thr, uint8_t* out16);
// out[i][j] = out[j][i] = part[0][a][b] + part[1][a][b] + ... in split order, a = min(i, j),
// b = max(i, j)
void launch_sharing_finish_prod(hipStream_t st, const double* part, uint64_t n_splits, uint64_t I,
                                double* out);
void launch_sharing_finish_count(hipStream_t st, const int32_t* part, uint64_t n_splits,
                                 uint64_t I, uint64_t* out);

}  // namespace nghmm
