// kernels_summary.hpp -- launch interface of the region and site summaries (kernels_summary.hip):
// the decoded path and the posteriors reduced along the sites per (individual, region) and along
// the individuals per site, in one pass over both arrays.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace nghmm {

enum { SUMMARY_VITERBI = 1, SUMMARY_POSTERIOR = 2 };   // = NGHMM_SUMMARY_* (a bit mask)

// One record per (individual, region) and one per site, laid out as nghmm_region_stat and
// nghmm_site_stat (include/nghmm.h).
struct RegionRec {
  uint64_t vit_sites, post_sites;
  double post_sum, vit_mb;
};
static_assert(sizeof(RegionRec) == 32, "nghmm_region_stat is 32 bytes");
struct SiteRec {
  uint32_t vit_count, post_count;
  double post_sum;
};
static_assert(sizeof(SiteRec) == 16, "nghmm_site_stat is 16 bytes");

// sites per lane of the pass (a multiple of 16: the blocked path's 16-site blocks never straddle
// two segments); ngsf-hmm_amd/hmm.py states the same number as SUMMARY_SEGMENT_SITES
constexpr uint64_t kSummarySeg = 2048;
inline uint64_t summary_segments(uint64_t S) { return (S + kSummarySeg - 1) / kSummarySeg; }

// A piece = the sites [lo, hi) that one region shares with one segment (never empty, never across
// a segment edge); the pieces are ordered by site.  first != 0: lo is the region's first site (the
// site before it never contributes to vit_mb); 0: the region goes on from the piece -- or, at the
// first site of a site shard, from the shard -- before.
struct SummaryPiece {
  uint64_t lo, hi;
  uint32_t region, first;
};
static_assert(sizeof(SummaryPiece) == 24, "three words");

// The pass.  what: SUMMARY_* mask; path16 (VITERBI) blocked [S/16][I][16]; marg (POSTERIOR)
// [S][I]; pos [S]; prev_state (may be NULL = all 0) [I]: the decoded state at the site in front
// of site 0.  seg_piece [summary_segments(S) + 1]: the first piece of every segment;
// piece_out [n_pieces][I] (may be NULL when there are no pieces); site_part (NULL: no site
// records) [ceil(I / 64)][S]: per site the partial record of every block of 64 individuals.
void launch_summary_pass(hipStream_t st, int what, const uint8_t* path16, const double* marg,
                         const double* pos, const uint8_t* prev_state, double thr, uint64_t S,
                         uint64_t I, const SummaryPiece* pieces, const uint32_t* seg_piece,
                         RegionRec* piece_out, SiteRec* site_part);
// out[i][r] (r < n_regions) = the pieces piece_first[r] .. piece_first[r + 1] - 1 of piece_out
// added in that order
void launch_summary_finish_regions(hipStream_t st, const RegionRec* piece_out,
                                   const uint32_t* piece_first, uint64_t n_regions, uint64_t I,
                                   RegionRec* out);
// out[s] = site_part[0][s] + site_part[1][s] + ... in block order (n_blocks >= 2)
void launch_summary_finish_sites(hipStream_t st, const SiteRec* site_part, uint64_t n_blocks,
                                 uint64_t S, SiteRec* out);
// out[i] = the decoded state of individual i at the handle's last site
void launch_summary_last_state(hipStream_t st, const uint8_t* path16, uint64_t S, uint64_t I,
                               uint8_t* out);

}  // namespace nghmm
