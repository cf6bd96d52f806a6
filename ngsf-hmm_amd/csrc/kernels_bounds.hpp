// kernels_bounds.hpp -- credible bounds of the two ends of an IBD tract (kernels_bounds.hip): host
// interface.  include/nghmm.h (nghmm_tract_bounds) has the definition.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_fast.hpp"
#include "kernels_support.hpp"   // support_pieces, and the boundary vectors a call starts from

namespace nghmm {

constexpr uint32_t BOUNDS_MAX_LEVELS = 8;
constexpr uint64_t BOUNDS_NONE = ~0ull;

// a chromosome start in the site distances (fast_dev.hpp stores it as kDStart = 1e22)
inline bool bounds_chrom_start(double d) { return !(d < 1e22); }

// A range of one handle, in handle-local sites; ordered and disjoint within an individual, as
// SupportRange.  The anchor pass walks the cores; the other two walk the STRETCHES between two
// limits lo < hi: the sites lo + 1 .. hi, whose factors g_t the two searches share, and, where lo
// is a chromosome start and no anchor, lo itself, which has no factor (nofact).
struct BoundRange {
  uint64_t first, last;   // closed
  uint64_t piece0;        // slot of the range's first piece (one per lane-chunk; exact mode: one)
  uint32_t nofact;        // 1: `first` is the stretch's lo: no factor and no check there
  uint32_t search;        // bit 0: the search to the right of the anchor lo (H); bit 1: to the left of the anchor hi (G)
};
static_assert(sizeof(BoundRange) == 32, "BoundRange");

// anchor pass, per piece: the smallest P(z = 0 | y), its lowest site, and P(z = 1 | y) there
struct BoundAnchor {
  double p0, p1;
  uint64_t site;
  uint64_t pad;
};
static_assert(sizeof(BoundAnchor) == 32, "BoundAnchor");

// sum pass, per piece: ln prod g over its sites (-inf with a factor 0); the same over the sites in
// front of its lowest factor 0 (all of them without one); ln P(z = 1 | y) at the range's first site
// (the piece that holds it)
struct BoundSum {
  double total, leftrun, lp1_first;
  uint64_t has_zero;
};
static_assert(sizeof(BoundSum) == 32, "BoundSum");

// locate pass, per piece, in: off_g = ln prod g over the stretch's sites behind the piece minus
// ln P(z_hi = 1 | y); off_h = ln prod g from the stretch's first factor through the piece's leftrun
struct BoundOff {
  double off_g, off_h;
};
// ... out, per level: the highest site of the piece at which G fails, the lowest at which H fails
// (handle-local; BOUNDS_NONE: none)
struct BoundFail {
  uint64_t g[BOUNDS_MAX_LEVELS], h[BOUNDS_MAX_LEVELS];
};

struct BoundLevels {
  double ln[BOUNDS_MAX_LEVELS];   // logarithms of the levels, descending
  uint32_t n;
};

// fast mode; fs.bound holds both halves of the boundary vectors (sample_fast_forward,
// support_fast_bounds).  d_ioff [I + 1], d_rec [ranges]; anchor and sum: one output per piece.
bool bounds_fast_anchor(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                        const uint64_t* d_ioff, const BoundRange* d_rec, BoundAnchor* d_piece);
bool bounds_fast_sum(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                     const uint64_t* d_ioff, const BoundRange* d_rec, BoundSum* d_piece);
// (locate: d_fail [pieces] is scratch; d_out [n], one record per range: of its pieces' failing
// sites the highest for G and the lowest for H)
bool bounds_fast_locate(FastState& fs, hipStream_t st, const double* d_indF, const double* d_alpha,
                        const uint64_t* d_ioff, const BoundRange* d_rec, const BoundOff* d_off,
                        const BoundLevels& lv, BoundFail* d_fail, uint64_t n, BoundFail* d_out);

// exact mode: one lane per individual in log space, the forward array filled as
// launch_support_exact fills it (fw [S + 1][I][2]); a range is one piece.  pass 0: anchors
// (d_out = BoundAnchor), 1: sums (BoundSum), 2: locate (d_off in, BoundFail out).
void launch_bounds_exact(int pass, hipStream_t st, const double* eprob, const double* pos, double* fw,
                         uint64_t S, uint64_t I, const double* d_indF, const double* d_alpha,
                         const uint64_t* d_ioff, const BoundRange* d_rec, const BoundOff* d_off,
                         const BoundLevels& lv, void* d_out, int* d_flags);

}  // namespace nghmm
